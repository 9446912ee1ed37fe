// Device-side helpers shared by several kernels.
#pragma once
#include "oiva_internal.h"

#include <type_traits>
#include <utility>

namespace oiva {

constexpr float kEpsR = 1e-15f;  // reference overiva.py:170

// block-wide sum of one double per thread, fixed order (wave shuffle tree, then the waves in order);
// every thread of the block must call it; scratch holds kWaves doubles
__device__ __forceinline__ double block_sum(double v, double* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[wave] = v;
    __syncthreads();
    double s = 0.;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += scratch[w];
    return s;
}

// gamma_k = mean_t R[t,k]  (reference overiva.py:158) from the per-block partial sums the activation kernel left
// behind R (rsum_offset_floats): a fixed-order sum of T/256 float64 values at wave-uniform addresses (scalar
// loads), so every lane of every kernel obtains the same bits for the price of a few instructions.
__device__ __forceinline__ double gamma_of(const float* __restrict__ R, int T, int K, int k) {
    const double* S = reinterpret_cast<const double*>(R + rsum_offset_floats(T, K));
    const int nblk = rsum_blocks(T);
    double s = 0.;
    for (int b = 0; b < nblk; ++b) s += S[(size_t)b * K + k];
    return s / (double)T;
}

// 1 / max(r / gamma, eps)   (reference overiva.py:159, :170-173) with ginv = 1 / gamma
__device__ __forceinline__ float activation_weight(float r, float ginv) {
    float rn = r * ginv;
    rn = rn < kEpsR ? kEpsR : rn;   // a NaN stays NaN, like r[r < eps] = eps in the reference
    return 1.f / rn;
}

// one M-vector (M complex64 = M*8 bytes, 16-byte aligned for even M) into split re/im registers
template <int M>
__device__ __forceinline__ void load_x(const float2* __restrict__ p, float (&xr)[M], float (&xi)[M]) {
    if constexpr (M % 2 == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int i = 0; i < M / 2; ++i) {
            const float4 v = p4[i];
            xr[2 * i] = v.x;
            xi[2 * i] = v.y;
            xr[2 * i + 1] = v.z;
            xi[2 * i + 1] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float2 v = p[i];
            xr[i] = v.x;
            xi[i] = v.y;
        }
    }
}

// ---- the non-temporal form of a wave's load step (4 frames x 16 bins of M = 4 or 8 channels), HBM -> LDS ----
// nt loads bypass the L1, which is what merges the M/2 requests a lane makes for its own M-vector: a lane-strided nt step moves
// every line M/2 times across the L2 (3.6 TB/s against 6.0 plain, profiles/mallbench.log).  So the nt step is ROW-CONTIGUOUS: the
// 16 bins of one frame are one run of 128 M bytes, instruction j of the step takes 1 KB of the step's runs, lane l its bytes
// [16 l, 16 l + 16), and the step lands in LDS frame by frame, bin by bin -- float4 index (frame * 16 + bin) * M/2 + piece.
// Lane (bin b, frame phase q) then reads the same M-vector it loads itself in the plain form.
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;
template <int M>
struct XRows {
    static_assert(M == 4 || M == 8, "whole 1-KB instructions of 16-byte pieces");
    static constexpr int kPieces = M / 2;               // 16-byte pieces of one M-vector
    static constexpr int kLanesPerRow = 16 * kPieces;   // lanes that take one frame's run
    static constexpr int kFramesPerInstr = 64 / kLanesPerRow;
    // what this lane requests: frame (of the step's four) in instruction j, and its float2 offset inside a frame of F bins
    static __device__ __forceinline__ int frame(int lane, int j) { return j * kFramesPerInstr + lane / kLanesPerRow; }
    static __device__ __forceinline__ int offset(int lane, int f0, int F) {
        const int r = lane % kLanesPerRow, f = f0 + r / kPieces;
        return (f < F ? f : F - 1) * M + (r % kPieces) * 2;      // bins past the end: the last bin (legal, never stored)
    }
    // float4 index of lane (b, q)'s first piece in the landed step
    static __device__ __forceinline__ int slot(int b, int q) { return (q * 16 + b) * kPieces; }
    // request the step whose frames are t0 .. t0 + 3 into `stage` (wave-uniform); frames >= t_lim re-request frame T - 1.
    // AUX: the cache policy bits of the instruction (0 plain, 2 nt)
    template <int AUX>
    static __device__ __forceinline__ void issue(const float2* __restrict__ X, size_t frame_stride, int off, int lane, int t0, int t_lim, int T,
                                                 float4* stage) {
#pragma unroll
        for (int j = 0; j < kPieces; ++j) {
            const int t = t0 + frame(lane, j);
            const float2* src = X + (size_t)(t < t_lim ? t : T - 1) * frame_stride + off;
            __builtin_amdgcn_global_load_lds((gvoid_t*)src, (lvoid_t*)(stage + j * 64), 16, 0, AUX);
        }
    }
    static __device__ __forceinline__ void issue_nt(const float2* __restrict__ X, size_t frame_stride, int off, int lane, int t0, int t_lim,
                                                    int T, float4* stage) {
        issue<2>(X, frame_stride, off, lane, t0, t_lim, T, stage);
    }
};

// ---- a lane's read of its own M-vector from a stage of a per-wave LDS-DMA ring (cov_dma_kernel, the streamed power_kernel) ----
// The counted wait and the LDS reads sit in one asm block: hipcc counts LDS-DMA like any load and drains the whole queue
// (vmcnt(0)) in front of any LDS access it can see.  INFLIGHT = the requests that may stay outstanding: those of the steps issued
// behind the one that is read (every step issues PIECES of them).
// ring_read: a stage that landed lane by lane (piece j of the lane's vector at stage + j * 1024 + lane * 16);
// ring_read_rows: one that landed row by row (XRows): the lane's pieces lie side by side.
template <int PIECES, int INFLIGHT>
__device__ __forceinline__ void ring_read(unsigned addr, float4 (&v)[PIECES]) {
    static_assert(PIECES == 2 || PIECES == 4, "M in {4, 8}");
    if constexpr (PIECES == 4)
        asm volatile(
            "s_waitcnt vmcnt(%5)\n\t"
            "ds_read_b128 %0, %4\n\t"
            "ds_read_b128 %1, %4 offset:1024\n\t"
            "ds_read_b128 %2, %4 offset:2048\n\t"
            "ds_read_b128 %3, %4 offset:3072\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
            : "v"(addr), "n"(INFLIGHT)
            : "memory");
    else
        asm volatile(
            "s_waitcnt vmcnt(%3)\n\t"
            "ds_read_b128 %0, %2\n\t"
            "ds_read_b128 %1, %2 offset:1024\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1])
            : "v"(addr), "n"(INFLIGHT)
            : "memory");
}
template <int PIECES, int INFLIGHT>
__device__ __forceinline__ void ring_read_rows(unsigned addr, float4 (&v)[PIECES]) {
    static_assert(PIECES == 2 || PIECES == 4, "M in {4, 8}");
    if constexpr (PIECES == 4)
        asm volatile(
            "s_waitcnt vmcnt(%5)\n\t"
            "ds_read_b128 %0, %4\n\t"
            "ds_read_b128 %1, %4 offset:16\n\t"
            "ds_read_b128 %2, %4 offset:32\n\t"
            "ds_read_b128 %3, %4 offset:48\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
            : "v"(addr), "n"(INFLIGHT)
            : "memory");
    else
        asm volatile(
            "s_waitcnt vmcnt(%3)\n\t"
            "ds_read_b128 %0, %2\n\t"
            "ds_read_b128 %1, %2 offset:16\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1])
            : "v"(addr), "n"(INFLIGHT)
            : "memory");
}

// ---- fp32 / fp64 matrix-core tile of shape 16x16x4 (A, B: one value per lane; C/D: 4 values per lane) ----
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

template <typename REAL>
struct Mfma;
template <>
struct Mfma<float> {
    using acc_t = f32x4;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);     // exact fp32 fmaf chain over the 4 k
    }
    // C/D layout: lane l, register r -> row; the column is l & 15
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};
template <>
struct Mfma<double> {
    using acc_t = f64x4;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }   // NOT the fp32 map
};

// ---- register-level lane exchanges (no LDS crossbar): DPP within 16-lane rows, v_permlane{16,32}_swap
//      across rows.  Values wider than 32 bits go through them one dword at a time. ----
template <int CTRL>
__device__ __forceinline__ int dpp32(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) { return __int_as_float(dpp32<CTRL>(__float_as_int(v))); }
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned v) { return (unsigned)dpp32<CTRL>((int)v); }
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    return __hiloint2double(dpp32<CTRL>(__double2hiint(v)), dpp32<CTRL>(__double2loint(v)));
}
// same, writing only the banks (groups of 4 lanes of a 16-lane row) selected by BANKS; the other lanes keep `old`
template <int CTRL, int BANKS>
__device__ __forceinline__ int dpp32_banks(int old, int x) {
    return __builtin_amdgcn_update_dpp(old, x, CTRL, 0xF, BANKS, false);
}
template <int CTRL, int BANKS>
__device__ __forceinline__ float dpp_banks(float old, float v) {
    return __int_as_float(dpp32_banks<CTRL, BANKS>(__float_as_int(old), __float_as_int(v)));
}
template <int CTRL, int BANKS>
__device__ __forceinline__ double dpp_banks(double old, double v) {
    return __hiloint2double(dpp32_banks<CTRL, BANKS>(__double2hiint(old), __double2hiint(v)),
                            dpp32_banks<CTRL, BANKS>(__double2loint(old), __double2loint(v)));
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): loop indices that must be compile-time constants
// (DPP controls, lane numbers of v_readlane)
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}
constexpr int kDppXor1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;   // quad_perm [2,3,0,1]
constexpr int kDppRor4 = 0x124;  // row_ror:4
constexpr int kDppRor8 = 0x128;  // row_ror:8
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane l <-> 7 - l inside each group of 8
// a + b where b is the value of the lane 16 (32) lanes away: the swap of a register with itself
// leaves {own row pair member, other row pair member} in the two results
__device__ __forceinline__ float swapsum16(float v) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swapsum32(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ double swapsum16(double v) {
    auto h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(v), (unsigned)__double2hiint(v), false, false);
    auto l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(v), (unsigned)__double2loint(v), false, false);
    return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
__device__ __forceinline__ double swapsum32(double v) {
    auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(v), (unsigned)__double2hiint(v), false, false);
    auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(v), (unsigned)__double2loint(v), false, false);
    return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
__device__ __forceinline__ unsigned swapmax16(unsigned v) {
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return r[0] > r[1] ? r[0] : r[1];
}
__device__ __forceinline__ unsigned swapmax32(unsigned v) {
    auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return r[0] > r[1] ? r[0] : r[1];
}


}  // namespace oiva
