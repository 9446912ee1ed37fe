// Per-lane arithmetic of the demixing passes (reference overiva.py:140, :153/:155), shared by the streaming kernels
// (kernels_demix.hip) and the X-resident iteration kernel (kernels_resident.hip).
#pragma once
#include "oiva_device.h"

namespace oiva {

// conj(W[f][m][k0+kk]) for the lane's bin; W_hat is (F, M, M) row-major, column k = demixing vector k
template <int M, int KP>
__device__ __forceinline__ void load_wconj(const float2* __restrict__ What, int f, int k0, int K, float (&wr)[KP][M],
                                           float (&wi)[KP][M]) {
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float2 v = make_float2(0.f, 0.f);
            if (k0 + kk < K) v = What[((size_t)f * M + m) * M + k0 + kk];
            wr[kk][m] = v.x;
            wi[kk][m] = -v.y;
        }
    }
}

// The same in two steps for the head of power_kernel: load_w_raw requests the lane's W as it lies in memory, with nothing
// between the requests that depends on one of them (load_wconj's conjugation after every element makes hipcc wait for every
// element: M * KP / 2 dependent round trips), finish_wconj forms the values load_wconj returns once they have all been asked for.
// Even M and KP: columns k0 + 2p and k0 + 2p + 1 of a row are 16 adjacent, aligned bytes (k0 = blockIdx.z * KP is even, a row is
// M * 8 bytes); otherwise 8-byte loads.  A column >= K is not branched around: column 0 is read in its place and the value
// zeroed afterwards (for even M a pair that starts below K ends below M, inside the row).
template <int M, int KP>
struct WRaw {
    static constexpr bool kWide = M % 2 == 0 && KP % 2 == 0;
    float4 v4[kWide ? KP / 2 : 1][kWide ? M : 1];
    float2 v2[kWide ? 1 : KP][kWide ? 1 : M];
};
template <int M, int KP>
__device__ __forceinline__ void load_w_raw(const float2* __restrict__ What, int f, int k0, int K, WRaw<M, KP>& w) {
    const float2* row0 = What + (size_t)f * M * M;
    if constexpr (WRaw<M, KP>::kWide) {
#pragma unroll
        for (int p = 0; p < KP / 2; ++p) {
            const int c = k0 + 2 * p < K ? k0 + 2 * p : 0;
#pragma unroll
            for (int m = 0; m < M; ++m) w.v4[p][m] = *reinterpret_cast<const float4*>(row0 + m * M + c);
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) {
            const int c = k0 + kk < K ? k0 + kk : 0;
#pragma unroll
            for (int m = 0; m < M; ++m) w.v2[kk][m] = row0[m * M + c];
        }
    }
}
template <int M, int KP>
__device__ __forceinline__ void finish_wconj(const WRaw<M, KP>& w, int k0, int K, float (&wr)[KP][M], float (&wi)[KP][M]) {
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
        const bool on = k0 + kk < K;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float re, im;
            if constexpr (WRaw<M, KP>::kWide) {
                const float4 v = w.v4[kk / 2][m];
                re = kk % 2 ? v.z : v.x;
                im = kk % 2 ? v.w : v.y;
            } else {
                re = w.v2[kk][m].x;
                im = w.v2[kk][m].y;
            }
            wr[kk][m] = on ? re : 0.f;
            wi[kk][m] = -(on ? im : 0.f);
        }
    }
}

// y = sum_m conj(w_m) x_m
template <int M>
__device__ __forceinline__ void demix_one(const float (&wr)[M], const float (&wi)[M], const float (&xr)[M],
                                          const float (&xi)[M], float& yr, float& yi) {
    float ar = 0.f, ai = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        ar = fmaf(wr[m], xr[m], ar);
        ar = fmaf(-wi[m], xi[m], ar);
        ai = fmaf(wr[m], xi[m], ai);
        ai = fmaf(wi[m], xr[m], ai);
    }
    yr = ar;
    yi = ai;
}

// sum over the 16 lanes of a DPP row (= the 16 bins of one frame phase); every lane gets the total
__device__ __forceinline__ float row16_sum(float v) {
    int x;
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, false);
    v += __int_as_float(x);
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, false);
    v += __int_as_float(x);
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141 /* row_half_mirror */, 0xF, 0xF, false);
    v += __int_as_float(x);
    x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140 /* row_mirror */, 0xF, 0xF, false);
    v += __int_as_float(x);
    return v;
}

// Power pass of one workgroup of batch_power_kernel (kernels_batch.hip): power_kernel's lanes and sums (kernels_demix.hip), so a
// problem's partial powers are those of its single-problem plan.  (power_kernel keeps its own copy of this body: the code the
// compiler makes of the shared form differs from the single-problem kernel's, and that kernel is timed by the benchmarks.)
// 4 waves x 16 bins =
// the 64-bin batch `bx`, 4 frame phases per wave, frames [by * tcp, by * tcp + tcp), sources [k0, k0 + KP);
// Ppart[bx][t][k] = sum over the batch's bins of |w_{f,k}^H x_{t,f}|^2 (each wave's 16 bins by row16_sum, then the waves in
// order).  sp: kWaves * tcp * KP floats of LDS.
constexpr int kBatchPowUnroll = 2;

template <int M, int KP>
__device__ __forceinline__ void power_block(const float2* __restrict__ X, const float2* __restrict__ What,
                                            float* __restrict__ Ppart, int T, int F, int K, int tcp, unsigned bx, unsigned by, int k0,
                                            float* sp) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int b = lane & 15;
    const int q = lane >> 4;
    const int f = (bx * kWaves + wave) * kBinsPerWave + b;
    const bool fvalid = f < F;
    const int fc = fvalid ? f : F - 1;
    const int t_begin = by * tcp;
    const int t_end = min(T, t_begin + tcp);
    const int len = t_end - t_begin;
    const int nsteps = (len + 3) >> 2;

    float wr[KP][M], wi[KP][M];
    load_wconj<M, KP>(What, fc, k0, K, wr, wi);

    // kBatchPowUnroll steps are loaded before any of them is consumed: a wave keeps kBatchPowUnroll * 64 * M * 8
    // bytes in flight, which is what hides HBM latency here (more resident waves only thrash the L1,
    // because a lane's M*8 bytes arrive through M/2 separate dwordx4 requests to the same lines).
    const size_t frame_stride = (size_t)F * M;
    const float2* pbase = X + (size_t)fc * M;
    for (int i = 0; i < nsteps; i += kBatchPowUnroll) {
        float xr[kBatchPowUnroll][M], xi[kBatchPowUnroll][M];
#pragma unroll
        for (int u = 0; u < kBatchPowUnroll; ++u) {
            const int tl = 4 * (i + u) + q;
            const int t = tl < len ? t_begin + tl : T - 1;      // clamped: legal address, result unused
            load_x<M>(pbase + (size_t)t * frame_stride, xr[u], xi[u]);
        }
#pragma unroll
        for (int u = 0; u < kBatchPowUnroll; ++u) {
            const int tl = 4 * (i + u) + q;
            const bool live = tl < len;
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                float yr, yi;
                demix_one<M>(wr[kk], wi[kk], xr[u], xi[u], yr, yi);
                float pw = fmaf(yr, yr, yi * yi);
                pw = fvalid ? pw : 0.f;
                pw = row16_sum(pw);
                if (b == 0 && live) sp[(wave * tcp + tl) * KP + kk] = pw;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < len * KP; e += kBlock) {
        const int tl = e / KP, kk = e - tl * KP;
        float s = sp[(0 * tcp + tl) * KP + kk];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += sp[(w * tcp + tl) * KP + kk];
        if (k0 + kk < K) Ppart[((size_t)bx * T + t_begin + tl) * K + k0 + kk] = s;
    }
}

}  // namespace oiva
