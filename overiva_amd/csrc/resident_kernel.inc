// X-resident iteration kernel: the whole loop body of reference overiva.py:138-190 -- demix + source powers (:140,
// :153/:155), activation (:152-173), weighted covariance of all sources (:179), IP1 solve + normalisation (:181-186)
// and the orthogonal-constraint update of J (:189-190) -- for n iterations in ONE launch, with X read from HBM once
// per launch instead of twice per iteration.
//
// When it applies.  The (bins x frames x channels) tensor must fit the chip's registers + LDS: workgroup (g, c) of the
// NB x NS grid (one per CU, all resident) owns bin group g (16 bins) x frame split c (TW <= 256 frames) for the whole
// launch; lane (b, q) keeps the M-vectors of bin b at frames q + 16 j, j < J: the first JR = 8 of them in 8*M*2
// registers (the accumulator half of the unified register file: one wave per SIMD may use 512), the rest in LDS
// (128 KB of the 160).  That is BASELINE configs[1] (513 x 1000 x 4: 72 KB of LDS per CU) and one rank's shard of the
// headline shape at 8 GPUs (256 x 4000 x 8: exactly 16 bins x 250 frames = 250 KB per CU).
//
// Dependencies inside an iteration, and how they are met without kernel boundaries.  Every hand-off is between the
// 16-odd workgroups of one row (same bins) or one column (same frames) of the grid, never grid-wide:
//   power   : (g, c) demixes its tile and publishes sum_{16 bins} |y|^2 for its frames         -> column c
//   activate: (g, c) adds the NB parts of its frames in the fixed order of the four-launch path (64-bin batches),
//             r = 2 sqrt(p) | p / F, weights 1 / r into an LDS table, sum_t r of the split      (redundantly per row)
//   cov     : weighted covariance of its tile, 16 frame phases added in float64 through LDS,
//             partial per (split, bin, source) published                                          -> row g
//   update  : (g, c) owns bins c, c + NS, ... of the group (one lane group per bin on its waves): adds the NS partials
//             in float64, gamma = mean_t r from the splits' sums, the structured IP1 / J chain of update_chain.h,
//             W_hat^H stays in registers across iterations; publishes conj(w_k)                   -> row g
// gamma (overiva.py:158) is applied AFTER the covariance sums: V = gamma * sum_t (1/r_t) x x^H / T, which equals
// the reference's sum_t (gamma / r_t) x x^H / T.  The floor r / gamma >= 1e-15 (:170-171) needs gamma, which a workgroup
// learns only after its accumulation: frames below the floor are accumulated a second time with the weight difference
// (`finish` in the covariance phase), so the floor sits exactly where the reference puts it; inputs without silent frames
// pay one load, hidden behind the reduction.
// Hand-offs: the data is the flag.  Every published word is one naturally aligned 4- or 8-byte agent-scope atomic
// store that carries the epoch in mantissa bits nobody needs: the two low bits of a float32 pair (|y|^2 parts,
// demixing vectors: a 1.2e-7 relative perturbation of quantities that only feed the activations) and the 16 low bits
// of a float64 partial sum of float32 products (2^-36 relative).  A consumer re-reads its own words until every tag is
// the current epoch: no release fence, no drain of the producer's stores, no separate flag and no acquire -- one memory
// round trip per hop instead of four.  Parts are double-buffered by epoch parity (a column's workgroups can be one
// iteration apart); the other buffers are reused every iteration, which the dependency chain makes safe.  Every wait
// gives up after timeout_ticks and makes the whole launch return with a code in ctrl[0].  The final W_hat is written to a
// staging copy which the host moves into place only if ctrl[0] is still 0: a launch that gave up -- in whatever
// iteration -- changed nothing.
#pragma once
#include "cov_arith.h"
#include "demix_arith.h"
#include "resident.h"
#include "update_chain.h"

namespace oiva {
namespace {

using u64 = unsigned long long;
typedef __attribute__((address_space(1))) const void gvoid_res_t;
typedef __attribute__((address_space(3))) void lvoid_res_t;
constexpr float kTinyR = 1e-20f;
constexpr int kResChunk = 16;                 // accumulators combined per LDS round
constexpr int kResStride = kBlock + 1;        // +1: conflict-free transposed read
constexpr int kResRedFloats = kResChunk * kResStride;

__device__ __forceinline__ u64 ld64(const void* p) {
    return __hip_atomic_load(static_cast<u64*>(const_cast<void*>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st64(void* p, u64 v) {
    __hip_atomic_store(static_cast<u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// plain store: the line stays in the XCD's L2 (an agent-scope store writes through and DROPS it, so that even a reader on the
// same XCD fetches it from the fabric).  Only for hand-offs whose two ends were VERIFIED to share an XCD (row_local below).
__device__ __forceinline__ void st64_plain(void* p, u64 v) { *static_cast<u64*>(p) = v; }
__device__ __forceinline__ unsigned ld32(const void* p) {
    return __hip_atomic_load(static_cast<unsigned*>(const_cast<void*>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st32(void* p, unsigned v) {
    __hip_atomic_store(static_cast<unsigned*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// system scope: words in another GPU's memory (stores over xGMI) and words other GPUs store into ours
__device__ __forceinline__ u64 ld64_sys(const void* p) {
    return __hip_atomic_load(static_cast<u64*>(const_cast<void*>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st64_sys(void* p, u64 v) {
    __hip_atomic_store(static_cast<u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned ld32_sys(const void* p) {
    return __hip_atomic_load(static_cast<unsigned*>(const_cast<void*>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st32_sys(void* p, unsigned v) {
    __hip_atomic_store(static_cast<unsigned*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float2 ld_f2(const float2* p) {
    const u64 u = ld64(p);
    return make_float2(__uint_as_float((unsigned)u), __uint_as_float((unsigned)(u >> 32)));
}
__device__ __forceinline__ void st_f2(float2* p, float2 v) { st64(p, (u64)__float_as_uint(v.x) | ((u64)__float_as_uint(v.y) << 32)); }
__device__ __forceinline__ float ld_f1(const float* p) { return __uint_as_float(ld32(p)); }
__device__ __forceinline__ void st_f1(float* p, float v) { st32(p, __float_as_uint(v)); }
__device__ __forceinline__ double ld_f64(const double* p) { return __longlong_as_double((long long)ld64(p)); }
__device__ __forceinline__ void st_f64(double* p, double v) { st64(p, (u64)__double_as_longlong(v)); }

// ---- tagged words ----
__device__ __forceinline__ u64 pack_f2(float a, float b, unsigned tag) {      // tag: 2 bits, one in each float's lowest mantissa bit
    const unsigned x = (__float_as_uint(a) & ~1u) | (tag & 1u), y = (__float_as_uint(b) & ~1u) | ((tag >> 1) & 1u);
    return (u64)x | ((u64)y << 32);
}
__device__ __forceinline__ unsigned tag_f2(u64 u) { return ((unsigned)u & 1u) | (((unsigned)(u >> 32) & 1u) << 1); }
__device__ __forceinline__ float lo_f2(u64 u) { return __uint_as_float((unsigned)u & ~1u); }
__device__ __forceinline__ float hi_f2(u64 u) { return __uint_as_float((unsigned)(u >> 32) & ~1u); }
__device__ __forceinline__ unsigned pack_f1(float a, unsigned tag) { return (__float_as_uint(a) & ~3u) | (tag & 3u); }
__device__ __forceinline__ unsigned tag_f1(unsigned u) { return u & 3u; }
__device__ __forceinline__ float val_f1(unsigned u) { return __uint_as_float(u & ~3u); }
__device__ __forceinline__ u64 pack_f64(double v, unsigned tag) { return ((u64)__double_as_longlong(v) & ~(u64)0xFFFF) | (u64)(tag & 0xFFFFu); }
__device__ __forceinline__ unsigned tag_f64(u64 u) { return (unsigned)(u & 0xFFFF); }
__device__ __forceinline__ double val_f64(u64 u) { return __longlong_as_double((long long)(u & ~(u64)0xFFFF)); }

// a polling wave asks, every few passes, whether to give up: another workgroup already did, or `timeout` ticks of the
// 100 MHz clock have passed since t0 (then it records `code`)
__device__ __forceinline__ bool give_up(unsigned spins, long long t0, unsigned* ctrl, long long timeout, unsigned code) {
    if ((spins & 7u) != 0u) return false;
    if (ld32(ctrl) != 0u) return true;
    if (wall_clock64() - t0 > timeout) {
        atomicCAS(ctrl, 0u, code);
        return true;
    }
    return false;
}

// The frames a lane keeps in registers live in the ACCUMULATOR half of the unified register file: inline-asm "a" operands,
// which the register allocator cannot move, so that the 256 architectural registers stay free for the 128 covariance
// accumulators.  A frame is copied out (v_accvgpr_read) where it is used.  (Left to the compiler, a plain array of 128
// floats that is live for the whole kernel ends in scratch memory.)
template <int M, int JR>
struct AccFrames {
    static constexpr int PIECES = M / 2;
    float v[JR > 0 ? JR : 1][2 * M];
    template <int J>
    __device__ __forceinline__ void put(const float4 (&x)[PIECES]) {
#pragma unroll
        for (int p = 0; p < PIECES; ++p) {
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(v[J][4 * p + 0]) : "v"(x[p].x));
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(v[J][4 * p + 1]) : "v"(x[p].y));
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(v[J][4 * p + 2]) : "v"(x[p].z));
            asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(v[J][4 * p + 3]) : "v"(x[p].w));
        }
    }
    template <int J>
    __device__ __forceinline__ void get(float4 (&x)[PIECES]) const {
#pragma unroll
        for (int p = 0; p < PIECES; ++p) {
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x[p].x) : "a"(v[J][4 * p + 0]));
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x[p].y) : "a"(v[J][4 * p + 1]));
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x[p].z) : "a"(v[J][4 * p + 2]));
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x[p].w) : "a"(v[J][4 * p + 3]));
        }
    }
};

// R = arithmetic of the per-bin update (float | double); COV64: the covariance sums as float64 sums of exact float64 products
// (the `precise` arithmetic, OIVA_PREC_COV_F64: 4 channels only -- 32 float64 accumulators per lane)
template <int M, int K, int JR, typename R, bool COV64 = false>
__global__ __launch_bounds__(kBlock, 1) void resident_kernel(const ResidentArgs a) {
    static_assert(!COV64 || (M == 4 && sizeof(R) == 8), "float64 covariance: 4 channels, float64 per-bin algebra");
    static_assert(M == 2 || M == 4 || M == 6 || M == 8, "even channel counts (16-byte pieces of an M-vector)");
    static_assert(K == 1 || K == 2, "structured update for 1 or 2 sources");
    constexpr int NA = M * M;
    constexpr int PIECES = M / 2;     // 16-byte pieces of one M-vector
    constexpr int MP = M <= 2 ? 2 : (M <= 4 ? 4 : 8);      // the update's square lane layout is a power of two (6 channels: 8 x 8, identity outside 6 x 6)
    constexpr int G = MP * MP;        // lanes per bin in the update
    constexpr int BW = 64 / G;        // bins per wave in the update
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ __attribute__((aligned(16))) u64 rs_dma[kWaves][128];      // the row's sums of r as each wave fetched them (floor_request)
    const ResidentGeom gm = a.g;
    const int JL = gm.J - JR;
    float4* xs = reinterpret_cast<float4*>(smem);                                        // [JL][PIECES][kBlock]
    float* wtab = reinterpret_cast<float*>(smem + (size_t)JL * PIECES * kBlock * 16);    // [TW][K] float, or double (COV64)
    double* wtab64 = reinterpret_cast<double*>(wtab);
    float* red = wtab + 2 * kResidentMaxTW * K;                                          // [kResChunk][kResStride]
    double* bsum = reinterpret_cast<double*>(red + kResRedFloats);                       // [kWaves] (+ 16 spare bytes)
    float* rtab = reinterpret_cast<float*>(bsum + kWaves + 2);                           // [TW][K] the activations r of the split's frames

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = lane & 15;
    const int q = tid >> 4;                   // frame phase 0..15
    const int bid = blockIdx.x;
    // Workgroup -> (bin group g, frame split c).  Two of the three hand-offs of an iteration run along a ROW (same g): the
    // partial covariances to the bin's owner and the new demixing vectors back.  Workgroup b is observed to run on XCD b % 8
    // (not a guarantee), so with a multiple of 8 bin groups the rows are dealt to the XCDs -- XCD x gets rows x NB/8 ... --
    // and a row's words can stay in that XCD's L2 (plain stores) instead of travelling through the fabric; whether a row really
    // sits on one XCD is CHECKED below (row_local) before any plain store is made.
    const bool remap = gm.NB % 8 == 0 && gm.NS > 1;
    const int g = remap ? (bid % 8) * (gm.NB / 8) + (bid / 8) / gm.NS : bid / gm.NS;
    const int c = remap ? (bid / 8) % gm.NS : bid - g * gm.NS;
    const int f = g * 16 + b;
    const bool fvalid = f < a.F;
    const int fc = fvalid ? f : a.F - 1;
    const int t0 = c * gm.TW;
    const int t_end = min(a.T, t0 + gm.TW);
    const int Fp = gm.NB * 16;
    const size_t part_rows = (size_t)gm.NS * gm.TW;       // frames (padded) per bin group in the parts buffer

    auto stamp = [&](int it, int i) {
        if (a.stamps != nullptr && tid == 0 && (bid == 0 || a.stamp_all))
            a.stamps[((size_t)(a.stamp_all ? bid : 0) * a.n_iter + it) * kResidentStamps + i] = (u64)wall_clock64();
    };
    const unsigned giveup_code = (unsigned)bid << 8;

    // ---- which XCD am I on?  published now, compared with the row's other workgroups after the load of X ----
    unsigned my_xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
    my_xcc &= 15u;
    const unsigned launch_tag = (a.epoch0 + 1u) << 8;                  // (epochs never repeat between two clearings of the buffers)
    if (tid == 0 && (bid != a.stall_block || a.stall_iter > 0)) st32(a.xcc_tab + (size_t)g * gm.NS + c, launch_tag | (my_xcc + 1u));

    // ---- X: HBM -> registers / LDS, once per launch (frames past the split or the tensor, bins past F: zeros) ----
    AccFrames<M, JR> xacc;       // the JR register frames, in the accumulator half of the register file
    {
        const float4* px = reinterpret_cast<const float4*>(a.X + (size_t)fc * M);
        const size_t fs4 = (size_t)a.F * PIECES;
        auto fetch = [&](int j, float4 (&v)[PIECES]) {
            const int t = t0 + q + 16 * j;
            const bool live = fvalid && t < t_end;
            const float4* src = px + (size_t)(live ? t : 0) * fs4;
#pragma unroll
            for (int p = 0; p < PIECES; ++p) {
                v[p] = src[p];
                if (!live) v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        static_for<JR>([&](auto jc) {
            float4 v[PIECES];
            fetch(decltype(jc)::value, v);
            xacc.template put<decltype(jc)::value>(v);
        });
        for (int j = JR; j < gm.J; ++j) {
            float4 v[PIECES];
            fetch(j, v);
#pragma unroll
            for (int p = 0; p < PIECES; ++p) xs[((j - JR) * PIECES + p) * kBlock + tid] = v[p];
        }
    }
    // every workgroup of my row on my XCD?  (one word per workgroup, stored before the load of X: no wait in practice; the
    // answer is the same in every workgroup of the row -- producers and consumers of its words agree on the store flavour)
    bool row_local = gm.NS == 1;
    if (gm.NS > 1) {
        const long long tw0 = wall_clock64();
        unsigned w = 0;
        bool bad = false;
        for (unsigned spins = 1;; ++spins) {
            w = ld32(a.xcc_tab + (size_t)g * gm.NS + (lane < gm.NS ? lane : 0));
            if (__all((w & ~255u) == launch_tag)) break;
            if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, ((unsigned)bid << 8) | 5u)) {
                bad = true;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (__syncthreads_or(bad ? 1 : 0)) return;
        row_local = __all((w & 255u) == my_xcc + 1u);
    }
    auto st64_row = [&](void* p, u64 v) {
        if (row_local)
            st64_plain(p, v);
        else
            st64(p, v);
    };
    auto lds_x = [&](int j, float4 (&v)[PIECES]) {
#pragma unroll
        for (int p = 0; p < PIECES; ++p) v[p] = xs[((j - JR) * PIECES + p) * kBlock + tid];
    };

    // ---- per-bin state of the update: lane (i, j) of a group of G lanes holds element [i][j] ----
    const int uwave = wave;
    const int slot0 = c + gm.NS * (uwave * BW);                // first bin (of the group's 16) this wave updates
    const bool wave_updates = slot0 < 16 && g * 16 + slot0 < a.F;
    // the lane's place in the update: element (i, j) of the matrices of bin fu.  Recomputed from the lane number inside
    // every update phase (through an opaque copy of it, so that the compiler cannot keep these values -- and the addresses
    // derived from them -- in registers across the covariance phase, where every register counts)
    struct UGeom {
        int i, j, slot, fu, off;
        bool valid, in;              // valid: the lane group has a bin; in: (i, j) inside the M x M matrices
        float sgn;
    };
    auto ugeom = [&](int ul) {
        UGeom u;
        u.i = (ul % G) / MP;
        u.j = (ul % G) % MP;
        u.slot = c + gm.NS * (uwave * BW + ul / G);
        u.valid = u.slot < 16 && g * 16 + u.slot < a.F;
        u.fu = g * 16 + (u.valid ? u.slot : slot0);            // lane groups without a bin shadow the wave's first one
        u.off = 0;
        u.sgn = 0.f;
        u.in = u.i < M && u.j < M;
        if (u.in) herm_offsets(M, u.i, u.j, u.off, u.sgn);
        return u;
    };
    const Cx<R> czero = {R(0), R(0)};
    Cx<R> Bm = czero, Cm = czero;                              // W_hat^H and Cx of the bin
    {
        const UGeom u = ugeom(lane);
        Bm = {R(u.i == u.j ? 1 : 0), R(0)};
        if (wave_updates && u.in) {
            const size_t idx = ((size_t)u.fu * M + u.j) * M + u.i;     // B[i][j] = conj(W_hat[j][i])
            if (sizeof(R) == 8 && a.what64_valid) {
                const double2 v = a.What64[idx];
                Bm = {R(v.x), R(-v.y)};
            } else {
                const float2 v = a.What[idx];
                Bm = {R(v.x), R(-v.y)};
            }
            const double* pc = a.Cx + (size_t)u.fu * NA + u.off;
            Cm.re = R(pc[0]);
            if (u.sgn != 0.f) Cm.im = R(u.sgn * pc[1]);
        }
    }

    v2f wc[K][M];                                              // conj(w_k) of the lane's bin, (re, im) pairs
    {
        float wr[K][M], wi[K][M];
        load_wconj<M, K>(a.What, fc, 0, K, wr, wi);
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
#pragma unroll
            for (int m = 0; m < M; ++m) wc[kk][m] = v2f{wr[kk][m], wi[kk][m]};
    }
    const float inv_f_total = 1.f / (float)a.F_total;
    u64* const vpart_w = reinterpret_cast<u64*>(a.vpart);      // tagged float64 words
    u64* const rsum_w = reinterpret_cast<u64*>(a.rsum);
    const int rs_row = (gm.NS * K + 1) & ~1;                   // words per row of the sums of r (even: rows start on 16 bytes)
    u64* const wpub_w = reinterpret_cast<u64*>(a.wpub);        // tagged (re, im) float32 pairs

    for (int it = 0; it < a.n_iter; ++it) {
        const unsigned epoch = a.epoch0 + 1u + (unsigned)it;
        const int par = (int)(epoch & 1u);
        bool fail = false;
        const bool stalled = bid == a.stall_block && it >= a.stall_iter;       // test hook: this workgroup publishes nothing (from that iteration on)
        stamp(it, 0);
        // ================= demix + source powers (overiva.py:140, :153/:155) =================
        {
            float* mypart = a.parts + (((size_t)par * gm.NB + g) * part_rows + t0) * K;
            // y_k = sum_m conj(w_km) x_m on (re, im) pairs: two packed FMAs per (channel, source), two chains per source
            auto power_frame = [&](const float4 (&v)[PIECES], int j) {
                float pw[K];
#pragma unroll
                for (int kk = 0; kk < K; ++kk) {
                    v2f y0 = {0.f, 0.f}, y1 = {0.f, 0.f};
#pragma unroll
                    for (int p = 0; p < PIECES; ++p) {
                        const v2f x0 = {v[p].x, v[p].y}, x1 = {v[p].z, v[p].w};
                        y0 = pk_fma_w0(wc[kk][2 * p], x0, y0);
                        y1 = pk_fma_w0(wc[kk][2 * p + 1], x1, y1);
                        y0 = pk_fma_wy_rot(wc[kk][2 * p], x0, y0);
                        y1 = pk_fma_wy_rot(wc[kk][2 * p + 1], x1, y1);
                    }
                    const v2f y = y0 + y1;
                    pw[kk] = row16_sum(fmaf(y.x, y.x, y.y * y.y));          // the 16 bins of the group (zero rows for bins >= F)
                }
                if (b == 0 && !stalled) {
                    const int tl = q + 16 * j;
                    if constexpr (K == 2)
                        st64(reinterpret_cast<u64*>(mypart) + tl, pack_f2(pw[0], pw[1], epoch));
                    else
                        st32(mypart + tl, pack_f1(pw[0], epoch));
                }
            };
            static_for<JR>([&](auto jc) {
                float4 v[PIECES];
                xacc.template get<decltype(jc)::value>(v);
                power_frame(v, decltype(jc)::value);
            });
            if (JR < gm.J) {                       // LDS frames, the next one requested before the current is used
                float4 cur[PIECES], nxt[PIECES];
                lds_x(JR, cur);
                for (int j = JR; j < gm.J; ++j) {
                    if (j + 1 < gm.J) lds_x(j + 1, nxt);
                    power_frame(cur, j);
#pragma unroll
                    for (int p = 0; p < PIECES; ++p) cur[p] = nxt[p];
                }
            }
        }
        stamp(it, 1);
        // ================= activation (overiva.py:152-155, :170-173) =================
        double rs[K];
        {
            const int tl = tid;                   // one thread per frame of the split
            const bool mine = tl < gm.TW;
            const bool live = mine && t0 + tl < t_end;
            float p[K];
#pragma unroll
            for (int kk = 0; kk < K; ++kk) p[kk] = 0.f;
            // (addresses as a wave-uniform base + a 32-bit lane offset: 64-bit per-lane addresses of 32 loads in flight would
            //  take 64 registers)
            const float* ubase = a.parts + ((size_t)par * gm.NB * part_rows + t0) * K;
            const unsigned voff = (unsigned)((mine ? tl : 0) * K);
            const size_t gstride = part_rows * K;
            const long long tw0 = wall_clock64();
            // Bins sharded over several GPUs: every workgroup adds its OWN rank's parts itself, exactly as on one GPU (no hop
            // inside the rank); the column's leader (one workgroup per rank and frame split) also stores that sum into every OTHER
            // rank's gather buffer (peer stores over xGMI, same tagged words), and every workgroup of the column, on every rank,
            // adds the ranks' sums in rank order -- its own as the tagged word the other ranks see (same bits everywhere), the
            // others' from its rank's buffer.  The other ranks' leaders gather while this workgroup does, so what the exchange
            // adds to the single-GPU hop is their stores' flight and one poll.
            const bool multi = a.world > 1;
            const bool leader = g == c % gm.NB;
            // Many bin groups (2049 bins = 129 groups, one frame split): every workgroup gathering every group's parts is
            // NB x TW x K words per workgroup (19 us of a 33 us iteration, measured).  Two hops instead: the workgroups of a
            // column share its TW frames out (reduce-scatter: workgroup g sums frames [g S, g S + S) over all NB producers,
            // one producer per thread), publish those sums, and every workgroup reads the TW sums (all-gather): 2 (TW K)
            // words per workgroup and two hand-offs.
            const bool twohop = !multi && gm.NB >= kResidentTwoHopGroups;
            if (twohop) {
                constexpr int kMaxS = (kResidentMaxTW + kResidentTwoHopGroups - 1) / kResidentTwoHopGroups;
                using word_t = std::conditional_t<K == 2, u64, unsigned>;
                const int S = (gm.TW + gm.NB - 1) / gm.NB;
                const int s_lo = g * S, ns = min(S, gm.TW - s_lo);       // this workgroup's frames of the column (ns <= 0: none)
                float* const psum = a.psum + ((size_t)par * part_rows + t0) * K;
                if (ns > 0) {                                            // (workgroup-uniform)
                    const bool prod = tid < gm.NB;                       // thread = producer (NB <= 256 = kBlock)
                    const float* src = a.parts + (((size_t)par * gm.NB + (prod ? tid : 0)) * part_rows + t0 + s_lo) * K;
                    float v[kMaxS][K];
                    for (unsigned spins = 1;; ++spins) {
                        bool ok = true;
#pragma unroll
                        for (int sidx = 0; sidx < kMaxS; ++sidx) {
                            word_t x;
                            if constexpr (K == 2)
                                x = sidx < ns ? ld64(src + sidx * K) : pack_f2(0.f, 0.f, epoch);
                            else
                                x = sidx < ns ? ld32(src + sidx * K) : pack_f1(0.f, epoch);
                            if constexpr (K == 2) {
                                ok = ok && tag_f2(x) == (epoch & 3u);
                                v[sidx][0] = lo_f2(x);
                                v[sidx][1] = hi_f2(x);
                            } else {
                                ok = ok && tag_f1(x) == (epoch & 3u);
                                v[sidx][0] = val_f1(x);
                            }
                        }
                        if (__all(ok || !prod)) break;
                        if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 1u)) {
                            fail = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    // sum over the producers: butterfly inside the wave, the four waves in order (fixed order)
#pragma unroll
                    for (int sidx = 0; sidx < kMaxS; ++sidx) {
#pragma unroll
                        for (int kk = 0; kk < K; ++kk) {
                            float x = prod ? v[sidx][kk] : 0.f;
#pragma unroll
                            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
                            if (lane == 0) red[(sidx * K + kk) * kWaves + wave] = x;
                        }
                    }
                    __syncthreads();
                    if (tid < ns && !fail && !stalled) {
                        float sk[K];
#pragma unroll
                        for (int kk = 0; kk < K; ++kk) {
                            const float* rp = red + (tid * K + kk) * kWaves;
                            sk[kk] = ((rp[0] + rp[1]) + rp[2]) + rp[3];
                        }
                        if constexpr (K == 2)
                            st64(reinterpret_cast<u64*>(psum) + s_lo + tid, pack_f2(sk[0], sk[1], epoch));
                        else
                            st32(psum + s_lo + tid, pack_f1(sk[0], epoch));
                    }
                    __syncthreads();                                     // `red` is reused below
                }
                // all-gather: one word per frame of the split
                for (unsigned spins = 1;; ++spins) {
                    bool ok = true;
                    if (mine) {
                        if constexpr (K == 2) {
                            const u64 x = ld64(psum + (size_t)tl * K);
                            ok = tag_f2(x) == (epoch & 3u);
                            p[0] = lo_f2(x);
                            p[1] = hi_f2(x);
                        } else {
                            const unsigned x = ld32(psum + tl);
                            ok = tag_f1(x) == (epoch & 3u);
                            p[0] = val_f1(x);
                        }
                    }
                    if (__all(ok)) break;
                    if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 2u)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            } else {
                // sentinels: the word each of a producer's four waves stores LAST (its last frame phase at the last frame index:
                // the waves of the power phase run unsynchronised, so one word per workgroup says nothing about the other three
                // waves -- measured: with a single sentinel the payload pass of a 33-producer column failed and was repeated,
                // 5.7 us per hop instead of 2.5).  A pass over 4 NB words instead of the wave's NB KB while the column computes.
                for (unsigned spins = 1;; ++spins) {
                    // (all of a lane's words requested before any is looked at: `ok && load` would make every load wait for
                    //  the one before it)
                    unsigned bad = 0;
                    for (int i0 = 0; i0 < 4 * gm.NB; i0 += 256) {
                        unsigned tg[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int i = i0 + 64 * u + lane;
                            const int ic = i < 4 * gm.NB ? i : 4 * gm.NB - 1;
                            const int gs = ic >> 2, tls = 4 * (ic & 3) + 3 + 16 * (gm.J - 1);
                            const float* sp = a.parts + (((size_t)par * gm.NB + gs) * part_rows + t0 + tls) * K;
                            if constexpr (K == 2)
                                tg[u] = tag_f2(ld64(sp));
                            else
                                tg[u] = tag_f1(ld32(sp));
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) bad |= tg[u] ^ (epoch & 3u);
                    }
                    if (__all(bad == 0u)) break;
                    if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 1u)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                constexpr int CH = M == 4 ? 4 : 2;       // rounds of 16 producers requested together (register budget)
                for (int g0 = 0; g0 < gm.NB && !fail; g0 += 16 * CH) {
                    float v[CH][16][K];
                    for (unsigned spins = 1;; ++spins) {
                        // All words are requested before any is looked at, by the lanes that own a frame and for the
                        // producers that exist only: these loads are served by the fabric, not by L2, and every workgroup of
                        // the column fetches the same words -- at configs[1] idle lanes and clamped duplicates were 60 % of
                        // 23 MB per pass.  (A test of each word right behind its load serialises the loads: 13 us per hop.)
                        using word_t = std::conditional_t<K == 2, u64, unsigned>;
                        word_t xw[CH][16];
                        word_t fill;
                        if constexpr (K == 2)
                            fill = pack_f2(0.f, 0.f, epoch);
                        else
                            fill = pack_f1(0.f, epoch);
#pragma unroll
                        for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
                            for (int u = 0; u < 16; ++u) xw[ch][u] = fill;
                        }
                        if (mine) {
#pragma unroll
                            for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
                                for (int u = 0; u < 16; ++u) {
                                    const int gg = g0 + 16 * ch + u;
                                    if (gg < gm.NB) {                                  // wave-uniform
                                        const float* ub = ubase + gg * gstride;
                                        if constexpr (K == 2)
                                            xw[ch][u] = ld64(ub + voff);
                                        else
                                            xw[ch][u] = ld32(ub + voff);
                                    }
                                }
                            }
                        }
                        bool ok = true;
#pragma unroll
                        for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
                            for (int u = 0; u < 16; ++u) {
                                if constexpr (K == 2) {
                                    ok = ok && tag_f2(xw[ch][u]) == (epoch & 3u);
                                    v[ch][u][0] = lo_f2(xw[ch][u]);
                                    v[ch][u][1] = hi_f2(xw[ch][u]);
                                } else {
                                    ok = ok && tag_f1(xw[ch][u]) == (epoch & 3u);
                                    v[ch][u][0] = val_f1(xw[ch][u]);
                                }
                            }
                        }
                        if (a.stamps != nullptr && tid == 0 && (bid == 0 || a.stamp_all))      // diagnostics: passes over the payload
                            a.stamps[((size_t)(a.stamp_all ? bid : 0) * a.n_iter + it) * kResidentStamps + 9] = spins;
                        if (__all(ok || !mine)) break;
                        if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 1u)) {
                            fail = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
#pragma unroll
                    for (int ch = 0; ch < CH; ++ch) {
                        if (g0 + 16 * ch < gm.NB) {
#pragma unroll
                            for (int u4 = 0; u4 < 4; ++u4) {
#pragma unroll
                                for (int kk = 0; kk < K; ++kk) {
                                    float e[4];
#pragma unroll
                                    for (int x = 0; x < 4; ++x) e[x] = g0 + 16 * ch + 4 * u4 + x < gm.NB ? v[ch][4 * u4 + x][kk] : 0.f;
                                    p[kk] += ((e[0] + e[1]) + e[2]) + e[3];
                                }
                            }
                        }
                    }
                }
            }
            if (multi) {
                const size_t goff = ((size_t)par * a.world * part_rows + t0 + (mine ? tl : 0)) * K;      // + rank * part_rows * K
                if (leader && mine && !fail && !stalled) {
                    for (int r = 0; r < a.world; ++r) {
                        if (r == a.rank) continue;
                        // (loop-back: one GPU plays all `world` ranks -- the same stores, into slot r of the OWN buffer, the phantom
                        //  ranks' sums exact zeros: everything of the multi-GPU path but the flight over xGMI, and the same result)
                        float* dst = a.loopback ? a.gath[a.rank] + goff + (size_t)r * part_rows * K
                                                : a.gath[r] + goff + (size_t)a.rank * part_rows * K;
                        if constexpr (K == 2)
                            st64_sys(dst, pack_f2(a.loopback ? 0.f : p[0], a.loopback ? 0.f : p[1], epoch));
                        else
                            st32_sys(dst, pack_f1(a.loopback ? 0.f : p[0], epoch));
                    }
                }
                // this rank's sum as the other ranks read it: through the tagged word
                float own[K];
                if constexpr (K == 2) {
                    const u64 x = pack_f2(p[0], p[1], epoch);
                    own[0] = lo_f2(x);
                    own[1] = hi_f2(x);
                } else {
                    own[0] = val_f1(pack_f1(p[0], epoch));
                }
#pragma unroll
                for (int kk = 0; kk < K; ++kk) p[kk] = 0.f;
                // The other ranks' words of a pass are requested TOGETHER, as raw buffer loads with the system-scope cache bits: a
                // system-scope atomic load is followed by `s_waitcnt vmcnt(0)` (hipcc), i.e. seven round trips to the uncached
                // gather buffer per pass at eight ranks instead of one (the same finding as in activation_xchg_kernel).
                const auto gsrc = __builtin_amdgcn_make_buffer_rsrc(a.gath[a.rank], 0, (int)((size_t)2 * a.world * part_rows * K * sizeof(float)), 0x00020000);
                for (int r0 = 0; r0 < a.world && !fail; r0 += 8) {
                    float v[8][K];
                    for (unsigned spins = 1;; ++spins) {
                        using word_t = std::conditional_t<K == 2, u64, unsigned>;
                        word_t xw[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int r = r0 + u < a.world ? r0 + u : a.world - 1;
                            const int off = (int)((goff + (size_t)r * part_rows * K) * sizeof(float));
                            if constexpr (K == 2) {
                                const auto w2 = __builtin_amdgcn_raw_buffer_load_b64(gsrc, off, 0, /*sc0 sc1: system scope*/ 17);
                                xw[u] = (u64)w2[0] | ((u64)w2[1] << 32);
                            } else {
                                xw[u] = __builtin_amdgcn_raw_buffer_load_b32(gsrc, off, 0, 17);
                            }
                        }
                        bool ok = true;
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int r = r0 + u < a.world ? r0 + u : a.world - 1;
                            if (r == a.rank) {              // (wave-uniform: the own slot is never written, its word is not looked at)
#pragma unroll
                                for (int kk = 0; kk < K; ++kk) v[u][kk] = own[kk];
                                continue;
                            }
                            if constexpr (K == 2) {
                                ok = ok && tag_f2(xw[u]) == (epoch & 3u);
                                v[u][0] = lo_f2(xw[u]);
                                v[u][1] = hi_f2(xw[u]);
                            } else {
                                ok = ok && tag_f1(xw[u]) == (epoch & 3u);
                                v[u][0] = val_f1(xw[u]);
                            }
                        }
                        if (__all(ok || !mine)) break;
                        if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 4u)) {
                            fail = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
#pragma unroll
                        for (int kk = 0; kk < K; ++kk) p[kk] += r0 + u < a.world ? v[u][kk] : 0.f;       // rank order
                    }
                }
            }
            if (__syncthreads_or(fail ? 1 : 0)) return;
            stamp(it, 2);
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                float r = a.model == OIVA_MODEL_LAPLACE ? 2.f * sqrtf(p[kk]) : p[kk] * inv_f_total;
                r = live ? r : 0.f;
                const float rf = r < kTinyR ? kTinyR : r;        // a NaN stays NaN, like r[r < eps] = eps in the reference
                if (mine) {
                    if constexpr (COV64)
                        wtab64[tl * K + kk] = live ? 1. / (double)rf : 0.;
                    else
                        wtab[tl * K + kk] = live ? 1.f / rf : 0.f;
                    rtab[tl * K + kk] = live ? r : __builtin_inff();      // (frames past the end: weight 0, never floored)
                }
                rs[kk] = block_sum((double)r, bsum);             // sum_t r over the split, for gamma (overiva.py:158)
            }
        }
        __syncthreads();
        if (tid == 0 && !stalled) {
#pragma unroll
            for (int kk = 0; kk < K; ++kk) st64_row(rsum_w + (size_t)g * rs_row + c * K + kk, pack_f64(rs[kk], epoch));
        }
        stamp(it, 3);
        // ================= weighted covariance of all sources (overiva.py:179) =================
        {
            // The floor r / gamma >= 1e-15 (overiva.py:170-171).  gamma is the mean over ALL frames, i.e. over the row's NS
            // splits, whose sums are published only now -- so the accumulation runs with the unfloored weights 1 / r_t
            // (1 / 1e-20 for r_t = 0), and frames below the floor are corrected afterwards.  The row's sums are requested when
            // the accumulation ends, the reduction over the frame phases starts on the unfloored sums, and the barrier of
            // its last LDS round carries the decision: every thread has tested its frame against eps * gamma by then.  Only
            // if some frame of the split is below the floor -- silence -- the frames that need it are accumulated a second
            // time, from zero, with the weight difference 1 / (eps gamma) - 1 / r_t, reduced the same way and added to the
            // split's partial before it is published.  Exact, and free when no frame is silent: one load of <= 64 words
            // hidden behind the reduction.
            // (the request moves the words straight into LDS -- global_load_lds, 16 bytes per lane, sc1 like the agent-scope loads
            //  of the polls: no register is held while it is in flight, and the wave reads what it fetched itself, ordered by its
            //  own vmcnt.  Inline assembly: behind the builtin hipcc puts s_waitcnt vmcnt(0) in front of the NEXT LDS read it
            //  sees, whatever the address -- the accumulation's own reads of X -- which would wait for the round trip on the
            //  spot.  The compiler's own vmcnt bookkeeping stays valid: an extra operation in flight only makes its waits stricter.)
            auto floor_request = [&]() {
                const int pl = 2 * lane < gm.NS * K ? lane : 0;                 // lane l fetches words 2 l, 2 l + 1 of the row
                const u64* src = rsum_w + (size_t)g * rs_row + 2 * pl;
                const unsigned dst = (unsigned)(uintptr_t)(&rs_dma[wave][0]);   // LDS byte address (wave-uniform); lane l lands at + 16 l
                unsigned keep_m0;                                               // (M0 = LDS base of the transfer; put back afterwards)
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off sc1\n\ts_nop 1\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep_m0)
                             : "v"(src), "s"(dst)
                             : "memory");
            };
            // 1 / gamma_k of the row from the splits' sums; false: gave up waiting
            auto row_ginv = [&](double (&ginv)[K]) -> bool {
                const int ne = gm.NS * K;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                u64 word = rs_dma[wave][lane < ne ? lane : 0];
                if (!__all(tag_f64(word) == (epoch & 0xFFFFu))) {      // not there yet (rare): poll
                    const long long tw0 = wall_clock64();
                    for (unsigned spins = 1;; ++spins) {
                        word = ld64(rsum_w + (size_t)g * rs_row + (lane < ne ? lane : 0));
                        if (__all(tag_f64(word) == (epoch & 0xFFFFu))) break;
                        if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 2u)) return false;
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                // lane c K + k holds the sum of split c: a tree over the lanes of equal k (the update adds them in split order;
                // the last bit of gamma may differ from its value, which only moves the floor test by that bit)
                double v = lane < ne ? val_f64(word) : 0.;
                if constexpr (K == 1) v += dpp<kDppXor1>(v);
                v += dpp<kDppXor2>(v);
                v += dpp<kDppRor4>(v);
                v += dpp<kDppRor8>(v);
                v = swapsum16(v);
                v = swapsum32(v);
#pragma unroll
                for (int kk = 0; kk < K; ++kk)
                    ginv[kk] = (double)a.T / __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), kk), __builtin_amdgcn_readlane(__double2loint(v), kk));
                return true;
            };
            auto below = [&](float r, double ginv) -> bool {       // the test of the four-launch path (activation_weight)
                if constexpr (COV64)
                    return (double)r * ginv < (double)kEpsR;
                else
                    return r * (float)ginv < kEpsR;
            };
            // evaluated by every thread before the reduction's last barrier: 1 = my frame is below the floor, 2 = gave up
            auto floor_vote = [&]() -> int {
                double ginv[K];
                if (!row_ginv(ginv)) return 2;
                int low = 0;
                if (tid < gm.TW) {
#pragma unroll
                    for (int kk = 0; kk < K; ++kk) low |= below(rtab[tid * K + kk], ginv[kk]) ? 1 : 0;
                }
                return low;
            };
            // the slow path's weights: the difference to the floored weight for frames below the floor, 0 for the others
            // (false: gave up).  Ends with a barrier.
            auto floor_weights = [&]() -> bool {
                double ginv[K];
                const bool ok = row_ginv(ginv);
                if (__syncthreads_or(ok ? 0 : 1)) return false;
                if (tid < gm.TW) {
#pragma unroll
                    for (int kk = 0; kk < K; ++kk) {
                        const bool fl = below(rtab[tid * K + kk], ginv[kk]);
                        if constexpr (COV64)
                            wtab64[tid * K + kk] = fl ? ginv[kk] / (double)kEpsR - wtab64[tid * K + kk] : 0.;
                        else
                            wtab[tid * K + kk] = fl ? (float)ginv[kk] / kEpsR - wtab[tid * K + kk] : 0.f;
                    }
                }
                __syncthreads();
                return true;
            };
            // frame j of the lane, j known at run time only (the register frames through a wave-uniform switch)
            auto fetch_frame = [&](int j, float4 (&v)[PIECES]) {
                if (j < JR) {
                    static_for<JR>([&](auto jc) {
                        if (j == decltype(jc)::value) xacc.template get<decltype(jc)::value>(v);
                    });
                } else {
                    lds_x(j, v);
                }
            };
            // second pass over the frames whose correction weight is not zero in some lane of the wave
            auto correct_frames = [&](auto&& cov_frame) {
                for (int j = 0; j < gm.J; ++j) {
                    bool nz = false;
#pragma unroll
                    for (int kk = 0; kk < K; ++kk) {
                        if constexpr (COV64)
                            nz = nz || wtab64[(q + 16 * j) * K + kk] != 0.;
                        else
                            nz = nz || wtab[(q + 16 * j) * K + kk] != 0.f;
                    }
                    if (!__any(nz)) continue;
                    float4 v[PIECES];
                    fetch_frame(j, v);
                    cov_frame(v, j);
                }
            };

            // ---- sum over the 16 frame phases ----
            // float32 accumulators: first inside the wave, in registers: its 4 phases sit 16 lanes apart, and two rounds of lane
            // swaps (v_permlane32_swap, v_permlane16_swap: one instruction exchanges the halves / the odd and even rows of TWO
            // registers) leave every lane with a QUARTER of the accumulators, each summed over the wave's four phases -- row rho
            // of the wave holds elements e + Q (rho & 1) + H (rho >> 1), e < Q.  Then the four waves through LDS, added in
            // float64: a quarter of the LDS traffic and 3 barriers instead of 16.  The float32 chain of an element is 16 frames
            // of a lane plus the 4-lane tree.  float64 accumulators (COV64): rounds of 8 doubles through the same scratch.
            // The results stay in registers (a __syncthreads() behind a write-through store waits for the store's round trip)
            // and are stored by `publish`; the barrier of the last round is a __syncthreads_or of `vote()`.
            // (the lane-swap rounds want a power of two: 6 channels pad their 36 / 72 accumulators with zeros to 64 / 128)
            constexpr int NACC0 = NA * K;
            constexpr int NACC = COV64 ? NACC0 : (NACC0 <= 16 ? 16 : (NACC0 <= 32 ? 32 : (NACC0 <= 64 ? 64 : 128)));
            constexpr int RH = NACC / 2, RQ = NACC / 4;
            constexpr int RS = COV64 ? kResChunk / 2 : (RQ < 16 ? RQ : 16);     // accumulators per LDS round of the fast path
            constexpr int RNR = COV64 ? NACC / RS : RQ / RS;
            constexpr int RNB = COV64 ? 1 : RS / 4;                             // results per thread and round
            constexpr int NRES = RNR * RNB;                                     // results per thread (float32 paths: NACC / 16 either way)
            static_assert(COV64 || (RQ % RS == 0 && RS % 4 == 0 && NRES == NACC / 16), "whole rounds");
            // Few frames per lane (small problems: no time to gain there, and the four lanes' float32 tree would be most of the
            // float32 rounding of a sum): all 16 phases through LDS, added in float64, as in round 3.
            const bool all_f64 = !COV64 && JR == 0 && gm.J <= kResidentF64ReduceFrames;      // (JR > 0: more than 8 frames per lane)
            int rt = tid;                        // (opaque copy: the indices below are recomputed here every iteration, not kept)
            asm volatile("" : "+v"(rt));
            const int rslot = rt % RS, rrho = (rt / RS) & 3, rgrp = rt / (4 * RS);
            auto reduce = [&](auto&& at, double (&res)[NRES], auto&& vote) -> int {
                int flag = 0;
                if constexpr (COV64) {
                    const int bb = rt >> 4, aa = rt & 15;
                    double* red64 = reinterpret_cast<double*>(red);
                    static_for<RNR>([&](auto rc) {
                        constexpr int r0 = decltype(rc)::value * RS;
                        if constexpr (decltype(rc)::value > 0) __syncthreads();
                        static_for<RS>([&](auto ac) { red64[decltype(ac)::value * kResStride + rt] = at(std::integral_constant<int, r0 + decltype(ac)::value>{}); });
                        if constexpr (decltype(rc)::value == RNR - 1)
                            flag = __syncthreads_or(vote());
                        else
                            __syncthreads();
                        double sum = 0.;
                        if (aa < RS) {
#pragma unroll
                            for (int qq = 0; qq < 16; ++qq) sum += red64[aa * kResStride + qq * 16 + bb];
                        }
                        res[decltype(rc)::value] = sum;
                    });
                } else if (all_f64) {
                    const int bb = rt >> 4, aa = rt & 15;              // result r of the thread: element 16 r + aa of bin bb
                    static_for<NRES>([&](auto rc) {
                        constexpr int r0 = decltype(rc)::value * 16;
                        if constexpr (decltype(rc)::value > 0) __syncthreads();
                        static_for<16>([&](auto ac) { red[decltype(ac)::value * kResStride + rt] = at(std::integral_constant<int, r0 + decltype(ac)::value>{}); });
                        if constexpr (decltype(rc)::value == NRES - 1)
                            flag = __syncthreads_or(vote());
                        else
                            __syncthreads();
                        double sum = 0.;
#pragma unroll
                        for (int qq = 0; qq < 16; ++qq) sum += (double)red[aa * kResStride + qq * 16 + bb];
                        res[decltype(rc)::value] = sum;
                    });
                } else {
                    float t[RQ];
                    static_for<RQ>([&](auto ec) {
                        constexpr int e = decltype(ec)::value;
                        auto sw32 = [](float x, float y) {
                            auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                            return __uint_as_float(r[0]) + __uint_as_float(r[1]);
                        };
                        const float sa = sw32(at(std::integral_constant<int, e>{}), at(std::integral_constant<int, e + RH>{}));            // rows 0-1: e, rows 2-3: e + H
                        const float sb = sw32(at(std::integral_constant<int, e + RQ>{}), at(std::integral_constant<int, e + RQ + RH>{}));  // e + Q | e + Q + H
                        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(sa), __float_as_uint(sb), false, false);
                        t[e] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
                    });
                    static_for<RNR>([&](auto rc) {
                        constexpr int r0 = decltype(rc)::value * RS;
                        if constexpr (decltype(rc)::value > 0) __syncthreads();
                        static_for<RS>([&](auto ac) { red[decltype(ac)::value * kResStride + rt] = t[r0 + decltype(ac)::value]; });
                        if constexpr (decltype(rc)::value == RNR - 1)
                            flag = __syncthreads_or(vote());
                        else
                            __syncthreads();
#pragma unroll
                        for (int i = 0; i < RNB; ++i) {
                            const float* rp = red + rslot * kResStride + rrho * 16 + rgrp * RNB + i;
                            res[decltype(rc)::value * RNB + i] = (((double)rp[0] + (double)rp[64]) + (double)rp[128]) + (double)rp[192];
                        }
                    });
                }
                return flag;
            };
            auto publish = [&](const double (&res)[NRES]) {
                if (stalled) return;
                if (COV64 || all_f64) {
                    const int bb = rt >> 4, aa = rt & 15;
                    constexpr int ST = COV64 ? RS : 16;
                    u64* out = vpart_w + ((size_t)c * Fp + g * 16 + bb) * K * NA;
                    if (aa < ST)
                        static_for<NRES>([&](auto rc) {
                            if (decltype(rc)::value * ST + aa < NACC0) st64_row(out + decltype(rc)::value * ST + aa, pack_f64(res[decltype(rc)::value], epoch));
                        });
                } else {
                    // (a bin's words all come from one wave; the word the consumers watch -- source K - 1, last packed element:
                    //  row 3, the last slot of the last round -- goes in that wave's last store of the bin)
                    const int e0 = rslot + RQ * (rrho & 1) + RH * (rrho >> 1);
                    u64* out = vpart_w + ((size_t)c * Fp + g * 16 + rgrp * RNB) * K * NA + e0;
                    static_for<RNR>([&](auto rc) {
#pragma unroll
                        for (int i = 0; i < RNB; ++i)
                            if (e0 + decltype(rc)::value * RS < NACC0)
                                st64_row(out + (size_t)i * K * NA + decltype(rc)::value * RS, pack_f64(res[decltype(rc)::value * RNB + i], epoch));
                    });
                }
            };
            // accumulate, with the request half way (done by the caller) -> reduce | vote -> [correct, reduce, add] -> publish
            auto finish = [&](auto&& at0, auto&& clear, auto&& cov_frame) {
                stamp(it, 4);
                // (accumulators past the real ones -- padding of the lane-swap rounds -- read as zeros)
                auto at = [&](auto ec) {
                    if constexpr (decltype(ec)::value < NACC0)
                        return at0(ec);
                    else
                        return decltype(at0(std::integral_constant<int, 0>{}))(0);
                };
                double res[NRES];
                const int flag = reduce(at, res, floor_vote);
                if (flag) {
                    __syncthreads();                    // every wave is done with the reduction scratch and the unfloored weights
                    if (!floor_weights()) {
                        fail = true;
                        return;
                    }
                    clear();
                    correct_frames(cov_frame);
                    double res2[NRES];
                    (void)reduce(at, res2, []() { return 0; });
#pragma unroll
                    for (int r = 0; r < NRES; ++r) res[r] += res2[r];
                }
                publish(res);
            };

            if constexpr (COV64) {
                // float64 sums of exact products (overiva.py:127-128,179 for complex128 input): one lane per (bin, frame), 16
                // real sums per source
                double acc[K][NA];
                auto clear = [&]() {
#pragma unroll
                    for (int kk = 0; kk < K; ++kk)
#pragma unroll
                        for (int e = 0; e < NA; ++e) acc[kk][e] = 0.;
                };
                clear();
                auto cov_frame = [&](const float4 (&v)[PIECES], int j) {
                    double xr[M], xi[M], w[K];
#pragma unroll
                    for (int p = 0; p < PIECES; ++p) {
                        xr[2 * p] = v[p].x;
                        xi[2 * p] = v[p].y;
                        xr[2 * p + 1] = v[p].z;
                        xi[2 * p + 1] = v[p].w;
                    }
#pragma unroll
                    for (int kk = 0; kk < K; ++kk) w[kk] = wtab64[(q + 16 * j) * K + kk];
                    accumulate<M, K, false, double>(acc, xr, xi, w);
                };
                for (int j = 0; j < gm.J; ++j) {
                    if (j == gm.J / 2) floor_request();
                    float4 v[PIECES];
                    lds_x(j, v);
                    cov_frame(v, j);
                }
                finish([&](auto ec) { return acc[decltype(ec)::value / NA][decltype(ec)::value % NA]; }, clear, cov_frame);
            } else if constexpr (K == 2) {
                PkAcc2<M> pacc;
                pacc.clear();
                auto cov_frame = [&](const float4 (&v)[PIECES], int j) {
                    v2f x[M];
#pragma unroll
                    for (int p = 0; p < PIECES; ++p) {
                        x[2 * p] = v2f{v[p].x, v[p].y};
                        x[2 * p + 1] = v2f{v[p].z, v[p].w};
                    }
                    const float2 w = *reinterpret_cast<const float2*>(wtab + (q + 16 * j) * 2);
                    pacc.add(x, v2f{w.x, w.y});
                };
                static_for<JR>([&](auto jc) {
                    float4 v[PIECES];
                    xacc.template get<decltype(jc)::value>(v);
                    cov_frame(v, decltype(jc)::value);
                });
                if (JR > 0) floor_request();              // (the register frames took a few microseconds: the row's sums have landed)
                if (JR < gm.J) {
                    float4 cur[PIECES], nxt[PIECES];
                    lds_x(JR, cur);
                    for (int j = JR; j < gm.J; ++j) {
                        if (j + 1 < gm.J) lds_x(j + 1, nxt);
                        if (JR == 0 && j == gm.J / 2) floor_request();
                        cov_frame(cur, j);
#pragma unroll
                        for (int p = 0; p < PIECES; ++p) cur[p] = nxt[p];
                    }
                }
                finish([&](auto ec) { return pacc.at(decltype(ec)::value); }, [&]() { pacc.clear(); }, cov_frame);
            } else {
                float acc[1][NA];
                auto clear = [&]() {
#pragma unroll
                    for (int e = 0; e < NA; ++e) acc[0][e] = 0.f;
                };
                clear();
                auto cov_frame = [&](const float4 (&v)[PIECES], int j) {
                    float xr[M], xi[M];
#pragma unroll
                    for (int p = 0; p < PIECES; ++p) {
                        xr[2 * p] = v[p].x;
                        xi[2 * p] = v[p].y;
                        xr[2 * p + 1] = v[p].z;
                        xi[2 * p + 1] = v[p].w;
                    }
                    const float w[1] = {wtab[q + 16 * j]};
                    accumulate<M, 1, false, float>(acc, xr, xi, w);
                };
                static_for<JR>([&](auto jc) {
                    float4 v[PIECES];
                    xacc.template get<decltype(jc)::value>(v);
                    cov_frame(v, decltype(jc)::value);
                });
                if (JR > 0) floor_request();
                for (int j = JR; j < gm.J; ++j) {
                    if (JR == 0 && j == gm.J / 2) floor_request();
                    float4 v[PIECES];
                    lds_x(j, v);
                    cov_frame(v, j);
                }
                finish([&](auto ec) { return acc[0][decltype(ec)::value]; }, clear, cov_frame);
            }
            if (fail) return;       // (block-uniform: decided behind a __syncthreads_or)
        }
        stamp(it, 5);
        // ================= per-bin update (overiva.py:158-167 scale, :181-190) =================
        if (wave_updates) {
            int ul = lane;
            asm volatile("" : "+v"(ul));
            const UGeom ug = ugeom(ul);
            const Sq<MP, R> sq(ul % G);
            const int ui = ug.i, uj = ug.j, fu = ug.fu, off = ug.off;
            const bool uvalid = ug.valid, uin = ug.in;
            const float sgn = ug.sgn;
            // V_s = gamma_s / T * fixed-order float64 sum of the splits' partials (reduction tail of overiva.py:179);
            // gamma_k = mean_t r (overiva.py:158) from the splits' sums of r.  All words of a round of 16 splits (and
            // the sums of r) are requested together and re-read until every one carries this epoch.
            // (one straight-line batch of loads for all sources: a variant in which a second wave took the second source's
            //  partials and inversion -- predicated loads -- measured 2 us SLOWER per iteration; the two inversions interleave
            //  well enough in one wave)
            const size_t sstride = (size_t)Fp * K * NA;
            const int e = ul % G;               // lane of the bin's group; lanes e < M * M each sum one packed word over the splits
            const unsigned vvoff = (unsigned)(fu * K * NA + (e < NA ? e : 0));      // lane part of the addresses; the rest is wave-uniform
            const int ne = gm.NS * K;           // sums of r of the row: <= 64 words, lane l fetches word l
            double se[K];
#pragma unroll
            for (int s = 0; s < K; ++s) se[s] = 0.;
            u64 rs_word = 0;
            const long long tw0 = wall_clock64();
            // sentinel: the word of this bin a split's workgroup stores last (source K - 1, last packed element)
            {
                const int cs = ul % gm.NS;
                const u64* sp = vpart_w + cs * sstride + ((size_t)fu * K + (K - 1)) * NA + (NA - 1);
                for (unsigned spins = 1;; ++spins) {
                    if (__all(tag_f64(ld64(sp)) == (epoch & 0xFFFFu))) break;
                    if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 2u)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            for (int c0 = 0; c0 < gm.NS && !fail; c0 += 16) {
                u64 vw[K][16];
                for (unsigned spins = 1;; ++spins) {
                    bool ok = true;
                    if (c0 == 0) {
                        rs_word = ld64(rsum_w + (size_t)g * rs_row + (ul < ne ? ul : 0));
                        ok = tag_f64(rs_word) == (epoch & 0xFFFFu);
                    }
#pragma unroll
                    for (int s = 0; s < K; ++s) {
#pragma unroll
                        for (int u = 0; u < 16; ++u) {
                            const int cc = c0 + u < gm.NS ? c0 + u : gm.NS - 1;
                            vw[s][u] = ld64(vpart_w + (cc * sstride + (size_t)s * NA) + vvoff);
                            ok = ok && tag_f64(vw[s][u]) == (epoch & 0xFFFFu);
                        }
                    }
                    if (__all(ok)) break;
                    if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 2u)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
#pragma unroll
                for (int s = 0; s < K; ++s) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) se[s] += (c0 + u < gm.NS ? 1. : 0.) * val_f64(vw[s][u]);
                }
            }
            stamp(it, 6);
            if (!fail) {
                double gam[K];
                const double mine = val_f64(rs_word);
#pragma unroll
                for (int kk = 0; kk < K; ++kk) {
                    double sum = 0.;
                    for (int cc = 0; cc < gm.NS; ++cc) {      // split order
                        const int src = cc * K + kk;
                        sum += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mine), src),
                                                __builtin_amdgcn_readlane(__double2loint(mine), src));
                    }
                    gam[kk] = sum / (double)a.T;
                }
                // element [i][j] of V_s = packed words off (re) and off + 1 (im) of the bin, held by the lanes of its group
                Cx<R> V[K];
                const int gbase = ul - e;
#pragma unroll
                for (int s = 0; s < K; ++s) {
                    const double sr = __shfl(se[s], gbase + off, 64);
                    const double si = __shfl(se[s], gbase + (off + 1 < NA ? off + 1 : off), 64);
                    const double sc = gam[s] / (double)a.T;
                    V[s] = {R(sr * sc), R(si * sc * (double)sgn)};
                    if (!uin) V[s] = {R(ui == uj ? 1 : 0), R(0)};      // identity outside M x M
                }
                // W[:, k] /= gamma (laplace) | sqrt(gamma) (gauss), overiva.py:163 / :167
                if (ui < K) {
                    const double g0 = gam[0], g1 = gam[K - 1];
                    const double gk = ui == 0 ? g0 : g1;
                    const R sc = R(1. / (a.model == OIVA_MODEL_LAPLACE ? gk : sqrt(gk)));
                    Bm.re *= sc;
                    Bm.im *= sc;
                }
                bg_chain<MP, R, K>(sq, Bm, Cm, V, M);
                if (uvalid && ui < K && uj < M && !stalled)    // conj(w_k)[m] = B[k][m]
                    st64_row(wpub_w + ((size_t)fu * K + ui) * M + uj, pack_f2((float)Bm.re, (float)Bm.im, epoch));
                // the final W_hat goes to a staging copy: the host moves it into place only when NO workgroup gave up (a time-out
                // that strikes in the last iteration must not leave some bins written and others not)
                if (uvalid && uin && it + 1 == a.n_iter) {
                    const size_t idx = ((size_t)fu * M + uj) * M + ui;
                    a.What_out[idx] = make_float2((float)Bm.re, (float)-Bm.im);
                    if (sizeof(R) == 8 && a.What64_out != nullptr) a.What64_out[idx] = make_double2((double)Bm.re, (double)-Bm.im);
                }
            }
        }
        stamp(it, 7);
        // ================= the row's new demixing vectors, for the next iteration's power phase =================
        if (it + 1 < a.n_iter) {
            constexpr int NW = 16 * K * M;                 // words of the group's 16 bins
            constexpr int RW = (NW + 63) / 64;
            u64* wl = reinterpret_cast<u64*>(red);         // the reduction scratch is free here
            if (wave == 0) {
                const u64* wb = wpub_w + (size_t)g * NW;
                const long long tw0 = wall_clock64();
                u64 wv[RW];
                for (unsigned spins = 1;; ++spins) {
                    bool ok = true;
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        const int wd = lane + 64 * r;
                        const bool need = wd < NW && g * 16 + wd / (K * M) < a.F;     // bins past F are never written
                        wv[r] = ld64(wb + (wd < NW ? wd : 0));
                        ok = ok && (!need || tag_f2(wv[r]) == (epoch & 3u));
                    }
                    if (__all(ok)) break;
                    if (give_up(spins, tw0, a.ctrl, a.timeout_ticks, giveup_code | 3u)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
#pragma unroll
                for (int r = 0; r < RW; ++r)
                    if (lane + 64 * r < NW) wl[lane + 64 * r] = wv[r];
            }
            if (__syncthreads_or(fail ? 1 : 0)) return;
            const u64* mine_w = wl + (size_t)(fc - g * 16) * K * M;
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const u64 x = mine_w[kk * M + m];
                    wc[kk][m] = v2f{lo_f2(x), hi_f2(x)};
                }
            }
        } else {
            // (dead values: without this the old vectors stay live around the whole loop body, i.e. across the covariance
            //  phase, and the register allocator parks them in the accumulator file and fetches them back for every frame)
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
#pragma unroll
                for (int m = 0; m < M; ++m) wc[kk][m] = v2f{0.f, 0.f};
            }
        }
        if (__syncthreads_or(fail ? 1 : 0)) return;
        stamp(it, 8);
    }
}

template <int M, int K, int JR, typename R, bool COV64 = false>
hipError_t launch_resident_one(hipStream_t s, const ResidentArgs& a) {
    auto kern = resident_kernel<M, K, JR, R, COV64>;
    // (the attribute and the occupancy answer are per kernel, device and LDS size: asked once, not on every launch -- the two
    //  calls cost more host time than the launch itself)
    static thread_local int ok_dev = -1, ok_lds = -1;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (ok_dev != dev || ok_lds != a.g.lds_bytes) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, a.g.lds_bytes);
        if (e != hipSuccess) return e;
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlock, (size_t)a.g.lds_bytes);
        if (e != hipSuccess) return e;
        if (per_cu < 1) return hipErrorLaunchOutOfResources;      // the grid must be resident as a whole (one workgroup per CU)
        ok_dev = dev;
        ok_lds = a.g.lds_bytes;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.g.NB * a.g.NS)), dim3(kBlock), (size_t)a.g.lds_bytes, s, a);
    return hipGetLastError();
}

template <int M>
hipError_t launch_resident_m(hipStream_t s, const ResidentArgs& a, int K, bool update_f64, bool cov_f64) {
    constexpr int JRM = M >= 6 ? kResidentRegFrames : 0;
    const bool regs = a.g.JR > 0;
    if (regs && JRM == 0) return hipErrorInvalidValue;
    if (cov_f64) {
        if constexpr (M == 4) {
            if (!update_f64 || regs) return hipErrorInvalidValue;
            if (K == 2) return launch_resident_one<M, 2, 0, double, true>(s, a);
            if (K == 1) return launch_resident_one<M, 1, 0, double, true>(s, a);
        }
        return hipErrorInvalidValue;
    }
    if constexpr (M > 2) {      // (sources with background channels only, K < M: resident_geometry)
        if (K == 2) {
            if (regs) return update_f64 ? launch_resident_one<M, 2, JRM, double>(s, a) : launch_resident_one<M, 2, JRM, float>(s, a);
            return update_f64 ? launch_resident_one<M, 2, 0, double>(s, a) : launch_resident_one<M, 2, 0, float>(s, a);
        }
    }
    if (K == 1) {
        if (regs) return update_f64 ? launch_resident_one<M, 1, JRM, double>(s, a) : launch_resident_one<M, 1, JRM, float>(s, a);
        return update_f64 ? launch_resident_one<M, 1, 0, double>(s, a) : launch_resident_one<M, 1, 0, float>(s, a);
    }
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace oiva
