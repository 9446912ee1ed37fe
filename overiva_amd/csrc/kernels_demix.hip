// Kernels that apply the demixing vectors to X: the per-iteration source-power pass and the epilogue.
//
//   power : p[t,k] = sum_f |w_{f,k}^H x_{t,f}|^2      reference overiva.py:140 + the norms of :153/:155
//           (Y itself is never stored inside the loop: the reference's Y /= gamma at :162/:166 is dead)
//   stats : per-bin sums for projection back          reference overiva.py:197-198 (pyroomacoustics formula)
//   write : Y[t,f,k] = w_{f,k}^H x_{t,f} (* conj z)   reference overiva.py:192-199
#include "oiva_device.h"
#include "demix_arith.h"

namespace oiva {
namespace {

// ---------------------------------------------------------------------------------------------
// power: block = 4 waves x 16 bins = 64 bins, 4 frame phases per wave, frames [t_begin, t_begin+tcp)
// rev: the pass runs AGAINST the covariance pass (ord.cs splits, each walked ascending): the rows of the grid take their chunks
// tail first (power_chunk_tail_first) and every chunk is walked from its last step to its first, so that the launch starts on
// the X the covariance pass read last and ends on the X it reads first.  Frames are independent of each other (the sums run
// over bins), so every word of Ppart keeps its place and its bits.  rev == 0: chunk = row, ascending.
// NT: the instantiation that follows the load policy of X (kernel_choice.h; 8 channels, launched only where some group
// streams).  Every load step goes HBM -> LDS row by row (XRows, oiva_device.h), a step of a resident group with plain requests, one
// of a streamed group with nt requests, into a private ring of kPowStages stages per wave: the wave requests step n + 1, waits
// with a counted vmcnt for step n alone and picks its own M-vector up from there -- the registers the arithmetic sees are the
// same values as in the plain instantiation.  A wave reads only what it requested itself: no barrier inside the loop.  Steps
// past the end of the chunk re-request a legal address that is never consumed, so that every step adds the same count to vmcnt.
// hipcc counts LDS-DMA like any load and drains the queue (vmcnt(0)) in front of every LDS access it can see: the reads of
// the ring (ring_read_rows) and the store of a step's sums (lds_store) are inline assembly for that reason.
// Two stages, measured on the pure-read form (tools/mallbench.hip, rows q = "e"): three and four run slower.
// ---------------------------------------------------------------------------------------------
constexpr int kPowUnroll = 2;
constexpr int kPowStages = 2;

// sp[idx] = v out of the compiler's sight (see above); LDS stores of a wave complete in order, the wave waits for them with
// lds_stores_done() before anyone reads them
__device__ __forceinline__ void lds_store(float* base, int idx, float v) {
    asm volatile("ds_write_b32 %0, %1" : : "v"((unsigned)(uintptr_t)base + 4u * (unsigned)idx), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_stores_done() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

template <int M, int KP, bool NT = false>
__global__ __launch_bounds__(kBlock) void power_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                       float* __restrict__ Ppart, int T, int F, int K, int tcp, int rev, PowOrder ord,
                                                       int xplain, int xctc) {
    extern __shared__ __attribute__((aligned(16))) float sp[];  // [kWaves][tcp][KP]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = NT ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int b = lane & 15;
    const int q = lane >> 4;
    const int f = (blockIdx.x * kWaves + wave) * kBinsPerWave + b;
    const bool fvalid = f < F;
    const int fc = fvalid ? f : F - 1;
    const int k0 = blockIdx.z * KP;
    const int chunk = ord.cs > 0 ? power_chunk_tail_first(blockIdx.y, gridDim.y, ord) : (int)blockIdx.y;
    const int t_begin = chunk * tcp;
    const int t_end = min(T, t_begin + tcp);
    const int len = t_end - t_begin;
    const int nsteps = (len + 3) >> 2;
    [[maybe_unused]] const int ngroups = (nsteps + kPowUnroll - 1) / kPowUnroll;      // (the plain instantiation's walk)

    // conj(W) of the lane's bin, requested raw and finished when all of it is on its way (load_w_raw, demix_arith.h): one memory
    // round trip instead of one per element.  Not where holding the raw words beside the finished ones costs the
    // instantiation a wave per SIMD (hipcc's resource remarks: one source per pass at 10..16 channels 52..76 -> 65..85 registers,
    // the streamed form with four sources 91 -> 118): pow_blocks_per_cu feeds the choice of the geometry, which stays.
    constexpr bool kRawW = NT ? KP <= 2 : (KP >= 2 || M <= 9);
    float wr[KP][M], wi[KP][M];
    [[maybe_unused]] WRaw<M, KP> wraw;

    const size_t frame_stride = (size_t)F * M;
    [[maybe_unused]] const float2* pbase = X + (size_t)fc * M;
    if constexpr (NT) {
        constexpr int PIECES = XRows<M>::kPieces, STAGE = PIECES * 64;      // float4 per stage per wave
        __shared__ float4 ring[kWaves * kPowStages * STAGE];
        float4* wring = ring + wave * kPowStages * STAGE;                   // wave-uniform
        // where this chunk starts in its covariance split (a chunk is no longer than a split: choose_x_policy), this lane's
        // place in a row-contiguous step and in the landed one
        const int off0 = t_begin % xctc;
        const int row_off = XRows<M>::offset(lane, (blockIdx.x * kWaves + wave) * kBinsPerWave, F);
        const unsigned rd_rows = (unsigned)(uintptr_t)wring + XRows<M>::slot(b, q) * 16;
        auto step_of = [&](int n) { return rev ? nsteps - 1 - n : n; };     // the n-th step of the walk
        auto issue = [&](int n, int s) {
            const int i = n < nsteps ? step_of(n) : 0;
            const int t_lim = n < nsteps ? t_end : 0;                       // past the end: frame T - 1 four times
            if (x_group_plain(x_split_offset(off0, 4 * i, xctc), xplain))   // wave-uniform
                XRows<M>::template issue<0>(X, frame_stride, row_off, lane, t_begin + 4 * i, t_lim, T, wring + s * STAGE);
            else
                XRows<M>::template issue<2>(X, frame_stride, row_off, lane, t_begin + 4 * i, t_lim, T, wring + s * STAGE);
        };
        auto consume = [&](int n, int s) {
            float4 v[PIECES];
            ring_read_rows<PIECES, (kPowStages - 1) * PIECES>(rd_rows + s * STAGE * 16, v);
            float xr[M], xi[M];
#pragma unroll
            for (int j = 0; j < PIECES; ++j) xr[2 * j] = v[j].x, xi[2 * j] = v[j].y, xr[2 * j + 1] = v[j].z, xi[2 * j + 1] = v[j].w;
            const int tl = 4 * step_of(n) + q;
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                float yr, yi;
                demix_one<M>(wr[kk], wi[kk], xr, xi, yr, yi);
                float pw = fmaf(yr, yr, yi * yi);
                pw = fvalid ? pw : 0.f;
                pw = row16_sum(pw);
                if (b == 0 && tl < len) lds_store(sp, (wave * tcp + tl) * KP + kk, pw);
            }
        };
        static_assert(kPowStages == 2, "the loop is unrolled over the stages by hand");
        // Step 0 of X and W travel together and are waited for ONCE, in front of the loop: with loads of registers still counted
        // at the head of the loop hipcc drains the queue there, every step's requests included, so W must have arrived before the
        // loop -- but not before the first request leaves.  The queue is empty behind the wait: consume(0)'s counted wait finds
        // step 0 landed and only step 1 outstanding.  The register fence keeps every use of W behind the wait.
        if constexpr (kRawW) {
            issue(0, 0);
            load_w_raw<M, KP>(What, fc, k0, K, wraw);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            finish_wconj<M, KP>(wraw, k0, K, wr, wi);
        } else {
            load_wconj<M, KP>(What, fc, k0, K, wr, wi);
        }
#pragma unroll
        for (int kk = 0; kk < KP; ++kk)
#pragma unroll
            for (int m = 0; m < M; ++m) asm volatile("" : "+v"(wr[kk][m]), "+v"(wi[kk][m]));
        if constexpr (!kRawW) issue(0, 0);
        int n = 0;
        for (; n + 2 <= nsteps; n += 2) {       // stage indices are compile-time constants in the unrolled body
            issue(n + 1, 1); consume(n, 0);
            issue(n + 2, 0); consume(n + 1, 1);
        }
        if (n < nsteps) { issue(n + 1, 1); consume(n, 0); }
        lds_stores_done();
    } else {
        // kPowUnroll steps are loaded before any of them is consumed: a wave keeps kPowUnroll * 64 * M * 8
        // bytes in flight, which is what hides HBM latency here (more resident waves only thrash the L1,
        // because a lane's M*8 bytes arrive through M/2 separate dwordx4 requests to the same lines).
        if constexpr (kRawW) {
            load_w_raw<M, KP>(What, fc, k0, K, wraw);
            finish_wconj<M, KP>(wraw, k0, K, wr, wi);
        } else {
            load_wconj<M, KP>(What, fc, k0, K, wr, wi);
        }
        for (int g = 0; g < ngroups; ++g) {
            const int i = (rev ? ngroups - 1 - g : g) * kPowUnroll;
            float xr[kPowUnroll][M], xi[kPowUnroll][M];
#pragma unroll
            for (int u = 0; u < kPowUnroll; ++u) {
                const int tl = 4 * (i + u) + q;
                const int t = tl < len ? t_begin + tl : T - 1;      // clamped: legal address, result unused
                load_x<M>(pbase + (size_t)t * frame_stride, xr[u], xi[u]);
            }
#pragma unroll
            for (int u = 0; u < kPowUnroll; ++u) {
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
    }
    __syncthreads();
    for (int e = tid; e < len * KP; e += kBlock) {
        const int tl = e / KP, kk = e - tl * KP;
        float s = sp[(0 * tcp + tl) * KP + kk];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += sp[(w * tcp + tl) * KP + kk];
        if (k0 + kk < K) Ppart[((size_t)blockIdx.x * T + t_begin + tl) * K + k0 + kk] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// stats: same lane geometry as the covariance pass (16 bins per block, 16 frame phases);
//        per (bin, source): num = sum_t conj(x_0) y,  den = sum_t |y|^2
// ---------------------------------------------------------------------------------------------
template <int M, int KP>
__global__ __launch_bounds__(kBlock) void stats_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                       float* __restrict__ Spart, int T, int F, int K, int tc) {
    __shared__ float lds[3 * KP * (kBlock + 1)];
    const int tid = threadIdx.x;
    const int b = tid & 15;
    const int q = tid >> 4;
    const int f = blockIdx.x * kBinsPerWave + b;
    const int fc = f < F ? f : F - 1;
    const int k0 = blockIdx.z * KP;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const int nsteps = (t_end - t_begin + 15) >> 4;

    float wr[KP][M], wi[KP][M];
    load_wconj<M, KP>(What, fc, k0, K, wr, wi);
    float nr[KP], ni[KP], dn[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) nr[kk] = ni[kk] = dn[kk] = 0.f;

    const size_t frame_stride = (size_t)F * M;
    const float2* px = X + ((size_t)(t_begin + q) * F + fc) * M;
    for (int i = 0; i < nsteps; ++i) {
        const int t = t_begin + q + 16 * i;
        if (t < t_end) {
            float xr[M], xi[M];
            load_x<M>(px, xr, xi);
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                float yr, yi;
                demix_one<M>(wr[kk], wi[kk], xr, xi, yr, yi);
                // conj(x0) * y
                nr[kk] = fmaf(xr[0], yr, fmaf(xi[0], yi, nr[kk]));
                ni[kk] = fmaf(xr[0], yi, fmaf(-xi[0], yr, ni[kk]));
                dn[kk] = fmaf(yr, yr, fmaf(yi, yi, dn[kk]));
            }
        }
        px += 16 * frame_stride;
    }
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
        lds[(3 * kk + 0) * (kBlock + 1) + tid] = nr[kk];
        lds[(3 * kk + 1) * (kBlock + 1) + tid] = ni[kk];
        lds[(3 * kk + 2) * (kBlock + 1) + tid] = dn[kk];
    }
    __syncthreads();
    // thread e -> (bin bb, value v): sum the 16 phases
    for (int e = tid; e < 16 * 3 * KP; e += kBlock) {
        const int bb = e / (3 * KP), v = e - bb * (3 * KP);
        float s = 0.f;
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) s += lds[v * (kBlock + 1) + qq * 16 + bb];
        const int fo = blockIdx.x * kBinsPerWave + bb;
        const int kk = v / 3, c = v - 3 * kk;
        if (fo < F && k0 + kk < K) Spart[(((size_t)blockIdx.y * F + fo) * K + k0 + kk) * 3 + c] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// write: Y (T, F, K) complex64; z from the stats partials when projecting back
// ---------------------------------------------------------------------------------------------
template <int M, int KP>
__global__ __launch_bounds__(kBlock) void write_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                       const float* __restrict__ Spart, int nsplit,
                                                       float2* __restrict__ Y, int T, int F, int K, int tc) {
    const int tid = threadIdx.x;
    const int b = tid & 15;
    const int q = tid >> 4;
    const int f = blockIdx.x * kBinsPerWave + b;
    if (f >= F) return;
    const int k0 = blockIdx.z * KP;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);

    float wr[KP][M], wi[KP][M];
    load_wconj<M, KP>(What, f, k0, K, wr, wi);
    // fold conj(z) into the demixing vector: y*conj(z) = (conj(z) w^H) x
    if (Spart != nullptr) {
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) {
            if (k0 + kk < K) {
                double sr = 0., si = 0., sd = 0.;
                for (int s = 0; s < nsplit; ++s) {
                    const float* p = Spart + (((size_t)s * F + f) * K + k0 + kk) * 3;
                    sr += p[0];
                    si += p[1];
                    sd += p[2];
                }
                float zr = 1.f, zi = 0.f;
                if (sd > 0.) {
                    zr = (float)(sr / sd);
                    zi = (float)(si / sd);
                }
                // multiply conj(w) (held as wr + i wi) by conj(z) = zr - i zi
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float a = wr[kk][m], c = wi[kk][m];
                    wr[kk][m] = a * zr + c * zi;
                    wi[kk][m] = c * zr - a * zi;
                }
            }
        }
    }
    const size_t frame_stride = (size_t)F * M;
    const float2* px = X + ((size_t)(t_begin + q) * F + f) * M;
    for (int t = t_begin + q; t < t_end; t += 16) {
        float xr[M], xi[M];
        load_x<M>(px, xr, xi);
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) {
            float yr, yi;
            demix_one<M>(wr[kk], wi[kk], xr, xi, yr, yi);
            if (k0 + kk < K) Y[((size_t)t * F + f) * K + k0 + kk] = make_float2(yr, yi);
        }
        px += 16 * frame_stride;
    }
}

template <int M, int KP>
hipError_t launch_power_one(hipStream_t s, const float2* X, const float2* What, float* Ppart, int T, int F, int K,
                            const PowGeom& g) {
    if constexpr (!pow_kp_reachable(M, KP)) return hipErrorInvalidValue;      // (more sources per pass than channels: never asked for)
    dim3 grid(g.nb, g.nsplit, (K + KP - 1) / KP);
    const size_t shmem = (size_t)kWaves * g.tcp * KP * sizeof(float);
    // (the streamed form: X streams only behind the lane covariance kernel, which 8 channels take with one or two sources --
    //  choose_cov_kind, choose_x_policy)
    if constexpr (M == 8 && KP <= 2) {
        if (g.xplain < kXPeriod) {
            if (g.xctc < g.tcp || g.xctc % kXGroup != 0) return hipErrorInvalidValue;      // (choose_x_policy never asks for it)
            hipLaunchKernelGGL((power_kernel<M, KP, true>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, g.tcp, g.rev, g.ord, g.xplain, g.xctc);
            return hipGetLastError();
        }
    }
    if constexpr (pow_kp_reachable(M, KP)) {
        hipLaunchKernelGGL((power_kernel<M, KP, false>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, g.tcp, g.rev, g.ord, kXPeriod, 0);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

template <int M, int KP>
hipError_t pow_occupancy_one(int* n, size_t shmem) {
    if constexpr (pow_kp_reachable(M, KP)) return hipOccupancyMaxActiveBlocksPerMultiprocessor(n, power_kernel<M, KP>, kBlock, shmem);
    return hipErrorInvalidValue;
}

template <int M, int KP>
hipError_t launch_stats_one(hipStream_t s, const float2* X, const float2* What, float* Spart, int T, int F, int K,
                            const CovGeom& g) {
    dim3 grid(g.nbg, g.nsplit, (K + KP - 1) / KP);
    hipLaunchKernelGGL((stats_kernel<M, KP>), grid, dim3(kBlock), 0, s, X, What, Spart, T, F, K, g.tc);
    return hipGetLastError();
}

template <int M, int KP>
hipError_t launch_write_one(hipStream_t s, const float2* X, const float2* What, const float* Spart, int nsplit,
                            float2* Y, int T, int F, int K) {
    const int tc = 256;
    dim3 grid((F + kBinsPerWave - 1) / kBinsPerWave, (T + tc - 1) / tc, (K + KP - 1) / KP);
    hipLaunchKernelGGL((write_kernel<M, KP>), grid, dim3(kBlock), 0, s, X, What, Spart, nsplit, Y, T, F, K, tc);
    return hipGetLastError();
}

// dispatch (M, KP) -> instantiation.  KP in {1, 2, 4}.
#define OIVA_DISPATCH_M(CALL)            \
    switch (M) {                         \
        case 1: CALL(1); break;          \
        case 2: CALL(2); break;          \
        case 3: CALL(3); break;          \
        case 4: CALL(4); break;          \
        case 5: CALL(5); break;          \
        case 6: CALL(6); break;          \
        case 7: CALL(7); break;          \
        case 8: CALL(8); break;          \
        case 9: CALL(9); break;          \
        case 10: CALL(10); break;        \
        case 11: CALL(11); break;        \
        case 12: CALL(12); break;        \
        case 13: CALL(13); break;        \
        case 14: CALL(14); break;        \
        case 15: CALL(15); break;        \
        case 16: CALL(16); break;        \
    }

}  // namespace

hipError_t pow_blocks_per_cu(int M, int kp, int tcp, int* n) {
    const size_t shmem = (size_t)kWaves * tcp * kp * sizeof(float);
#define CALL(MM)                                                                                                   \
    if (kp == 1) return pow_occupancy_one<MM, 1>(n, shmem);       \
    if (kp == 2) return pow_occupancy_one<MM, 2>(n, shmem);       \
    if (kp == 4) return pow_occupancy_one<MM, 4>(n, shmem);
    OIVA_DISPATCH_M(CALL)
#undef CALL
    return hipErrorInvalidValue;
}

hipError_t launch_power(hipStream_t s, const float2* X, const float2* Xpad, const float2* What, float* Ppart, int T, int F, int M,
                        int K, const PowGeom& g) {
    if (!traits(g.kind).supported(M, K)) return hipErrorInvalidValue;
    switch (g.kind) {
        case PowKind::Wide: return launch_power_wide(s, X, What, Ppart, T, F, M, K, g);
        case PowKind::Mfma: return Xpad ? launch_power_mfma(s, Xpad, What, Ppart, T, F, M, M + 1, K) : launch_power_mfma(s, X, What, Ppart, T, F, M, M, K);
        case PowKind::Lds: return launch_power_lds(s, X, What, Ppart, T, F, M, K);
        case PowKind::Lane: break;
    }
#define CALL(MM)                                                                                        \
    if (g.kp == 1) return launch_power_one<MM, 1>(s, X, What, Ppart, T, F, K, g);                       \
    if (g.kp == 2) return launch_power_one<MM, 2>(s, X, What, Ppart, T, F, K, g);                       \
    if (g.kp == 4) return launch_power_one<MM, 4>(s, X, What, Ppart, T, F, K, g);
    OIVA_DISPATCH_M(CALL)
#undef CALL
    return hipErrorInvalidValue;
}

hipError_t launch_demix_stats(hipStream_t s, const float2* X, const float2* What, float* Spart, int T, int F, int M,
                              int K, const CovGeom& g) {
    if (M > kNarrowMax) return launch_demix_stats_wide(s, X, What, Spart, T, F, M, K, g);
#define CALL(MM) return launch_stats_one<MM, 2>(s, X, What, Spart, T, F, K, g);
    OIVA_DISPATCH_M(CALL)
#undef CALL
    return hipErrorInvalidValue;
}

hipError_t launch_demix_write(hipStream_t s, const float2* X, const float2* What, const float* Spart, int nsplit,
                              float2* Y, int T, int F, int M, int K) {
    if (M > kNarrowMax) return launch_demix_write_wide(s, X, What, Spart, nsplit, Y, T, F, M, K);
#define CALL(MM) return launch_write_one<MM, 2>(s, X, What, Spart, nsplit, Y, T, F, K);
    OIVA_DISPATCH_M(CALL)
#undef CALL
    return hipErrorInvalidValue;
}

}  // namespace oiva
