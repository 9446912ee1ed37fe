// Kernels of the complex128 data path of the batched solver (oiva_batch_set_data_c128, batch.hip): X is held as the
// caller's complex128 and every stage runs in float64.  One set, reading the problem table, serves oiva_batch_create and
// oiva_batch_create_ragged.
//
//   X      (sum T_b, F, M) complex128, packed: problem b holds frames [x_off_b, x_off_b + T_b)
//   What64 (B*F, M, M) complex128, element [m][s] = W[f, m, s]; What its complex64 copy (kept for get_w's consumers)
//   Ppart  problem b's [parts][T_b][K] float64 at p_off_b: |y|^2 added over the 64 bins of a part
//   Rw     (sum T_b, K) float64: r after the activation, the weights 1 / max(r / gamma, eps) after the finalize launch
//   Gs     [B][rblocks][K] float64: the sums of r over blocks of kBlock frames, from which gamma follows
//   Vpart  [max nsplit][B*F][K][M*M] packed Hermitian partials, as the complex64 batch's: read by launch_update
//   Z      (B*F, K) complex128: the projection-back scales
//
// Orders of summation (functions of (bin, frame) within the room and of its T and F alone): the channels of a demix in ascending
// order as one FMA chain; the 64 bins of a part by the fixed butterfly over the lanes; the parts in order; r over blocks of
// kBlock frames by block_sum, the blocks in order; a covariance over a split's frames in order, the splits in order (sum_vpart);
// the projection-back sums lane-strided over the frames, closed by the butterfly.
#include <algorithm>

#include "oiva_device.h"

namespace oiva {
namespace {

constexpr double kEpsR64 = 1e-15;      // reference overiva.py:170, as the float64 the reference compares with
constexpr int kPartBins = 64;          // bins per part of the power pass: one per lane
constexpr int kPowFrames = 32;         // frames per workgroup of the power pass
constexpr int kPowSources = 4;         // sources whose columns of W a lane holds at a time
constexpr int kCovBins = 16;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int M>
__device__ __forceinline__ void load_x128(const double2* __restrict__ p, double (&xr)[M], double (&xi)[M]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double2 v = p[m];
        xr[m] = v.x;
        xi[m] = v.y;
    }
}

// y = sum_m x_m conj(w_m), the channels in ascending order (ilrma_power_kernel's chain)
template <int M>
__device__ __forceinline__ void demix128(const double (&xr)[M], const double (&xi)[M], const double (&wr)[M], const double (&wi)[M],
                                         double& yr, double& yi) {
    yr = 0.;
    yi = 0.;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        yr = fma(xr[m], wr[m], yr);
        yr = fma(xi[m], wi[m], yr);
        yi = fma(xi[m], wr[m], yi);
        yi = fma(-xr[m], wi[m], yi);
    }
}

// ---------------------------------------------------------------------------------------------
// demix + power, overiva.py:140 and the norms at :153/:155.  Workgroup = one 64-bin part x kPowFrames frames of one problem
// (grid = parts x frame tiles of the longest problem x problems); lane = bin, a wave takes every fourth frame of the tile.  A
// lane holds kPowSources columns of its bin's W; |y|^2 of the 64 bins is closed by the butterfly and lane 0 stores it.
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kBlock) void c128_power_kernel(const double2* __restrict__ X, const double2* __restrict__ What64,
                                                            double* __restrict__ Ppart, const RaggedProblem* __restrict__ probs, int F,
                                                            int K) {
    const int prob = blockIdx.z;
    const RaggedProblem d = probs[prob];
    const int t0 = blockIdx.y * kPowFrames;
    if (t0 >= d.T) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * kPartBins + lane;
    const bool live = f < F;
    const int fc = live ? f : F - 1;                  // lanes past F read the last bin and add 0.
    const double2* Xb = X + d.x_off * F * M;
    const double2* Wb = What64 + ((size_t)prob * F + fc) * M * M;
    double* Pb = Ppart + d.p_off + (size_t)blockIdx.x * d.T * K;
    const int t_end = min(d.T, t0 + kPowFrames);
    for (int k0 = 0; k0 < K; k0 += kPowSources) {
        double wr[kPowSources][M], wi[kPowSources][M];
#pragma unroll
        for (int kk = 0; kk < kPowSources; ++kk) {
            const int s = min(k0 + kk, K - 1);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double2 w = Wb[m * M + s];
                wr[kk][m] = w.x;
                wi[kk][m] = w.y;
            }
        }
        for (int t = t0 + wave; t < t_end; t += kWaves) {
            double xr[M], xi[M];
            load_x128<M>(Xb + ((size_t)t * F + fc) * M, xr, xi);
#pragma unroll
            for (int kk = 0; kk < kPowSources; ++kk) {
                if (k0 + kk < K) {                    // (uniform)
                    double yr, yi;
                    demix128<M>(xr, xi, wr[kk], wi[kk], yr, yi);
                    const double p = wave_sum(live ? fma(yr, yr, yi * yi) : 0.);
                    if (lane == 0) Pb[(size_t)t * K + k0 + kk] = p;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// activation, overiva.py:152-155: the parts in order, r = 2 sqrt(p) | p / F, and the sum of r over this block of kBlock frames
// (grid = blocks of frames of the longest problem x sources x problems)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void c128_activation_kernel(const double* __restrict__ Ppart, int nparts, double* __restrict__ Rw,
                                                                 double* __restrict__ Gs, const RaggedProblem* __restrict__ probs, int K,
                                                                 int model, int F, int rblocks) {
    __shared__ double wsum[kWaves];
    const int prob = blockIdx.z;
    const RaggedProblem d = probs[prob];
    if ((int)blockIdx.x >= rsum_blocks(d.T)) return;
    const int t = blockIdx.x * kBlock + threadIdx.x, k = blockIdx.y;
    double r = 0.;
    if (t < d.T) {
        const double* Pb = Ppart + d.p_off + (size_t)t * K + k;
        double p = 0.;
        for (int i = 0; i < nparts; ++i) p += Pb[(size_t)i * d.T * K];
        r = model == OIVA_MODEL_LAPLACE ? 2. * sqrt(p) : p / (double)F;
        Rw[(d.x_off + t) * K + k] = r;
    }
    const double s = block_sum(r, wsum);              // frames past T add 0.
    if (threadIdx.x == 0) Gs[((size_t)prob * rblocks + blockIdx.x) * K + k] = s;
}

// ---------------------------------------------------------------------------------------------
// gamma = mean_t r (overiva.py:158) from the block sums in order; r <- 1 / max(r / gamma, eps) in place (:159, :170-173, a NaN
// stays NaN); columns 0..K-1 of W divided by gamma | sqrt(gamma) (:161-167) in float64, so that the shared per-bin update runs
// without a pending scale (grid = blocks of max(T K, F M K) elements of the largest problem x problems)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void c128_finalize_kernel(double* __restrict__ Rw, const double* __restrict__ Gs,
                                                               double2* __restrict__ What64, float2* __restrict__ What,
                                                               const RaggedProblem* __restrict__ probs, int F, int M, int K, int model,
                                                               int rblocks) {
    __shared__ double gam[8];
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    if ((int)threadIdx.x < K) {
        const int nblk = rsum_blocks(d.T);
        double s = 0.;
        for (int b = 0; b < nblk; ++b) s += Gs[((size_t)prob * rblocks + b) * K + threadIdx.x];
        gam[threadIdx.x] = s / (double)d.T;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < (long long)d.T * K) {
        const int k = (int)(i % K);
        double* p = Rw + d.x_off * K + i;
        double rn = *p / gam[k];
        rn = rn < kEpsR64 ? kEpsR64 : rn;
        *p = 1. / rn;
    }
    if (i < (long long)F * M * K) {
        const int f = (int)(i / (M * K));
        const int rem = (int)(i - (long long)f * M * K);
        const int m = rem / K, k = rem - m * K;
        const size_t idx = ((size_t)prob * F + f) * M * M + (size_t)m * M + k;
        const double sc = model == OIVA_MODEL_LAPLACE ? gam[k] : sqrt(gam[k]);
        double2 w = What64[idx];
        w.x /= sc;
        w.y /= sc;
        What64[idx] = w;
        What[idx] = make_float2((float)w.x, (float)w.y);
    }
}

// ---------------------------------------------------------------------------------------------
// weighted covariance, overiva.py:179, and with UNIT the input covariance (:87, K = 1, w = 1): batch_cov_block's items -- thread
// = (bin, entry c <= d of the Hermitian half) holding the sums of all sources, one product serving them all -- on double2 X staged
// in LDS in chunks of CH frames (32 up to 4 channels, 16 from 5 on: 32 KB; the chunk length enters no sum).  Workgroup = 16 bins
// x one frame split of one problem (grid = bin groups x splits of the longest problem x problems).
// ---------------------------------------------------------------------------------------------
template <int M, bool UNIT>
__global__ __launch_bounds__(kBlock) void c128_cov_kernel(const double2* __restrict__ X, const double* __restrict__ Wt,
                                                          const RaggedProblem* __restrict__ probs, double* __restrict__ Vpart, int F, int K,
                                                          int nbins_all) {
    constexpr int CH = M <= 4 ? 32 : 16;
    constexpr int E = M * (M + 1) / 2;
    constexpr int NI = (kCovBins * E + kBlock - 1) / kBlock;
    constexpr int KM = UNIT ? 1 : M;
    __shared__ double2 xs[CH][kCovBins][M];
    __shared__ double ws[CH][KM];

    const int prob = blockIdx.z;
    const RaggedProblem d = probs[prob];
    if ((int)blockIdx.y >= d.nsplit) return;
    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * kCovBins;
    const int t_begin = blockIdx.y * d.tc;
    const int t_end = min(d.T, t_begin + d.tc);
    const double2* Xb = X + d.x_off * F * M;
    const double* Wb = UNIT ? nullptr : Wt + d.x_off * K;
    const int nk = UNIT ? 1 : K;

    int ib[NI], ic[NI], id[NI];
    bool iv[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int it = tid + j * kBlock;
        iv[j] = it < kCovBins * E;
        const int itc = iv[j] ? it : 0;
        ib[j] = itc / E;
        int e = itc - ib[j] * E, c = 0;
        while (e >= M - c) {
            e -= M - c;
            ++c;
        }
        ic[j] = c;
        id[j] = c + e;
    }
    double ar[NI][KM], ai[NI][KM];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int k = 0; k < KM; ++k) ar[j][k] = ai[j][k] = 0.;

    for (int tc0 = t_begin; tc0 < t_end; tc0 += CH) {
        const int len = min(CH, t_end - tc0);
        __syncthreads();
        for (int i = tid; i < len * kCovBins * M; i += kBlock) {
            const int tl = i / (kCovBins * M);
            const int r = i - tl * (kCovBins * M);
            const int f = f0 + r / M;
            xs[tl][r / M][r % M] = f < F ? Xb[((size_t)(tc0 + tl) * F + f0) * M + r] : make_double2(0., 0.);
        }
        if constexpr (!UNIT) {
            for (int i = tid; i < len * KM; i += kBlock) {
                const int tl = i / KM, k = i - tl * KM;
                ws[tl][k] = k < K ? Wb[(size_t)(tc0 + tl) * K + k] : 0.;
            }
        }
        __syncthreads();
        for (int tl = 0; tl < len; ++tl) {
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const double2 xc = xs[tl][ib[j]][ic[j]];
                const double2 xd = xs[tl][ib[j]][id[j]];
                const double pre = fma(xc.x, xd.x, xc.y * xd.y);       // x_c conj(x_d)
                const double pim = fma(xc.y, xd.x, -(xc.x * xd.y));
#pragma unroll
                for (int k = 0; k < KM; ++k) {
                    if (k < nk) {
                        const double w = UNIT ? 1. : ws[tl][k];
                        ar[j][k] = fma(w, pre, ar[j][k]);
                        ai[j][k] = fma(w, pim, ai[j][k]);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int f = f0 + ib[j];
        if (!iv[j] || f >= F) continue;
        double* out = Vpart + ((size_t)blockIdx.y * nbins_all + (size_t)prob * F + f) * nk * M * M;
        const int c = ic[j], dd = id[j];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k < nk) {
                if (c == dd) {
                    out[(size_t)k * M * M + c] = ar[j][k];
                } else {
                    const int a = herm_pair_index(M, c, dd);
                    out[(size_t)k * M * M + a] = ar[j][k];
                    out[(size_t)k * M * M + a + 1] = ai[j][k];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// projection back (oracle.projection_back, no clipping): z[f,k] = sum_t conj(x[t,f,0]) y[t,f,k] / sum_t |y[t,f,k]|^2, 1 where the
// denominator is 0.  One wave per (problem, bin) (grid = groups of 4 bins x problems): the lanes stride over the frames, the
// bin's W is broadcast from LDS, the butterfly closes the three sums of every source.
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kBlock) void c128_projback_kernel(const double2* __restrict__ X, const double2* __restrict__ What64,
                                                               double2* __restrict__ Z, const RaggedProblem* __restrict__ probs, int F,
                                                               int K) {
    __shared__ double2 wsm[kWaves][M * M];
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * kWaves + wave;
    const int fc = f < F ? f : F - 1;
    for (int i = lane; i < M * M; i += 64) wsm[wave][i] = What64[((size_t)prob * F + fc) * M * M + i];
    __syncthreads();
    const double2* Xb = X + d.x_off * F * M;
    double nr[M], ni[M], dn[M];
#pragma unroll
    for (int s = 0; s < M; ++s) nr[s] = ni[s] = dn[s] = 0.;
    for (int t = lane; t < d.T; t += 64) {
        double xr[M], xi[M];
        load_x128<M>(Xb + ((size_t)t * F + fc) * M, xr, xi);
#pragma unroll
        for (int s = 0; s < M; ++s) {
            if (s < K) {
                double wr[M], wi[M];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double2 w = wsm[wave][m * M + s];
                    wr[m] = w.x;
                    wi[m] = w.y;
                }
                double yr, yi;
                demix128<M>(xr, xi, wr, wi, yr, yi);
                nr[s] += fma(xr[0], yr, xi[0] * yi);           // conj(ref) y
                ni[s] += fma(xr[0], yi, -(xi[0] * yr));
                dn[s] += fma(yr, yr, yi * yi);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < M; ++s) {
        if (s < K) {
            const double a = wave_sum(nr[s]), b = wave_sum(ni[s]), c = wave_sum(dn[s]);
            if (lane == 0 && f < F) Z[((size_t)prob * F + f) * K + s] = c > 0. ? make_double2(a / c, b / c) : make_double2(1., 0.);
        }
    }
}

// Y[t,f,k] = sum_m x[t,f,m] conj(W[f,m,k]) (overiva.py:192), times conj(z[f,k]) when Z is given (:197-199); thread = (frame, bin)
// (grid = blocks of T F elements of the longest problem x problems)
template <int M>
__global__ __launch_bounds__(kBlock) void c128_demix_kernel(const double2* __restrict__ X, const double2* __restrict__ What64,
                                                            const double2* __restrict__ Z, double2* __restrict__ Y,
                                                            const RaggedProblem* __restrict__ probs, int F, int K) {
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)d.T * F) return;
    const int t = (int)(i / F), f = (int)(i - (long long)t * F);
    double xr[M], xi[M];
    load_x128<M>(X + ((d.x_off + t) * F + f) * M, xr, xi);
    const double2* Wb = What64 + ((size_t)prob * F + f) * M * M;
    double2* Yb = Y + ((d.x_off + t) * F + f) * K;
    for (int s = 0; s < K; ++s) {
        double wr[M], wi[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double2 w = Wb[m * M + s];
            wr[m] = w.x;
            wi[m] = w.y;
        }
        double yr, yi;
        demix128<M>(xr, xi, wr, wi, yr, yi);
        if (Z != nullptr) {
            const double2 z = Z[((size_t)prob * F + f) * K + s];
            const double pr = fma(yr, z.x, yi * z.y);          // y conj(z)
            const double pi = fma(yi, z.x, -(yr * z.y));
            yr = pr;
            yi = pi;
        }
        Yb[s] = make_double2(yr, yi);
    }
}

#define OIVA_C128_DISPATCH_M(CALL) \
    switch (M) {                   \
        case 1: CALL(1); break;    \
        case 2: CALL(2); break;    \
        case 3: CALL(3); break;    \
        case 4: CALL(4); break;    \
        case 5: CALL(5); break;    \
        case 6: CALL(6); break;    \
        case 7: CALL(7); break;    \
        case 8: CALL(8); break;    \
    }

unsigned blocks_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

int c128_parts(int F) { return (F + kPartBins - 1) / kPartBins; }

hipError_t launch_c128_power(hipStream_t s, const double2* X, const double2* What64, double* Ppart, const RaggedProblem* prob, int B,
                             int max_T, int F, int M, int K) {
    const dim3 grid((unsigned)c128_parts(F), (unsigned)((max_T + kPowFrames - 1) / kPowFrames), (unsigned)B);
    if (M < 1 || M > 8) return hipErrorInvalidValue;
#define CALL(MM) hipLaunchKernelGGL(c128_power_kernel<MM>, grid, dim3(kBlock), 0, s, X, What64, Ppart, prob, F, K)
    OIVA_C128_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_c128_activation(hipStream_t s, const double* Ppart, double* Rw, double* Gs, double2* What64, float2* What,
                                  const RaggedProblem* prob, int B, int max_T, int F, int M, int K, int model, int rblocks) {
    hipLaunchKernelGGL(c128_activation_kernel, dim3((unsigned)rblocks, (unsigned)K, (unsigned)B), dim3(kBlock), 0, s, Ppart, c128_parts(F),
                       Rw, Gs, prob, K, model, F, rblocks);
    const long long n = std::max((long long)max_T * K, (long long)F * M * K);
    hipLaunchKernelGGL(c128_finalize_kernel, dim3(blocks_of(n), (unsigned)B), dim3(kBlock), 0, s, Rw, Gs, What64, What, prob, F, M, K,
                       model, rblocks);
    return hipGetLastError();
}

hipError_t launch_c128_cov(hipStream_t s, const double2* X, const double* Wt, const RaggedProblem* prob, double* Vpart, int B, int F,
                           int M, int K, int max_nsplit) {
    const dim3 grid((unsigned)((F + kCovBins - 1) / kCovBins), (unsigned)max_nsplit, (unsigned)B);
    const int nbins_all = B * F;
    if (M < 1 || M > 8) return hipErrorInvalidValue;
#define CALL(MM)                                                                                                          \
    if (Wt == nullptr)                                                                                                    \
        hipLaunchKernelGGL((c128_cov_kernel<MM, true>), grid, dim3(kBlock), 0, s, X, Wt, prob, Vpart, F, 1, nbins_all);   \
    else                                                                                                                  \
        hipLaunchKernelGGL((c128_cov_kernel<MM, false>), grid, dim3(kBlock), 0, s, X, Wt, prob, Vpart, F, K, nbins_all);
    OIVA_C128_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_c128_demix(hipStream_t s, const double2* X, const double2* What64, double2* Z, double2* Y, const RaggedProblem* prob,
                             int B, int max_T, int F, int M, int K, bool proj_back) {
    if (M < 1 || M > 8) return hipErrorInvalidValue;
    const dim3 pgrid((unsigned)((F + kWaves - 1) / kWaves), (unsigned)B);
    const dim3 grid(blocks_of((long long)max_T * F), (unsigned)B);
    const double2* Zr = proj_back ? Z : nullptr;
#define CALL(MM)                                                                                                         \
    if (proj_back) hipLaunchKernelGGL(c128_projback_kernel<MM>, pgrid, dim3(kBlock), 0, s, X, What64, Z, prob, F, K);    \
    hipLaunchKernelGGL(c128_demix_kernel<MM>, grid, dim3(kBlock), 0, s, X, What64, Zr, Y, prob, F, K)
    OIVA_C128_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

}  // namespace oiva
