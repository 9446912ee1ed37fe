// Weighted covariance of one workgroup of the batched passes (batch_cov_kernel, kernels_batch.hip; ragged_cov_kernel,
// kernels_ragged.hip): one body, so that a problem of a ragged batch sums exactly as the dense batch sums it.
#pragma once
#include "oiva_device.h"

namespace oiva {

// ---------------------------------------------------------------------------------------------
// weighted covariance, float64 (the `precise` arithmetic): V_k[f] = sum_t w[t,k] x_{t,f} x_{t,f}^H, overiva.py:179, as
// float64 sums of exact float64 products; with UNIT the input covariance (overiva.py:87, K = 1, w = 1).
// Workgroup = 16 bins (grid.x) of problem `prob` x one frame split (grid.y); the problem's (T, F, M) X starts at frame x_frame0
// of X, its activation buffer at float r_off of R (unused with UNIT); wscale: (B, K), written at grid.x = grid.y = 0.  Chunks of
// kBatchChunk frames of the 16 bins are staged in LDS with their weights; thread = (bin, entry c <= d of the Hermitian
// half) -- up to NI of them --, holding the sums of ALL sources, so one product x_c conj(x_d) serves every source.  A sum runs over the split's frames in order; the partial of every split is
// stored packed (herm_pair_index) and the update adds the splits in order (sum_vpart).
// ---------------------------------------------------------------------------------------------
constexpr int kBatchChunk = 32;
constexpr int kBatchBins = 16;

template <int M, bool UNIT>
__device__ __forceinline__ void batch_cov_block(const float2* __restrict__ X, size_t x_frame0, const float* __restrict__ R, size_t r_off,
                                                float* __restrict__ wscale, int model, double* __restrict__ Vpart, int T, int F, int K,
                                                int tc, int nbins_all, int prob) {
    constexpr int E = M * (M + 1) / 2;                           // entries of the Hermitian half
    constexpr int NI = (kBatchBins * E + kBlock - 1) / kBlock;   // (bin, entry) items per thread
    constexpr int KM = UNIT ? 1 : M;                             // sources held (K <= M)
    __shared__ float2 xs[kBatchChunk][kBatchBins][M];
    __shared__ double ws[kBatchChunk][KM];

    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * kBatchBins;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const float2* Xb = X + x_frame0 * F * M;
    const float* Rb = UNIT ? nullptr : R + r_off;
    const int nk = UNIT ? 1 : K;

    // scale normalisation of the activations (overiva.py:158-159), as cov_kernel's float64 form: thread k forms 1/gamma_k
    __shared__ double ginv[KM];
    if constexpr (!UNIT) {
        if (tid < K) {
            const double gamma = gamma_of(Rb, T, K, tid);
            ginv[tid] = 1. / gamma;
            if (blockIdx.x == 0 && blockIdx.y == 0)
                wscale[(size_t)prob * K + tid] = model == OIVA_MODEL_LAPLACE ? (float)gamma : (float)sqrt(gamma);   // overiva.py:163 / :167
        }
    }

    // this thread's items: bin bb[j], channels c[j] <= d[j]
    int ib[NI], ic[NI], id[NI];
    bool iv[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int it = tid + j * kBlock;
        iv[j] = it < kBatchBins * E;
        const int itc = iv[j] ? it : 0;
        ib[j] = itc / E;
        int e = itc - ib[j] * E, c = 0;
        while (e >= M - c) {         // row c of the half holds M - c entries (c, c..M-1)
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

    for (int tc0 = t_begin; tc0 < t_end; tc0 += kBatchChunk) {
        const int len = min(kBatchChunk, t_end - tc0);
        __syncthreads();      // (also orders the first chunk behind ginv)
        // stage the chunk: frame t holds the 16 bins' M channels contiguously; bins past F are zeros
        for (int i = tid; i < len * kBatchBins * M; i += kBlock) {
            const int tl = i / (kBatchBins * M);
            const int r = i - tl * (kBatchBins * M);
            const int f = f0 + r / M;
            xs[tl][r / M][r % M] = f < F ? Xb[((size_t)(tc0 + tl) * F + f0) * M + r] : make_float2(0.f, 0.f);
        }
        if constexpr (!UNIT) {
            for (int i = tid; i < len * KM; i += kBlock) {
                const int tl = i / KM, k = i - tl * KM;
                double w = 0.;
                if (k < K) {
                    double rn = (double)Rb[(size_t)(tc0 + tl) * K + k] * ginv[k];
                    rn = rn < (double)kEpsR ? (double)kEpsR : rn;     // a NaN stays NaN, like r[r < eps] = eps
                    w = 1. / rn;
                }
                ws[tl][k] = w;
            }
        }
        __syncthreads();
        for (int tl = 0; tl < len; ++tl) {
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const float2 xc = xs[tl][ib[j]][ic[j]];
                const float2 xd = xs[tl][ib[j]][id[j]];
                // x_c conj(x_d): exact float64 products of float32 data, summed as accumulate() (cov_arith.h) does
                const double pre = fma((double)xc.x, (double)xd.x, (double)xc.y * (double)xd.y);
                const double pim = fma((double)xc.y, (double)xd.x, -((double)xc.x * (double)xd.y));
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

    // packed partial of this split: [split][prob * F + f][k][M*M]
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int f = f0 + ib[j];
        if (!iv[j] || f >= F) continue;
        double* out = Vpart + ((size_t)blockIdx.y * nbins_all + (size_t)prob * F + f) * nk * M * M;
        const int c = ic[j], d = id[j];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k < nk) {
                if (c == d) {
                    out[(size_t)k * M * M + c] = ar[j][k];
                } else {
                    const int a = herm_pair_index(M, c, d);
                    out[(size_t)k * M * M + a] = ar[j][k];
                    out[(size_t)k * M * M + a + 1] = ai[j][k];
                }
            }
        }
    }
}

}  // namespace oiva
