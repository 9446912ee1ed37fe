// Kernels of the batched iteration (overiva_batch, batch.hip): B problems of one shape per launch.
//
//   X      (B, T, F, M) complex64, problem-major: the host layout, uploaded in one copy
//   What   (B*F, M, M), Cx [B*F][M*M], Vpart [nsplit][B*F][K][M*M]: per-bin buffers of B*F bins, problem-major
//   Ppart  [B][nb][T][K], R: B activation buffers of r_buffer_bytes(T, K) each, wscale (B, K)
//
// The problem index comes from the grid (blockIdx.z), and a workgroup's bins never straddle two problems: the 64-bin batches
// of the power pass and the 16-bin groups of the covariance pass are counted within each problem, so the ragged last group of
// every problem is handled as the single-problem kernels handle theirs.  Every order of summation is a function of the bin and
// the frame within the problem (never of B, of the problem's place in the batch, or of the grid position): a problem gets the
// same bits alone, in a batch of 8, or in a permuted batch.  The per-bin stages that read neither X nor the activations (the
// update, the J initialisation, the eigensolver) run the single-problem kernels on B*F bins (UpdateArgs::wscale_bins).
#include "oiva_device.h"
#include "activation_arith.h"
#include "demix_arith.h"

namespace oiva {
namespace {

// ---------------------------------------------------------------------------------------------
// demix + power: power_block per problem (grid.z = problem x source pass).  The same lanes and sums as power_kernel, so
// a problem's partial powers are those of its single-problem plan.
// ---------------------------------------------------------------------------------------------
template <int M, int KP>
__global__ __launch_bounds__(kBlock) void batch_power_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                             float* __restrict__ Ppart, int T, int F, int K, int tcp, int nz) {
    extern __shared__ __attribute__((aligned(16))) float sp[];  // [kWaves][tcp][KP]
    const int prob = blockIdx.z / nz;
    const int kz = blockIdx.z - prob * nz;
    const float2* Xb = X + (size_t)prob * T * F * M;
    const float2* Wb = What + (size_t)prob * F * M * M;
    float* Pb = Ppart + (size_t)prob * gridDim.x * T * K;
    power_block<M, KP>(Xb, Wb, Pb, T, F, K, tcp, blockIdx.x, blockIdx.y, kz * KP, sp);
}

// ---------------------------------------------------------------------------------------------
// activation: activation_block per problem (grid.z = problem): r, the float64 block sums behind it (from which gamma and the
// eps floor follow in the covariance pass) from that problem's 64-bin parts only
// ---------------------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(kBlock) void batch_activation_kernel(const float* __restrict__ parts, int nparts, float* __restrict__ R,
                                                                  size_t r_stride, int T, int K, int model, float inv_f_total) {
    __shared__ double wsum[kWaves];
    const int prob = blockIdx.z;
    activation_block<NP>(parts + (size_t)prob * nparts * T * K, nparts, R + (size_t)prob * r_stride, T, K, model, inv_f_total,
                         blockIdx.x, blockIdx.y, wsum);
}

// ---------------------------------------------------------------------------------------------
// weighted covariance, float64 (the `precise` arithmetic): V_k[f] = sum_t w[t,k] x_{t,f} x_{t,f}^H, overiva.py:179, as
// float64 sums of exact float64 products; with UNIT the input covariance (overiva.py:87, K = 1, w = 1).
// Workgroup = 16 bins of one problem x one frame split.  Chunks of kBatchChunk frames of the 16 bins are staged in LDS with
// their weights; thread = (bin, entry c <= d of the Hermitian half) -- up to NI of them --, holding the sums of ALL sources, so
// one product x_c conj(x_d) serves every source.  A sum runs over the split's frames in order; the partial of every split is
// stored packed (herm_pair_index) and the update adds the splits in order (sum_vpart).
// ---------------------------------------------------------------------------------------------
constexpr int kBatchChunk = 32;
constexpr int kBatchBins = 16;

template <int M, bool UNIT>
__global__ __launch_bounds__(kBlock) void batch_cov_kernel(const float2* __restrict__ X, const float* __restrict__ R, size_t r_stride,
                                                           float* __restrict__ wscale, int model, double* __restrict__ Vpart, int T,
                                                           int F, int K, int tc, int nbins_all) {
    constexpr int E = M * (M + 1) / 2;                           // entries of the Hermitian half
    constexpr int NI = (kBatchBins * E + kBlock - 1) / kBlock;   // (bin, entry) items per thread
    constexpr int KM = UNIT ? 1 : M;                             // sources held (K <= M)
    __shared__ float2 xs[kBatchChunk][kBatchBins][M];
    __shared__ double ws[kBatchChunk][KM];

    const int tid = threadIdx.x;
    const int prob = blockIdx.z;
    const int f0 = blockIdx.x * kBatchBins;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const float2* Xb = X + (size_t)prob * T * F * M;
    const float* Rb = UNIT ? nullptr : R + (size_t)prob * r_stride;
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

#define OIVA_BATCH_DISPATCH_M(CALL) \
    switch (M) {                    \
        case 1: CALL(1); break;     \
        case 2: CALL(2); break;     \
        case 3: CALL(3); break;     \
        case 4: CALL(4); break;     \
        case 5: CALL(5); break;     \
        case 6: CALL(6); break;     \
        case 7: CALL(7); break;     \
        case 8: CALL(8); break;     \
    }

}  // namespace

int batch_cov_bins_per_block() { return kBatchBins; }

hipError_t launch_batch_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, int B, int T, int F, int M, int K,
                              int kp, int nsplit, int tcp) {
    const int nb = (F + kBinsPerWave * kWaves - 1) / (kBinsPerWave * kWaves);
    const int nz = (K + kp - 1) / kp;
    const dim3 grid((unsigned)nb, (unsigned)nsplit, (unsigned)(B * nz));
    const size_t shmem = (size_t)kWaves * tcp * kp * sizeof(float);
    if (M < 1 || M > 8 || tcp > kPowMaxFrames) return hipErrorInvalidValue;
#define CALL(MM)                                                                                                              \
    if (kp == 1) hipLaunchKernelGGL((batch_power_kernel<MM, 1>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, tcp, nz); \
    else if (kp == 2) hipLaunchKernelGGL((batch_power_kernel<MM, 2>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, tcp, nz); \
    else if (kp == 4) hipLaunchKernelGGL((batch_power_kernel<MM, 4>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, tcp, nz); \
    else return hipErrorInvalidValue;
    OIVA_BATCH_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_batch_activation(hipStream_t s, const float* parts, int nparts, float* R, size_t r_stride, int B, int T, int K,
                                   int model, int F) {
    const dim3 grid((unsigned)rsum_blocks(T), (unsigned)K, (unsigned)B);
    const float inv = 1.f / (float)F;
    if (nparts <= 8)
        hipLaunchKernelGGL(batch_activation_kernel<8>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, T, K, model, inv);
    else if (nparts <= 16)
        hipLaunchKernelGGL(batch_activation_kernel<16>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, T, K, model, inv);
    else
        hipLaunchKernelGGL(batch_activation_kernel<32>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, T, K, model, inv);
    return hipGetLastError();
}

hipError_t launch_batch_cov(hipStream_t s, const float2* X, const float* R, size_t r_stride, float* wscale, int model, double* Vpart,
                            int B, int T, int F, int M, int K, int nsplit, int tc) {
    const dim3 grid((unsigned)((F + kBatchBins - 1) / kBatchBins), (unsigned)nsplit, (unsigned)B);
    const int nbins_all = B * F;
    if (M < 1 || M > 8) return hipErrorInvalidValue;
#define CALL(MM)                                                                                                          \
    if (R == nullptr)                                                                                                     \
        hipLaunchKernelGGL((batch_cov_kernel<MM, true>), grid, dim3(kBlock), 0, s, X, R, r_stride, wscale, model, Vpart, T, F, 1, tc, nbins_all); \
    else                                                                                                                  \
        hipLaunchKernelGGL((batch_cov_kernel<MM, false>), grid, dim3(kBlock), 0, s, X, R, r_stride, wscale, model, Vpart, T, F, K, tc, nbins_all);
    OIVA_BATCH_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

}  // namespace oiva
