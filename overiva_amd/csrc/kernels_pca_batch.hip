// Kernels of the batched PCA front end (auxiva_pca_batch, oiva_batch_project_dev / oiva_batch_compose_w in batch.hip): B problems
// of one F, M <= 8 and K < M but of T_b frames each, driven from the problem table as the ragged batch's kernels are
// (kernels_ragged.hip; a dense batch is the table of equal lengths).
//
//   project : Xr[t,f,k] = sum_m conj(P[b,f,m,k]) X[t,f,m]      reference auxiva_pca.py:79-81, all problems in ONE launch
//             X (sum T_b, F, M), Xr (sum T_b, F, K) complex64, both packed along the frames; P = columns 0..K-1 of What (B*F, M, M)
//   compose : W_tot[:, :K] = P[:, :K] W_red, float64           np.matmul(P, W_red) of auxiva_pca.py (ours), per (problem, bin)
//
// project keeps the lanes of the power pass -- a wave is 16 bins x 4 frame phases, a workgroup the 64-bin batch blockIdx.x and the
// frames [blockIdx.y * tcp_b, + tcp_b) of problem blockIdx.z / passes, kBatchPowUnroll frame steps loaded before the first is
// consumed -- and the per-lane arithmetic of the epilogue (load_wconj / demix_one, demix_arith.h): every output element is the
// float32 FMA chain write_kernel (kernels_demix.hip) forms without projection back.  No sum crosses lanes, so a problem's bits do
// not depend on the batch it is in.  A workgroup past its own problem's extent returns at entry.
#include <type_traits>
#include "oiva_device.h"
#include "demix_arith.h"

namespace oiva {
// (the kernel of a (channels, sources per pass) pair is instantiated only where pow_kp_reachable holds: kernel_choice.h)
template <int I>
using IntC = std::integral_constant<int, I>;
namespace {

template <int M, int KP>
__global__ __launch_bounds__(kBlock) void pca_project_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                             float2* __restrict__ Xr, const RaggedProblem* __restrict__ probs, int F,
                                                             int K, int nz) {
    const int prob = blockIdx.z / nz;
    const int k0 = (blockIdx.z - prob * nz) * KP;
    const RaggedProblem d = probs[prob];
    if ((int)blockIdx.y >= d.pw_nsplit) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int b = lane & 15;
    const int q = lane >> 4;
    const int f = (blockIdx.x * kWaves + wave) * kBinsPerWave + b;
    const bool fvalid = f < F;
    const int fc = fvalid ? f : F - 1;
    const int T = d.T;
    const int t_begin = blockIdx.y * d.tcp;
    const int t_end = min(T, t_begin + d.tcp);
    const int len = t_end - t_begin;
    const int nsteps = (len + 3) >> 2;

    float wr[KP][M], wi[KP][M];
    load_wconj<M, KP>(What + (size_t)prob * F * M * M, fc, k0, K, wr, wi);

    const size_t frame_stride = (size_t)F * M;
    const float2* pbase = X + d.x_off * frame_stride + (size_t)fc * M;
    float2* ybase = Xr + (d.x_off * F + (size_t)fc) * K + k0;
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
            const bool live = fvalid && tl < len;
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                float yr, yi;
                demix_one<M>(wr[kk], wi[kk], xr[u], xi[u], yr, yi);
                if (live && k0 + kk < K) ybase[(size_t)(t_begin + tl) * F * K + kk] = make_float2(yr, yi);
            }
        }
    }
}

// one lane per (bin of the batch, row r): row r of P times W_red, all K columns, then written over row r of P -- no lane reads
// what another writes
template <int K>
__global__ __launch_bounds__(kBlock) void pca_compose_kernel(float2* __restrict__ What, double2* __restrict__ What64,
                                                             const double2* __restrict__ Wred, long long nrows, int M) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= nrows) return;
    const long long bin = e / M;
    double2* prow = What64 + (size_t)e * M;
    const double2* wr = Wred + (size_t)bin * K * K;
    double2 p[K], o[K];
#pragma unroll
    for (int j = 0; j < K; ++j) p[j] = prow[j];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double sr = 0., si = 0.;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double2 w = wr[j * K + k];
            sr += p[j].x * w.x - p[j].y * w.y;
            si += p[j].x * w.y + p[j].y * w.x;
        }
        o[k] = make_double2(sr, si);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        prow[k] = o[k];
        What[(size_t)e * M + k] = make_float2((float)o[k].x, (float)o[k].y);
    }
}

}  // namespace

hipError_t launch_pca_project(hipStream_t s, const float2* X, const float2* What, float2* Xr, const RaggedProblem* prob, int B, int F,
                              int M, int K, int kp, int max_pw_nsplit) {
    const int nb = (F + kBinsPerWave * kWaves - 1) / (kBinsPerWave * kWaves);
    const int nz = (K + kp - 1) / kp;
    const dim3 grid((unsigned)nb, (unsigned)max_pw_nsplit, (unsigned)(B * nz));
    if (M < 1 || M > 8 || K < 1 || K > M) return hipErrorInvalidValue;
    auto go = [&](auto mm, auto kk) -> hipError_t {      // (a generic lambda: the branch not taken is not instantiated)
        constexpr int MM = decltype(mm)::value, KP = decltype(kk)::value;
        if constexpr (pow_kp_reachable(MM, KP)) {
            hipLaunchKernelGGL((pca_project_kernel<MM, KP>), grid, dim3(kBlock), 0, s, X, What, Xr, prob, F, K, nz);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    };
#define CALL(MM) \
    return kp == 1 ? go(IntC<MM>{}, IntC<1>{}) : kp == 2 ? go(IntC<MM>{}, IntC<2>{}) : kp == 4 ? go(IntC<MM>{}, IntC<4>{}) : hipErrorInvalidValue;
    switch (M) {
        case 1: CALL(1); break;
        case 2: CALL(2); break;
        case 3: CALL(3); break;
        case 4: CALL(4); break;
        case 5: CALL(5); break;
        case 6: CALL(6); break;
        case 7: CALL(7); break;
        case 8: CALL(8); break;
    }
#undef CALL
    return hipGetLastError();
}

hipError_t launch_pca_compose(hipStream_t s, float2* What, double2* What64, const double2* Wred, long long nbins, int M, int K) {
    if (M < 1 || M > 8 || K < 1 || K > M) return hipErrorInvalidValue;
    const long long nrows = nbins * M;
    const dim3 grid((unsigned)((nrows + kBlock - 1) / kBlock));
#define CALL(KK) hipLaunchKernelGGL(pca_compose_kernel<KK>, grid, dim3(kBlock), 0, s, What, What64, Wred, nrows, M)
    switch (K) {
        case 1: CALL(1); break;
        case 2: CALL(2); break;
        case 3: CALL(3); break;
        case 4: CALL(4); break;
        case 5: CALL(5); break;
        case 6: CALL(6); break;
        case 7: CALL(7); break;
        case 8: CALL(8); break;
    }
#undef CALL
    return hipGetLastError();
}

}  // namespace oiva
