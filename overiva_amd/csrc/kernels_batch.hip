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
#include <type_traits>
#include "oiva_device.h"
#include "activation_arith.h"
#include "demix_arith.h"
#include "batch_cov_arith.h"

namespace oiva {
// (the kernel of a (channels, sources per pass) pair is instantiated only where pow_kp_reachable holds: kernel_choice.h)
template <int I>
using IntC = std::integral_constant<int, I>;
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
// weighted covariance, float64 (batch_cov_block, batch_cov_arith.h): workgroup = 16 bins x one frame split of problem grid.z
// ---------------------------------------------------------------------------------------------
template <int M, bool UNIT>
__global__ __launch_bounds__(kBlock) void batch_cov_kernel(const float2* __restrict__ X, const float* __restrict__ R, size_t r_stride,
                                                           float* __restrict__ wscale, int model, double* __restrict__ Vpart, int T,
                                                           int F, int K, int tc, int nbins_all) {
    const int prob = blockIdx.z;
    batch_cov_block<M, UNIT>(X, (size_t)prob * T, R, (size_t)prob * r_stride, wscale, model, Vpart, T, F, K, tc, nbins_all, prob);
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
    auto go = [&](auto mm, auto kk) -> hipError_t {      // (a generic lambda: the branch not taken is not instantiated)
        constexpr int MM = decltype(mm)::value, KP = decltype(kk)::value;
        if constexpr (pow_kp_reachable(MM, KP)) {
            hipLaunchKernelGGL((batch_power_kernel<MM, KP>), grid, dim3(kBlock), shmem, s, X, What, Ppart, T, F, K, tcp, nz);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    };
#define CALL(MM) \
    return kp == 1 ? go(IntC<MM>{}, IntC<1>{}) : kp == 2 ? go(IntC<MM>{}, IntC<2>{}) : kp == 4 ? go(IntC<MM>{}, IntC<4>{}) : hipErrorInvalidValue;
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
