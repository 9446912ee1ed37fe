// Kernels of the ragged batch (overiva_batch_ragged, oiva_batch_create_ragged in batch.hip): B problems of one F, M <= 8 and K
// but of T_b frames each.
//
//   X      (sum T_b, F, M) complex64, packed: problem b holds frames [x_off_b, x_off_b + T_b)
//   prob   (B) RaggedProblem records (oiva_internal.h): offsets and the geometry of every pass, functions of T_b alone
//   What, Cx, wscale, Vpart [max nsplit][B*F][K][M*M]: as the dense batch's (kernels_batch.hip); problem b writes (and the update
//          reads) its first nsplit_b splits only
//   Ppart  problem b's [nb][T_b][K] at p_off_b;  R: problem b's activation buffer of r_buffer_bytes(T_b, K) at r_off_b
//
// Each kernel is the dense batch's with the problem's own base pointers, T_b and splits: the same workgroup bodies (power_block,
// activation_block, batch_cov_block), so problem b gets the bits of a dense batch of T_b frames.  A grid is sized by the largest
// problem; a workgroup past its own problem's extent returns at entry, before any barrier.  The records are read through a
// pointer, so a captured graph stays valid for the batch's life.
#include <type_traits>
#include "oiva_device.h"
#include "activation_arith.h"
#include "batch_cov_arith.h"
#include "demix_arith.h"

namespace oiva {
// (the kernel of a (channels, sources per pass) pair is instantiated only where pow_kp_reachable holds: kernel_choice.h)
template <int I>
using IntC = std::integral_constant<int, I>;
namespace {

// demix + power (grid = 64-bin batches x max power splits x problem * source passes)
template <int M, int KP>
__global__ __launch_bounds__(kBlock) void ragged_power_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                              float* __restrict__ Ppart, const RaggedProblem* __restrict__ probs, int F,
                                                              int K, int nz) {
    extern __shared__ __attribute__((aligned(16))) float sp[];  // [kWaves][max tcp][KP]
    const int prob = blockIdx.z / nz;
    const int kz = blockIdx.z - prob * nz;
    const RaggedProblem d = probs[prob];
    if ((int)blockIdx.y >= d.pw_nsplit) return;
    power_block<M, KP>(X + d.x_off * F * M, What + (size_t)prob * F * M * M, Ppart + d.p_off, d.T, F, K, d.tcp, blockIdx.x,
                       blockIdx.y, kz * KP, sp);
}

// activation (grid = max rsum_blocks x sources x problems)
template <int NP>
__global__ __launch_bounds__(kBlock) void ragged_activation_kernel(const float* __restrict__ parts, int nparts, float* __restrict__ R,
                                                                   const RaggedProblem* __restrict__ probs, int K, int model,
                                                                   float inv_f_total) {
    __shared__ double wsum[kWaves];
    const RaggedProblem d = probs[blockIdx.z];
    if ((int)blockIdx.x >= rsum_blocks(d.T)) return;
    activation_block<NP>(parts + d.p_off, nparts, R + d.r_off, d.T, K, model, inv_f_total, blockIdx.x, blockIdx.y, wsum);
}

// weighted covariance, float64; UNIT: the input covariance (grid = 16-bin groups x max covariance splits x problems)
template <int M, bool UNIT>
__global__ __launch_bounds__(kBlock) void ragged_cov_kernel(const float2* __restrict__ X, const float* __restrict__ R,
                                                            const RaggedProblem* __restrict__ probs, float* __restrict__ wscale, int model,
                                                            double* __restrict__ Vpart, int F, int K, int nbins_all) {
    const int prob = blockIdx.z;
    const RaggedProblem d = probs[prob];
    if ((int)blockIdx.y >= d.nsplit) return;
    batch_cov_block<M, UNIT>(X, d.x_off, R, d.r_off, wscale, model, Vpart, d.T, F, K, d.tc, nbins_all, prob);
}

// Cx = (1 / T_b) * the sum of problem b's nsplit_b partials, in split order (sum_parts_kernel's arithmetic)
__global__ __launch_bounds__(kBlock) void ragged_sum_parts_kernel(const double* __restrict__ parts, const RaggedProblem* __restrict__ probs,
                                                                  double* __restrict__ out, long long n, int per_prob) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const RaggedProblem d = probs[e / per_prob];
    double s = 0.;
    for (int i = 0; i < d.nsplit; ++i) s += parts[(size_t)i * n + e];
    out[e] = s * d.inv_T;
}

#define OIVA_RAGGED_DISPATCH_M(CALL) \
    switch (M) {                     \
        case 1: CALL(1); break;      \
        case 2: CALL(2); break;      \
        case 3: CALL(3); break;      \
        case 4: CALL(4); break;      \
        case 5: CALL(5); break;      \
        case 6: CALL(6); break;      \
        case 7: CALL(7); break;      \
        case 8: CALL(8); break;      \
    }

}  // namespace

hipError_t launch_ragged_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, const RaggedProblem* prob, int B, int F,
                               int M, int K, int kp, int max_pw_nsplit, int max_tcp) {
    const int nb = (F + kBinsPerWave * kWaves - 1) / (kBinsPerWave * kWaves);
    const int nz = (K + kp - 1) / kp;
    const dim3 grid((unsigned)nb, (unsigned)max_pw_nsplit, (unsigned)(B * nz));
    const size_t shmem = (size_t)kWaves * max_tcp * kp * sizeof(float);
    if (M < 1 || M > 8 || max_tcp > kPowMaxFrames) return hipErrorInvalidValue;
    auto go = [&](auto mm, auto kk) -> hipError_t {      // (a generic lambda: the branch not taken is not instantiated)
        constexpr int MM = decltype(mm)::value, KP = decltype(kk)::value;
        if constexpr (pow_kp_reachable(MM, KP)) {
            hipLaunchKernelGGL((ragged_power_kernel<MM, KP>), grid, dim3(kBlock), shmem, s, X, What, Ppart, prob, F, K, nz);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    };
#define CALL(MM) \
    return kp == 1 ? go(IntC<MM>{}, IntC<1>{}) : kp == 2 ? go(IntC<MM>{}, IntC<2>{}) : kp == 4 ? go(IntC<MM>{}, IntC<4>{}) : hipErrorInvalidValue;
    OIVA_RAGGED_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_ragged_activation(hipStream_t s, const float* parts, int nparts, float* R, const RaggedProblem* prob, int B, int K,
                                    int model, int F, int max_rblocks) {
    const dim3 grid((unsigned)max_rblocks, (unsigned)K, (unsigned)B);
    const float inv = 1.f / (float)F;
    if (nparts <= 8)
        hipLaunchKernelGGL(ragged_activation_kernel<8>, grid, dim3(kBlock), 0, s, parts, nparts, R, prob, K, model, inv);
    else if (nparts <= 16)
        hipLaunchKernelGGL(ragged_activation_kernel<16>, grid, dim3(kBlock), 0, s, parts, nparts, R, prob, K, model, inv);
    else
        hipLaunchKernelGGL(ragged_activation_kernel<32>, grid, dim3(kBlock), 0, s, parts, nparts, R, prob, K, model, inv);
    return hipGetLastError();
}

hipError_t launch_ragged_cov(hipStream_t s, const float2* X, const float* R, const RaggedProblem* prob, float* wscale, int model,
                             double* Vpart, int B, int F, int M, int K, int max_nsplit) {
    const dim3 grid((unsigned)((F + kBatchBins - 1) / kBatchBins), (unsigned)max_nsplit, (unsigned)B);
    const int nbins_all = B * F;
    if (M < 1 || M > 8) return hipErrorInvalidValue;
#define CALL(MM)                                                                                                                    \
    if (R == nullptr)                                                                                                               \
        hipLaunchKernelGGL((ragged_cov_kernel<MM, true>), grid, dim3(kBlock), 0, s, X, R, prob, wscale, model, Vpart, F, 1, nbins_all); \
    else                                                                                                                            \
        hipLaunchKernelGGL((ragged_cov_kernel<MM, false>), grid, dim3(kBlock), 0, s, X, R, prob, wscale, model, Vpart, F, K, nbins_all);
    OIVA_RAGGED_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_ragged_sum_parts(hipStream_t s, const double* parts, const RaggedProblem* prob, double* Cx, int B, int F, int M) {
    const int per_prob = F * M * M;
    const long long n = (long long)B * per_prob;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(ragged_sum_parts_kernel, grid, dim3(kBlock), 0, s, parts, prob, Cx, n, per_prob);
    return hipGetLastError();
}

}  // namespace oiva
