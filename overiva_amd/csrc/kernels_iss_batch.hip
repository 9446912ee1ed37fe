// Kernels of batched determined AuxIVA by iterative source steering (auxiva_iss_batch, batch.hip: oiva_batch_iss_*):
// B rooms of T_b frames each from the problem table, K = M <= 8, every stage in float64 on complex64 X.
//
//   X      (sum T_b, F, M) complex64, packed: room b holds frames [x_off_b, x_off_b + T_b)
//   What64 (B*F, M, M) complex128, element [m][s] = W[f, m, s]; What its complex64 copy (what the batch's demix reads)
//   Part   room b's [groups_b][T_b][M] float64 at x_off_b * max_groups * M: |y|^2 added over the bins of a group
//   Rw     (sum T_b, M) float64: r; Phi (sum T_b, M) float64: the weights 1 / max(r / gamma, eps)
//
// A workgroup of the sweep owns one group of G = iss_group_bins(T_b, F, M) consecutive bins of one room, holds their demixed
// signals as a complex128 slab [bin][channel][frame] in dynamic LDS and runs the M rank-1 steps there, one wavefront per bin.
// Orders of summation (functions of (bin, frame) within the room and of its T, F and M alone): the channels of a demix in
// ascending order as one FMA chain; every sum over the frames of a bin lane-strided and sequential per lane, closed by the fixed
// butterfly over the channel's lanes; the bins of a group in ascending order; the groups 16 apart in order per lane and the 16
// lanes in order; r lane-strided over 256 threads, closed by block_sum.
// A room therefore gets the same bits alone, in a larger batch, in a permuted one or among rooms of other lengths.
#include <algorithm>

#include "oiva_device.h"

namespace oiva {
namespace {

constexpr double kEpsR64 = 1e-15;      // reference overiva.py:170

// ---------------------------------------------------------------------------------------------
// demix, n_steps rank-1 steps, partial powers.  grid = (groups of the room with the most, rooms), kBlock threads.
//   head: thread = (frame, bin of the group), the bin fastest, so a frame's read is G*M*8 contiguous bytes; y of the M channels
//         as FMA chains from the group's W in LDS, stored to the slab
//   sweep: wavefront w takes bins w, w + 4, ...; lane = (channel m, frame lane), J = 64, 32, 16, 16, 8 ... frame lanes per
//         channel (stride J over the frames).  Step k: d_m and sum_t phi_m y_m conj(y_k) of the lane's channel, then
//         y_m -= v_m y_k from the old y_k; the bin's W lies one element per lane and is updated through __shfl
//   tail: thread = (frame, channel): |y|^2 of the group's bins in ascending order
// n_steps = 0: demix and partial powers only (W is not written).
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kBlock) void iss_sweep_kernel(const float2* __restrict__ X, double2* __restrict__ What64,
                                                           float2* __restrict__ What, const double* __restrict__ Phi,
                                                           double* __restrict__ Part, const RaggedProblem* __restrict__ probs, int F,
                                                           int max_groups, int n_steps) {
    extern __shared__ double2 slab[];                  // [G][M][T]
    __shared__ double2 wsm[kIssMaxGroup][M * M];
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    const int T = d.T;
    const int G = iss_group_bins(T, F, M);
    const int f0 = blockIdx.x * G;
    if (f0 >= F) return;                               // (past the room's groups: before any barrier)
    const int gn = min(G, F - f0);                     // live bins of the group
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < gn * M * M; i += kBlock) wsm[i / (M * M)][i % (M * M)] = What64[((size_t)prob * F + f0) * M * M + i];
    __syncthreads();

    const float2* Xb = X + d.x_off * F * M;
    for (int i = tid; i < T * gn; i += kBlock) {
        const int t = i / gn, g = i - t * gn;
        float xr[M], xi[M];
        load_x<M>(Xb + ((size_t)t * F + f0 + g) * M, xr, xi);
#pragma unroll
        for (int s = 0; s < M; ++s) {
            double yr = 0., yi = 0.;
#pragma unroll
            for (int m = 0; m < M; ++m) {              // x conj(w), channels in ascending order
                const double2 w = wsm[g][m * M + s];
                yr = fma((double)xr[m], w.x, yr);
                yr = fma((double)xi[m], w.y, yr);
                yi = fma((double)xi[m], w.x, yi);
                yi = fma(-(double)xr[m], w.y, yi);
            }
            slab[((size_t)g * M + s) * T + t] = make_double2(yr, yi);
        }
    }
    __syncthreads();

    if (n_steps > 0) {
        // lane = (channel lm, frame lane lj): J frame lanes per channel, so that a step costs three sums per lane, closed over
        // the J lanes of the channel, instead of 3 M sums closed over the wavefront
        constexpr int J = M == 1 ? 64 : M == 2 ? 32 : M <= 4 ? 16 : 8;
        constexpr int U = 4;                           // frames a lane has in flight (enters no sum)
        const int lm = lane / J, lj = lane - lm * J;
        const bool active = lm < M;
        const int mc = active ? lm : M - 1;
        const int tstart = active ? lj : T;            // (lanes past the M channels take no frame)
        const double* ph = Phi + d.x_off * M + mc;     // [t][m]
        const int e = lane < M * M ? lane : 0;         // this lane's element of W: row e / M, column e % M
        const int wrow = e / M, wcol = e - wrow * M;
        for (int g = wave; g < gn; g += kWaves) {
            double2* yb = slab + (size_t)g * M * T;
            double2* ym_p = yb + (size_t)mc * T;
            double2 w = wsm[g][e];
            for (int k = 0; k < n_steps; ++k) {
                const double2* yk_p = yb + (size_t)k * T;
                double dd = 0., nr = 0., ni = 0.;
                for (int t0 = tstart; t0 < T; t0 += J * U) {
                    double2 yk[U], ym[U];
                    double p[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = t0 + u * J;
                        const int tc = t < T ? t : t0;
                        yk[u] = yk_p[tc];
                        ym[u] = ym_p[tc];
                        p[u] = t < T ? ph[(size_t)tc * M] : 0.;        // frames past T add 0.
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (t0 + u * J < T) {
                            const double a = fma(yk[u].x, yk[u].x, yk[u].y * yk[u].y);
                            dd = fma(p[u], a, dd);
                            nr = fma(p[u], fma(ym[u].x, yk[u].x, ym[u].y * yk[u].y), nr);       // y_m conj(y_k)
                            ni = fma(p[u], fma(ym[u].y, yk[u].x, -(ym[u].x * yk[u].y)), ni);
                        }
                    }
                }
#pragma unroll
                for (int off = J / 2; off > 0; off >>= 1) {
                    dd += __shfl_xor(dd, off, 64);
                    nr += __shfl_xor(nr, off, 64);
                    ni += __shfl_xor(ni, off, 64);
                }
                double vr, vi;
                if (mc != k) {
                    vr = dd > 0. ? nr / dd : 0.;
                    vi = dd > 0. ? ni / dd : 0.;
                } else {
                    vr = dd > 0. ? 1. - 1. / sqrt(dd / (double)T) : 0.;
                    vi = 0.;
                }
                // y_m -= v_m y_k from the old y_k: every frame belongs to one (lane, batch), and a batch reads before it writes
                for (int t0 = tstart; t0 < T; t0 += J * U) {
                    double2 yk[U], ym[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = t0 + u * J;
                        const int tc = t < T ? t : t0;
                        yk[u] = yk_p[tc];
                        ym[u] = ym_p[tc];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = t0 + u * J;
                        if (t < T) {
                            ym[u].x -= fma(vr, yk[u].x, -(vi * yk[u].y));
                            ym[u].y -= fma(vr, yk[u].y, vi * yk[u].x);
                            ym_p[t] = ym[u];
                        }
                    }
                }
                // W[:, m] -= conj(v_m) W[:, k], from the old column k; v_m from the first lane of channel m
                const double wkr = __shfl(w.x, wrow * M + k, 64), wki = __shfl(w.y, wrow * M + k, 64);
                const double cr = __shfl(vr, wcol * J, 64), ci = __shfl(vi, wcol * J, 64);
                w.x -= fma(cr, wkr, ci * wki);
                w.y -= fma(cr, wki, -(ci * wkr));
            }
            if (lane < M * M) {
                const size_t idx = ((size_t)prob * F + f0 + g) * M * M + lane;
                What64[idx] = w;
                What[idx] = make_float2((float)w.x, (float)w.y);
            }
        }
        __syncthreads();
    }

    double* Pb = Part + d.x_off * max_groups * M + (size_t)blockIdx.x * T * M;
    for (int i = tid; i < T * M; i += kBlock) {
        const int t = i / M, m = i - t * M;
        double p = 0.;
        for (int g = 0; g < gn; ++g) {
            const double2 y = slab[((size_t)g * M + m) * T + t];
            p += fma(y.x, y.x, y.y * y.y);
        }
        Pb[i] = p;
    }
}

// ---------------------------------------------------------------------------------------------
// activation, first launch, overiva.py:152-155: p[t,k] from the group partials and r = 2 sqrt(p) | p / F.  Workgroup = 16
// consecutive (frame, source) elements (a run of 128 bytes in every group's partial) x 16 group lanes: lane j adds groups j,
// j + 16, ... in ascending order, the 16 lane sums are added in order (grid = runs of the longest room x rooms)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void iss_activation_kernel(const double* __restrict__ Part, double* __restrict__ Rw,
                                                                const RaggedProblem* __restrict__ probs, int M, int model, int F,
                                                                int max_groups) {
    __shared__ double part[kIssGroupLanes][kIssGroupLanes + 1];
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    const int n = d.T * M;
    if ((int)blockIdx.x * kIssGroupLanes >= n) return;     // (past the room's frames: before the barrier)
    const int e = threadIdx.x & (kIssGroupLanes - 1), j = threadIdx.x / kIssGroupLanes;
    const int idx = blockIdx.x * kIssGroupLanes + e;
    const int ng = iss_groups(d.T, F, M);
    double acc = 0.;
    if (idx < n) {
        const double* Pb = Part + d.x_off * max_groups * M + idx;
#pragma unroll 4
        for (int g = j; g < ng; g += kIssGroupLanes) acc += Pb[(size_t)g * n];
    }
    part[j][e] = acc;
    __syncthreads();
    if (j == 0 && idx < n) {
        double p = 0.;
#pragma unroll
        for (int jj = 0; jj < kIssGroupLanes; ++jj) p += part[jj][e];
        Rw[d.x_off * M + idx] = model == OIVA_MODEL_LAPLACE ? 2. * sqrt(p) : p / (double)F;
    }
}

// second launch: gamma = mean_t r (overiva.py:158), by every workgroup for itself: thread i adds frames i, i + 256, ... in
// order, block_sum closes; phi = 1 / max(r / gamma, eps) (:159, :170-173, a NaN stays NaN); the columns of W divided by gamma |
// sqrt(gamma) (:161-167), both copies (grid = blocks of max(T M, F M M) elements of the largest room x rooms)
__global__ __launch_bounds__(kBlock) void iss_finalize_kernel(const double* __restrict__ Rw, double* __restrict__ Phi,
                                                              double2* __restrict__ What64, float2* __restrict__ What,
                                                              const RaggedProblem* __restrict__ probs, int F, int M, int model) {
    __shared__ double gam[8];
    __shared__ double wsum[kWaves];
    const int prob = blockIdx.y;
    const RaggedProblem d = probs[prob];
    const double* Rb = Rw + d.x_off * M;
    for (int k = 0; k < M; ++k) {
        double s = 0.;
        for (int t = threadIdx.x; t < d.T; t += kBlock) s += Rb[(size_t)t * M + k];
        s = block_sum(s, wsum);
        if (threadIdx.x == 0) gam[k] = s / (double)d.T;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < (long long)d.T * M) {
        double rn = Rb[i] / gam[(int)(i % M)];
        rn = rn < kEpsR64 ? kEpsR64 : rn;
        Phi[d.x_off * M + i] = 1. / rn;
    }
    if (i < (long long)F * M * M) {
        const int k = (int)(i % M);
        const size_t idx = (size_t)prob * F * M * M + (size_t)i;
        const double sc = model == OIVA_MODEL_LAPLACE ? gam[k] : sqrt(gam[k]);
        double2 w = What64[idx];
        w.x /= sc;
        w.y /= sc;
        What64[idx] = w;
        What[idx] = make_float2((float)w.x, (float)w.y);
    }
}

#define OIVA_ISS_DISPATCH_M(CALL) \
    switch (M) {                  \
        case 1: CALL(1); break;   \
        case 2: CALL(2); break;   \
        case 3: CALL(3); break;   \
        case 4: CALL(4); break;   \
        case 5: CALL(5); break;   \
        case 6: CALL(6); break;   \
        case 7: CALL(7); break;   \
        case 8: CALL(8); break;   \
    }

unsigned blocks_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t iss_sweep_prepare(int M) {
    if (M < 1 || M > 8) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    // the slab of one group may take kIssSlabBytes of dynamic LDS: above the default limit of a launch
#define CALL(MM) \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&iss_sweep_kernel<MM>), hipFuncAttributeMaxDynamicSharedMemorySize, kIssSlabBytes)
    OIVA_ISS_DISPATCH_M(CALL)
#undef CALL
    return e;
}

hipError_t launch_iss_sweep(hipStream_t s, const float2* X, double2* What64, float2* What, const double* Phi, double* Part,
                            const RaggedProblem* prob, int B, int F, int M, int max_groups, size_t slab_bytes, int n_steps) {
    if (M < 1 || M > 8 || n_steps < 0 || n_steps > M || slab_bytes > (size_t)kIssSlabBytes) return hipErrorInvalidValue;
    const dim3 grid((unsigned)max_groups, (unsigned)B);
#define CALL(MM) \
    hipLaunchKernelGGL(iss_sweep_kernel<MM>, grid, dim3(kBlock), slab_bytes, s, X, What64, What, Phi, Part, prob, F, max_groups, n_steps)
    OIVA_ISS_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_iss_activation(hipStream_t s, const double* Part, double* Rw, double* Phi, double2* What64, float2* What,
                                 const RaggedProblem* prob, int B, int max_T, int F, int M, int model, int max_groups) {
    const unsigned runs = (unsigned)((max_T * M + kIssGroupLanes - 1) / kIssGroupLanes);
    hipLaunchKernelGGL(iss_activation_kernel, dim3(runs, (unsigned)B), dim3(kBlock), 0, s, Part, Rw, prob, M, model, F, max_groups);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long n = std::max((long long)max_T * M, (long long)F * M * M);
    hipLaunchKernelGGL(iss_finalize_kernel, dim3(blocks_of(n), (unsigned)B), dim3(kBlock), 0, s, Rw, Phi, What64, What, prob, F, M, model);
    return hipGetLastError();
}

}  // namespace oiva
