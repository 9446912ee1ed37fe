// Internal declarations shared by the translation units of liboveriva_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <string>

#include "kernel_choice.h"
#include "overiva_hip.h"

namespace oiva {

// records the thread-local message oiva_last_error() returns and hands back `code` (host_util.hip)
int fail_with(int code, const std::string& msg);
// exchange.hip: rank / world / slot size and every rank's gather buffer as mapped in this process; -1 unless connected
int xchg_peers(oiva_xchg* x, char** peers, int* rank, int* world, size_t* slot_bytes);

// packed Hermitian layout of one M x M covariance: M real diagonals, then for every c < d
// (row-major) the pair (re, im) of V[c][d] = sum w * x_c * conj(x_d).  M*M floats in total.
__host__ __device__ inline int herm_pair_index(int M, int c, int d) {  // c < d
    return M + 2 * (c * M - (c * (c + 1)) / 2 + (d - c - 1));
}

// Layout of the activation buffer R: (T, K) float32 activations r, kPhasesPerWave zeroed pad rows (kernels read
// whole groups of 4 frames), then -- 8-byte aligned -- one float64 partial sum of r per (block of kBlock frames,
// source), written by the activation kernel, from which every consumer derives gamma_k = mean_t r[t,k]
// (overiva.py:158) in the same fixed order.
__host__ __device__ inline size_t rsum_offset_floats(int T, int K) { return (((size_t)T + kPhasesPerWave) * K + 1) & ~(size_t)1; }
__host__ __device__ inline int rsum_blocks(int T) { return (T + kBlock - 1) / kBlock; }
__host__ __device__ inline size_t r_buffer_bytes(int T, int K) {
    return rsum_offset_floats(T, K) * sizeof(float) + (size_t)rsum_blocks(T) * K * sizeof(double);
}

// Launch of the dominant (covariance) kernel.  When the calling thread has armed a pair of events (arm_kernel_timer), the
// kernel is launched with them attached to its own dispatch (hipExtLaunchKernelGGL): their elapsed time is the kernel's
// duration as the profiler reports it, without the ~3 us of a separate event record in front and behind.
struct KernelTimer {
    hipEvent_t start = nullptr, stop = nullptr;
};
KernelTimer& kernel_timer();
inline void arm_kernel_timer(hipEvent_t start, hipEvent_t stop) {
    kernel_timer().start = start;
    kernel_timer().stop = stop;
}
template <typename Kern, typename... Args>
hipError_t launch_dominant(Kern kernel, dim3 grid, dim3 block, size_t shmem, hipStream_t s, Args... args) {
    KernelTimer& t = kernel_timer();
    if (t.start != nullptr) {
        hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)shmem, s, t.start, t.stop, 0, args...);
        t.start = t.stop = nullptr;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shmem, s, args...);
    }
    return hipGetLastError();
}

// the chunk that row y of power_kernel's grid takes (PowOrder and make_pow_order: kernel_choice.h)
__host__ __device__ inline int power_chunk_tail_first(int y, int n, const PowOrder& o) {
    if (y < o.q * o.cs) return o.first[y % o.cs + 1] - 1 - y / o.cs;
    y -= o.q * o.cs;
    for (int r = o.q; r < n; ++r)
        for (int s = 0; s < o.cs; ++s)
            if (o.first[s + 1] - o.first[s] > r && y-- == 0) return o.first[s + 1] - 1 - r;
    return n - 1;      // (not reached: the rows hold n chunks in all)
}

// ---- launchers (one per kernel family; each .hip file owns its template instantiations) -------
// Weighted covariance pass, overiva.py:179 (and :87 with unit weights).
//   X (T,F,M) c64; R (T,K) f32 activations r (unnormalised) or nullptr for unit weights (then K must be 1)
//   weights: w[t,k] = 1 / max(R[t,k] / gamma_k, eps), gamma_k = mean_t R (overiva.py:158-173); with raw != 0
//   gamma is taken as 1.  wscale (K): out, gamma (laplace) | sqrt(gamma) (gauss), written by one workgroup.
//   Vpart [nsplit][F][K][M*M] packed partial sums (NOT divided by T), float32 or (f64 != 0) float64
//   f64: accumulate in float64 (the reference's arithmetic: its float64 r_inv promotes overiva.py:179 to complex128)
// Xpad: (T, F, M + 1) copy of X with one zero channel behind every bin's M (odd 9..15 channels; launch_pad_channels), read by
// the vector-ALU kernels when g.pad is set; else nullptr
// g.xplain, g.rows: the load policy of X and the instantiation of cov_dma_kernel<8, KC> that follows it (kernel_choice.h)
hipError_t launch_cov(hipStream_t s, const float2* X, const float2* Xpad, const float* R, float* Wt, float* wscale, int model, int raw,
                      void* Vpart, bool f64, int T, int F, int M, int K, const CovGeom& g);
hipError_t launch_pad_channels(hipStream_t s, const float2* X, float2* Xpad, long long n_tf, int M);
// planar matrix-core kernel for 9..16 channels (grid = F bins x nsplit, tc frames per split, tc multiple of 4)
//   Wt (T,16): scratch for the final weights (written by a small pre-pass)
hipError_t launch_cov_mfma(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                           void* Vpart, bool f64, int T, int F, int M, int K, int nsplit, int tc);
// vector-ALU kernel for 10, 12, 14, 16 channels and K <= 4 sources, float32 arithmetic (kernels_cov_quad.hip): the Hermitian
// half split over four lanes per (bin, frame); tc multiple of 8; Vpart float64; R == nullptr: unit weights (K = 1);
// Wt (T,16): scratch for the final weights, as for launch_cov_mfma
hipError_t launch_cov_quad(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                           double* Vpart, int T, int F, int M, int Mv, int K, const CovGeom& g);
// pre-pass of the 9..16-channel kernels: Wt (T, Kp) = 1 / max(r / gamma, eps), columns >= K zero; writes wscale (K)
hipError_t launch_cov_weights(hipStream_t s, const float* R, float* Wt, float* wscale, int model, int raw, int T, int K, int Kp);
// float64 vector-ALU kernel for 8 channels (kernels_cov_pair64.hip): the Hermitian half split over two lanes per (bin, frame),
// 32 bins per workgroup (grid.x = ceil(F / 32)), tc multiple of 8, Vpart float64; Wt: the (T, 16) float scratch, used as
// (T, 8) doubles; R == nullptr: unit weights (K = 1)
hipError_t launch_cov_pair64(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                             double* Vpart, int T, int F, int M, int K, const CovGeom& g);
// float32 kernel for 8 channels and three or more sources, FOUR per pass over X (kernels_cov_pair32.hip): the Hermitian half
// over two lanes per (bin, frame), 32 bins per workgroup, tc multiple of 8, Vpart float64; Wt: (T, 16) scratch as for
// launch_cov_mfma; R == nullptr: unit weights (K = 1) on the same geometry
hipError_t launch_cov_pair32(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                             double* Vpart, int T, int F, int M, int K, const CovGeom& g);
// float32 vector-ALU kernel for 10, 12, 14, 16 channels and up to 16 sources in ONE pass (kernels_cov_half16.hip): the
// Hermitian half over 32 lanes per (bin, frame), 2 bins per workgroup (grid.x = ceil(F / 2)), tc multiple of 16, Vpart
// float64; Wt: (T + 1, 16) scratch (row T is zeroed by the launcher); R == nullptr: unit weights (K = 1)
hipError_t launch_cov_half16(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                             double* Vpart, int T, int F, int M, int Mv, int K, const CovGeom& g);
// its weights pre-pass and that of the float64 form, shared with the matrix-core kinds (Hmfma, Hmfma64)
hipError_t launch_cov_half16_weights(hipStream_t s, const float* R, float* Wt, float* wscale, int model, int raw, int T, int K);
hipError_t launch_cov_half16_weights_f64(hipStream_t s, const float* R, float* Wt, float* wscale, int model, int raw, int T, int K);
// the same decomposition with float64 sums (the `precise` arithmetic), 3..16 sources, 4 or 8 per pass; Wt: (T + 1, 16) DOUBLES
// 9..16 sources: the sources as rows of the fp32 matrix-core instruction, Hermitian products on the vector ALU (kernels_cov_hmfma.hip)
hipError_t launch_cov_hmfma(hipStream_t s, const float2* X, const float* Wt, double* Vpart, int T, int F, int M, int Mv, int K, const CovGeom& g);
hipError_t launch_cov_hmfma64(hipStream_t s, const float2* X, const double* Wt, double* Vpart, int T, int F, int M, int Mv, int K, const CovGeom& g);
hipError_t launch_cov_half16_f64(hipStream_t s, const float2* X, const float* R, float* Wt, float* wscale, int model, int raw,
                                 double* Vpart, int T, int F, int M, int Mv, int K, const CovGeom& g);
hipError_t cov_blocks_per_cu(int M, int kc, bool f64, int* n, bool rows = false);

// Demix + source power, overiva.py:140 + the norms at :153/:155.
//   What (F,M,M) c64 row-major;  Ppart [nb][T][K]
//   Xpad: (T, F, M + 1) zero-padded copy of X (odd 9..15 channels, many sources) or nullptr
hipError_t launch_power(hipStream_t s, const float2* X, const float2* Xpad, const float2* What, float* Ppart, int T, int F, int M,
                        int K, const PowGeom& g);
// matrix-core variant for 9..16 channels (same Ppart layout, one pass over X for all sources)
hipError_t launch_power_mfma(hipStream_t s, const float2* X, const float2* What, float* Ppart, int T, int F, int M, int Mp, int K);
hipError_t launch_power_lds(hipStream_t s, const float2* X, const float2* What, float* Ppart, int T, int F, int M, int K);
hipError_t pow_blocks_per_cu(int M, int kp, int tcp, int* n);

// Source activation, overiva.py:152-155: parts [nparts][T][K] -> R (T,K) = 2 sqrt(p) | p / F_total.
// activation with the exchange of the ranks' partial powers inside it (bins sharded over GPUs; kernels_misc.hip)
constexpr int kCanonBlocks = 8;      // the sum over the 64-bin parts is associated in at most this many blocks (activation_kernel)
hipError_t launch_activation_xchg(hipStream_t s, const float* parts, int nparts, char* const* gath, int rank, int world, int loopback,
                                  int nblk_own, int nblk_peer, unsigned* epochs, unsigned* ctrl, long long timeout_ticks, float* R, int T, int K,
                                  int model, int F_total);
hipError_t launch_activation(hipStream_t s, const float* parts, int nparts, float* R, int T, int K, int model,
                             int F_total);
// fixed-order float64 sum of partial buffers (float32, or float64 when f64): out[e] = scale * sum_i parts[i][e]
hipError_t launch_sum_parts(hipStream_t s, const void* parts, bool f64, int nparts, double* out, long long n, double scale);

// One problem of a ragged batch (oiva_batch_create_ragged, kernels_ragged.hip): where its data lie in the packed buffers and
// the geometry of its passes.  Every field is a function of the problem's own frame count T (and of F, M, K), never of B or
// of the other problems: the same numbers as a dense batch of T frames uses (batch.hip, frame_geom).
struct RaggedProblem {
    size_t x_off;     // first frame of the problem in the packed (sum T, F, M) X / (sum T, F, K) Y
    size_t p_off;     // its partial powers [nb][T][K] in Ppart (floats)
    size_t r_off;     // its activation buffer of r_buffer_bytes(T, K) in R (floats; even, so the float64 sums stay aligned)
    double inv_T;     // 1 / T as the host forms it (the scale of the input covariance)
    int T;
    int tcp, pw_nsplit;   // power pass: frames per split, splits
    int nsplit, tc;       // covariance pass: splits, frames per split
};

// Per-bin sequential update, overiva.py:181-190 (+ :161-167 W scaling, + :96-98 J init when init_only).
struct UpdateArgs {
    float2* What;         // (F,M,M) in/out (complex64: what the streaming kernels read)
    double2* What64;      // (F,M,M) complex128 copy carried between iterations by the float64 variants (or nullptr)
    const double* Cx;     // [F][M*M] packed, already divided by T
    const void* Vpart;    // [nsplit][F][K][M*M] packed partial sums, float32 or (vpart_f64) float64
    int vpart_f64;
    const float* wscale;  // (K) or nullptr
    int nsplit;
    int T, F, M, K;
    int init_only;        // 1: only (re)compute J from W and Cx
    int use_double;       // per-bin algebra in fp64
    int layout;           // 0: one lane per matrix element (M <= 8), 1: one lane per matrix row
    int wscale_bins = 0;  // batched plans (kernels_batch.hip): F is B problems of this many bins each and wscale is (B, K); 0: (K)
    // ragged batches (kernels_ragged.hip): the (B) problem records; bin f belongs to problem f / wscale_bins, whose V is the sum of
    // ITS nsplit partials scaled by 1 / ITS T (T and nsplit above are then the batch's largest).  nullptr on every other path.
    const RaggedProblem* ragged = nullptr;
};
// frame count and covariance split count behind bin f's V (the M <= 8 float64 update forms the batches dispatch)
__device__ __forceinline__ int update_frames(const UpdateArgs& a, int f) { return a.ragged ? a.ragged[f / a.wscale_bins].T : a.T; }
__device__ __forceinline__ int update_nsplit(const UpdateArgs& a, int f) {
    return a.ragged ? a.ragged[f / a.wscale_bins].nsplit : a.nsplit;
}
// the pending scale of column i of bin f (overiva.py:163 / :167): the bin's problem's row of wscale
__device__ __forceinline__ float wscale_at(const UpdateArgs& a, int f, int i) {
    return a.wscale[(a.wscale_bins > 0 ? (size_t)(f / a.wscale_bins) * a.K : 0) + i];
}
// W_hat element idx: the float64 variants keep their own complex128 copy so that nothing is rounded to
// float32 between iterations; the complex64 array is always written (the streaming kernels read it)
template <typename R>
__device__ __forceinline__ void load_what(const UpdateArgs& a, size_t idx, R& re, R& im) {
    if (sizeof(R) == 8 && a.What64 != nullptr) {
        const double2 v = a.What64[idx];
        re = (R)v.x;
        im = (R)v.y;
    } else {
        const float2 v = a.What[idx];
        re = (R)v.x;
        im = (R)v.y;
    }
}
template <typename R>
__device__ __forceinline__ void store_what(const UpdateArgs& a, size_t idx, R re, R im) {
    a.What[idx] = make_float2((float)re, (float)im);
    if (sizeof(R) == 8 && a.What64 != nullptr) a.What64[idx] = make_double2((double)re, (double)im);
}
// one packed partial as float64 whatever its storage type
__device__ __forceinline__ double load_vpart(const void* base, int f64, size_t idx) {
    return f64 ? static_cast<const double*>(base)[idx] : (double)static_cast<const float*>(base)[idx];
}
// fixed-order float64 sum of the nsplit frame-split partials of one packed element and of its neighbour idx + 1
// (the imaginary part of an off-diagonal entry; a valid address for every element of a packed matrix with M > 1,
// discarded by the caller where it means nothing).  Branch-free: the loads of 16 splits are issued together
// (splits past nsplit re-read the last one and are masked), so a sum costs one memory round trip per 16 splits.
template <int kBatch, typename P>
__device__ __forceinline__ void sum_vpart_b(const P* __restrict__ base, size_t idx, size_t stride, int nsplit, double& sr,
                                            double& si) {
    sr = 0.;
    si = 0.;
    for (int s0 = 0; s0 < nsplit; s0 += kBatch) {
        P vr[kBatch], vi[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int sp = s0 + u < nsplit ? s0 + u : nsplit - 1;
            vr[u] = base[idx + (size_t)sp * stride];
            vi[u] = base[idx + (size_t)sp * stride + 1];
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const double m = s0 + u < nsplit ? 1. : 0.;
            sr += m * (double)vr[u];
            si += m * (double)vi[u];
        }
    }
}
// (round 5: the batch follows the number of splits -- 2, 4, 8 or 16 loads per part in flight: with the batch of 16 whatever nsplit,
//  the four splits of the headline shape cost 12 masked re-reads of the last split and 12 multiplications by zero per part and
//  source: update 11.9 -> 10.1 us there, 17.3 -> 12.8 at 2049 x 235 x 5 / 5, 26.8 -> 23.2 at 8 / 4; same sums in the same order)
template <typename P>
__device__ __forceinline__ void sum_vpart_t(const P* __restrict__ base, size_t idx, size_t stride, int nsplit, double& sr,
                                            double& si) {
    if (nsplit <= 2)          // (uniform)
        sum_vpart_b<2>(base, idx, stride, nsplit, sr, si);
    else if (nsplit <= 4)
        sum_vpart_b<4>(base, idx, stride, nsplit, sr, si);
    else if (nsplit <= 8)
        sum_vpart_b<8>(base, idx, stride, nsplit, sr, si);
    else
        sum_vpart_b<16>(base, idx, stride, nsplit, sr, si);
}
__device__ __forceinline__ void sum_vpart(const void* base, int f64, size_t idx, size_t stride, int nsplit, bool pair,
                                          double& sr, double& si) {
    if (f64)          // uniform
        sum_vpart_t(static_cast<const double*>(base), idx, stride, nsplit, sr, si);
    else
        sum_vpart_t(static_cast<const float*>(base), idx, stride, nsplit, sr, si);
    if (!pair) si = 0.;
}
// the per-bin update: choose_update (kernel_choice.h) on the arguments and the process's switches, then the launcher of the file
// that holds the chosen kernel -- which only turns the choice's integers into template arguments
hipError_t launch_update(hipStream_t s, const UpdateArgs& a);
const UpdSwitches& update_switches();      // the four environment switches, read once per process (host_util.hip)
hipError_t launch_update_wave16(hipStream_t s, const UpdateArgs& a, const UpdChoice& c);   // Wave16, Det16 (kernels_update16.hip)
hipError_t launch_update_det16r(hipStream_t s, const UpdateArgs& a, const UpdChoice& c);   // Det16Rows (kernels_update16r.hip)
// covariance + per-bin update of the same bins in ONE launch (kernels_cov_update.hip): 8 channels, 2 sources + background,
// float32 products; frames in four splits of tc (one per wave of a 4-bin workgroup).  Same bits as launch_cov followed by
// launch_update when the plan's covariance geometry is those four splits (cov_update_supported, kernel_choice.h).
// a: What, What64, Cx, T, F, use_double.
hipError_t launch_cov_update(hipStream_t s, const float2* X, const float* R, float* wscale, int model, const UpdateArgs& a, int tc);

// Epilogue, overiva.py:192-199.
//   stats: per-bin sums for projection back: [nsplit][F][K][3] = (Re num, Im num, den)
hipError_t launch_demix_stats(hipStream_t s, const float2* X, const float2* What, float* Spart, int T, int F, int M,
                              int K, const CovGeom& g);
//   write Y (T,F,K) c64, scaled by conj(z) when Spart != nullptr
hipError_t launch_demix_write(hipStream_t s, const float2* X, const float2* What, const float* Spart, int nsplit,
                              float2* Y, int T, int F, int M, int K);
// OGIVE (ive.py:33-256): per-bin state and kernels (kernels_ogive.hip); the streaming passes are the AuxIVA ones
struct OgiveState {
    const double* Cx;    // [F][M*M] packed Hermitian, / T
    double2* CxInv;      // (F, M, M) complex128
    double* CxNorm;      // (F) Frobenius norm of Cx
    double2* A;          // (F, M) mixing vector a
    double2* Delta;      // (F, M) last step of every bin
    double* Lambda;      // (F) lambda_a
    int* DoA;            // (F) mixing-vector step selected
    int* DoW;            // (F) demixing-vector step selected
    double* Dnorm;       // (F) ||delta_f||
    int* ctrl;           // [0] stopping rule met, [1] epochs run, [2] step-kernel workgroups done this epoch
    double* maxdelta;    // [0] max_f ||delta_f|| of the last epoch, [1] running max of the current one (bit pattern)
    float2* What;        // (F, M, M): column 0 = w, what the streaming kernels read
    double2* What64;     // complex128 copy
};
constexpr int kModelOgiveLaplace = 2;   // activation r = sqrt(p) / sqrt(F) (ive.py:210); OIVA_MODEL_GAUSS serves ive.py:213
hipError_t launch_ogive_init(hipStream_t s, const OgiveState& st, int F, int M, int mode);
hipError_t launch_ogive_switch(hipStream_t s, const OgiveState& st, int F, int M);
hipError_t launch_ogive_step(hipStream_t s, const OgiveState& st, const void* Vpart, bool vpart_f64, int nsplit, int T, int F,
                             int M, double mu, double tol);

// W_hat = [eigenvectors of the K largest eigenvalues of Cx, ascending | [0; -I]]   (auxiva_pca.py:75-81); evals (F, M)
// ascending or nullptr; lapack_phase: W = conj(vecs) with every vector's largest component real (overiva.py:106-109)
hipError_t launch_pca_subspace(hipStream_t s, const double* Cx, float2* What, double2* What64, double* evals, int F, int M, int K,
                               bool lapack_phase);

// The wide path, 17..32 channels (kernels_wide.hip): the launchers above hand over to these for M > kNarrowMax.  Same buffer
// layouts as the narrow kernels (Vpart always float64).
//   covariance: float64 sums of exact float64 products whatever the arithmetic mode; Wt: (T, K) doubles of scratch
hipError_t launch_cov_wide(hipStream_t s, const float2* X, const float* R, void* Wt, float* wscale, int model, int raw, double* Vpart,
                           int T, int F, int M, int K, const CovGeom& g);
hipError_t launch_power_wide(hipStream_t s, const float2* X, const float2* What, float* Ppart, int T, int F, int M, int K, const PowGeom& g);
hipError_t launch_demix_stats_wide(hipStream_t s, const float2* X, const float2* What, float* Spart, int T, int F, int M, int K,
                                   const CovGeom& g);
hipError_t launch_demix_write_wide(hipStream_t s, const float2* X, const float2* What, const float* Spart, int nsplit, float2* Y, int T,
                                   int F, int M, int K);
hipError_t launch_update_wide(hipStream_t s, const UpdateArgs& a, const UpdChoice& c);

// The batched iteration (kernels_batch.hip, batch.hip): B problems of one shape, <= 8 channels, `precise` arithmetic.
//   X (B, T, F, M); What (B*F, M, M); Ppart [B][nb][T][K]; R: B buffers of r_stride floats (r_buffer_bytes(T, K) / 4);
//   wscale (B, K); Vpart [nsplit][B*F][K][M*M] float64 (K = 1 with R == nullptr: unit weights, the input covariance)
hipError_t launch_batch_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, int B, int T, int F, int M, int K,
                              int kp, int nsplit, int tcp);
hipError_t launch_batch_activation(hipStream_t s, const float* parts, int nparts, float* R, size_t r_stride, int B, int T, int K,
                                   int model, int F);
hipError_t launch_batch_cov(hipStream_t s, const float2* X, const float* R, size_t r_stride, float* wscale, int model, double* Vpart,
                            int B, int T, int F, int M, int K, int nsplit, int tc);

// The ragged batch (kernels_ragged.hip, batch.hip): B problems of T_b frames each, one F, M <= 8, K.  X packed (sum T, F, M);
// What, Cx, Vpart, wscale as the dense batch's (Vpart [max nsplit][B*F][K][M*M]: problem b writes and the update reads its
// first nsplit_b splits only); Ppart and R at the records' offsets.  Grids are sized by the largest problem; the workgroups
// past a problem's own extent return at entry.
hipError_t launch_ragged_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, const RaggedProblem* prob, int B, int F,
                               int M, int K, int kp, int max_pw_nsplit, int max_tcp);
hipError_t launch_ragged_activation(hipStream_t s, const float* parts, int nparts, float* R, const RaggedProblem* prob, int B, int K,
                                    int model, int F, int max_rblocks);
hipError_t launch_ragged_cov(hipStream_t s, const float2* X, const float* R, const RaggedProblem* prob, float* wscale, int model,
                             double* Vpart, int B, int F, int M, int K, int max_nsplit);
// Cx [B*F][M*M] = (1 / T_b) * the sum of problem b's own nsplit_b unit-weight partials (as launch_sum_parts for one problem)
hipError_t launch_ragged_sum_parts(hipStream_t s, const double* parts, const RaggedProblem* prob, double* Cx, int B, int F, int M);

// The complex128 data path of either batch (kernels_batch_c128.hip, batch.hip: oiva_batch_set_data_c128), float64 throughout, from
// the problem table.  X packed (sum T, F, M) complex128; Ppart: problem b's [c128_parts(F)][T_b][K] at p_off_b; Rw (sum T, K): r,
// then the weights; Gs [B][rblocks][K]: the block sums of r; Vpart as above (Wt == nullptr: unit weights, K = 1).
int c128_parts(int F);
hipError_t launch_c128_power(hipStream_t s, const double2* X, const double2* What64, double* Ppart, const RaggedProblem* prob, int B,
                             int max_T, int F, int M, int K);
// two launches: r and its block sums; then gamma, the weights in place, and W's columns divided by gamma | sqrt(gamma)
hipError_t launch_c128_activation(hipStream_t s, const double* Ppart, double* Rw, double* Gs, double2* What64, float2* What,
                                  const RaggedProblem* prob, int B, int max_T, int F, int M, int K, int model, int rblocks);
hipError_t launch_c128_cov(hipStream_t s, const double2* X, const double* Wt, const RaggedProblem* prob, double* Vpart, int B, int F,
                           int M, int K, int max_nsplit);
// Y (sum T, F, K) complex128; with proj_back the scales Z (B*F, K) first
hipError_t launch_c128_demix(hipStream_t s, const double2* X, const double2* What64, double2* Z, double2* Y, const RaggedProblem* prob,
                             int B, int max_T, int F, int M, int K, bool proj_back);

// The batched PCA front end (kernels_pca_batch.hip, batch.hip; auxiva_pca.py:79-81 and the composition of the filters behind it).
//   project: Xr (sum T, F, K) packed = the K principal components of every problem's X, one launch from the problem table; What
//   (B*F, M, M) holds P in columns 0..K-1.  The float32 chain of launch_demix_write without projection back, element by element.
hipError_t launch_pca_project(hipStream_t s, const float2* X, const float2* What, float2* Xr, const RaggedProblem* prob, int B, int F,
                              int M, int K, int kp, int max_pw_nsplit);
//   compose: columns 0..K-1 of What64 (nbins, M, M) <- P[:, :K] * Wred (nbins, K, K) in float64, and rounded into What
hipError_t launch_pca_compose(hipStream_t s, float2* What, double2* What64, const double2* Wred, long long nbins, int M, int K);

// Batched OGIVE (kernels_ogive_batch.hip, batch.hip): B problems of one shape, <= 8 channels, K = 1, `precise` arithmetic.
//   bin: OgiveState of the B*F bins (bin index = problem * F + bin; its ctrl / maxdelta are only the scratch ogive_init_kernel
//   resets); done, epochs, maxdelta (B): the per-problem stopping rule; runmax, ticket (B): the step kernel's hand-off.
//   Opart [osplit][B*F][2M+1] float64: per frame split, s = sum_t rinv_t x_t conj(y_t) (M complex) and zeta = sum_t rinv_t |y_t|^2
struct OgiveBatchState {
    OgiveState bin;
    int* done;
    int* epochs;
    double* maxdelta;
    unsigned long long* runmax;
    unsigned* ticket;
};
hipError_t launch_batch_ogive_switch(hipStream_t s, const OgiveBatchState& st, int B, int F, int M);
hipError_t launch_batch_ogive_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, const int* done, int B, int T, int F,
                                    int M, int nsplit, int tcp);
hipError_t launch_batch_ogive_activation(hipStream_t s, const float* parts, int nparts, float* R, size_t r_stride, const int* done, int B,
                                         int T, int amodel, int F);
hipError_t launch_batch_ogive_framesum(hipStream_t s, const float2* X, const double2* What64, const float* R, size_t r_stride,
                                       const int* done, double* Opart, int B, int T, int F, int M, int osplit, int otc);
hipError_t launch_batch_ogive_step(hipStream_t s, const OgiveBatchState& st, const double* Opart, int osplit, int B, int F, int M, double mu,
                                   double tol);

// Batched ILRMA (kernels_ilrma_batch.hip, batch.hip): B rooms of one shape, K = M <= 8, L <= 16 components, float64 state.
//   Tn (B, K, F, L); Vn (B, K, L, T); P, R (B, K, F, T), t fastest; Upart [2][ilrma_v_chunks(F)][B*K][L][T]; rowsum (B, K, F);
//   lam (B, K).  The per-bin IP1 step is launch_update on the partials launch_ilrma_cov leaves in the batch's Vpart.
struct IlrmaState {
    double* Tn;
    double* Vn;
    double* P;
    double* R;
    double* Upart;
    double* rowsum;
    double* lam;
    int L;
};
int ilrma_v_chunks(int F);
hipError_t launch_ilrma_power(hipStream_t s, const float2* X, const double2* What64, const IlrmaState& st, int B, int T, int F, int M);
hipError_t launch_ilrma_t(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K);          // Tn, then its rows of R
hipError_t launch_ilrma_v(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K);          // Vn (two launches)
hipError_t launch_ilrma_r(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K);          // R = Tn Vn
hipError_t launch_ilrma_cov(hipStream_t s, const float2* X, const IlrmaState& st, double* Vpart, int B, int T, int F, int M, int nsplit,
                            int tc);
//   rowsum, lam = sqrt(mean P), then P, R, Tn / lam^2 and W / lam (three launches)
hipError_t launch_ilrma_normalise(hipStream_t s, const IlrmaState& st, float2* What, double2* What64, int B, int T, int F, int M);

// Batched determined AuxIVA by iterative source steering (kernels_iss_batch.hip, batch.hip): B rooms from the
// problem table, K = M <= 8, float64 on complex64 X.  A workgroup of the sweep holds a group of consecutive bins of one room as
// complex128 in LDS; the group size is a function of the room's own T and of F and M alone.
constexpr int kIssMaxGroup = 8;               // bins of a group at most
constexpr int kIssSlabElems = 8192;           // T * M of one room at most: one bin's slab of 128 KiB
constexpr int kIssSlabBytes = kIssSlabElems * 16;
constexpr int kIssGroupLanes = 16;            // the activation adds a room's group partials in 16 strided sequences, then those in order
__host__ __device__ inline int iss_group_bins(int T, int F, int M) {
    const int fit = kIssSlabElems / (T * M);  // bins whose slab fits
    int g = M < 4 ? kIssMaxGroup : 4;         // a frame's read of 128 bytes or more where it fits, a bin per wavefront
    g = g < fit ? g : fit;
    g = g < F ? g : F;
    return g > 1 ? g : 1;
}
__host__ __device__ inline int iss_groups(int T, int F, int M) {
    const int g = iss_group_bins(T, F, M);
    return (F + g - 1) / g;
}
//   raises the dynamic LDS limit of the sweep kernel of M channels (once per device and M)
hipError_t iss_sweep_prepare(int M);
//   Part: room b's [iss_groups(T_b, F, M)][T_b][M] at x_off_b * max_groups * M; Phi (sum T_b, M): the weights; n_steps rank-1
//   steps (0: demix and partial powers only); slab_bytes: the largest group slab of the batch
hipError_t launch_iss_sweep(hipStream_t s, const float2* X, double2* What64, float2* What, const double* Phi, double* Part,
                            const RaggedProblem* prob, int B, int F, int M, int max_groups, size_t slab_bytes, int n_steps);
//   two launches: r into Rw (sum T_b, M); then gamma, the weights into Phi (sum T_b, M), W's columns scaled
hipError_t launch_iss_activation(hipStream_t s, const double* Part, double* Rw, double* Phi, double2* What64, float2* What,
                                 const RaggedProblem* prob, int B, int max_T, int F, int M, int model, int max_groups);

// Batched FIVE (kernels_five_batch.hip, batch.hip): the per-bin step of single-source extraction, the smallest
// eigenpair of the pencil (V_f, Cx_f) of nbins = B*F bins of M <= 8 channels in float64, 16 lanes per bin.
//   Li (nbins, M, M) complex128 = L^-1 of the Cholesky factor Cx_f = L L^H; non-finite where Cx_f is not positive definite
hipError_t launch_five_begin(hipStream_t s, const double* Cx, double2* Li, int nbins, int M);
//   Vpart [max nsplit][nbins][1][M*M]: bin f's room prob[f / F] adds its own nsplit partials in order and divides by its T;
//   w = Li^H u / sqrt(lambda) into column 0 of What64 and of What
hipError_t launch_five_update(hipStream_t s, const double* Vpart, const double2* Li, double2* What64, float2* What,
                              const RaggedProblem* prob, int nbins, int F, int M);

// The per-bin update of batched IP2 (kernels_ip2_batch.hip, batch.hip): the schedule of iteration `iteration`
// (pair steps and at most two single IP1 steps, J after every step when K < M) for every bin of the batch in one launch, float64.
// a: What, What64, Cx, Vpart (float64 partials), F = all bins, M <= 8, K, wscale_bins = bins per room, ragged = the problem table
// or nullptr with T and nsplit; wscale is not read.
hipError_t launch_ip2_update(hipStream_t s, const UpdateArgs& a, int iteration);

// The batched STFT (kernels_bstft.hip, bstft.hip): the passes around hipFFT for B rooms at once.  One record per room; a dense
// batch is the special case of equal records.
struct BstftRoom {
    long long s_off;   // first sample of the room in the packed (sum n_b, M) audio
    long long t_off;   // first frame of the room in the packed frame axis (its output starts at sample t_off * hop)
    int T;             // frames, n / hop
    int n;             // samples
};
int bstft_lds_stride(int C);
//   frames[(t * C + c) * L + i] = win[i] * x_room[(t_local * hop - (L - hop) + i), c], zero before the room's first sample
hipError_t launch_bstft_frame(hipStream_t s, const float* x, const float* win, float* frames, const BstftRoom* rooms, int B,
                              long long frames_total, int C, int L, int hop);
//   spec (frames_total * C, F) <-> X (frames_total, F, C), tiled through the LDS
hipError_t launch_bstft_to_tfc(hipStream_t s, const float2* spec, float2* X, long long frames_total, int F, int C);
hipError_t launch_bstft_from_tfc(hipStream_t s, const float2* Y, float2* spec, long long frames_total, int F, int C);
//   y packed (n_out = sum T_b * hop, C): per-room overlap-add in increasing t, * 1 / L
hipError_t launch_bstft_overlap_add(hipStream_t s, const float* frames, const float* win, float* y, const BstftRoom* rooms, int B,
                                    long long n_out, int C, int L, int hop);

// BSS Eval (kernels_bsseval.hip, bsseval.hip): SDR / SIR / SAR of S sets of estimates against one set of references, B rooms,
// float64.  One record per room; a dense batch is the special case of equal records.  Every field is a function of the room's own
// (n, N, Lf).  The buffers of consecutive sets lie one set after the other; G, Gf and Hf hold the rooms of one group and are shared
// by the sets; a single evaluation (oiva_bsseval) is one set, a sets handle (oiva_bsssets) one group.
constexpr int kBssMaxSrc = 8;       // sources per room
constexpr int kBssMaxFilter = 512;  // filter taps
constexpr int kBssSeg = 2048;       // samples per segment of the lag sums: segment g of a room is [g * kBssSeg, min(n, (g + 1) * kBssSeg))
constexpr int kBssBlock = 64;       // block size of the Cholesky factorisation, the substitutions and the quadratic forms
struct BssRoom {
    long long sig_off;   // first element of the room's (N, n) signals in the packed signals of a set
    int n;               // samples
    int nseg;            // ceil(n / kBssSeg)
    int seg_off;         // its first segment in the flat list of (room, segment) pairs
    int pad;
};
//   S sets of N signals each (sig, the sets sig_stride apart) against the references: part [room segment][set][k][i][Lf], Epart
//   [room segment][set][k], then out (S, B, N, N, Lf) and E (S, B, N) with the segments added in order
hipError_t launch_bss_lags(hipStream_t s, const double* ref, const double* sig, long long sig_stride, const BssRoom* rooms,
                           const int2* segs, long long total_segs, int B, int S, int N, int Lf, double* part, double* Epart, double* out,
                           double* E);
//   rooms g0 .. g0 + rooms - 1 of rlag (B, N, N, Lf) into the group's G, Gf (to be factored), Hf (the diagonal blocks, to be
//   factored); thr is indexed by the room of the batch
hipError_t launch_bss_assemble(hipStream_t s, const double* rlag, double* G, double* Gf, double* Hf, double* thr, int g0, int rooms, int N,
                               int Lf);
//   nmat dense dim x dim matrices, lower triangle in place; matrix m belongs to room g0 + m / per_room, whose flag a bad pivot sets
hipError_t launch_bss_cholesky(hipStream_t s, double* A, int nmat, int dim, int* flag, const double* thr, int g0, int per_room);
//   C <- D, c <- D[j], then both through the group's factors Gf and Hf, for S sets of (B, N, N Lf)
hipError_t launch_bss_solve(hipStream_t s, const double* Gf, const double* Hf, const double* D, double* C, double* c, int g0, int rooms,
                            int B, int S, int N, int Lf, const int* flag);
//   the quadratic forms of the group's rooms, then crit: per set sdr, sir, sar (B, N, N) [room, estimate, reference]
hipError_t launch_bss_criteria(hipStream_t s, const double* D, const double* E, const double* G, const double* C, const double* c,
                               double* qL, double* qS, double* crit, int g0, int rooms, int B, int S, int N, int Lf, int diag_only,
                               const int* flag);

// Shoebox image-source rooms (kernels_room.hip, room.hip): impulse responses, premix and mix-down of B rooms of S
// sources and M microphones, float64.  One record per room; every field is the room's own.
constexpr int kRoomFdl = 81;          // taps of one image's windowed sinc
constexpr int kRoomHalf = 40;         // its fixed lag
constexpr int kRoomMaxOrder = 32;
constexpr int kRoomMaxSrc = 16;
constexpr int kRoomMaxMic = 32;
constexpr int kRoomMaxRir = 65536;
struct RoomRec {
    double dim[3];       // Lx, Ly, Lz
    double beta[6];      // sqrt(1 - alpha) of the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz
    long long rir_off;   // first element of the room's (S, M, Lr) impulse responses in the packed buffer
    int Lr;              // length of its impulse responses
    int pad;
};
//   images (n_img) of (nx, ny, nz, 0) in enumeration order; src (B, S, 3), mic (B, M, 3); tau = d * fs_over_c
//   kmax[b] = max(kmax[b], largest k of room b): an integer max, the caller zeroes it
hipError_t launch_room_kmax(hipStream_t s, const RoomRec* rooms, const double* src, const double* mic, const char4* images, int n_img,
                            int B, int S, int M, double fs_over_c, int* kmax);
//   rir packed by rooms[b].rir_off: every sample of every pair is written, its terms added in the order of the images
hipError_t launch_room_rir(hipStream_t s, const RoomRec* rooms, const double* src, const double* mic, const char4* images, int n_img,
                           int B, int S, int M, int max_Lr, double fs_over_c, double* rir);
//   dst (rows, nfft) = src (rows, len), zero-padded; the rows of src lie src_stride apart
hipError_t launch_room_pad(hipStream_t s, const double* src, long long src_stride, int len, double* dst, int nfft, int rows);
//   H (S, M, nf) *= X (S, nf)
hipError_t launch_room_product(hipStream_t s, double2* H, const double2* X, int nf, int S, int M);
//   premix (rows, n_out) = y (rows, nfft)[:n_out] / nfft
hipError_t launch_room_unpack(hipStream_t s, const double* y, int nfft, double* premix, int n_out, int rows);
//   std[s_] = population standard deviation of premix[s_, ref_mic, :] of one room (S, M, n_out): mean first, then the squares, a
//   fixed tree
hipError_t launch_room_std(hipStream_t s, const double* premix, int S, int M, int n_out, int ref_mic, double* std);
//   mix (n_out, M) and ref (K + 1, n_out, M) of one room: premix[s_] / std[s_] * scale[s_], targets s_ < K, the rest and
//   sigma_n * noise (n_out, M; may be null) to the background
hipError_t launch_room_mix(hipStream_t s, const double* premix, const double* std, const double* scale, const double* noise,
                           double sigma_n, int S, int M, int K, int n_out, double* mix, double* ref);

// The sweep's hand-overs (kernels_sweep.hip, sweep.hip): room simulation -> batched STFT -> BSS Eval on the device.
// One record per room of the group the sweep handle was made for; every field but ref_off is a function of the room's own
// (n_out, frame, hop) and of the rooms before it.
constexpr int kSweepMaxChan = 8;      // channels of y, as the batched solvers
constexpr int kSweepChunk = 4096;     // samples per workgroup of the standard deviation: chunk j of a room is [j, j + 1) * kSweepChunk
struct SweepRoom {
    long long y_off;     // first sample of the room in the packed (sum T_b hop, C) synthesis
    long long ref_off;   // first element of its (K + 1, n_out, M) references in the room handle's buffer (set by take_mix)
    long long sig_off;   // first element of its (K + 1, m) rows in the packed ref / est of oiva_bsseval
    long long fil_off;   // first sample of its filler row in the packed (sum m_b) filler
    int n_out;           // samples of the mix
    int ny;              // samples of the synthesis, T * hop
    int m;               // samples that are evaluated, ny - (frame - hop)
    int pad;
};
//   out (n) float32 = in (n) float64, round to nearest even
hipError_t launch_sweep_cast(hipStream_t s, const double* in, float* out, long long n);
//   std (B, 8): population standard deviation of the C channels of every room's y; part: 2 * B * 8 * max_chunks doubles
hipError_t launch_sweep_std(hipStream_t s, const float* y, const SweepRoom* rooms, int B, int C, int max_chunks, double* part,
                            double* std);
//   order (B, 8): the channels by descending std, ties to the lower index; reorder == 0: the identity
hipError_t launch_sweep_order(hipStream_t s, const double* std, int B, int C, int reorder, int* order);
//   est[b, k, i] = y[b, i + offset, order[b, k]] (k < K), est[b, K, i] = filler[b, i], ref[b, j, i] = room_ref[b, j, i, ref_mic]
//   (j <= K), i < m_b
hipError_t launch_sweep_align(hipStream_t s, const float* y, const double* room_ref, const double* filler, const int* order,
                              const SweepRoom* rooms, int B, int C, int M, int K, int ref_mic, int offset, int max_m, double* est,
                              double* ref);
// What the sweep sees of the other handles (defined next to each struct: room.hip, bsseval.hip, bstft.hip; not exported).
struct RoomGroupView {      // the mixed group g0 of a room handle
    int device, rooms, M, K;
    const double* mix;      // packed (n_out_b, M) of the group's rooms
    const double* ref;      // room i of the group at (K + 1) * mix_off[i], (K + 1, n_out_b, M)
    long long mix_total;    // elements of mix
};
//   OIVA_ERR_STATE unless the group is mixed; n_out, mix_off: `rooms` entries each (at most max_rooms are written)
int room_group_view(oiva_room* p, int g0, RoomGroupView* view, int* n_out, long long* mix_off, int max_rooms);
struct BssSignalView {
    int device, B, N, Lf;
    long long sig_total;
    double *ref, *est;
};
//   lengths: B entries (at most max_rooms are written)
void bsseval_signal_view(oiva_bsseval* p, BssSignalView* view, int* lengths, int max_rooms);
//   what oiva_bsseval_set_signals leaves behind once ref and est are written
void bsseval_mark_signals(oiva_bsseval* p);
void bstft_dims(oiva_bstft* p, int* device, int* B, int* M, int* frame, int* hop, long long* samples_total);

// The device random generator (kernels_rng.hip, rng.hip): Philox-4x64-10 under a key per stream, counter
// (block, purpose, 0, 0), four standard normals per block.  One record per stream; every value is a function of the stream's own
// key, of the purpose and of its index in the stream.
constexpr int kRngMaxGridX = 65535;
constexpr int kRngMaxStreams = 65535;
constexpr long long kRngMaxCount = 1ll << 40;      // elements of one handle
constexpr int kRngMaxRaw = 1 << 20;                // blocks of one oiva_rng_raw call
struct RngStream {
    unsigned long long k0, k1;   // the stream's key
    long long off;               // first element of its values in the packed output
    long long count;             // its length
};
//   out packed by streams[i].off: elements [0, count) of every stream, nothing behind them; max_count: the longest stream
hipError_t launch_rng_normal(hipStream_t s, const RngStream* streams, int n_streams, long long max_count, unsigned long long purpose,
                             double* out);
//   words (n, 4): the raw words of blocks first .. first + n - 1 of one stream
hipError_t launch_rng_raw(hipStream_t s, unsigned long long k0, unsigned long long k1, unsigned long long purpose,
                          unsigned long long first, int n, unsigned long long* words);
//   the body of oiva_room_mix and oiva_rng_room_mix (room.hip): the group's noise from the host (noise_host, may be null: no
//   noise), or, with keys, drawn into the handle's noise buffer: room g0 + i of the group under (key0[i], key1[i]), purpose 0
int room_mix_body(oiva_room* p, int g0, int K, double sinr, double snr, int ref_mic, const double* sources_var,
                  const double* noise_host, const unsigned long long* key0, const unsigned long long* key1);

// The decay measurement (kernels_decay.hip, decay.hip): Schroeder integral, threshold crossings and the masked sums
// of the fit for a packed batch of responses, float64.  One record per response; every result is a function of the response's own
// samples and length.
constexpr int kDecayTile = 1024;            // samples per tile, counted from sample 0: kBlock lanes of 4 consecutive samples
constexpr int kDecayMaxLen = 1 << 24;       // samples of one response
constexpr int kDecayMaxResp = 1 << 22;      // responses of one handle
struct DecayRec {
    long long off;       // first sample of the response in the packed input (and in the packed curve)
    int len;             // its length
    int pad;
};
//   e0 (n_resp), idx (n_resp, 2) = i_a, i_b (-1: none), sums (n_resp, 2) = sum D, sum n D over theta_b < E[n] <= theta_a with
//   theta = E[0] * fa, E[0] * fb; curve: null or packed like `in`
hipError_t launch_decay(hipStream_t s, const DecayRec* recs, int n_resp, const double* in, double fa, double fb, double* curve, double* e0,
                        int* idx, double* sums);
//   binds n_resp responses that lie packed at `dev` on `device` (borrowed) to a decay handle: OIVA_ERR_ARG unless the device and
//   the table of lengths are the handle's (decay.hip; the caller is oiva_decay_set_room in room.hip)
int decay_bind(oiva_decay* p, int device, const double* dev, const int* lengths, int n_resp);

// dense complex128 <-> complex64 conversion on the device
hipError_t launch_cast_c128_to_c64(hipStream_t s, const double2* in, float2* out, long long n);
hipError_t launch_cast_c64_to_c128(hipStream_t s, const float2* in, double2* out, long long n);

// unpack packed Hermitian float64 [nmat][M*M] -> full complex nmat x (M,M): complex64, or complex128 when out_f64
hipError_t launch_unpack_herm(hipStream_t s, const double* packed, void* full, bool out_f64, long long nmat, int M);

}  // namespace oiva
