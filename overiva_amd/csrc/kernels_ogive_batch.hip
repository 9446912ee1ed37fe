// Kernels of batched OGIVE (ogive_batch, batch.hip): B problems of one shape, one epoch of ive.py:190-246 for all of them.
//
//   X      (B, T, F, M) complex64, problem-major (the layout of kernels_batch.hip)
//   per-bin state of B*F bins (OgiveState, bin index = problem * F + bin); done / epochs / maxdelta per problem
//   Ppart  [B][nb][T], R: B activation buffers, Opart [osplit][B*F][2M+1] float64
//
// One epoch: the switching criterion (every 10 epochs, update="switching"), demix + power pass, activation, the frame sums
// s = X^T psi, zeta = Y^T psi of ive.py:221-227 straight from X, and the per-bin step with the stopping rule of its problem.
// The problem index is blockIdx.z and a workgroup never holds bins of two problems.  A workgroup whose problem is done
// returns at once; `done` is written only by the last workgroup of a problem in the step kernel, the last launch of an
// epoch, so every kernel of one epoch sees the same value.  Every order of summation is a function of (bin, frame) within
// the problem, so a problem's bits -- and the epoch at which its rule fires -- do not depend on B, on its place in the batch
// or on which other problems have stopped.  The arithmetic of the per-bin kernels is that of kernels_ogive.hip (copied:
// the single-problem kernels stay as they are).
#include "oiva_device.h"
#include "activation_arith.h"
#include "demix_arith.h"

namespace oiva {
namespace {

struct Zb {
    double re, im;
};
__device__ __forceinline__ Zb zmul(Zb a, Zb b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Zb zconj(Zb a) { return {a.re, -a.im}; }
__device__ __forceinline__ Zb zinv(Zb a) {
    const double d = 1.0 / (a.re * a.re + a.im * a.im);
    return {a.re * d, -a.im * d};
}
__device__ __forceinline__ void zacc(Zb& s, Zb a, Zb b) {   // s += a * b
    s.re += a.re * b.re - a.im * b.im;
    s.im += a.re * b.im + a.im * b.re;
}
// entry (i, j) of a packed Hermitian matrix held as M diagonals then (re, im) of every i < j pair
__device__ __forceinline__ Zb herm_at(const double* __restrict__ p, int M, int i, int j) {
    if (i == j) return {p[i], 0.};
    if (i < j) {
        const int o = herm_pair_index(M, i, j);
        return {p[o], p[o + 1]};
    }
    const int o = herm_pair_index(M, j, i);
    return {p[o], -p[o + 1]};
}

// ---------------------------------------------------------------------------------------------
// switching criterion, ive.py:146-166 (ogive_switch_kernel's arithmetic), one thread per bin, grid.z = problem
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(64) void batch_ogive_switch_kernel(OgiveBatchState sb, int F) {
    const int prob = blockIdx.z;
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F || sb.done[prob]) return;
    const OgiveState& st = sb.bin;
    const size_t fb = (size_t)prob * F + f;
    const double* cx = st.Cx + fb * M * M;
    Zb an[M], bn[M];
    const Zb a0 = {st.A[fb * M].x, st.A[fb * M].y};
    const Zb ia0 = zinv(a0);
#pragma unroll
    for (int m = 0; m < M; ++m) an[m] = zmul(Zb{st.A[fb * M + m].x, st.A[fb * M + m].y}, ia0);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        Zb s = {0., 0.};
#pragma unroll
        for (int j = 0; j < M; ++j) zacc(s, herm_at(cx, M, i, j), an[j]);
        bn[i] = s;
    }
    const Zb lmb = bn[0];
    const Zb il = zinv(lmb);
    double p1 = 0., nb = 0.;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        bn[m] = zmul(bn[m], il);
        const double dr = an[m].re - bn[m].re, di = an[m].im - bn[m].im;
        p1 += dr * dr + di * di;
        nb += bn[m].re * bn[m].re + bn[m].im * bn[m].im;
    }
    p1 = sqrt(p1) / st.CxNorm[fb];
    double p2 = 0.;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            Zb cbb = zmul(lmb, zmul(bn[i], zconj(bn[j])));          // lmb * b b^H / ||b||^2
            cbb = {cbb.re / nb, cbb.im / nb};
            const Zb c = herm_at(cx, M, i, j);
            const double dr = c.re - cbb.re, di = c.im - cbb.im;
            p2 += dr * dr + di * di;
        }
    const double kappa = p1 * sqrt(p2) / sqrt((double)M);
    st.DoA[fb] = kappa >= 0.1 ? 1 : 0;                                // ive.py:163-166 (NaN -> demixing step off too)
    st.DoW[fb] = kappa < 0.1 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// demix + power pass (power_block, one source) and activation (activation_block) of the problems still running
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kBlock) void batch_ogive_power_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                                   float* __restrict__ Ppart, const int* __restrict__ done, int T, int F,
                                                                   int tcp) {
    extern __shared__ __attribute__((aligned(16))) float sp[];  // [kWaves][tcp]
    const int prob = blockIdx.z;
    if (done[prob]) return;
    power_block<M, 1>(X + (size_t)prob * T * F * M, What + (size_t)prob * F * M * M, Ppart + (size_t)prob * gridDim.x * T, T, F, 1, tcp,
                      blockIdx.x, blockIdx.y, 0, sp);
}

template <int NP>
__global__ __launch_bounds__(kBlock) void batch_ogive_activation_kernel(const float* __restrict__ parts, int nparts, float* __restrict__ R,
                                                                        size_t r_stride, const int* __restrict__ done, int T, int amodel,
                                                                        float inv_f_total) {
    __shared__ double wsum[kWaves];
    const int prob = blockIdx.z;
    if (done[prob]) return;
    activation_block<NP>(parts + (size_t)prob * nparts * T, nparts, R + (size_t)prob * r_stride, T, 1, amodel, inv_f_total, blockIdx.x, 0,
                         wsum);
}

// ---------------------------------------------------------------------------------------------
// frame sums, ive.py:215-227: per bin f of the problem, over the frames of split blockIdx.y,
//     s_f = sum_t rinv_t x_{t,f} conj(y_{t,f})   (M complex)      zeta_f = sum_t rinv_t |y_{t,f}|^2
// with y = w^H x in float64 from the complex128 w and rinv = 1 / max(r, eps) in float64 (the weights the single-problem
// path gives its covariance pass).  Workgroup = 64 bins (lane = bin; a (frame, bin)'s M channels are one contiguous load)
// x 4 waves; wave v sums the split's frames t_begin + v, + 4, ... in order, then the waves' sums are added in wave order.
// ---------------------------------------------------------------------------------------------
constexpr int kOgSumBins = 64;
constexpr int kOgSumUnroll = 2;

template <int M>
__global__ __launch_bounds__(kBlock) void batch_ogive_framesum_kernel(const float2* __restrict__ X, const double2* __restrict__ What64,
                                                                      const float* __restrict__ R, size_t r_stride,
                                                                      const int* __restrict__ done, double* __restrict__ Opart, int T,
                                                                      int F, int tc, int nbins_all) {
    constexpr int NS = 2 * M + 1;
    __shared__ double red[kWaves - 1][NS][kOgSumBins];
    const int prob = blockIdx.z;
    if (done[prob]) return;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int f = blockIdx.x * kOgSumBins + lane;
    const bool fvalid = f < F;
    const int fc = fvalid ? f : F - 1;
    const float2* Xb = X + (size_t)prob * T * F * M;
    const float* Rb = R + (size_t)prob * r_stride;
    const size_t fb = (size_t)prob * F + fc;

    double wr[M], wi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double2 v = What64[(fb * M + m) * M];                   // column 0 of W_hat
        wr[m] = v.x;
        wi[m] = v.y;
    }
    double sr[M], si[M], z = 0.;
#pragma unroll
    for (int m = 0; m < M; ++m) sr[m] = si[m] = 0.;

    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const size_t frame_stride = (size_t)F * M;
    const float2* pbase = Xb + (size_t)fc * M;
    for (int t0 = t_begin + wave; t0 < t_end; t0 += kWaves * kOgSumUnroll) {
        float xr[kOgSumUnroll][M], xi[kOgSumUnroll][M];
        float rr[kOgSumUnroll];
#pragma unroll
        for (int u = 0; u < kOgSumUnroll; ++u) {
            const int t = t0 + u * kWaves;
            const int tcl = t < t_end ? t : t_end - 1;                 // clamped: legal address, result unused
            rr[u] = Rb[tcl];
            load_x<M>(pbase + (size_t)tcl * frame_stride, xr[u], xi[u]);
        }
#pragma unroll
        for (int u = 0; u < kOgSumUnroll; ++u) {
            if (t0 + u * kWaves >= t_end) break;
            double rn = (double)rr[u];
            rn = rn < (double)kEpsR ? (double)kEpsR : rn;               // a NaN stays NaN, like r[r < eps] = eps
            const double ri = 1. / rn;
            // y = sum_m x_m conj(w_m)   (ive.py:153 demix: X @ conj(W))
            double yr = 0., yi = 0.;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double a = xr[u][m], b = xi[u][m];
                yr = fma(wr[m], a, fma(wi[m], b, yr));
                yi = fma(wr[m], b, fma(-wi[m], a, yi));
            }
            const double cr = ri * yr, ci = ri * yi;                  // rinv y: psi = conj(rinv y)
            z = fma(cr, yr, fma(ci, yi, z));
#pragma unroll
            for (int m = 0; m < M; ++m) {                               // x_m conj(rinv y)
                const double a = xr[u][m], b = xi[u][m];
                sr[m] = fma(a, cr, fma(b, ci, sr[m]));
                si[m] = fma(b, cr, fma(-a, ci, si[m]));
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            red[wave - 1][2 * m][lane] = sr[m];
            red[wave - 1][2 * m + 1][lane] = si[m];
        }
        red[wave - 1][2 * M][lane] = z;
    }
    __syncthreads();
    if (wave > 0 || !fvalid) return;
    double* out = Opart + ((size_t)blockIdx.y * nbins_all + (size_t)prob * F + f) * NS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double a = sr[m], b = si[m];
#pragma unroll
        for (int v = 0; v < kWaves - 1; ++v) {
            a += red[v][2 * m][lane];
            b += red[v][2 * m + 1][lane];
        }
        out[2 * m] = a;
        out[2 * m + 1] = b;
    }
#pragma unroll
    for (int v = 0; v < kWaves - 1; ++v) z += red[v][2 * M][lane];
    out[2 * M] = z;
}

// ---------------------------------------------------------------------------------------------
// per-bin step, ive.py:228-246: ogive_step_kernel's arithmetic with x_psi = s / zeta from the split partials (added in split
// order) and the stopping rule of each problem.  MP lanes per bin; grid = (bin groups of the problem, 1, problem).  The last
// workgroup of a problem (its ticket) folds the problem's max ||delta||, counts the epoch and sets done when max < tol.
// ---------------------------------------------------------------------------------------------
template <int MP>
__global__ __launch_bounds__(64) void batch_ogive_step_kernel(OgiveBatchState sb, const double* __restrict__ Opart, int osplit, int F,
                                                              int M, int nbins_all, double mu, double tol) {
    constexpr int kBins = 64 / MP;
    __shared__ Zb sv[kBins][MP];
    __shared__ double sr[kBins][MP];
    __shared__ double sdn[kBins];
    const int prob = blockIdx.z;
    if (sb.done[prob]) return;                                           // uniform over the problem's workgroups in this epoch
    const OgiveState& st = sb.bin;
    const int g = threadIdx.x / MP, i = threadIdx.x % MP;
    const int fraw = blockIdx.x * kBins + g;
    const bool live = fraw < F && i < M;
    const int ic = i < M ? i : M - 1;                                    // padding lanes shadow a real one and store nothing
    const size_t f = (size_t)prob * F + (fraw < F ? fraw : F - 1);
    const int NA = M * M;
    const int NS = 2 * M + 1;
    auto sum_seq = [&](double term) {                                    // sum_j term_j, j ascending, on every lane of the bin
        __syncthreads();
        sr[g][i] = term;
        __syncthreads();
        double s = 0.;
#pragma unroll
        for (int j = 0; j < MP; ++j)
            if (j < M) s += sr[g][j];
        return s;
    };
    auto share = [&](Zb v) {
        __syncthreads();
        sv[g][i] = v;
        __syncthreads();
    };
    auto packed_entry = [&](const double* p, int j) -> Zb {              // entry (ic, j) of a packed Hermitian matrix
        if (j == ic) return {p[ic], 0.};
        const int lo = j < ic ? j : ic, hi = j < ic ? ic : j;
        const int o = herm_pair_index(M, lo, hi);
        return {p[o], j < ic ? -p[o + 1] : p[o + 1]};
    };
    const double2 w0 = st.What64[(f * M + ic) * M], a0 = st.A[f * M + ic];
    Zb w = {w0.x, w0.y}, a = {a0.x, a0.y};
    const bool do_a = st.DoA[f] != 0, do_w = st.DoW[f] != 0;
    // x_psi = (X^T psi) / zeta, ive.py:221-227: fixed-order sums of the frame-split partials
    double xre = 0., xim = 0., zeta = 0.;
    for (int sp = 0; sp < osplit; ++sp) {
        const double* o = Opart + ((size_t)sp * nbins_all + f) * NS;
        xre += o[2 * ic];
        xim += o[2 * ic + 1];
        zeta += o[2 * M];
    }
    const Zb xpsi = {xre / zeta, xim / zeta};
    const double* cx = st.Cx + f * NA;
    const double2* Ci = st.CxInv + (f * M + ic) * M;
    auto inv_row_times = [&]() {                                         // row ic of Cx^-1 times the shared vector
        Zb s = {0., 0.};
#pragma unroll
        for (int j = 0; j < MP; ++j)
            if (j < M) zacc(s, Zb{Ci[j].x, Ci[j].y}, sv[g][j]);
        return s;
    };
    Zb dl = {0., 0.};
    if (do_w) {                                                          // ive.py:231-232
        dl = {a.re - xpsi.re, a.im - xpsi.im};
        w = {w.re + mu * dl.re, w.im + mu * dl.im};
    }
    share(do_w ? w : xpsi);
    Zb t = {0., 0.};
    if (do_w) {                                                          // ive.py:240 -> :136-139: a = Cx w / Re(w^H Cx w)
#pragma unroll
        for (int j = 0; j < MP; ++j)
            if (j < M) zacc(t, packed_entry(cx, j), sv[g][j]);
    } else if (do_a) {                                                   // ive.py:236-237
        t = inv_row_times();
        const double la = st.Lambda[f];
        dl = {w.re - t.re * la, w.im - t.im * la};
        a = {a.re + mu * dl.re, a.im + mu * dl.im};
    }
    const double wcw = sum_seq(do_w ? w.re * t.re + w.im * t.im : 0.);
    if (do_w) {
        const double l = 1.0 / wcw;
        a = {t.re * l, t.im * l};
    }
    const double dsq = sum_seq(dl.re * dl.re + dl.im * dl.im);
    const bool stepped = do_w || do_a;
    // lambda_a = 1 / Re(a^H Cx^-1 a) for every bin, w = lambda_a Cx^-1 a where the mixing step ran (ive.py:141-144)
    share(a);
    t = inv_row_times();
    const double la = 1.0 / sum_seq(a.re * t.re + a.im * t.im);
    if (do_a) w = {t.re * la, t.im * la};
    const double dn = stepped ? sqrt(dsq) : st.Dnorm[f];                 // bins without a step keep their last delta
    if (live) {
        st.A[f * M + i] = make_double2(a.re, a.im);
        st.What64[(f * M + i) * M] = make_double2(w.re, w.im);
        st.What[(f * M + i) * M] = make_float2((float)w.re, (float)w.im);
        if (stepped) st.Delta[f * M + i] = make_double2(dl.re, dl.im);
        if (i == 0) {
            st.Lambda[f] = la;
            if (stepped) st.Dnorm[f] = dn;
        }
    }
    // stopping rule of this problem: a non-negative double orders like its bit pattern and every NaN sorts above +inf, which is
    // numpy's rule too (the max of an array holding NaN is NaN, NaN < tol is False).  The max is order-free (atomicMax on the
    // bits); the hand-off to the problem's last workgroup is an agent-scope release (fence + ticket) / acquire (ticket + fence).
    if (i == 0) sdn[g] = fraw < F ? dn : 0.;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long top = 0;
        for (int k = 0; k < kBins; ++k) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(sdn[k]) & 0x7fffffffffffffffull;
            top = bits > top ? bits : top;
        }
        __hip_atomic_fetch_max(sb.runmax + prob, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned prev = __hip_atomic_fetch_add(sb.ticket + prob, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __threadfence();
            const unsigned long long bits = __hip_atomic_exchange(sb.runmax + prob, 0ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            const double mx = __longlong_as_double((long long)bits);
            __hip_atomic_store(sb.ticket + prob, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sb.epochs[prob] += 1;
            sb.maxdelta[prob] = mx;
            if (mx < tol) sb.done[prob] = 1;
        }
    }
}

#define OIVA_OGB_DISPATCH_M(CALL) \
    switch (M) {                  \
        case 1: CALL(1); break;   \
        case 2: CALL(2); break;   \
        case 3: CALL(3); break;   \
        case 4: CALL(4); break;   \
        case 5: CALL(5); break;   \
        case 6: CALL(6); break;   \
        case 7: CALL(7); break;   \
        case 8: CALL(8); break;   \
        default: return hipErrorInvalidValue; \
    }

}  // namespace

hipError_t launch_batch_ogive_switch(hipStream_t s, const OgiveBatchState& st, int B, int F, int M) {
    const dim3 grid((unsigned)((F + 63) / 64), 1, (unsigned)B);
#define CALL(MM) hipLaunchKernelGGL((batch_ogive_switch_kernel<MM>), grid, dim3(64), 0, s, st, F)
    OIVA_OGB_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_batch_ogive_power(hipStream_t s, const float2* X, const float2* What, float* Ppart, const int* done, int B, int T, int F,
                                    int M, int nsplit, int tcp) {
    const int nb = (F + kBinsPerWave * kWaves - 1) / (kBinsPerWave * kWaves);
    const dim3 grid((unsigned)nb, (unsigned)nsplit, (unsigned)B);
    const size_t shmem = (size_t)kWaves * tcp * sizeof(float);
    if (tcp > kPowMaxFrames) return hipErrorInvalidValue;
#define CALL(MM) hipLaunchKernelGGL((batch_ogive_power_kernel<MM>), grid, dim3(kBlock), shmem, s, X, What, Ppart, done, T, F, tcp)
    OIVA_OGB_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_batch_ogive_activation(hipStream_t s, const float* parts, int nparts, float* R, size_t r_stride, const int* done, int B,
                                         int T, int amodel, int F) {
    const dim3 grid((unsigned)rsum_blocks(T), 1, (unsigned)B);
    const float inv = 1.f / (float)F;
    if (nparts <= 8)
        hipLaunchKernelGGL(batch_ogive_activation_kernel<8>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, done, T, amodel, inv);
    else if (nparts <= 16)
        hipLaunchKernelGGL(batch_ogive_activation_kernel<16>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, done, T, amodel, inv);
    else
        hipLaunchKernelGGL(batch_ogive_activation_kernel<32>, grid, dim3(kBlock), 0, s, parts, nparts, R, r_stride, done, T, amodel, inv);
    return hipGetLastError();
}

hipError_t launch_batch_ogive_framesum(hipStream_t s, const float2* X, const double2* What64, const float* R, size_t r_stride,
                                       const int* done, double* Opart, int B, int T, int F, int M, int osplit, int otc) {
    const dim3 grid((unsigned)((F + kOgSumBins - 1) / kOgSumBins), (unsigned)osplit, (unsigned)B);
    const int nbins_all = B * F;
#define CALL(MM)                                                                                                                      \
    hipLaunchKernelGGL((batch_ogive_framesum_kernel<MM>), grid, dim3(kBlock), 0, s, X, What64, R, r_stride, done, Opart, T, F, otc, \
                       nbins_all)
    OIVA_OGB_DISPATCH_M(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_batch_ogive_step(hipStream_t s, const OgiveBatchState& st, const double* Opart, int osplit, int B, int F, int M, double mu,
                                   double tol) {
    if (M < 1 || M > 8) return hipErrorInvalidValue;
    const int mp = M <= 4 ? 4 : 8;
    const dim3 grid((unsigned)((F + 64 / mp - 1) / (64 / mp)), 1, (unsigned)B);
    const int nbins_all = B * F;
    if (mp == 4)
        hipLaunchKernelGGL(batch_ogive_step_kernel<4>, grid, dim3(64), 0, s, st, Opart, osplit, F, M, nbins_all, mu, tol);
    else
        hipLaunchKernelGGL(batch_ogive_step_kernel<8>, grid, dim3(64), 0, s, st, Opart, osplit, F, M, nbins_all, mu, tol);
    return hipGetLastError();
}

}  // namespace oiva
