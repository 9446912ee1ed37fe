// Kernels of batched FIVE (five_batch, batch.hip: oiva_batch_five_*): the per-bin step of fast independent vector
// extraction, the smallest eigenpair of the Hermitian pencil (V_f, Cx_f) of every bin of B rooms, all in float64.
//
//   Cx     [B*F][M*M] float64, the input covariance packed as a Hermitian half (herm_pair_index), already divided by T_b
//   Vpart  [max nsplit][B*F][1][M*M] float64: the frame-split partials of the weighted covariance pass, packed, not divided
//   Li     (B*F, M, M) complex128, row major: the inverse of the lower Cholesky factor of Cx_f (zeros above the diagonal)
//   What64 (B*F, M, M) complex128, element [m][s]; the step writes column 0; What is its complex64 copy
//
// Both kernels give 16 lanes to a bin, so a wavefront holds four bins and is a workgroup of its own: its barriers cost a wait
// for its own LDS traffic.  A bin's matrices are padded tiles [N][N + 1] of complex128 in LDS (N = M rounded up to even: a
// row stride of N + 1 slots of 16 bytes puts the N elements of a column on different slots).  The bin's room comes from the
// problem table (its T and its number of frame splits), so dense and ragged batches take one path.
//
// five_begin_kernel: right-looking Cholesky Cx = L L^H column by column, then L^-1 by forward substitution, lane c the column
//   c.  A pivot that is not positive gives inf or NaN, which stays: the room ends non-finite.
// five_update_kernel:
//   1. V = (sum of the room's nsplit partials in split order) / T_b
//   2. G = Li V, A = G Li^H (the lower half computed, the upper mirrored, the diagonal real)
//   3. cyclic Jacobi on A: the round-robin order of kernels_evd.hip, N/2 disjoint pairs per round; lanes < N/2 form the
//      rotations, the 16 lanes apply them to the columns of A and of the eigenvector matrix in place, then to the rows of A.
//      A sweep starts while off(A)^2 > 1e-30 diag(A)^2 (kernels_evd.hip's criterion); a bin that has met it is frozen while the
//      wavefront's other bins go on, so its bits are its own
//   4. lambda = the smallest diagonal entry (ties: the lowest index), u its eigenvector; w = Li^H u / sqrt(lambda)
//   5. column 0 of What64 and of What
// Orders of summation are functions of the bin's own M, T_b and nsplit alone: every dot product is one chain in ascending
// index, the sums over a tile are lane-strided and closed by the fixed butterfly over the bin's 16 lanes.  No atomics.
#include "oiva_device.h"

namespace oiva {
namespace {

constexpr int kFiveLanes = 16;                    // lanes of a bin
constexpr int kFiveBins = 64 / kFiveLanes;        // bins of a wavefront = of a workgroup
constexpr int kFiveMaxSweeps = 30;

struct Zd {
    double re, im;
};
__device__ __forceinline__ Zd zmul(Zd a, Zd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Zd zmulc(Zd a, Zd b) { return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }   // a conj(b)
__device__ __forceinline__ Zd zconj(Zd a) { return {a.re, -a.im}; }
__device__ __forceinline__ Zd zsub(Zd a, Zd b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ Zd zadd(Zd a, Zd b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Zd zscale(Zd a, double c) { return {a.re * c, a.im * c}; }
// acc + a b and acc + a conj(b), each component one FMA chain
__device__ __forceinline__ Zd zfma(Zd a, Zd b, Zd acc) {
    return {fma(-a.im, b.im, fma(a.re, b.re, acc.re)), fma(a.im, b.re, fma(a.re, b.im, acc.im))};
}
__device__ __forceinline__ Zd zfmac(Zd a, Zd b, Zd acc) {
    return {fma(a.im, b.im, fma(a.re, b.re, acc.re)), fma(a.im, b.re, fma(-a.re, b.im, acc.im))};
}

// pair k of round r of the round-robin tournament on n (even) players (kernels_evd.hip)
__device__ __forceinline__ void pair_of(int n, int r, int k, int& p, int& q) {
    if (k == 0) {
        p = n - 1;
        q = r;
    } else {
        p = (r + k) % (n - 1);
        q = (r - k + (n - 1)) % (n - 1);
    }
}

// entry (i, j) of the Hermitian matrix packed at h (M real diagonals, then (re, im) of the entries c < d row by row)
__device__ __forceinline__ Zd herm_entry(const double* __restrict__ h, int M, int i, int j) {
    if (i == j) return {h[i], 0.};
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int o = herm_pair_index(M, lo, hi);
    return {h[o], i < j ? h[o + 1] : -h[o + 1]};
}

// sum over the bin's 16 lanes, the same bits in every one of them
__device__ __forceinline__ double bin_sum(double v) {
#pragma unroll
    for (int off = kFiveLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int N>
__global__ __launch_bounds__(64) void five_begin_kernel(const double* __restrict__ Cx, double2* __restrict__ Li, int nbins, int M) {
    __shared__ Zd C[kFiveBins][N][N + 1], R[kFiveBins][N][N + 1];
    const int g = threadIdx.x / kFiveLanes, lane = threadIdx.x % kFiveLanes;
    const int f = blockIdx.x * kFiveBins + g;
    const int fr = f < nbins ? f : nbins - 1;          // (a bin past the end repeats the last one and stores nothing)
    const double* cx = Cx + (size_t)fr * M * M;
    Zd(*c)[N + 1] = C[g];
    Zd(*r)[N + 1] = R[g];
    for (int e = lane; e < N * N; e += kFiveLanes) {
        const int i = e / N, j = e % N;
        c[i][j] = i < M && j < M ? herm_entry(cx, M, i, j) : Zd{0., 0.};
        r[i][j] = {0., 0.};
    }
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        const double inv = 1. / sqrt(c[j][j].re);      // inf or NaN where the pivot is not positive
        __syncthreads();
        if (lane >= j && lane < M) c[lane][j] = lane == j ? Zd{c[j][j].re * inv, 0.} : zscale(c[lane][j], inv);
        __syncthreads();
        for (int e = lane; e < N * N; e += kFiveLanes) {
            const int i = e / N, k = e % N;
            if (k > j && i >= k && i < M) c[i][k] = zsub(c[i][k], zmulc(c[i][j], c[k][j]));
        }
        __syncthreads();
    }
    // column `lane` of L^-1 by forward substitution: R[i][c] = -(sum_{k = c}^{i - 1} L[i][k] R[k][c]) / L[i][i]
    if (lane < M) {
        const int col = lane;
        r[col][col] = {1. / c[col][col].re, 0.};
        for (int i = col + 1; i < M; ++i) {
            Zd s = {0., 0.};
            for (int k = col; k < i; ++k) s = zfma(c[i][k], r[k][col], s);
            r[i][col] = zscale(s, -1. / c[i][i].re);
        }
    }
    __syncthreads();
    if (f < nbins)
        for (int e = lane; e < M * M; e += kFiveLanes) {
            const Zd v = r[e / M][e % M];
            Li[(size_t)f * M * M + e] = make_double2(v.re, v.im);
        }
}

template <int N>
__global__ __launch_bounds__(64) void five_update_kernel(const double* __restrict__ Vpart, const double2* __restrict__ Li,
                                                         double2* __restrict__ What64, float2* __restrict__ What,
                                                         const RaggedProblem* __restrict__ probs, int nbins, int F, int M) {
    constexpr int NP = N / 2;
    __shared__ Zd TA[kFiveBins][N][N + 1], TL[kFiveBins][N][N + 1], TE[kFiveBins][N][N + 1];
    __shared__ double RC[kFiveBins][NP];
    __shared__ Zd RS[kFiveBins][NP];
    const int g = threadIdx.x / kFiveLanes, lane = threadIdx.x % kFiveLanes;
    const int f = blockIdx.x * kFiveBins + g;
    const int fr = f < nbins ? f : nbins - 1;          // (a bin past the end repeats the last one and stores nothing)
    const int MM = M * M;
    const RaggedProblem d = probs[fr / F];
    Zd(*A)[N + 1] = TA[g];
    Zd(*L)[N + 1] = TL[g];
    Zd(*E)[N + 1] = TE[g];
    double* rc = RC[g];
    Zd* rs = RS[g];

    // ---- 1. V (into A's tile) and Li ------------------------------------------------------------------------------------------
    const size_t per_split = (size_t)nbins * MM;
    const double* vp = Vpart + (size_t)fr * MM;
    const double frames = (double)d.T;
    for (int e = lane; e < N * N; e += kFiveLanes) {
        const int i = e / N, j = e % N;
        Zd v = {0., 0.}, l = {0., 0.};
        if (i < M && j < M) {
            if (i <= j) {
                const int o = i == j ? i : herm_pair_index(M, i, j);
                double sr = 0., si = 0.;
                for (int s = 0; s < d.nsplit; ++s) {       // the room's own splits, in order
                    sr += vp[(size_t)s * per_split + o];
                    if (i != j) si += vp[(size_t)s * per_split + o + 1];
                }
                v = {sr / frames, si / frames};
                A[i][j] = v;
                if (i != j) A[j][i] = zconj(v);
            }
            const double2 q = Li[(size_t)fr * MM + i * M + j];
            l = {q.x, q.y};
        } else {
            A[i][j] = v;
        }
        L[i][j] = l;
    }
    __syncthreads();

    // ---- 2. G = Li V (into E's tile), then A = G Li^H -------------------------------------------------------------------------
    for (int e = lane; e < N * N; e += kFiveLanes) {
        const int i = e / N, j = e % N;
        Zd s = {0., 0.};
        for (int k = 0; k <= i; ++k) s = zfma(L[i][k], A[k][j], s);
        E[i][j] = s;
    }
    __syncthreads();
    for (int e = lane; e < N * N; e += kFiveLanes) {
        const int i = e / N, j = e % N;
        if (i >= j) {
            Zd s = {0., 0.};
            for (int k = 0; k <= j; ++k) s = zfmac(E[i][k], L[j][k], s);
            if (i == j) {
                A[i][i] = {s.re, 0.};
            } else {
                A[i][j] = s;
                A[j][i] = zconj(s);
            }
        }
    }
    __syncthreads();
    for (int e = lane; e < N * N; e += kFiveLanes) E[e / N][e % N] = {e / N == e % N ? 1. : 0., 0.};
    __syncthreads();

    // ---- 3. cyclic Jacobi -----------------------------------------------------------------------------------------------------
    for (int sweep = 0; sweep < kFiveMaxSweeps; ++sweep) {
        double off = 0., dg = 0.;
        for (int e = lane; e < N * N; e += kFiveLanes) {
            const Zd a = A[e / N][e % N];
            const double m = a.re * a.re + a.im * a.im;
            if (e / N == e % N) dg += m;
            else off += m;
        }
        off = bin_sum(off);
        dg = bin_sum(dg);
        const bool live = off > 1e-30 * dg;            // the same in the bin's 16 lanes; false for a NaN
        if (!__syncthreads_or(live ? 1 : 0)) break;
        for (int r = 0; r < N - 1; ++r) {
            if (live && lane < NP) {
                int p, q;
                pair_of(N, r, lane, p, q);
                const Zd apq = A[p][q];
                const double m = sqrt(apq.re * apq.re + apq.im * apq.im);
                double c = 1.;
                Zd se = {0., 0.};
                if (m > 1e-300) {
                    const double tau = (A[q][q].re - A[p][p].re) / (2. * m);
                    const double t = (tau >= 0. ? 1. : -1.) / (fabs(tau) + sqrt(1. + tau * tau));
                    c = 1. / sqrt(1. + t * t);
                    const double s = t * c;
                    se = {s * apq.re / m, s * apq.im / m};       // s e^{i phi}
                }
                rc[lane] = c;
                rs[lane] = se;
            }
            __syncthreads();
            // columns: (A J)[:, p] = A[:, p] c - A[:, q] conj(se);  (A J)[:, q] = A[:, p] se + A[:, q] c   (and E); the pairs of a
            // round are disjoint, so every item rewrites its own two entries
            if (live)
                for (int e = lane; e < N * NP; e += kFiveLanes) {
                    const int i = e / NP, k = e % NP;
                    int p, q;
                    pair_of(N, r, k, p, q);
                    const double c = rc[k];
                    const Zd se = rs[k];
                    const Zd ap = A[i][p], aq = A[i][q];
                    A[i][p] = zsub(zscale(ap, c), zmulc(aq, se));
                    A[i][q] = zadd(zmul(ap, se), zscale(aq, c));
                    const Zd vp2 = E[i][p], vq2 = E[i][q];
                    E[i][p] = zsub(zscale(vp2, c), zmulc(vq2, se));
                    E[i][q] = zadd(zmul(vp2, se), zscale(vq2, c));
                }
            __syncthreads();
            // rows: (J^H B)[p, :] = c B[p, :] - se B[q, :];  (J^H B)[q, :] = conj(se) B[p, :] + c B[q, :]
            if (live)
                for (int e = lane; e < N * NP; e += kFiveLanes) {
                    const int j = e / NP, k = e % NP;
                    int p, q;
                    pair_of(N, r, k, p, q);
                    const double c = rc[k];
                    const Zd se = rs[k];
                    const Zd bp = A[p][j], bq = A[q][j];
                    A[p][j] = zsub(zscale(bp, c), zmul(se, bq));
                    A[q][j] = zadd(zmulc(bp, se), zscale(bq, c));
                }
            __syncthreads();
        }
    }

    // ---- 4. the smallest eigenvalue, w = Li^H u / sqrt(lambda) ------------------------------------------------------------------
    int jmin = 0;
    double lam = A[0][0].re;
    for (int i = 1; i < M; ++i) {
        const double l = A[i][i].re;
        if (l < lam) {
            lam = l;
            jmin = i;
        }
    }
    if (lane < M && f < nbins) {
        Zd s = {0., 0.};
        for (int i = lane; i < M; ++i) s = zfmac(E[i][jmin], L[i][lane], s);      // conj(Li[i][m]) u[i]
        const double sc = 1. / sqrt(lam);
        const size_t o = ((size_t)f * M + lane) * M;
        What64[o] = make_double2(s.re * sc, s.im * sc);
        What[o] = make_float2((float)(s.re * sc), (float)(s.im * sc));
    }
}

}  // namespace

#define OIVA_FIVE_DISPATCH(kernel, ...)                                                        \
    switch ((M + 1) / 2) {                                                                    \
        case 1: hipLaunchKernelGGL(kernel<2>, grid, dim3(64), 0, s, __VA_ARGS__); break;       \
        case 2: hipLaunchKernelGGL(kernel<4>, grid, dim3(64), 0, s, __VA_ARGS__); break;       \
        case 3: hipLaunchKernelGGL(kernel<6>, grid, dim3(64), 0, s, __VA_ARGS__); break;       \
        case 4: hipLaunchKernelGGL(kernel<8>, grid, dim3(64), 0, s, __VA_ARGS__); break;       \
        default: return hipErrorInvalidValue;                                                 \
    }

hipError_t launch_five_begin(hipStream_t s, const double* Cx, double2* Li, int nbins, int M) {
    if (M < 1 || nbins < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nbins + kFiveBins - 1) / kFiveBins));
    OIVA_FIVE_DISPATCH(five_begin_kernel, Cx, Li, nbins, M)
    return hipGetLastError();
}

hipError_t launch_five_update(hipStream_t s, const double* Vpart, const double2* Li, double2* What64, float2* What,
                              const RaggedProblem* prob, int nbins, int F, int M) {
    if (M < 1 || nbins < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nbins + kFiveBins - 1) / kFiveBins));
    OIVA_FIVE_DISPATCH(five_update_kernel, Vpart, Li, What64, What, prob, nbins, F, M)
    return hipGetLastError();
}

#undef OIVA_FIVE_DISPATCH

}  // namespace oiva
