// The device bodies of BSS Eval shared by kernels_bsseval.hip (one estimate set per handle) and kernels_bsssets.hip
// (many estimate sets per reference set).  A kernel of either file resolves, from its grid, the room, the set and the matrix it works on
// and hands the body pointers that start there; every sum below is a chain owned by one element (a lane's lag, a right-hand-side
// column, a vector's accumulator, a pair), so an element gets the same bits whichever kernel runs its chain.
#pragma once
#include "oiva_device.h"

namespace oiva {

constexpr int kBssTile = 128;             // samples of the lag pass staged per step
constexpr int kBssLagLanes = 256;         // lags per workgroup of the lag pass: one per lane
constexpr int kBssPad = kBssBlock + 1;    // row stride of a staged tile: column reads by consecutive lanes spread over the banks
constexpr int kBssMaxVec = kBssMaxSrc * kBssMaxSrc + kBssMaxSrc;

// ---------------------------------------------------------------------------------------------
// lag sums of samples [u0, u1) of one signal b (n samples) against the N references a (N, n): lane = lag tau0 + threadIdx.x, N
// accumulators, one per reference s_i, and the energy of b at the lane's lag.  A step stages kBssTile samples of the N references and
// kBssTile + 256 of b; its products are added in ascending u from zero and the step's sum is then added to the segment's: chains of
// kBssTile and of kBssSeg / kBssTile additions, not one of kBssSeg (the SAR subtracts numbers a thousand times its denominator and
// answers to the last bits of G, D and E: DESIGN.md 3.10).
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void bss_lag_body(const double* __restrict__ a, const double* __restrict__ b, int n, int u0, int u1, int tau0,
                                             double (&acc)[N], double& accE) {
    constexpr int NP = (N + 1) & ~1;
    __shared__ __attribute__((aligned(16))) double sa[kBssTile][NP];
    __shared__ double sb[kBssTile + kBssLagLanes];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.;
    accE = 0.;
    for (int t0 = u0; t0 < u1; t0 += kBssTile) {
        const int len = min(kBssTile, u1 - t0);
        for (int idx = tid; idx < kBssTile * N; idx += kBssLagLanes) {
            const int i = idx / kBssTile;
            const int u = idx - i * kBssTile;
            sa[u][i] = u < len ? a[(size_t)i * n + t0 + u] : 0.;
        }
        for (int idx = tid; idx < kBssTile + kBssLagLanes; idx += kBssLagLanes) {
            const long long g = (long long)t0 + tau0 + idx;
            sb[idx] = g < n ? b[g] : 0.;
        }
        __syncthreads();
        double tile[N];
#pragma unroll
        for (int i = 0; i < N; ++i) tile[i] = 0.;
        double tileE = 0.;
#pragma unroll 4
        for (int u = 0; u < len; ++u) {
            const double bv = sb[u + tid];
#pragma unroll
            for (int i = 0; i < N; ++i) tile[i] = fma(sa[u][i], bv, tile[i]);
            tileE = fma(bv, bv, tileE);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += tile[i];
        accE += tileE;
        __syncthreads();
    }
}

// the nseg partial sums that lie `stride` apart, added in order
__device__ __forceinline__ double bss_seg_sum(const double* __restrict__ part, size_t stride, int nseg) {
    double s = 0.;
    for (int g = 0; g < nseg; ++g) s += part[(size_t)g * stride];
    return s;
}

// ---------------------------------------------------------------------------------------------
// assembly of one room from its reference lag sums lg[i][j][tau] (row stride N Lf, rows x < N): G and the copy to be factored, both
// triangles, matrix `mat` of the launch; the diagonal blocks once more as the small systems; the pivot threshold of the room.
// r_ij[tau] is read as it was summed for tau >= 0 and from the mirrored pair for tau < 0, so G is symmetric to the bit.
// Grid: x = 256 columns, y = row.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void bss_assemble_body(const double* __restrict__ lg, double* __restrict__ G, double* __restrict__ Gf,
                                                  double* __restrict__ Hf, double* __restrict__ thr, int room, int mat, int N, int Lf) {
    const int nt = N * Lf;
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;
    if (row == 0 && col == 0) {
        double md = 0.;
        for (int i = 0; i < N; ++i) md = fmax(md, lg[((size_t)i * N + i) * Lf]);
        thr[room] = (double)nt * 2.220446049250313e-16 * md;
    }
    if (col >= nt) return;
    const int i = row / Lf, p = row - i * Lf;
    const int j = col / Lf, q = col - j * Lf;
    const int tau = p - q;
    double v;
    if (tau > 0)
        v = lg[((size_t)j * N + i) * Lf + tau];
    else if (tau < 0)
        v = lg[((size_t)i * N + j) * Lf - tau];
    else
        v = lg[((size_t)max(i, j) * N + min(i, j)) * Lf];
    const size_t at = ((size_t)mat * nt + row) * nt + col;
    G[at] = v;
    Gf[at] = v;
    if (i == j) Hf[(((size_t)mat * N + j) * Lf + p) * Lf + q] = v;
}

// C[room][k] = D_k and c[room][j][k] = D_k[j] from the room's D (N, N Lf): the right-hand sides, overwritten by the substitutions
__device__ __forceinline__ void bss_init_rhs_body(const double* __restrict__ Droom, double* __restrict__ C, double* __restrict__ c, int room,
                                                  int N, int Lf) {
    const int nt = N * Lf;
    const int e = blockIdx.x * 256 + threadIdx.x;       // (k, j, p)
    if (e >= N * nt) return;
    const int k = e / nt, jp = e - k * nt;
    const int j = jp / Lf, p = jp - j * Lf;
    const double v = Droom[(size_t)k * nt + jp];
    C[((size_t)room * N + k) * nt + jp] = v;
    c[((((size_t)room * N + j) * N + k) * Lf) + p] = v;
}

// ---------------------------------------------------------------------------------------------
// substitution with the factor A (dim x dim, lower) of one matrix per workgroup of 256, R <= 8 right-hand sides X (R, dim): forward
// L y = x, or (BWD) backward L^T x = y.  Per block: the diagonal block by wave 0, lane = row, the solved element handed on by a
// shuffle; then the product of the solved block with every tile beside it leaves the rows still to come.
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__device__ __forceinline__ void bss_trsv_body(const double* __restrict__ A, int dim, double* __restrict__ X, int R) {
    constexpr int kNb = kBssBlock;
    __shared__ double T[kNb][kBssPad];
    __shared__ double Y[kNb][kBssMaxSrc];
    const int tid = threadIdx.x;
    const int nblk = (dim + kNb - 1) / kNb;
    for (int kk = 0; kk < nblk; ++kk) {
        const int k = BWD ? nblk - 1 - kk : kk;
        const int k0 = k * kNb;
        for (int idx = tid; idx < kNb * kNb; idx += 256) {
            const int r = idx / kNb, cc = idx - r * kNb;
            T[r][cc] = (k0 + r < dim && cc <= r) ? A[(size_t)(k0 + r) * dim + k0 + cc] : (r == cc ? 1. : 0.);
        }
        __syncthreads();
        if (tid < 64) {
            const int m = tid;
            double y[kBssMaxSrc];
#pragma unroll
            for (int r = 0; r < kBssMaxSrc; ++r) y[r] = (r < R && k0 + m < dim) ? X[(size_t)r * dim + k0 + m] : 0.;
            for (int s = 0; s < kNb; ++s) {
                const int cc = BWD ? kNb - 1 - s : s;
                const double piv = T[cc][cc];
                const double l = BWD ? (m < cc ? T[cc][m] : 0.) : (m > cc ? T[m][cc] : 0.);
#pragma unroll
                for (int r = 0; r < kBssMaxSrc; ++r) {
                    const double t = __shfl(y[r], cc, 64) / piv;
                    y[r] = m == cc ? t : fma(-l, t, y[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < kBssMaxSrc; ++r) {
                Y[m][r] = y[r];
                if (r < R && k0 + m < dim) X[(size_t)r * dim + k0 + m] = y[r];
            }
        }
        __syncthreads();
        const int jbeg = BWD ? 0 : k + 1, jend = BWD ? k : nblk;
        for (int j = jbeg; j < jend; ++j) {
            const int j0 = j * kNb;
            for (int idx = tid; idx < kNb * kNb; idx += 256) {
                const int r = idx / kNb, cc = idx - r * kNb;
                if (BWD)      // rows of block k, columns of block j: T[c][m]
                    T[r][cc] = k0 + r < dim ? A[(size_t)(k0 + r) * dim + j0 + cc] : 0.;
                else          // rows of block j, columns of block k: T[m][c]
                    T[r][cc] = j0 + r < dim ? A[(size_t)(j0 + r) * dim + k0 + cc] : 0.;
            }
            __syncthreads();
            const int m = tid & 63;
            for (int r = tid >> 6; r < R; r += 4) {
                double acc = 0.;
                for (int cc = 0; cc < kNb; ++cc) acc = fma(BWD ? T[cc][m] : T[m][cc], Y[cc][r], acc);
                if (j0 + m < dim) X[(size_t)r * dim + j0 + m] -= acc;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------
// quadratic forms v^T Q v of nvec vectors with one matrix Q (row stride N Lf: the unfactored G of a room, or -- SMALL -- its block
// G_jj): one workgroup of 256 per 64 rows (blockIdx.x); lane = row, wave w owns vectors w, w + 4, ...  Per vector the block's share
// sum_m v[m] (Q v)[m] is written to q[vector][row block], the rows added in ascending order; the criteria body adds the blocks.
//   large: vector v < nd is d = C_k - embed_j(c_kj) for pair (k, j) = (v / N, v % N), or (v, v) when only the pairs k = j are
//          evaluated (nd = N); vector nd + k is C_k
//   small: vector k is c_kj, j the block
// C and c are those of one estimate set, indexed by the room of the batch.
// ---------------------------------------------------------------------------------------------
template <bool SMALL>
__device__ __forceinline__ double bss_vec(const double* __restrict__ C, const double* __restrict__ c, int room, int jblk, int v, int e,
                                          int N, int Lf, int nd) {
    if (SMALL) return c[(((size_t)room * N + jblk) * N + v) * Lf + e];
    const int nt = N * Lf;
    if (v >= nd) return C[((size_t)room * N + (v - nd)) * nt + e];
    const int k = nd == N ? v : v / N, j = nd == N ? v : v - k * N;
    const double big = C[((size_t)room * N + k) * nt + e];
    const int ej = e - j * Lf;
    return (ej >= 0 && ej < Lf) ? big - c[(((size_t)room * N + j) * N + k) * Lf + ej] : big;
}

template <bool SMALL>
__device__ __forceinline__ void bss_quad_body(const double* __restrict__ Q, const double* __restrict__ C, const double* __restrict__ c,
                                              double* __restrict__ q, int N, int Lf, int nd, int nvec, int room, int jblk) {
    constexpr int kNb = kBssBlock;
    __shared__ double T[kNb][kBssPad];
    __shared__ double V[kNb][kBssMaxVec + 1];
    const int tid = threadIdx.x;
    const int nt = N * Lf;
    const int dim = SMALL ? Lf : nt;
    const int nrb = (dim + kNb - 1) / kNb;
    const int r0 = blockIdx.x * kNb;
    const int m = tid & 63, w = tid >> 6;
    constexpr int kPer = (kBssMaxVec + 3) / 4;
    double acc[kPer];
#pragma unroll
    for (int s = 0; s < kPer; ++s) acc[s] = 0.;
    for (int c0 = 0; c0 < dim; c0 += kNb) {
        for (int idx = tid; idx < kNb * kNb; idx += 256) {
            const int r = idx / kNb, cc = idx - r * kNb;
            T[r][cc] = (r0 + r < dim && c0 + cc < dim) ? Q[(size_t)(r0 + r) * nt + c0 + cc] : 0.;
        }
        for (int idx = tid; idx < kNb * nvec; idx += 256) {
            const int cc = idx / nvec, v = idx - cc * nvec;
            V[cc][v] = c0 + cc < dim ? bss_vec<SMALL>(C, c, room, jblk, v, c0 + cc, N, Lf, nd) : 0.;
        }
        __syncthreads();
        for (int cc = 0; cc < kNb; ++cc) {
            const double g = T[m][cc];
#pragma unroll
            for (int s = 0; s < kPer; ++s)
                if (w + 4 * s < nvec) acc[s] = fma(g, V[cc][w + 4 * s], acc[s]);
        }
        __syncthreads();
    }
    // the rows of this block: V[m][v] <- v[m] * (Q v)[m], then one lane per vector adds the 64 rows in order
#pragma unroll
    for (int s = 0; s < kPer; ++s) {
        const int v = w + 4 * s;
        if (v < nvec) V[m][v] = r0 + m < dim ? bss_vec<SMALL>(C, c, room, jblk, v, r0 + m, N, Lf, nd) * acc[s] : 0.;
    }
    __syncthreads();
    if (tid < nvec) {
        double s = 0.;
        for (int r = 0; r < kNb; ++r) s += V[r][tid];
        q[(size_t)tid * nrb + blockIdx.x] = s;
    }
}

__device__ __forceinline__ double bss_db(double num, double den) { return den > 0. ? 10. * log10(num / den) : (double)INFINITY; }

// one workgroup of 256 per pair v = blockIdx.x of one room: the two inner products with D_k (lane-strided sums closed by the fixed
// tree of block_sum), the block sums of the quadratic forms, the three ratios.  Droom: the room's D (N, N Lf); E, C, c and the
// results: one estimate set's, indexed by the room of the batch; qLroom, qSroom: the room's rows of the quadratic forms
__device__ __forceinline__ void bss_criteria_body(const double* __restrict__ Droom, const double* __restrict__ E, const double* __restrict__ C,
                                                  const double* __restrict__ c, const double* __restrict__ qLroom,
                                                  const double* __restrict__ qSroom, double* __restrict__ sdr, double* __restrict__ sir,
                                                  double* __restrict__ sar, int N, int Lf, int nd, int room) {
    constexpr int kNb = kBssBlock;
    __shared__ double red[kWaves];
    const int tid = threadIdx.x;
    const int v = blockIdx.x;
    const int k = nd == N ? v : v / N, j = nd == N ? v : v - k * N;
    const int nt = N * Lf;
    const double* Dk = Droom + (size_t)k * nt;
    const double* Ck = C + ((size_t)room * N + k) * nt;
    const double* ckj = c + (((size_t)room * N + j) * N + k) * Lf;
    double s1 = 0., s2 = 0.;
    for (int e = tid; e < Lf; e += 256) s1 = fma(Dk[(size_t)j * Lf + e], ckj[e], s1);
    for (int e = tid; e < nt; e += 256) s2 = fma(Dk[e], Ck[e], s2);
    const double d_small = block_sum(s1, red);
    const double d_big = block_sum(s2, red);
    if (tid != 0) return;
    const int nrbL = (nt + kNb - 1) / kNb, nrbS = (Lf + kNb - 1) / kNb;
    double a = 0., interf = 0., tot = 0.;
    for (int r = 0; r < nrbS; ++r) a += qSroom[((size_t)j * kBssMaxVec + k) * nrbS + r];
    for (int r = 0; r < nrbL; ++r) interf += qLroom[(size_t)v * nrbL + r];
    for (int r = 0; r < nrbL; ++r) tot += qLroom[(size_t)(nd + k) * nrbL + r];
    const double Ek = E[(size_t)room * N + k];
    const double res = Ek - 2. * d_small + a;
    const double art = Ek - 2. * d_big + tot;
    const size_t at = ((size_t)room * N + k) * N + j;
    sdr[at] = bss_db(a, res);
    sir[at] = N == 1 ? (double)INFINITY : bss_db(a, interf);
    sar[at] = bss_db(tot, art);
}

}  // namespace oiva
