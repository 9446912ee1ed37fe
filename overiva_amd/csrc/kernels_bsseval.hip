// Kernels of BSS Eval (bsseval.hip: oiva_bsseval_* and oiva_bsssets_*): SDR, SIR and SAR of S sets of estimates against one set
// of references, B rooms of N <= 8 sources, filter length Lf <= 512, rooms of their own lengths.  All arithmetic is float64
// (DESIGN.md 3.10).  A single evaluation is one set; the rooms run in groups of `rooms` from room g0 on when G does not fit for all.
//
//   sig       packed signals (sum_b N * n_b) per set, the sets sig_stride apart: room b holds its (N, n_b) signals, row-major, at
//             rooms[b].sig_off.  The references are a set like any other.
//   part      [room segment][set][k][i][Lf]: partial lag sums of one segment of kBssSeg samples;  Epart [room segment][set][k]
//   rlag      (B, N, N, Lf): rlag[b][x][i][tau] = sum_u s_i[u] s_x[u + tau]: the lag sums of the references against themselves
//   per set, the sets one after the other:  D (B, N, N Lf), the lag sums of the estimates;  E (B, N);  C (B, N, N Lf): D_k, then
//             G^-1 D_k;  c (B, N[j], N[k], Lf): D_k[j], then G_jj^-1 D_k[j];  crit 3 x (B, N, N);  qL (rooms, kBssMaxVec, blocks of
//             N Lf), qS (rooms, N, kBssMaxVec, blocks of Lf): quadratic forms per 64-row block of G / G_jj of the group's rooms,
//             added in block order by the criteria kernel
//   G, Gf     (rooms, N Lf, N Lf) both triangles, the second one factored in place (lower);  Hf (rooms * N, Lf, Lf): the blocks
//             G_jj; shared by the sets
//
// Every kernel resolves the room, the set and the matrix from its grid and hands the body of bss_arith.h pointers that start
// there; a workgroup never holds two rooms or two sets.  A launcher starts a group at room g0 by handing its kernels the arrays
// that are indexed by the room of the batch (rlag, thr, D, E, C, c, crit, flag) from room g0 on, so that a kernel counts rooms
// from the start of its group.  Every sum runs in an order that is a function of the
// room's own (n, N, Lf) and of the element's index: the lag sums run sample by sample inside 128-sample steps, the steps are added
// in order inside segments whose bounds follow from n alone and the segments are added in order; the factorisation, the
// substitutions and the quadratic forms walk 64-wide blocks in ascending order with one fixed order inside a block.  Nothing
// depends on B, on the room's place in the batch, on the lengths of the other rooms, on how the rooms are grouped for memory, on S,
// on the set's place among the sets or on the other sets.  A room therefore gets the same bits alone, in a larger batch, in a
// permuted one and in a ragged one, and a set the bits of a single evaluation of its signals.
//
// A flagged room (a pivot that is not finite or <= N Lf eps max_diag(G)) is skipped by every later kernel; the others run on.
#include "bss_arith.h"
#include "oiva_device.h"

namespace oiva {
namespace {

constexpr int kLagLanes = kBssLagLanes;
constexpr int kNb = kBssBlock;      // block size of the factorisation, the substitutions and the quadratic forms
constexpr int kPad = kBssPad;       // row stride of a staged tile
constexpr int kPadT = kNb + 2;      // row stride of a transposed panel: 16-byte aligned groups of four rows
constexpr int kMaxVec = kBssMaxVec;

__device__ __forceinline__ bool room_flagged(const int* flag, int room) { return flag[room] != 0; }

// ---------------------------------------------------------------------------------------------
// lag sums: one workgroup = (room, segment, (set, signal k), 256 lags) of S sets of N signals each, against the room's N
// references; the chain of a lane is bss_lag_body (bss_arith.h)
// ---------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(kLagLanes) void bss_lag_kernel(const double* __restrict__ ref, const double* __restrict__ sig,
                                                             long long sig_stride, const BssRoom* __restrict__ rooms,
                                                             const int2* __restrict__ segs, double* __restrict__ part,
                                                             double* __restrict__ Epart, int S, int Lf) {
    const int tid = threadIdx.x;
    const int2 rs = segs[blockIdx.x];
    const BssRoom r = rooms[rs.x];
    const int seg = rs.y;
    const int se = blockIdx.y / N, k = blockIdx.y - se * N;
    const int tau0 = blockIdx.z * kLagLanes;
    const int n = r.n;
    const double* a = ref + r.sig_off;
    const double* b = sig + (size_t)se * sig_stride + r.sig_off + (size_t)k * n;
    const int u0 = seg * kBssSeg;
    const int u1 = min(n, u0 + kBssSeg);
    double acc[N];
    double accE;
    bss_lag_body<N>(a, b, n, u0, u1, tau0, acc, accE);
    const int tau = tau0 + tid;
    const size_t row = ((size_t)r.seg_off + seg) * S + se;
    if (tau < Lf) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[((row * N + k) * N + i) * Lf + tau] = acc[i];
    }
    if (tau == 0) Epart[row * N + k] = accE;
}

// out[set][b][e] = sum over the room's segments, in order;  E[set][b][k] likewise.  Grid (elements, room, set)
__global__ __launch_bounds__(256) void bss_lag_sum_kernel(const BssRoom* __restrict__ rooms, const double* __restrict__ part,
                                                           const double* __restrict__ Epart, double* __restrict__ out,
                                                           double* __restrict__ E, int B, int S, int N, int Lf) {
    const BssRoom r = rooms[blockIdx.y];
    const int se = blockIdx.z;
    const size_t per = (size_t)N * N * Lf;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t first = (size_t)r.seg_off * S + se;
    if (e < per) out[((size_t)se * B + blockIdx.y) * per + e] = bss_seg_sum(part + first * per + e, (size_t)S * per, r.nseg);
    if (e < (size_t)N) E[((size_t)se * B + blockIdx.y) * N + e] = bss_seg_sum(Epart + first * N + e, (size_t)S * N, r.nseg);
}

// ---------------------------------------------------------------------------------------------
// assembly of gridDim.z rooms: G and the copy to be factored, both triangles; the diagonal blocks once more as
// the small systems; the pivot threshold of the room.  r_ij[tau] is read as it was summed for tau >= 0 and from the mirrored
// pair for tau < 0, so G is symmetric to the bit.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bss_assemble_kernel(const double* __restrict__ rlag, double* __restrict__ G, double* __restrict__ Gf,
                                                            double* __restrict__ Hf, double* __restrict__ thr, int N, int Lf) {
    const int room = blockIdx.z;
    bss_assemble_body(rlag + (size_t)room * N * N * Lf, G, Gf, Hf, thr, room, room, N, Lf);
}

// C[b][k] = D_k and c[b][j][k] = D_k[j]: the right-hand sides, overwritten by the substitutions.  Grid (elements, room, set); a
// flagged room keeps them as its C and c
__global__ __launch_bounds__(256) void bss_init_rhs_kernel(const double* __restrict__ D, double* __restrict__ C, double* __restrict__ c,
                                                            int B, int N, int Lf) {
    const int room = blockIdx.y;
    const size_t set = (size_t)blockIdx.z * B * N * N * Lf;
    bss_init_rhs_body(D + set + (size_t)room * N * N * Lf, C + set, c + set, room, N, Lf);
}

// ---------------------------------------------------------------------------------------------
// blocked Cholesky, right-looking, lower triangle in place, block size kNb.  Matrix m of the launch belongs to room
// g0 + m / per_room.  Step k0: the diagonal block (one workgroup per matrix), the panel below it (one wave per 64 rows), the
// trailing update (one workgroup per 64 x 64 tile of the lower triangle).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bss_chol_diag_kernel(double* __restrict__ A, long long stride, int dim, int k0, int* flag,
                                                             const double* __restrict__ thr, int g0, int per_room) {
    __shared__ double T[kNb][kPad];
    const int tid = threadIdx.x;
    const int room = g0 + blockIdx.x / per_room;
    if (room_flagged(flag, room)) return;
    A += (size_t)blockIdx.x * stride;
    const int nb = min(kNb, dim - k0);
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
        const int r = idx / kNb, cc = idx - r * kNb;
        T[r][cc] = (r < nb && cc <= r) ? A[(size_t)(k0 + r) * dim + k0 + cc] : 0.;
    }
    __syncthreads();
    const double tol = thr[room];
    for (int cc = 0; cc < nb; ++cc) {
        const double d = T[cc][cc];
        if (!(d > tol) || !isfinite(d)) {          // (uniform: every lane reads the same pivot)
            if (tid == 0) flag[room] = 1;
            return;
        }
        const double s = sqrt(d);
        __syncthreads();
        if (tid == cc)
            T[cc][cc] = s;
        else if (tid > cc && tid < nb)
            T[tid][cc] = T[tid][cc] / s;
        __syncthreads();
        for (int idx = tid; idx < kNb * kNb; idx += 256) {
            const int r = idx / kNb, q = idx - r * kNb;
            if (q > cc && r >= q && r < nb) T[r][q] = fma(-T[r][cc], T[q][cc], T[r][q]);
        }
        __syncthreads();
    }
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
        const int r = idx / kNb, cc = idx - r * kNb;
        if (r < nb && cc <= r) A[(size_t)(k0 + r) * dim + k0 + cc] = T[r][cc];
    }
}

// L_mk = A_mk L_kk^-T for the 64 rows of tile blockIdx.x below the diagonal block: lane = row, forward substitution in the LDS
__global__ __launch_bounds__(64) void bss_chol_panel_kernel(double* __restrict__ A, long long stride, int dim, int k0, const int* flag,
                                                             int g0, int per_room) {
    __shared__ double Lk[kNb][kPad];
    __shared__ double T[kNb][kPad];
    const int lane = threadIdx.x;
    if (room_flagged(flag, g0 + blockIdx.y / per_room)) return;
    A += (size_t)blockIdx.y * stride;
    const int r0 = k0 + kNb * (blockIdx.x + 1);
    const int nr = min(kNb, dim - r0);
    for (int r = 0; r < kNb; ++r) {
        Lk[r][lane] = lane <= r ? A[(size_t)(k0 + r) * dim + k0 + lane] : 0.;
        T[r][lane] = r < nr ? A[(size_t)(r0 + r) * dim + k0 + lane] : 0.;
    }
    __syncthreads();
    for (int cc = 0; cc < kNb; ++cc) {
        double acc = T[lane][cc];
        for (int j = 0; j < cc; ++j) acc = fma(-T[lane][j], Lk[cc][j], acc);
        T[lane][cc] = acc / Lk[cc][cc];
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) A[(size_t)(r0 + r) * dim + k0 + lane] = T[r][lane];
}

// A_mn -= L_mk L_nk^T for one 64 x 64 tile (m >= n) of the part behind block column k0; a lane owns 4 x 4 elements and adds the 64
// products of each in ascending order before the one subtraction
__global__ __launch_bounds__(256) void bss_chol_update_kernel(double* __restrict__ A, long long stride, int dim, int k0, const int* flag,
                                                               int g0, int per_room) {
    __shared__ __attribute__((aligned(16))) double Pm[kNb][kPadT];
    __shared__ __attribute__((aligned(16))) double Pn[kNb][kPadT];
    const int tid = threadIdx.x;
    if (room_flagged(flag, g0 + blockIdx.y / per_room)) return;
    A += (size_t)blockIdx.y * stride;
    int tm = (int)((sqrt(8. * blockIdx.x + 1.) - 1.) * .5);
    while ((tm + 1) * (tm + 2) / 2 <= (int)blockIdx.x) ++tm;
    while (tm * (tm + 1) / 2 > (int)blockIdx.x) --tm;
    const int tn = blockIdx.x - tm * (tm + 1) / 2;
    const int rm0 = k0 + kNb * (tm + 1), rn0 = k0 + kNb * (tn + 1);
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
        const int r = idx / kNb, cc = idx - r * kNb;
        Pm[cc][r] = rm0 + r < dim ? A[(size_t)(rm0 + r) * dim + k0 + cc] : 0.;
        Pn[cc][r] = rn0 + r < dim ? A[(size_t)(rn0 + r) * dim + k0 + cc] : 0.;
    }
    __syncthreads();
    const int ty = tid / 16, tx = tid % 16;
    double acc[4][4] = {};
#pragma unroll 4
    for (int cc = 0; cc < kNb; ++cc) {
        const double2 a01 = *reinterpret_cast<const double2*>(&Pm[cc][4 * ty]);
        const double2 a23 = *reinterpret_cast<const double2*>(&Pm[cc][4 * ty + 2]);
        const double2 b01 = *reinterpret_cast<const double2*>(&Pn[cc][4 * tx]);
        const double2 b23 = *reinterpret_cast<const double2*>(&Pn[cc][4 * tx + 2]);
        const double av[4] = {a01.x, a01.y, a23.x, a23.y};
        const double bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = rm0 + 4 * ty + i, q = rn0 + 4 * tx + j;
            if (r < dim && q <= r) A[(size_t)r * dim + q] -= acc[i][j];
        }
}

// ---------------------------------------------------------------------------------------------
// substitution with the factor of one matrix per workgroup, R <= 8 right-hand sides: bss_trsv_body (bss_arith.h).  Grid (matrix,
// set): matrix m belongs to room m / per_room; X of one set is (nmat, R, dim), the sets set_stride apart
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void bss_trsv_kernel(const double* __restrict__ A, long long stride, int dim, double* __restrict__ X,
                                                        long long set_stride, int R, const int* __restrict__ flag, int per_room) {
    if (room_flagged(flag, blockIdx.x / per_room)) return;
    bss_trsv_body<BWD>(A + (size_t)blockIdx.x * stride, dim, X + (size_t)blockIdx.y * set_stride + (size_t)blockIdx.x * R * dim, R);
}

// quadratic forms v^T Q v of nvec vectors with one matrix Q (the unfactored G of a room, or -- SMALL -- its block G_jj): one
// workgroup per 64 rows, bss_quad_body (bss_arith.h).  Grid (row block, room or (room, j), set)
template <bool SMALL>
__global__ __launch_bounds__(256) void bss_quad_kernel(const double* __restrict__ G, const double* __restrict__ C, const double* __restrict__ c,
                                                        double* __restrict__ q, int B, int N, int Lf, int nd, int nvec,
                                                        const int* __restrict__ flag) {
    const int nt = N * Lf;
    const int room = SMALL ? blockIdx.y / N : blockIdx.y;
    const int jblk = SMALL ? blockIdx.y % N : 0;
    if (room_flagged(flag, room)) return;
    const int nrb = ((SMALL ? Lf : nt) + kNb - 1) / kNb;
    const double* Q = G + (size_t)room * nt * nt + (SMALL ? (size_t)jblk * Lf * (nt + 1) : 0);
    const size_t set = (size_t)blockIdx.z * B * N * nt;
    const size_t rows = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    bss_quad_body<SMALL>(Q, C + set, c + set, q + rows * kMaxVec * nrb, N, Lf, nd, nvec, room, jblk);
}

// one workgroup per (pair, room, set): bss_criteria_body (bss_arith.h)
__global__ __launch_bounds__(256) void bss_criteria_kernel(const double* __restrict__ D, const double* __restrict__ E,
                                                            const double* __restrict__ C, const double* __restrict__ c,
                                                            const double* __restrict__ qL, const double* __restrict__ qS,
                                                            double* __restrict__ crit, int B, int N, int Lf, int nd,
                                                            const int* __restrict__ flag) {
    const int room = blockIdx.y;
    if (room_flagged(flag, room)) return;
    const int nt = N * Lf;
    const int nrbL = (nt + kNb - 1) / kNb, nrbS = (Lf + kNb - 1) / kNb;
    const size_t se = blockIdx.z;
    const size_t set = se * B * N * nt, nn = (size_t)B * N * N, rows = se * gridDim.y + room;
    double* out = crit + se * 3 * nn;
    bss_criteria_body(D + set + (size_t)room * N * nt, E + se * B * N, C + set, c + set, qL + rows * kMaxVec * nrbL,
                      qS + rows * N * kMaxVec * nrbS, out, out + nn, out + 2 * nn, N, Lf, nd, room);
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
template <int N>
static hipError_t lag_launch(hipStream_t s, const double* ref, const double* sig, long long sig_stride, const BssRoom* rooms,
                             const int2* segs, long long total_segs, int S, int Lf, double* part, double* Epart) {
    const dim3 grid((unsigned)total_segs, N * S, (Lf + kLagLanes - 1) / kLagLanes);
    hipLaunchKernelGGL(bss_lag_kernel<N>, grid, dim3(kLagLanes), 0, s, ref, sig, sig_stride, rooms, segs, part, Epart, S, Lf);
    return hipGetLastError();
}

hipError_t launch_bss_lags(hipStream_t s, const double* ref, const double* sig, long long sig_stride, const BssRoom* rooms,
                           const int2* segs, long long total_segs, int B, int S, int N, int Lf, double* part, double* Epart, double* out,
                           double* E) {
    hipError_t e = hipErrorInvalidValue;
    switch (N) {
        case 1: e = lag_launch<1>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 2: e = lag_launch<2>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 3: e = lag_launch<3>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 4: e = lag_launch<4>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 5: e = lag_launch<5>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 6: e = lag_launch<6>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 7: e = lag_launch<7>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        case 8: e = lag_launch<8>(s, ref, sig, sig_stride, rooms, segs, total_segs, S, Lf, part, Epart); break;
        default: break;
    }
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((N * N * Lf + 255) / 256), B, S);
    hipLaunchKernelGGL(bss_lag_sum_kernel, grid, dim3(256), 0, s, rooms, part, Epart, out, E, B, S, N, Lf);
    return hipGetLastError();
}

hipError_t launch_bss_assemble(hipStream_t s, const double* rlag, double* G, double* Gf, double* Hf, double* thr, int g0, int rooms, int N,
                               int Lf) {
    const int nt = N * Lf;
    hipLaunchKernelGGL(bss_assemble_kernel, dim3((nt + 255) / 256, nt, rooms), dim3(256), 0, s, rlag + (size_t)g0 * N * nt, G, Gf, Hf,
                       thr + g0, N, Lf);
    return hipGetLastError();
}

hipError_t launch_bss_cholesky(hipStream_t s, double* A, int nmat, int dim, int* flag, const double* thr, int g0, int per_room) {
    const long long stride = (long long)dim * dim;
    const int nblk = (dim + kNb - 1) / kNb;
    for (int k = 0; k < nblk; ++k) {
        const int k0 = k * kNb, rest = nblk - 1 - k;
        hipLaunchKernelGGL(bss_chol_diag_kernel, dim3(nmat), dim3(256), 0, s, A, stride, dim, k0, flag, thr, g0, per_room);
        if (rest > 0) {
            hipLaunchKernelGGL(bss_chol_panel_kernel, dim3(rest, nmat), dim3(64), 0, s, A, stride, dim, k0, flag, g0, per_room);
            hipLaunchKernelGGL(bss_chol_update_kernel, dim3(rest * (rest + 1) / 2, nmat), dim3(256), 0, s, A, stride, dim, k0, flag, g0,
                               per_room);
        }
    }
    return hipGetLastError();
}

hipError_t launch_bss_solve(hipStream_t s, const double* Gf, const double* Hf, const double* D, double* C, double* c, int g0, int rooms,
                            int B, int S, int N, int Lf, const int* flag) {
    const int nt = N * Lf;
    const long long set = (long long)B * N * nt, big = (long long)nt * nt, small = (long long)Lf * Lf;
    const size_t at = (size_t)g0 * N * nt;      // the group's first room in D, C and c
    D += at, C += at, c += at, flag += g0;
    hipLaunchKernelGGL(bss_init_rhs_kernel, dim3((N * nt + 255) / 256, rooms, S), dim3(256), 0, s, D, C, c, B, N, Lf);
    hipLaunchKernelGGL(bss_trsv_kernel<false>, dim3(rooms, S), dim3(256), 0, s, Gf, big, nt, C, set, N, flag, 1);
    hipLaunchKernelGGL(bss_trsv_kernel<true>, dim3(rooms, S), dim3(256), 0, s, Gf, big, nt, C, set, N, flag, 1);
    hipLaunchKernelGGL(bss_trsv_kernel<false>, dim3(rooms * N, S), dim3(256), 0, s, Hf, small, Lf, c, set, N, flag, N);
    hipLaunchKernelGGL(bss_trsv_kernel<true>, dim3(rooms * N, S), dim3(256), 0, s, Hf, small, Lf, c, set, N, flag, N);
    return hipGetLastError();
}

hipError_t launch_bss_criteria(hipStream_t s, const double* D, const double* E, const double* G, const double* C, const double* c,
                               double* qL, double* qS, double* crit, int g0, int rooms, int B, int S, int N, int Lf, int diag_only,
                               const int* flag) {
    const int nt = N * Lf;
    const int nd = diag_only ? N : N * N;
    const size_t at = (size_t)g0 * N * nt;      // the group's first room in D, C and c
    D += at, C += at, c += at, E += (size_t)g0 * N, crit += (size_t)g0 * N * N, flag += g0;
    hipLaunchKernelGGL(bss_quad_kernel<false>, dim3((nt + kNb - 1) / kNb, rooms, S), dim3(256), 0, s, G, C, c, qL, B, N, Lf, nd, nd + N, flag);
    hipLaunchKernelGGL(bss_quad_kernel<true>, dim3((Lf + kNb - 1) / kNb, rooms * N, S), dim3(256), 0, s, G, C, c, qS, B, N, Lf, nd, N, flag);
    hipLaunchKernelGGL(bss_criteria_kernel, dim3(nd, rooms, S), dim3(256), 0, s, D, E, C, c, qL, qS, crit, B, N, Lf, nd, flag);
    return hipGetLastError();
}

}  // namespace oiva
