// Kernels of bss_eval_batch (bsseval.hip: oiva_bsseval_*): SDR, SIR and SAR of B rooms of N <= 8 sources, filter length
// Lf <= 512, rooms of their own lengths.  All arithmetic is float64.
//
//   ref, est  packed (sum_b N * n_b): room b holds its (N, n_b) references / estimates, row-major, at rooms[b].sig_off
//   part      per room [nseg][2N][N][Lf]: partial lag sums of one segment of kBssSeg samples;  Epart (sum nseg, N)
//   lag       (B, 2N, N, Lf): lag[b][x][i][tau] = sum_u s_i[u] b_x[u + tau], b_x = s_x (x < N) or e_{x-N}; D_k is lag[b][N + k]
//   G, Gf     (group, N Lf, N Lf) both triangles, the second one factored in place (lower);  Hf (group * N, Lf, Lf): the blocks G_jj
//   C         (B, N, N Lf): D_k, then G^-1 D_k;  c (B, N[j], N[k], Lf): D_k[j], then G_jj^-1 D_k[j]
//   qL, qS    quadratic forms per 64-row block of G / G_jj, added in block order by the criteria kernel
//
// The room comes from the grid and a workgroup never holds two rooms.  Every sum runs in an order that is a function of the
// room's own (n, N, Lf) and of the element's index: the lag sums run sample by sample inside 128-sample steps, the steps are added in order
// inside segments whose bounds follow from n alone and the segments are added in order; the factorisation, the substitutions and the quadratic forms walk 64-wide blocks in
// ascending order with one fixed order inside a block.  Nothing depends on B, on the room's place in the batch, on the lengths of
// the other rooms or on how the rooms are grouped for memory.  A room therefore gets the same bits alone, in a larger batch, in a
// permuted one and in a ragged one.
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
// lag sums: one workgroup = (room, segment, signal b_x, 256 lags); the chain of a lane is bss_lag_body (bss_arith.h)
// ---------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(kLagLanes) void bss_lag_kernel(const double* __restrict__ ref, const double* __restrict__ est,
                                                             const BssRoom* __restrict__ rooms, const int2* __restrict__ segs,
                                                             double* __restrict__ part, double* __restrict__ Epart, int Lf) {
    const int tid = threadIdx.x;
    const int2 rs = segs[blockIdx.x];
    const BssRoom r = rooms[rs.x];
    const int seg = rs.y;
    const int x = blockIdx.y;
    const int tau0 = blockIdx.z * kLagLanes;
    const int n = r.n;
    const double* a = ref + r.sig_off;
    const double* b = (x < N ? ref + r.sig_off + (size_t)x * n : est + r.sig_off + (size_t)(x - N) * n);
    const int u0 = seg * kBssSeg;
    const int u1 = min(n, u0 + kBssSeg);
    double acc[N];
    double accE;
    bss_lag_body<N>(a, b, n, u0, u1, tau0, acc, accE);
    const int tau = tau0 + tid;
    if (tau < Lf) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[r.part_off + (((size_t)seg * 2 * N + x) * N + i) * Lf + tau] = acc[i];
    }
    if (x >= N && tau == 0) Epart[((size_t)r.seg_off + seg) * N + (x - N)] = accE;
}

// lag[b][e] = sum over the room's segments, in order;  E[b][k] likewise
__global__ __launch_bounds__(256) void bss_lag_sum_kernel(const BssRoom* __restrict__ rooms, const double* __restrict__ part,
                                                           const double* __restrict__ Epart, double* __restrict__ lag,
                                                           double* __restrict__ E, int N, int Lf) {
    const BssRoom r = rooms[blockIdx.y];
    const size_t per = (size_t)2 * N * N * Lf;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < per) {
        lag[(size_t)blockIdx.y * per + e] = bss_seg_sum(part + r.part_off + e, per, r.nseg);
    }
    if (e < (size_t)N) {
        E[(size_t)blockIdx.y * N + e] = bss_seg_sum(Epart + (size_t)r.seg_off * N + e, N, r.nseg);
    }
}

// ---------------------------------------------------------------------------------------------
// assembly of rooms g0 .. g0 + gridDim.z - 1: G and the copy to be factored, both triangles; the diagonal blocks once more as
// the small systems; the pivot threshold of the room.  r_ij[tau] is read as it was summed for tau >= 0 and from the mirrored
// pair for tau < 0, so G is symmetric to the bit.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bss_assemble_kernel(const double* __restrict__ lag, double* __restrict__ G, double* __restrict__ Gf,
                                                            double* __restrict__ Hf, double* __restrict__ thr, int g0, int N, int Lf) {
    const int room = g0 + blockIdx.z;
    bss_assemble_body(lag + (size_t)room * 2 * N * N * Lf, G, Gf, Hf, thr, room, blockIdx.z, N, Lf);
}

// C[b][k] = D_k and c[b][j][k] = D_k[j]: the right-hand sides, overwritten by the substitutions
__global__ __launch_bounds__(256) void bss_init_rhs_kernel(const double* __restrict__ lag, double* __restrict__ C, double* __restrict__ c,
                                                            int g0, int N, int Lf) {
    const int room = g0 + blockIdx.y;
    bss_init_rhs_body(lag + ((size_t)room * 2 * N + N) * N * Lf, C, c, room, N, Lf);
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
// substitution with the factor of one matrix per workgroup, R <= 8 right-hand sides X (R, dim): bss_trsv_body (bss_arith.h)
// ---------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void bss_trsv_kernel(const double* __restrict__ A, long long stride, int dim, double* __restrict__ X,
                                                        int R, const int* flag, int g0, int per_room) {
    if (room_flagged(flag, g0 + blockIdx.x / per_room)) return;
    bss_trsv_body<BWD>(A + (size_t)blockIdx.x * stride, dim, X + (size_t)blockIdx.x * R * dim, R);
}

// quadratic forms v^T Q v of nvec vectors with one matrix Q (the unfactored G of a room, or -- SMALL -- its block G_jj): one
// workgroup per 64 rows, bss_quad_body (bss_arith.h)
template <bool SMALL>
__global__ __launch_bounds__(256) void bss_quad_kernel(const double* __restrict__ G, const double* __restrict__ C, const double* __restrict__ c,
                                                        double* __restrict__ q, int N, int Lf, int nd, int nvec, const int* flag, int g0) {
    const int nt = N * Lf;
    const int loc = SMALL ? blockIdx.y / N : blockIdx.y;        // room within the group
    const int jblk = SMALL ? blockIdx.y % N : 0;
    const int room = g0 + loc;
    if (room_flagged(flag, room)) return;
    const int nrb = ((SMALL ? Lf : nt) + kNb - 1) / kNb;
    const double* Q = G + (size_t)loc * nt * nt + (SMALL ? (size_t)jblk * Lf * (nt + 1) : 0);
    bss_quad_body<SMALL>(Q, C, c, q + (size_t)blockIdx.y * kMaxVec * nrb, N, Lf, nd, nvec, room, jblk);
}

// one workgroup per (pair, room): bss_criteria_body (bss_arith.h)
__global__ __launch_bounds__(256) void bss_criteria_kernel(const double* __restrict__ lag, const double* __restrict__ E,
                                                            const double* __restrict__ C, const double* __restrict__ c,
                                                            const double* __restrict__ qL, const double* __restrict__ qS,
                                                            double* __restrict__ sdr, double* __restrict__ sir, double* __restrict__ sar,
                                                            int N, int Lf, int nd, const int* flag, int g0) {
    const int loc = blockIdx.y, room = g0 + loc;
    if (room_flagged(flag, room)) return;
    const int nt = N * Lf;
    const int nrbL = (nt + kNb - 1) / kNb, nrbS = (Lf + kNb - 1) / kNb;
    bss_criteria_body(lag + ((size_t)room * 2 * N + N) * nt, E, C, c, qL + (size_t)loc * kMaxVec * nrbL,
                      qS + (size_t)loc * N * kMaxVec * nrbS, sdr, sir, sar, N, Lf, nd, room);
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
template <int N>
static hipError_t lag_launch(hipStream_t s, const double* ref, const double* est, const BssRoom* rooms, const int2* segs,
                             long long total_segs, int Lf, double* part, double* Epart) {
    const dim3 grid((unsigned)total_segs, 2 * N, (Lf + kLagLanes - 1) / kLagLanes);
    hipLaunchKernelGGL(bss_lag_kernel<N>, grid, dim3(kLagLanes), 0, s, ref, est, rooms, segs, part, Epart, Lf);
    return hipGetLastError();
}

hipError_t launch_bss_lags(hipStream_t s, const double* ref, const double* est, const BssRoom* rooms, const int2* segs,
                           long long total_segs, int B, int N, int Lf, double* part, double* Epart, double* lag, double* E) {
    hipError_t e = hipErrorInvalidValue;
    switch (N) {
        case 1: e = lag_launch<1>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 2: e = lag_launch<2>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 3: e = lag_launch<3>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 4: e = lag_launch<4>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 5: e = lag_launch<5>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 6: e = lag_launch<6>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 7: e = lag_launch<7>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        case 8: e = lag_launch<8>(s, ref, est, rooms, segs, total_segs, Lf, part, Epart); break;
        default: break;
    }
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((2 * N * N * Lf + 255) / 256), B);
    hipLaunchKernelGGL(bss_lag_sum_kernel, grid, dim3(256), 0, s, rooms, part, Epart, lag, E, N, Lf);
    return hipGetLastError();
}

hipError_t launch_bss_assemble(hipStream_t s, const double* lag, double* G, double* Gf, double* Hf, double* thr, double* C, double* c,
                               int g0, int rooms, int N, int Lf) {
    const int nt = N * Lf;
    hipLaunchKernelGGL(bss_assemble_kernel, dim3((nt + 255) / 256, nt, rooms), dim3(256), 0, s, lag, G, Gf, Hf, thr, g0, N, Lf);
    hipLaunchKernelGGL(bss_init_rhs_kernel, dim3((N * nt + 255) / 256, rooms), dim3(256), 0, s, lag, C, c, g0, N, Lf);
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

hipError_t launch_bss_solve(hipStream_t s, const double* A, int nmat, int dim, double* X, int R, const int* flag, int g0, int per_room) {
    const long long stride = (long long)dim * dim;
    hipLaunchKernelGGL(bss_trsv_kernel<false>, dim3(nmat), dim3(256), 0, s, A, stride, dim, X, R, flag, g0, per_room);
    hipLaunchKernelGGL(bss_trsv_kernel<true>, dim3(nmat), dim3(256), 0, s, A, stride, dim, X, R, flag, g0, per_room);
    return hipGetLastError();
}

hipError_t launch_bss_criteria(hipStream_t s, const double* lag, const double* E, const double* G, const double* C, const double* c,
                               double* qL, double* qS, double* sdr, double* sir, double* sar, int g0, int rooms, int N, int Lf,
                               int diag_only, const int* flag) {
    const int nt = N * Lf;
    const int nd = diag_only ? N : N * N;
    hipLaunchKernelGGL(bss_quad_kernel<false>, dim3((nt + kNb - 1) / kNb, rooms), dim3(256), 0, s, G, C, c, qL, N, Lf, nd, nd + N, flag, g0);
    hipLaunchKernelGGL(bss_quad_kernel<true>, dim3((Lf + kNb - 1) / kNb, rooms * N), dim3(256), 0, s, G, C, c, qS, N, Lf, nd, N, flag, g0);
    hipLaunchKernelGGL(bss_criteria_kernel, dim3(nd, rooms), dim3(256), 0, s, lag, E, C, c, qL, qS, sdr, sir, sar, N, Lf, nd, flag, g0);
    return hipGetLastError();
}

}  // namespace oiva
