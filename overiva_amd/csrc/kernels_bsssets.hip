// Kernels of bss_eval_sets_batch (bsssets.hip: oiva_bsssets_*): SDR, SIR and SAR of S estimate sets against one set of references,
// B rooms of N <= 8 sources, filter length Lf <= 512 ("Many estimate sets").  The reference half -- the lag sums
// r_ij, G, its factor and the factors of its diagonal blocks -- is made once; the kernels here are that half's lag pass and
// assembly, and the estimate half with a set axis in the grid.  The Cholesky kernels are those of kernels_bsseval.hip
// (launch_bss_cholesky).  Every chain of additions is a body of bss_arith.h, the one kernels_bsseval.hip runs: a set gets the bits
// of oiva_bsseval on the same signals, whatever S, its place among the sets and the other sets are.
//
//   sig       packed signals (sum_b N * n_b) per set, the sets sig_stride apart (the references: one set)
//   part      [room segment][set][k][i][Lf]: partial lag sums of one segment of kBssSeg samples;  Epart [room segment][set][k]
//   rlag      (B, N, N, Lf): rlag[b][x][i][tau] = sum_u s_i[u] s_x[u + tau]
//   per set, the sets one after the other:  D (B, N, N Lf);  E (B, N);  C (B, N, N Lf);  c (B, N[j], N[k], Lf);
//             qL (B, kBssMaxVec, blocks of N Lf);  qS (B, N, kBssMaxVec, blocks of Lf);  crit 3 x (B, N, N)
//   G, Gf     (B, N Lf, N Lf), Hf (B * N, Lf, Lf): shared by all sets, read-only after the preparation
//
// A flagged room (bss_chol_diag_kernel) is skipped by every kernel of the estimate half; the others run on.
#include "bss_arith.h"
#include "oiva_device.h"

namespace oiva {
namespace {

constexpr int kNb = kBssBlock;

// ---------------------------------------------------------------------------------------------
// lag sums: one workgroup = (room, segment, (set, signal k), 256 lags) of S sets of N signals each, against the room's N references
// ---------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(kBssLagLanes) void bsssets_lag_kernel(const double* __restrict__ ref, const double* __restrict__ sig,
                                                                    long long sig_stride, const BssRoom* __restrict__ rooms,
                                                                    const int2* __restrict__ segs, double* __restrict__ part,
                                                                    double* __restrict__ Epart, int S, int Lf) {
    const int tid = threadIdx.x;
    const int2 rs = segs[blockIdx.x];
    const BssRoom r = rooms[rs.x];
    const int seg = rs.y;
    const int se = blockIdx.y / N, k = blockIdx.y - se * N;
    const int tau0 = blockIdx.z * kBssLagLanes;
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
    if (Epart != nullptr && tau == 0) Epart[row * N + k] = accE;
}

// out[set][b][e] = sum over the room's segments, in order;  E[set][b][k] likewise (E may be null: the references)
__global__ __launch_bounds__(256) void bsssets_lag_sum_kernel(const BssRoom* __restrict__ rooms, const double* __restrict__ part,
                                                               const double* __restrict__ Epart, double* __restrict__ out,
                                                               double* __restrict__ E, int B, int S, int N, int Lf) {
    const BssRoom r = rooms[blockIdx.y];
    const int se = blockIdx.z;
    const size_t per = (size_t)N * N * Lf;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t first = (size_t)r.seg_off * S + se;
    if (e < per) out[((size_t)se * B + blockIdx.y) * per + e] = bss_seg_sum(part + first * per + e, (size_t)S * per, r.nseg);
    if (E != nullptr && e < (size_t)N) E[((size_t)se * B + blockIdx.y) * N + e] = bss_seg_sum(Epart + first * N + e, (size_t)S * N, r.nseg);
}

__global__ __launch_bounds__(256) void bsssets_assemble_kernel(const double* __restrict__ rlag, double* __restrict__ G,
                                                                double* __restrict__ Gf, double* __restrict__ Hf, double* __restrict__ thr,
                                                                int N, int Lf) {
    const int room = blockIdx.z;
    bss_assemble_body(rlag + (size_t)room * N * N * Lf, G, Gf, Hf, thr, room, room, N, Lf);
}

// grid (elements, room, set)
__global__ __launch_bounds__(256) void bsssets_init_rhs_kernel(const double* __restrict__ D, double* __restrict__ C, double* __restrict__ c,
                                                                int B, int N, int Lf, const int* __restrict__ flag) {
    const int room = blockIdx.y;
    if (flag[room] != 0) return;
    const size_t set = (size_t)blockIdx.z * B * N * N * Lf;
    bss_init_rhs_body(D + set + (size_t)room * N * N * Lf, C + set, c + set, room, N, Lf);
}

// grid (matrix, set): matrix m belongs to room m / per_room; X of one set is (nmat, R, dim), the sets set_stride apart
template <bool BWD>
__global__ __launch_bounds__(256) void bsssets_trsv_kernel(const double* __restrict__ A, long long stride, int dim, double* __restrict__ X,
                                                            long long set_stride, int R, const int* __restrict__ flag, int per_room) {
    if (flag[blockIdx.x / per_room] != 0) return;
    bss_trsv_body<BWD>(A + (size_t)blockIdx.x * stride, dim, X + (size_t)blockIdx.y * set_stride + (size_t)blockIdx.x * R * dim, R);
}

// grid (row block, room or (room, j), set)
template <bool SMALL>
__global__ __launch_bounds__(256) void bsssets_quad_kernel(const double* __restrict__ G, const double* __restrict__ C,
                                                            const double* __restrict__ c, double* __restrict__ q, int B, int N, int Lf, int nd,
                                                            int nvec, const int* __restrict__ flag) {
    const int nt = N * Lf;
    const int room = SMALL ? blockIdx.y / N : blockIdx.y;
    const int jblk = SMALL ? blockIdx.y % N : 0;
    if (flag[room] != 0) return;
    const int nrb = ((SMALL ? Lf : nt) + kNb - 1) / kNb;
    const double* Q = G + (size_t)room * nt * nt + (SMALL ? (size_t)jblk * Lf * (nt + 1) : 0);
    const size_t set = (size_t)blockIdx.z * B * N * nt;
    const size_t rows = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    bss_quad_body<SMALL>(Q, C + set, c + set, q + rows * kBssMaxVec * nrb, N, Lf, nd, nvec, room, jblk);
}

// grid (pair, room, set)
__global__ __launch_bounds__(256) void bsssets_criteria_kernel(const double* __restrict__ D, const double* __restrict__ E,
                                                                const double* __restrict__ C, const double* __restrict__ c,
                                                                const double* __restrict__ qL, const double* __restrict__ qS,
                                                                double* __restrict__ crit, int B, int N, int Lf, int nd,
                                                                const int* __restrict__ flag) {
    const int room = blockIdx.y;
    if (flag[room] != 0) return;
    const int nt = N * Lf;
    const int nrbL = (nt + kNb - 1) / kNb, nrbS = (Lf + kNb - 1) / kNb;
    const size_t se = blockIdx.z;
    const size_t set = se * B * N * nt, nn = (size_t)B * N * N;
    double* out = crit + se * 3 * nn;
    bss_criteria_body(D + set + (size_t)room * N * nt, E + se * B * N, C + set, c + set, qL + (se * B + room) * kBssMaxVec * nrbL,
                      qS + (se * B + room) * N * kBssMaxVec * nrbS, out, out + nn, out + 2 * nn, N, Lf, nd, room);
}

template <int N>
hipError_t lag_launch(hipStream_t s, const double* ref, const double* sig, long long sig_stride, const BssRoom* rooms, const int2* segs,
                      long long total_segs, int S, int Lf, double* part, double* Epart) {
    const dim3 grid((unsigned)total_segs, N * S, (Lf + kBssLagLanes - 1) / kBssLagLanes);
    hipLaunchKernelGGL(bsssets_lag_kernel<N>, grid, dim3(kBssLagLanes), 0, s, ref, sig, sig_stride, rooms, segs, part, Epart, S, Lf);
    return hipGetLastError();
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
hipError_t launch_bsssets_lags(hipStream_t s, const double* ref, const double* sig, long long sig_stride, const BssRoom* rooms,
                               const int2* segs, long long total_segs, int B, int S, int N, int Lf, double* part, double* Epart,
                               double* out, double* E) {
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
    hipLaunchKernelGGL(bsssets_lag_sum_kernel, grid, dim3(256), 0, s, rooms, part, Epart, out, E, B, S, N, Lf);
    return hipGetLastError();
}

hipError_t launch_bsssets_assemble(hipStream_t s, const double* rlag, double* G, double* Gf, double* Hf, double* thr, int B, int N, int Lf) {
    const int nt = N * Lf;
    hipLaunchKernelGGL(bsssets_assemble_kernel, dim3((nt + 255) / 256, nt, B), dim3(256), 0, s, rlag, G, Gf, Hf, thr, N, Lf);
    return hipGetLastError();
}

hipError_t launch_bsssets_solve(hipStream_t s, const double* Gf, const double* Hf, const double* D, double* C, double* c, int B, int S, int N,
                                int Lf, const int* flag) {
    const int nt = N * Lf;
    const long long set = (long long)B * N * nt;
    hipLaunchKernelGGL(bsssets_init_rhs_kernel, dim3((N * nt + 255) / 256, B, S), dim3(256), 0, s, D, C, c, B, N, Lf, flag);
    hipLaunchKernelGGL(bsssets_trsv_kernel<false>, dim3(B, S), dim3(256), 0, s, Gf, (long long)nt * nt, nt, C, set, N, flag, 1);
    hipLaunchKernelGGL(bsssets_trsv_kernel<true>, dim3(B, S), dim3(256), 0, s, Gf, (long long)nt * nt, nt, C, set, N, flag, 1);
    hipLaunchKernelGGL(bsssets_trsv_kernel<false>, dim3(B * N, S), dim3(256), 0, s, Hf, (long long)Lf * Lf, Lf, c, set, N, flag, N);
    hipLaunchKernelGGL(bsssets_trsv_kernel<true>, dim3(B * N, S), dim3(256), 0, s, Hf, (long long)Lf * Lf, Lf, c, set, N, flag, N);
    return hipGetLastError();
}

hipError_t launch_bsssets_criteria(hipStream_t s, const double* D, const double* E, const double* G, const double* C, const double* c,
                                   double* qL, double* qS, double* crit, int B, int S, int N, int Lf, int diag_only, const int* flag) {
    const int nt = N * Lf;
    const int nd = diag_only ? N : N * N;
    hipLaunchKernelGGL(bsssets_quad_kernel<false>, dim3((nt + kNb - 1) / kNb, B, S), dim3(256), 0, s, G, C, c, qL, B, N, Lf, nd, nd + N, flag);
    hipLaunchKernelGGL(bsssets_quad_kernel<true>, dim3((Lf + kNb - 1) / kNb, B * N, S), dim3(256), 0, s, G, C, c, qS, B, N, Lf, nd, N, flag);
    hipLaunchKernelGGL(bsssets_criteria_kernel, dim3(nd, B, S), dim3(256), 0, s, D, E, C, c, qL, qS, crit, B, N, Lf, nd, flag);
    return hipGetLastError();
}

}  // namespace oiva
