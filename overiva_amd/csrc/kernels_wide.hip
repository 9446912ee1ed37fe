// The wide path: every stage of the iteration for 17..32 channels                 reference overiva.py:87-199
//
// The kernels of 1..16 channels hold a bin's vectors and matrices in per-lane register arrays sized by the channel count; at
// 32 channels those arrays no longer fit.  The kernels here serve any 17 <= M <= 32 (kWideMax) and 1 <= K <= M with run-time
// M and K, and are selected by M alone (the launchers of kernels_cov.hip, kernels_demix.hip, kernels_update.hip and
// kernels_evd.hip hand over to them for M > kNarrowMax).  They keep every buffer layout of the narrow path: the packed
// Hermitian partials Vpart [nsplit][F][K][M*M], the per-64-bin partial powers Ppart [nb][T][K], the projection-back
// statistics Spart [nsplit][F][K][3].
//
//   covariance  V_k = sum_t w_k[t] x_t x_t^H  (overiva.py:179; :87 with unit weights).  One workgroup per (bin, frame split,
//               pass of sources).  With x = a + ib:  Re V = sum w (a a^T + b b^T),  Im V[c][d] = P[d][c] - P[c][d] with
//               P = sum w a b^T -- weighted Gram matrices with the frames as the contraction of the matrix instruction and the
//               channels on its 32 rows and columns (lanes >= M load zero):
//               v_mfma_f64_16x16x4_f64 on the four 16 x 16 blocks of Re and P, four frames per instruction of P and two per
//               instruction of Re: float64 sums of exact float64 products, in every arithmetic mode (`fast` and `mixed`
//               differ from `precise` in the per-bin algebra only here).  A float32 form on v_mfma_f32_32x32x2_f32 (1.5
//               instructions per frame, 128-frame chains folded into float64) measured 5.4 ms against 14.4 ms at
//               2048 x 4000 x 32 / 2 and passed the stage tests, but its end-to-end validation was not finished: not
//               shipped.
//   power       p[t,k] = sum over a 64-bin batch of |w_k^H x|^2 (overiva.py:140, :153/:155): one lane per bin, the
//               demixing vectors of the workgroup's 64 bins in LDS, the sum over the batch a fixed butterfly over the 64
//               lanes -- its order depends on the bin's place inside its batch of 64 only, as in the narrow kernels.
//   stats/write projection back and Y (overiva.py:192-199), same lane geometry.
//   update      the per-bin sequential algebra (overiva.py:176-190, the pending W /= wscale, the J initialisation of
//               :96-98,120-123): one workgroup of 256 threads per bin, every matrix in LDS, Gauss-Jordan elimination with
//               partial pivoting (rows never move: the pivot row is marked used), float64 in every mode.
#include "oiva_device.h"
#include "update_chain.h"

namespace oiva {
namespace {

constexpr int kWideKc64 = 2;        // sources per pass over X of the covariance kernel

// packed Hermitian entry e of an M x M matrix (herm_pair_index): row c, column d, part (0: real, 1: imaginary); c == d: diagonal
__device__ __forceinline__ void packed_entry(int M, int e, int& c, int& d, int& part) {
    if (e < M) {
        c = d = e;
        part = 0;
        return;
    }
    int q = (e - M) >> 1;
    part = (e - M) & 1;
    c = 0;
    while (q >= M - 1 - c) {
        q -= M - 1 - c;
        ++c;
    }
    d = c + 1 + q;
}

// ---------------------------------------------------------------------------------------------------------------------------
// covariance, float64 sums of exact float64 products on v_mfma_f64_16x16x4_f64: A/B lane l = row / column l & 15, contraction index l >> 4;
// C/D register r of lane l: row (l >> 4) + 4 r, column l & 15.  Blocks (I, J) of the 32 x 32 matrices: rows 16 I.., columns 16 J..
//   P  (4 frames per instruction): contraction index q = frame t + q;  A = w a[16 I + row], B = b[16 J + col]
//   Re (2 frames per instruction): q = (frame t + (q >> 1), part q & 1);  A = w u[16 I + row], B = u[16 J + col], u = a | b
// ---------------------------------------------------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(kBlock, 1) void wide_cov64_kernel(const float2* __restrict__ X, const double* __restrict__ Wt,
                                                               double* __restrict__ Vpart, int T, int F, int M, int K, int Kp, int tc) {
    __shared__ double tile[2][kWideMax][kWideMax + 1];     // Re and P of one source, summed over the waves
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rc = lane & 15, q = lane >> 4;
    const int f = blockIdx.x;
    const int k0 = blockIdx.z * KC;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const int NA = M * M;
    const size_t frame_stride = (size_t)F * M;
    const float2* pbin = X + (size_t)f * M;

    f64x4 re[KC][2][2], pp[KC][2][2];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int J = 0; J < 2; ++J)
#pragma unroll
                for (int r = 0; r < 4; ++r) re[kk][I][J][r] = pp[kk][I][J][r] = 0.;

    // channels rc and 16 + rc of frame t (zero past the split or past M)
    auto fetch = [&](int t, double (&a)[2], double (&b)[2]) {
        const bool live = t < t_end;
#pragma unroll
        for (int I = 0; I < 2; ++I) {
            const int c = 16 * I + rc;
            const bool ok = live && c < M;
            const float2 v = pbin[(size_t)(live ? t : T - 1) * frame_stride + (ok ? c : 0)];
            a[I] = ok ? (double)v.x : 0.;
            b[I] = ok ? (double)v.y : 0.;
        }
    };
    auto weight = [&](int t, int kk) {
        if (Wt == nullptr) return 1.;
        return t < t_end && k0 + kk < K ? Wt[(size_t)t * Kp + k0 + kk] : 0.;
    };
    // the waves take the groups of four frames in turn
    for (int t0 = t_begin + 4 * wave; t0 < t_end; t0 += 4 * kWaves) {
        double pa[2], pb[2], ra[2][2], rb[2][2];
        fetch(t0 + q, pa, pb);
        fetch(t0 + (q >> 1), ra[0], rb[0]);
        fetch(t0 + 2 + (q >> 1), ra[1], rb[1]);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const double wp = weight(t0 + q, kk);
            const double w0 = weight(t0 + (q >> 1), kk), w1 = weight(t0 + 2 + (q >> 1), kk);
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int J = 0; J < 2; ++J) {
                    pp[kk][I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(wp * pa[I], pb[J], pp[kk][I][J], 0, 0, 0);
                    const double u0i = (q & 1) ? rb[0][I] : ra[0][I], u0j = (q & 1) ? rb[0][J] : ra[0][J];
                    const double u1i = (q & 1) ? rb[1][I] : ra[1][I], u1j = (q & 1) ? rb[1][J] : ra[1][J];
                    re[kk][I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0 * u0i, u0j, re[kk][I][J], 0, 0, 0);
                    re[kk][I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1 * u1i, u1j, re[kk][I][J], 0, 0, 0);
                }
        }
    }
    // the waves' tiles added in a fixed order (wave 0..3), then the packed entries
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        for (int wv = 0; wv < kWaves; ++wv) {
            if (wave == wv) {
#pragma unroll
                for (int I = 0; I < 2; ++I)
#pragma unroll
                    for (int J = 0; J < 2; ++J)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * I + q + 4 * r, col = 16 * J + rc;
                            tile[0][row][col] = (wv == 0 ? 0. : tile[0][row][col]) + re[kk][I][J][r];
                            tile[1][row][col] = (wv == 0 ? 0. : tile[1][row][col]) + pp[kk][I][J][r];
                        }
            }
            __syncthreads();
        }
        if (k0 + kk < K) {
            double* out = Vpart + (((size_t)blockIdx.y * F + f) * K + k0 + kk) * NA;
            for (int e = tid; e < NA; e += kBlock) {
                int c, d, part;
                packed_entry(M, e, c, d, part);
                out[e] = part == 0 ? tile[0][c][d] : tile[1][d][c] - tile[1][c][d];
            }
        }
        __syncthreads();
    }
}

// float64 weights of the `precise` covariance: Wt[t][k] = 1 / max(r[t,k] / gamma_k, eps) (overiva.py:158-173); writes wscale
__global__ __launch_bounds__(kBlock) void wide_weights64_kernel(const float* __restrict__ R, double* __restrict__ Wt,
                                                                float* __restrict__ wscale, int model, int raw, int T, int K) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (long long)T * K) return;
    const int t = (int)(e / K), k = (int)(e - (long long)t * K);
    const double gamma = (raw & 1) ? 1. : gamma_of(R, T, K, k);
    double rn = (double)R[(size_t)t * K + k] / gamma;
    rn = rn < (double)kEpsR ? (double)kEpsR : rn;          // a NaN stays NaN, like r[r < eps] = eps in the reference
    Wt[e] = 1. / rn;
    if (t == 0 && wscale != nullptr && !(raw & 1))
        wscale[k] = model == OIVA_MODEL_LAPLACE ? (float)gamma : (float)sqrt(gamma);   // overiva.py:163 / :167
}

// ---------------------------------------------------------------------------------------------------------------------------
// demixing passes: one lane per bin of a 64-bin batch (grid.x), the waves take the frames of the split (grid.y) in turn,
// sources k0 .. k0 + KP - 1 (grid.z); conj(W[f][m][k]) of the batch in LDS as [kk][m][lane] (conflict-free reads)
// ---------------------------------------------------------------------------------------------------------------------------
enum { kWidePower = 0, kWideStats = 1, kWideWrite = 2 };

template <int KP, int MODE>
__global__ __launch_bounds__(kBlock) void wide_demix_kernel(const float2* __restrict__ X, const float2* __restrict__ What,
                                                            float* __restrict__ out, const float* __restrict__ Spart, int nsplit_s,
                                                            float2* __restrict__ Y, int T, int F, int M, int K, int tc) {
    __shared__ float2 wl[KP][kWideMax][64];
    __shared__ float red[kWaves][3 * KP][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x * 64 + lane;
    const bool fvalid = f < F;
    const int k0 = blockIdx.z * KP;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);

    for (int e = tid; e < KP * kWideMax * 64; e += kBlock) {
        const int kk = e / (kWideMax * 64), m = (e / 64) % kWideMax, b = e % 64;
        const int fb = blockIdx.x * 64 + b;
        float2 v = make_float2(0.f, 0.f);
        if (fb < F && m < M && k0 + kk < K) {
            const float2 w = What[((size_t)fb * M + m) * M + k0 + kk];
            v = make_float2(w.x, -w.y);
            if (MODE == kWideWrite && Spart != nullptr) {
                // y conj(z) = (conj(z) conj(w))^T x: fold the projection-back factor into the vector
                double sr = 0., si = 0., sd = 0.;
                for (int s = 0; s < nsplit_s; ++s) {
                    const float* p = Spart + (((size_t)s * F + fb) * K + k0 + kk) * 3;
                    sr += p[0];
                    si += p[1];
                    sd += p[2];
                }
                float zr = 1.f, zi = 0.f;
                if (sd > 0.) {
                    zr = (float)(sr / sd);
                    zi = (float)(si / sd);
                }
                v = make_float2(v.x * zr + v.y * zi, v.y * zr - v.x * zi);
            }
        }
        wl[kk][m][b] = v;
    }
    __syncthreads();

    const size_t frame_stride = (size_t)F * M;
    const float2* pbin = X + (size_t)(fvalid ? f : F - 1) * M;
    float nr[KP], ni[KP], dn[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) nr[kk] = ni[kk] = dn[kk] = 0.f;
    for (int t = t_begin + wave; t < t_end; t += kWaves) {
        const float2* px = pbin + (size_t)t * frame_stride;
        float yr[KP], yi[KP];
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) yr[kk] = yi[kk] = 0.f;
        float2 x0 = make_float2(0.f, 0.f);
#pragma unroll
        for (int m = 0; m < kWideMax; ++m) {
            if (m < M) {
                const float2 x = px[m];
                if (m == 0) x0 = x;
#pragma unroll
                for (int kk = 0; kk < KP; ++kk) {
                    const float2 w = wl[kk][m][lane];
                    yr[kk] = fmaf(w.x, x.x, fmaf(-w.y, x.y, yr[kk]));
                    yi[kk] = fmaf(w.x, x.y, fmaf(w.y, x.x, yi[kk]));
                }
            }
        }
        if constexpr (MODE == kWidePower) {
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                float pw = fvalid ? fmaf(yr[kk], yr[kk], yi[kk] * yi[kk]) : 0.f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) pw += __shfl_xor(pw, off, 64);
                if (lane == 0 && k0 + kk < K) out[((size_t)blockIdx.x * T + t) * K + k0 + kk] = pw;
            }
        } else if constexpr (MODE == kWideStats) {
#pragma unroll
            for (int kk = 0; kk < KP; ++kk) {
                nr[kk] = fmaf(x0.x, yr[kk], fmaf(x0.y, yi[kk], nr[kk]));       // conj(x0) y
                ni[kk] = fmaf(x0.x, yi[kk], fmaf(-x0.y, yr[kk], ni[kk]));
                dn[kk] = fmaf(yr[kk], yr[kk], fmaf(yi[kk], yi[kk], dn[kk]));
            }
        } else {
            if (fvalid) {
#pragma unroll
                for (int kk = 0; kk < KP; ++kk)
                    if (k0 + kk < K) Y[((size_t)t * F + f) * K + k0 + kk] = make_float2(yr[kk], yi[kk]);
            }
        }
    }
    if constexpr (MODE == kWideStats) {
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) {
            red[wave][3 * kk + 0][lane] = nr[kk];
            red[wave][3 * kk + 1][lane] = ni[kk];
            red[wave][3 * kk + 2][lane] = dn[kk];
        }
        __syncthreads();
        for (int e = tid; e < 3 * KP * 64; e += kBlock) {
            const int v = e / 64, b = e % 64;
            const int fo = blockIdx.x * 64 + b, kk = v / 3, c = v % 3;
            float s = red[0][v][b];
#pragma unroll
            for (int wv = 1; wv < kWaves; ++wv) s += red[wv][v][b];
            if (fo < F && k0 + kk < K) out[(((size_t)blockIdx.y * F + fo) * K + k0 + kk) * 3 + c] = s;
        }
    }
}

template <int MODE>
hipError_t launch_demix_wide(hipStream_t s, const float2* X, const float2* What, float* out, const float* Spart, int nsplit_s, float2* Y,
                             int T, int F, int M, int K, int kp, int nsplit, int tc) {
    const dim3 grid((F + 63) / 64, nsplit, (K + kp - 1) / kp);
    // (the statistics and the write of the epilogue take two sources per pass whatever K; only the power pass has 1 and 4)
    if (kp == 2) {
        hipLaunchKernelGGL((wide_demix_kernel<2, MODE>), grid, dim3(kBlock), 0, s, X, What, out, Spart, nsplit_s, Y, T, F, M, K, tc);
        return hipGetLastError();
    }
    if constexpr (MODE == kWidePower) {
        if (kp == 1) hipLaunchKernelGGL((wide_demix_kernel<1, MODE>), grid, dim3(kBlock), 0, s, X, What, out, Spart, nsplit_s, Y, T, F, M, K, tc);
        else if (kp == 4) hipLaunchKernelGGL((wide_demix_kernel<4, MODE>), grid, dim3(kBlock), 0, s, X, What, out, Spart, nsplit_s, Y, T, F, M, K, tc);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------------------------------
// per-bin update: one workgroup per bin, matrices in LDS
// ---------------------------------------------------------------------------------------------------------------------------
struct Zw {
    double re, im;
};
__device__ __forceinline__ Zw zmul(Zw a, Zw b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Zw zdiv(Zw a, Zw b) {
    const double n = 1. / (b.re * b.re + b.im * b.im);
    return {(a.re * b.re + a.im * b.im) * n, (a.im * b.re - a.re * b.im) * n};
}
__device__ __forceinline__ void zfma(Zw& acc, Zw a, Zw b) {
    acc.re = fma(a.re, b.re, fma(-a.im, b.im, acc.re));
    acc.im = fma(a.re, b.im, fma(a.im, b.re, acc.im));
}

// Gauss-Jordan elimination of columns 0..npiv-1 of the rows 0..nrow-1 of A (ncol columns), partial pivoting without moving
// rows: the pivot of column c is the unused row of largest modulus (the first on ties), perm[c] its index.  Every thread of
// the block calls it.
__device__ void wide_gauss_jordan(Zw (*A)[kWideMax + 2], int nrow, int ncol, int npiv, int* perm, int* used, Zw* fct) {
    const int tid = threadIdx.x;
    for (int c = 0; c < npiv; ++c) {
        if (tid < 64) {
            double mag = double(-1);
            int bl = tid;
            if (tid < nrow && !used[tid]) mag = A[tid][c].re * A[tid][c].re + A[tid][c].im * A[tid][c].im;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double om = __shfl_xor(mag, off, 64);
                const int ol = __shfl_xor(bl, off, 64);
                const bool take = (om > mag) || (om == mag && ol < bl);
                mag = take ? om : mag;
                bl = take ? ol : bl;
            }
            if (tid == 0) {
                perm[c] = bl;
                used[bl] = 1;
            }
        }
        __syncthreads();
        const int p = perm[c];
        if (tid < nrow) fct[tid] = tid == p ? Zw{double(0), double(0)} : zdiv(A[tid][c], A[p][c]);
        __syncthreads();
        const int w = ncol - c;
        for (int e = tid; e < nrow * w; e += kBlock) {
            const int r = e / w, j = c + e % w;
            if (r != p) {
                const Zw fr = fct[r], pj = A[p][j];
                Zw v = A[r][j];
                v.re -= fr.re * pj.re - fr.im * pj.im;
                v.im -= fr.re * pj.im + fr.im * pj.re;
                A[r][j] = j == c ? Zw{double(0), double(0)} : v;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void wide_update_kernel(UpdateArgs a) {
    __shared__ Zw B[kWideMax][kWideMax + 1];       // W_hat^H
    __shared__ Zw V[kWideMax][kWideMax + 1];       // V_s
    __shared__ Zw A[kWideMax][kWideMax + 2];       // W_hat^H V_s | e_s, then [W^H Cx]_{:K}
    __shared__ Zw Tm[kWideMax][kWideMax + 1];      // rows 0..K-1 of W^H Cx
    __shared__ Zw wv[kWideMax], fct[kWideMax];
    __shared__ int perm[kWideMax], used[kWideMax];
    __shared__ double dsum;
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    const int M = a.M, K = a.K, NA = M * M;
    const Zw zero = {double(0), double(0)};

    for (int e = tid; e < NA; e += kBlock) {
        const int i = e / M, m = e % M;               // B[i][m] = conj(W_hat[f][m][i])
        double vr, vi;
        load_what<double>(a, ((size_t)f * M + m) * M + i, vr, vi);
        if (a.wscale != nullptr && i < K) {           // overiva.py:163 / :167
            const double sc = double(1) / double(a.wscale[i]);
            vr *= sc;
            vi *= sc;
        }
        B[i][m] = {vr, -vi};
    }
    __syncthreads();
    const double* cx = a.Cx + (size_t)f * NA;
    auto cx_at = [&](int i, int j) {
        int off;
        float sgn;
        herm_offsets(M, i, j, off, sgn);
        return Zw{double(cx[off]), sgn != 0.f ? double(sgn * cx[off + 1]) : double(0)};
    };
    // row i of W^H Cx, i < K
    auto tm_row = [&](int i) {
        for (int j = tid; j < M; j += kBlock) {
            Zw s = zero;
            for (int m = 0; m < M; ++m) zfma(s, B[i][m], cx_at(m, j));
            Tm[i][j] = s;
        }
    };
    if (K < M) {
        for (int e = tid; e < K * M; e += kBlock) {
            const int i = e / M, j = e % M;
            Zw s = zero;
            for (int m = 0; m < M; ++m) zfma(s, B[i][m], cx_at(m, j));
            Tm[i][j] = s;
        }
        __syncthreads();
    }

    const int nsrc = a.init_only ? 0 : K;
    const double invT = double(1) / double(a.T);
    for (int s = 0; s <= nsrc; ++s) {
        const bool solve = s < nsrc;                  // the last trip exists only for init_only's J update
        if (!solve && !a.init_only) break;
        if (solve) {
            // V_s: fixed-order float64 sum of the frame-split partials, / T
            for (int e = tid; e < NA; e += kBlock) {
                const int i = e / M, j = e % M;
                int off;
                float sgn;
                herm_offsets(M, i, j, off, sgn);
                double sr, si;
                sum_vpart(a.Vpart, a.vpart_f64, ((size_t)f * K + s) * NA + off, (size_t)a.F * K * NA, a.nsplit, sgn != 0.f, sr, si);
                V[i][j] = {double(sr) * invT, double(si) * double(sgn) * invT};
            }
            if (tid < kWideMax) used[tid] = 0;
            __syncthreads();
            // A = W_hat^H V_s | e_s
            for (int e = tid; e < M * (M + 1); e += kBlock) {
                const int i = e / (M + 1), j = e % (M + 1);
                Zw acc = {double(j == M && i == s ? 1 : 0), double(0)};
                if (j < M)
                    for (int m = 0; m < M; ++m) zfma(acc, B[i][m], V[m][j]);
                A[i][j] = acc;
            }
            __syncthreads();
            wide_gauss_jordan(A, M, M + 1, M, perm, used, fct);
            // w[c] = rhs / pivot on the row that pivoted column c  (overiva.py:181-182)
            if (tid < M) wv[tid] = zdiv(A[perm[tid]][M], A[perm[tid]][tid]);
            __syncthreads();
            // d = w^H V w  (overiva.py:185-186): row sums by lane, then a fixed-order sum
            if (tid < 64) {
                double part = double(0);
                if (tid < M) {
                    Zw u = zero;
                    for (int j = 0; j < M; ++j) zfma(u, V[tid][j], wv[j]);
                    part = wv[tid].re * u.re + wv[tid].im * u.im;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
                if (tid == 0) dsum = part;
            }
            __syncthreads();
            const double sc = double(1) / sqrt(dsum);
            if (tid < M) B[s][tid] = {wv[tid].re * sc, -wv[tid].im * sc};
            __syncthreads();
        }
        if (K < M) {
            if (solve) {
                tm_row(s);
                __syncthreads();
            }
            // J = (W^H Cx)[:, :K]^{-1} (W^H Cx)[:, K:]  (overiva.py:96-98)
            for (int e = tid; e < K * M; e += kBlock) A[e / M][e % M] = Tm[e / M][e % M];
            if (tid < kWideMax) used[tid] = 0;
            __syncthreads();
            wide_gauss_jordan(A, K, M, K, perm, used, fct);
            // W_hat[m][j] = J[m][j - K] (m < K <= j): row j of W_hat^H, entry m = conj
            for (int e = tid; e < K * (M - K); e += kBlock) {
                const int m = e / (M - K), j = K + e % (M - K);
                const int pr = perm[m];
                const Zw v = zdiv(A[pr][j], A[pr][m]);
                B[j][m] = {v.re, -v.im};
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < NA; e += kBlock) {
        const int i = e / M, m = e % M;
        store_what<double>(a, ((size_t)f * M + m) * M + i, B[i][m].re, -B[i][m].im);
    }
}

}  // namespace

static bool wide_channels(int M) { return M > kNarrowMax && M <= kWideMax; }
static_assert(traits(CovKind::Wide).sources(kWideMax) == kWideKc64, "kernel_choice.h");

hipError_t launch_cov_wide(hipStream_t s, const float2* X, const float* R, void* Wt, float* wscale, int model, int raw, double* Vpart,
                           int T, int F, int M, int K, const CovGeom& g) {
    if (!wide_channels(M) || K < 1 || K > M) return hipErrorInvalidValue;
    const bool unit = R == nullptr;
    const int kc = unit ? 1 : g.kc;
    const dim3 grid(F, g.nsplit, (K + kc - 1) / kc);
    double* wt = unit ? nullptr : static_cast<double*>(Wt);
    if (!unit) {
        if (Wt == nullptr) return hipErrorInvalidValue;
        wide_weights64_kernel<<<dim3((unsigned)(((long long)T * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, s>>>(R, wt, wscale, model, raw, T, K);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (kc == 1) return launch_dominant(wide_cov64_kernel<1>, grid, dim3(kBlock), 0, s, X, (const double*)wt, Vpart, T, F, M, K, K, g.tc);
    if (kc == 2) return launch_dominant(wide_cov64_kernel<2>, grid, dim3(kBlock), 0, s, X, (const double*)wt, Vpart, T, F, M, K, K, g.tc);
    return hipErrorInvalidValue;
}

hipError_t launch_power_wide(hipStream_t s, const float2* X, const float2* What, float* Ppart, int T, int F, int M, int K, const PowGeom& g) {
    if (!wide_channels(M)) return hipErrorInvalidValue;
    return launch_demix_wide<kWidePower>(s, X, What, Ppart, nullptr, 0, nullptr, T, F, M, K, g.kp, g.nsplit, g.tcp);
}

hipError_t launch_demix_stats_wide(hipStream_t s, const float2* X, const float2* What, float* Spart, int T, int F, int M, int K,
                                   const CovGeom& g) {
    if (!wide_channels(M)) return hipErrorInvalidValue;
    return launch_demix_wide<kWideStats>(s, X, What, Spart, nullptr, 0, nullptr, T, F, M, K, 2, g.nsplit, g.tc);
}

hipError_t launch_demix_write_wide(hipStream_t s, const float2* X, const float2* What, const float* Spart, int nsplit, float2* Y, int T,
                                   int F, int M, int K) {
    if (!wide_channels(M)) return hipErrorInvalidValue;
    const int tc = 256;
    return launch_demix_wide<kWideWrite>(s, X, What, nullptr, Spart, nsplit, Y, T, F, M, K, 2, (T + tc - 1) / tc, tc);
}

static_assert(traits(UpdKind::Wide).block == kBlock && traits(UpdKind::Wide).bins == 1, "kernel_choice.h");

hipError_t launch_update_wide(hipStream_t s, const UpdateArgs& a, const UpdChoice& c) {
    // float64 in every arithmetic mode; with `fast` (a.What64 == nullptr) W_hat is carried in complex64 between iterations
    hipLaunchKernelGGL(wide_update_kernel, dim3(ceil_div(a.F, c.bins_per_block)), dim3(c.block), 0, s, a);
    return hipGetLastError();
}

}  // namespace oiva
