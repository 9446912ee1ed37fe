// Kernels of batched ILRMA (ilrma_batch, batch.hip: oiva_batch_ilrma_*): B rooms of one shape per launch, determined (K = M <= 8),
// L <= 16 NMF components per source, `precise` arithmetic: float64 state, float64 sums.
//
//   X      (B, T, F, M) complex64, What64 / What (B*F, M, M): the batch's own
//   Tn     (B, K, F, L), Vn (B, K, L, T)            float64, positive
//   P, R   (B, K, F, T) float64, t fastest: P[s,f,t] = |y[t,f,s]|^2, R[s] = Tn[s] Vn[s]
//   Upart  [2][nchunk][B*K][L][T]: numerator and denominator partials of the V update per chunk of kIlVBins bins
//   rowsum (B, K, F), lam (B, K): the two stages of the normalisation's mean of P
//   Vpart  [nsplit][B*F][K][M*M]: the batch's packed frame-split partials, read by the float64 per-bin update (launch_update)
//
// The room index comes from the grid (blockIdx.z, with the source where a launch runs per source) and a workgroup never holds two
// rooms.  Every sum runs in an order that is a function of (bin, frame, component) within the room: lane-strided sequential
// sums closed by one fixed butterfly, bins in ascending order inside chunks whose bounds follow from F, chunks and frame splits
// added in order.  A room therefore gets the same bits alone, in a larger batch or in a permuted one.
#include "oiva_device.h"
#include "batch_cov_arith.h"

namespace oiva {
namespace {

constexpr double kIlEps = 2.220446049250313e-16;   // np.finfo(np.float64).eps: the floor of Tn and Vn
constexpr int kIlPowBins = 16;      // tile of the power pass: 16 bins (contiguous in X) x 32 frames (contiguous in P)
constexpr int kIlPowFrames = 32;
constexpr int kIlVBins = 64;        // bins per chunk of the V update: ceil(F / 64) chunks, a function of F alone
constexpr int kIlRBins = 16;        // bins per workgroup of the R rewrite

// the fixed butterfly that closes every lane-strided sum: all 64 lanes end with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
// power: P[b,s,f,t] = |sum_m x[t,f,m] conj(W[f,m,s])|^2 in float64 from What64.  X is (T, F, M) and P has t fastest, so the
// pass transposes through an LDS tile: the loads of X run along (bin, channel), the stores of P along the frames.  The rows of
// the tile are padded by one element, which spreads the 32 frames of a bin over the banks.
// ---------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kBlock) void ilrma_power_kernel(const float2* __restrict__ X, const double2* __restrict__ What64,
                                                             double* __restrict__ P, int T, int F) {
    constexpr int ROW = kIlPowBins * M;
    __shared__ float2 xs[kIlPowFrames][ROW + 1];
    __shared__ double2 wsm[kIlPowBins][M * M];
    const int tid = threadIdx.x;
    const int prob = blockIdx.z;
    const int f0 = blockIdx.x * kIlPowBins;
    const int t0 = blockIdx.y * kIlPowFrames;
    const int len = min(kIlPowFrames, T - t0);
    const float2* Xb = X + (size_t)prob * T * F * M;
    for (int i = tid; i < len * ROW; i += kBlock) {
        const int tl = i / ROW;
        const int r = i - tl * ROW;
        const int f = f0 + r / M;
        xs[tl][r] = f < F ? Xb[((size_t)(t0 + tl) * F + f0) * M + r] : make_float2(0.f, 0.f);
    }
    for (int i = tid; i < kIlPowBins * M * M; i += kBlock) {
        const int bb = i / (M * M);
        const int e = i - bb * (M * M);
        const int f = f0 + bb;
        wsm[bb][e] = f < F ? What64[((size_t)prob * F + f) * M * M + e] : make_double2(0., 0.);
    }
    __syncthreads();
    const int tl = tid & (kIlPowFrames - 1);
    const int bg = tid / kIlPowFrames;                     // 0..7: bins bg and bg + 8
#pragma unroll
    for (int j = 0; j < kIlPowBins * kIlPowFrames / kBlock; ++j) {
        const int bb = bg + j * (kBlock / kIlPowFrames);
        const int f = f0 + bb;
        if (tl >= len || f >= F) continue;
        double xr[M], xi[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float2 v = xs[tl][bb * M + m];
            xr[m] = (double)v.x;
            xi[m] = (double)v.y;
        }
#pragma unroll
        for (int s = 0; s < M; ++s) {
            double yr = 0., yi = 0.;
#pragma unroll
            for (int m = 0; m < M; ++m) {                  // x conj(w), channels in ascending order
                const double2 w = wsm[bb][m * M + s];
                yr = fma(xr[m], w.x, yr);
                yr = fma(xi[m], w.y, yr);
                yi = fma(xi[m], w.x, yi);
                yi = fma(-xr[m], w.y, yi);
            }
            P[(((size_t)prob * M + s) * F + f) * T + t0 + tl] = fma(yr, yr, yi * yi);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// T update: one wavefront per row (b, s, f).  Lanes stride over the frames; for every component l the two sums
// sum_t P iR^2 Vn[l,t] and sum_t iR Vn[l,t] are lane-strided sequential sums closed by the butterfly.  Lane l then updates and
// floors Tn[b,s,f,l], and the wavefront rewrites R[b,s,f,:] from the new row.  LP: L rounded up (register arrays).
// ---------------------------------------------------------------------------------------------
template <int LP>
__global__ __launch_bounds__(kBlock) void ilrma_t_kernel(const double* __restrict__ P, double* __restrict__ R, double* __restrict__ Tn,
                                                         const double* __restrict__ Vn, int T, int F, int K, int L) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int s = blockIdx.y, prob = blockIdx.z;
    if (f >= F) return;                                    // (the whole wavefront; the kernel has no barrier)
    const size_t bs = (size_t)prob * K + s;
    const size_t row = (bs * F + f) * T;
    const double* Vs = Vn + bs * L * T;
    double num[LP], den[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) num[l] = den[l] = 0.;
    for (int t = lane; t < T; t += 64) {
        const double ir = 1. / R[row + t];
        const double a = P[row + t] * (ir * ir);
#pragma unroll
        for (int l = 0; l < LP; ++l) {
            if (l < L) {
                const double v = Vs[(size_t)l * T + t];
                num[l] = fma(a, v, num[l]);
                den[l] = fma(ir, v, den[l]);
            }
        }
    }
    double my_num = 0., my_den = 1.;
#pragma unroll
    for (int l = 0; l < LP; ++l) {
        if (l < L) {                                       // (uniform)
            const double n = wave_sum(num[l]);
            const double d = wave_sum(den[l]);
            if (lane == l) {
                my_num = n;
                my_den = d;
            }
        }
    }
    double tn = 0.;
    if (lane < L) {
        double* q = Tn + (bs * F + f) * L + lane;
        tn = *q * sqrt(my_num / my_den);
        if (tn < kIlEps) tn = kIlEps;                      // a NaN stays NaN, like Tn[Tn < eps] = eps
        *q = tn;
    }
    double tl[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) tl[l] = __shfl(tn, l, 64);
    for (int t = lane; t < T; t += 64) {
        double r = 0.;
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) r = fma(tl[l], Vs[(size_t)l * T + t], r);
        R[row + t] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// V update, first launch: lane = frame, workgroup = 256 frames x one chunk of kIlVBins bins of (b, s).  The bins of the chunk in
// ascending order; the chunk's partial sums of every component go to Upart.
// ---------------------------------------------------------------------------------------------
template <int LP>
__global__ __launch_bounds__(kBlock) void ilrma_v_part_kernel(const double* __restrict__ P, const double* __restrict__ R,
                                                              const double* __restrict__ Tn, double* __restrict__ Upart, int T, int F,
                                                              int L, size_t half) {
    __shared__ double tn[kIlVBins][LP];
    const int tid = threadIdx.x;
    const size_t bs = blockIdx.z;
    const int f_begin = blockIdx.y * kIlVBins;
    const int f_end = min(F, f_begin + kIlVBins);
    for (int i = tid; i < kIlVBins * LP; i += kBlock) {
        const int bb = i / LP, l = i - bb * LP;
        const int f = f_begin + bb;
        tn[bb][l] = (f < F && l < L) ? Tn[(bs * F + f) * L + l] : 0.;
    }
    __syncthreads();
    const int t = blockIdx.x * kBlock + tid;
    if (t >= T) return;
    double num[LP], den[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) num[l] = den[l] = 0.;
    for (int f = f_begin; f < f_end; ++f) {
        const size_t idx = (bs * F + f) * T + t;
        const double ir = 1. / R[idx];
        const double a = P[idx] * (ir * ir);
#pragma unroll
        for (int l = 0; l < LP; ++l) {
            const double w = tn[f - f_begin][l];
            num[l] = fma(w, a, num[l]);
            den[l] = fma(w, ir, den[l]);
        }
    }
    const size_t out = (((size_t)blockIdx.y * gridDim.z + bs) * L) * T + t;
#pragma unroll
    for (int l = 0; l < LP; ++l) {
        if (l < L) {
            Upart[out + (size_t)l * T] = num[l];
            Upart[half + out + (size_t)l * T] = den[l];
        }
    }
}

// V update, second launch: the chunk partials added in chunk order, the update and the floor.  grid (frames / 256, L, B*K)
__global__ __launch_bounds__(kBlock) void ilrma_v_finish_kernel(const double* __restrict__ Upart, double* __restrict__ Vn, int T, int L,
                                                                int nchunk, size_t half) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const size_t bs = blockIdx.z;
    const int l = blockIdx.y;
    const size_t stride = (size_t)gridDim.z * L * T;
    const size_t at = (bs * L + l) * T + t;
    double n = 0., d = 0.;
    for (int c = 0; c < nchunk; ++c) {
        n += Upart[(size_t)c * stride + at];
        d += Upart[half + (size_t)c * stride + at];
    }
    double v = Vn[at] * sqrt(n / d);
    if (v < kIlEps) v = kIlEps;
    Vn[at] = v;
}

// R = Tn Vn, element-wise over (b, s, f, t): lane = frame with its column of Vn in registers, kIlRBins bins per workgroup; the
// components in ascending order, as the T update's rewrite of its own row
template <int LP>
__global__ __launch_bounds__(kBlock) void ilrma_r_kernel(const double* __restrict__ Tn, const double* __restrict__ Vn, double* __restrict__ R,
                                                         int T, int F, int L) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const size_t bs = blockIdx.z;
    double v[LP];
#pragma unroll
    for (int l = 0; l < LP; ++l) v[l] = l < L ? Vn[(bs * L + l) * T + t] : 0.;
    const int f_begin = blockIdx.y * kIlRBins;
    const int f_end = min(F, f_begin + kIlRBins);
    for (int f = f_begin; f < f_end; ++f) {
        const double* q = Tn + (bs * F + f) * L;
        double r = 0.;
#pragma unroll
        for (int l = 0; l < LP; ++l)
            if (l < L) r = fma(q[l], v[l], r);
        R[(bs * F + f) * T + t] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// weighted covariance: the body of batch_cov_block (batch_cov_arith.h) -- the same (bin, Hermitian entry) items, the same split
// bounds, the same sums in frame order -- with the weight 1 / R[b,s,f,t] per (frame, bin, source) staged next to X instead of
// 1 / r[t,s] per (frame, source).  K = M sources.  The chunk is 16 frames from 5 channels on, which keeps X and the weights
// within 32 KB of LDS; the length of a chunk does not enter any sum.
// ---------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void ilrma_cov_block(const float2* __restrict__ X, size_t x_frame0, const double* __restrict__ Rb,
                                                double* __restrict__ Vpart, int T, int F, int tc, int nbins_all, int prob) {
    constexpr int E = M * (M + 1) / 2;                           // entries of the Hermitian half
    constexpr int NI = (kBatchBins * E + kBlock - 1) / kBlock;   // (bin, entry) items per thread
    constexpr int CH = M > 4 ? kBatchChunk / 2 : kBatchChunk;
    __shared__ float2 xs[CH][kBatchBins][M];
    __shared__ double ws[CH][kBatchBins][M];

    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * kBatchBins;
    const int t_begin = blockIdx.y * tc;
    const int t_end = min(T, t_begin + tc);
    const float2* Xb = X + x_frame0 * F * M;

    // this thread's items: bin ib[j], channels ic[j] <= id[j]
    int ib[NI], ic[NI], id[NI];
    bool iv[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int it = tid + j * kBlock;
        iv[j] = it < kBatchBins * E;
        const int itc = iv[j] ? it : 0;
        ib[j] = itc / E;
        int e = itc - ib[j] * E, c = 0;
        while (e >= M - c) {         // row c of the half holds M - c entries (c, c..M-1)
            e -= M - c;
            ++c;
        }
        ic[j] = c;
        id[j] = c + e;
    }
    double ar[NI][M], ai[NI][M];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int k = 0; k < M; ++k) ar[j][k] = ai[j][k] = 0.;

    for (int tc0 = t_begin; tc0 < t_end; tc0 += CH) {
        const int len = min(CH, t_end - tc0);
        __syncthreads();
        // stage the chunk: frame t holds the 16 bins' M channels contiguously; bins past F are zeros
        for (int i = tid; i < len * kBatchBins * M; i += kBlock) {
            const int tl = i / (kBatchBins * M);
            const int r = i - tl * (kBatchBins * M);
            const int f = f0 + r / M;
            xs[tl][r / M][r % M] = f < F ? Xb[((size_t)(tc0 + tl) * F + f0) * M + r] : make_float2(0.f, 0.f);
        }
        // ... and its weights: R has the frames fastest, so the loads run along them
        for (int i = tid; i < len * kBatchBins * M; i += kBlock) {
            const int tl = i % len;
            const int q = i / len;
            const int bb = q % kBatchBins, k = q / kBatchBins;
            const int f = f0 + bb;
            ws[tl][bb][k] = f < F ? 1. / Rb[((size_t)k * F + f) * T + tc0 + tl] : 0.;
        }
        __syncthreads();
        for (int tl = 0; tl < len; ++tl) {
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const float2 xc = xs[tl][ib[j]][ic[j]];
                const float2 xd = xs[tl][ib[j]][id[j]];
                // x_c conj(x_d): exact float64 products of float32 data, summed as batch_cov_block does
                const double pre = fma((double)xc.x, (double)xd.x, (double)xc.y * (double)xd.y);
                const double pim = fma((double)xc.y, (double)xd.x, -((double)xc.x * (double)xd.y));
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const double w = ws[tl][ib[j]][k];
                    ar[j][k] = fma(w, pre, ar[j][k]);
                    ai[j][k] = fma(w, pim, ai[j][k]);
                }
            }
        }
    }

    // packed partial of this split: [split][prob * F + f][k][M*M]
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int f = f0 + ib[j];
        if (!iv[j] || f >= F) continue;
        double* out = Vpart + ((size_t)blockIdx.y * nbins_all + (size_t)prob * F + f) * M * M * M;
        const int c = ic[j], d = id[j];
#pragma unroll
        for (int k = 0; k < M; ++k) {
            if (c == d) {
                out[(size_t)k * M * M + c] = ar[j][k];
            } else {
                const int a = herm_pair_index(M, c, d);
                out[(size_t)k * M * M + a] = ar[j][k];
                out[(size_t)k * M * M + a + 1] = ai[j][k];
            }
        }
    }
}

template <int M>
__global__ __launch_bounds__(kBlock) void ilrma_cov_kernel(const float2* __restrict__ X, const double* __restrict__ R,
                                                           double* __restrict__ Vpart, int T, int F, int tc, int nbins_all) {
    const int prob = blockIdx.z;
    ilrma_cov_block<M>(X, (size_t)prob * T, R + (size_t)prob * M * F * T, Vpart, T, F, tc, nbins_all, prob);
}

// ---------------------------------------------------------------------------------------------
// normalisation: rowsum[b,s,f] = sum_t P (one wavefront per row: lane-strided, then the butterfly); lam[b,s] = sqrt of the mean
// over (f, t), from the row sums of the F bins in the same fixed form (one wavefront per (b, s)); then one scaling launch, one
// wavefront per row: P and R by 1 / lam^2, the row of Tn by 1 / lam^2, column s of W of the bin by 1 / lam (both copies).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ilrma_rowsum_kernel(const double* __restrict__ P, double* __restrict__ rowsum, int T, int F) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (f >= F) return;
    const size_t bs = blockIdx.z;
    const double* p = P + (bs * F + f) * T;
    double a = 0.;
    for (int t = lane; t < T; t += 64) a += p[t];
    a = wave_sum(a);
    if (lane == 0) rowsum[bs * F + f] = a;
}

__global__ __launch_bounds__(64) void ilrma_lambda_kernel(const double* __restrict__ rowsum, double* __restrict__ lam, int T, int F) {
    const int lane = threadIdx.x;
    const size_t bs = blockIdx.x;
    double a = 0.;
    for (int f = lane; f < F; f += 64) a += rowsum[bs * F + f];
    a = wave_sum(a);
    if (lane == 0) lam[bs] = sqrt(a / ((double)F * (double)T));
}

__global__ __launch_bounds__(kBlock) void ilrma_scale_kernel(const double* __restrict__ lam, double* __restrict__ P, double* __restrict__ R,
                                                             double* __restrict__ Tn, float2* __restrict__ What, double2* __restrict__ What64,
                                                             int T, int F, int M, int L) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (f >= F) return;
    const int s = blockIdx.y, prob = blockIdx.z;
    const size_t bs = (size_t)prob * M + s;
    const double la = lam[bs];
    const double l2 = la * la;
    const size_t row = (bs * F + f) * T;
    for (int t = lane; t < T; t += 64) {
        P[row + t] /= l2;
        R[row + t] /= l2;
    }
    if (lane < L) Tn[(bs * F + f) * L + lane] /= l2;
    if (lane < M) {
        const size_t idx = (((size_t)prob * F + f) * M + lane) * M + s;
        double2 w = What64[idx];
        w.x /= la;
        w.y /= la;
        What64[idx] = w;
        What[idx] = make_float2((float)w.x, (float)w.y);
    }
}

#define OIVA_ILRMA_DISPATCH_L(CALL) \
    if (L <= 1) { CALL(1); }        \
    else if (L <= 2) { CALL(2); }   \
    else if (L <= 4) { CALL(4); }   \
    else if (L <= 8) { CALL(8); }   \
    else { CALL(16); }

unsigned blocks_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

int ilrma_v_chunks(int F) { return (F + kIlVBins - 1) / kIlVBins; }

hipError_t launch_ilrma_power(hipStream_t s, const float2* X, const double2* What64, const IlrmaState& st, int B, int T, int F, int M) {
    const dim3 grid(blocks_of(F, kIlPowBins), blocks_of(T, kIlPowFrames), (unsigned)B);
    switch (M) {
#define CALL(MM) \
    case MM: hipLaunchKernelGGL(ilrma_power_kernel<MM>, grid, dim3(kBlock), 0, s, X, What64, st.P, T, F); break;
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
#undef CALL
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ilrma_t(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K) {
    const int L = st.L;
    if (L < 1 || L > 16) return hipErrorInvalidValue;
    const dim3 grid(blocks_of(F, kWaves), (unsigned)K, (unsigned)B);
#define CALL(LP) hipLaunchKernelGGL(ilrma_t_kernel<LP>, grid, dim3(kBlock), 0, s, st.P, st.R, st.Tn, st.Vn, T, F, K, L)
    OIVA_ILRMA_DISPATCH_L(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_ilrma_v(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K) {
    const int L = st.L;
    if (L < 1 || L > 16) return hipErrorInvalidValue;
    const int nchunk = ilrma_v_chunks(F);
    const size_t half = (size_t)nchunk * B * K * L * T;
    const dim3 grid(blocks_of(T, kBlock), (unsigned)nchunk, (unsigned)(B * K));
#define CALL(LP) hipLaunchKernelGGL(ilrma_v_part_kernel<LP>, grid, dim3(kBlock), 0, s, st.P, st.R, st.Tn, st.Upart, T, F, L, half)
    OIVA_ILRMA_DISPATCH_L(CALL)
#undef CALL
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid2(blocks_of(T, kBlock), (unsigned)L, (unsigned)(B * K));
    hipLaunchKernelGGL(ilrma_v_finish_kernel, grid2, dim3(kBlock), 0, s, st.Upart, st.Vn, T, L, nchunk, half);
    return hipGetLastError();
}

hipError_t launch_ilrma_r(hipStream_t s, const IlrmaState& st, int B, int T, int F, int K) {
    const int L = st.L;
    if (L < 1 || L > 16) return hipErrorInvalidValue;
    const dim3 grid(blocks_of(T, kBlock), blocks_of(F, kIlRBins), (unsigned)(B * K));
#define CALL(LP) hipLaunchKernelGGL(ilrma_r_kernel<LP>, grid, dim3(kBlock), 0, s, st.Tn, st.Vn, st.R, T, F, L)
    OIVA_ILRMA_DISPATCH_L(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_ilrma_cov(hipStream_t s, const float2* X, const IlrmaState& st, double* Vpart, int B, int T, int F, int M, int nsplit,
                            int tc) {
    const dim3 grid(blocks_of(F, kBatchBins), (unsigned)nsplit, (unsigned)B);
    const int nbins_all = B * F;
    switch (M) {
#define CALL(MM) \
    case MM: hipLaunchKernelGGL(ilrma_cov_kernel<MM>, grid, dim3(kBlock), 0, s, X, st.R, Vpart, T, F, tc, nbins_all); break;
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
#undef CALL
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ilrma_normalise(hipStream_t s, const IlrmaState& st, float2* What, double2* What64, int B, int T, int F, int M) {
    const dim3 rows(blocks_of(F, kWaves), 1, (unsigned)(B * M));
    hipLaunchKernelGGL(ilrma_rowsum_kernel, rows, dim3(kBlock), 0, s, st.P, st.rowsum, T, F);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ilrma_lambda_kernel, dim3((unsigned)(B * M)), dim3(64), 0, s, st.rowsum, st.lam, T, F);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid(blocks_of(F, kWaves), (unsigned)M, (unsigned)B);
    hipLaunchKernelGGL(ilrma_scale_kernel, grid, dim3(kBlock), 0, s, st.lam, st.P, st.R, st.Tn, What, What64, T, F, M, st.L);
    return hipGetLastError();
}

}  // namespace oiva
