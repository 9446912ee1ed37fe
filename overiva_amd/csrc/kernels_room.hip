// Kernels of simulate_batch / rir_batch (room.hip: oiva_room_*): the image-source method in a shoebox for B rooms of S sources and
// M microphones, the passes around hipFFT of the convolution, and the mix-down.  All arithmetic is float64.
//
//   images    (n_img) char4 (nx, ny, nz, 0): |nx| + |ny| + |nz| <= max_order in the order nx, ny, nz ascending -- the order of
//             summation of every impulse response sample
//   rir       packed: room b holds its (S, M, Lr_b) impulse responses at rooms[b].rir_off
//   premix    one room (S, M, n_out), n_out = n + Lr - 1;  mix (n_out, M), ref (K + 1, n_out, M)
//
// The room and the pair come from the grid and a workgroup never holds two of either.  Every sample of an impulse response has
// one owner -- one lane of one wave -- which adds the taps of the images in the order of the table: no atomics on floating-point
// numbers anywhere, and no order of operations that depends on B, on the room's place in the batch or on the other rooms.
#include "oiva_device.h"

// products and sums stay apart in this file: an image's k must come out the same in the k_max pass and in the impulse response
// pass, whatever the compiler makes of the code around it (the two explicit fma below are unaffected)
#pragma clang fp contract(off)

namespace oiva {
namespace {

constexpr int kRirThreads = 256;                         // one image per lane and chunk
constexpr int kRirRegs = 4;                              // samples a lane owns
constexpr int kRirSeg = 64 * kRirRegs;                   // samples a wave owns, contiguous
constexpr int kRirSlab = kRirSeg * (kRirThreads / 64);   // samples a workgroup owns
constexpr int kNoHit = 0x3fffffff;                       // the k of a table entry past the last image
constexpr double kPi = 3.141592653589793238462643383279502884;

// beta^e, e >= 0, by squaring
__device__ __forceinline__ double ipow(double beta, int e) {
    double r = 1., b = beta;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// the coordinate of image n along an axis of length L, and its reflections at the wall at 0 and at the far wall
__device__ __forceinline__ double axis_image(int n, double L, double s, int* at_zero, int* at_far) {
    const int a = n < 0 ? -n : n;
    const int more = (a + 1) >> 1, less = a >> 1;
    *at_zero = n < 0 ? more : less;
    *at_far = n < 0 ? less : more;
    return (n & 1) ? (double)(n + 1) * L - s : (double)n * L + s;
}

// one image of one (source, microphone) pair: k, phi and g = prod beta_w^count_w / (4 pi d)
__device__ __forceinline__ void image_term(const RoomRec& r, char4 n, const double* __restrict__ sp, const double* __restrict__ mp,
                                           double fs_over_c, int* k, double* phi, double* g) {
    int z0, z1;
    const double dx = axis_image(n.x, r.dim[0], sp[0], &z0, &z1) - mp[0];
    double gain = ipow(r.beta[0], z0) * ipow(r.beta[1], z1);
    const double dy = axis_image(n.y, r.dim[1], sp[1], &z0, &z1) - mp[1];
    gain *= ipow(r.beta[2], z0) * ipow(r.beta[3], z1);
    const double dz = axis_image(n.z, r.dim[2], sp[2], &z0, &z1) - mp[2];
    gain *= ipow(r.beta[4], z0) * ipow(r.beta[5], z1);
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    const double tau = d * fs_over_c;
    const double kf = floor(tau + 0.5);
    *k = (int)kf;
    *phi = tau - kf;
    *g = gain / (4. * kPi * d);
}

// ---------------------------------------------------------------------------------------------
// k_max: one workgroup = (pair, room); the lanes stride over the images; an integer max all the way
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRirThreads) void room_kmax_kernel(const RoomRec* __restrict__ rooms, const double* __restrict__ src,
                                                                 const double* __restrict__ mic, const char4* __restrict__ images,
                                                                 int n_img, int S, int M, double fs_over_c, int* __restrict__ kmax) {
    __shared__ int part[kRirThreads / 64];
    const int room = blockIdx.y, pair = blockIdx.x;
    const int s = pair / M, m = pair - s * M;
    const RoomRec r = rooms[room];
    const double* sp = src + ((size_t)room * S + s) * 3;
    const double* mp = mic + ((size_t)room * M + m) * 3;
    int best = 0;
    for (int i = threadIdx.x; i < n_img; i += kRirThreads) {
        int k;
        double phi, g;
        image_term(r, images[i], sp, mp, fs_over_c, &k, &phi, &g);
        best = max(best, k);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kRirThreads / 64; ++w) best = max(best, part[w]);
        atomicMax(&kmax[room], best);
    }
}

// ---------------------------------------------------------------------------------------------
// impulse responses: one workgroup = (slab of kRirSlab samples, pair, room); wave w owns samples [w0, w0 + kRirSeg) of the slab,
// lane l of it the samples w0 + 64 r + l, r < kRirRegs, in registers.  The images go by in chunks of 256: lane i of the
// workgroup computes image i's (k, phi, g) into an LDS table; every wave then walks the table in order -- a ballot over 64
// entries finds the images whose window [k, k + 81) meets the wave's samples, and the set bits are taken in ascending order --
// and adds g win[j] sinc(j - H - phi) with sin(pi (j - H - phi)) = -(-1)^(j - H) sin(pi phi): one sine per image.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRirThreads) void room_rir_kernel(const RoomRec* __restrict__ rooms, const double* __restrict__ src,
                                                                const double* __restrict__ mic, const char4* __restrict__ images,
                                                                int n_img, int S, int M, double fs_over_c, double* __restrict__ rir) {
    __shared__ double s_win[kRoomFdl];
    __shared__ int s_k[kRirThreads];
    __shared__ double s_phi[kRirThreads], s_c1[kRirThreads], s_g[kRirThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int room = blockIdx.z, pair = blockIdx.y;
    const RoomRec r = rooms[room];
    const int Lr = r.Lr;
    const int slab0 = blockIdx.x * kRirSlab;
    if (slab0 >= Lr) return;                          // (the whole workgroup: the grid is sized by the longest room)
    const int s = pair / M, m = pair - s * M;
    const double* sp = src + ((size_t)room * S + s) * 3;
    const double* mp = mic + ((size_t)room * M + m) * 3;
    const int w0 = slab0 + wave * kRirSeg;
    const int w1 = min(w0 + kRirSeg, Lr);             // the window is clipped at Lr (w1 <= w0: nothing of this wave's is kept)
    if (tid < kRoomFdl) s_win[tid] = 0.5 - 0.5 * cospi((double)tid / (double)kRoomHalf);
    double acc[kRirRegs];
#pragma unroll
    for (int q = 0; q < kRirRegs; ++q) acc[q] = 0.;
    for (int c0 = 0; c0 < n_img; c0 += kRirThreads) {
        __syncthreads();                              // the table of the chunk before has been walked by every wave
        const int i = c0 + tid;
        int k = kNoHit;
        double phi = 0., g = 0.;
        if (i < n_img) image_term(r, images[i], sp, mp, fs_over_c, &k, &phi, &g);
        s_k[tid] = k;
        s_phi[tid] = phi;
        s_g[tid] = g;
        s_c1[tid] = g * sinpi(phi) / kPi;
        __syncthreads();
        for (int q = 0; q < kRirThreads / 64; ++q) {
            const int kk = s_k[q * 64 + lane];
            unsigned long long hits = __ballot(kk < w1 && kk + kRoomFdl > w0);
            while (hits) {
                const int e = q * 64 + __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                const int ke = s_k[e];
                const double phie = s_phi[e], c1 = s_c1[e], ge = s_g[e];
#pragma unroll
                for (int t = 0; t < kRirRegs; ++t) {
                    const int base = w0 + t * 64;
                    if (ke < base + 64 && ke + kRoomFdl > base) {
                        const int j = base + lane - ke;
                        if ((unsigned)j < (unsigned)kRoomFdl) {
                            const int jh = j - kRoomHalf;
                            const double x = (double)jh - phie;
                            const double w = s_win[j];
                            const double term = x == 0. ? ge * w : w * ((jh & 1) ? c1 : -c1) / x;
                            acc[t] += term;
                        }
                    }
                }
            }
        }
    }
    double* out = rir + r.rir_off + (size_t)pair * Lr;
#pragma unroll
    for (int t = 0; t < kRirRegs; ++t) {
        const int idx = w0 + t * 64 + lane;
        if (idx < Lr) out[idx] = acc[t];
    }
}

// ---------------------------------------------------------------------------------------------
// the passes around the transforms of one room
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void room_pad_kernel(const double* __restrict__ src, long long src_stride, int len,
                                                        double* __restrict__ dst, int nfft) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;
    if (t < nfft) dst[row * nfft + t] = t < len ? src[row * src_stride + t] : 0.;
}

__global__ __launch_bounds__(256) void room_product_kernel(double2* __restrict__ H, const double2* __restrict__ X, int nf, int M) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;                    // s * M + m
    if (f >= nf) return;
    const double2 x = X[(row / M) * nf + f];
    const double2 h = H[row * nf + f];
    H[row * nf + f] = make_double2(h.x * x.x - h.y * x.y, h.x * x.y + h.y * x.x);
}

__global__ __launch_bounds__(256) void room_unpack_kernel(const double* __restrict__ y, int nfft, double* __restrict__ premix,
                                                           int n_out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;
    if (t < n_out) premix[row * n_out + t] = y[row * nfft + t] / (double)nfft;
}

// block-wide sum in a fixed order: the wave's shuffle tree, then the waves in order; every thread gets the sum
__device__ __forceinline__ double room_block_sum(double v, double* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double sum = 0.;
#pragma unroll
    for (int w = 0; w < 256 / 64; ++w) sum += scratch[w];
    return sum;
}

// population standard deviation of premix[s, ref_mic, :]: one workgroup per source; lane i adds samples i, i + 256, ...
__global__ __launch_bounds__(256) void room_std_kernel(const double* __restrict__ premix, int M, int n_out, int ref_mic,
                                                        double* __restrict__ std) {
    __shared__ double scratch[256 / 64];
    const double* x = premix + ((size_t)blockIdx.x * M + ref_mic) * n_out;
    double sum = 0.;
    for (int t = threadIdx.x; t < n_out; t += 256) sum += x[t];
    const double mean = room_block_sum(sum, scratch) / (double)n_out;
    double sq = 0.;
    for (int t = threadIdx.x; t < n_out; t += 256) {
        const double d = x[t] - mean;
        sq = fma(d, d, sq);
    }
    const double var = room_block_sum(sq, scratch) / (double)n_out;
    if (threadIdx.x == 0) std[blockIdx.x] = sqrt(var);
}

// one thread per (t, m): the sources in order, targets into mix and their own ref, the rest into the background
__global__ __launch_bounds__(256) void room_mix_kernel(const double* __restrict__ premix, const double* __restrict__ std,
                                                        const double* __restrict__ scale, const double* __restrict__ noise,
                                                        double sigma_n, int S, int M, int K, int n_out, double* __restrict__ mix,
                                                        double* __restrict__ ref) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // t * M + m
    const long long total = (long long)n_out * M;
    if (idx >= total) return;
    const int t = (int)(idx / M), m = (int)(idx - (long long)t * M);
    double target = 0., back = 0.;
    for (int s = 0; s < S; ++s) {
        const double v = premix[((size_t)s * M + m) * n_out + t] / std[s] * scale[s];
        if (s < K) {
            ref[(size_t)s * total + idx] = v;
            target += v;
        } else {
            back += v;
        }
    }
    if (noise) back += sigma_n * noise[idx];
    ref[(size_t)K * total + idx] = back;
    mix[idx] = target + back;
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
hipError_t launch_room_kmax(hipStream_t s, const RoomRec* rooms, const double* src, const double* mic, const char4* images, int n_img,
                            int B, int S, int M, double fs_over_c, int* kmax) {
    hipLaunchKernelGGL(room_kmax_kernel, dim3(S * M, B), dim3(kRirThreads), 0, s, rooms, src, mic, images, n_img, S, M, fs_over_c, kmax);
    return hipGetLastError();
}

hipError_t launch_room_rir(hipStream_t s, const RoomRec* rooms, const double* src, const double* mic, const char4* images, int n_img,
                           int B, int S, int M, int max_Lr, double fs_over_c, double* rir) {
    hipLaunchKernelGGL(room_rir_kernel, dim3((max_Lr + kRirSlab - 1) / kRirSlab, S * M, B), dim3(kRirThreads), 0, s, rooms, src, mic,
                       images, n_img, S, M, fs_over_c, rir);
    return hipGetLastError();
}

hipError_t launch_room_pad(hipStream_t s, const double* src, long long src_stride, int len, double* dst, int nfft, int rows) {
    hipLaunchKernelGGL(room_pad_kernel, dim3((nfft + 255) / 256, rows), dim3(256), 0, s, src, src_stride, len, dst, nfft);
    return hipGetLastError();
}

hipError_t launch_room_product(hipStream_t s, double2* H, const double2* X, int nf, int S, int M) {
    hipLaunchKernelGGL(room_product_kernel, dim3((nf + 255) / 256, S * M), dim3(256), 0, s, H, X, nf, M);
    return hipGetLastError();
}

hipError_t launch_room_unpack(hipStream_t s, const double* y, int nfft, double* premix, int n_out, int rows) {
    hipLaunchKernelGGL(room_unpack_kernel, dim3((n_out + 255) / 256, rows), dim3(256), 0, s, y, nfft, premix, n_out);
    return hipGetLastError();
}

hipError_t launch_room_std(hipStream_t s, const double* premix, int S, int M, int n_out, int ref_mic, double* std) {
    hipLaunchKernelGGL(room_std_kernel, dim3(S), dim3(256), 0, s, premix, M, n_out, ref_mic, std);
    return hipGetLastError();
}

hipError_t launch_room_mix(hipStream_t s, const double* premix, const double* std, const double* scale, const double* noise,
                           double sigma_n, int S, int M, int K, int n_out, double* mix, double* ref) {
    const long long total = (long long)n_out * M;
    hipLaunchKernelGGL(room_mix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, premix, std, scale, noise, sigma_n, S, M,
                       K, n_out, mix, ref);
    return hipGetLastError();
}

}  // namespace oiva
