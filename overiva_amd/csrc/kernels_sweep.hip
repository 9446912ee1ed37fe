// Kernels of sweep_batch (sweep.hip: oiva_sweep_*): the hand-overs between the room simulation, the batched STFT
// and BSS Eval on the device.  Nothing here is arithmetic of a solver: a cast, a statistic that is used only for an ordering, and
// exact gathers.
//
//   x       packed (n) float64 -> float32, round to nearest even (the host's ndarray.astype(np.float32))
//   y       packed (sum_b T_b hop, C) float32, the synthesis of the batched STFT: room b's (ny_b, C) at rooms[b].y_off samples
//   std     (B, 8): population standard deviation of every channel of every room over all ny_b samples, float64, two passes
//   order   (B, 8): the channels by descending std, an exact tie to the lower index (numpy.argsort(-std, kind="stable"))
//   est/ref packed (sum_b N m_b), N = K + 1: room b's (N, m_b) rows at rooms[b].sig_off, the layout launch_bss_lags reads
//
// A workgroup never holds two rooms, the chunks of a room are kSweepChunk samples whatever B is, and every sum is added in a
// fixed order (the lanes' strided sums, the wave's shuffle tree, the waves in order, the chunks in order): no atomics on
// floating-point numbers, and a room's values do not depend on B or on its place in the batch.
#include "oiva_device.h"

namespace oiva {
namespace {

// block-wide sum in a fixed order: the wave's shuffle tree, then the waves in order; every thread gets the sum
__device__ __forceinline__ double sweep_block_sum(double v, double* scratch) {
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

// a lane converts two neighbours: a wave reads 1024 contiguous bytes (eight cache lines) and writes 512 (four) per step
__global__ __launch_bounds__(256) void sweep_cast_kernel(const double* __restrict__ in, float* __restrict__ out, long long n) {
    const long long pairs = n >> 1, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += stride) {
        const double2 v = reinterpret_cast<const double2*>(in)[i];
        reinterpret_cast<float2*>(out)[i] = make_float2((float)v.x, (float)v.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = (float)in[n - 1];
}

// Standard deviation of the C channels of room blockIdx.y in three launches of one kernel:
//   pass 0: part[0][b][c][j] = the sum of chunk j = blockIdx.x
//   pass 1: part[1][b][c][j] = the sum of (v - mean)^2 of the chunk, mean = (chunks of pass 0 added in order) / ny
//   pass 2: std[b][c] = sqrt((chunks of pass 1 added in order) / ny), lane c of workgroup (0, b)
// A lane takes whole samples: the C loads of a wave cover one contiguous run of 64 C floats.
__global__ __launch_bounds__(256) void sweep_std_kernel(const float* __restrict__ y, const SweepRoom* __restrict__ rooms, int C,
                                                         int max_chunks, int pass, double* __restrict__ part,
                                                         double* __restrict__ std) {
    __shared__ double scratch[256 / 64];
    const int b = blockIdx.y, j = blockIdx.x;
    const SweepRoom r = rooms[b];
    const int chunks = (r.ny + kSweepChunk - 1) / kSweepChunk;
    if (j >= chunks) return;                                   // (uniform)
    const size_t per_pass = (size_t)gridDim.y * kSweepMaxChan * max_chunks;
    double* mine = part + ((size_t)b * kSweepMaxChan) * max_chunks;
    if (pass == 2) {
        if (j == 0 && (int)threadIdx.x < C) {
            const double* p = mine + per_pass + (size_t)threadIdx.x * max_chunks;
            double sum = 0.;
            for (int q = 0; q < chunks; ++q) sum += p[q];
            std[b * kSweepMaxChan + threadIdx.x] = sqrt(sum / (double)r.ny);
        }
        return;
    }
    double mean[kSweepMaxChan], acc[kSweepMaxChan];
#pragma unroll
    for (int c = 0; c < kSweepMaxChan; ++c) {
        mean[c] = acc[c] = 0.;
        if (pass == 1 && c < C) {
            const double* p = mine + (size_t)c * max_chunks;
            double sum = 0.;
            for (int q = 0; q < chunks; ++q) sum += p[q];
            mean[c] = sum / (double)r.ny;
        }
    }
    const float* x = y + (size_t)r.y_off * C;
    const int i1 = min(r.ny, (j + 1) * kSweepChunk);
    for (int i = j * kSweepChunk + threadIdx.x; i < i1; i += 256) {
#pragma unroll
        for (int c = 0; c < kSweepMaxChan; ++c)
            if (c < C) {
                const double d = (double)x[(size_t)i * C + c] - mean[c];
                acc[c] = pass == 1 ? fma(d, d, acc[c]) : acc[c] + d;
            }
    }
#pragma unroll
    for (int c = 0; c < kSweepMaxChan; ++c)
        if (c < C) {                                           // (uniform)
            const double sum = sweep_block_sum(acc[c], scratch);
            if (threadIdx.x == 0) mine[(size_t)pass * per_pass + (size_t)c * max_chunks + j] = sum;
        }
}

// one lane per room: channel c goes to the place of its rank, the number of channels that come before it.  A value that is not
// a number counts as the smallest, as numpy.argsort places it.
__global__ __launch_bounds__(64) void sweep_order_kernel(const double* __restrict__ std, int B, int C, int reorder,
                                                          int* __restrict__ order) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double s[kSweepMaxChan];
#pragma unroll
    for (int c = 0; c < kSweepMaxChan; ++c) {
        const double v = c < C ? std[b * kSweepMaxChan + c] : 0.;
        s[c] = v == v ? v : -1.;                               // (a standard deviation is >= 0)
    }
#pragma unroll
    for (int c = 0; c < kSweepMaxChan; ++c) {
        if (c >= C) continue;
        int rank = 0;
#pragma unroll
        for (int d = 0; d < kSweepMaxChan; ++d)
            if (d < C && (s[d] > s[c] || (s[d] == s[c] && d < c))) ++rank;
        order[b * kSweepMaxChan + (reorder ? rank : c)] = c;
    }
}

// est and ref of room blockIdx.y, 256 samples per workgroup, one per lane.  A lane reads its sample's whole run of C floats --
// the C loads of a wave cover 64 C contiguous floats, every cache line of y is fetched once -- and keeps the K channels the
// order names.  Of the references only the microphone ref_mic is wanted: a wave's loads touch the contiguous run of 64 M
// doubles of its samples and use one in M, which is what the (K + 1, n_out, M) layout costs.  Every store is unit-stride.
__global__ __launch_bounds__(256) void sweep_align_kernel(const float* __restrict__ y, const double* __restrict__ room_ref,
                                                           const double* __restrict__ filler, const int* __restrict__ order,
                                                           const SweepRoom* __restrict__ rooms, int C, int M, int K, int ref_mic,
                                                           int offset, double* __restrict__ est, double* __restrict__ ref) {
    const int b = blockIdx.y;
    const SweepRoom r = rooms[b];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.m) return;
    int ord[kSweepMaxChan];
#pragma unroll
    for (int k = 0; k < kSweepMaxChan; ++k) ord[k] = k < K ? order[b * kSweepMaxChan + k] : -1;
    float keep[kSweepMaxChan];
#pragma unroll
    for (int k = 0; k < kSweepMaxChan; ++k) keep[k] = 0.f;
    const float* x = y + ((size_t)r.y_off + (size_t)(i + offset)) * C;
#pragma unroll
    for (int c = 0; c < kSweepMaxChan; ++c)
        if (c < C) {
            const float v = x[c];
#pragma unroll
            for (int k = 0; k < kSweepMaxChan; ++k) keep[k] = ord[k] == c ? v : keep[k];
        }
    double* e = est + r.sig_off + i;
    double* o = ref + r.sig_off + i;
    const double* src = room_ref + r.ref_off + (size_t)i * M + ref_mic;
#pragma unroll
    for (int k = 0; k < kSweepMaxChan; ++k)
        if (k < K) {
            e[(size_t)k * r.m] = (double)keep[k];
            o[(size_t)k * r.m] = src[(size_t)k * r.n_out * M];
        }
    e[(size_t)K * r.m] = filler[r.fil_off + i];
    o[(size_t)K * r.m] = src[(size_t)K * r.n_out * M];
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
hipError_t launch_sweep_cast(hipStream_t s, const double* in, float* out, long long n) {
    const long long blocks = std::min<long long>(((n >> 1) + 255) / 256, 65535);
    hipLaunchKernelGGL(sweep_cast_kernel, dim3((unsigned)std::max<long long>(blocks, 1)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

hipError_t launch_sweep_std(hipStream_t s, const float* y, const SweepRoom* rooms, int B, int C, int max_chunks, double* part,
                            double* std) {
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(sweep_std_kernel, dim3(pass == 2 ? 1 : max_chunks, B), dim3(256), 0, s, y, rooms, C, max_chunks, pass, part,
                           std);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_sweep_order(hipStream_t s, const double* std, int B, int C, int reorder, int* order) {
    hipLaunchKernelGGL(sweep_order_kernel, dim3((B + 63) / 64), dim3(64), 0, s, std, B, C, reorder, order);
    return hipGetLastError();
}

hipError_t launch_sweep_align(hipStream_t s, const float* y, const double* room_ref, const double* filler, const int* order,
                              const SweepRoom* rooms, int B, int C, int M, int K, int ref_mic, int offset, int max_m, double* est,
                              double* ref) {
    hipLaunchKernelGGL(sweep_align_kernel, dim3((max_m + 255) / 256, B), dim3(256), 0, s, y, room_ref, filler, order, rooms, C, M, K,
                       ref_mic, offset, est, ref);
    return hipGetLastError();
}

}  // namespace oiva
