// Kernels of the device random generator (rng.hip: oiva_rng_*): seeded standard normals for the sensor noise and
// the filler row of the sweep, so that neither crosses the bus.
//
// The generator is Philox-4x64-10, a counter-based one: block j of a stream is a pure function of the stream's key (k0, k1) and of
// the counter (j, purpose, 0, 0), and gives four 64-bit words.  Word w becomes u = ((w >> 12) + 0.5) 2^-52, exact in float64 and
// strictly inside (0, 1); words 0, 1 and words 2, 3 each become a Box-Muller pair r cos(2 pi u_b), r sin(2 pi u_b) with
// r = sqrt(-2 ln u_a).  Element n of a stream is value n mod 4 of block n div 4: a stream is a prefix of every longer one, and no
// value depends on the batch, on the stream's place in it or on the launch geometry.
//
//   streams  one record per stream: its key, the first element of its values in the packed output, its length
//   out      packed float64, stream after stream; a stream's base is 8-byte aligned and no more when the lengths before it sum to
//            an odd number
//
// One lane per block.  The 128-bit products are __umul64hi and the low product; the angle goes through sinpi / cospi of 2 u < 2,
// which need no large-argument reduction (the reduction of sin / cos is what puts a table walk into scratch memory).  A lane
// writes only the values of its block that lie below the stream's length: in the packed output the ones behind belong to the next
// stream and to another lane.
#include "oiva_device.h"

namespace oiva {
namespace {

constexpr unsigned long long kPhiloxM0 = 0xD2E7470EE14C6C93ull, kPhiloxM1 = 0xCA5A826395121157ull;
constexpr unsigned long long kPhiloxW0 = 0x9E3779B97F4A7C15ull, kPhiloxW1 = 0xBB67AE8584CAA73Bull;

struct Words4 {
    unsigned long long w0, w1, w2, w3;
};

// the ten rounds on the counter (j, purpose, 0, 0) under the key (k0, k1)
__device__ __forceinline__ Words4 philox4x64_10(unsigned long long j, unsigned long long purpose, unsigned long long k0,
                                                unsigned long long k1) {
    unsigned long long c0 = j, c1 = purpose, c2 = 0, c3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long hi0 = __umul64hi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const unsigned long long hi1 = __umul64hi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return Words4{c0, c1, c2, c3};
}

// u in (0, 1): the top 52 bits, moved half a step off the grid (an integer below 2^52 plus one half is exact in float64)
__device__ __forceinline__ double unit_open(unsigned long long w) { return ((double)(w >> 12) + 0.5) * 0x1p-52; }

__device__ __forceinline__ double2 box_muller(unsigned long long wa, unsigned long long wb) {
    const double r = sqrt(-2. * log(unit_open(wa)));
    const double t = 2. * unit_open(wb);                        // the angle over pi, in (0, 2): exact
    return make_double2(r * cospi(t), r * sinpi(t));
}

// stream blockIdx.y, the blocks blockIdx.x * 256 + threadIdx.x, + gridDim.x * 256, ...
__global__ __launch_bounds__(256) void rng_normal_kernel(const RngStream* __restrict__ streams, unsigned long long purpose,
                                                          double* __restrict__ out) {
    const RngStream s = streams[blockIdx.y];
    const long long blocks = (s.count + 3) >> 2, stride = (long long)gridDim.x * 256;
    double* dst = out + s.off;
    const bool aligned16 = (reinterpret_cast<unsigned long long>(dst) & 15ull) == 0;      // (uniform)
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < blocks; j += stride) {
        const Words4 w = philox4x64_10((unsigned long long)j, purpose, s.k0, s.k1);
        const double2 a = box_muller(w.w0, w.w1), b = box_muller(w.w2, w.w3);
        const long long n = j << 2;
        if (n + 4 <= s.count) {
            if (aligned16) {
                reinterpret_cast<double2*>(dst + n)[0] = a;
                reinterpret_cast<double2*>(dst + n)[1] = b;
            } else {
                dst[n] = a.x, dst[n + 1] = a.y, dst[n + 2] = b.x, dst[n + 3] = b.y;
            }
        } else {                                                // the stream's last block, cut: 1..3 values are its own
            dst[n] = a.x;
            if (n + 1 < s.count) dst[n + 1] = a.y;
            if (n + 2 < s.count) dst[n + 2] = b.x;
        }
    }
}

// test hook: the raw words of blocks first .. first + n - 1, four per block
__global__ __launch_bounds__(256) void rng_raw_kernel(unsigned long long k0, unsigned long long k1, unsigned long long purpose,
                                                       unsigned long long first, int n, unsigned long long* __restrict__ words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Words4 w = philox4x64_10(first + (unsigned long long)i, purpose, k0, k1);
    unsigned long long* dst = words + (size_t)i * 4;
    dst[0] = w.w0, dst[1] = w.w1, dst[2] = w.w2, dst[3] = w.w3;
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------
hipError_t launch_rng_normal(hipStream_t s, const RngStream* streams, int n_streams, long long max_count, unsigned long long purpose,
                             double* out) {
    const long long blocks = (max_count + 3) >> 2;
    const long long groups = std::min<long long>(std::max<long long>((blocks + 255) / 256, 1), kRngMaxGridX);
    hipLaunchKernelGGL(rng_normal_kernel, dim3((unsigned)groups, (unsigned)n_streams), dim3(256), 0, s, streams, purpose, out);
    return hipGetLastError();
}

hipError_t launch_rng_raw(hipStream_t s, unsigned long long k0, unsigned long long k1, unsigned long long purpose,
                          unsigned long long first, int n, unsigned long long* words) {
    hipLaunchKernelGGL(rng_raw_kernel, dim3((n + 255) / 256), dim3(256), 0, s, k0, k1, purpose, first, n, words);
    return hipGetLastError();
}

}  // namespace oiva
