// Kernel of the decay measurement (decay.hip: oiva_decay_*): the Schroeder integral E[n] = sum_{k >= n} h[k]^2 of
// every response of a packed batch, the two threshold crossings of the curve and the masked sums of the least-squares fit, in
// float64.
//
//   recs     one record per response: the first element of its samples in the packed input, its length (1 .. 2^24)
//   in       packed float64, response after response; a response's base is 8-byte aligned and no more when the lengths before it
//            sum to an odd number
//   curve    null, or packed like `in`: E[n] of every response
//
// One 256-lane workgroup per response.  The response is cut into tiles of kDecayTile = 1024 samples COUNTED FROM SAMPLE 0 (the
// last tile may be cut; what it lacks counts as zeros) and walked from the last tile to the first; in a tile lane t owns the
// samples 4 t .. 4 t + 3.  The order of every sum is a function of (n, L) alone:
//   in the lane   s3 = q3, s2 = q2 + s3, s1 = q1 + s2, s0 = q0 + s1                                    (q = h^2, one rounding)
//   in the wave   a Hillis-Steele suffix scan of s0 over the 64 lanes, steps 1, 2, 4, .. 32; x = the scan's value one lane up
//                 (0 in lane 63); the wave's total is s0 + x of its lane 0
//   in the tile   the totals of the later waves, the last first: m = ((t3 + t2) + t1) ... down to the wave's own
//   E[n]          = ((s_e + x) + m) + carry, and the carry of the next (earlier) tile is ((m + t) of wave 0) + carry = its E at the
//                 tile's first sample
// so a response has the same bits alone, in any batch, at any place in it; no atomics, no workgroup waits for another.  Two walks:
// the first leaves E[0], the second forms the same bits again and holds every E[n] against theta_a = E[0] fa and theta_b = E[0] fb:
// i_a, i_b = the smallest n with E[n] <= theta (an integer min), and over theta_b < E[n] <= theta_a the sums of
// D = 10 log10(E[n] / E[0]) and of n D, each lane adding its own samples tile by tile, then a fixed tree over the workgroup.
// Products are rounded on their own (no contraction into the sums): the vector and the scalar load path give the same bits.
#include <climits>

#include "oiva_device.h"

#pragma clang fp contract(off)

namespace oiva {
namespace {

constexpr int kDecayPerLane = kDecayTile / kBlock;
static_assert(kDecayPerLane == 4, "a lane takes two 16-byte loads per tile");

// the squares of this lane's four samples of the tile that starts at `base`; samples at or behind L count as zeros
__device__ __forceinline__ void decay_squares(const double* __restrict__ h, int L, int base, bool aligned16, double (&q)[kDecayPerLane]) {
    const int n0 = base + kDecayPerLane * (int)threadIdx.x;
    double v[kDecayPerLane];
    if (aligned16 && base + kDecayTile <= L) {      // (uniform: a whole tile of an aligned response)
        const double2 a = reinterpret_cast<const double2*>(h + n0)[0], b = reinterpret_cast<const double2*>(h + n0)[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
#pragma unroll
        for (int e = 0; e < kDecayPerLane; ++e) v[e] = n0 + e < L ? h[n0 + e] : 0.;
    }
#pragma unroll
    for (int e = 0; e < kDecayPerLane; ++e) q[e] = v[e] * v[e];
}

// q -> the suffix sums inside the lane; returns what lies behind the lane inside the tile, ((x) + m) as two terms, and the tile's
// total.  tot: kWaves doubles of LDS, another set than the tile before used (one barrier per tile)
__device__ __forceinline__ void decay_tile_suffix(double (&q)[kDecayPerLane], double* tot, double* in_wave, double* later_waves,
                                                  double* tile_total) {
    q[2] += q[3];
    q[1] += q[2];
    q[0] += q[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc = q[0];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_down(inc, off, 64);
        if (lane + off < 64) inc += up;
    }
    double x = __shfl_down(inc, 1, 64);
    if (lane == 63) x = 0.;
    const double wave_total = __shfl(q[0] + x, 0, 64);
    if (lane == 0) tot[wave] = wave_total;
    __syncthreads();
    double m = 0., mine = 0.;
#pragma unroll
    for (int w = kWaves - 1; w >= 0; --w) {
        if (w == wave) mine = m;
        m += tot[w];
    }
    *in_wave = x, *later_waves = mine, *tile_total = m;
}

__device__ __forceinline__ int block_min(int v, int* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = scratch[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = min(m, scratch[w]);
    return m;
}

__global__ __launch_bounds__(kBlock) void decay_kernel(const DecayRec* __restrict__ recs, const double* __restrict__ in, double fa,
                                                       double fb, double* __restrict__ curve, double* __restrict__ e0_out,
                                                       int* __restrict__ idx_out, double* __restrict__ sum_out) {
    __shared__ double tot[2][kWaves];
    __shared__ double red[kWaves];
    __shared__ int redi[kWaves];
    const DecayRec r = recs[blockIdx.x];
    const double* h = in + r.off;
    const int L = r.len, tiles = (L + kDecayTile - 1) / kDecayTile;
    const bool aligned16 = (reinterpret_cast<unsigned long long>(h) & 15ull) == 0;      // (uniform)
    int par = 0;

    // ---- first walk: E[0] ----
    double carry = 0.;
    for (int j = tiles - 1; j >= 0; --j, par ^= 1) {
        double q[kDecayPerLane], x, m, t;
        decay_squares(h, L, j * kDecayTile, aligned16, q);
        decay_tile_suffix(q, tot[par], &x, &m, &t);
        carry = t + carry;
    }
    const double e0 = carry;
    const double theta_a = e0 * fa, theta_b = e0 * fb;

    // ---- second walk: the same bits again, held against the thresholds ----
    double* out = curve ? curve + r.off : nullptr;
    const bool out_aligned16 = (reinterpret_cast<unsigned long long>(out) & 15ull) == 0;      // (a borrowed input may lie otherwise)
    int ia = INT_MAX, ib = INT_MAX;
    double sd = 0., snd = 0.;
    carry = 0.;
    for (int j = tiles - 1; j >= 0; --j, par ^= 1) {
        double q[kDecayPerLane], x, m, t;
        const int base = j * kDecayTile, n0 = base + kDecayPerLane * (int)threadIdx.x;
        decay_squares(h, L, base, aligned16, q);
        decay_tile_suffix(q, tot[par], &x, &m, &t);
        double E[kDecayPerLane];
#pragma unroll
        for (int e = 0; e < kDecayPerLane; ++e) E[e] = ((q[e] + x) + m) + carry;
        carry = t + carry;
#pragma unroll
        for (int e = kDecayPerLane - 1; e >= 0; --e) {      // (the lane's samples from the last to the first, as the tiles go)
            const int n = n0 + e;
            if (n >= L) continue;
            if (E[e] <= theta_a) ia = min(ia, n);
            if (E[e] <= theta_b) ib = min(ib, n);
            if (E[e] <= theta_a && E[e] > theta_b) {
                const double D = 10. * log10(E[e] / e0);
                sd += D;
                const double nD = (double)n * D;
                snd += nD;
            }
        }
        if (out) {
            if (out_aligned16 && base + kDecayTile <= L) {
                reinterpret_cast<double2*>(out + n0)[0] = make_double2(E[0], E[1]);
                reinterpret_cast<double2*>(out + n0)[1] = make_double2(E[2], E[3]);
            } else {
#pragma unroll
                for (int e = 0; e < kDecayPerLane; ++e)
                    if (n0 + e < L) out[n0 + e] = E[e];
            }
        }
    }
    ia = block_min(ia, redi);
    ib = block_min(ib, redi);
    sd = block_sum(sd, red);
    snd = block_sum(snd, red);
    if (threadIdx.x == 0) {
        const bool silent = !(e0 > 0.);      // an all-zero response: every E[n] is 0 = theta, and no crossing is reported
        e0_out[blockIdx.x] = e0;
        idx_out[2 * (size_t)blockIdx.x] = silent || ia == INT_MAX ? -1 : ia;
        idx_out[2 * (size_t)blockIdx.x + 1] = silent || ib == INT_MAX ? -1 : ib;
        sum_out[2 * (size_t)blockIdx.x] = sd;
        sum_out[2 * (size_t)blockIdx.x + 1] = snd;
    }
}

}  // namespace

// ---- launcher ----------------------------------------------------------------------------------------------------------------
hipError_t launch_decay(hipStream_t s, const DecayRec* recs, int n_resp, const double* in, double fa, double fb, double* curve, double* e0,
                        int* idx, double* sums) {
    hipLaunchKernelGGL(decay_kernel, dim3((unsigned)n_resp), dim3(kBlock), 0, s, recs, in, fa, fb, curve, e0, idx, sums);
    return hipGetLastError();
}

}  // namespace oiva
