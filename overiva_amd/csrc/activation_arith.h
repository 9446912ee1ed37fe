// Source activation of one workgroup of batch_activation_kernel (kernels_batch.hip), reference overiva.py:152-155: the arithmetic
// and canonical order of activation_kernel (kernels_misc.hip), so a problem's r is that of its single-problem plan.
// (activation_kernel keeps its own copy: the single-problem kernels stay the code the benchmarks timed.)
#pragma once
#include "oiva_device.h"

namespace oiva {

// Canonical sum over `count` parts starting at part `first` of one (frame, source) element -- the parts in blocks of `bs`
// consecutive ones counted from part 0, each block added sequentially, then the block sums sequentially (see
// activation_kernel) -- with the loads of up to NP parts IN FLIGHT TOGETHER: the kernel is a chain of round trips to
// data other XCDs wrote, and round 4's form made one trip per block (8 at the headline shape: 5.6 us against 4.5 for the
// plain sequential sum of round 3).  State (p, pb) carries over chunks of NP parts; a block boundary is a select.
template <int NP>
struct BatchCanonSum {
    float p = 0.f, pb = 0.f;
    // parts [i0, i0 + NP) of which those < i1 exist; a block ends after part i when (i + 1) % bs == 0
    __device__ __forceinline__ void chunk(const float* __restrict__ parts, size_t n, size_t e, int i0, int i1, int bs) {
        float v[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) v[u] = i0 + u < i1 ? parts[(size_t)(i0 + u) * n + e] : 0.f;
        int left = bs - i0 % bs;                       // parts until the current block is complete
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            pb += v[u];                                // (a + 0.f is exact: parts past i1 change nothing)
            const bool end = --left == 0;
            p = end ? p + pb : p;
            pb = end ? 0.f : pb;
            left = end ? bs : left;
        }
    }
    __device__ __forceinline__ float total() const { return p + pb; }       // the last block may be short (pb = 0.f if not: exact)
};

// frames [bx * kBlock, bx * kBlock + kBlock) of source `by`: R[t,k] from the parts, and the float64 sum of this block's r
// behind R (rsum_offset_floats); wsum: kWaves doubles of LDS
template <int NP>
__device__ __forceinline__ void activation_block(const float* __restrict__ parts, int nparts, float* __restrict__ R, int T,
                                                 int K, int model, float inv_f_total, unsigned bx, unsigned by, double* wsum) {
    const int t = bx * kBlock + threadIdx.x;      // grid = (blocks of kBlock frames, sources)
    const int k = by;
    const size_t n = (size_t)T * K;
    float r = 0.f;
    if (t < T) {
        const size_t e = (size_t)t * K + k;
        // Canonical order of the sum over the parts (all paths of the library, whatever the number of GPUs): the parts in
        // blocks of ceil(nparts / 8) consecutive ones -- at most 8 blocks --, each block added sequentially, then the block
        // sums sequentially.  A rank of a sharded run that holds whole blocks can send their sums instead of its parts and
        // every rank still forms the SAME sum: the same bits of r at 1, 2, 4 and 8 GPUs (activation_xchg_kernel).  Up to 8
        // parts the order is the plain sequential one.
        const int bs = (nparts + kCanonBlocks - 1) / kCanonBlocks;
        BatchCanonSum<NP> cs;
        for (int i0 = 0; i0 < nparts; i0 += NP) cs.chunk(parts, n, e, i0, nparts, bs);
        // (a short last block: p + pb; complete blocks leave pb = 0.f and p + 0.f is exact -- but p = 0.f + pb for a single
        //  block must not become (0.f + pb) + 0.f with a different rounding: it is not, x + 0.f = x)
        const float p = cs.total();
        r = model == OIVA_MODEL_LAPLACE ? 2.f * sqrtf(p) : (model == kModelOgiveLaplace ? sqrtf(p * inv_f_total) : p * inv_f_total);
        R[e] = r;
    }
    double s = (double)r;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) tot += wsum[w];
        reinterpret_cast<double*>(R + rsum_offset_floats(T, K))[(size_t)bx * K + k] = tot;
    }
}

}  // namespace oiva
