// Kernels of the batched STFT (oiva_bstft_*, bstft.hip): the passes around hipFFT for B rooms of different lengths at once.
//
//   x       packed (sum n_b, M) float32 audio: room b holds samples [s_off_b, s_off_b + n_b)
//   rooms   (B) BstftRoom records (oiva_internal.h): sample offset, frame offset, T_b = n_b / hop, n_b
//   frames  (sum T_b * C, L) float32: row (t * C + c) is the windowed frame t of channel c, t the GLOBAL frame index
//   spec    (sum T_b * C, F) complex64, F = L / 2 + 1: what hipFFT writes (analysis) or reads (synthesis)
//   X / Y   (sum T_b, F, C) complex64: the solver's layout, a dense batch's (B, T, F, C) when all T_b agree
//   y       packed (sum T_b * hop, K) float32
//
// Every pass is a pure stream (each byte read once and written once; the framing re-reads its L / hop overlapping
// samples from the cache) and is built the same way: a workgroup reads one contiguous run, stages it in the LDS as
// [channel][index] rows and writes contiguous runs again, so both sides of every transpose are coalesced.  The LDS row
// stride S is chosen by the host (bstft_lds_stride) so that the 32 lanes the LDS serves per cycle, which in the
// interleaved phase touch 32 / C indices of C rows, fall on 32 different banks: S = 32 / C (mod 32).
// The arithmetic per element is stft.hip's: x * win_a in float32; win_s * frame summed over the covering frames in
// increasing t, then * (1 / L).  Nothing crosses a room boundary: a frame's samples before its room's first are zero, and an
// output sample sums frames of its own room only.
#include "oiva_internal.h"

namespace oiva {
namespace {

constexpr int kTile = kBlock;      // samples / bins / output samples per workgroup tile (one per lane)

// the room that holds global frame tg: the last record whose t_off <= tg (every room has T >= 1, so t_off increases strictly)
__device__ __forceinline__ int room_of_frame(const BstftRoom* __restrict__ rooms, int B, long long tg) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rooms[mid].t_off <= tg)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// framing + window: grid (global frame, tile of kTile frame positions).  The tile's positions of all C channels are
// kTile * C contiguous floats of the interleaved audio.  VEC (C % 4 == 0 and L % 4 == 0): 128-bit reads and writes.
template <int C, bool VEC>
__global__ __launch_bounds__(kBlock) void bstft_frame_kernel(const float* __restrict__ x, const float* __restrict__ win,
                                                             float* __restrict__ frames, const BstftRoom* __restrict__ rooms,
                                                             int B, int L, int hop, int S) {
    extern __shared__ __attribute__((aligned(16))) float sf[];      // [C][S]
    const long long tg = blockIdx.x;
    const int n0 = blockIdx.y * kTile;
    const int nt = min(kTile, L - n0);
    const BstftRoom r = rooms[room_of_frame(rooms, B, tg)];
    const long long s0 = (tg - r.t_off) * hop - (L - hop) + n0;     // room-local sample of the tile's first position
    const float* xr = x + r.s_off * C;
    if constexpr (VEC) {
        constexpr int V = C / 4;                    // float4 per sample
        for (int i = threadIdx.x; i < nt * V; i += kBlock) {
            const int n = i / V, c0 = 4 * (i % V);
            const long long s = s0 + n;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s >= 0 && s < r.n) v = *reinterpret_cast<const float4*>(xr + s * C + c0);
            sf[(c0 + 0) * S + n] = v.x;
            sf[(c0 + 1) * S + n] = v.y;
            sf[(c0 + 2) * S + n] = v.z;
            sf[(c0 + 3) * S + n] = v.w;
        }
        __syncthreads();
        const int q = nt / 4;                                       // float4 per row of the tile
        for (int i = threadIdx.x; i < q * C; i += kBlock) {
            const int c = i / q, n = 4 * (i % q);
            float4 v = *reinterpret_cast<const float4*>(sf + c * S + n);
            if (win) {
                const float4 w = *reinterpret_cast<const float4*>(win + n0 + n);
                v.x *= w.x, v.y *= w.y, v.z *= w.z, v.w *= w.w;
            }
            *reinterpret_cast<float4*>(frames + (tg * C + c) * L + n0 + n) = v;
        }
    } else {
        for (int i = threadIdx.x; i < nt * C; i += kBlock) {
            const int n = i / C, c = i % C;
            const long long s = s0 + n;
            sf[c * S + n] = (s >= 0 && s < r.n) ? xr[s * C + c] : 0.f;
        }
        __syncthreads();
        const int n = threadIdx.x;
        if (n < nt) {
            const float w = win ? win[n0 + n] : 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) frames[(tg * C + c) * L + n0 + n] = sf[c * S + n] * w;
        }
    }
}

// spec (frame * C + c, F) -> X (frame, F, C): grid (global frame, tile of kTile bins)
template <int C>
__global__ __launch_bounds__(kBlock) void bstft_to_tfc_kernel(const float2* __restrict__ spec, float2* __restrict__ X, int F, int S) {
    extern __shared__ __attribute__((aligned(16))) float2 sc[];     // [C][S]
    const long long tg = blockIdx.x;
    const int f0 = blockIdx.y * kTile;
    const int nf = min(kTile, F - f0);
    const int f = threadIdx.x;
    if (f < nf) {
#pragma unroll
        for (int c = 0; c < C; ++c) sc[c * S + f] = spec[(tg * C + c) * F + f0 + f];
    }
    __syncthreads();
    float2* out = X + (tg * F + f0) * C;
    for (int i = threadIdx.x; i < nf * C; i += kBlock) out[i] = sc[(i % C) * S + i / C];
}

// Y (frame, F, C) -> spec (frame * C + c, F)
template <int C>
__global__ __launch_bounds__(kBlock) void bstft_from_tfc_kernel(const float2* __restrict__ Y, float2* __restrict__ spec, int F, int S) {
    extern __shared__ __attribute__((aligned(16))) float2 sc[];     // [C][S]
    const long long tg = blockIdx.x;
    const int f0 = blockIdx.y * kTile;
    const int nf = min(kTile, F - f0);
    const float2* in = Y + (tg * F + f0) * C;
    for (int i = threadIdx.x; i < nf * C; i += kBlock) sc[(i % C) * S + i / C] = in[i];
    __syncthreads();
    const int f = threadIdx.x;
    if (f < nf) {
#pragma unroll
        for (int c = 0; c < C; ++c) spec[(tg * C + c) * F + f0 + f] = sc[c * S + f];
    }
}

// overlap-add as a gather: grid (tile of kTile packed output samples).  Output sample s of a room sums, in increasing t, the
// frames of THAT room that cover it (stft.hip, overlap_add_kernel); the tile's C channels leave as kTile * C contiguous floats.
template <int C>
__global__ __launch_bounds__(kBlock) void bstft_overlap_add_kernel(const float* __restrict__ frames, const float* __restrict__ win,
                                                                   float* __restrict__ y, const BstftRoom* __restrict__ rooms, int B,
                                                                   int L, int hop, long long n_out, int S) {
    extern __shared__ __attribute__((aligned(16))) float sf[];      // [C][S]
    const long long g0 = (long long)blockIdx.x * kTile;
    const long long g = g0 + threadIdx.x;
    if (g < n_out) {
        const BstftRoom r = rooms[room_of_frame(rooms, B, g / hop)];    // output sample g lies in the hop of global frame g / hop
        const long long s = g - r.t_off * hop;
        const long long pos = s + (L - hop);                 // position on the axis that includes the zero state
        long long t_hi = pos / hop;                          // last frame covering pos
        if (t_hi > r.T - 1) t_hi = r.T - 1;
        long long t_lo = (pos - L) / hop + 1;                // first frame with t*hop + L > pos
        if (pos - L < 0) t_lo = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (long long t = t_lo; t <= t_hi; ++t) {
                const int n = (int)(pos - t * hop);
                if (n >= 0 && n < L) acc += frames[((r.t_off + t) * C + c) * L + n] * (win ? win[n] : 1.f);
            }
            sf[c * S + threadIdx.x] = acc * (1.f / (float)L);
        }
    }
    __syncthreads();
    const long long left = (n_out - g0) * C;
    float* out = y + g0 * C;
    for (int i = threadIdx.x; i < kTile * C && i < left; i += kBlock) out[i] = sf[(i % C) * S + i / C];
}

#define OIVA_BSTFT_DISPATCH_C(CALL) \
    switch (C) {                    \
        case 1: CALL(1); break;     \
        case 2: CALL(2); break;     \
        case 3: CALL(3); break;     \
        case 4: CALL(4); break;     \
        case 5: CALL(5); break;     \
        case 6: CALL(6); break;     \
        case 7: CALL(7); break;     \
        case 8: CALL(8); break;     \
        default: return hipErrorInvalidValue; \
    }

}  // namespace

int bstft_lds_stride(int C) {
    const int want = ((32 + C - 1) / C) % 32;
    int s = kTile;
    while (s % 32 != want) ++s;
    return s;
}

hipError_t launch_bstft_frame(hipStream_t s, const float* x, const float* win, float* frames, const BstftRoom* rooms, int B,
                              long long frames_total, int C, int L, int hop) {
    const int S = bstft_lds_stride(C);
    const dim3 grid((unsigned)frames_total, (unsigned)((L + kTile - 1) / kTile));
    const size_t shmem = (size_t)C * S * sizeof(float);
    const bool vec = C % 4 == 0 && L % 4 == 0;
#define CALL(CC)                                                                                                                  \
    if (vec) hipLaunchKernelGGL((bstft_frame_kernel<CC, (CC % 4 == 0)>), grid, dim3(kBlock), shmem, s, x, win, frames, rooms, B, L, hop, S); \
    else hipLaunchKernelGGL((bstft_frame_kernel<CC, false>), grid, dim3(kBlock), shmem, s, x, win, frames, rooms, B, L, hop, S);
    OIVA_BSTFT_DISPATCH_C(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_bstft_to_tfc(hipStream_t s, const float2* spec, float2* X, long long frames_total, int F, int C) {
    const int S = bstft_lds_stride(C);
    const dim3 grid((unsigned)frames_total, (unsigned)((F + kTile - 1) / kTile));
    const size_t shmem = (size_t)C * S * sizeof(float2);
#define CALL(CC) hipLaunchKernelGGL((bstft_to_tfc_kernel<CC>), grid, dim3(kBlock), shmem, s, spec, X, F, S);
    OIVA_BSTFT_DISPATCH_C(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_bstft_from_tfc(hipStream_t s, const float2* Y, float2* spec, long long frames_total, int F, int C) {
    const int S = bstft_lds_stride(C);
    const dim3 grid((unsigned)frames_total, (unsigned)((F + kTile - 1) / kTile));
    const size_t shmem = (size_t)C * S * sizeof(float2);
#define CALL(CC) hipLaunchKernelGGL((bstft_from_tfc_kernel<CC>), grid, dim3(kBlock), shmem, s, Y, spec, F, S);
    OIVA_BSTFT_DISPATCH_C(CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_bstft_overlap_add(hipStream_t s, const float* frames, const float* win, float* y, const BstftRoom* rooms, int B,
                                    long long n_out, int C, int L, int hop) {
    const int S = bstft_lds_stride(C);
    const dim3 grid((unsigned)((n_out + kTile - 1) / kTile));
    const size_t shmem = (size_t)C * S * sizeof(float);
#define CALL(CC) hipLaunchKernelGGL((bstft_overlap_add_kernel<CC>), grid, dim3(kBlock), shmem, s, frames, win, y, rooms, B, L, hop, n_out, S);
    OIVA_BSTFT_DISPATCH_C(CALL)
#undef CALL
    return hipGetLastError();
}

}  // namespace oiva
