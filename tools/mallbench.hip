// Can a fixed share of X stay in the 256 MiB Infinity Cache while the rest of X streams past it non-temporally?
//
// Pure-read forms of the two headline passes over X (T frames x F bins x 8 channels complex64, 524 MB at 4000 x 2048), same lane
// geometry, same requests, no arithmetic beyond a sum that keeps the loads alive:
//   cov : cov_dma_kernel  -- 16 bins x 16 frame phases per workgroup, splits of `ctc` frames, global_load_lds_dwordx4 into a
//                            4-stage ring per wave (three steps in flight), grid (F / 16, splits)
//   pow : power_kernel    -- 64 bins x 4 frame phases per workgroup, chunks of `tcp` frames, global_load_dwordx4 into registers
//                            (two steps in flight), grid (F / 64, chunks)
// Every step of a wave is 4 frames x 16 bins = four 1-KB rows; a lane takes 16 B at a 64-B lane stride, the four pieces of its 64-B
// vector by four consecutive instructions ("addr": "lane").  "addr": "row" is the row-contiguous form of an nt step: lane l takes
// bytes [16 l, 16 l + 16) of row j in instruction j, into LDS, and reads its own 64-B vector back from there (the covariance
// kernel's ring takes it as it is; the power kernel gets a landing area of one step per step in flight).  Plain steps are
// lane-strided in every row of the table but the rings' ("plain_addr", "cov_plain_addr").
// One policy per frame, the rule of csrc/kernel_choice.h: frames in groups of 16 counted from the start of their covariance
// split, a group resident (plain load) or streamed (nt load, or plain as the control).  Layout `il`: group % 16 < n16 (resident
// and streamed groups interleaved through every split); layout `first`: the first groups of every split.
//
// Every row: flush the cache (memset of another buffer of X's size), read the resident share once with plain loads, then `kPasses`
// passes, each timed by events.  One JSON line per row; pass_us[0] is the pass right behind the priming read.
//   q = "c": nt against plain for the whole buffer, no share; nt lane-strided and row-contiguous
//   q = "a": is the share still there in the later passes?  share swept, layout first, rest nt against rest plain, both kernels
//   q = "b": interleaved against share-first, and the two kernels alternating as in an iteration (kern = "pair")
//   q = "e": the power pass through a per-wave RING of S stages of 4 KB (S = 2, 3, 4; "addr": "ring", "stages": S) with counted
//            vmcnt, as the covariance kernel streams: every wave keeps S - 1 steps in flight all the time, where the landing-area
//            form above loads two steps, waits for both and consumes both.  Chunks walked from their last step to their first, as
//            the kernel does when the pass runs against the covariance pass.  Streamed groups row-contiguous nt; resident groups
//            "plain_addr": "lane" (lane-addressed plain global_load_lds, the covariance kernel's plain step) or "row"
//            (row-contiguous plain).  Shares 0 and 268 MB interleaved, the pass alone and the two passes alternating; the
//            `pow ... addr row` rows of the same shares are repeated beside them as the yardstick of the same run.  Then the same
//            in 8 chunks of 500 frames (one workgroup per CU), and X of one shard of two and of four (262 and 131 MB, all plain,
//            384 workgroups): register loads against the ring.
//   q = "f": the covariance stream through a ring of S = 2, 3, 4 stages ("cov_stages", counted wait (S - 1) * 4), its plain steps
//            lane-addressed or row-contiguous ("cov_plain_addr"), shares 0 and 268 MB interleaved, alone and alternating with the
//            power stream in the kernel's present form (ring of 2 stages, row-contiguous, 8 chunks of 500 frames).  The covariance
//            kernel's present form (4 stages, lane-addressed plain steps) stands in front of and behind every block as the
//            yardstick of the same run.  Then X of one shard of two and of four, all plain, at the shards' splits.
//   q = "d": (the program's first question, docs/HISTORY_rounds_1-3.md §3.1) buffers of 128 .. 500 MiB streamed by 2048 concurrent
//            workgroups, every pass in the same direction against passes of alternating direction
// No step waits on anything but its own kernels; the whole sweep is about 170 rows of 7 launches of < 0.2 ms (1-2 s of GPU time
// behind 1.1 GB of allocations).  Run it under a time limit:
//
//   hipcc -O3 --offload-arch=gfx950 tools/mallbench.hip -o mallbench && timeout -k 10 120 ./mallbench > profiles/mallbench.log
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kM8 = 64;        // bytes of one (frame, bin): 8 channels complex64
constexpr int kPasses = 6;

struct Policy {
    int ctc;      // frames per covariance split (multiple of 16)
    int n16;      // layout il: groups g with g % 16 < n16 are resident
    int nfirst;   // layout first (>= 0): groups g < nfirst of every split are resident; -1: layout il
    int rest_nt;  // streamed groups: 1 nt loads, 0 plain loads
    int contig;   // 1: nt steps row-contiguous through LDS
    int ring;     // pow: 0 the landing-area form, S = 2..4 a ring of S stages per wave
    int rowplain; // ring: 1 plain steps row-contiguous too, 0 lane-addressed
    int cov_ring; // cov: stages of the ring per wave, 2..4 (0: the kernel's four)
    int cov_rowplain; // cov: 1 plain steps row-contiguous too, 0 lane-addressed
};
struct Shape {
    int T, F;
    int tc;       // frames per workgroup (split or chunk)
};

__device__ __forceinline__ bool resident(const Policy& p, int t) {
    const int s = t / p.ctc;
    const int g = (t - s * p.ctc) >> 4;
    return p.nfirst >= 0 ? g < p.nfirst : (g & 15) < p.n16;
}

// byte address of piece j of this lane for the step whose four frames start at t0 (frames past t_end: frame T - 1, as the kernels do)
__device__ __forceinline__ const char* piece(const char* X, const Shape& sh, bool rows, int t0, int t_end, int f0, int lane, int j) {
    const int tq = t0 + (rows ? j : lane >> 4);
    const int t = tq < t_end ? tq : sh.T - 1;
    const size_t row = ((size_t)t * sh.F + f0) * kM8;
    return X + row + (rows ? lane * 16 : (lane & 15) * kM8 + j * 16);
}

// ---- the covariance pass's stream: LDS-DMA ring of S stages per wave (the kernel's: 4), S - 1 steps in flight, counted vmcnt ----
// Policy::cov_rowplain: plain steps row-contiguous like the nt ones (one addressing form, one read form); 0: lane-addressed
template <int S>
__global__ __launch_bounds__(256, 2) void cov_stream(const char* __restrict__ X, float* out, Shape sh, Policy p) {
    __shared__ float4 ring[4 * S * 256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f0 = blockIdx.x * 16;
    const int t_begin = blockIdx.y * sh.tc;
    const int t_end = min(sh.T, t_begin + sh.tc);
    const int nsteps = (t_end - t_begin + 15) >> 4;
    float4* wring = ring + wave * S * 256;
    const unsigned rd_base = (unsigned)(uintptr_t)wring + lane * 16;
    auto plain = [&](int i) { return resident(p, min(t_begin + 16 * i + 4 * wave, sh.T - 1)) || !p.rest_nt; };
    const unsigned rd_rows = (unsigned)(uintptr_t)wring + ((lane >> 4) * 16 + (lane & 15)) * 64;
    auto issue = [&](int i, int s) {
        const int t0 = t_begin + 16 * i + 4 * wave;
        const int tl = i < nsteps ? t0 : sh.T;      // steps past the end re-request the last frame
        if (plain(i)) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds((gvoid_t*)piece(X, sh, p.cov_rowplain, tl, t_end, f0, lane, j), (lvoid_t*)(wring + s * 256 + j * 64), 16, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds((gvoid_t*)piece(X, sh, p.contig, tl, t_end, f0, lane, j), (lvoid_t*)(wring + s * 256 + j * 64), 16, 0, 2);
        }
    };
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto consume = [&](int i, int s) {
        float4 v0, v1, v2, v3;
        if (plain(i) ? p.cov_rowplain : p.contig)
            asm volatile(
                "s_waitcnt vmcnt(%5)\n\t"
                "ds_read_b128 %0, %4\n\t"
                "ds_read_b128 %1, %4 offset:16\n\t"
                "ds_read_b128 %2, %4 offset:32\n\t"
                "ds_read_b128 %3, %4 offset:48\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                : "v"(rd_rows + s * 4096), "n"((S - 1) * 4)
                : "memory");
        else
            asm volatile(
                "s_waitcnt vmcnt(%5)\n\t"
                "ds_read_b128 %0, %4\n\t"
                "ds_read_b128 %1, %4 offset:1024\n\t"
                "ds_read_b128 %2, %4 offset:2048\n\t"
                "ds_read_b128 %3, %4 offset:3072\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                : "v"(rd_base + s * 4096), "n"((S - 1) * 4)
                : "memory");
        acc.x += v0.x + v1.x + v2.x + v3.x;
        acc.y += v0.y + v1.y + v2.y + v3.y;
        acc.z += v0.z + v1.z + v2.z + v3.z;
        acc.w += v0.w + v1.w + v2.w + v3.w;
    };
#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue(u, u);
    int i = 0;
    for (; i + S <= nsteps; i += S) {
#pragma unroll
        for (int u = 0; u < S; ++u) {      // stage indices are compile-time constants in the unrolled body
            issue(i + u + S - 1, (u + S - 1) % S);
            consume(i + u, u);
        }
    }
#pragma unroll
    for (int u = 0; u < S - 1; ++u)
        if (i + u < nsteps) {
            issue(i + u + S - 1, (u + S - 1) % S);
            consume(i + u, u);
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) out[0] = acc.x;
}

// ---- the power pass's stream: register loads, two steps in flight ----
__global__ __launch_bounds__(256) void pow_stream(const char* __restrict__ X, float* out, Shape sh, Policy p) {
    __shared__ f32x4 rows[4 * 2 * 256];      // the landing area of the row-contiguous nt steps
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f0 = (blockIdx.x * 4 + wave) * 16;
    const int t_begin = blockIdx.y * sh.tc;
    const int t_end = min(sh.T, t_begin + sh.tc);
    const int nsteps = (t_end - t_begin + 3) >> 2;
    f32x4* wrows = rows + wave * 2 * 256;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < nsteps; i += 2) {
        f32x4 v[2][4];
        bool plain[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t0 = t_begin + 4 * (i + u);
            plain[u] = resident(p, min(t0, sh.T - 1)) || !p.rest_nt;
            if (plain[u]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][j] = *reinterpret_cast<const f32x4*>(piece(X, sh, false, t0, t_end, f0, lane, j));
            } else if (p.contig) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    __builtin_amdgcn_global_load_lds((gvoid_t*)piece(X, sh, true, t0, t_end, f0, lane, j), (lvoid_t*)(wrows + u * 256 + j * 64), 16, 0, 2);
            } else {
                // (in a branch beside plain loads of the same addresses __builtin_nontemporal_load loses its nt when the two are merged)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(v[u][j]) : "v"(piece(X, sh, false, t0, t_end, f0, lane, j)) : "memory");
            }
        }
        if (p.rest_nt && !p.contig)
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(v[0][0]), "+v"(v[0][1]), "+v"(v[0][2]), "+v"(v[0][3]), "+v"(v[1][0]), "+v"(v[1][1]), "+v"(v[1][2]), "+v"(v[1][3])
                         :
                         : "memory");
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!plain[u] && p.contig) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][j] = wrows[u * 256 + ((lane >> 4) * 16 + (lane & 15)) * 4 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += v[u][j];
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) out[0] = acc.x;
}

// ---- the power pass's stream through a ring: S stages of 4 KB per wave, S - 1 steps in flight, counted vmcnt ----
template <int S>
__global__ __launch_bounds__(256) void pow_ring(const char* __restrict__ X, float* out, Shape sh, Policy p) {
    extern __shared__ __attribute__((aligned(16))) float4 pring[];      // [4 waves][S][256]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f0 = (blockIdx.x * 4 + wave) * 16;
    const int t_begin = blockIdx.y * sh.tc;
    const int t_end = min(sh.T, t_begin + sh.tc);
    const int nsteps = (t_end - t_begin + 3) >> 2;
    float4* wring = pring + wave * S * 256;
    const unsigned rd_base = (unsigned)(uintptr_t)wring + lane * 16;
    const unsigned rd_rows = (unsigned)(uintptr_t)wring + ((lane >> 4) * 16 + (lane & 15)) * 64;
    // walk position n -> step nsteps - 1 - n (descending); positions past the end re-request frame T - 1, never consumed
    auto t0_of = [&](int n) { return t_begin + 4 * (nsteps - 1 - n); };
    auto plain = [&](int n) { return resident(p, min(t0_of(n), sh.T - 1)) || !p.rest_nt; };
    auto issue = [&](int n, int s) {
        const bool past = n >= nsteps;
        const int t0 = past ? sh.T : t0_of(n);
        if (past || !plain(n)) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds((gvoid_t*)piece(X, sh, true, t0, t_end, f0, lane, j), (lvoid_t*)(wring + s * 256 + j * 64), 16, 0, 2);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds((gvoid_t*)piece(X, sh, p.rowplain, t0, t_end, f0, lane, j), (lvoid_t*)(wring + s * 256 + j * 64), 16, 0, 0);
        }
    };
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto consume = [&](int n, int s) {
        float4 v0, v1, v2, v3;
        if (!plain(n) || p.rowplain)
            asm volatile(
                "s_waitcnt vmcnt(%5)\n\t"
                "ds_read_b128 %0, %4\n\t"
                "ds_read_b128 %1, %4 offset:16\n\t"
                "ds_read_b128 %2, %4 offset:32\n\t"
                "ds_read_b128 %3, %4 offset:48\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                : "v"(rd_rows + s * 4096), "n"((S - 1) * 4)
                : "memory");
        else
            asm volatile(
                "s_waitcnt vmcnt(%5)\n\t"
                "ds_read_b128 %0, %4\n\t"
                "ds_read_b128 %1, %4 offset:1024\n\t"
                "ds_read_b128 %2, %4 offset:2048\n\t"
                "ds_read_b128 %3, %4 offset:3072\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                : "v"(rd_base + s * 4096), "n"((S - 1) * 4)
                : "memory");
        acc.x += v0.x + v1.x + v2.x + v3.x;
        acc.y += v0.y + v1.y + v2.y + v3.y;
        acc.z += v0.z + v1.z + v2.z + v3.z;
        acc.w += v0.w + v1.w + v2.w + v3.w;
    };
#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue(u, u);
    int n = 0;
    for (; n + S <= nsteps; n += S) {
#pragma unroll
        for (int u = 0; u < S; ++u) {      // stage indices are compile-time constants in the unrolled body
            issue(n + u + S - 1, (u + S - 1) % S);
            consume(n + u, u);
        }
    }
#pragma unroll
    for (int u = 0; u < S - 1; ++u)
        if (n + u < nsteps) {
            issue(n + u + S - 1, (u + S - 1) % S);
            consume(n + u, u);
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) out[0] = acc.x;
}

// the resident share alone, once, with plain loads: one wave per 1-KB row
__global__ __launch_bounds__(256) void prime(const char* __restrict__ X, float* out, Shape sh, Policy p) {
    const int lane = threadIdx.x & 63;
    const long long nrows = (long long)sh.T * (sh.F / 16);
    const long long nwaves = (long long)gridDim.x * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += nwaves) {
        const int t = (int)(r / (sh.F / 16));
        if (!resident(p, t)) continue;
        acc += *reinterpret_cast<const f32x4*>(X + (size_t)r * 1024 + lane * 16);
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) out[0] = acc.x;
}

// q = "d": every workgroup streams its own contiguous chunk ascending or descending
__global__ __launch_bounds__(256) void dir_stream(const float4* __restrict__ X, float* out, size_t chunk4, int dir) {
    const float4* p = X + (size_t)blockIdx.x * chunk4;
    float4 acc = make_float4(0, 0, 0, 0);
    const size_t n = chunk4 / 256;
    for (size_t i = 0; i < n; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t it = dir ? (n - 1 - (i + u)) : (i + u);
            const float4 v = p[it * 256 + threadIdx.x];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 12345.678f) out[0] = acc.x;
}

struct Bench {
    Shape cov, pow;
    char *X = nullptr, *other = nullptr;
    float* out = nullptr;
    size_t bytes = 0, flush_bytes = 0;      // of X as the rows read it; of the buffer whose memset flushes the cache
    hipEvent_t ev[kPasses + 1];

    double share_mb(const Policy& p) const {
        long long frames = 0;
        for (int t = 0; t < cov.T; ++t) {
            const int g = (t % p.ctc) >> 4;
            frames += p.nfirst >= 0 ? g < p.nfirst : (g & 15) < p.n16;
        }
        return (double)frames * cov.F * kM8 / 1e6;
    }
    void pass(const char* kern, int n, const Policy& p) {
        const bool c = !strcmp(kern, "cov") || (!strcmp(kern, "pair") && (n & 1));      // pair: power, covariance, power, ...
        if (c) {
            const dim3 grid(cov.F / 16, (cov.T + cov.tc - 1) / cov.tc);
            if (p.cov_ring == 2) cov_stream<2><<<grid, 256>>>(X, out, cov, p);
            if (p.cov_ring == 3) cov_stream<3><<<grid, 256>>>(X, out, cov, p);
            if (p.cov_ring == 0 || p.cov_ring == 4) cov_stream<4><<<grid, 256>>>(X, out, cov, p);
        } else if (p.ring == 0)
            pow_stream<<<dim3(pow.F / 64, (pow.T + pow.tc - 1) / pow.tc), 256>>>(X, out, pow, p);
        else {
            const dim3 grid(pow.F / 64, (pow.T + pow.tc - 1) / pow.tc);
            if (p.ring == 2) pow_ring<2><<<grid, 256, 2 * 16384>>>(X, out, pow, p);
            if (p.ring == 3) pow_ring<3><<<grid, 256, 3 * 16384>>>(X, out, pow, p);
            if (p.ring == 4) pow_ring<4><<<grid, 256, 4 * 16384>>>(X, out, pow, p);
        }
    }
    void row(const char* q, const char* kern, Policy p) {
        CHECK(hipMemsetAsync(other, 0x3c, flush_bytes));
        if (share_mb(p) > 0.) prime<<<1024, 256>>>(X, out, cov, p);
        for (int n = 0; n < kPasses; ++n) {
            CHECK(hipEventRecord(ev[n]));
            pass(kern, n, p);
        }
        CHECK(hipEventRecord(ev[kPasses]));
        CHECK(hipEventSynchronize(ev[kPasses]));
        CHECK(hipGetLastError());
        float us[kPasses];
        for (int n = 0; n < kPasses; ++n) {
            CHECK(hipEventElapsedTime(&us[n], ev[n], ev[n + 1]));
            us[n] *= 1e3f;
        }
        float tail[kPasses - 2];
        std::copy(us + 2, us + kPasses, tail);
        std::sort(tail, tail + kPasses - 2);
        const double steady = 0.5 * (tail[(kPasses - 2) / 2 - 1] + tail[(kPasses - 2) / 2]);
        printf("{\"q\": \"%s\", \"kern\": \"%s\", \"layout\": \"%s\", \"rest\": \"%s\", \"addr\": \"%s\", ", q, kern, p.nfirst >= 0 ? "first" : "il",
               p.rest_nt ? "nt" : "plain", p.ring ? "ring" : (p.contig ? "row" : "lane"));
        if (p.ring) printf("\"stages\": %d, \"plain_addr\": \"%s\", ", p.ring, p.rowplain ? "row" : "lane");
        if (!strcmp(q, "e")) printf("\"x_mb\": %.0f, \"tcp\": %d, ", (double)bytes / 1e6, pow.tc);
        if (!strcmp(q, "f"))
            printf("\"x_mb\": %.0f, \"ctc\": %d, \"tcp\": %d, \"cov_stages\": %d, \"cov_plain_addr\": \"%s\", ", (double)bytes / 1e6, cov.tc, pow.tc,
                   p.cov_ring ? p.cov_ring : 4, p.cov_rowplain ? "row" : "lane");
        printf("\"share_mb\": %.1f, \"pass_us\": [", share_mb(p));
        for (int n = 0; n < kPasses; ++n) printf("%s%.1f", n ? ", " : "", us[n]);
        printf("], \"steady_us\": %.1f, \"steady_tbps\": %.2f}\n", steady, (double)bytes / steady / 1e6);
        fflush(stdout);
    }
};

int main() {
    Bench b;
    const int T = 4000, F = 2048;
    b.cov = Shape{T, F, 1008};      // headline geometry: 4 covariance splits, 12 power chunks of 336 frames
    b.pow = Shape{T, F, 336};
    b.bytes = b.flush_bytes = (size_t)T * F * kM8;
    CHECK(hipFuncSetAttribute((const void*)pow_ring<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 16384));
    CHECK(hipMalloc(&b.X, b.bytes));
    CHECK(hipMalloc(&b.other, b.bytes));
    CHECK(hipMalloc(&b.out, 4));
    CHECK(hipMemset(b.X, 0x3c, b.bytes));
    for (auto& e : b.ev) CHECK(hipEventCreate(&e));
    const int ctc = b.cov.tc, groups = ctc / 16;      // 63 groups per split

    const char* kerns[3] = {"cov", "pow", "pair"};
    // (c) the whole buffer, no share: plain, nt lane-strided, nt row-contiguous
    for (int k = 0; k < 3; ++k) {
        b.row("c", kerns[k], Policy{ctc, 0, -1, 0, 0});
        b.row("c", kerns[k], Policy{ctc, 0, -1, 1, 0});
        b.row("c", kerns[k], Policy{ctc, 0, -1, 1, 1});
    }
    // (a) a share of S MB at the head of every split, the rest nt (lane-strided, row-contiguous) or plain
    for (int k = 0; k < 2; ++k)
        for (int S : {0, 64, 128, 160, 192, 224, 240}) {
            const int nfirst = (int)((double)S * 1e6 / (double)b.bytes * groups + 0.5);
            b.row("a", kerns[k], Policy{ctc, 0, nfirst, 1, 0});
            b.row("a", kerns[k], Policy{ctc, 0, nfirst, 1, 1});
            b.row("a", kerns[k], Policy{ctc, 0, nfirst, 0, 0});
        }
    // (b) interleaved against share-first at the shares the rule can give (nt steps row-contiguous), each kernel and the two
    // alternating as in an iteration
    for (int k = 0; k < 3; ++k)
        for (int n16 = 0; n16 <= 8; ++n16) {
            b.row("b", kerns[k], Policy{ctc, n16, -1, 1, 1});
            if (n16 > 0) b.row("b", kerns[k], Policy{ctc, 0, (n16 * groups + 8) / 16, 1, 1});
        }
    // (e) the power pass through a ring of S stages per wave, beside the landing-area rows of the same run
    for (int n16 : {0, 8})
        for (int k = 1; k < 3; ++k) {
            b.row("e", kerns[k], Policy{ctc, n16, -1, 1, 1});
            for (int S = 2; S <= 4; ++S)
                for (int rowplain = 0; rowplain < (n16 ? 2 : 1); ++rowplain) b.row("e", kerns[k], Policy{ctc, n16, -1, 1, 1, S, rowplain});
            b.row("e", kerns[k], Policy{ctc, n16, -1, 1, 1});
        }
    // ... and in 8 chunks of 500 frames: 256 workgroups, one per CU
    b.pow = Shape{T, F, 500};
    for (int k = 1; k < 3; ++k) {
        b.row("e", kerns[k], Policy{ctc, 8, -1, 1, 1});
        for (int S = 2; S <= 4; ++S) b.row("e", kerns[k], Policy{ctc, 8, -1, 1, 1, S, 1});
        b.row("e", kerns[k], Policy{ctc, 8, -1, 1, 1});
    }
    b.pow = Shape{T, F, 336};
    // X of one shard of two and of four, all plain, the chip's 384 workgroups: register loads against the ring
    for (int shards : {2, 4}) {
        b.pow = Shape{T, F / shards, 336 / shards};
        b.cov = Shape{T, F / shards, 1008};
        b.bytes = (size_t)T * (F / shards) * kM8;
        b.row("e", "pow", Policy{ctc, 0, -1, 0, 0});
        for (int S = 2; S <= 4; ++S)
            for (int rowplain = 0; rowplain < 2; ++rowplain) b.row("e", "pow", Policy{ctc, 0, -1, 0, 0, S, rowplain});
        b.row("e", "pow", Policy{ctc, 0, -1, 0, 0});
    }
    b.cov = Shape{T, F, 1008};
    b.bytes = b.flush_bytes;
    // (f) the covariance stream: ring of S stages, plain steps lane-addressed or row-contiguous, alone and alternating with the power
    // stream in its present form (ring of 2 stages, row-contiguous, 8 chunks of 500 frames); the kernel's form (4 stages, lane-
    // addressed plain steps) in front of and behind every block as the yardstick of the same run
    b.pow = Shape{T, F, 500};
    for (int n16 : {0, 8})
        for (int k : {0, 2}) {
            b.row("f", kerns[k], Policy{ctc, n16, -1, 1, 1, 2, 1, 4, 0});
            for (int S = 2; S <= 4; ++S)
                for (int rowplain = 0; rowplain < (n16 ? 2 : 1); ++rowplain) b.row("f", kerns[k], Policy{ctc, n16, -1, 1, 1, 2, 1, S, rowplain});
            b.row("f", kerns[k], Policy{ctc, n16, -1, 1, 1, 2, 1, 4, 0});
        }
    // ... and X of one shard of two and of four, all plain, at the shards' splits (8 of 512 frames, 14 of 288): lane against row
    for (int shards : {2, 4}) {
        b.cov = Shape{T, F / shards, shards == 2 ? 512 : 288};
        b.bytes = (size_t)T * (F / shards) * kM8;
        b.row("f", "cov", Policy{b.cov.tc, 0, -1, 0, 0, 0, 0, 4, 0});
        for (int S = 2; S <= 4; ++S)
            for (int rowplain = 0; rowplain < 2; ++rowplain) b.row("f", "cov", Policy{b.cov.tc, 0, -1, 0, 0, 0, 0, S, rowplain});
        b.row("f", "cov", Policy{b.cov.tc, 0, -1, 0, 0, 0, 0, 4, 0});
    }
    b.pow = Shape{T, F, 336};
    b.cov = Shape{T, F, 1008};
    b.bytes = b.flush_bytes;
    // (d) same direction against alternating direction
    for (size_t mb : {128, 256, 384, 500}) {      // MiB, up to X's size
        const size_t bytes = mb << 20, chunk4 = bytes / 16 / 2048 / 1024 * 1024;
        float us[2];
        for (int mode = 0; mode < 2; ++mode) {
            for (int w = 0; w < 4; ++w) dir_stream<<<2048, 256>>>((const float4*)b.X, b.out, chunk4, mode ? (w & 1) : 0);
            CHECK(hipEventRecord(b.ev[0]));
            for (int r = 0; r < 20; ++r) dir_stream<<<2048, 256>>>((const float4*)b.X, b.out, chunk4, mode ? (r & 1) : 0);
            CHECK(hipEventRecord(b.ev[1]));
            CHECK(hipEventSynchronize(b.ev[1]));
            CHECK(hipEventElapsedTime(&us[mode], b.ev[0], b.ev[1]));
            us[mode] *= 1e3f / 20;
        }
        const double moved = (double)chunk4 * 16 * 2048;
        printf("{\"q\": \"d\", \"mb\": %zu, \"same_direction_us\": %.1f, \"same_direction_tbps\": %.2f, \"alternating_us\": %.1f, \"alternating_tbps\": %.2f}\n", mb,
               us[0], moved / us[0] / 1e6, us[1], moved / us[1] / 1e6);
    }
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(b.X));
    CHECK(hipFree(b.other));
    CHECK(hipFree(b.out));
    return 0;
}
