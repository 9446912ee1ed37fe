// The host layer shared by plan.hip, batch.hip, stft.hip, bstft.hip and exchange.hip: error plumbing, the current-device guard,
// device allocation, graph capture and its cache, W_hat packing, the statistics geometry and the OGIVE per-bin state.  Host code
// only: no kernels, no translation unit of its own (the allocation pool behind dev_malloc / big_alloc lives in plan.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "oiva_internal.h"

// ---- errors: every failure goes through fail_with, which keeps the message oiva_last_error() returns ----------------------
#define OIVA_TRY_HIP(expr)                                                                                              \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return oiva::fail_with(OIVA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)
// (names hipFFT only where it is used: a translation unit that uses it includes <hipfft/hipfft.h> itself)
#define OIVA_TRY_FFT(expr)                                                                                              \
    do {                                                                                                                \
        hipfftResult r_ = (expr);                                                                                       \
        if (r_ != HIPFFT_SUCCESS)                                                                                       \
            return oiva::fail_with(OIVA_ERR_HIP, std::string(#expr) + ": hipfft error " + std::to_string((int)r_));     \
    } while (0)
#define OIVA_NEED(cond, code, msg)                       \
    do {                                                 \
        if (!(cond)) return oiva::fail_with(code, msg);  \
    } while (0)

namespace oiva {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// makes `dev` the calling thread's current device for the life of the guard and puts back what it found: every entry point
// leaves the caller's current device alone
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- device allocation (defined next to the pool in plan.hip) ------------------------------------------------------------
// hipMalloc of the library: before an allocation fails for want of memory the pool's idle buffers go back to the driver and
// the allocation is tried once more
hipError_t dev_malloc(void** out, size_t bytes);
template <class P>
hipError_t dev_malloc(P** out, size_t bytes) {
    return dev_malloc(reinterpret_cast<void**>(out), bytes);
}
// buffers of >= 16 MB come from and go back to the process-wide pool (exact-size reuse, per device)
hipError_t big_alloc(int dev, void** out, size_t bytes);
void big_free(int dev, void* ptr, size_t bytes);

// "allocate these N buffers, the first error wins": every call after a failure does nothing.  With `keep` every pointer is
// also remembered there, for an owner that frees its buffers from one list.
struct AllocChain {
    hipError_t err = hipSuccess;
    std::vector<void*>* keep = nullptr;
    bool ok() const { return err == hipSuccess; }
    template <class P>
    void operator()(P** out, size_t bytes) {
        if (!ok()) return;
        err = dev_malloc(out, bytes);
        if (keep && *out) keep->push_back(*out);
    }
};

// ---- graph capture -----------------------------------------------------------------------------------------------------------
// What `body` launches on `stream` as an executable graph (stream capture records, it does not execute).  The capture is always
// ended; a failing body's status is what comes back, not the capture's.  upload: move the executable graph to the device now --
// otherwise its FIRST launch pays for that, inside whatever the caller is timing (a few percent of a 20-iteration run).
template <class Body>
int capture_graph(hipStream_t stream, Body&& body, hipGraphExec_t* exec, bool upload) {
    hipGraph_t graph = nullptr;
    OIVA_TRY_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipError_t e = hipStreamEndCapture(stream, &graph);
    if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    OIVA_TRY_HIP(e);
    e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    OIVA_TRY_HIP(e);
    if (upload) OIVA_TRY_HIP(hipGraphUpload(*exec, stream));
    return OIVA_OK;
}

// the executable graphs of one handle by an integer key (iterations per replay), least recently used first
struct GraphCache {
    int capacity;
    std::vector<std::pair<int, hipGraphExec_t>> held;
    explicit GraphCache(int cap) : capacity(cap) {}
    bool empty() const { return held.empty(); }
    // the graph of `key`: a hit moves to the back; a miss captures body (uploaded) and, when the cache is full, evicts the front
    // after waiting for the stream (the evicted graph may still be replaying)
    template <class Body>
    int get(hipStream_t stream, int key, Body&& body, hipGraphExec_t* out) {
        for (size_t i = 0; i < held.size(); ++i)
            if (held[i].first == key) {
                std::rotate(held.begin() + (long)i, held.begin() + (long)i + 1, held.end());
                *out = held.back().second;
                return OIVA_OK;
            }
        hipGraphExec_t exec = nullptr;
        const int rc = capture_graph(stream, body, &exec, true);
        if (rc) return rc;
        if ((int)held.size() >= capacity) {
            OIVA_TRY_HIP(hipStreamSynchronize(stream));
            OIVA_TRY_HIP(hipGraphExecDestroy(held.front().second));
            held.erase(held.begin());
        }
        held.emplace_back(key, exec);
        *out = exec;
        return OIVA_OK;
    }
    int clear() {
        while (!held.empty()) {
            hipGraphExec_t g = held.back().second;
            held.pop_back();
            OIVA_TRY_HIP(hipGraphExecDestroy(g));
        }
        return OIVA_OK;
    }
};

// ---- W_hat packing ---------------------------------------------------------------------------------------------------------
// W0 (nbins, M, K) complex64 / complex128 (nullptr: identity) -> W_hat (nbins, M, M) = [W0 | [0; -I]]     (overiva.py:113-123)
inline std::vector<double2> pack_what(const void* W0, int f64, size_t nbins, int M, int K) {
    std::vector<double2> wh(nbins * M * M, make_double2(0., 0.));
    for (size_t f = 0; f < nbins; ++f) {
        double2* m = wh.data() + f * M * M;
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < K; ++k) {
                const size_t i = (f * M + r) * K + k;
                if (!W0) {
                    m[r * M + k] = make_double2(r == k ? 1. : 0., 0.);           // overiva.py:113-114
                } else if (f64) {
                    m[r * M + k] = static_cast<const double2*>(W0)[i];            // overiva.py:116-117
                } else {
                    const float2 v = static_cast<const float2*>(W0)[i];
                    m[r * M + k] = make_double2(v.x, v.y);
                }
            }
        for (int r = K; r < M; ++r) m[r * M + r] = make_double2(-1., 0.);        // overiva.py:122-123
    }
    return wh;
}
// the way back for bins [f0, f0 + n): columns 0..K-1 of W_hat into W_host (all bins, M, K) in complex64 / complex128, or nowhere
// when W_host is nullptr; says whether every element of those columns is finite
inline bool unpack_w(const std::vector<double2>& wh, size_t f0, size_t n, int M, int K, void* W_host, int f64) {
    bool finite = true;
    for (size_t f = f0; f < f0 + n; ++f)
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < K; ++k) {
                const double2 v = wh[(f * M + r) * M + k];
                finite = finite && std::isfinite(v.x) && std::isfinite(v.y);
                const size_t i = (f * M + r) * K + k;
                if (!W_host) continue;
                if (f64)
                    static_cast<double2*>(W_host)[i] = v;
                else
                    static_cast<float2*>(W_host)[i] = make_float2((float)v.x, (float)v.y);
            }
    return finite;
}

// ---- geometry of the projection-back statistics pass, 1..16 channels: 16-bin groups, two sources per pass, at most 16 frame
// splits of >= 128 frames, as many as fill four workgroups per compute unit.  One definition for the plan and for every problem
// of a batch: a batch's Y is overiva()'s, bit for bit.
inline CovGeom stats_geom(int T, int F, int K, int n_cu) {
    CovGeom g{};
    g.nbg = ceil_div(F, kBinsPerWave);
    g.kc = 2;
    const int blocks = g.nbg * ceil_div(K, g.kc);
    int ns = std::max(1, n_cu * 4 / std::max(1, blocks));
    ns = std::min(ns, std::max(1, T / 128));
    ns = std::min(16, ns);
    g.tc = round_up(ceil_div(T, ns), 16);
    g.nsplit = ceil_div(T, g.tc);
    return g;
}

// ---- the per-bin state of OGIVE for nbins bins of M channels (Cx, What and What64 are the owner's own buffers) ---------------
inline void alloc_ogive_state(OgiveState& st, size_t nbins, size_t M, AllocChain& alloc) {
    alloc(&st.CxInv, nbins * M * M * sizeof(double2));
    alloc(&st.CxNorm, nbins * sizeof(double));
    alloc(&st.A, nbins * M * sizeof(double2));
    alloc(&st.Delta, nbins * M * sizeof(double2));
    alloc(&st.Lambda, nbins * sizeof(double));
    alloc(&st.DoA, nbins * sizeof(int));
    alloc(&st.DoW, nbins * sizeof(int));
    alloc(&st.Dnorm, nbins * sizeof(double));
    alloc(&st.ctrl, 4 * sizeof(int));
    alloc(&st.maxdelta, 2 * sizeof(double));
}

}  // namespace oiva
