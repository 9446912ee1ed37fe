// The host layer shared by plan.hip, batch.hip, bsseval.hip, room.hip, stft.hip, bstft.hip and exchange.hip: error plumbing, the
// current-device guard, the owner of a handle's device and pinned memory (DeviceArena) and of its stream and events (HandleStream),
// graph capture and its cache, W_hat packing, the statistics geometry and the OGIVE per-bin state.  Host code only, no kernels.
// What is state -- the last error, the allocators and their process-wide pool of large buffers, the count of live buffers --
// is defined in host_util.hip; nothing else in the library frees device memory, an event or a stream (host_io.hip keeps its
// process-wide pinned ring).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
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

// ---- device allocation (host_util.hip) -------------------------------------------------------------------------------------
// hipMalloc of the library: before an allocation fails for want of memory the pool's idle buffers go back to the driver and
// the allocation is tried once more.  fine_malloc: fine-grained device memory (system-scope atomics, IPC exchange buffers).
// Every free takes the byte count of its allocation: the library counts what it has handed out (oiva_test_live_buffers).
hipError_t dev_malloc(void** out, size_t bytes);
hipError_t fine_malloc(void** out, size_t bytes);
void dev_free(void* ptr, size_t bytes);
hipError_t pinned_malloc(void** out, size_t bytes);
void pinned_free(void* ptr, size_t bytes);
// buffers of >= 16 MB come from and go back to the process-wide pool (exact-size reuse, per device)
hipError_t big_alloc(int dev, void** out, size_t bytes);
void big_free(int dev, void* ptr, size_t bytes);

enum class Mem { plain, pooled, pinned, fine };      // dev_malloc | big_alloc | pinned_malloc | fine_malloc

// The one owner of a handle's device and pinned memory (or, on the stack, of a call's temporaries: ScopedDev).  The handle keeps
// raw pointers; the arena remembers each buffer with its size and kind and gives all of them back in clear(), newest first.
// take() chains as "allocate these N buffers, the first error wins": after a failure every take does nothing until status()
// has handed the error over.  The pointer a buffer is taken into lives at least as long as the arena holds the buffer.
class DeviceArena {
public:
    explicit DeviceArena(int device = 0) : device(device) {}
    ~DeviceArena() { clear(); }
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;

    int device;                       // of the pooled kind
    bool ok() const { return err == hipSuccess; }
    // a step between the takes of a chain (a memset, a copy, opening the stream) joins it: the first error wins
    void note(hipError_t e) { err = ok() ? e : err; }
    // the chain's error, which it hands over: the next chain starts clean
    hipError_t status() { return std::exchange(err, hipSuccess); }

    template <class P>
    void take(P** out, size_t bytes, Mem kind = Mem::plain) {
        if (!ok()) return;
        void* v = nullptr;
        switch (kind) {
            case Mem::plain: err = dev_malloc(&v, bytes); break;
            case Mem::pooled: err = big_alloc(device, &v, bytes); break;
            case Mem::pinned: err = pinned_malloc(&v, bytes); break;
            case Mem::fine: err = fine_malloc(&v, bytes); break;
        }
        if (!ok()) return;
        held.push_back({v, bytes, kind, out});
        *out = static_cast<P*>(v);
    }
    // ... and filled from `bytes` of host memory (synchronous)
    template <class P>
    void take_filled(P** out, const void* host, size_t bytes) {
        take(out, bytes);
        if (ok()) err = hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice);
    }
    // one buffer outside a chain: its status at once
    template <class P>
    hipError_t take_one(P** out, size_t bytes, Mem kind = Mem::plain) {
        take(out, bytes, kind);
        return status();
    }
    size_t mark() const { return held.size(); }
    // frees what was taken after mark(), newest first; a pointer that still holds such a buffer is nulled
    void release_to(size_t mark) {
        while (held.size() > mark) {
            const Held h = held.back();
            held.pop_back();
            void* now = nullptr;      // (the slot is a P* of some P: read and nulled as bytes, not through a void* lvalue)
            std::memcpy(&now, h.slot, sizeof now);
            if (now == h.p) std::memset(h.slot, 0, sizeof now);
            give_back(h);
        }
    }
    // frees the buffer *ptr now and nulls the pointer; a pointer that is null or holds nothing of this arena is left alone
    template <class P>
    void release(P** ptr) {
        for (size_t i = held.size(); i-- > 0;)
            if (held[i].p == static_cast<const void*>(*ptr)) {
                give_back(held[i]);
                held.erase(held.begin() + (long)i);
                *ptr = nullptr;
                return;
            }
    }
    void clear() { release_to(0); }

private:
    hipError_t err = hipSuccess;
    struct Held {
        void* p;
        size_t bytes;
        Mem kind;
        void* slot;       // the owner's pointer it was taken into (the owner may have swapped it with another since)
    };
    std::vector<Held> held;
    void give_back(const Held& h) {
        switch (h.kind) {
            case Mem::pooled: big_free(device, h.p, h.bytes); break;
            case Mem::pinned: pinned_free(h.p, h.bytes); break;
            default: dev_free(h.p, h.bytes);
        }
    }
};
using ScopedDev = DeviceArena;      // on the stack: a call's staging and scratch buffers, gone on every way out

// A handle's stream -- the caller's, borrowed, or a non-blocking one of its own -- and its events.  Converts to hipStream_t, so
// launch code passes it as the stream.
struct HandleStream {
    hipStream_t stream = nullptr;
    bool own = false;
    std::vector<hipEvent_t> events;
    operator hipStream_t() const { return stream; }
    HandleStream() = default;
    ~HandleStream() { close(); }
    HandleStream(const HandleStream&) = delete;
    HandleStream& operator=(const HandleStream&) = delete;

    hipError_t open(void* user_stream, int n_events, bool timing = true) {
        if (user_stream) {
            stream = static_cast<hipStream_t>(user_stream);
        } else {
            const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
            own = true;
        }
        return add_events(n_events, timing);
    }
    hipError_t add_events(int n, bool timing = true) {
        for (int i = 0; i < n; ++i) {
            hipEvent_t ev = nullptr;
            const hipError_t e = timing ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
            events.push_back(ev);
        }
        return hipSuccess;
    }
    void close() {
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
        events.clear();
        if (own && stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        own = false;
    }
    // record event i, run body (an int status), record event j, wait for it: *ms is the time between the two
    template <class Body>
    int elapsed_ms(int i, int j, Body&& body, float* ms) {
        OIVA_TRY_HIP(hipEventRecord(events[i], stream));
        const int rc = body();
        if (rc) return rc;
        OIVA_TRY_HIP(hipEventRecord(events[j], stream));
        OIVA_TRY_HIP(hipEventSynchronize(events[j]));
        OIVA_TRY_HIP(hipEventElapsedTime(ms, events[i], events[j]));
        return OIVA_OK;
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
inline void alloc_ogive_state(OgiveState& st, size_t nbins, size_t M, DeviceArena& mem) {
    mem.take(&st.CxInv, nbins * M * M * sizeof(double2));
    mem.take(&st.CxNorm, nbins * sizeof(double));
    mem.take(&st.A, nbins * M * sizeof(double2));
    mem.take(&st.Delta, nbins * M * sizeof(double2));
    mem.take(&st.Lambda, nbins * sizeof(double));
    mem.take(&st.DoA, nbins * sizeof(int));
    mem.take(&st.DoW, nbins * sizeof(int));
    mem.take(&st.Dnorm, nbins * sizeof(double));
    mem.take(&st.ctrl, 4 * sizeof(int));
    mem.take(&st.maxdelta, 2 * sizeof(double));
}

}  // namespace oiva
