// The part of the host layer (host_util.h) that is state: the thread's last error, the covariance kernel's armed timer, and every
// allocation of the library -- hipMalloc with one retry, the process-wide pool of large buffers, pinned host words -- with the
// count of what is handed out.  Host code only.  Outside this file only host_io.hip (its pinned ring) frees to the driver.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "host_util.h"

using namespace oiva;

namespace {

thread_local std::string g_err;

// buffers handed out and not yet given back (a pooled buffer resting in the pool counts as given back)
std::atomic<long long> g_live_count{0}, g_live_bytes{0};
hipError_t handed_out(hipError_t e, size_t bytes, int n = 1) {
    if (e == hipSuccess) {
        g_live_count += n;
        g_live_bytes += n * (long long)bytes;
    }
    return e;
}
void given_back(size_t bytes) { (void)handed_out(hipSuccess, bytes, -1); }

// ---- large device buffers (X, Y, staging) come from a process-wide pool -------------------------------------------
// The drop-in call creates and destroys a plan per call; hipMalloc + hipFree of the 524 MB of X and the 131 MB of Y at the
// headline shape were ~2.5 ms of a 22 ms call.  Buffers of >= 16 MB go back to the pool instead of the driver (exact-size
// reuse, per device), at most $OIVA_POOL_MB (default 2048) held; oiva_pool_trim() releases them.
struct BigPool {
    struct Entry {
        void* p;
        size_t bytes;
        int dev;
    };
    std::mutex m;
    std::vector<Entry> held;      // oldest first
    size_t total = 0;
};
BigPool& big_pool() {
    static BigPool* bp = new BigPool;      // (never destroyed: the HIP runtime may be gone when static destructors run)
    return *bp;
}
constexpr size_t kPoolMinBytes = (size_t)16 << 20;
size_t pool_cap_bytes() {
    static const size_t cap = [] {
        const char* v = std::getenv("OIVA_POOL_MB");
        return (size_t)(v ? std::max(0, std::atoi(v)) : 2048) << 20;
    }();
    return cap;
}
// every buffer the pool holds goes back to the driver (oiva_pool_trim; hipMalloc when the driver is out of memory)
void pool_release_all() {
    BigPool& bp = big_pool();
    std::lock_guard<std::mutex> g(bp.m);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto& e : bp.held) {
        (void)hipSetDevice(e.dev);
        (void)hipFree(e.p);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    bp.held.clear();
    bp.total = 0;
}
// hipMalloc of the library: the pool's idle buffers are memory the caller thinks is free, so before an allocation fails for
// want of memory they are handed back and the allocation is tried once more
hipError_t malloc_retry(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipErrorOutOfMemory) return e;
    (void)hipGetLastError();
    pool_release_all();
    return hipMalloc(out, bytes);
}

}  // namespace

int oiva::fail_with(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
oiva::KernelTimer& oiva::kernel_timer() {
    static thread_local KernelTimer t;
    return t;
}

// the switches of the per-bin update's choice (choose_update, kernel_choice.h; INTEGRATION.md "switches"), read once per process
const oiva::UpdSwitches& oiva::update_switches() {
    static const UpdSwitches sw = [] {
        UpdSwitches u;
        auto is = [](const char* name, char c) { const char* v = std::getenv(name); return v && v[0] == c; };
        if (const char* v = std::getenv("OIVA_UPDATE_GRAM")) u.gram = std::atoi(v);
        u.det = !is("OIVA_UPDATE_DET", '0');
        u.det16_inverse = is("OIVA_DET16_INVERSE", '1');
        u.det16_rows = !is("OIVA_DET16_ROWS", '0');
        return u;
    }();
    return sw;
}

hipError_t oiva::dev_malloc(void** out, size_t bytes) { return handed_out(malloc_retry(out, bytes), bytes); }
hipError_t oiva::fine_malloc(void** out, size_t bytes) {
    return handed_out(hipExtMallocWithFlags(out, bytes, hipDeviceMallocFinegrained), bytes);
}
void oiva::dev_free(void* ptr, size_t bytes) {
    if (!ptr) return;
    given_back(bytes);
    (void)hipFree(ptr);
}
hipError_t oiva::pinned_malloc(void** out, size_t bytes) { return handed_out(hipHostMalloc(out, bytes, hipHostMallocDefault), bytes); }
void oiva::pinned_free(void* ptr, size_t bytes) {
    if (!ptr) return;
    given_back(bytes);
    (void)hipHostFree(ptr);
}
hipError_t oiva::big_alloc(int dev, void** out, size_t bytes) {
    if (bytes >= kPoolMinBytes) {
        BigPool& bp = big_pool();
        std::lock_guard<std::mutex> g(bp.m);
        for (size_t i = bp.held.size(); i-- > 0;)
            if (bp.held[i].dev == dev && bp.held[i].bytes == bytes) {
                *out = bp.held[i].p;
                bp.total -= bytes;
                bp.held.erase(bp.held.begin() + (long)i);
                return handed_out(hipSuccess, bytes);
            }
    }
    return handed_out(malloc_retry(out, bytes), bytes);
}
void oiva::big_free(int dev, void* ptr, size_t bytes) {
    if (!ptr) return;
    given_back(bytes);
    if (bytes >= kPoolMinBytes && bytes <= pool_cap_bytes()) {
        BigPool& bp = big_pool();
        std::lock_guard<std::mutex> g(bp.m);
        while (!bp.held.empty() && bp.total + bytes > pool_cap_bytes()) {
            (void)hipFree(bp.held.front().p);
            bp.total -= bp.held.front().bytes;
            bp.held.erase(bp.held.begin());
        }
        bp.held.push_back({ptr, bytes, dev});
        bp.total += bytes;
        return;
    }
    (void)hipFree(ptr);
}

extern "C" {

const char* oiva_last_error(void) { return g_err.c_str(); }

int oiva_pool_trim(void) {
    pool_release_all();
    return OIVA_OK;
}

int oiva_test_live_buffers(long long* count, long long* bytes) {
    OIVA_NEED(count && bytes, OIVA_ERR_ARG, "null argument");
    *count = g_live_count.load();
    *bytes = g_live_bytes.load();
    return OIVA_OK;
}

}  // extern "C"
