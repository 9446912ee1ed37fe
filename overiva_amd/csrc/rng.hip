// C ABI of the device random generator (oiva_rng_*, include/overiva_hip.h): seeded standard normals in float64, drawn where they
// are used.  Host code only; the kernels live in kernels_rng.hip and the stream's definition is DESIGN.md 3.13.
//
//   create   : n streams of counts[i] elements each, packed one after the other (sum counts[i] float64 on the device)
//   fill     : every stream under its key (key0[i], key1[i]) and one purpose
//   get, ptr : the packed values on the host; where they lie on the device (the filler_dev of oiva_sweep_evaluate)
//   raw      : test hook: the raw Philox words of some blocks of one stream
//   room_mix : oiva_room_mix with the group's noise drawn into the room handle's own buffer (the body is room.hip's)
// A value is a function of (key, purpose, index in the stream) alone: not of the other streams, of the stream's place in the
// handle or of the launch.  Every call is synchronous.
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

struct oiva_rng {
    int device = 0;
    long long total = 0, longest = 0;
    bool filled = false;
    HandleStream stream;
    DeviceArena mem;
    std::vector<RngStream> streams;
    RngStream* streams_dev = nullptr;
    double* out = nullptr;
};

extern "C" {

oiva_status oiva_rng_create(oiva_rng** out, int device, int n_streams, const long long* counts, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(counts != nullptr, OIVA_ERR_ARG, "null counts");
    OIVA_NEED(n_streams >= 1 && n_streams <= kRngMaxStreams, OIVA_ERR_ARG, "n_streams must be in 1..65535");
    std::vector<RngStream> streams(n_streams);
    long long total = 0, longest = 0;
    for (int i = 0; i < n_streams; ++i) {
        OIVA_NEED(counts[i] >= 1 && counts[i] <= kRngMaxCount, OIVA_ERR_ARG,
                  "stream " + std::to_string(i) + " must hold 1..2^40 elements, got " + std::to_string(counts[i]));
        streams[i] = RngStream{0ull, 0ull, total, counts[i]};
        total += counts[i];
        longest = std::max(longest, counts[i]);
        OIVA_NEED(total <= kRngMaxCount, OIVA_ERR_ARG, "the streams hold more than 2^40 elements");
    }
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_rng* p = new oiva_rng();
    p->device = p->mem.device = device;
    p->total = total, p->longest = longest;
    p->streams = streams;
    DeviceArena& mem = p->mem;
    mem.note(p->stream.open(stream, 2));
    mem.take(&p->streams_dev, (size_t)n_streams * sizeof(RngStream));
    mem.take(&p->out, (size_t)total * sizeof(double), Mem::pooled);
    if (!mem.ok()) {
        const hipError_t e = mem.status();
        oiva_rng_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_rng_destroy(oiva_rng* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_rng_fill(oiva_rng* p, const unsigned long long* key0, const unsigned long long* key1, unsigned long long purpose) {
    OIVA_NEED(p && key0 && key1, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    p->filled = false;
    for (size_t i = 0; i < p->streams.size(); ++i) p->streams[i].k0 = key0[i], p->streams[i].k1 = key1[i];
    OIVA_TRY_HIP(hipMemcpyAsync(p->streams_dev, p->streams.data(), p->streams.size() * sizeof(RngStream), hipMemcpyHostToDevice,
                                p->stream));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[0], p->stream));
    OIVA_TRY_HIP(launch_rng_normal(p->stream, p->streams_dev, (int)p->streams.size(), p->longest, purpose, p->out));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[1], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->filled = true;
    return OIVA_OK;
}

oiva_status oiva_rng_fill_ms(oiva_rng* p, float* ms) {
    OIVA_NEED(p && ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->filled, OIVA_ERR_STATE, "fill has not run");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipEventElapsedTime(ms, p->stream.events[0], p->stream.events[1]));
    return OIVA_OK;
}

oiva_status oiva_rng_get(oiva_rng* p, double* host_packed) {
    OIVA_NEED(p && host_packed, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->filled, OIVA_ERR_STATE, "fill has not run");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpy(host_packed, p->out, (size_t)p->total * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_rng_ptr(oiva_rng* p, void** dev_packed) {
    OIVA_NEED(p && dev_packed, OIVA_ERR_ARG, "null argument");
    *dev_packed = nullptr;
    OIVA_NEED(p->filled, OIVA_ERR_STATE, "fill has not run");
    *dev_packed = p->out;
    return OIVA_OK;
}

oiva_status oiva_rng_raw(int device, unsigned long long key0, unsigned long long key1, unsigned long long purpose,
                         unsigned long long first_block, int n_blocks, unsigned long long* words_host) {
    OIVA_NEED(words_host != nullptr, OIVA_ERR_ARG, "null words");
    OIVA_NEED(n_blocks >= 1 && n_blocks <= kRngMaxRaw, OIVA_ERR_ARG, "n_blocks must be in 1..2^20");
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    ScopedDev tmp(device);
    unsigned long long* words = nullptr;
    const size_t bytes = (size_t)n_blocks * 4 * sizeof(unsigned long long);
    OIVA_TRY_HIP(tmp.take_one(&words, bytes));
    OIVA_TRY_HIP(launch_rng_raw(nullptr, key0, key1, purpose, first_block, n_blocks, words));
    OIVA_TRY_HIP(hipMemcpy(words_host, words, bytes, hipMemcpyDeviceToHost));      // (the null stream: the copy waits for the kernel)
    return OIVA_OK;
}

oiva_status oiva_rng_room_mix(oiva_room* room, int g0, int K, double sinr, double snr, int ref_mic, const double* sources_var,
                              const unsigned long long* key0, const unsigned long long* key1) {
    OIVA_NEED(room && key0 && key1, OIVA_ERR_ARG, "null argument");
    return room_mix_body(room, g0, K, sinr, snr, ref_mic, sources_var, nullptr, key0, key1);
}

}  // extern "C"
