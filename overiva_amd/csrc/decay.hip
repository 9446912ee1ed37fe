// C ABI of the decay measurement (oiva_decay_*, include/overiva_hip.h): Schroeder integral, threshold crossings and the masked sums
// of the least-squares fit for a packed batch of impulse responses, in float64.  Host code only; the kernel lives in
// kernels_decay.hip and the algorithm is DESIGN.md 3.14.
//
//   create            : n_resp responses of lengths[i] samples, packed one after the other
//   set_host, set_dev : the samples from the host (into the handle's own buffer), or where they lie on the device (borrowed)
//   set_room          : the room handle's own responses where they lie (room.hip calls decay_bind)
//   run               : one launch: E[0], i_a, i_b, sum D, sum n D of every response; with keep_curve every E[n] as well
//   get, get_curve    : the results of the last run on the host
// The two threshold factors are formed here, once, in double: the kernel multiplies E[0] by them.  Every call is synchronous.
#include <cmath>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

struct oiva_decay {
    int device = 0;
    long long total = 0;
    bool ran = false, kept = false;
    HandleStream stream;               // two events: the bracket of the last run's kernel
    DeviceArena mem;
    std::vector<DecayRec> recs;
    DecayRec* recs_dev = nullptr;
    const double* in = nullptr;        // the handle's own buffer or the caller's
    double *own = nullptr, *curve = nullptr, *e0 = nullptr, *sums = nullptr;
    int* idx = nullptr;
};

int oiva::decay_bind(oiva_decay* p, int device, const double* dev, const int* lengths, int n_resp) {
    OIVA_NEED(p && dev && lengths, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(device == p->device, OIVA_ERR_ARG, "the responses lie on device " + std::to_string(device) + ", the decay handle on " +
                                                      std::to_string(p->device));
    OIVA_NEED(n_resp == (int)p->recs.size(), OIVA_ERR_ARG, "the decay handle holds " + std::to_string(p->recs.size()) +
                                                               " responses, the room " + std::to_string(n_resp));
    for (int i = 0; i < n_resp; ++i)
        OIVA_NEED(lengths[i] == p->recs[i].len, OIVA_ERR_ARG, "response " + std::to_string(i) + " has " + std::to_string(lengths[i]) +
                                                                  " samples, the decay handle's table " + std::to_string(p->recs[i].len));
    p->in = dev;
    p->ran = p->kept = false;
    return OIVA_OK;
}

extern "C" {

oiva_status oiva_decay_create(oiva_decay** out, int device, int n_resp, const int* lengths, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(lengths != nullptr, OIVA_ERR_ARG, "null lengths");
    OIVA_NEED(n_resp >= 1 && n_resp <= kDecayMaxResp, OIVA_ERR_ARG, "n_resp must be in 1..2^22");
    std::vector<DecayRec> recs(n_resp);
    long long total = 0;
    for (int i = 0; i < n_resp; ++i) {
        OIVA_NEED(lengths[i] >= 1 && lengths[i] <= kDecayMaxLen, OIVA_ERR_ARG,
                  "response " + std::to_string(i) + " must hold 1..2^24 samples, got " + std::to_string(lengths[i]));
        recs[i] = DecayRec{total, lengths[i], 0};
        total += lengths[i];
    }
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_decay* p = new oiva_decay();
    p->device = p->mem.device = device;
    p->total = total;
    p->recs = recs;
    DeviceArena& mem = p->mem;
    mem.note(p->stream.open(stream, 2));
    mem.take_filled(&p->recs_dev, recs.data(), (size_t)n_resp * sizeof(DecayRec));
    mem.take(&p->e0, (size_t)n_resp * sizeof(double));
    mem.take(&p->sums, (size_t)n_resp * 2 * sizeof(double));
    mem.take(&p->idx, (size_t)n_resp * 2 * sizeof(int));
    if (!mem.ok()) {
        const hipError_t e = mem.status();
        oiva_decay_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_decay_destroy(oiva_decay* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_decay_set_host(oiva_decay* p, const double* host_packed) {
    OIVA_NEED(p && host_packed, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    p->ran = p->kept = false;
    p->in = nullptr;
    if (!p->own) {
        const hipError_t e = p->mem.take_one(&p->own, (size_t)p->total * sizeof(double), Mem::pooled);
        if (e != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("allocation of the responses failed: ") + hipGetErrorString(e));
    }
    OIVA_TRY_HIP(hipMemcpyAsync(p->own, host_packed, (size_t)p->total * sizeof(double), hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->in = p->own;
    return OIVA_OK;
}

oiva_status oiva_decay_set_dev(oiva_decay* p, const void* dev_packed) {
    OIVA_NEED(p && dev_packed, OIVA_ERR_ARG, "null argument");
    OIVA_NEED((reinterpret_cast<unsigned long long>(dev_packed) & 7ull) == 0, OIVA_ERR_ARG, "the responses must be 8-byte aligned");
    p->ran = p->kept = false;
    p->in = static_cast<const double*>(dev_packed);
    return OIVA_OK;
}

oiva_status oiva_decay_run(oiva_decay* p, double fs, double start_db, double decay_db, int keep_curve) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(std::isfinite(fs) && fs > 0., OIVA_ERR_ARG, "fs must be finite and > 0");
    OIVA_NEED(std::isfinite(start_db) && start_db >= 0., OIVA_ERR_ARG, "start_db must be finite and >= 0");
    OIVA_NEED(std::isfinite(decay_db) && decay_db > 0., OIVA_ERR_ARG, "decay_db must be finite and > 0");
    OIVA_NEED(p->in != nullptr, OIVA_ERR_STATE, "no responses set");
    const double fa = std::pow(10., -start_db / 10.), fb = std::pow(10., -(start_db + decay_db) / 10.);
    DeviceGuard guard(p->device);
    p->ran = p->kept = false;
    if (keep_curve && !p->curve) {
        const hipError_t e = p->mem.take_one(&p->curve, (size_t)p->total * sizeof(double), Mem::pooled);
        if (e != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("allocation of the curves failed: ") + hipGetErrorString(e));
    }
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[0], p->stream));
    OIVA_TRY_HIP(launch_decay(p->stream, p->recs_dev, (int)p->recs.size(), p->in, fa, fb, keep_curve ? p->curve : nullptr, p->e0, p->idx,
                              p->sums));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[1], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->ran = true;
    p->kept = keep_curve != 0;
    return OIVA_OK;
}

oiva_status oiva_decay_get(oiva_decay* p, double* e0, int* i_a, int* i_b, double* sum_d, double* sum_nd) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->ran, OIVA_ERR_STATE, "run has not run");
    DeviceGuard guard(p->device);
    const size_t n = p->recs.size();
    if (e0) OIVA_TRY_HIP(hipMemcpy(e0, p->e0, n * sizeof(double), hipMemcpyDeviceToHost));
    if (i_a || i_b) {
        std::vector<int> idx(2 * n);
        OIVA_TRY_HIP(hipMemcpy(idx.data(), p->idx, 2 * n * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (i_a) i_a[i] = idx[2 * i];
            if (i_b) i_b[i] = idx[2 * i + 1];
        }
    }
    if (sum_d || sum_nd) {
        std::vector<double> sums(2 * n);
        OIVA_TRY_HIP(hipMemcpy(sums.data(), p->sums, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (sum_d) sum_d[i] = sums[2 * i];
            if (sum_nd) sum_nd[i] = sums[2 * i + 1];
        }
    }
    return OIVA_OK;
}

oiva_status oiva_decay_get_curve(oiva_decay* p, double* curve_host_packed) {
    OIVA_NEED(p && curve_host_packed, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->ran && p->kept, OIVA_ERR_STATE, "the last run did not keep the curves");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpy(curve_host_packed, p->curve, (size_t)p->total * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_decay_ms(oiva_decay* p, float* ms) {
    OIVA_NEED(p && ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->ran, OIVA_ERR_STATE, "run has not run");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipEventElapsedTime(ms, p->stream.events[0], p->stream.events[1]));
    return OIVA_OK;
}

}  // extern "C"
