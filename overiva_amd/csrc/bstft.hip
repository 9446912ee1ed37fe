// C ABI of the batched STFT (oiva_bstft_*, include/overiva_hip.h): analysis and synthesis of B rooms of different lengths in one
// set of launches, X produced in (and Y consumed from) the layout of the batched solvers on the device.  Host code only; the
// kernels live in kernels_bstft.hip.  The transform is hipFFT: one batched R2C / C2R plan over all frames of all rooms and
// channels.  Framing convention and per-element arithmetic are stft.hip's (one room per handle).
//
//   analysis : packed x (sum n_b, M) float32, host  ->  X (sum T_b, F, M) complex64, device     T_b = n_b / hop, F = frame/2 + 1
//              upload | framing + window | R2C | (frame * M + c, F) -> (frame, F, M)
//   synthesis: Y (sum T_b, F, K) complex64, device  ->  packed y (sum T_b * hop, K) float32, host
//              (frame, F, K) -> (frame * K + c, F) | C2R | overlap-add per room | download
// oiva_bstft_analysis_dev starts from audio already on the device (a copy, or a cast from float64, in place of the upload) and
// oiva_bstft_synthesis_keep ends before the download: the handle's packed audio stays where it is (the sweep, sweep.hip).
// Every call is synchronous; events around every phase are kept for oiva_bstft_phase_ms.
#include <hipfft/hipfft.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {

constexpr int kMaxChannels = 8;        // as the batched solvers
constexpr int kPhases = 8;             // upload, framing, R2C, to (t, F, M) | from (t, F, K), C2R, overlap-add, download

}  // namespace

struct oiva_bstft {
    int device = 0;
    int B = 0, M = 0, L = 0, hop = 0, F = 0;
    long long samples_total = 0, frames_total = 0;
    HandleStream stream;      // events of the analysis: [0..4], of the synthesis: [5..9]
    DeviceArena mem;
    std::vector<BstftRoom> rooms;
    BstftRoom* rooms_dev = nullptr;
    hipfftHandle fwd = 0, inv = 0;
    bool have_fwd = false, have_inv = false;
    int inv_chan = -1;        // channel count the inverse plan was made for
    float* win_a = nullptr;   // (L) or nullptr
    float* win_s = nullptr;
    float* x = nullptr;       // packed (samples_total, M) in | (frames_total * hop, K) out
    float* frames = nullptr;  // (frames_total * M, L)
    float2* spec = nullptr;   // (frames_total * M, F)
    float2* X = nullptr;      // (frames_total, F, M)
    bool timed_a = false, timed_s = false;
    bool kept_s = false;      // the last synthesis left its audio on the device: its download phase reads 0
};

namespace {

// the analysis behind whatever fills the handle's packed audio x (`fill`: an upload, a device copy or a cast, on the stream)
template <class Fill>
int analysis_from(oiva_bstft* p, void** X_dev, Fill&& fill) {
    const int M = p->M, L = p->L, F = p->F;
    if (!p->have_fwd) {
        int n[1] = {L};
        OIVA_TRY_FFT(hipfftPlanMany(&p->fwd, 1, n, nullptr, 1, L, nullptr, 1, F, HIPFFT_R2C, (int)(p->frames_total * M)));
        OIVA_TRY_FFT(hipfftSetStream(p->fwd, p->stream));
        p->have_fwd = true;
    }
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[0], p->stream));
    OIVA_TRY_HIP(fill());
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[1], p->stream));
    OIVA_TRY_HIP(launch_bstft_frame(p->stream, p->x, p->win_a, p->frames, p->rooms_dev, p->B, p->frames_total, M, L, p->hop));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[2], p->stream));
    OIVA_TRY_FFT(hipfftExecR2C(p->fwd, p->frames, reinterpret_cast<hipfftComplex*>(p->spec)));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[3], p->stream));
    OIVA_TRY_HIP(launch_bstft_to_tfc(p->stream, p->spec, p->X, p->frames_total, F, M));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[4], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->timed_a = true;
    *X_dev = p->X;
    return OIVA_OK;
}

// the synthesis up to the packed (frames_total * hop, K) audio in the handle's x; events 5..8 recorded, nothing waited for
int synthesis_to_x(oiva_bstft* p, const void* Y_dev, int K) {
    const int L = p->L, F = p->F;
    // one inverse plan per channel count (the solver returns fewer channels than the analysis had)
    if (!p->have_inv || p->inv_chan != K) {
        if (p->have_inv) OIVA_TRY_FFT(hipfftDestroy(p->inv));
        p->have_inv = false;
        int n[1] = {L};
        OIVA_TRY_FFT(hipfftPlanMany(&p->inv, 1, n, nullptr, 1, F, nullptr, 1, L, HIPFFT_C2R, (int)(p->frames_total * K)));
        OIVA_TRY_FFT(hipfftSetStream(p->inv, p->stream));
        p->have_inv = true;
        p->inv_chan = K;
    }
    const long long n_out = p->frames_total * p->hop;
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[5], p->stream));
    OIVA_TRY_HIP(launch_bstft_from_tfc(p->stream, static_cast<const float2*>(Y_dev), p->spec, p->frames_total, F, K));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[6], p->stream));
    OIVA_TRY_FFT(hipfftExecC2R(p->inv, reinterpret_cast<hipfftComplex*>(p->spec), p->frames));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[7], p->stream));
    OIVA_TRY_HIP(launch_bstft_overlap_add(p->stream, p->frames, p->win_s, p->x, p->rooms_dev, p->B, n_out, K, L, p->hop));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[8], p->stream));
    return OIVA_OK;
}

}  // namespace

void oiva::bstft_dims(oiva_bstft* p, int* device, int* B, int* M, int* frame, int* hop, long long* samples_total) {
    *device = p->device, *B = p->B, *M = p->M, *frame = p->L, *hop = p->hop, *samples_total = p->samples_total;
}

extern "C" {

oiva_status oiva_bstft_create(oiva_bstft** out, int device, int B, const int* n_samples, int M, int frame, int hop, const float* win_a,
                              const float* win_s, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(n_samples != nullptr, OIVA_ERR_ARG, "null n_samples");
    OIVA_NEED(B >= 1, OIVA_ERR_ARG, "B must be >= 1");
    OIVA_NEED(M >= 1 && M <= kMaxChannels, OIVA_ERR_ARG, "the batched path runs on 1..8 channels");
    OIVA_NEED(frame >= 2 && frame % 2 == 0, OIVA_ERR_ARG, "frame must be even and >= 2");
    OIVA_NEED(hop >= 1 && hop <= frame, OIVA_ERR_ARG, "hop must be in 1..frame");
    const int F = frame / 2 + 1;
    const double lim31 = 2147483648., lim63 = 9223372036854775808.;
    double samples = 0., frames = 0.;
    for (int b = 0; b < B; ++b) {
        OIVA_NEED(n_samples[b] >= hop, OIVA_ERR_ARG, "room " + std::to_string(b) + " is shorter than one hop");
        const double Tb = n_samples[b] / hop;
        OIVA_NEED((double)n_samples[b] * M < lim31 && Tb * M * (frame + 2) < lim31, OIVA_ERR_ARG,
                  "room " + std::to_string(b) + " is too large (2^31 elements per room)");
        samples += n_samples[b];
        frames += Tb;
    }
    // the largest buffer is X / spec: frames * M * F complex64; hipFFT counts its transforms in an int
    OIVA_NEED(frames * M * F * 8. < lim63 && samples * M * 4. < lim63 && frames * M < lim31 && frames < lim31, OIVA_ERR_ARG,
              "batch too large");
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_bstft* p = new oiva_bstft();
    p->device = device;
    p->B = B, p->M = M, p->L = frame, p->hop = hop, p->F = F;
    p->rooms.resize(B);
    for (int b = 0; b < B; ++b) {
        BstftRoom& r = p->rooms[b];
        r.s_off = p->samples_total;
        r.t_off = p->frames_total;
        r.n = n_samples[b];
        r.T = n_samples[b] / hop;
        p->samples_total += r.n;
        p->frames_total += r.T;
    }
    DeviceArena& mem = p->mem;
    mem.note(p->stream.open(stream, 10));
    const size_t rows = (size_t)p->frames_total * M;
    mem.take(&p->x, (size_t)std::max(p->samples_total, p->frames_total * hop) * M * sizeof(float));
    mem.take(&p->frames, rows * frame * sizeof(float));
    mem.take(&p->spec, rows * F * sizeof(float2));
    mem.take(&p->X, rows * F * sizeof(float2));
    mem.take_filled(&p->rooms_dev, p->rooms.data(), (size_t)B * sizeof(BstftRoom));
    if (win_a) mem.take_filled(&p->win_a, win_a, frame * sizeof(float));
    if (win_s) mem.take_filled(&p->win_s, win_s, frame * sizeof(float));
    if (!mem.ok()) {
        const hipError_t e = mem.status();
        oiva_bstft_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_bstft_destroy(oiva_bstft* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->have_fwd) (void)hipfftDestroy(p->fwd);
    if (p->have_inv) (void)hipfftDestroy(p->inv);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_bstft_shape(oiva_bstft* p, int* frames, int* n_freq) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    if (frames)
        for (int b = 0; b < p->B; ++b) frames[b] = p->rooms[b].T;
    if (n_freq) *n_freq = p->F;
    return OIVA_OK;
}

oiva_status oiva_bstft_analysis(oiva_bstft* p, const float* x_host, void** X_dev) {
    OIVA_NEED(p && x_host && X_dev, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    return analysis_from(p, X_dev, [&] {
        return hipMemcpyAsync(p->x, x_host, (size_t)p->samples_total * p->M * sizeof(float), hipMemcpyHostToDevice, p->stream);
    });
}

oiva_status oiva_bstft_analysis_dev(oiva_bstft* p, const void* x_dev, int f64, void** X_dev) {
    OIVA_NEED(p && x_dev && X_dev, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(f64 == 0 || f64 == 1, OIVA_ERR_ARG, "f64 must be 0 (float32 audio) or 1 (float64 audio)");
    DeviceGuard guard(p->device);
    const long long n = p->samples_total * p->M;
    return analysis_from(p, X_dev, [&] {
        if (f64) return launch_sweep_cast(p->stream, static_cast<const double*>(x_dev), p->x, n);
        return hipMemcpyAsync(p->x, x_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, p->stream);
    });
}

oiva_status oiva_bstft_synthesis_keep(oiva_bstft* p, const void* Y_dev, int K, void** y_dev) {
    OIVA_NEED(p && Y_dev && y_dev, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(K >= 1 && K <= p->M, OIVA_ERR_ARG, "synthesis takes 1..M channels");
    DeviceGuard guard(p->device);
    const int rc = synthesis_to_x(p, Y_dev, K);
    if (rc) return rc;
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[9], p->stream));      // (no download: that phase reads 0)
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->timed_s = p->kept_s = true;
    *y_dev = p->x;
    return OIVA_OK;
}

oiva_status oiva_bstft_synthesis_dev(oiva_bstft* p, const void* Y_dev, int K, float* y_host) {
    OIVA_NEED(p && Y_dev && y_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(K >= 1 && K <= p->M, OIVA_ERR_ARG, "synthesis takes 1..M channels");
    DeviceGuard guard(p->device);
    const int rc = synthesis_to_x(p, Y_dev, K);
    if (rc) return rc;
    OIVA_TRY_HIP(hipMemcpyAsync(y_host, p->x, (size_t)p->frames_total * p->hop * K * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[9], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->timed_s = true;
    p->kept_s = false;
    return OIVA_OK;
}

oiva_status oiva_bstft_phase_ms(oiva_bstft* p, float* ms) {
    OIVA_NEED(p && ms, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    for (int i = 0; i < kPhases; ++i) ms[i] = 0.f;
    if (p->timed_a)
        for (int i = 0; i < 4; ++i) OIVA_TRY_HIP(hipEventElapsedTime(&ms[i], p->stream.events[i], p->stream.events[i + 1]));
    if (p->timed_s)
        for (int i = 0; i < (p->kept_s ? 3 : 4); ++i)
            OIVA_TRY_HIP(hipEventElapsedTime(&ms[4 + i], p->stream.events[5 + i], p->stream.events[6 + i]));
    return OIVA_OK;
}

oiva_status oiva_device_to_host(void* host, const void* dev, long long bytes) {
    OIVA_NEED(host && dev, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(bytes >= 0, OIVA_ERR_ARG, "negative size");
    OIVA_TRY_HIP(hipMemcpy(host, dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return OIVA_OK;
}

}  // extern "C"
