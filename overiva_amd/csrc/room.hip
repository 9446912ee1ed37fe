// C ABI of the shoebox room simulation (oiva_room_*, include/overiva_hip.h): image-source impulse responses, premix and mix-down of
// B rooms of S sources and M microphones, each room of its own size, lengths and signal length, in float64.  Host code only; the
// kernels live in kernels_room.hip and the algorithm is DESIGN.md 3.11.
//
//   compute_rir : k_max of every room -> Lr_b, then every sample of every impulse response, rir packed (sum_b S M Lr_b)
//   set_signals : packed signals (sum_b S n_b) float64, host -> device; sizes the transforms and the room groups
//   convolve    : one group of rooms, room by room: pad | D2Z of the S signals and the S M responses | product | Z2D | unpack
//   mix         : one group of rooms, room by room: standard deviations at ref_mic | weighted sums -> mix, ref
//   oiva_decay_room_set_absorption : new wall absorptions: the responses become stale and compute_rir may run again (the image
//                 kernel alone: k_max, the lengths and the buffers stay); oiva_decay_set_room lends the responses to a decay handle
// The convolution is ONE transform per signal, of nfft_b = the power of two >= n_b + Lr_b - 1 points: a room's plans follow from
// its own (nfft_b, S, M), and rooms with the same nfft share them.  When the premix of all rooms does not fit the device (or
// max_group asks for less) the rooms go through convolve and mix in groups; a room's bits do not depend on the grouping, on B or
// on the other rooms, since every launch after the impulse responses holds one room.  Every call is synchronous.
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {
constexpr int kStages = 4;      // k_max, impulse responses, convolution, mix-down
constexpr int kMaxGrid = 65535;

struct RoomPlans {
    hipfftHandle fwd = 0, inv = 0;      // D2Z of S + S M rows, Z2D of S M rows
};
struct RoomSig {
    int n = 0, n_out = 0, nfft = 0;
    long long sig_off = 0;              // first element of the room's (S, n) signals in the packed signals
    long long prem_off = 0, mix_off = 0;      // of its premix (S, M, n_out) and mix (n_out, M) in the group's buffers
};
}  // namespace

struct oiva_room {
    int device = 0;
    int B = 0, S = 0, M = 0, max_order = 0, n_img = 0, fixed_len = 0;
    double fs_over_c = 0.;
    int group = 0, mix_K = 0;
    bool have_rir = false, have_sig = false;
    std::vector<char> convolved, mixed;      // per group start g0
    HandleStream stream;               // two events: the bracket of oiva_room_time_stages
    DeviceArena mem;
    std::vector<RoomRec> rooms;
    std::vector<RoomSig> sig;
    std::map<int, RoomPlans> plans;    // by nfft
    RoomRec* rooms_dev = nullptr;
    char4* images = nullptr;
    double *src = nullptr, *mic = nullptr, *rir = nullptr, *signals = nullptr;
    int* kmax = nullptr;
    double *real = nullptr, *premix = nullptr, *mix = nullptr, *ref = nullptr, *noise = nullptr, *std = nullptr, *scale = nullptr;
    double2* spec = nullptr;
    long long rir_total = 0, sig_total = 0;
    size_t sig_mark = 0, mix_mark = 0;
    bool have_sig_mark = false, have_mix_mark = false;
};

namespace {

int n_images(int N) { return (2 * N + 1) * (2 * N * N + 2 * N + 3) / 3; }

int next_pow2(long long n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// elements of the premix and of the mix of the largest group of `group` consecutive rooms
void group_extent(const oiva_room* p, int group, size_t* prem, size_t* mix) {
    *prem = *mix = 0;
    for (int g0 = 0; g0 < p->B; g0 += group) {
        size_t a = 0, b = 0;
        for (int r = g0; r < std::min(p->B, g0 + group); ++r) {
            a += (size_t)p->S * p->M * p->sig[r].n_out;
            b += (size_t)p->M * p->sig[r].n_out;
        }
        *prem = std::max(*prem, a);
        *mix = std::max(*mix, b);
    }
}

void place_group(oiva_room* p) {
    for (int g0 = 0; g0 < p->B; g0 += p->group) {
        long long a = 0, b = 0;
        for (int r = g0; r < std::min(p->B, g0 + p->group); ++r) {
            p->sig[r].prem_off = a;
            p->sig[r].mix_off = b;
            a += (long long)p->S * p->M * p->sig[r].n_out;
            b += (long long)p->M * p->sig[r].n_out;
        }
    }
}

int stage_kmax(oiva_room* p) {
    OIVA_TRY_HIP(hipMemsetAsync(p->kmax, 0, (size_t)p->B * sizeof(int), p->stream));
    OIVA_TRY_HIP(launch_room_kmax(p->stream, p->rooms_dev, p->src, p->mic, p->images, p->n_img, p->B, p->S, p->M, p->fs_over_c, p->kmax));
    return OIVA_OK;
}

int stage_rir(oiva_room* p) {
    int longest = 0;
    for (const RoomRec& r : p->rooms) longest = std::max(longest, r.Lr);
    OIVA_TRY_HIP(launch_room_rir(p->stream, p->rooms_dev, p->src, p->mic, p->images, p->n_img, p->B, p->S, p->M, longest, p->fs_over_c,
                                 p->rir));
    return OIVA_OK;
}

int plans_of(oiva_room* p, int nfft, RoomPlans** out) {
    auto it = p->plans.find(nfft);
    if (it == p->plans.end()) {
        RoomPlans pl;
        int n[1] = {nfft};
        const int nf = nfft / 2 + 1, SM = p->S * p->M;
        OIVA_TRY_FFT(hipfftPlanMany(&pl.fwd, 1, n, nullptr, 1, nfft, nullptr, 1, nf, HIPFFT_D2Z, p->S + SM));
        if (hipfftPlanMany(&pl.inv, 1, n, nullptr, 1, nf, nullptr, 1, nfft, HIPFFT_Z2D, SM) != HIPFFT_SUCCESS) {
            (void)hipfftDestroy(pl.fwd);
            return fail_with(OIVA_ERR_HIP, "hipfftPlanMany (Z2D) failed for " + std::to_string(nfft) + " points");
        }
        it = p->plans.emplace(nfft, pl).first;
        OIVA_TRY_FFT(hipfftSetStream(pl.fwd, p->stream));
        OIVA_TRY_FFT(hipfftSetStream(pl.inv, p->stream));
    }
    *out = &it->second;
    return OIVA_OK;
}

int convolve_room(oiva_room* p, int b) {
    const RoomSig& g = p->sig[b];
    const RoomRec& r = p->rooms[b];
    const int S = p->S, SM = p->S * p->M, nfft = g.nfft, nf = nfft / 2 + 1;
    RoomPlans* pl = nullptr;
    const int rc = plans_of(p, nfft, &pl);
    if (rc) return rc;
    double* rows_h = p->real + (size_t)S * nfft;
    double2* spec_h = p->spec + (size_t)S * nf;
    OIVA_TRY_HIP(launch_room_pad(p->stream, p->signals + g.sig_off, g.n, g.n, p->real, nfft, S));
    OIVA_TRY_HIP(launch_room_pad(p->stream, p->rir + r.rir_off, r.Lr, r.Lr, rows_h, nfft, SM));
    OIVA_TRY_FFT(hipfftExecD2Z(pl->fwd, p->real, reinterpret_cast<hipfftDoubleComplex*>(p->spec)));
    OIVA_TRY_HIP(launch_room_product(p->stream, spec_h, p->spec, nf, S, p->M));
    OIVA_TRY_FFT(hipfftExecZ2D(pl->inv, reinterpret_cast<hipfftDoubleComplex*>(spec_h), rows_h));
    OIVA_TRY_HIP(launch_room_unpack(p->stream, rows_h, nfft, p->premix + g.prem_off, g.n_out, SM));
    return OIVA_OK;
}

int stage_convolve(oiva_room* p, int g0) {
    for (int b = g0; b < std::min(p->B, g0 + p->group); ++b) {
        const int rc = convolve_room(p, b);
        if (rc) return rc;
    }
    return OIVA_OK;
}

int stage_mix(oiva_room* p, int g0, int K, double sigma_n, int ref_mic, bool with_noise) {
    for (int b = g0; b < std::min(p->B, g0 + p->group); ++b) {
        const RoomSig& g = p->sig[b];
        const double* prem = p->premix + g.prem_off;
        double* std = p->std + (size_t)b * p->S;
        OIVA_TRY_HIP(launch_room_std(p->stream, prem, p->S, p->M, g.n_out, ref_mic, std));
        OIVA_TRY_HIP(launch_room_mix(p->stream, prem, std, p->scale, with_noise ? p->noise + g.mix_off : nullptr, sigma_n, p->S, p->M, K,
                                     g.n_out, p->mix + g.mix_off, p->ref + (size_t)(K + 1) * g.mix_off));
    }
    return OIVA_OK;
}

// scale[s] of the S sources and sigma_n
int mix_scales(const oiva_room* p, int K, double sinr, double snr, const double* sources_var, std::vector<double>* scale,
               double* sigma_n) {
    double total = 0.;
    for (int s = 0; s < K; ++s) {
        const double v = sources_var ? sources_var[s] : 1.;
        OIVA_NEED(std::isfinite(v) && v >= 0., OIVA_ERR_ARG, "sources_var must be finite and >= 0");
        total += v;
    }
    OIVA_NEED(!std::isnan(sinr) && !std::isnan(snr), OIVA_ERR_ARG, "sinr and snr must not be NaN");
    OIVA_NEED(K < p->S || (std::isinf(sinr) && sinr > 0.), OIVA_ERR_ARG, "without interferers (n_targets == S) sinr must be +inf");
    *sigma_n = std::sqrt(std::pow(10., -snr / 10.) * total);
    const double sigma_i =
        K < p->S ? std::sqrt(std::max(0., std::pow(10., -sinr / 10.) * total - *sigma_n * *sigma_n) / (double)(p->S - K)) : 0.;
    scale->assign(p->S, sigma_i);
    for (int s = 0; s < K; ++s) (*scale)[s] = std::sqrt(sources_var ? sources_var[s] : 1.);
    return OIVA_OK;
}

// the group's mix, ref and noise buffers for K targets
int alloc_mix(oiva_room* p, int K) {
    if (p->have_mix_mark && p->mix_K == K) return OIVA_OK;
    if (p->have_mix_mark) p->mem.release_to(p->mix_mark);
    p->have_mix_mark = false;
    size_t prem = 0, mix = 0;
    group_extent(p, p->group, &prem, &mix);
    const size_t keep = p->mem.mark();
    p->mem.take(&p->mix, mix * sizeof(double), Mem::pooled);
    p->mem.take(&p->noise, mix * sizeof(double), Mem::pooled);
    p->mem.take(&p->ref, (size_t)(K + 1) * mix * sizeof(double), Mem::pooled);
    const hipError_t e = p->mem.status();
    if (e != hipSuccess) {
        p->mem.release_to(keep);
        return fail_with(OIVA_ERR_HIP, std::string("allocation of the mix failed: ") + hipGetErrorString(e));
    }
    p->mix_mark = keep;
    p->have_mix_mark = true;
    p->mix_K = K;
    return OIVA_OK;
}

}  // namespace

// the sweep's view of a mixed group (sweep.hip): where its mix and its references lie on the device
int oiva::room_group_view(oiva_room* p, int g0, RoomGroupView* view, int* n_out, long long* mix_off, int max_rooms) {
    OIVA_NEED(p->have_sig && g0 >= 0 && g0 < p->B && g0 % p->group == 0 && p->mixed[g0], OIVA_ERR_STATE,
              "this group of the room handle has not been mixed");
    const int last = std::min(p->B, g0 + p->group) - 1;
    view->device = p->device, view->rooms = last - g0 + 1, view->M = p->M, view->K = p->mix_K;
    view->mix = p->mix, view->ref = p->ref;
    view->mix_total = p->sig[last].mix_off + (long long)p->M * p->sig[last].n_out;
    for (int b = g0; b <= last && b - g0 < max_rooms; ++b) {
        n_out[b - g0] = p->sig[b].n_out;
        mix_off[b - g0] = p->sig[b].mix_off;
    }
    return OIVA_OK;
}

// oiva_room_mix, and oiva_rng_room_mix (rng.hip) with the keys of the group's rooms: the noise is then drawn where the copy from
// the host would have put it, one stream per room at the room's place in the group's buffer, and the same mix-down runs
int oiva::room_mix_body(oiva_room* p, int g0, int K, double sinr, double snr, int ref_mic, const double* sources_var,
                        const double* noise_host, const unsigned long long* key0, const unsigned long long* key1) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(K >= 1 && K <= p->S, OIVA_ERR_ARG, "n_targets must be in 1..S");
    OIVA_NEED(ref_mic >= 0 && ref_mic < p->M, OIVA_ERR_ARG, "ref_mic must be in 0..M-1");
    OIVA_NEED(p->have_sig && g0 >= 0 && g0 < p->B && p->convolved[g0], OIVA_ERR_STATE, "this group has not been convolved");
    std::vector<double> scale;
    double sigma_n = 0.;
    int rc = mix_scales(p, K, sinr, snr, sources_var, &scale, &sigma_n);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    if ((rc = alloc_mix(p, K))) return rc;
    const int last = std::min(p->B, g0 + p->group) - 1;
    const size_t n = (size_t)p->sig[last].mix_off + (size_t)p->M * p->sig[last].n_out;
    ScopedDev tmp(p->device);
    OIVA_TRY_HIP(hipMemcpyAsync(p->scale, scale.data(), (size_t)p->S * sizeof(double), hipMemcpyHostToDevice, p->stream));
    if (noise_host) OIVA_TRY_HIP(hipMemcpyAsync(p->noise, noise_host, n * sizeof(double), hipMemcpyHostToDevice, p->stream));
    if (key0) {
        std::vector<RngStream> streams(last - g0 + 1);
        long long longest = 0;
        for (int b = g0; b <= last; ++b) {
            const long long count = (long long)p->M * p->sig[b].n_out;      // (ends inside the noise buffer: alloc_mix sized it so)
            streams[b - g0] = RngStream{key0[b - g0], key1[b - g0], p->sig[b].mix_off, count};
            longest = std::max(longest, count);
        }
        RngStream* streams_dev = nullptr;
        tmp.take_filled(&streams_dev, streams.data(), streams.size() * sizeof(RngStream));
        OIVA_TRY_HIP(tmp.status());
        OIVA_TRY_HIP(launch_rng_normal(p->stream, streams_dev, (int)streams.size(), longest, 0ull, p->noise));
    }
    if ((rc = stage_mix(p, g0, K, sigma_n, ref_mic, noise_host != nullptr || key0 != nullptr))) {
        (void)hipStreamSynchronize(p->stream);      // (the stream table is this call's)
        return rc;
    }
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));      // (scale is the caller's stack until here)
    p->mixed[g0] = 1;
    return OIVA_OK;
}

extern "C" {

oiva_status oiva_room_create(oiva_room** out, int device, int B, int S, int M, double fs, double c, int max_order, const double* room_dim,
                             const double* sources, const double* mics, const double* absorption6, int rir_length, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(room_dim && sources && mics && absorption6, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(B >= 1 && B <= kMaxGrid, OIVA_ERR_ARG, "B must be in 1..65535");
    OIVA_NEED(S >= 1 && S <= kRoomMaxSrc, OIVA_ERR_ARG, "the room simulation runs on 1..16 sources");
    OIVA_NEED(M >= 1 && M <= kRoomMaxMic, OIVA_ERR_ARG, "the room simulation runs on 1..32 microphones");
    OIVA_NEED(std::isfinite(fs) && fs > 0. && std::isfinite(c) && c > 0., OIVA_ERR_ARG, "fs and c must be finite and > 0");
    OIVA_NEED(max_order >= 0 && max_order <= kRoomMaxOrder, OIVA_ERR_ARG, "max_order must be in 0..32");
    OIVA_NEED(rir_length >= 0 && rir_length <= kRoomMaxRir, OIVA_ERR_ARG, "rir_length must be in 1..65536 (0: per room)");
    // the farthest image is nearer than (max_order + 1) diagonals: its k must stay an int whatever the lengths are
    for (int b = 0; b < B; ++b) {
        double diag = 0.;
        for (int a = 0; a < 3; ++a) {
            const double L = room_dim[b * 3 + a];
            OIVA_NEED(std::isfinite(L) && L > 0., OIVA_ERR_ARG, "room " + std::to_string(b) + ": the box must have finite sides > 0");
            diag += L * L;
            for (int s = 0; s < S; ++s) {
                const double x = sources[((size_t)b * S + s) * 3 + a];
                OIVA_NEED(x > 0. && x < L, OIVA_ERR_ARG, "room " + std::to_string(b) + ": a source is not strictly inside the box");
            }
            for (int m = 0; m < M; ++m) {
                const double x = mics[((size_t)b * M + m) * 3 + a];
                OIVA_NEED(x > 0. && x < L, OIVA_ERR_ARG, "room " + std::to_string(b) + ": a microphone is not strictly inside the box");
            }
        }
        OIVA_NEED((max_order + 1) * std::sqrt(diag) * fs / c < 5e8, OIVA_ERR_ARG,
                  "room " + std::to_string(b) + ": the delays do not fit an int");
        for (int w = 0; w < 6; ++w) {
            const double a = absorption6[b * 6 + w];
            OIVA_NEED(a >= 0. && a < 1., OIVA_ERR_ARG, "absorption must be in [0, 1)");
        }
        for (int s = 0; s < S; ++s)
            for (int m = 0; m < M; ++m) {
                const double* x = sources + ((size_t)b * S + s) * 3;
                const double* y = mics + ((size_t)b * M + m) * 3;
                OIVA_NEED(x[0] != y[0] || x[1] != y[1] || x[2] != y[2], OIVA_ERR_ARG,
                          "room " + std::to_string(b) + ": a source at zero distance from a microphone");
            }
    }
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_room* p = new oiva_room();
    p->device = p->mem.device = device;
    p->B = B, p->S = S, p->M = M, p->max_order = max_order, p->fixed_len = rir_length;
    p->fs_over_c = fs / c;
    p->n_img = n_images(max_order);
    std::vector<char4> img;
    img.reserve(p->n_img);
    for (int nx = -max_order; nx <= max_order; ++nx)
        for (int ny = -max_order; ny <= max_order; ++ny)
            for (int nz = -max_order; nz <= max_order; ++nz)
                if (std::abs(nx) + std::abs(ny) + std::abs(nz) <= max_order) img.push_back(make_char4((char)nx, (char)ny, (char)nz, 0));
    p->rooms.resize(B);
    for (int b = 0; b < B; ++b) {
        RoomRec& r = p->rooms[b];
        for (int a = 0; a < 3; ++a) r.dim[a] = room_dim[b * 3 + a];
        for (int w = 0; w < 6; ++w) r.beta[w] = std::sqrt(1. - absorption6[b * 6 + w]);
        r.rir_off = 0, r.Lr = 0, r.pad = 0;
    }
    DeviceArena& mem = p->mem;
    mem.note(p->stream.open(stream, 2));
    mem.take_filled(&p->images, img.data(), img.size() * sizeof(char4));
    mem.take_filled(&p->src, sources, (size_t)B * S * 3 * sizeof(double));
    mem.take_filled(&p->mic, mics, (size_t)B * M * 3 * sizeof(double));
    mem.take_filled(&p->rooms_dev, p->rooms.data(), (size_t)B * sizeof(RoomRec));
    mem.take(&p->kmax, (size_t)B * sizeof(int));
    mem.take(&p->std, (size_t)B * S * sizeof(double));
    mem.take(&p->scale, (size_t)S * sizeof(double));
    if (!mem.ok() || (int)img.size() != p->n_img) {
        const hipError_t e = mem.status();
        oiva_room_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_room_destroy(oiva_room* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (auto& kv : p->plans) {
        (void)hipfftDestroy(kv.second.fwd);
        (void)hipfftDestroy(kv.second.inv);
    }
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_room_compute_rir(oiva_room* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(!p->have_rir, OIVA_ERR_STATE, "the impulse responses of this handle are computed already");
    DeviceGuard guard(p->device);
    if (p->rir) {      // after new absorptions: k_max, the lengths and the buffer do not depend on them
        const int rc = stage_rir(p);
        if (rc) return rc;
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        p->have_rir = true;
        return OIVA_OK;
    }
    int rc = stage_kmax(p);
    if (rc) return rc;
    std::vector<int> kmax(p->B);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(kmax.data(), p->kmax, (size_t)p->B * sizeof(int), hipMemcpyDeviceToHost));
    p->rir_total = 0;
    for (int b = 0; b < p->B; ++b) {
        RoomRec& r = p->rooms[b];
        const long long L = p->fixed_len ? p->fixed_len : (long long)kmax[b] + kRoomFdl;
        OIVA_NEED(L >= 1 && L <= kRoomMaxRir, OIVA_ERR_ARG, "room " + std::to_string(b) + ": impulse responses of " + std::to_string(L) +
                                                                 " samples (at most 65536)");
        r.Lr = (int)L;
        r.rir_off = p->rir_total;
        p->rir_total += (long long)p->S * p->M * L;
    }
    OIVA_TRY_HIP(hipMemcpy(p->rooms_dev, p->rooms.data(), (size_t)p->B * sizeof(RoomRec), hipMemcpyHostToDevice));
    const hipError_t e = p->mem.take_one(&p->rir, (size_t)p->rir_total * sizeof(double), Mem::pooled);
    if (e != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("allocation of the impulse responses failed: ") + hipGetErrorString(e));
    rc = stage_rir(p);
    if (rc) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->have_rir = true;
    return OIVA_OK;
}

oiva_status oiva_room_rir_lengths(oiva_room* p, int* lengths, int* images) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_rir || !lengths, OIVA_ERR_STATE, "compute_rir has not run");
    if (lengths)
        for (int b = 0; b < p->B; ++b) lengths[b] = p->rooms[b].Lr;
    if (images) *images = p->n_img;
    return OIVA_OK;
}

oiva_status oiva_room_get_rir(oiva_room* p, double* rir_host) {
    OIVA_NEED(p && rir_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_rir, OIVA_ERR_STATE, "compute_rir has not run");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpy(rir_host, p->rir, (size_t)p->rir_total * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_room_set_signals(oiva_room* p, const int* n_samples, const double* signals_host, int max_group) {
    OIVA_NEED(p && n_samples && signals_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_rir, OIVA_ERR_STATE, "compute_rir has not run");
    OIVA_NEED(max_group >= 0, OIVA_ERR_ARG, "max_group must be >= 0");
    for (int b = 0; b < p->B; ++b) {
        OIVA_NEED(n_samples[b] >= 1, OIVA_ERR_ARG, "room " + std::to_string(b) + " has no samples");
        OIVA_NEED((long long)n_samples[b] + p->rooms[b].Lr - 1 <= (1ll << 26), OIVA_ERR_ARG,
                  "room " + std::to_string(b) + " is too long (2^26 output samples per room)");
    }
    DeviceGuard guard(p->device);
    if (p->have_sig_mark) p->mem.release_to(p->sig_mark);      // (the mix buffers lie above: they go too)
    p->have_sig_mark = p->have_mix_mark = p->have_sig = false;
    p->sig.assign(p->B, RoomSig());
    p->sig_total = 0;
    int nfft_max = 0;
    for (int b = 0; b < p->B; ++b) {
        RoomSig& g = p->sig[b];
        g.n = n_samples[b];
        g.n_out = g.n + p->rooms[b].Lr - 1;
        g.nfft = next_pow2(g.n_out);
        g.sig_off = p->sig_total;
        p->sig_total += (long long)p->S * g.n;
        nfft_max = std::max(nfft_max, g.nfft);
    }
    const size_t rows = (size_t)p->S + (size_t)p->S * p->M;
    const size_t keep = p->mem.mark();
    p->mem.take(&p->signals, (size_t)p->sig_total * sizeof(double), Mem::pooled);
    p->mem.take(&p->real, rows * nfft_max * sizeof(double), Mem::pooled);
    p->mem.take(&p->spec, rows * (nfft_max / 2 + 1) * sizeof(double2), Mem::pooled);
    hipError_t e = p->mem.status();
    if (e == hipSuccess) {
        // as many rooms per group as the memory holds: halve until the allocation succeeds
        int group = max_group > 0 ? std::min(p->B, max_group) : p->B;
        const size_t inner = p->mem.mark();
        for (;;) {
            size_t prem = 0, mix = 0;
            group_extent(p, group, &prem, &mix);
            e = p->mem.take_one(&p->premix, prem * sizeof(double), Mem::pooled);
            if (e != hipErrorOutOfMemory || group == 1) break;
            (void)hipGetLastError();
            p->mem.release_to(inner);
            group = (group + 1) / 2;
        }
        p->group = group;
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->signals, signals_host, (size_t)p->sig_total * sizeof(double), hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) {
        p->mem.release_to(keep);
        return fail_with(OIVA_ERR_HIP, std::string("set_signals failed: ") + hipGetErrorString(e));
    }
    place_group(p);
    p->sig_mark = keep;
    p->have_sig_mark = true;
    p->have_sig = true;
    p->convolved.assign(p->B, 0);
    p->mixed.assign(p->B, 0);
    return OIVA_OK;
}

oiva_status oiva_room_groups(oiva_room* p, int* rooms_per_group) {
    OIVA_NEED(p && rooms_per_group, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    *rooms_per_group = p->group;
    return OIVA_OK;
}

oiva_status oiva_room_convolve(oiva_room* p, int g0) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    OIVA_NEED(p->have_rir, OIVA_ERR_STATE, "the absorptions changed: compute_rir has not run since");
    OIVA_NEED(g0 >= 0 && g0 < p->B && g0 % p->group == 0, OIVA_ERR_ARG, "g0 must be the first room of a group");
    DeviceGuard guard(p->device);
    std::fill(p->convolved.begin(), p->convolved.end(), 0);      // (one premix buffer: the group before is gone)
    std::fill(p->mixed.begin(), p->mixed.end(), 0);
    const int rc = stage_convolve(p, g0);
    if (rc) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->convolved[g0] = 1;
    return OIVA_OK;
}

oiva_status oiva_room_get_premix(oiva_room* p, int g0, double* premix_host) {
    OIVA_NEED(p && premix_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_sig && g0 >= 0 && g0 < p->B && p->convolved[g0], OIVA_ERR_STATE, "this group has not been convolved");
    DeviceGuard guard(p->device);
    const int last = std::min(p->B, g0 + p->group) - 1;
    const size_t n = (size_t)p->sig[last].prem_off + (size_t)p->S * p->M * p->sig[last].n_out;
    OIVA_TRY_HIP(hipMemcpy(premix_host, p->premix, n * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_room_mix(oiva_room* p, int g0, int K, double sinr, double snr, int ref_mic, const double* sources_var,
                          const double* noise_host) {
    return room_mix_body(p, g0, K, sinr, snr, ref_mic, sources_var, noise_host, nullptr, nullptr);
}

oiva_status oiva_room_get_mix(oiva_room* p, int g0, double* mix_host, double* ref_host) {
    OIVA_NEED(p && mix_host && ref_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_sig && g0 >= 0 && g0 < p->B && p->mixed[g0], OIVA_ERR_STATE, "this group has not been mixed");
    DeviceGuard guard(p->device);
    const int last = std::min(p->B, g0 + p->group) - 1;
    const size_t n = (size_t)p->sig[last].mix_off + (size_t)p->M * p->sig[last].n_out;
    OIVA_TRY_HIP(hipMemcpy(mix_host, p->mix, n * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(ref_host, p->ref, (size_t)(p->mix_K + 1) * n * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_room_time_stages(oiva_room* p, int n, int K, double sinr, double snr, int ref_mic, float* per_stage_ms) {
    OIVA_NEED(p && per_stage_ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(n >= 1, OIVA_ERR_ARG, "n must be >= 1");
    OIVA_NEED(K >= 1 && K <= p->S, OIVA_ERR_ARG, "n_targets must be in 1..S");
    OIVA_NEED(ref_mic >= 0 && ref_mic < p->M, OIVA_ERR_ARG, "ref_mic must be in 0..M-1");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    OIVA_NEED(p->have_rir, OIVA_ERR_STATE, "the absorptions changed: compute_rir has not run since");
    std::vector<double> scale;
    double sigma_n = 0.;
    int rc = mix_scales(p, K, sinr, snr, nullptr, &scale, &sigma_n);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    if ((rc = alloc_mix(p, K))) return rc;
    OIVA_TRY_HIP(hipMemcpy(p->scale, scale.data(), (size_t)p->S * sizeof(double), hipMemcpyHostToDevice));
    for (int b = 0; b < p->B; ++b) {                      // (the plans are made outside the brackets)
        RoomPlans* pl = nullptr;
        if ((rc = plans_of(p, p->sig[b].nfft, &pl))) return rc;
    }
    std::fill(p->convolved.begin(), p->convolved.end(), 0);
    std::fill(p->mixed.begin(), p->mixed.end(), 0);
    double sum[kStages] = {};
    for (int it = 0; it < n; ++it) {
        float ms = 0.f;
        if ((rc = p->stream.elapsed_ms(0, 1, [&] { return stage_kmax(p); }, &ms))) return rc;
        sum[0] += ms;
        if ((rc = p->stream.elapsed_ms(0, 1, [&] { return stage_rir(p); }, &ms))) return rc;
        sum[1] += ms;
        for (int g0 = 0; g0 < p->B; g0 += p->group) {
            if ((rc = p->stream.elapsed_ms(0, 1, [&] { return stage_convolve(p, g0); }, &ms))) return rc;
            sum[2] += ms;
            if ((rc = p->stream.elapsed_ms(0, 1, [&] { return stage_mix(p, g0, K, sigma_n, ref_mic, false); }, &ms))) return rc;
            sum[3] += ms;
        }
    }
    for (int s = 0; s < kStages; ++s) per_stage_ms[s] = (float)(sum[s] / n);
    const int last_g0 = (p->B - 1) / p->group * p->group;
    p->convolved[last_g0] = p->mixed[last_g0] = 1;
    return OIVA_OK;
}

// ---- the decay measurement's view of the room handle (oiva_decay_*, decay.hip) ---------------------------------
oiva_status oiva_decay_set_room(oiva_decay* decay, oiva_room* p) {
    OIVA_NEED(decay && p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_rir, OIVA_ERR_STATE, "compute_rir has not run");
    std::vector<int> lengths;
    lengths.reserve((size_t)p->B * p->S * p->M);
    for (const RoomRec& r : p->rooms) lengths.insert(lengths.end(), (size_t)p->S * p->M, r.Lr);
    return decay_bind(decay, p->device, p->rir, lengths.data(), (int)lengths.size());
}

oiva_status oiva_decay_room_set_absorption(oiva_room* p, const double* absorption6) {
    OIVA_NEED(p && absorption6, OIVA_ERR_ARG, "null argument");
    for (int i = 0; i < p->B * 6; ++i) OIVA_NEED(absorption6[i] >= 0. && absorption6[i] < 1., OIVA_ERR_ARG, "absorption must be in [0, 1)");
    DeviceGuard guard(p->device);
    for (int b = 0; b < p->B; ++b)
        for (int w = 0; w < 6; ++w) p->rooms[b].beta[w] = std::sqrt(1. - absorption6[b * 6 + w]);
    p->have_rir = false;
    std::fill(p->convolved.begin(), p->convolved.end(), 0);
    std::fill(p->mixed.begin(), p->mixed.end(), 0);
    OIVA_TRY_HIP(hipMemcpy(p->rooms_dev, p->rooms.data(), (size_t)p->B * sizeof(RoomRec), hipMemcpyHostToDevice));
    return OIVA_OK;
}

}  // extern "C"
