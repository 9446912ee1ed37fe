// C ABI of the sweep step (oiva_sweep_*, include/overiva_hip.h): the hand-overs that keep the audio on the device from the mix of
// the room simulation to the criteria of BSS Eval.  Host code only; the kernels live in kernels_sweep.hip and the contract is
// DESIGN.md 3.12.
//
//   take_mix : the mixed group g0 of an oiva_room -> oiva_bstft_analysis_dev of its float64 mix; remembers where its ref lies
//   evaluate : Y (sum T_b, F, C) complex64, device -> oiva_bstft_synthesis_keep | standard deviation of every channel | order |
//              est and ref of an oiva_bsseval handle, on the device; the caller then runs oiva_bsseval_run
// One handle = the rooms of one group: their output lengths n_out_b, (M, K, frame, hop, ref_mic).  Of room b the samples
// [0, m_b), m_b = T_b hop - (frame - hop), T_b = n_out_b / hop, are evaluated: this project's STFT has no delay, so these are
// the samples the reference's y[frame / 2 : m + frame / 2] names (its hop is frame / 2).  Every call is synchronous.
#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {
constexpr int kAlignOffset = 0;      // first sample of y that lines up with sample 0 of the references
}  // namespace

struct oiva_sweep {
    int device = 0;
    int B = 0, M = 0, K = 0, frame = 0, hop = 0, ref_mic = 0, Lf = 0;
    int max_m = 0, max_chunks = 0;
    long long m_total = 0, y_total = 0;
    HandleStream stream;
    DeviceArena mem;
    std::vector<SweepRoom> rooms;
    SweepRoom* rooms_dev = nullptr;
    double *filler = nullptr, *std = nullptr, *part = nullptr;
    int* order = nullptr;
    oiva_room* room = nullptr;       // whose group g0 was taken (its ref is read by every evaluate)
    int g0 = -1;
    const double* room_ref = nullptr;
    bool have_filler = false;
    int last_C = 0;                  // channels of the last evaluate, 0: none
};

namespace {

// the handles of one evaluate agree with the sweep handle
int check_bstft(const oiva_sweep* p, oiva_bstft* st) {
    int device = 0, B = 0, M = 0, frame = 0, hop = 0;
    long long samples = 0;
    bstft_dims(st, &device, &B, &M, &frame, &hop, &samples);
    long long want = 0;
    for (const SweepRoom& r : p->rooms) want += r.n_out;
    OIVA_NEED(device == p->device && B == p->B && M == p->M && frame == p->frame && hop == p->hop && samples == want, OIVA_ERR_ARG,
              "the STFT handle was not made for this sweep's rooms (device, B, M, frame, hop, lengths)");
    return OIVA_OK;
}

int check_bsseval(const oiva_sweep* p, oiva_bsseval* ev, BssSignalView* view) {
    std::vector<int> lengths(p->B);
    bsseval_signal_view(ev, view, lengths.data(), p->B);
    bool same = view->device == p->device && view->B == p->B && view->N == p->K + 1 && view->Lf == p->Lf;
    for (int b = 0; same && b < p->B; ++b) same = lengths[b] == p->rooms[b].m;
    OIVA_NEED(same, OIVA_ERR_ARG, "the BSS Eval handle was not made for this sweep (device, B, N = K + 1, filter_length, lengths m_b)");
    return OIVA_OK;
}

}  // namespace

extern "C" {

oiva_status oiva_sweep_create(oiva_sweep** out, int device, int B, const int* n_out, int M, int K, int frame, int hop, int ref_mic,
                              int filter_length, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(n_out != nullptr, OIVA_ERR_ARG, "null n_out");
    OIVA_NEED(B >= 1 && B <= 65535, OIVA_ERR_ARG, "B must be in 1..65535");
    OIVA_NEED(M >= 1 && M <= kSweepMaxChan, OIVA_ERR_ARG, "the sweep runs on 1..8 microphones");
    OIVA_NEED(K >= 1 && K <= M && K + 1 <= kBssMaxSrc, OIVA_ERR_ARG, "n_targets must be in 1..min(M, 7)");
    OIVA_NEED(frame >= 2 && frame % 2 == 0, OIVA_ERR_ARG, "frame must be even and >= 2");
    OIVA_NEED(hop >= 1 && hop <= frame, OIVA_ERR_ARG, "hop must be in 1..frame");
    OIVA_NEED(ref_mic >= 0 && ref_mic < M, OIVA_ERR_ARG, "ref_mic must be in 0..M-1");
    OIVA_NEED(filter_length >= 1 && filter_length <= kBssMaxFilter, OIVA_ERR_ARG, "filter_length must be in 1..512");
    std::vector<SweepRoom> rooms(B);
    long long y_total = 0, m_total = 0;
    int max_m = 0, max_ny = 0;
    for (int b = 0; b < B; ++b) {
        SweepRoom& r = rooms[b];
        OIVA_NEED(n_out[b] >= 1 && (long long)n_out[b] * M * (K + 1) < (1ll << 40), OIVA_ERR_ARG,
                  "room " + std::to_string(b) + " has no samples or is too long");
        r.n_out = n_out[b];
        r.ny = n_out[b] / hop * hop;
        const long long m = (long long)r.ny - (frame - hop);
        OIVA_NEED(m >= 1, OIVA_ERR_ARG, "room " + std::to_string(b) + " is too short for one complete frame (" + std::to_string(n_out[b]) +
                                            " samples, frame " + std::to_string(frame) + ", hop " + std::to_string(hop) + ")");
        r.m = (int)m;
        r.y_off = y_total, r.ref_off = 0, r.fil_off = m_total, r.sig_off = (long long)(K + 1) * m_total, r.pad = 0;
        y_total += r.ny;
        m_total += r.m;
        max_m = std::max(max_m, r.m);
        max_ny = std::max(max_ny, r.ny);
    }
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_sweep* p = new oiva_sweep();
    p->device = p->mem.device = device;
    p->B = B, p->M = M, p->K = K, p->frame = frame, p->hop = hop, p->ref_mic = ref_mic, p->Lf = filter_length;
    p->rooms = rooms;
    p->y_total = y_total, p->m_total = m_total, p->max_m = max_m;
    p->max_chunks = (max_ny + kSweepChunk - 1) / kSweepChunk;
    DeviceArena& mem = p->mem;
    mem.note(p->stream.open(stream, 2));
    mem.take_filled(&p->rooms_dev, p->rooms.data(), (size_t)B * sizeof(SweepRoom));
    mem.take(&p->filler, (size_t)m_total * sizeof(double), Mem::pooled);
    mem.take(&p->std, (size_t)B * kSweepMaxChan * sizeof(double));
    mem.take(&p->order, (size_t)B * kSweepMaxChan * sizeof(int));
    mem.take(&p->part, (size_t)2 * B * kSweepMaxChan * p->max_chunks * sizeof(double));
    if (!mem.ok()) {
        const hipError_t e = mem.status();
        oiva_sweep_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_sweep_destroy(oiva_sweep* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_sweep_set_filler(oiva_sweep* p, const double* filler_host) {
    OIVA_NEED(p && filler_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpyAsync(p->filler, filler_host, (size_t)p->m_total * sizeof(double), hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->have_filler = true;
    return OIVA_OK;
}

oiva_status oiva_sweep_take_mix(oiva_sweep* p, oiva_room* room, int g0, oiva_bstft* bstft, void** X_dev) {
    OIVA_NEED(p && room && bstft && X_dev, OIVA_ERR_ARG, "null argument");
    RoomGroupView view;
    std::vector<int> n_out(p->B);
    std::vector<long long> mix_off(p->B);
    int rc = room_group_view(room, g0, &view, n_out.data(), mix_off.data(), p->B);
    if (rc) return rc;
    bool same = view.device == p->device && view.rooms == p->B && view.M == p->M && view.K == p->K;
    for (int b = 0; same && b < p->B; ++b) same = n_out[b] == p->rooms[b].n_out;
    OIVA_NEED(same, OIVA_ERR_ARG, "the group of the room handle is not the one this sweep was made for (device, rooms, M, K, lengths)");
    if ((rc = check_bstft(p, bstft))) return rc;
    DeviceGuard guard(p->device);
    p->room = nullptr, p->last_C = 0;
    for (int b = 0; b < p->B; ++b) p->rooms[b].ref_off = (long long)(p->K + 1) * mix_off[b];
    OIVA_TRY_HIP(hipMemcpyAsync(p->rooms_dev, p->rooms.data(), (size_t)p->B * sizeof(SweepRoom), hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    if ((rc = oiva_bstft_analysis_dev(bstft, view.mix, 1, X_dev))) return rc;      // (the room's calls are synchronous: mix is there)
    p->room = room, p->g0 = g0, p->room_ref = view.ref;
    return OIVA_OK;
}

oiva_status oiva_sweep_evaluate(oiva_sweep* p, oiva_bstft* bstft, const void* Y_dev, int C, int reorder, oiva_bsseval* bsseval,
                                const double* filler_dev) {
    OIVA_NEED(p && bstft && Y_dev && bsseval, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(C >= p->K && C <= p->M, OIVA_ERR_ARG, "Y must hold n_targets..M channels");
    OIVA_NEED(reorder == 0 || reorder == 1, OIVA_ERR_ARG, "reorder must be 0 or 1");
    OIVA_NEED(p->room != nullptr, OIVA_ERR_STATE, "take_mix has not run");
    OIVA_NEED(filler_dev || p->have_filler, OIVA_ERR_STATE, "no filler: call oiva_sweep_set_filler or pass one");
    RoomGroupView view;
    int rc = room_group_view(p->room, p->g0, &view, nullptr, nullptr, 0);      // (STATE: the room handle has moved on to another group)
    if (rc) return rc;
    OIVA_NEED(view.ref == p->room_ref && view.K == p->K, OIVA_ERR_STATE, "the room handle was mixed again since take_mix");
    if ((rc = check_bstft(p, bstft))) return rc;
    BssSignalView sig;
    if ((rc = check_bsseval(p, bsseval, &sig))) return rc;
    DeviceGuard guard(p->device);
    void* y = nullptr;
    if ((rc = oiva_bstft_synthesis_keep(bstft, Y_dev, C, &y))) return rc;
    p->last_C = 0;
    const float* yf = static_cast<const float*>(y);
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[0], p->stream));
    OIVA_TRY_HIP(launch_sweep_std(p->stream, yf, p->rooms_dev, p->B, C, p->max_chunks, p->part, p->std));
    OIVA_TRY_HIP(launch_sweep_order(p->stream, p->std, p->B, C, reorder, p->order));
    OIVA_TRY_HIP(launch_sweep_align(p->stream, yf, p->room_ref, filler_dev ? filler_dev : p->filler, p->order, p->rooms_dev, p->B, C,
                                    p->M, p->K, p->ref_mic, kAlignOffset, p->max_m, sig.est, sig.ref));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[1], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    bsseval_mark_signals(bsseval);
    p->last_C = C;
    return OIVA_OK;
}

oiva_status oiva_sweep_phase_ms(oiva_sweep* p, float* ms) {
    OIVA_NEED(p && ms, OIVA_ERR_ARG, "null argument");
    *ms = 0.f;
    if (!p->last_C) return OIVA_OK;
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipEventElapsedTime(ms, p->stream.events[0], p->stream.events[1]));
    return OIVA_OK;
}

oiva_status oiva_sweep_get_order(oiva_sweep* p, int* order, double* std) {
    OIVA_NEED(p && order && std, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->last_C > 0, OIVA_ERR_STATE, "evaluate has not run");
    DeviceGuard guard(p->device);
    std::vector<int> o((size_t)p->B * kSweepMaxChan);
    std::vector<double> s((size_t)p->B * kSweepMaxChan);
    OIVA_TRY_HIP(hipMemcpy(o.data(), p->order, o.size() * sizeof(int), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(s.data(), p->std, s.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < p->B; ++b)
        for (int c = 0; c < p->last_C; ++c) {
            order[b * p->last_C + c] = o[(size_t)b * kSweepMaxChan + c];
            std[b * p->last_C + c] = s[(size_t)b * kSweepMaxChan + c];
        }
    return OIVA_OK;
}

oiva_status oiva_sweep_get_signals(oiva_sweep* p, oiva_bsseval* bsseval, double* ref_host, double* est_host) {
    OIVA_NEED(p && bsseval && ref_host && est_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->last_C > 0, OIVA_ERR_STATE, "evaluate has not run");
    BssSignalView sig;
    const int rc = check_bsseval(p, bsseval, &sig);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpy(ref_host, sig.ref, (size_t)sig.sig_total * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(est_host, sig.est, (size_t)sig.sig_total * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

}  // extern "C"
