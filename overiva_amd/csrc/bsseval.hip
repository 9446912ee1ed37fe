// C ABI of BSS Eval on the device (oiva_bsseval_*, include/overiva_hip.h): SDR, SIR and SAR of B rooms of N sources, each room of
// its own length, in float64.  Host code only; the kernels live in kernels_bsseval.hip and the algorithm is DESIGN.md 3.10.
//
//   set_signals : packed references and estimates (sum_b N * n_b) float64, host -> device
//   correlate   : lag sums of all rooms -> lag (B, 2N, N, Lf), E (B, N)
//   factor      : G and its copy from the lag sums, Cholesky of the copy and of the N diagonal blocks     } room group by room
//   solve       : C_k = G^-1 D_k and c_kj = G_jj^-1 D_k[j]                                               } group when the two
//   criteria    : the quadratic forms and the three ratios                                               } copies of G do not fit
// The problem table holds one record per room; a dense batch is equal records.  When the two copies of G of all rooms do not fit
// the device (or max_group asks for less) the rooms run in groups through factor, solve and criteria; a room's bits do not depend
// on the grouping, since no kernel's order of operations depends on which rooms it is launched with.  The staged entry points need
// one group; oiva_bsseval_run walks the groups.  Every call is synchronous.
#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {
constexpr int kStages = 4;           // correlate, factor, solve, criteria
constexpr int kMaxVec = kBssMaxSrc * kBssMaxSrc + kBssMaxSrc;
constexpr int kMaxGridZ = 65535;
}  // namespace

struct oiva_bsseval {
    int device = 0;
    int B = 0, N = 0, Lf = 0, diag_only = 0;
    int group = 0;                 // rooms per pass through factor / solve / criteria
    int done = -1;                 // last stage completed on all rooms (staged use), -1: none; signals set: have_sig
    bool have_sig = false, have_result = false;
    long long sig_total = 0, seg_total = 0, part_total = 0;
    HandleStream stream;           // two events: the bracket of oiva_bsseval_time_stages
    DeviceArena mem;               // every buffer below, pooled
    std::vector<BssRoom> rooms;
    BssRoom* rooms_dev = nullptr;
    int2* segs_dev = nullptr;
    double *ref = nullptr, *est = nullptr, *part = nullptr, *Epart = nullptr, *lag = nullptr, *E = nullptr;
    double *G = nullptr, *Gf = nullptr, *Hf = nullptr, *thr = nullptr, *C = nullptr, *c = nullptr, *qL = nullptr, *qS = nullptr;
    double* crit = nullptr;        // sdr, sir, sar: 3 x (B, N, N)
    int* flag = nullptr;
};

namespace {

template <class P>
void take(oiva_bsseval* p, P** out, size_t bytes) {
    p->mem.take(out, std::max<size_t>(bytes, 8), Mem::pooled);
}

// the buffers whose size follows the group: both copies of G, the diagonal blocks, the block sums of the quadratic forms
hipError_t alloc_group(oiva_bsseval* p, int group) {
    const size_t nt = (size_t)p->N * p->Lf, Lf = p->Lf, N = p->N;
    const size_t nrbL = (nt + kBssBlock - 1) / kBssBlock, nrbS = (Lf + kBssBlock - 1) / kBssBlock;
    take(p, &p->G, group * nt * nt * sizeof(double));
    take(p, &p->Gf, group * nt * nt * sizeof(double));
    take(p, &p->Hf, group * N * Lf * Lf * sizeof(double));
    take(p, &p->qL, group * kMaxVec * nrbL * sizeof(double));
    take(p, &p->qS, group * N * kMaxVec * nrbS * sizeof(double));
    return p->mem.status();
}

int stage_correlate(oiva_bsseval* p) {
    OIVA_TRY_HIP(launch_bss_lags(p->stream, p->ref, p->est, p->rooms_dev, p->segs_dev, p->seg_total, p->B, p->N, p->Lf, p->part, p->Epart,
                                 p->lag, p->E));
    return OIVA_OK;
}
int stage_factor(oiva_bsseval* p, int g0, int n) {
    const int nt = p->N * p->Lf;
    OIVA_TRY_HIP(launch_bss_assemble(p->stream, p->lag, p->G, p->Gf, p->Hf, p->thr, p->C, p->c, g0, n, p->N, p->Lf));
    OIVA_TRY_HIP(launch_bss_cholesky(p->stream, p->Gf, n, nt, p->flag, p->thr, g0, 1));
    OIVA_TRY_HIP(launch_bss_cholesky(p->stream, p->Hf, n * p->N, p->Lf, p->flag, p->thr, g0, p->N));
    return OIVA_OK;
}
int stage_solve(oiva_bsseval* p, int g0, int n) {
    const size_t nt = (size_t)p->N * p->Lf;
    OIVA_TRY_HIP(launch_bss_solve(p->stream, p->Gf, n, (int)nt, p->C + (size_t)g0 * p->N * nt, p->N, p->flag, g0, 1));
    OIVA_TRY_HIP(launch_bss_solve(p->stream, p->Hf, n * p->N, p->Lf, p->c + (size_t)g0 * p->N * nt, p->N, p->flag, g0, p->N));
    return OIVA_OK;
}
int stage_criteria(oiva_bsseval* p, int g0, int n) {
    const size_t nn = (size_t)p->B * p->N * p->N;
    OIVA_TRY_HIP(launch_bss_criteria(p->stream, p->lag, p->E, p->G, p->C, p->c, p->qL, p->qS, p->crit, p->crit + nn, p->crit + 2 * nn, g0, n,
                                     p->N, p->Lf, p->diag_only, p->flag));
    return OIVA_OK;
}
// before the first room is factored: nothing flagged, every ratio NaN until its kernel writes it
int reset_results(oiva_bsseval* p) {
    OIVA_TRY_HIP(hipMemsetAsync(p->flag, 0, (size_t)p->B * sizeof(int), p->stream));
    OIVA_TRY_HIP(hipMemsetAsync(p->crit, 0xFF, (size_t)3 * p->B * p->N * p->N * sizeof(double), p->stream));
    return OIVA_OK;
}
int run_stage(oiva_bsseval* p, int stage, int g0, int n) {
    switch (stage) {
        case 0: return stage_correlate(p);
        case 1: return stage_factor(p, g0, n);
        case 2: return stage_solve(p, g0, n);
        default: return stage_criteria(p, g0, n);
    }
}
int read_flags(oiva_bsseval* p, std::vector<int>& st) {
    st.resize(p->B);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(st.data(), p->flag, (size_t)p->B * sizeof(int), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

}  // namespace

// the sweep's view of the handle (sweep.hip): it writes ref and est on the device instead of oiva_bsseval_set_signals
void oiva::bsseval_signal_view(oiva_bsseval* p, BssSignalView* view, int* lengths, int max_rooms) {
    view->device = p->device, view->B = p->B, view->N = p->N, view->Lf = p->Lf;
    view->sig_total = p->sig_total;
    view->ref = p->ref, view->est = p->est;
    for (int b = 0; b < p->B && b < max_rooms; ++b) lengths[b] = p->rooms[b].n;
}
void oiva::bsseval_mark_signals(oiva_bsseval* p) {
    p->have_sig = true;
    p->have_result = false;
    p->done = -1;
}

extern "C" {

oiva_status oiva_bsseval_create(oiva_bsseval** out, int device, int B, const int* n_samples, int N, int filter_length, int diag_only,
                                int max_group, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(n_samples != nullptr, OIVA_ERR_ARG, "null n_samples");
    OIVA_NEED(B >= 1, OIVA_ERR_ARG, "B must be >= 1");
    OIVA_NEED(N >= 1 && N <= kBssMaxSrc, OIVA_ERR_ARG, "bss_eval runs on 1..8 sources");
    OIVA_NEED(filter_length >= 1 && filter_length <= kBssMaxFilter, OIVA_ERR_ARG, "filter_length must be in 1..512");
    OIVA_NEED(max_group >= 0, OIVA_ERR_ARG, "max_group must be >= 0");
    const double lim31 = 2147483648.;
    double segs = 0.;
    for (int b = 0; b < B; ++b) {
        OIVA_NEED(n_samples[b] >= 1, OIVA_ERR_ARG, "room " + std::to_string(b) + " has no samples");
        OIVA_NEED((double)n_samples[b] + kBssSeg + kBssMaxFilter < lim31, OIVA_ERR_ARG, "room " + std::to_string(b) + " is too long");
        segs += (n_samples[b] + kBssSeg - 1) / kBssSeg;
    }
    OIVA_NEED(segs < lim31, OIVA_ERR_ARG, "batch too large");
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);
    oiva_bsseval* p = new oiva_bsseval();
    p->device = p->mem.device = device;
    p->B = B, p->N = N, p->Lf = filter_length, p->diag_only = diag_only ? 1 : 0;
    const size_t per_seg = (size_t)2 * N * N * filter_length;
    p->rooms.resize(B);
    std::vector<int2> segs_host;
    for (int b = 0; b < B; ++b) {
        BssRoom& r = p->rooms[b];
        r.n = n_samples[b];
        r.nseg = (r.n + kBssSeg - 1) / kBssSeg;
        r.sig_off = p->sig_total;
        r.part_off = p->part_total;
        r.seg_off = (int)p->seg_total;
        r.pad = 0;
        p->sig_total += (long long)N * r.n;
        p->part_total += (long long)r.nseg * per_seg;
        p->seg_total += r.nseg;
        for (int g = 0; g < r.nseg; ++g) segs_host.push_back(make_int2(b, g));
    }
    p->mem.note(p->stream.open(stream, 2));
    const size_t nt = (size_t)N * filter_length, nn = (size_t)B * N * N;
    take(p, &p->rooms_dev, (size_t)B * sizeof(BssRoom));
    take(p, &p->segs_dev, segs_host.size() * sizeof(int2));
    take(p, &p->ref, (size_t)p->sig_total * sizeof(double));
    take(p, &p->est, (size_t)p->sig_total * sizeof(double));
    take(p, &p->part, (size_t)p->part_total * sizeof(double));
    take(p, &p->Epart, (size_t)p->seg_total * N * sizeof(double));
    take(p, &p->lag, (size_t)B * per_seg * sizeof(double));
    take(p, &p->E, (size_t)B * N * sizeof(double));
    take(p, &p->thr, (size_t)B * sizeof(double));
    take(p, &p->C, (size_t)B * N * nt * sizeof(double));
    take(p, &p->c, (size_t)B * N * nt * sizeof(double));
    take(p, &p->crit, 3 * nn * sizeof(double));
    take(p, &p->flag, (size_t)B * sizeof(int));
    hipError_t e = p->mem.status();
    if (e == hipSuccess) e = hipMemcpy(p->rooms_dev, p->rooms.data(), (size_t)B * sizeof(BssRoom), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->segs_dev, segs_host.data(), segs_host.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // as many rooms per group as the grid admits and the memory holds: halve until the allocation succeeds
        int group = std::min(B, kMaxGridZ / N);
        if (max_group > 0) group = std::min(group, max_group);
        const size_t keep = p->mem.mark();
        for (;;) {
            e = alloc_group(p, group);
            if (e != hipErrorOutOfMemory || group == 1) break;
            (void)hipGetLastError();
            p->mem.release_to(keep);
            group = (group + 1) / 2;
        }
        p->group = group;
    }
    if (e != hipSuccess) {
        oiva_bsseval_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_bsseval_destroy(oiva_bsseval* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_bsseval_groups(oiva_bsseval* p, int* rooms_per_group) {
    OIVA_NEED(p && rooms_per_group, OIVA_ERR_ARG, "null argument");
    *rooms_per_group = p->group;
    return OIVA_OK;
}

oiva_status oiva_bsseval_set_signals(oiva_bsseval* p, const double* ref_host, const double* est_host) {
    OIVA_NEED(p && ref_host && est_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    const size_t bytes = (size_t)p->sig_total * sizeof(double);
    OIVA_TRY_HIP(hipMemcpyAsync(p->ref, ref_host, bytes, hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipMemcpyAsync(p->est, est_host, bytes, hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->have_sig = true;
    p->have_result = false;
    p->done = -1;
    return OIVA_OK;
}

oiva_status oiva_bsseval_stage(oiva_bsseval* p, int stage) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(stage >= 0 && stage < kStages, OIVA_ERR_ARG, "no such stage");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    OIVA_NEED(stage <= p->done + 1, OIVA_ERR_STATE, "the stages run in order: correlate, factor, solve, criteria");
    OIVA_NEED(stage == 0 || p->group == p->B, OIVA_ERR_STATE,
              "the rooms run in groups of " + std::to_string(p->group) + ": the staged calls need one group, use oiva_bsseval_run");
    DeviceGuard guard(p->device);
    if (stage == 1) {
        const int rc = reset_results(p);
        if (rc) return rc;
    }
    const int rc = run_stage(p, stage, 0, p->B);
    if (rc) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->done = stage;
    p->have_result = stage == kStages - 1;
    return OIVA_OK;
}

oiva_status oiva_bsseval_run(oiva_bsseval* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    DeviceGuard guard(p->device);
    int rc = stage_correlate(p);
    if (rc) return rc;
    rc = reset_results(p);
    if (rc) return rc;
    for (int g0 = 0; g0 < p->B; g0 += p->group) {
        const int n = std::min(p->group, p->B - g0);
        for (int stage = 1; stage < kStages; ++stage) {
            rc = run_stage(p, stage, g0, n);
            if (rc) return rc;
        }
    }
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->done = p->group == p->B ? kStages - 1 : 0;
    p->have_result = true;
    return OIVA_OK;
}

oiva_status oiva_bsseval_get_gram(oiva_bsseval* p, double* G_host, double* D_host, double* E_host) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->done >= (G_host ? 1 : 0), OIVA_ERR_STATE, G_host ? "G is there after factor (one group)" : "correlate has not run");
    DeviceGuard guard(p->device);
    const size_t nt = (size_t)p->N * p->Lf;
    if (G_host) OIVA_TRY_HIP(hipMemcpy(G_host, p->G, (size_t)p->B * nt * nt * sizeof(double), hipMemcpyDeviceToHost));
    if (D_host)
        for (int b = 0; b < p->B; ++b)
            OIVA_TRY_HIP(hipMemcpy(D_host + (size_t)b * p->N * nt, p->lag + ((size_t)b * 2 * p->N + p->N) * nt, p->N * nt * sizeof(double),
                                   hipMemcpyDeviceToHost));
    if (E_host) OIVA_TRY_HIP(hipMemcpy(E_host, p->E, (size_t)p->B * p->N * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_bsseval_get_filters(oiva_bsseval* p, double* C_host, double* c_host) {
    OIVA_NEED(p && C_host && c_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->done >= 2 || p->have_result, OIVA_ERR_STATE, "solve has not run");
    DeviceGuard guard(p->device);
    const size_t bytes = (size_t)p->B * p->N * p->N * p->Lf * sizeof(double);
    OIVA_TRY_HIP(hipMemcpy(C_host, p->C, bytes, hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(c_host, p->c, bytes, hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_bsseval_status(oiva_bsseval* p, int* status) {
    OIVA_NEED(p && status, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->done >= 1 || p->have_result, OIVA_ERR_STATE, "factor has not run");
    DeviceGuard guard(p->device);
    std::vector<int> st;
    const int rc = read_flags(p, st);
    if (rc) return rc;
    std::copy(st.begin(), st.end(), status);
    return OIVA_OK;
}

oiva_status oiva_bsseval_get_criteria(oiva_bsseval* p, double* sdr, double* sir, double* sar) {
    OIVA_NEED(p && sdr && sir && sar, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_result, OIVA_ERR_STATE, "criteria has not run");
    DeviceGuard guard(p->device);
    const size_t nn = (size_t)p->B * p->N * p->N;
    std::vector<int> st;
    const int rc = read_flags(p, st);
    if (rc) return rc;
    OIVA_TRY_HIP(hipMemcpy(sdr, p->crit, nn * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(sir, p->crit + nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(sar, p->crit + 2 * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    std::string which;
    for (int b = 0; b < p->B; ++b)
        if (st[b]) which += (which.empty() ? "" : ", ") + std::to_string(b);
    if (!which.empty())
        return fail_with(OIVA_ERR_NUMERIC, "the Gram matrix of the delayed references is not positive definite to working precision "
                                           "(linearly dependent references) in problem(s) " + which);
    return OIVA_OK;
}

oiva_status oiva_bsseval_time_stages(oiva_bsseval* p, int n, float* per_stage_ms) {
    OIVA_NEED(p && per_stage_ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(n >= 1, OIVA_ERR_ARG, "n must be >= 1");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    DeviceGuard guard(p->device);
    double sum[kStages] = {};
    for (int it = 0; it < n; ++it) {
        int rc = reset_results(p);
        if (rc) return rc;
        for (int g0 = -1; g0 < p->B; g0 = g0 < 0 ? 0 : g0 + p->group) {       // (-1: the one pass over all rooms, correlate)
            const int rooms = std::min(p->group, p->B - std::max(g0, 0));
            for (int stage = g0 < 0 ? 0 : 1; stage < (g0 < 0 ? 1 : kStages); ++stage) {
                float ms = 0.f;
                if ((rc = p->stream.elapsed_ms(0, 1, [&] { return run_stage(p, stage, std::max(g0, 0), rooms); }, &ms))) return rc;
                sum[stage] += ms;
            }
        }
    }
    for (int s = 0; s < kStages; ++s) per_stage_ms[s] = (float)(sum[s] / n);
    p->done = p->group == p->B ? kStages - 1 : 0;
    p->have_result = true;
    return OIVA_OK;
}

}  // extern "C"
