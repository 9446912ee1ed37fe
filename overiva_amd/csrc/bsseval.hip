// C ABI of BSS Eval on the device (include/overiva_hip.h): SDR, SIR and SAR of B rooms of N sources, each room of its own length,
// in float64.  Host code only; the kernels live in kernels_bsseval.hip and the algorithm is DESIGN.md 3.10.  One core (BssCore and
// the functions on it) -- the checks, the room and segment tables, the buffers, the stages, the flags -- and two handles on top:
//
//   oiva_bsseval_* : one set of estimates per set of references.  set_signals, then
//       correlate : lag sums of the references and the estimates in one pass -> rlag, D, E
//       factor    : G and its copy from rlag, Cholesky of the copy and of the N diagonal blocks         } room group by room
//       solve     : C_k = G^-1 D_k and c_kj = G_jj^-1 D_k[j]                                             } group when the two
//       criteria  : the quadratic forms and the three ratios                                             } copies of G do not fit
//     When the two copies of G of all rooms do not fit the device (or max_group asks for less) the rooms run in groups through
//     factor, solve and criteria.  The staged entry points need one group; oiva_bsseval_run walks the groups.
//   oiva_bsssets_* : up to max_sets sets of estimates per set of references, all rooms in one group (a caller short of memory
//     makes handles of fewer rooms).  set_references, set_estimates or take (device to device from an oiva_bsseval), then
//       prepare   : the reference half, once per set of references: rlag, factor
//       evaluate  : the estimate half of sets e0 .. e0 + n - 1 in one set of launches: D and E, solve, criteria
//
// The problem table holds one record per room; a dense batch is equal records.  A room's bits do not depend on the grouping and a
// set's bits not on max_sets, on the sets evaluated with it or on its place among them: no kernel's order of operations depends on
// which rooms or sets it is launched with (bss_arith.h).  Every call is synchronous.
#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {

constexpr int kStages = 4;           // correlate, factor, solve, criteria
constexpr int kPhases = 4;           // prepare; correlate, solve, criteria of the last evaluate
constexpr int kMaxVec = kBssMaxSrc * kBssMaxSrc + kBssMaxSrc;
constexpr int kMaxGrid = 65535;

// B rooms, S sets of estimates, the rooms in groups of `group` through factor, solve and criteria
struct BssCore {
    int device = 0;
    int B = 0, N = 0, Lf = 0, diag_only = 0, S = 0, group = 0;
    long long sig_total = 0, seg_total = 0;
    HandleStream stream;
    DeviceArena mem;               // every buffer below, pooled
    std::vector<BssRoom> rooms;
    BssRoom* rooms_dev = nullptr;
    int2* segs_dev = nullptr;
    // set 0 of sig, lag and Eall: the references (lag: rlag); sets 1 .. S: the estimates (lag: D)
    double *sig = nullptr, *part = nullptr, *Epart = nullptr, *lag = nullptr, *Eall = nullptr;
    double *G = nullptr, *Gf = nullptr, *Hf = nullptr, *thr = nullptr, *C = nullptr, *c = nullptr, *qL = nullptr, *qS = nullptr;
    double* crit = nullptr;        // per set sdr, sir, sar: 3 x (B, N, N)
    int* flag = nullptr;

    size_t nt() const { return (size_t)N * Lf; }
    size_t nn() const { return (size_t)B * N * N; }
    size_t per_set() const { return (size_t)B * N * nt(); }                      // rlag, and D, C and c of one set
    double* est(int e) const { return sig + (size_t)(1 + e) * sig_total; }
    double* D(int e) const { return lag + (1 + e) * per_set(); }
    double* E(int e) const { return Eall + (size_t)(1 + e) * B * N; }
};

// ---- creation: the checks in the order "arguments before the device", the tables, the buffers ---------------------------------
int check_shape(const int* n_samples, int B, int N, int Lf) {
    OIVA_NEED(n_samples != nullptr, OIVA_ERR_ARG, "null n_samples");
    OIVA_NEED(B >= 1, OIVA_ERR_ARG, "B must be >= 1");
    OIVA_NEED(N >= 1 && N <= kBssMaxSrc, OIVA_ERR_ARG, "bss_eval runs on 1..8 sources");
    OIVA_NEED(Lf >= 1 && Lf <= kBssMaxFilter, OIVA_ERR_ARG, "filter_length must be in 1..512");
    return OIVA_OK;
}

int check_rooms(int device, int B, const int* n_samples) {
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
    return OIVA_OK;
}

template <class P>
void take(BssCore& c, P** out, size_t bytes) {
    c.mem.take(out, std::max<size_t>(bytes, 8), Mem::pooled);
}

// everything but the buffers whose size follows the group; a lag pass holds the partial sums of up to part_sets sets
hipError_t setup(BssCore& c, int device, int B, const int* n_samples, int N, int Lf, int diag_only, int S, int part_sets, int n_events,
                 void* stream) {
    c.device = c.mem.device = device;
    c.B = B, c.N = N, c.Lf = Lf, c.diag_only = diag_only ? 1 : 0, c.S = S;
    c.rooms.resize(B);
    std::vector<int2> segs_host;
    for (int b = 0; b < B; ++b) {
        BssRoom& r = c.rooms[b];
        r.n = n_samples[b];
        r.nseg = (r.n + kBssSeg - 1) / kBssSeg;
        r.sig_off = c.sig_total;
        r.seg_off = (int)c.seg_total;
        r.pad = 0;
        c.sig_total += (long long)N * r.n;
        c.seg_total += r.nseg;
        for (int g = 0; g < r.nseg; ++g) segs_host.push_back(make_int2(b, g));
    }
    c.mem.note(c.stream.open(stream, n_events));
    const size_t per_seg = (size_t)N * N * Lf, sets = (size_t)1 + S;
    take(c, &c.rooms_dev, (size_t)B * sizeof(BssRoom));
    take(c, &c.segs_dev, segs_host.size() * sizeof(int2));
    take(c, &c.sig, sets * c.sig_total * sizeof(double));
    take(c, &c.part, (size_t)part_sets * c.seg_total * per_seg * sizeof(double));
    take(c, &c.Epart, (size_t)part_sets * c.seg_total * N * sizeof(double));
    take(c, &c.lag, sets * c.per_set() * sizeof(double));
    take(c, &c.Eall, sets * B * N * sizeof(double));
    take(c, &c.thr, (size_t)B * sizeof(double));
    take(c, &c.C, S * c.per_set() * sizeof(double));
    take(c, &c.c, S * c.per_set() * sizeof(double));
    take(c, &c.crit, S * 3 * c.nn() * sizeof(double));
    take(c, &c.flag, (size_t)B * sizeof(int));
    hipError_t e = c.mem.status();
    if (e == hipSuccess) e = hipMemcpy(c.rooms_dev, c.rooms.data(), (size_t)B * sizeof(BssRoom), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c.segs_dev, segs_host.data(), segs_host.size() * sizeof(int2), hipMemcpyHostToDevice);
    return e;
}

// the buffers whose size follows the group: both copies of G, the diagonal blocks, the block sums of the quadratic forms
hipError_t alloc_group(BssCore& c, int group) {
    const size_t nt = c.nt(), Lf = c.Lf, N = c.N, rows = (size_t)c.S * group;
    const size_t nrbL = (nt + kBssBlock - 1) / kBssBlock, nrbS = (Lf + kBssBlock - 1) / kBssBlock;
    take(c, &c.G, group * nt * nt * sizeof(double));
    take(c, &c.Gf, group * nt * nt * sizeof(double));
    take(c, &c.Hf, group * N * Lf * Lf * sizeof(double));
    take(c, &c.qL, rows * kMaxVec * nrbL * sizeof(double));
    take(c, &c.qS, rows * N * kMaxVec * nrbS * sizeof(double));
    c.group = group;
    return c.mem.status();
}

int alloc_failed(hipError_t e) {
    if (e == hipErrorOutOfMemory) (void)hipGetLastError();
    return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
}

void teardown(BssCore& c) {
    DeviceGuard guard(c.device);
    if (c.stream) (void)hipStreamSynchronize(c.stream);
    c.mem.clear();
    c.stream.close();
}

// ---- the stages, on rooms g0 .. g0 + rooms - 1 and estimate sets e0 .. e0 + n_sets - 1 ------------------------------------------
// lag sums of n_sets signal sets from set s0 on (0: the references, 1 + e: estimate set e), every room
int lags(BssCore& c, int s0, int n_sets) {
    OIVA_TRY_HIP(launch_bss_lags(c.stream, c.sig, c.sig + (size_t)s0 * c.sig_total, c.sig_total, c.rooms_dev, c.segs_dev, c.seg_total, c.B,
                                 n_sets, c.N, c.Lf, c.part, c.Epart, c.lag + s0 * c.per_set(), c.Eall + (size_t)s0 * c.B * c.N));
    return OIVA_OK;
}
int factor(BssCore& c, int g0, int rooms) {
    OIVA_TRY_HIP(launch_bss_assemble(c.stream, c.lag, c.G, c.Gf, c.Hf, c.thr, g0, rooms, c.N, c.Lf));
    OIVA_TRY_HIP(launch_bss_cholesky(c.stream, c.Gf, rooms, (int)c.nt(), c.flag, c.thr, g0, 1));
    OIVA_TRY_HIP(launch_bss_cholesky(c.stream, c.Hf, rooms * c.N, c.Lf, c.flag, c.thr, g0, c.N));
    return OIVA_OK;
}
int solve(BssCore& c, int g0, int rooms, int e0, int n_sets) {
    const size_t at = e0 * c.per_set();
    OIVA_TRY_HIP(launch_bss_solve(c.stream, c.Gf, c.Hf, c.D(e0), c.C + at, c.c + at, g0, rooms, c.B, n_sets, c.N, c.Lf, c.flag));
    return OIVA_OK;
}
int criteria(BssCore& c, int g0, int rooms, int e0, int n_sets) {
    const size_t at = e0 * c.per_set();
    OIVA_TRY_HIP(launch_bss_criteria(c.stream, c.D(e0), c.E(e0), c.G, c.C + at, c.c + at, c.qL, c.qS, c.crit + (size_t)e0 * 3 * c.nn(), g0,
                                     rooms, c.B, n_sets, c.N, c.Lf, c.diag_only, c.flag));
    return OIVA_OK;
}
// before the first room is factored: nothing flagged
int reset_flags(BssCore& c) {
    OIVA_TRY_HIP(hipMemsetAsync(c.flag, 0, (size_t)c.B * sizeof(int), c.stream));
    return OIVA_OK;
}
// every ratio NaN until its kernel writes it
int reset_criteria(BssCore& c, int e0, int n_sets) {
    OIVA_TRY_HIP(hipMemsetAsync(c.crit + (size_t)e0 * 3 * c.nn(), 0xFF, (size_t)n_sets * 3 * c.nn() * sizeof(double), c.stream));
    return OIVA_OK;
}

// ---- reading back ---------------------------------------------------------------------------------------------------------------
int read_flags(BssCore& c, int* st) {
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    OIVA_TRY_HIP(hipMemcpy(st, c.flag, (size_t)c.B * sizeof(int), hipMemcpyDeviceToHost));
    return OIVA_OK;
}
// OIVA_ERR_NUMERIC naming the flagged rooms, OIVA_OK when there is none
int flagged_rooms(BssCore& c) {
    std::vector<int> st(c.B);
    const int rc = read_flags(c, st.data());
    if (rc) return rc;
    std::string which;
    for (int b = 0; b < c.B; ++b)
        if (st[b]) which += (which.empty() ? "" : ", ") + std::to_string(b);
    if (!which.empty())
        return fail_with(OIVA_ERR_NUMERIC, "the Gram matrix of the delayed references is not positive definite to working precision "
                                           "(linearly dependent references) in problem(s) " + which);
    return OIVA_OK;
}
int get_gram(BssCore& c, int e, double* G_host, double* D_host, double* E_host) {
    if (G_host) OIVA_TRY_HIP(hipMemcpy(G_host, c.G, (size_t)c.B * c.nt() * c.nt() * sizeof(double), hipMemcpyDeviceToHost));
    if (D_host) OIVA_TRY_HIP(hipMemcpy(D_host, c.D(e), c.per_set() * sizeof(double), hipMemcpyDeviceToHost));
    if (E_host) OIVA_TRY_HIP(hipMemcpy(E_host, c.E(e), (size_t)c.B * c.N * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}
int get_filters(BssCore& c, int e, double* C_host, double* c_host) {
    OIVA_TRY_HIP(hipMemcpy(C_host, c.C + e * c.per_set(), c.per_set() * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(c_host, c.c + e * c.per_set(), c.per_set() * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

}  // namespace

// =================================================================================================================================
// oiva_bsseval: the core with one set, the rooms in groups
// =================================================================================================================================
struct oiva_bsseval {
    BssCore c;                     // two events: the bracket of oiva_bsseval_time_stages
    int done = -1;                 // last stage completed on all rooms (staged use), -1: none
    bool have_sig = false, have_result = false;
};

namespace {

int run_stage(BssCore& c, int stage, int g0, int rooms) {
    switch (stage) {
        case 0: return lags(c, 0, 2);
        case 1: return factor(c, g0, rooms);
        case 2: return solve(c, g0, rooms, 0, 1);
        default: return criteria(c, g0, rooms, 0, 1);
    }
}
int reset_results(BssCore& c) {
    const int rc = reset_flags(c);
    return rc ? rc : reset_criteria(c, 0, 1);
}

}  // namespace

// the sweep's view of the handle (sweep.hip): it writes ref and est on the device instead of oiva_bsseval_set_signals
void oiva::bsseval_signal_view(oiva_bsseval* p, BssSignalView* view, int* lengths, int max_rooms) {
    const BssCore& c = p->c;
    view->device = c.device, view->B = c.B, view->N = c.N, view->Lf = c.Lf;
    view->sig_total = c.sig_total;
    view->ref = c.sig, view->est = c.est(0);
    for (int b = 0; b < c.B && b < max_rooms; ++b) lengths[b] = c.rooms[b].n;
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
    int rc = check_shape(n_samples, B, N, filter_length);
    if (rc) return rc;
    OIVA_NEED(max_group >= 0, OIVA_ERR_ARG, "max_group must be >= 0");
    if ((rc = check_rooms(device, B, n_samples))) return rc;
    DeviceGuard guard(device);
    oiva_bsseval* p = new oiva_bsseval();
    BssCore& c = p->c;
    hipError_t e = setup(c, device, B, n_samples, N, filter_length, diag_only, 1, 2, 2, stream);
    if (e == hipSuccess) {
        // as many rooms per group as the grid admits and the memory holds: halve until the allocation succeeds
        int group = std::min(B, kMaxGrid / N);
        if (max_group > 0) group = std::min(group, max_group);
        const size_t keep = c.mem.mark();
        for (;;) {
            e = alloc_group(c, group);
            if (e != hipErrorOutOfMemory || group == 1) break;
            (void)hipGetLastError();
            c.mem.release_to(keep);
            group = (group + 1) / 2;
        }
    }
    if (e != hipSuccess) {
        oiva_bsseval_destroy(p);
        return alloc_failed(e);
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_bsseval_destroy(oiva_bsseval* p) {
    if (!p) return OIVA_OK;
    teardown(p->c);
    delete p;
    return OIVA_OK;
}

oiva_status oiva_bsseval_groups(oiva_bsseval* p, int* rooms_per_group) {
    OIVA_NEED(p && rooms_per_group, OIVA_ERR_ARG, "null argument");
    *rooms_per_group = p->c.group;
    return OIVA_OK;
}

oiva_status oiva_bsseval_set_signals(oiva_bsseval* p, const double* ref_host, const double* est_host) {
    OIVA_NEED(p && ref_host && est_host, OIVA_ERR_ARG, "null argument");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    const size_t bytes = (size_t)c.sig_total * sizeof(double);
    OIVA_TRY_HIP(hipMemcpyAsync(c.sig, ref_host, bytes, hipMemcpyHostToDevice, c.stream));
    OIVA_TRY_HIP(hipMemcpyAsync(c.est(0), est_host, bytes, hipMemcpyHostToDevice, c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    bsseval_mark_signals(p);
    return OIVA_OK;
}

oiva_status oiva_bsseval_stage(oiva_bsseval* p, int stage) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(stage >= 0 && stage < kStages, OIVA_ERR_ARG, "no such stage");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    BssCore& c = p->c;
    OIVA_NEED(stage <= p->done + 1, OIVA_ERR_STATE, "the stages run in order: correlate, factor, solve, criteria");
    OIVA_NEED(stage == 0 || c.group == c.B, OIVA_ERR_STATE,
              "the rooms run in groups of " + std::to_string(c.group) + ": the staged calls need one group, use oiva_bsseval_run");
    DeviceGuard guard(c.device);
    int rc = stage == 1 ? reset_results(c) : OIVA_OK;
    if (rc || (rc = run_stage(c, stage, 0, c.B))) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    p->done = stage;
    p->have_result = stage == kStages - 1;
    return OIVA_OK;
}

oiva_status oiva_bsseval_run(oiva_bsseval* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    int rc = run_stage(c, 0, 0, c.B);
    if (rc || (rc = reset_results(c))) return rc;
    for (int g0 = 0; g0 < c.B; g0 += c.group)
        for (int stage = 1; stage < kStages; ++stage)
            if ((rc = run_stage(c, stage, g0, std::min(c.group, c.B - g0)))) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    p->done = c.group == c.B ? kStages - 1 : 0;
    p->have_result = true;
    return OIVA_OK;
}

oiva_status oiva_bsseval_get_gram(oiva_bsseval* p, double* G_host, double* D_host, double* E_host) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->done >= (G_host ? 1 : 0), OIVA_ERR_STATE, G_host ? "G is there after factor (one group)" : "correlate has not run");
    DeviceGuard guard(p->c.device);
    return get_gram(p->c, 0, G_host, D_host, E_host);
}

oiva_status oiva_bsseval_get_filters(oiva_bsseval* p, double* C_host, double* c_host) {
    OIVA_NEED(p && C_host && c_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->done >= 2 || p->have_result, OIVA_ERR_STATE, "solve has not run");
    DeviceGuard guard(p->c.device);
    return get_filters(p->c, 0, C_host, c_host);
}

oiva_status oiva_bsseval_status(oiva_bsseval* p, int* status) {
    OIVA_NEED(p && status, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->done >= 1 || p->have_result, OIVA_ERR_STATE, "factor has not run");
    DeviceGuard guard(p->c.device);
    return read_flags(p->c, status);
}

oiva_status oiva_bsseval_get_criteria(oiva_bsseval* p, double* sdr, double* sir, double* sar) {
    OIVA_NEED(p && sdr && sir && sar, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_result, OIVA_ERR_STATE, "criteria has not run");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    double* const outs[3] = {sdr, sir, sar};
    for (int m = 0; m < 3; ++m) OIVA_TRY_HIP(hipMemcpy(outs[m], c.crit + m * c.nn(), c.nn() * sizeof(double), hipMemcpyDeviceToHost));
    return flagged_rooms(c);
}

oiva_status oiva_bsseval_time_stages(oiva_bsseval* p, int n, float* per_stage_ms) {
    OIVA_NEED(p && per_stage_ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(n >= 1, OIVA_ERR_ARG, "n must be >= 1");
    OIVA_NEED(p->have_sig, OIVA_ERR_STATE, "signals not set");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    double sum[kStages] = {};
    for (int it = 0; it < n; ++it) {
        int rc = reset_results(c);
        if (rc) return rc;
        for (int g0 = -1; g0 < c.B; g0 = g0 < 0 ? 0 : g0 + c.group) {       // (-1: the one pass over all rooms, correlate)
            const int rooms = std::min(c.group, c.B - std::max(g0, 0));
            for (int stage = g0 < 0 ? 0 : 1; stage < (g0 < 0 ? 1 : kStages); ++stage) {
                float ms = 0.f;
                if ((rc = c.stream.elapsed_ms(0, 1, [&] { return run_stage(c, stage, std::max(g0, 0), rooms); }, &ms))) return rc;
                sum[stage] += ms;
            }
        }
    }
    for (int s = 0; s < kStages; ++s) per_stage_ms[s] = (float)(sum[s] / n);
    p->done = c.group == c.B ? kStages - 1 : 0;
    p->have_result = true;
    return OIVA_OK;
}

}  // extern "C"

// =================================================================================================================================
// oiva_bsssets: the core with max_sets sets, all rooms in one group.  It keeps the estimates of every set and partial sums for
// max_sets sets
// =================================================================================================================================
struct oiva_bsssets {
    BssCore c;                     // six events: the bracket of prepare and the four marks of evaluate
    bool have_ref = false, prepared = false;
    std::vector<char> have_est, evaluated;      // per set
    bool timed[kPhases] = {};
    long long preparations = 0, sets_evaluated = 0;
};

namespace {

void new_references(oiva_bsssets* p) {
    p->have_ref = true;
    p->prepared = false;
    std::fill(p->evaluated.begin(), p->evaluated.end(), 0);
}

void new_estimates(oiva_bsssets* p, int e) {
    p->have_est[e] = 1;
    p->evaluated[e] = 0;
}

int check_set(const oiva_bsssets* p, int e) {
    OIVA_NEED(e >= 0 && e < p->c.S, OIVA_ERR_ARG, "set " + std::to_string(e) + " is not in 0.." + std::to_string(p->c.S - 1));
    return OIVA_OK;
}

int check_sets(const oiva_bsssets* p, int e0, int n_sets) {
    OIVA_NEED(e0 >= 0 && n_sets >= 1 && e0 <= p->c.S - n_sets, OIVA_ERR_ARG,
              "sets " + std::to_string(e0) + ".." + std::to_string(e0 + n_sets - 1) + " are not in 0.." + std::to_string(p->c.S - 1));
    return OIVA_OK;
}

}  // namespace

extern "C" {

oiva_status oiva_bsssets_create(oiva_bsssets** out, int device, int B, const int* n_samples, int N, int filter_length, int diag_only,
                                int max_sets, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    int rc = check_shape(n_samples, B, N, filter_length);
    if (rc) return rc;
    OIVA_NEED(max_sets >= 1, OIVA_ERR_ARG, "max_sets must be >= 1");
    OIVA_NEED(max_sets <= kMaxGrid / N, OIVA_ERR_ARG, "max_sets must be <= " + std::to_string(kMaxGrid / N) + " for " + std::to_string(N) + " sources");
    OIVA_NEED(B <= kMaxGrid / N, OIVA_ERR_ARG,
              "one handle holds at most " + std::to_string(kMaxGrid / N) + " rooms of " + std::to_string(N) + " sources");
    if ((rc = check_rooms(device, B, n_samples))) return rc;
    DeviceGuard guard(device);
    oiva_bsssets* p = new oiva_bsssets();
    p->have_est.assign(max_sets, 0);
    p->evaluated.assign(max_sets, 0);
    hipError_t e = setup(p->c, device, B, n_samples, N, filter_length, diag_only, max_sets, max_sets, 6, stream);
    if (e == hipSuccess) e = alloc_group(p->c, B);
    if (e != hipSuccess) {
        oiva_bsssets_destroy(p);
        return alloc_failed(e);
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_bsssets_destroy(oiva_bsssets* p) {
    if (!p) return OIVA_OK;
    teardown(p->c);
    delete p;
    return OIVA_OK;
}

oiva_status oiva_bsssets_set_references(oiva_bsssets* p, const double* ref_host_packed) {
    OIVA_NEED(p && ref_host_packed, OIVA_ERR_ARG, "null argument");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    OIVA_TRY_HIP(hipMemcpyAsync(c.sig, ref_host_packed, (size_t)c.sig_total * sizeof(double), hipMemcpyHostToDevice, c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    new_references(p);
    return OIVA_OK;
}

oiva_status oiva_bsssets_set_estimates(oiva_bsssets* p, int e, const double* est_host_packed) {
    OIVA_NEED(p && est_host_packed, OIVA_ERR_ARG, "null argument");
    const int rc = check_set(p, e);
    if (rc) return rc;
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    OIVA_TRY_HIP(hipMemcpyAsync(c.est(e), est_host_packed, (size_t)c.sig_total * sizeof(double), hipMemcpyHostToDevice, c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    new_estimates(p, e);
    return OIVA_OK;
}

oiva_status oiva_bsssets_take(oiva_bsssets* p, oiva_bsseval* from, int e, int with_references) {
    OIVA_NEED(p && from, OIVA_ERR_ARG, "null argument");
    const int rc = check_set(p, e);
    if (rc) return rc;
    BssCore& c = p->c;
    const BssCore& v = from->c;
    OIVA_NEED(v.device == c.device, OIVA_ERR_ARG,
              "the handles differ in their device: " + std::to_string(v.device) + " against " + std::to_string(c.device));
    OIVA_NEED(v.B == c.B, OIVA_ERR_ARG, "the handles differ in B: " + std::to_string(v.B) + " against " + std::to_string(c.B));
    OIVA_NEED(v.N == c.N, OIVA_ERR_ARG, "the handles differ in N: " + std::to_string(v.N) + " against " + std::to_string(c.N));
    OIVA_NEED(v.Lf == c.Lf, OIVA_ERR_ARG,
              "the handles differ in filter_length: " + std::to_string(v.Lf) + " against " + std::to_string(c.Lf));
    for (int b = 0; b < c.B; ++b)
        OIVA_NEED(v.rooms[b].n == c.rooms[b].n, OIVA_ERR_ARG,
                  "the handles differ in the length of room " + std::to_string(b) + ": " + std::to_string(v.rooms[b].n) + " against " +
                      std::to_string(c.rooms[b].n));
    DeviceGuard guard(c.device);
    const size_t bytes = (size_t)c.sig_total * sizeof(double);
    OIVA_TRY_HIP(hipMemcpyAsync(c.est(e), v.est(0), bytes, hipMemcpyDeviceToDevice, c.stream));
    if (with_references) OIVA_TRY_HIP(hipMemcpyAsync(c.sig, v.sig, bytes, hipMemcpyDeviceToDevice, c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    new_estimates(p, e);
    if (with_references) new_references(p);
    return OIVA_OK;
}

oiva_status oiva_bsssets_prepare(oiva_bsssets* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_ref, OIVA_ERR_STATE, "references not set");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    p->prepared = false;
    p->timed[0] = false;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[0], c.stream));
    int rc = reset_flags(c);
    if (rc || (rc = lags(c, 0, 1)) || (rc = factor(c, 0, c.B))) return rc;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[1], c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    p->prepared = true;
    p->timed[0] = true;
    ++p->preparations;
    return OIVA_OK;
}

oiva_status oiva_bsssets_evaluate(oiva_bsssets* p, int e0, int n_sets) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    int rc = check_sets(p, e0, n_sets);
    if (rc) return rc;
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    for (int e = e0; e < e0 + n_sets; ++e) OIVA_NEED(p->have_est[e], OIVA_ERR_STATE, "the estimates of set " + std::to_string(e) + " are not set");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    for (int i = 1; i < kPhases; ++i) p->timed[i] = false;
    for (int e = e0; e < e0 + n_sets; ++e) p->evaluated[e] = 0;
    if ((rc = reset_criteria(c, e0, n_sets))) return rc;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[2], c.stream));
    if ((rc = lags(c, 1 + e0, n_sets))) return rc;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[3], c.stream));
    if ((rc = solve(c, 0, c.B, e0, n_sets))) return rc;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[4], c.stream));
    if ((rc = criteria(c, 0, c.B, e0, n_sets))) return rc;
    OIVA_TRY_HIP(hipEventRecord(c.stream.events[5], c.stream));
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    for (int e = e0; e < e0 + n_sets; ++e) p->evaluated[e] = 1;
    for (int i = 1; i < kPhases; ++i) p->timed[i] = true;
    p->sets_evaluated += n_sets;
    return OIVA_OK;
}

oiva_status oiva_bsssets_get_criteria(oiva_bsssets* p, int e0, int n_sets, double* sdr, double* sir, double* sar) {
    OIVA_NEED(p && sdr && sir && sar, OIVA_ERR_ARG, "null argument");
    const int rc = check_sets(p, e0, n_sets);
    if (rc) return rc;
    for (int e = e0; e < e0 + n_sets; ++e) OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    const size_t n2 = (size_t)c.N * c.N, nn = c.nn();
    OIVA_TRY_HIP(hipStreamSynchronize(c.stream));
    std::vector<double> host((size_t)n_sets * 3 * nn);
    OIVA_TRY_HIP(hipMemcpy(host.data(), c.crit + (size_t)e0 * 3 * nn, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    double* const outs[3] = {sdr, sir, sar};
    for (int e = 0; e < n_sets; ++e)
        for (int m = 0; m < 3; ++m)
            for (int b = 0; b < c.B; ++b)
                std::copy_n(host.data() + ((size_t)e * 3 + m) * nn + b * n2, n2, outs[m] + ((size_t)b * n_sets + e) * n2);
    return flagged_rooms(c);
}

oiva_status oiva_bsssets_status(oiva_bsssets* p, int* status) {
    OIVA_NEED(p && status, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    DeviceGuard guard(p->c.device);
    return read_flags(p->c, status);
}

oiva_status oiva_bsssets_get_gram(oiva_bsssets* p, int e, double* G_host, double* D_host, double* E_host) {
    OIVA_NEED(p && D_host && E_host, OIVA_ERR_ARG, "null argument");
    const int rc = check_set(p, e);
    if (rc) return rc;
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    DeviceGuard guard(p->c.device);
    return get_gram(p->c, e, G_host, D_host, E_host);
}

oiva_status oiva_bsssets_get_filters(oiva_bsssets* p, int e, double* C_host, double* c_host) {
    OIVA_NEED(p && C_host && c_host, OIVA_ERR_ARG, "null argument");
    const int rc = check_set(p, e);
    if (rc) return rc;
    OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    DeviceGuard guard(p->c.device);
    return get_filters(p->c, e, C_host, c_host);
}

oiva_status oiva_bsssets_counts(oiva_bsssets* p, long long* preparations, long long* sets_evaluated) {
    OIVA_NEED(p && preparations && sets_evaluated, OIVA_ERR_ARG, "null argument");
    *preparations = p->preparations;
    *sets_evaluated = p->sets_evaluated;
    return OIVA_OK;
}

oiva_status oiva_bsssets_phase_ms(oiva_bsssets* p, float* ms) {
    OIVA_NEED(p && ms, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->timed[0] && p->timed[1], OIVA_ERR_STATE, "prepare and evaluate have not both run");
    BssCore& c = p->c;
    DeviceGuard guard(c.device);
    OIVA_TRY_HIP(hipEventElapsedTime(&ms[0], c.stream.events[0], c.stream.events[1]));
    for (int i = 1; i < kPhases; ++i) OIVA_TRY_HIP(hipEventElapsedTime(&ms[i], c.stream.events[i + 1], c.stream.events[i + 2]));
    return OIVA_OK;
}

}  // extern "C"
