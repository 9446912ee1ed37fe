// C ABI of BSS Eval for many estimate sets per reference set (oiva_bsssets_*, include/overiva_hip.h): SDR, SIR and SAR of up to
// max_sets estimate sets of B rooms of N sources against one set of references, in float64.  Host code only; the kernels live in
// kernels_bsssets.hip (and the Cholesky kernels in kernels_bsseval.hip) and the algorithm is DESIGN.md 3.10.
//
//   set_references, set_estimates, take : the packed signals, from the host or device to device from an oiva_bsseval handle
//   prepare   : the reference half, once per set of references: the lag sums r_ij, G and its copy, the Cholesky factor of the copy
//               and of the N diagonal blocks, the flags
//   evaluate  : the estimate half of sets e0 .. e0 + n - 1 in one set of launches: the lag sums D_k and E_k, the right-hand sides,
//               the substitutions, the quadratic forms and the three ratios
// The handle keeps the estimates of every set (not their lag sums) and partial sums for max_sets sets; all rooms are resident at
// once: there is no internal room grouping, a caller short of memory makes handles of fewer rooms.  A set's bits do not depend on
// max_sets, on the sets evaluated with it or on its place among them: the set is an axis of the grid and every chain of
// additions is the one oiva_bsseval runs (bss_arith.h).  Every call is synchronous.
#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {
constexpr int kMaxVec = kBssMaxSrc * kBssMaxSrc + kBssMaxSrc;
constexpr int kMaxGrid = 65535;
constexpr int kPhases = 4;           // prepare; correlate, solve, criteria of the last evaluate
}  // namespace

struct oiva_bsssets {
    int device = 0;
    int B = 0, N = 0, Lf = 0, diag_only = 0, max_sets = 0;
    bool have_ref = false, prepared = false;
    std::vector<char> have_est, evaluated;      // per set
    bool timed[kPhases] = {};
    long long sig_total = 0, seg_total = 0;
    long long preparations = 0, sets_evaluated = 0;
    HandleStream stream;           // six events: the bracket of prepare and the four marks of evaluate
    DeviceArena mem;               // every buffer below, pooled
    std::vector<BssRoom> rooms;
    BssRoom* rooms_dev = nullptr;
    int2* segs_dev = nullptr;
    double *ref = nullptr, *est = nullptr, *part = nullptr, *Epart = nullptr, *rlag = nullptr;
    double *G = nullptr, *Gf = nullptr, *Hf = nullptr, *thr = nullptr;
    double *D = nullptr, *E = nullptr, *C = nullptr, *c = nullptr, *qL = nullptr, *qS = nullptr;
    double* crit = nullptr;        // per set sdr, sir, sar: 3 x (B, N, N)
    int* flag = nullptr;

    size_t nt() const { return (size_t)N * Lf; }
    size_t per_set() const { return (size_t)B * N * nt(); }                      // D, C and c of one set
    size_t nrbL() const { return (nt() + kBssBlock - 1) / kBssBlock; }
    size_t nrbS() const { return ((size_t)Lf + kBssBlock - 1) / kBssBlock; }
};

namespace {

template <class P>
void take(oiva_bsssets* p, P** out, size_t bytes) {
    p->mem.take(out, std::max<size_t>(bytes, 8), Mem::pooled);
}

int read_flags(oiva_bsssets* p, std::vector<int>& st) {
    st.resize(p->B);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(st.data(), p->flag, (size_t)p->B * sizeof(int), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

void new_references(oiva_bsssets* p) {
    p->have_ref = true;
    p->prepared = false;
    std::fill(p->evaluated.begin(), p->evaluated.end(), 0);
}

void new_estimates(oiva_bsssets* p, int e) {
    p->have_est[e] = 1;
    p->evaluated[e] = 0;
}

}  // namespace

extern "C" {

oiva_status oiva_bsssets_create(oiva_bsssets** out, int device, int B, const int* n_samples, int N, int filter_length, int diag_only,
                                int max_sets, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(n_samples != nullptr, OIVA_ERR_ARG, "null n_samples");
    OIVA_NEED(B >= 1, OIVA_ERR_ARG, "B must be >= 1");
    OIVA_NEED(N >= 1 && N <= kBssMaxSrc, OIVA_ERR_ARG, "bss_eval runs on 1..8 sources");
    OIVA_NEED(filter_length >= 1 && filter_length <= kBssMaxFilter, OIVA_ERR_ARG, "filter_length must be in 1..512");
    OIVA_NEED(max_sets >= 1, OIVA_ERR_ARG, "max_sets must be >= 1");
    OIVA_NEED(max_sets <= kMaxGrid / N, OIVA_ERR_ARG, "max_sets must be <= " + std::to_string(kMaxGrid / N) + " for " + std::to_string(N) + " sources");
    OIVA_NEED(B <= kMaxGrid / N, OIVA_ERR_ARG,
              "one handle holds at most " + std::to_string(kMaxGrid / N) + " rooms of " + std::to_string(N) + " sources");
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
    oiva_bsssets* p = new oiva_bsssets();
    p->device = p->mem.device = device;
    p->B = B, p->N = N, p->Lf = filter_length, p->diag_only = diag_only ? 1 : 0, p->max_sets = max_sets;
    p->have_est.assign(max_sets, 0);
    p->evaluated.assign(max_sets, 0);
    p->rooms.resize(B);
    std::vector<int2> segs_host;
    for (int b = 0; b < B; ++b) {
        BssRoom& r = p->rooms[b];
        r.n = n_samples[b];
        r.nseg = (r.n + kBssSeg - 1) / kBssSeg;
        r.sig_off = p->sig_total;
        r.part_off = 0;             // (the partial sums of the sets are indexed by seg_off)
        r.seg_off = (int)p->seg_total;
        r.pad = 0;
        p->sig_total += (long long)N * r.n;
        p->seg_total += r.nseg;
        for (int g = 0; g < r.nseg; ++g) segs_host.push_back(make_int2(b, g));
    }
    p->mem.note(p->stream.open(stream, 6));
    const size_t nt = p->nt(), nn = (size_t)B * N * N, S = (size_t)max_sets, per_seg = (size_t)N * N * filter_length;
    take(p, &p->rooms_dev, (size_t)B * sizeof(BssRoom));
    take(p, &p->segs_dev, segs_host.size() * sizeof(int2));
    take(p, &p->ref, (size_t)p->sig_total * sizeof(double));
    take(p, &p->est, S * p->sig_total * sizeof(double));
    take(p, &p->part, S * p->seg_total * per_seg * sizeof(double));
    take(p, &p->Epart, S * p->seg_total * N * sizeof(double));
    take(p, &p->rlag, (size_t)B * per_seg * sizeof(double));
    take(p, &p->G, (size_t)B * nt * nt * sizeof(double));
    take(p, &p->Gf, (size_t)B * nt * nt * sizeof(double));
    take(p, &p->Hf, (size_t)B * N * filter_length * filter_length * sizeof(double));
    take(p, &p->thr, (size_t)B * sizeof(double));
    take(p, &p->D, S * p->per_set() * sizeof(double));
    take(p, &p->E, S * B * N * sizeof(double));
    take(p, &p->C, S * p->per_set() * sizeof(double));
    take(p, &p->c, S * p->per_set() * sizeof(double));
    take(p, &p->qL, S * B * kMaxVec * p->nrbL() * sizeof(double));
    take(p, &p->qS, S * B * N * kMaxVec * p->nrbS() * sizeof(double));
    take(p, &p->crit, S * 3 * nn * sizeof(double));
    take(p, &p->flag, (size_t)B * sizeof(int));
    hipError_t e = p->mem.status();
    if (e == hipSuccess) e = hipMemcpy(p->rooms_dev, p->rooms.data(), (size_t)B * sizeof(BssRoom), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->segs_dev, segs_host.data(), segs_host.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (e == hipErrorOutOfMemory) (void)hipGetLastError();
        oiva_bsssets_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    *out = p;
    return OIVA_OK;
}

oiva_status oiva_bsssets_destroy(oiva_bsssets* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    p->mem.clear();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

oiva_status oiva_bsssets_set_references(oiva_bsssets* p, const double* ref_host_packed) {
    OIVA_NEED(p && ref_host_packed, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpyAsync(p->ref, ref_host_packed, (size_t)p->sig_total * sizeof(double), hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    new_references(p);
    return OIVA_OK;
}

oiva_status oiva_bsssets_set_estimates(oiva_bsssets* p, int e, const double* est_host_packed) {
    OIVA_NEED(p && est_host_packed, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(e >= 0 && e < p->max_sets, OIVA_ERR_ARG, "set " + std::to_string(e) + " is not in 0.." + std::to_string(p->max_sets - 1));
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpyAsync(p->est + (size_t)e * p->sig_total, est_host_packed, (size_t)p->sig_total * sizeof(double),
                                hipMemcpyHostToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    new_estimates(p, e);
    return OIVA_OK;
}

oiva_status oiva_bsssets_take(oiva_bsssets* p, oiva_bsseval* from, int e, int with_references) {
    OIVA_NEED(p && from, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(e >= 0 && e < p->max_sets, OIVA_ERR_ARG, "set " + std::to_string(e) + " is not in 0.." + std::to_string(p->max_sets - 1));
    BssSignalView v{};
    std::vector<int> lens(p->B, 0);
    bsseval_signal_view(from, &v, lens.data(), p->B);
    OIVA_NEED(v.device == p->device, OIVA_ERR_ARG,
              "the handles differ in their device: " + std::to_string(v.device) + " against " + std::to_string(p->device));
    OIVA_NEED(v.B == p->B, OIVA_ERR_ARG, "the handles differ in B: " + std::to_string(v.B) + " against " + std::to_string(p->B));
    OIVA_NEED(v.N == p->N, OIVA_ERR_ARG, "the handles differ in N: " + std::to_string(v.N) + " against " + std::to_string(p->N));
    OIVA_NEED(v.Lf == p->Lf, OIVA_ERR_ARG,
              "the handles differ in filter_length: " + std::to_string(v.Lf) + " against " + std::to_string(p->Lf));
    for (int b = 0; b < p->B; ++b)
        OIVA_NEED(lens[b] == p->rooms[b].n, OIVA_ERR_ARG,
                  "the handles differ in the length of room " + std::to_string(b) + ": " + std::to_string(lens[b]) + " against " +
                      std::to_string(p->rooms[b].n));
    DeviceGuard guard(p->device);
    const size_t bytes = (size_t)p->sig_total * sizeof(double);
    OIVA_TRY_HIP(hipMemcpyAsync(p->est + (size_t)e * p->sig_total, v.est, bytes, hipMemcpyDeviceToDevice, p->stream));
    if (with_references) OIVA_TRY_HIP(hipMemcpyAsync(p->ref, v.ref, bytes, hipMemcpyDeviceToDevice, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    new_estimates(p, e);
    if (with_references) new_references(p);
    return OIVA_OK;
}

oiva_status oiva_bsssets_prepare(oiva_bsssets* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(p->have_ref, OIVA_ERR_STATE, "references not set");
    DeviceGuard guard(p->device);
    const int nt = (int)p->nt();
    p->prepared = false;
    p->timed[0] = false;
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[0], p->stream));
    OIVA_TRY_HIP(hipMemsetAsync(p->flag, 0, (size_t)p->B * sizeof(int), p->stream));
    OIVA_TRY_HIP(launch_bsssets_lags(p->stream, p->ref, p->ref, 0, p->rooms_dev, p->segs_dev, p->seg_total, p->B, 1, p->N, p->Lf, p->part,
                                     nullptr, p->rlag, nullptr));
    OIVA_TRY_HIP(launch_bsssets_assemble(p->stream, p->rlag, p->G, p->Gf, p->Hf, p->thr, p->B, p->N, p->Lf));
    OIVA_TRY_HIP(launch_bss_cholesky(p->stream, p->Gf, p->B, nt, p->flag, p->thr, 0, 1));
    OIVA_TRY_HIP(launch_bss_cholesky(p->stream, p->Hf, p->B * p->N, p->Lf, p->flag, p->thr, 0, p->N));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[1], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->prepared = true;
    p->timed[0] = true;
    ++p->preparations;
    return OIVA_OK;
}

oiva_status oiva_bsssets_evaluate(oiva_bsssets* p, int e0, int n_sets) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null handle");
    OIVA_NEED(e0 >= 0 && n_sets >= 1 && e0 <= p->max_sets - n_sets, OIVA_ERR_ARG,
              "sets " + std::to_string(e0) + ".." + std::to_string(e0 + n_sets - 1) + " are not in 0.." + std::to_string(p->max_sets - 1));
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    for (int e = e0; e < e0 + n_sets; ++e) OIVA_NEED(p->have_est[e], OIVA_ERR_STATE, "the estimates of set " + std::to_string(e) + " are not set");
    DeviceGuard guard(p->device);
    const size_t set = p->per_set(), nn = (size_t)p->B * p->N * p->N;
    double* D = p->D + e0 * set;
    double* E = p->E + (size_t)e0 * p->B * p->N;
    double* C = p->C + e0 * set;
    double* c = p->c + e0 * set;
    double* crit = p->crit + (size_t)e0 * 3 * nn;
    for (int i = 1; i < kPhases; ++i) p->timed[i] = false;
    for (int e = e0; e < e0 + n_sets; ++e) p->evaluated[e] = 0;
    // every ratio NaN until its kernel writes it
    OIVA_TRY_HIP(hipMemsetAsync(crit, 0xFF, (size_t)n_sets * 3 * nn * sizeof(double), p->stream));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[2], p->stream));
    OIVA_TRY_HIP(launch_bsssets_lags(p->stream, p->ref, p->est + (size_t)e0 * p->sig_total, p->sig_total, p->rooms_dev, p->segs_dev,
                                     p->seg_total, p->B, n_sets, p->N, p->Lf, p->part, p->Epart, D, E));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[3], p->stream));
    OIVA_TRY_HIP(launch_bsssets_solve(p->stream, p->Gf, p->Hf, D, C, c, p->B, n_sets, p->N, p->Lf, p->flag));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[4], p->stream));
    OIVA_TRY_HIP(launch_bsssets_criteria(p->stream, D, E, p->G, C, c, p->qL + (size_t)e0 * p->B * kMaxVec * p->nrbL(),
                                         p->qS + (size_t)e0 * p->B * p->N * kMaxVec * p->nrbS(), crit, p->B, n_sets, p->N, p->Lf,
                                         p->diag_only, p->flag));
    OIVA_TRY_HIP(hipEventRecord(p->stream.events[5], p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    for (int e = e0; e < e0 + n_sets; ++e) p->evaluated[e] = 1;
    for (int i = 1; i < kPhases; ++i) p->timed[i] = true;
    p->sets_evaluated += n_sets;
    return OIVA_OK;
}

oiva_status oiva_bsssets_get_criteria(oiva_bsssets* p, int e0, int n_sets, double* sdr, double* sir, double* sar) {
    OIVA_NEED(p && sdr && sir && sar, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(e0 >= 0 && n_sets >= 1 && e0 <= p->max_sets - n_sets, OIVA_ERR_ARG,
              "sets " + std::to_string(e0) + ".." + std::to_string(e0 + n_sets - 1) + " are not in 0.." + std::to_string(p->max_sets - 1));
    for (int e = e0; e < e0 + n_sets; ++e) OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    DeviceGuard guard(p->device);
    const size_t n2 = (size_t)p->N * p->N, nn = (size_t)p->B * n2;
    std::vector<int> st;
    const int rc = read_flags(p, st);
    if (rc) return rc;
    std::vector<double> host((size_t)n_sets * 3 * nn);
    OIVA_TRY_HIP(hipMemcpy(host.data(), p->crit + (size_t)e0 * 3 * nn, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    double* const outs[3] = {sdr, sir, sar};
    for (int e = 0; e < n_sets; ++e)
        for (int m = 0; m < 3; ++m)
            for (int b = 0; b < p->B; ++b)
                std::copy_n(host.data() + ((size_t)e * 3 + m) * nn + b * n2, n2, outs[m] + ((size_t)b * n_sets + e) * n2);
    std::string which;
    for (int b = 0; b < p->B; ++b)
        if (st[b]) which += (which.empty() ? "" : ", ") + std::to_string(b);
    if (!which.empty())
        return fail_with(OIVA_ERR_NUMERIC, "the Gram matrix of the delayed references is not positive definite to working precision "
                                           "(linearly dependent references) in problem(s) " + which);
    return OIVA_OK;
}

oiva_status oiva_bsssets_status(oiva_bsssets* p, int* status) {
    OIVA_NEED(p && status, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    DeviceGuard guard(p->device);
    std::vector<int> st;
    const int rc = read_flags(p, st);
    if (rc) return rc;
    std::copy(st.begin(), st.end(), status);
    return OIVA_OK;
}

oiva_status oiva_bsssets_get_gram(oiva_bsssets* p, int e, double* G_host, double* D_host, double* E_host) {
    OIVA_NEED(p && D_host && E_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(e >= 0 && e < p->max_sets, OIVA_ERR_ARG, "set " + std::to_string(e) + " is not in 0.." + std::to_string(p->max_sets - 1));
    OIVA_NEED(p->prepared, OIVA_ERR_STATE, "prepare has not run on these references");
    OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    DeviceGuard guard(p->device);
    const size_t nt = p->nt();
    if (G_host) OIVA_TRY_HIP(hipMemcpy(G_host, p->G, (size_t)p->B * nt * nt * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(D_host, p->D + (size_t)e * p->per_set(), p->per_set() * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(E_host, p->E + (size_t)e * p->B * p->N, (size_t)p->B * p->N * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_bsssets_get_filters(oiva_bsssets* p, int e, double* C_host, double* c_host) {
    OIVA_NEED(p && C_host && c_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(e >= 0 && e < p->max_sets, OIVA_ERR_ARG, "set " + std::to_string(e) + " is not in 0.." + std::to_string(p->max_sets - 1));
    OIVA_NEED(p->evaluated[e], OIVA_ERR_STATE, "set " + std::to_string(e) + " has not been evaluated");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipMemcpy(C_host, p->C + (size_t)e * p->per_set(), p->per_set() * sizeof(double), hipMemcpyDeviceToHost));
    OIVA_TRY_HIP(hipMemcpy(c_host, p->c + (size_t)e * p->per_set(), p->per_set() * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
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
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipEventElapsedTime(&ms[0], p->stream.events[0], p->stream.events[1]));
    for (int i = 1; i < kPhases; ++i) OIVA_TRY_HIP(hipEventElapsedTime(&ms[i], p->stream.events[i + 1], p->stream.events[i + 2]));
    return OIVA_OK;
}

}  // extern "C"
