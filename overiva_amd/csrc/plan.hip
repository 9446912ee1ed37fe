// C ABI of liboveriva_hip.so (see include/overiva_hip.h): plan life cycle, prologue, iteration,
// epilogue, measurement and test-only stage access.  Host code only; kernels live in kernels_*.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <mutex>
#include <string>
#include <vector>

#include "host_io.h"
#include "host_util.h"
#include "oiva_internal.h"
#include "resident.h"

using namespace oiva;

namespace {

constexpr int kGraphBatch = 8;       // iterations of the graph captured ahead of time (oiva_plan_use_graph)
constexpr int kGraphMaxIters = 32;   // longest graph captured on demand: an iterate(n) call is ceil(n / 32) replays
constexpr int kGraphCache = 6;       // captured lengths kept per plan

}  // namespace

struct oiva_plan {
    int device = 0;
    int T = 0, F = 0, M = 0, K = 0, model = 0, F_total = 0;
    HandleStream stream;        // two events: the bracket of the timers
    DeviceArena mem;            // every device and pinned buffer below (X_owned, Y and io_c128 pooled)

    const float2* X = nullptr;  // (T,F,M)
    float2* X_owned = nullptr;
    float2* X_pad = nullptr;    // (T, F, M + 1): X with a zero channel behind every bin's M, for the vector-ALU covariance kernels at 9/11/13/15 channels
    float2* What = nullptr;     // (F,M,M) complex64: what the streaming kernels read
    double2* What64 = nullptr;  // (F,M,M) complex128: carried between iterations by the float64 update
    bool what64_valid = false;
    double* Cx = nullptr;       // [F][M*M] packed, / T
    void* Vpart = nullptr;      // [nsplit][F][K][M*M] packed partial sums, float32 or float64 (cov_f64())
    float* Ppart = nullptr;     // [nb (or more, zero padded)][T][K]
    int ppart_alloc = 0;
    float* Plocal = nullptr;    // (T,K)
    void* Wwide = nullptr;      // 17..32 channels: (T, K) float64 final weights of the covariance pass
    float* R = nullptr;         // (T,K)
    float* wscale = nullptr;    // (K)
    float* Spart = nullptr;     // [nsplit][F][K][3]
    float2* Y = nullptr;        // (T,F,K), allocated on first demix
    double2* scratch_c = nullptr;  // K*F*M*M complex128, for getters
    double* scratch_p = nullptr;   // K*F*M*M packed float64, for getters

    CovGeom cov{};
    bool cov_quad_on = true;      // oiva_plan_set_cov_quad
    bool cov_hmfma_on = true;     // oiva_plan_set_cov_hmfma ($OIVA_COV_HMFMA=0: off)
    bool fuse_cov_update = false; // oiva_plan_set_fuse_cov_update ($OIVA_COV_UPDATE=1: on wherever the shape qualifies)
    int power_reverse = 1;        // oiva_plan_set_power_reverse ($OIVA_POWER_REVERSE=0: off): the power pass walks X against the covariance pass; 2: and takes its chunks tail first even in a grid of one round
    int pow_splits_req = 0;                       // oiva_plan_set_pow_splits (0: the rule's own count), kept for the choices that follow it
    double x_resident_mb = kXResidentDefaultMB;   // oiva_plan_set_x_resident_mb ($OIVA_X_RESIDENT_MB; <= 0: off): how much of X the two streaming passes keep in the Infinity Cache (XPolicy, kernel_choice.h)
    bool cov_rows_on = true;                      // oiva_plan_set_cov_rows ($OIVA_COV_ROWS=0: off): where the policy of X streams, the covariance pass runs its row instantiation (cov_rows_form, kernel_choice.h)
    CovGeom stg{};              // geometry of the projection-back statistics pass (16-bin groups, independent of cov)
    PowGeom pw{};
    int n_cu = 256;
    int vpart_splits_alloc = 0;

    bool have_x = false, have_cx = false, have_w = false;
    bool pad_valid = false;       // X_pad holds the current X
    bool wscale_pending = false;  // wscale computed (by the covariance pass), update not yet applied
    int raw_weights = 0;          // test hook: R holds final 1/weights, no gamma normalisation
    int prec = 0;                 // OIVA_PREC_* bits (oiva_plan_set_precision)
    bool upd_f64() const { return prec & OIVA_PREC_UPDATE_F64; }
    bool cov_f64() const { return prec & OIVA_PREC_COV_F64; }
    // element type of the covariance partials: the vector-ALU kernels always sum their float32 lane chains across lanes in
    // float64 and store float64 partials; the 9..16-channel matrix-core kernel stores its accumulator type (CovTraits::partials)
    bool vpart_f64() const { return partials_f64(cov, cov_f64()); }
    int use_graph = 0;
    // OGIVE (ive.py): per-bin state, allocated by oiva_plan_ogive_begin
    OgiveState og{};
    bool og_ready = false;
    int og_mode = 0, og_model = 0;
    // captured chunk of OGIVE epochs (five launches per epoch are latency bound on the reference's problem sizes)
    hipGraphExec_t og_graph = nullptr;
    int og_graph_n = 0, og_graph_phase = -1;
    double og_graph_mu = 0., og_graph_tol = 0.;
    // X-resident iteration (resident.h): geometry, exchange buffers, epoch of the last launch
    ResidentGeom rg{};
    bool res_ok = false;           // the shape qualifies
    bool res_on = false;
    void* res_block = nullptr;     // one allocation: parts | vpart | rsum | wpub | flags | ctrl | stamps
    float* res_parts = nullptr;
    float* res_psum = nullptr;
    double* res_vpart = nullptr;
    double* res_rsum = nullptr;
    float2* res_wpub = nullptr;
    unsigned* res_flags = nullptr; // ctrl words ([0] give-up code)
    float2* res_what = nullptr;    // second copies of W_hat / its complex128 form: a launch writes its final state there, and the
    double2* res_what64 = nullptr; //   plan swaps them with What / What64 when nobody gave up (own allocations)
    unsigned* res_code_host = nullptr;   // pinned: the give-up code of a launch, copied behind it on the stream
    unsigned long long* res_stamps = nullptr;
    size_t res_block_bytes = 0;
    unsigned res_epoch = 0;
    int res_last_code = 0, res_launches = 0, res_fallbacks = 0, res_stamped = 0;
    int res_timeout_ms = 0, res_stall = -1, res_stall_iter = 0;
    char* res_loop_buf = nullptr;  // loop-back: this plan plays all res_world ranks on one GPU (oiva_plan_resident_loopback)
    bool res_loopback = false;
    bool res_trace = false;        // timestamps of every workgroup (oiva_plan_resident_trace)
    unsigned long long* res_trace_buf = nullptr;
    int res_trace_iters = 0;
    char* res_gath[OIVA_XCHG_MAX_RANKS] = {};   // every rank's gather buffer (bins sharded over GPUs), else unused
    int res_rank = 0, res_world = 1;
    // exchange of the ranks' partial powers inside the activation kernel of the four-launch path (oiva_plan_fused_connect)
    bool fx_on = false, fx_loopback = false;
    char* fx_gath[OIVA_XCHG_MAX_RANKS] = {};
    int fx_rank = 0, fx_world = 1;
    int fx_nblk_own = 1, fx_nblk_peer = 1;      // block sums this rank forms / words per other rank's slot
    char* fx_loop_buf = nullptr;                // loop-back: this plan's own gather buffer
    unsigned* fx_state = nullptr;               // [0] give-up flag, [16 ...] one epoch counter per workgroup of the activation kernel
    unsigned* fx_flag_host = nullptr;           // pinned: fx_state[0] as copied behind the work on the plan's stream (check_fused)
    int fx_timeout_ms = 0, fx_stall = 0;
    // hand-over of Y to a host array in slabs of frames (demix_to_host): a second stream for the device-to-host copies, one
    // event pair per slot of the pinned ring, a device staging ring for complex128 output
    HandleStream io_stream;                     // untimed events: [s] slab written, [kHostRingSlots + s] slab copied, per slot s
    double2* io_c128[kHostRingSlots] = {};
    size_t io_c128_bytes = 0;                   // of each slot (all three or none)
    size_t io_slab_bytes = 0;                   // oiva_plan_set_io_slab (0: 8 MB)
    float2* ck_what = nullptr;                  // oiva_plan_save_w: a copy of W_hat (and of its complex128 form) on the device
    double2* ck_what64 = nullptr;
    bool ck_valid = false, ck_what64_valid = false;
    GraphCache graphs{kGraphCache};             // by iterations per replay
};

namespace {

// what the choice of the two streaming passes depends on (kernel_choice.h).  $OIVA_HMFMA_PART32 is read at every choice,
// $OIVA_COV_KC_WIDE and $OIVA_POWER_LDS once per process.
ChoiceIn choice_in(const oiva_plan* p) {
    static const bool kc_wide = [] { const char* v = std::getenv("OIVA_COV_KC_WIDE"); return !(v && v[0] == '0'); }();
    static const bool power_lds = [] { const char* v = std::getenv("OIVA_POWER_LDS"); return !(v && v[0] == '0'); }();
    const char* pv = std::getenv("OIVA_HMFMA_PART32");
    ChoiceIn c{};
    c.T = p->T, c.F = p->F, c.F_total = p->F_total, c.M = p->M, c.K = p->K, c.n_cu = p->n_cu;
    c.cov_f64 = p->cov_f64(), c.upd_f64 = p->upd_f64();
    c.cov_quad_on = p->cov_quad_on, c.cov_hmfma_on = p->cov_hmfma_on;
    c.part32 = pv && pv[0] == '1';
    c.kc_wide = kc_wide, c.power_lds = power_lds;
    c.x_resident_mb = p->x_resident_mb;
    return c;
}
// the device's answers (< 1: the query failed); asked[0] / asked[1] (may be nullptr) receive what each query returned
Occupancy device_occupancy(int* asked = nullptr) {
    Occupancy o;
    o.cov_blocks_per_cu = [asked](int M, int kc, bool f64) {
        int n = 0;
        if (cov_blocks_per_cu(M, kc, f64, &n) != hipSuccess) n = 0;
        if (asked) asked[0] = n;
        return n;
    };
    o.pow_blocks_per_cu = [asked](int M, int kp, int tcp) {
        int n = 0;
        if (pow_blocks_per_cu(M, kp, tcp, &n) != hipSuccess) n = 0;
        if (asked) asked[1] = n;
        return n;
    };
    return o;
}
void choose_cov_geom(oiva_plan* p, int nsplit_req) { p->cov = choose_cov(choice_in(p), device_occupancy(), nsplit_req); }
void choose_pow_geom(oiva_plan* p, int nsplit_req) {
    p->pow_splits_req = nsplit_req;
    p->pw = choose_pow(choice_in(p), device_occupancy(), nsplit_req);
}

void choose_stats_geom(oiva_plan* p) {
    CovGeom g;
    if (p->M > kNarrowMax) {
        // 17..32 channels: frame splits counted on F_total (as the covariance's above: the same partial sums on every rank)
        g.nbg = ceil_div(p->F_total, 64);
        g.kc = 2;
        const int nsplit = std::min(16, pick_splits(p->n_cu * 4, g.nbg * ceil_div(p->K, g.kc), p->T, 128));
        g.tc = round_up(ceil_div(p->T, nsplit), 16);
        g.nsplit = ceil_div(p->T, g.tc);
        p->stg = g;
        return;
    }
    p->stg = stats_geom(p->T, p->F, p->K, p->n_cu);
}

int drop_graph(oiva_plan* p) {
    const int rc = p->graphs.clear();
    if (rc) return rc;
    if (p->og_graph) {
        OIVA_TRY_HIP(hipGraphExecDestroy(p->og_graph));
        p->og_graph = nullptr;
    }
    return OIVA_OK;
}

size_t vpart_floats(const oiva_plan* p, int nsplit) { return (size_t)nsplit * p->F * p->K * p->M * p->M; }

int ensure_vpart(oiva_plan* p) {
    if (p->cov.nsplit > p->vpart_splits_alloc) {
        p->mem.release(&p->Vpart);
        OIVA_TRY_HIP(p->mem.take_one(&p->Vpart, (vpart_floats(p, p->cov.nsplit) + 2) * sizeof(double)));   // either element type; sum_vpart reads idx + 1
        p->vpart_splits_alloc = p->cov.nsplit;
    }
    return OIVA_OK;
}

// the load policy of X for the geometry of THIS launch (the setters of splits and precision change it after plan creation)
XPolicy x_policy(const oiva_plan* p) { return choose_x_policy(p->x_resident_mb, p->T, p->F, p->M, p->cov_f64(), p->cov, p->pw); }
CovGeom cov_geom_now(const oiva_plan* p) {
    CovGeom g = p->cov;
    const XPolicy x = x_policy(p);
    g.xplain = x.xplain();
    g.rows = cov_rows_form(x, p->cov_rows_on) ? 1 : 0;
    return g;
}

// ---- the five stages of one iteration -----------------------------------------------------------
int stage_power(oiva_plan* p) {
    // the order and the load policy follow the covariance geometry of THIS launch (oiva_plan_set_cov_splits and the precision
    // change it after the power geometry was chosen)
    PowGeom g = p->pw;
    g.xplain = x_policy(p).xplain();
    g.xctc = p->cov.tc;
    if (p->power_reverse) {
        g.rev = 1;
        // which chunk a row takes only matters when the rows do not all run at once; in one round the order table measured
        // as a loss on the 1024-bin shard
        if (g.rounds > 1 || p->power_reverse > 1) g.ord = make_pow_order(g.nsplit, g.tcp, p->cov.nsplit, p->cov.tc);
    }
    OIVA_TRY_HIP(launch_power(p->stream, p->X, p->X_pad && p->pad_valid ? p->X_pad : nullptr, p->What, p->Ppart, p->T, p->F, p->M, p->K, g));
    return OIVA_OK;
}
int stage_activation(oiva_plan* p, const float* parts, int nparts) {
    if (p->fx_on && parts == p->Ppart) {
        // bins sharded over GPUs, the ranks' sums exchanged by the activation kernel itself (no collective, no host in the loop)
        OIVA_TRY_HIP(launch_activation_xchg(p->stream, parts, nparts, p->fx_gath, p->fx_rank, p->fx_world, p->fx_loopback ? (p->fx_stall ? 2 : 1) : 0, p->fx_nblk_own, p->fx_nblk_peer, p->fx_state + 16,
                                       p->fx_state, (long long)(p->fx_timeout_ms > 0 ? p->fx_timeout_ms : 2000) * 100000, p->R, p->T, p->K,
                                       p->model, p->F_total));
        p->raw_weights = 0;
        return OIVA_OK;
    }
    OIVA_TRY_HIP(launch_activation(p->stream, parts, nparts, p->R, p->T, p->K, p->model, p->F_total));
    p->raw_weights = 0;
    return OIVA_OK;
}
int stage_cov(oiva_plan* p) {
    OIVA_TRY_HIP(launch_cov(p->stream, p->X, p->X_pad, p->R, p->Wwide ? static_cast<float*>(p->Wwide) : p->Plocal /* weights scratch, (T,16) */, p->wscale, p->model,
                       p->raw_weights, p->Vpart, p->cov_f64(), p->T, p->F, p->M, p->K, cov_geom_now(p)));
    p->wscale_pending = !p->raw_weights;
    return OIVA_OK;
}
int stage_update(oiva_plan* p, bool init_only) {
    UpdateArgs a;
    a.What = p->What;
    a.What64 = p->upd_f64() ? p->What64 : nullptr;
    a.Cx = p->Cx;
    a.Vpart = p->Vpart;
    a.vpart_f64 = p->vpart_f64() ? 1 : 0;
    a.wscale = (!init_only && p->wscale_pending) ? p->wscale : nullptr;
    a.nsplit = p->cov.nsplit;
    a.T = p->T;
    a.F = p->F;
    a.M = p->M;
    a.K = p->K;
    a.init_only = init_only ? 1 : 0;
    a.use_double = p->upd_f64() ? 1 : 0;
    a.layout = (p->prec & OIVA_PREC_UPDATE_ROWS) ? 1 : 0;
    OIVA_TRY_HIP(launch_update(p->stream, a));
    p->what64_valid = a.What64 != nullptr;      // the float32 variants leave the complex128 copy behind
    if (!init_only) p->wscale_pending = false;
    return OIVA_OK;
}

// covariance and per-bin update as one launch (kernels_cov_update.hip) where the plan's geometry is the kernel's: the headline
// shape and its neighbours (8 channels, 2 sources, four frame splits)
bool cov_update_applies(const oiva_plan* p) {
    return traits(p->cov.kind).fusable && p->fuse_cov_update && !p->cov_f64() && !p->raw_weights && !(p->prec & OIVA_PREC_UPDATE_ROWS) && p->K < p->M &&
           cov_update_supported(p->M, p->K, p->T, p->F, p->cov.nsplit, p->cov.tc);
}
int stage_cov_update(oiva_plan* p) {
    UpdateArgs a;
    a.What = p->What;
    a.What64 = p->upd_f64() ? p->What64 : nullptr;
    a.Cx = p->Cx;
    a.Vpart = nullptr;
    a.vpart_f64 = 1;
    a.wscale = nullptr;
    a.nsplit = p->cov.nsplit;
    a.T = p->T, a.F = p->F, a.M = p->M, a.K = p->K;
    a.init_only = 0;
    a.use_double = p->upd_f64() ? 1 : 0;
    a.layout = 0;
    OIVA_TRY_HIP(launch_cov_update(p->stream, p->X, p->R, p->wscale, p->model, a, p->cov.tc));
    p->what64_valid = a.What64 != nullptr;
    p->wscale_pending = false;
    return OIVA_OK;
}

int one_iteration(oiva_plan* p) {
    int rc;
    if ((rc = stage_power(p))) return rc;
    if ((rc = stage_activation(p, p->Ppart, p->pw.nb))) return rc;
    if (cov_update_applies(p)) return stage_cov_update(p);
    if ((rc = stage_cov(p))) return rc;
    return stage_update(p, false);
}

// ---- X-resident iteration (resident.h) -------------------------------------------------------------
constexpr int kResidentStampIters = 256;

bool resident_applies(const oiva_plan* p) {
    // (the float64 covariance of `precise` exists in the kernel for 4 channels: 32 float64 accumulators per lane)
    const bool arith_ok = !p->cov_f64() || (p->M == 4 && p->upd_f64());
    return p->M <= kNarrowMax && p->res_on && p->res_ok && (p->F == p->F_total || p->res_world > 1) && arith_ok && !p->raw_weights && !p->wscale_pending;
}

int resident_alloc(oiva_plan* p) {
    if (p->res_block) return OIVA_OK;
    const ResidentGeom& g = p->rg;
    const size_t Fp = (size_t)g.NB * 16, NA = (size_t)p->M * p->M, K = p->K;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_parts = up((size_t)2 * g.NB * g.NS * g.TW * K * sizeof(float));
    const size_t b_psum = up((size_t)2 * g.NS * g.TW * K * sizeof(float));
    const size_t b_vpart = up(((size_t)g.NS * Fp * K * NA + 2) * sizeof(double));
    const size_t b_rsum = up((size_t)g.NB * ((g.NS * K + 1) & ~(size_t)1) * sizeof(double) + 16);      // rows of an even number of words
    const size_t b_wpub = up(Fp * K * p->M * sizeof(float2));
    const size_t b_flags = up((16 + (size_t)g.NB * g.NS) * sizeof(unsigned));      // ctrl words, then the XCD table
    const size_t b_stamps = up((size_t)kResidentStampIters * kResidentStamps * sizeof(unsigned long long));
    const size_t total = b_parts + b_psum + b_vpart + b_rsum + b_wpub + b_flags + b_stamps;
    if (!p->res_what) OIVA_TRY_HIP(p->mem.take_one(&p->res_what, (size_t)p->F * NA * sizeof(float2)));
    if (!p->res_what64) OIVA_TRY_HIP(p->mem.take_one(&p->res_what64, (size_t)p->F * NA * sizeof(double2)));
    if (!p->res_code_host) OIVA_TRY_HIP(p->mem.take_one(&p->res_code_host, sizeof(unsigned), Mem::pinned));
    OIVA_TRY_HIP(p->mem.take_one(&p->res_block, total));
    OIVA_TRY_HIP(hipMemsetAsync(p->res_block, 0, total, p->stream));
    char* c = static_cast<char*>(p->res_block);
    p->res_parts = reinterpret_cast<float*>(c);
    c += b_parts;
    p->res_psum = reinterpret_cast<float*>(c);
    c += b_psum;
    p->res_vpart = reinterpret_cast<double*>(c);
    c += b_vpart;
    p->res_rsum = reinterpret_cast<double*>(c);
    c += b_rsum;
    p->res_wpub = reinterpret_cast<float2*>(c);
    c += b_wpub;
    p->res_flags = reinterpret_cast<unsigned*>(c);
    c += b_flags;
    p->res_stamps = reinterpret_cast<unsigned long long*>(c);
    p->res_block_bytes = total;
    p->res_epoch = 0;
    return OIVA_OK;
}

// n iterations in one persistent launch.  Synchronous.  *ran = false when the launch gave up (nothing changed):
// the caller then runs the four-launch path.
int run_resident(oiva_plan* p, int n, bool* ran) {
    *ran = false;
    int rc = resident_alloc(p);
    if (rc) return rc;
    const ResidentGeom& g = p->rg;
    ResidentArgs a{};
    a.X = p->X;
    a.What = p->What;
    a.What64 = p->upd_f64() ? p->What64 : nullptr;
    a.What_out = p->res_what;
    a.What64_out = p->upd_f64() ? p->res_what64 : nullptr;
    a.what64_valid = p->what64_valid ? 1 : 0;
    a.Cx = p->Cx;
    a.parts = p->res_parts;
    a.psum = p->res_psum;
    a.vpart = p->res_vpart;
    a.rsum = p->res_rsum;
    a.wpub = p->res_wpub;
    a.ctrl = p->res_flags;
    a.xcc_tab = p->res_flags + 16;
    a.stamps = n <= kResidentStampIters ? p->res_stamps : nullptr;
    a.stamp_all = 0;
    if (p->res_trace && n <= 64) {
        const size_t bytes = (size_t)g.NB * g.NS * n * kResidentStamps * sizeof(unsigned long long);
        p->mem.release(&p->res_trace_buf);
        OIVA_TRY_HIP(p->mem.take_one(&p->res_trace_buf, bytes));
        OIVA_TRY_HIP(hipMemsetAsync(p->res_trace_buf, 0, bytes, p->stream));
        a.stamps = p->res_trace_buf;
        a.stamp_all = 1;
        p->res_trace_iters = n;
    }
    a.T = p->T;
    a.F = p->F;
    a.F_total = p->F_total;
    a.model = p->model;
    a.g = g;
    a.n_iter = n;
    a.epoch0 = p->res_epoch;
    a.timeout_ticks = (long long)(p->res_timeout_ms > 0 ? p->res_timeout_ms : (p->res_world > 1 && !p->res_loopback ? 2000 : 250)) * 100000;   // 100 MHz clock; an iteration takes tens of microseconds (other ranks may start late: 2 s)
    a.stall_block = p->res_stall;
    a.stall_iter = p->res_stall_iter;
    a.rank = p->res_rank;
    a.world = p->res_world;
    a.loopback = p->res_loopback ? 1 : 0;
    for (int r = 0; r < OIVA_XCHG_MAX_RANKS; ++r) a.gath[r] = reinterpret_cast<float*>(p->res_gath[r]);
    OIVA_TRY_HIP(launch_resident(p->stream, a, p->M, p->K, p->upd_f64(), p->cov_f64()));
    p->res_launches++;
    OIVA_TRY_HIP(hipMemcpyAsync(p->res_code_host, a.ctrl, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));   // (pinned: one wait for both)
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    const unsigned code = *p->res_code_host;
    if (code != 0) {
        // some wait ran into its time-out (workgroups not co-resident, or the test hook): whatever the workgroups that did
        // finish wrote went to the staging copy, W_hat itself is untouched.
        // Clear the flags, start the epochs over and stay on the four-launch path from here on.
        OIVA_TRY_HIP(hipMemset(p->res_block, 0, p->res_block_bytes));
        p->res_epoch = 0;
        p->res_last_code = (int)code;
        p->res_fallbacks++;
        p->res_on = false;
        p->res_stamped = 0;
        if (p->res_world > 1)      // the other ranks' state is unknown: no silent fall-back, the caller has to decide for all of them
            return fail_with(OIVA_ERR_STATE, "the X-resident launch gave up waiting (code " + std::to_string(code) +
                                        "): a rank did not deliver its parts in time; W_hat of this rank is unchanged");
        return OIVA_OK;
    }
    // nobody gave up: the staged W_hat becomes the state -- the buffers change places (captured graphs of the four-launch path
    // hold the old addresses: dropped, they are rebuilt if that path is ever used)
    if (!p->graphs.empty() || p->og_graph) {
        int rcg = drop_graph(p);
        if (rcg) return rcg;
    }
    std::swap(p->What, p->res_what);
    if (a.What64_out) std::swap(p->What64, p->res_what64);
    p->og.What = p->What;
    p->og.What64 = p->What64;
    p->res_epoch += (unsigned)n;
    p->res_stamped = (a.stamps && !a.stamp_all) ? n : 0;
    p->what64_valid = a.What64 != nullptr;      // the float32 update leaves the complex128 copy behind
    p->wscale_pending = false;
    *ran = true;
    return OIVA_OK;
}

// The executable graph of `iters` iterations (stream capture records, it does not execute): taken from the plan's cache or
// captured, instantiated and uploaded now.  An iterate(n) call replays ONE graph of n iterations (n <= 32; else 32 at a time):
// a replay costs 10-16 us of which little hides behind the previous one, so the 20 steps of the driver's bench line as
// 8 + 8 + 1 + 1 + 1 + 1 (rounds 1-4) ran 4.7 us per iteration above the steady state of the same kernels (205.1 against 200.4
// us).  oiva_plan_use_graph captures the 8-iteration graph ahead of time, so that short calls never capture inside a
// caller's timed region; other lengths are captured by the first call that asks for them (0.1-0.4 ms) and kept.
int graph_for(oiva_plan* p, int iters, hipGraphExec_t* out) {
    return p->graphs.get(p->stream, iters, [&] {
        const bool pending = p->wscale_pending;
        const int raw = p->raw_weights;
        int r = OIVA_OK;
        for (int i = 0; i < iters && r == OIVA_OK; ++i) r = one_iteration(p);
        p->wscale_pending = pending;   // capturing toggled the host-side flags without running anything
        p->raw_weights = raw;
        return r;
    }, out);
}

int build_graphs(oiva_plan* p) {
    hipGraphExec_t g = nullptr;
    return graph_for(p, kGraphBatch, &g);
}

// W_hat lives twice on the device: complex64 for the streaming kernels, complex128 for the float64 update
int upload_what(oiva_plan* p, const std::vector<double2>& wh) {
    std::vector<float2> w32(wh.size());
    for (size_t i = 0; i < wh.size(); ++i) w32[i] = make_float2((float)wh[i].x, (float)wh[i].y);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(p->What, w32.data(), w32.size() * sizeof(float2), hipMemcpyHostToDevice));
    OIVA_TRY_HIP(hipMemcpy(p->What64, wh.data(), wh.size() * sizeof(double2), hipMemcpyHostToDevice));
    p->what64_valid = true;
    return OIVA_OK;
}

// the current W_hat in float64: the complex128 copy when the float64 update maintains it, else the complex64 one
int download_what(oiva_plan* p, std::vector<double2>& wh) {
    wh.resize((size_t)p->F * p->M * p->M);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    if (p->what64_valid) {
        OIVA_TRY_HIP(hipMemcpy(wh.data(), p->What64, wh.size() * sizeof(double2), hipMemcpyDeviceToHost));
        return OIVA_OK;
    }
    std::vector<float2> w32(wh.size());
    OIVA_TRY_HIP(hipMemcpy(w32.data(), p->What, w32.size() * sizeof(float2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < wh.size(); ++i) wh[i] = make_double2(w32[i].x, w32[i].y);
    return OIVA_OK;
}

// the padded copy of X the vector-ALU covariance kernels read at 9 / 11 / 13 / 15 channels
int ensure_pad(oiva_plan* p) {
    if (p->X_pad == nullptr || p->pad_valid) return OIVA_OK;
    OIVA_TRY_HIP(launch_pad_channels(p->stream, p->X, p->X_pad, (long long)p->T * p->F, p->M));
    p->pad_valid = true;
    return OIVA_OK;
}

int check_ready(oiva_plan* p) {
    OIVA_NEED(p != nullptr, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_x, OIVA_ERR_STATE, "X not set (oiva_plan_set_x_host/_dev)");
    OIVA_NEED(p->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_plan_covariance)");
    OIVA_NEED(p->have_w, OIVA_ERR_STATE, "demixing matrix not set (oiva_plan_set_w)");
    return OIVA_OK;
}

// X of the plan is now the array at X (its own copy or the caller's): captured graphs hold the old pointer, Cx and the padded
// copy are of the old array
int install_x(oiva_plan* p, const float2* X) {
    if (p->X != X) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        const int rc = drop_graph(p);
        if (rc) return rc;
    }
    p->X = X;
    p->have_x = true;
    p->have_cx = false;
    p->pad_valid = false;
    return OIVA_OK;
}
// what every setter of the iteration's geometry does around its change: the stream idle, no captured graph of the old
// geometry, `change` (a status; it re-chooses the geometry it touches), covariance partials for the splits there are now
template <class Change>
int change_geometry(oiva_plan* p, Change&& change) {
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    int rc = drop_graph(p);
    if (rc || (rc = change())) return rc;
    return ensure_vpart(p);
}

}  // namespace

extern "C" {

int oiva_version(void) { return 100; }

int oiva_device_count(int* n) {
    OIVA_NEED(n != nullptr, OIVA_ERR_ARG, "null pointer");
    OIVA_TRY_HIP(hipGetDeviceCount(n));
    return OIVA_OK;
}

int oiva_plan_create(oiva_plan** out, int device, int T, int F, int M, int K, int model, int F_total, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(T >= 1 && F >= 1, OIVA_ERR_ARG, "T and F must be >= 1");
    OIVA_NEED(M >= 1 && M <= OIVA_MAX_CHANNELS, OIVA_ERR_ARG, "number of channels must be in 1..32");
    OIVA_NEED(K >= 1 && K <= M, OIVA_ERR_ARG, "n_src must be in 1..n_chan");
    OIVA_NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    OIVA_NEED(F_total >= F, OIVA_ERR_ARG, "F_total must be >= F");
    int ndev = 0;
    OIVA_TRY_HIP(hipGetDeviceCount(&ndev));
    OIVA_NEED(device >= 0 && device < ndev, OIVA_ERR_ARG, "no such device");
    DeviceGuard guard(device);

    oiva_plan* p = new oiva_plan();
    p->device = p->mem.device = device;
    p->T = T;
    p->F = F;
    p->M = M;
    p->K = K;
    p->model = model;
    p->F_total = F_total;
    const hipError_t es = p->stream.open(stream, 0);
    if (es != hipSuccess) {
        oiva_plan_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(es));
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            p->n_cu = prop.multiProcessorCount;
    }
    if (M > 8 && M <= kNarrowMax && M % 2 == 1) {
        // 9 / 11 / 13 / 15 channels: the vector-ALU covariance kernels read 16-byte pieces at an even channel pitch, so
        // they get their own copy of X with one zero channel per bin (filled by oiva_plan_covariance; + (M + 1) / M of X)
        const hipError_t ep = p->mem.take_one(&p->X_pad, (size_t)T * F * (M + 1) * sizeof(float2));
        if (ep != hipSuccess) {
            oiva_plan_destroy(p);
            return fail_with(OIVA_ERR_HIP, std::string("allocation of the padded copy of X failed: ") + hipGetErrorString(ep));
        }
    }
    {
        const char* v = std::getenv("OIVA_COV_HMFMA");
        p->cov_hmfma_on = !(v && v[0] == '0');
        const char* u = std::getenv("OIVA_COV_UPDATE");
        p->fuse_cov_update = u && u[0] == '1';
        const char* r = std::getenv("OIVA_POWER_REVERSE");      // read here, once: the plan keeps what it was created with
        p->power_reverse = (r && r[0] == '0') ? 0 : (r && r[0] == '2') ? 2 : 1;
        const char* x = std::getenv("OIVA_X_RESIDENT_MB");
        if (x && x[0]) p->x_resident_mb = std::atof(x);
        const char* cr = std::getenv("OIVA_COV_ROWS");
        p->cov_rows_on = !(cr && cr[0] == '0');
    }
    choose_cov_geom(p, 0);
    choose_pow_geom(p, 0);
    choose_stats_geom(p);
    p->res_ok = resident_geometry(T, F, M, K, p->n_cu, 0, &p->rg);
    const size_t nTK = (size_t)T * K;
    const size_t nFMM = (size_t)F * M * M;
    DeviceArena& mem = p->mem;
    mem.take(&p->What, nFMM * sizeof(float2));
    mem.take(&p->What64, nFMM * sizeof(double2));
    mem.take(&p->Cx, nFMM * sizeof(double));
    mem.take(&p->Ppart, (size_t)p->pw.nb * nTK * sizeof(float));
    p->ppart_alloc = p->pw.nb;
    mem.take(&p->Plocal, std::max(nTK, ((size_t)T + 1) * 32) * sizeof(float));   // also the (T + 1, 16) weights scratch (floats or doubles)
    if (M > kNarrowMax) mem.take(&p->Wwide, nTK * sizeof(double));                // the wide path's (T, K) float64 weights
    mem.take(&p->R, r_buffer_bytes(T, K));   // activations, zeroed pad rows, per-block sums (rsum_offset_floats)
    if (mem.ok()) mem.note(hipMemset(p->R, 0, r_buffer_bytes(T, K)));
    mem.take(&p->wscale, (size_t)K * sizeof(float));
    mem.take(&p->Spart, (size_t)p->stg.nsplit * F * K * 3 * sizeof(float));
    mem.take(&p->scratch_c, (size_t)K * nFMM * sizeof(double2));
    mem.take(&p->scratch_p, std::max((size_t)K * nFMM, nTK) * sizeof(double));
    if (mem.ok()) mem.note(p->stream.add_events(2));
    if (!mem.ok()) {
        const hipError_t e = mem.status();
        oiva_plan_destroy(p);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    int rc = ensure_vpart(p);
    if (rc) {
        oiva_plan_destroy(p);
        return rc;
    }
    *out = p;
    return OIVA_OK;
}

int oiva_plan_destroy(oiva_plan* p) {
    if (!p) return OIVA_OK;
    DeviceGuard guard(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->io_stream) (void)hipStreamSynchronize(p->io_stream);
    (void)p->graphs.clear();
    if (p->og_graph) (void)hipGraphExecDestroy(p->og_graph);
    p->mem.clear();
    p->io_stream.close();
    p->stream.close();
    delete p;
    return OIVA_OK;
}

int oiva_plan_set_x_host(oiva_plan* p, const void* X, long long row_pitch_bytes) {
    OIVA_NEED(p && X, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    const size_t row = (size_t)p->F * p->M * sizeof(float2);
    const size_t pitch = row_pitch_bytes > 0 ? (size_t)row_pitch_bytes : row;
    OIVA_NEED(pitch >= row, OIVA_ERR_ARG, "row pitch smaller than one frame of this plan's bins");
    if (!p->X_owned) OIVA_TRY_HIP(p->mem.take_one(&p->X_owned, row * p->T, Mem::pooled));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy2D(p->X_owned, row, X, pitch, row, p->T, hipMemcpyHostToDevice));
    return install_x(p, p->X_owned);
}

int oiva_plan_set_x_host_c128(oiva_plan* p, const void* X, long long row_pitch_bytes) {
    OIVA_NEED(p && X, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    const size_t n_row = (size_t)p->F * p->M;
    const size_t row = n_row * sizeof(double2);
    const size_t pitch = row_pitch_bytes > 0 ? (size_t)row_pitch_bytes : row;
    OIVA_NEED(pitch >= row, OIVA_ERR_ARG, "row pitch smaller than one frame of this plan's bins");
    if (!p->X_owned) OIVA_TRY_HIP(p->mem.take_one(&p->X_owned, n_row * sizeof(float2) * p->T, Mem::pooled));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    // in slabs of frames through a staging buffer (<= 256 MB): the conversion of one slab overlaps nothing, but the
    // footprint stays bounded and the host never touches the data (a NumPy astype of 1 GB costs 60 ms)
    OIVA_TRY_HIP(staged_copy_c128(true, p->stream, const_cast<void*>(X), pitch, p->X_owned, n_row, p->T, kStageBytes, p->device, Mem::pooled));
    return install_x(p, p->X_owned);
}

int oiva_plan_set_x_dev(oiva_plan* p, const void* X_dev) {
    OIVA_NEED(p && X_dev, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(((uintptr_t)X_dev & 15) == 0, OIVA_ERR_ARG, "device X must be 16-byte aligned");
    DeviceGuard guard(p->device);
    return install_x(p, (const float2*)X_dev);
}

int oiva_plan_covariance(oiva_plan* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_x, OIVA_ERR_STATE, "X not set");
    DeviceGuard guard(p->device);
    // (the padded copy follows X here: every path that changes X clears have_cx, and the iteration needs Cx; a borrowed X
    //  rewritten in place needs a new Cx too)
    p->pad_valid = false;
    int rcp = ensure_pad(p);
    if (rcp) return rcp;
    // unit weights, one "source", on the plan's splits by the kind its traits name for that (never a matrix-core kind of many
    // sources): partials land in Vpart laid out as [nsplit][F][1][M*M]
    CovGeom g = p->cov;
    g.kind = traits(p->cov.kind).unit;
    g.kc = 1;
    g.part32 = 0;
    OIVA_TRY_HIP(launch_cov(p->stream, p->X, p->X_pad, nullptr, nullptr, nullptr, p->model, 0, p->Vpart, p->cov_f64(), p->T, p->F, p->M, 1, g));
    OIVA_TRY_HIP(launch_sum_parts(p->stream, p->Vpart, partials_f64(g, p->cov_f64()), g.nsplit, p->Cx, (long long)p->F * p->M * p->M, 1. / (double)p->T));
    p->have_cx = true;
    return OIVA_OK;
}

int oiva_plan_get_cx(oiva_plan* p, void* Cx_host, int f64) {
    OIVA_NEED(p && Cx_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_cx, OIVA_ERR_STATE, "input covariance not computed");
    DeviceGuard guard(p->device);
    const size_t n = (size_t)p->F * p->M * p->M;
    OIVA_TRY_HIP(launch_unpack_herm(p->stream, p->Cx, p->scratch_c, f64 != 0, p->F, p->M));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(Cx_host, p->scratch_c, n * (f64 ? sizeof(double2) : sizeof(float2)), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

int oiva_plan_set_w(oiva_plan* p, const void* W0_host, int f64) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_cx, OIVA_ERR_STATE, "input covariance not computed (needed for the orthogonality constraint)");
    DeviceGuard guard(p->device);
    const int M = p->M, K = p->K;
    const std::vector<double2> wh = pack_what(W0_host, f64, (size_t)p->F, M, K);
    int rc = upload_what(p, wh);
    if (rc) return rc;
    p->wscale_pending = false;
    p->have_w = true;
    if (K < M) return stage_update(p, true);  // J from the orthogonality constraint, overiva.py:120-121
    return OIVA_OK;
}

static int set_w_from_eigenvectors(oiva_plan* p, double* evals_host, bool lapack_phase);

int oiva_plan_set_w_pca(oiva_plan* p, double* evals_host) { return set_w_from_eigenvectors(p, evals_host, false); }
int oiva_plan_set_w_eig(oiva_plan* p) { return set_w_from_eigenvectors(p, nullptr, true); }

static int set_w_from_eigenvectors(oiva_plan* p, double* evals_host, bool lapack_phase) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_plan_covariance)");
    DeviceGuard guard(p->device);
    double* evals = evals_host ? p->scratch_p : nullptr;       // scratch_p holds at least K * F * M * M doubles
    OIVA_TRY_HIP(launch_pca_subspace(p->stream, p->Cx, p->What, p->What64, evals, p->F, p->M, p->K, lapack_phase));
    p->what64_valid = true;
    p->wscale_pending = false;
    p->have_w = true;
    if (evals_host) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        OIVA_TRY_HIP(hipMemcpy(evals_host, evals, (size_t)p->F * p->M * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (p->K < p->M) return stage_update(p, true);             // J from the orthogonality constraint
    return OIVA_OK;
}

static int check_fused(oiva_plan* p);

int oiva_plan_demix_dev(oiva_plan* p, int proj_back, void** Y_dev) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(Y_dev, OIVA_ERR_ARG, "null output");
    DeviceGuard guard(p->device);
    if ((rc = check_fused(p))) return rc;
    if (!p->Y) OIVA_TRY_HIP(p->mem.take_one(&p->Y, (size_t)p->F * p->K * sizeof(float2) * p->T, Mem::pooled));
    const float* sp = nullptr;
    if (proj_back) {
        OIVA_TRY_HIP(launch_demix_stats(p->stream, p->X, p->What, p->Spart, p->T, p->F, p->M, p->K, p->stg));
        sp = p->Spart;
    }
    OIVA_TRY_HIP(launch_demix_write(p->stream, p->X, p->What, sp, p->stg.nsplit, p->Y, p->T, p->F, p->M, p->K));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    *Y_dev = p->Y;
    return OIVA_OK;
}

int oiva_plan_iterate(oiva_plan* p, int n) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(n >= 0, OIVA_ERR_ARG, "negative iteration count");
    OIVA_NEED(p->F == p->F_total || resident_applies(p) || p->fx_on, OIVA_ERR_STATE,
              "plan owns a bin shard: drive it with oiva_plan_power / all-gather / oiva_plan_update (or connect an in-kernel exchange: "
              "oiva_plan_fused_connect, oiva_plan_resident_connect)");
    DeviceGuard guard(p->device);
    if (n == 0) return OIVA_OK;
    if (resident_applies(p)) {
        bool ran = false;
        if ((rc = run_resident(p, n, &ran))) return rc;
        if (ran) return OIVA_OK;
    }
    if (p->use_graph) {
        for (int left = n; left > 0;) {
            const int m = std::min(left, kGraphMaxIters);
            hipGraphExec_t g = nullptr;
            if ((rc = graph_for(p, m, &g))) return rc;
            OIVA_TRY_HIP(hipGraphLaunch(g, p->stream));
            left -= m;
        }
        // the host-side flags after n iterations, whether the graph was captured now (capturing runs stage_update, which sets
        // them) or taken from the cache (nothing runs on the host): the float32 update leaves the complex128 copy behind
        p->wscale_pending = false;
        p->raw_weights = 0;
        p->what64_valid = p->upd_f64();
        return OIVA_OK;
    }
    for (int i = 0; i < n; ++i)
        if ((rc = one_iteration(p))) return rc;
    return OIVA_OK;
}

int oiva_plan_power(oiva_plan* p) {
    int rc = check_ready(p);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    return stage_power(p);
}

int oiva_plan_power_buffer(oiva_plan* p, int parts_per_rank, void** parts_dev, long long* bytes) {
    OIVA_NEED(p && parts_dev, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(parts_per_rank >= p->pw.nb, OIVA_ERR_ARG, "parts_per_rank smaller than this plan's own bin batches");
    DeviceGuard guard(p->device);
    const size_t part = (size_t)p->T * p->K * sizeof(float);
    if (parts_per_rank > p->ppart_alloc) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        int rc = drop_graph(p);
        if (rc) return rc;
        p->mem.release(&p->Ppart);
        OIVA_TRY_HIP(p->mem.take_one(&p->Ppart, part * parts_per_rank));
        // parts beyond nb stay zero; on the plan's own stream, so that it is ordered before the next power pass
        OIVA_TRY_HIP(hipMemsetAsync(p->Ppart, 0, part * parts_per_rank, p->stream));
        p->ppart_alloc = parts_per_rank;
    }
    *parts_dev = p->Ppart;
    if (bytes) *bytes = (long long)(part * parts_per_rank);
    return OIVA_OK;
}

int oiva_plan_update(oiva_plan* p, const void* parts_dev, int nparts) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(parts_dev && nparts >= 1, OIVA_ERR_ARG, "need at least one part");
    DeviceGuard guard(p->device);
    if ((rc = stage_activation(p, (const float*)parts_dev, nparts))) return rc;
    if (cov_update_applies(p)) return stage_cov_update(p);
    if ((rc = stage_cov(p))) return rc;
    return stage_update(p, false);
}

// Y = demix(X, W) (+ projection back) into a host array, complex64 or complex128 (overiva.py:192-204).
//   $OIVA_DEMIX_IO = ring (default): slabs of frames; slab k is computed (write_kernel; for complex128 also widened on the
//       device), copied into a slot of the process-wide pinned ring on a second stream and moved from there into the
//       caller's array by the copy threads, all three overlapping across slabs;
//   register: the caller's array is page-locked for the call (hipHostRegister) and the slabs are copied straight into it;
//   legacy: one kernel over all frames, one synchronous hipMemcpy2D (the form up to round 4).
// Same bits in every mode: the kernel does the same arithmetic per (frame, bin) whatever the slab.
static int demix_to_host(oiva_plan* p, void* Y_host, long long row_pitch_bytes, int proj_back, bool c128) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(Y_host, OIVA_ERR_ARG, "null output");
    DeviceGuard guard(p->device);
    const size_t n_row = (size_t)p->F * p->K;
    const size_t row_dev = n_row * sizeof(float2);
    const size_t row = c128 ? n_row * sizeof(double2) : row_dev;
    const size_t pitch = row_pitch_bytes > 0 ? (size_t)row_pitch_bytes : row;
    OIVA_NEED(pitch >= row, OIVA_ERR_ARG, "row pitch smaller than one frame of this plan's bins");
    if ((rc = check_fused(p))) return rc;
    if (!p->Y) OIVA_TRY_HIP(p->mem.take_one(&p->Y, row_dev * p->T, Mem::pooled));
    const float* sp = nullptr;
    if (proj_back) {
        OIVA_TRY_HIP(launch_demix_stats(p->stream, p->X, p->What, p->Spart, p->T, p->F, p->M, p->K, p->stg));
        sp = p->Spart;
    }
    static const int mode = [] {
        const char* v = std::getenv("OIVA_DEMIX_IO");
        if (v && !std::strcmp(v, "legacy")) return 0;
        if (v && !std::strcmp(v, "register")) return 2;
        return 1;
    }();
    const size_t slab_target = p->io_slab_bytes ? p->io_slab_bytes : ((size_t)8 << 20);
    if (mode == 0 || (size_t)p->T * row < slab_target / 2) {
        // small outputs (and the legacy form): one kernel, one copy
        OIVA_TRY_HIP(launch_demix_write(p->stream, p->X, p->What, sp, p->stg.nsplit, p->Y, p->T, p->F, p->M, p->K));
        if (!c128) {
            OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
            OIVA_TRY_HIP(hipMemcpy2D(Y_host, pitch, p->Y, row, row, p->T, hipMemcpyDeviceToHost));
            return OIVA_OK;
        }
        OIVA_TRY_HIP(staged_copy_c128(false, p->stream, Y_host, pitch, p->Y, n_row, p->T, kStageBytes, p->device, Mem::plain));
        return OIVA_OK;
    }
    // ---- slabs of about 8 MB of output
    const int slab = (int)std::max<size_t>(1, std::min<size_t>((size_t)p->T, slab_target / row));
    const int nslab = ceil_div(p->T, slab);
    const size_t slab_bytes = (size_t)slab * row;
    if (!p->io_stream) OIVA_TRY_HIP(p->io_stream.open(nullptr, 0));
    if (p->io_stream.events.size() < 2 * kHostRingSlots)
        OIVA_TRY_HIP(p->io_stream.add_events(2 * kHostRingSlots - (int)p->io_stream.events.size(), /*timing*/ false));
    hipEvent_t* io_written = p->io_stream.events.data();
    hipEvent_t* io_copied = io_written + kHostRingSlots;
    if (c128 && p->io_c128_bytes < slab_bytes) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        // all three or none: the recorded size is that of every non-null slot, also after a failed allocation
        for (auto& b : p->io_c128) p->mem.release(&b);
        p->io_c128_bytes = 0;
        for (auto& b : p->io_c128) p->mem.take(&b, slab_bytes, Mem::pooled);
        if (!p->mem.ok()) {
            for (auto& b : p->io_c128) p->mem.release(&b);
            OIVA_TRY_HIP(p->mem.status());
        }
        p->io_c128_bytes = slab_bytes;
    }
    bool registered = false;
    void* pinned[kHostRingSlots] = {};
    if (mode == 2) {
        registered = hipHostRegister(Y_host, pitch * (size_t)(p->T - 1) + row, hipHostRegisterDefault) == hipSuccess;
        if (!registered) (void)hipGetLastError();      // (an unaligned or foreign range: the ring serves)
    }
    // (the pinned ring and the copy threads are process-wide: one hand-over at a time, whatever thread or plan asks)
    static std::mutex io_mutex;
    std::unique_lock<std::mutex> io_lock(io_mutex, std::defer_lock);
    if (!registered) {
        io_lock.lock();
        OIVA_TRY_HIP(host_ring_slots(slab_bytes, pinned));
    }
    auto finish = [&](hipError_t e) -> int {
        // nothing of this call is in flight when the ring (io_mutex) passes to the next caller, also after an error
        (void)hipStreamSynchronize(p->io_stream);
        if (registered) (void)hipHostUnregister(Y_host);
        if (e != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("final demix: ") + hipGetErrorString(e));
        return OIVA_OK;
    };
    auto issue = [&](int k) -> hipError_t {
        const int s = k % kHostRingSlots;
        const int t0 = k * slab, nt = std::min(slab, p->T - t0);
        float2* ydev = p->Y + (size_t)t0 * n_row;
        hipError_t e = launch_demix_write(p->stream, p->X + (size_t)t0 * p->F * p->M, p->What, sp, p->stg.nsplit, ydev, nt, p->F, p->M, p->K);
        const void* src = ydev;
        if (e == hipSuccess && c128) {
            e = launch_cast_c64_to_c128(p->stream, ydev, p->io_c128[s], (long long)nt * n_row);
            src = p->io_c128[s];
        }
        if (e == hipSuccess) e = hipEventRecord(io_written[s], p->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(p->io_stream, io_written[s], 0);
        if (e == hipSuccess) {
            if (registered)
                e = hipMemcpy2DAsync(static_cast<char*>(Y_host) + (size_t)t0 * pitch, pitch, src, row, row, nt, hipMemcpyDeviceToHost, p->io_stream);
            else
                e = hipMemcpyAsync(pinned[s], src, (size_t)nt * row, hipMemcpyDeviceToHost, p->io_stream);
        }
        if (e == hipSuccess) e = hipEventRecord(io_copied[s], p->io_stream);
        // (slot s -- the pinned buffer and, for complex128, the device staging buffer -- is rewritten by slab k + slots, which
        //  the loop below issues only after it has waited for THIS copy and moved its data on)
        return e;
    };
    int issued = 0;
    for (int k = 0; k < nslab; ++k) {
        hipError_t e = hipSuccess;
        while (issued < nslab && issued - k < kHostRingSlots && e == hipSuccess) e = issue(issued++);
        if (k == 0 && !registered && e == hipSuccess) {
            // the copy threads must not meet pages that were never touched (a fresh NumPy array): eight threads faulting the
            // same mapping in ran at 8 GB/s where resident pages take 41.  Populating them costs 1-2 ms for 131 MB -- next to
            // nothing when the caller already did (overiva() does, behind its iterations) -- and runs while the first slabs
            // are computed and cross PCIe.
            host_prefault(Y_host, pitch * (size_t)(p->T - 1) + row, /*may_touch*/ pitch == row);
        }
        if (e == hipSuccess) e = hipEventSynchronize(io_copied[k % kHostRingSlots]);
        if (e != hipSuccess) return finish(e);
        if (!registered) {
            const int t0 = k * slab, nt = std::min(slab, p->T - t0);
            host_copy_rows(static_cast<char*>(Y_host) + (size_t)t0 * pitch, pitch, pinned[k % kHostRingSlots], row, row, nt);
        }
    }
    return finish(hipStreamSynchronize(p->stream));
}

int oiva_plan_set_io_slab(oiva_plan* p, long long bytes) {
    OIVA_NEED(p && bytes >= 0, OIVA_ERR_ARG, "bad arguments");
    p->io_slab_bytes = (size_t)bytes;
    return OIVA_OK;
}

int oiva_plan_demix(oiva_plan* p, void* Y_host, long long row_pitch_bytes, int proj_back) {
    return demix_to_host(p, Y_host, row_pitch_bytes, proj_back, false);
}

int oiva_plan_demix_c128(oiva_plan* p, void* Y_host, long long row_pitch_bytes, int proj_back) {
    return demix_to_host(p, Y_host, row_pitch_bytes, proj_back, true);
}

int oiva_plan_get_w(oiva_plan* p, void* W_host, int f64) {
    OIVA_NEED(p && W_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_w, OIVA_ERR_STATE, "demixing matrix not set");
    DeviceGuard guard(p->device);
    int rc = check_fused(p);
    if (rc) return rc;
    std::vector<double2> wh;
    rc = download_what(p, wh);
    if (rc) return rc;
    const bool finite = unpack_w(wh, 0, (size_t)p->F, p->M, p->K, W_host, f64);
    if (!finite) return fail_with(OIVA_ERR_NUMERIC, "demixing matrix holds non-finite values (singular W_hat^H V)");
    return OIVA_OK;
}

// the in-kernel exchange of the four-launch path gave up waiting for a rank: recorded on the device, looked at by everything
// that hands results to the caller (sync, get_w, the demix entry points).  The flag is copied into a pinned word behind the
// work already queued on the plan's stream and read after ONE wait for that stream.
static int check_fused(oiva_plan* p) {
    if (!p->fx_state || !p->fx_on) return OIVA_OK;
    if (!p->fx_flag_host) OIVA_TRY_HIP(p->mem.take_one(&p->fx_flag_host, sizeof(unsigned), Mem::pinned));
    OIVA_TRY_HIP(hipMemcpyAsync(p->fx_flag_host, p->fx_state, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    const unsigned code = *p->fx_flag_host;
    if (code != 0)
        return fail_with(OIVA_ERR_STATE, "the exchange inside the activation kernel gave up waiting for a rank's partial powers (workgroup " +
                                        std::to_string(code - 1) + "): the state of this plan is undefined (oiva_plan_restore_w brings back the "
                                        "demixing matrices saved by oiva_plan_save_w; oiva_plan_fused_connect(p, NULL) clears the condition)");
    return OIVA_OK;
}

int oiva_plan_sync(oiva_plan* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    return check_fused(p);
}

int oiva_plan_save_w(oiva_plan* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_w, OIVA_ERR_STATE, "demixing matrix not set");
    DeviceGuard guard(p->device);
    const size_t n = (size_t)p->F * p->M * p->M;
    if (!p->ck_what) OIVA_TRY_HIP(p->mem.take_one(&p->ck_what, n * sizeof(float2)));
    if (!p->ck_what64) OIVA_TRY_HIP(p->mem.take_one(&p->ck_what64, n * sizeof(double2)));
    // on the plan's stream: ordered behind the iterations already queued, in front of the ones that follow
    OIVA_TRY_HIP(hipMemcpyAsync(p->ck_what, p->What, n * sizeof(float2), hipMemcpyDeviceToDevice, p->stream));
    OIVA_TRY_HIP(hipMemcpyAsync(p->ck_what64, p->What64, n * sizeof(double2), hipMemcpyDeviceToDevice, p->stream));
    p->ck_what64_valid = p->what64_valid;
    p->ck_valid = true;
    return OIVA_OK;
}

int oiva_plan_restore_w(oiva_plan* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->ck_valid, OIVA_ERR_STATE, "nothing saved (oiva_plan_save_w)");
    DeviceGuard guard(p->device);
    const size_t n = (size_t)p->F * p->M * p->M;
    OIVA_TRY_HIP(hipMemcpyAsync(p->What, p->ck_what, n * sizeof(float2), hipMemcpyDeviceToDevice, p->stream));
    OIVA_TRY_HIP(hipMemcpyAsync(p->What64, p->ck_what64, n * sizeof(double2), hipMemcpyDeviceToDevice, p->stream));
    p->what64_valid = p->ck_what64_valid;
    p->wscale_pending = false;
    p->have_w = true;
    return OIVA_OK;
}

static int fused_setup(oiva_plan* p) {
    const size_t words = 16 + (size_t)rsum_blocks(p->T) * p->K;
    if (!p->fx_state) OIVA_TRY_HIP(p->mem.take_one(&p->fx_state, words * sizeof(unsigned)));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemset(p->fx_state, 0, words * sizeof(unsigned)));
    return drop_graph(p);                       // captured graphs hold the other activation kernel
}

int oiva_plan_fused_connect(oiva_plan* p, oiva_xchg* x) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(!p->fx_loopback, OIVA_ERR_STATE, "the plan runs the loop-back exchange (oiva_plan_fused_loopback(p, 0) switches it off)");
    DeviceGuard guard(p->device);
    if (!x) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        p->fx_on = false;
        p->fx_world = 1;
        p->fx_rank = 0;
        for (auto& g : p->fx_gath) g = nullptr;
        if (p->fx_state) OIVA_TRY_HIP(hipMemset(p->fx_state, 0, sizeof(unsigned)));     // a wait that gave up is history now
        return drop_graph(p);
    }
    char* peers[OIVA_XCHG_MAX_RANKS];
    int rank = 0, world = 1;
    size_t slot = 0;
    OIVA_NEED(xchg_peers(x, peers, &rank, &world, &slot) == 0, OIVA_ERR_STATE, "exchange not connected");
    // slot = nblk * T * K * 8 bytes: nblk block sums per rank (every rank the same; 1 = the rank's sum)
    const size_t word_bytes = (size_t)p->T * p->K * 8;
    OIVA_NEED(slot % word_bytes == 0 && slot / word_bytes >= 1 && slot / word_bytes <= (size_t)kCanonBlocks, OIVA_ERR_ARG,
              "exchange slot size must be nblk * T * K * 8 bytes, nblk = 1 ... 8 block sums per rank");
    const int nblk = (int)(slot / word_bytes);
    OIVA_NEED(p->pw.nb % nblk == 0, OIVA_ERR_ARG, "the plan's 64-bin parts do not divide into that many blocks");
    OIVA_NEED((world - 1) * nblk <= kCanonBlocks, OIVA_ERR_ARG, "the activation kernel polls at most 8 words of the other ranks per frame and source (9 ranks of one sum each)");
    int rc = fused_setup(p);
    if (rc) return rc;
    // the epochs of this connection start at 1 again: words left in the own gather buffer by an earlier connection (tagged
    // 1 ... n) must not pass for current ones.  The other ranks store into this buffer from their first iteration on, so
    // the callers rendezvous between connecting and iterating (include/overiva_hip.h; sharded.py does).
    OIVA_TRY_HIP(hipMemset(peers[rank], 0, (size_t)2 * world * slot));
    OIVA_TRY_HIP(hipDeviceSynchronize());
    p->fx_nblk_own = p->fx_nblk_peer = nblk;
    for (int r = 0; r < OIVA_XCHG_MAX_RANKS; ++r) p->fx_gath[r] = peers[r];
    p->fx_rank = rank;
    p->fx_world = world;
    p->fx_on = true;
    return OIVA_OK;
}

int oiva_plan_fused_loopback(oiva_plan* p, int world) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(world >= 0 && world <= OIVA_XCHG_MAX_RANKS, OIVA_ERR_ARG, "bad number of ranks");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    p->mem.release(&p->fx_loop_buf);
    if (p->fx_loopback) {
        p->fx_on = p->fx_loopback = false;
        p->fx_world = 1;
        for (auto& g : p->fx_gath) g = nullptr;
        int rc = drop_graph(p);
        if (rc) return rc;
    }
    if (world <= 1) return OIVA_OK;
    OIVA_NEED(!p->fx_on, OIVA_ERR_STATE, "the plan is connected to other ranks (oiva_plan_fused_connect(p, NULL) disconnects)");
    OIVA_NEED(p->F == p->F_total, OIVA_ERR_STATE, "loop-back plays the other ranks with zeros: the plan must own all bins");
    // own blocks: those of the single-GPU sum (the result keeps its bits); per phantom rank the words a real rank of that
    // world would send: 8 / world blocks
    const int bsz = (p->pw.nb + kCanonBlocks - 1) / kCanonBlocks;
    p->fx_nblk_own = (p->pw.nb + bsz - 1) / bsz;
    p->fx_nblk_peer = std::max(1, kCanonBlocks / world);
    OIVA_NEED((world - 1) * p->fx_nblk_peer <= kCanonBlocks, OIVA_ERR_ARG, "at most 9 ranks");
    const size_t bytes = (size_t)2 * world * p->fx_nblk_peer * p->T * p->K * 8;
    OIVA_TRY_HIP(p->mem.take_one(&p->fx_loop_buf, bytes, Mem::fine));
    OIVA_TRY_HIP(hipMemset(p->fx_loop_buf, 0, bytes));
    int rc = fused_setup(p);
    if (rc) return rc;
    for (int r = 0; r < world; ++r) p->fx_gath[r] = p->fx_loop_buf;
    p->fx_rank = 0;
    p->fx_world = world;
    p->fx_loopback = true;
    p->fx_on = true;
    return OIVA_OK;
}

int oiva_plan_fused_debug(oiva_plan* p, int timeout_ms, int stall) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    DeviceGuard guard(p->device);
    p->fx_timeout_ms = timeout_ms;
    p->fx_stall = stall;
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    return drop_graph(p);                       // (both are kernel arguments of captured launches)
}

int oiva_plan_iterate_timed(oiva_plan* p, int n, float* total_ms, float* per_kernel_ms) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && total_ms, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(p->F == p->F_total, OIVA_ERR_STATE, "timed iterate needs a plan that owns all bins");
    DeviceGuard guard(p->device);
    if (!per_kernel_ms) return p->stream.elapsed_ms(0, 1, [&] { return oiva_plan_iterate(p, n); }, total_ms);
    // per-kernel: an event before every launch and one after the last launch of each iteration, all
    // recorded without draining the stream; elapsed times are read after one final synchronisation.
    for (int s = 0; s < OIVA_N_STAGES; ++s) per_kernel_ms[s] = 0.f;
    *total_ms = 0.f;
    const int per_it = OIVA_N_STAGES + 1;
    // (two local event owners: the bracketing events, which must all exist, and the covariance kernel's own pairs, of which
    //  as many are used as could be made)
    HandleStream bracket, kern;
    hipError_t err = bracket.add_events(n * per_it);
    if (err != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(err));
    if (kern.add_events(2 * n) != hipSuccess) (void)hipGetLastError();
    std::vector<hipEvent_t>& pool = bracket.events;
    std::vector<hipEvent_t> kev = kern.events;
    kev.resize((size_t)2 * n, nullptr);
    for (int it = 0; it < n && err == hipSuccess && rc == OIVA_OK; ++it) {
        hipEvent_t* e = pool.data() + (size_t)it * per_it;
        err = hipEventRecord(e[0], p->stream);
        if (err == hipSuccess && !(rc = stage_power(p))) err = hipEventRecord(e[1], p->stream);
        if (err == hipSuccess && !rc && !(rc = stage_activation(p, p->Ppart, p->pw.nb))) err = hipEventRecord(e[2], p->stream);
        const bool fused = cov_update_applies(p);          // covariance + update as one launch: all of it is stage 2, stage 3 is empty
        if (err == hipSuccess && !rc) {
            arm_kernel_timer(kev[2 * it], kev[2 * it + 1]);    // the covariance kernel's own start / stop (see launch_dominant)
            rc = fused ? stage_cov_update(p) : stage_cov(p);
            arm_kernel_timer(nullptr, nullptr);
            if (!rc) err = hipEventRecord(e[3], p->stream);
        }
        if (err == hipSuccess && !rc && !(fused ? OIVA_OK : (rc = stage_update(p, false)))) err = hipEventRecord(e[4], p->stream);
    }
    if (err == hipSuccess && rc == OIVA_OK) err = hipStreamSynchronize(p->stream);
    for (int it = 0; it < n && err == hipSuccess && rc == OIVA_OK; ++it) {
        hipEvent_t* e = pool.data() + (size_t)it * per_it;
        for (int s = 0; s < OIVA_N_STAGES && err == hipSuccess; ++s) {
            float ms = 0.f;
            err = hipEventElapsedTime(&ms, e[s], e[s + 1]);
            // the covariance stage is reported as the duration of its kernel proper (events attached to the dispatch),
            // which is what the roofline is about and what rocprofv3 shows; the bracketing events add ~3 us of gaps
            float kms = 0.f;
            // (where the stage is two launches -- a weights pre-pass in front of the kernel: 9..16 channels, the float64 kernel
            //  of 8 channels, 8 channels with three or more sources -- it keeps its bracketed time, so that the stages still add
            //  up to the total)
            const bool one_launch = traits(p->cov.kind).launches == 1;
            if (s == 2 && one_launch && kev[2 * it] && kev[2 * it + 1] && hipEventElapsedTime(&kms, kev[2 * it], kev[2 * it + 1]) == hipSuccess &&
                kms > 0.f && kms <= ms)
                ms = kms;
            else if (s == 2)
                (void)hipGetLastError();
            per_kernel_ms[s] += ms;
        }
    }
    if (err == hipSuccess && rc == OIVA_OK) err = hipEventElapsedTime(total_ms, pool[0], pool[(size_t)n * per_it - 1]);
    if (rc) return rc;
    OIVA_TRY_HIP(err);
    return OIVA_OK;
}

int oiva_plan_get_cov_splits(oiva_plan* p, int* nsplit) {
    OIVA_NEED(p && nsplit, OIVA_ERR_ARG, "null argument");
    *nsplit = p->cov.nsplit;
    return OIVA_OK;
}

int oiva_plan_set_cov_splits(oiva_plan* p, int nsplit) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(nsplit >= 0 && nsplit <= p->T, OIVA_ERR_ARG, "bad split count");
    return change_geometry(p, [&] { choose_cov_geom(p, nsplit); return OIVA_OK; });
}

int oiva_plan_set_cov_quad(oiva_plan* p, int enable, int* active) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    return change_geometry(p, [&] {
        p->cov_quad_on = enable != 0;
        choose_cov_geom(p, 0);
        if (active) *active = traits(p->cov.kind).quad_switch;
        return OIVA_OK;
    });
}

int oiva_plan_set_fuse_cov_update(oiva_plan* p, int enable, int* active) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    if (enable >= 0) {
        const int rc = change_geometry(p, [&] { p->fuse_cov_update = enable != 0; return OIVA_OK; });
        if (rc) return rc;
    }
    if (active) *active = cov_update_applies(p) ? 1 : 0;
    return OIVA_OK;
}

int oiva_plan_set_cov_hmfma(oiva_plan* p, int enable) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    return change_geometry(p, [&] { p->cov_hmfma_on = enable != 0; choose_cov_geom(p, 0); return OIVA_OK; });
}

int oiva_plan_set_pow_splits(oiva_plan* p, int nsplit) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(nsplit >= 0 && nsplit <= p->T, OIVA_ERR_ARG, "bad split count");
    return change_geometry(p, [&] { choose_pow_geom(p, nsplit); return OIVA_OK; });
}

int oiva_plan_set_power_reverse(oiva_plan* p, int enable) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    return change_geometry(p, [&] { p->power_reverse = enable < 0 ? 0 : enable > 2 ? 2 : enable; return OIVA_OK; });
}

int oiva_plan_set_x_resident_mb(oiva_plan* p, double mb) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(mb == mb, OIVA_ERR_ARG, "the budget is not a number");
    // (where X streams the power pass takes other chunks: choose_pow)
    return change_geometry(p, [&] { p->x_resident_mb = mb; choose_pow_geom(p, p->pow_splits_req); return OIVA_OK; });
}

int oiva_plan_get_x_resident(oiva_plan* p, int* n16, int* nt, int* reason) {
    OIVA_NEED(p && n16 && nt && reason, OIVA_ERR_ARG, "null argument");
    const XPolicy x = x_policy(p);
    *n16 = x.n16, *nt = x.nt ? 1 : 0, *reason = (int)x.why;
    return OIVA_OK;
}

int oiva_plan_set_cov_rows(oiva_plan* p, int enable) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    return change_geometry(p, [&] { p->cov_rows_on = enable != 0; return OIVA_OK; });
}

int oiva_plan_get_cov_rows(oiva_plan* p, int* rows) {
    OIVA_NEED(p && rows, OIVA_ERR_ARG, "null argument");
    *rows = cov_geom_now(p).rows;
    return OIVA_OK;
}

int oiva_plan_use_graph(oiva_plan* p, int enable) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    DeviceGuard guard(p->device);
    p->use_graph = enable ? 1 : 0;
    if (!enable) return drop_graph(p);
    if (p->have_x && p->have_cx && p->have_w && (p->F == p->F_total || p->fx_on)) return build_graphs(p);
    return OIVA_OK;
}

int oiva_plan_set_precision(oiva_plan* p, int flags) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED((flags & ~(OIVA_PREC_UPDATE_F64 | OIVA_PREC_UPDATE_ROWS | OIVA_PREC_COV_F64)) == 0, OIVA_ERR_ARG, "unknown precision flag");
    return change_geometry(p, [&] {
        if ((flags & OIVA_PREC_UPDATE_F64) && p->have_w && !p->what64_valid) {
            // switching the update to float64 mid-run: seed the complex128 copy from the complex64 state
            std::vector<double2> wh;
            int rc;
            if ((rc = download_what(p, wh)) || (rc = upload_what(p, wh))) return rc;
        }
        // (more than 8 channels: which float32 kernel takes the pass also depends on the arithmetic of the per-bin algebra;
        // 8 channels with three or more sources: the number of frame splits does)
        const bool cov_changed = ((flags ^ p->prec) & (OIVA_PREC_COV_F64 | (traits(p->cov.kind).update_arith ? OIVA_PREC_UPDATE_F64 : 0))) != 0;
        p->prec = flags;
        if (cov_changed) choose_cov_geom(p, 0);            // sources per pass and residency depend on the accumulator type
        if (cov_changed) choose_pow_geom(p, p->pow_splits_req);      // ... and whether X streams, which the power chunks follow
        return (int)OIVA_OK;
    });
}

// ---- X-resident iteration ------------------------------------------------------------------------------
int oiva_plan_set_resident(oiva_plan* p, int enable) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    if (!enable) {
        p->res_on = false;
        return OIVA_OK;
    }
    OIVA_NEED(p->res_ok, OIVA_ERR_ARG,
              "shape does not qualify for the X-resident iteration (4 or 8 channels, 1 or 2 sources with background channels, "
              "16 bins x <= 256 frames per compute unit)");
    DeviceGuard guard(p->device);
    int rc = resident_alloc(p);
    if (rc) return rc;
    p->res_on = true;
    return OIVA_OK;
}

int oiva_plan_set_resident_splits(oiva_plan* p, int nsplit) {
    OIVA_NEED(p && nsplit >= 0, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(!p->res_on, OIVA_ERR_STATE, "switch the resident iteration off before changing its geometry");
    DeviceGuard guard(p->device);
    ResidentGeom g;
    const bool ok = resident_geometry(p->T, p->F, p->M, p->K, p->n_cu, nsplit, &g);
    OIVA_NEED(ok || nsplit == 0, OIVA_ERR_ARG, "the shape does not fit on chip with that many frame splits");
    if (p->res_block) {                        // buffers were sized for the old geometry
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        p->mem.release(&p->res_block);
    }
    p->res_ok = ok;
    if (ok) p->rg = g;
    return OIVA_OK;
}

int oiva_plan_resident_loopback(oiva_plan* p, int world) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(world >= 0 && world <= OIVA_XCHG_MAX_RANKS, OIVA_ERR_ARG, "bad number of ranks");
    OIVA_NEED(!p->res_on, OIVA_ERR_STATE, "switch the resident iteration off before changing its exchange");
    DeviceGuard guard(p->device);
    if (p->res_loop_buf) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        p->mem.release(&p->res_loop_buf);
    }
    p->res_loopback = false;
    p->res_world = 1;
    p->res_rank = 0;
    for (auto& g : p->res_gath) g = nullptr;
    if (world <= 1) return OIVA_OK;
    OIVA_NEED(p->res_ok, OIVA_ERR_ARG, "shape does not qualify for the X-resident iteration");
    OIVA_NEED(p->F == p->F_total, OIVA_ERR_STATE, "loop-back plays the other ranks with zeros: the plan must own all bins");
    // the gather buffer of the multi-GPU exchange, same kind of memory (fine-grained, system-scope atomics), but nobody else
    // maps it: [2 (epoch parity)][world][NS * TW][K] floats
    const size_t bytes = (size_t)2 * world * p->rg.NS * p->rg.TW * p->K * sizeof(float);
    OIVA_TRY_HIP(p->mem.take_one(&p->res_loop_buf, bytes, Mem::fine));
    OIVA_TRY_HIP(hipMemset(p->res_loop_buf, 0, bytes));
    for (int r = 0; r < world; ++r) p->res_gath[r] = p->res_loop_buf;
    p->res_world = world;
    p->res_loopback = true;
    if (p->res_block) {                        // epochs restart with the fresh buffer
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        OIVA_TRY_HIP(hipMemset(p->res_block, 0, p->res_block_bytes));
        p->res_epoch = 0;
    }
    return OIVA_OK;
}

int oiva_plan_resident_connect(oiva_plan* p, oiva_xchg* x) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(!p->res_loopback, OIVA_ERR_STATE, "the plan runs the loop-back exchange (oiva_plan_resident_loopback(p, 0) switches it off)");
    if (!x) {                                  // back to a single rank
        p->res_world = 1;
        p->res_rank = 0;
        for (auto& g : p->res_gath) g = nullptr;
        return OIVA_OK;
    }
    OIVA_NEED(p->res_ok, OIVA_ERR_ARG, "shape does not qualify for the X-resident iteration");
    char* peers[OIVA_XCHG_MAX_RANKS];
    int rank = 0, world = 1;
    size_t slot = 0;
    OIVA_NEED(xchg_peers(x, peers, &rank, &world, &slot) == 0, OIVA_ERR_STATE, "exchange not connected");
    const size_t want = (size_t)p->rg.NS * p->rg.TW * p->K * sizeof(float);
    OIVA_NEED(slot == want, OIVA_ERR_ARG, "exchange slot size must be frame_splits * frames_per_split * K * 4 bytes of THIS plan "
                                     "(every rank must run the same split geometry)");
    for (int r = 0; r < OIVA_XCHG_MAX_RANKS; ++r) p->res_gath[r] = peers[r];
    p->res_rank = rank;
    p->res_world = world;
    return OIVA_OK;
}

int oiva_plan_resident_info(oiva_plan* p, int* info) {
    OIVA_NEED(p && info, OIVA_ERR_ARG, "null argument");
    const ResidentGeom& g = p->rg;
    const int v[OIVA_RESIDENT_INFO] = {p->res_ok ? 1 : 0, p->res_on ? 1 : 0, g.NB, g.NS, g.TW, g.J, g.JR, g.lds_bytes,
                                       p->res_last_code, p->res_launches, p->res_fallbacks, g.J * kBlock * p->M * 8};
    for (int i = 0; i < OIVA_RESIDENT_INFO; ++i) info[i] = v[i];
    return OIVA_OK;
}

int oiva_plan_resident_phases(oiva_plan* p, double* phase_us, int* n_iter) {
    OIVA_NEED(p && phase_us && n_iter, OIVA_ERR_ARG, "null argument");
    for (int i = 0; i < OIVA_RESIDENT_PHASES; ++i) phase_us[i] = 0.;
    *n_iter = 0;
    if (!p->res_stamps || p->res_stamped <= 0) return OIVA_OK;
    DeviceGuard guard(p->device);
    const int n = p->res_stamped;
    std::vector<unsigned long long> st((size_t)n * kResidentStamps);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(st.data(), p->res_stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    static_assert(OIVA_RESIDENT_PHASES <= kResidentStamps - 1, "one phase between consecutive stamps");
    for (int it = 0; it < n; ++it)
        for (int i = 0; i < OIVA_RESIDENT_PHASES; ++i)
            phase_us[i] += (double)(st[(size_t)it * kResidentStamps + i + 1] - st[(size_t)it * kResidentStamps + i]) * 0.01 / n;   // 100 MHz ticks
    *n_iter = n;
    return OIVA_OK;
}

int oiva_plan_resident_trace(oiva_plan* p, int enable, unsigned long long* stamps_host, int* n_wg, int* n_iter) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    DeviceGuard guard(p->device);
    p->res_trace = enable != 0;
    if (n_wg) *n_wg = p->rg.NB * p->rg.NS;
    if (n_iter) *n_iter = p->res_trace_buf ? p->res_trace_iters : 0;
    if (stamps_host && p->res_trace_buf) {
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        OIVA_TRY_HIP(hipMemcpy(stamps_host, p->res_trace_buf,
                          (size_t)p->rg.NB * p->rg.NS * p->res_trace_iters * kResidentStamps * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return OIVA_OK;
}

int oiva_plan_resident_debug(oiva_plan* p, int timeout_ms, int stall_block) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    p->res_timeout_ms = timeout_ms;
    p->res_stall = stall_block;
    p->res_stall_iter = 0;
    return OIVA_OK;
}

int oiva_plan_resident_debug_from(oiva_plan* p, int timeout_ms, int stall_block, int first_stalled_iteration) {
    OIVA_NEED(p && first_stalled_iteration >= 0, OIVA_ERR_ARG, "bad arguments");
    p->res_timeout_ms = timeout_ms;
    p->res_stall = stall_block;
    p->res_stall_iter = first_stalled_iteration;
    return OIVA_OK;
}

// ---- OGIVE (reference ive.py:33-256) ----------------------------------------------------------------
int oiva_plan_ogive_begin(oiva_plan* p, int update_mode, int model) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->M <= kNarrowMax, OIVA_ERR_ARG, "OGIVE runs on 1..16 channels (its per-bin state is sized for them)");
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(p->K == 1, OIVA_ERR_ARG, "OGIVE extracts one source: create the plan with K = 1");
    OIVA_NEED(p->F == p->F_total, OIVA_ERR_STATE, "OGIVE is not bin-sharded");
    OIVA_NEED(update_mode >= OIVA_OGIVE_DEMIX && update_mode <= OIVA_OGIVE_SWITCHING, OIVA_ERR_ARG, "unknown update mode");
    OIVA_NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    DeviceGuard guard(p->device);
    const size_t F = p->F, M = p->M;
    if (!p->og.maxdelta) {               // (the last of the state: all of it or none)
        const size_t before = p->mem.mark();
        alloc_ogive_state(p->og, F, M, p->mem);
        if (!p->mem.ok()) {
            p->mem.release_to(before);
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(p->mem.status()));
        }
    }
    if (!p->what64_valid) {              // the step kernel reads and writes the complex128 copy of w
        std::vector<double2> wh;
        if ((rc = download_what(p, wh)) || (rc = upload_what(p, wh))) return rc;
    }
    if (p->og_graph) {                   // a cached chunk of epochs was captured for the previous update mode / model
        OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
        OIVA_TRY_HIP(hipGraphExecDestroy(p->og_graph));
        p->og_graph = nullptr;
    }
    p->og.Cx = p->Cx;
    p->og.What = p->What;
    p->og.What64 = p->What64;
    p->og_mode = update_mode;
    p->og_model = model;
    OIVA_TRY_HIP(launch_ogive_init(p->stream, p->og, p->F, p->M, update_mode));
    p->og_ready = true;
    return OIVA_OK;
}

int oiva_plan_ogive_iterate(oiva_plan* p, int first_epoch, int n, double step_size, double tol, int* epochs_run,
                            int* converged, double* max_delta) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(p->og_ready, OIVA_ERR_STATE, "call oiva_plan_ogive_begin first");
    OIVA_NEED(n >= 0 && first_epoch >= 0, OIVA_ERR_ARG, "negative epoch count");
    DeviceGuard guard(p->device);
    int before[2] = {0, 0};
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(before, p->og.ctrl, sizeof(before), hipMemcpyDeviceToHost));
    const int amodel = p->og_model == OIVA_MODEL_LAPLACE ? kModelOgiveLaplace : OIVA_MODEL_GAUSS;
    auto epochs = [&](int e0, int count) -> int {
        for (int e = e0; e < e0 + count; ++e) {
            if (p->og_mode == OIVA_OGIVE_SWITCHING && e % 10 == 0) OIVA_TRY_HIP(launch_ogive_switch(p->stream, p->og, p->F, p->M));   // ive.py:192-193
            int r = stage_power(p);                                                             // ive.py:196 + the norm of :210/:213
            if (r) return r;
            OIVA_TRY_HIP(launch_activation(p->stream, p->Ppart, p->pw.nb, p->R, p->T, 1, amodel, p->F));   // ive.py:209-217 (floor + 1/r in the consumer)
            OIVA_TRY_HIP(launch_cov(p->stream, p->X, p->X_pad, p->R, p->Plocal, p->wscale, p->model, /*raw: weights 1 / max(r, eps)*/ 1, p->Vpart,
                               p->cov_f64(), p->T, p->F, p->M, 1, cov_geom_now(p)));           // ive.py:221-227
            OIVA_TRY_HIP(launch_ogive_step(p->stream, p->og, p->Vpart, p->vpart_f64(), p->cov.nsplit, p->T, p->F, p->M, step_size,
                                      tol));                                                     // ive.py:228-246
        }
        return OIVA_OK;
    };
    constexpr int kMinGraphEpochs = 8;
    if (n >= kMinGraphEpochs) {
        // a chunk of n epochs as one hipGraph, cached while (n, position in the 10-epoch switching cadence, step
        // size, tolerance) stay the same -- the usual case: the host runs equal chunks until the rule is met
        const int phase = first_epoch % 10;
        if (!p->og_graph || p->og_graph_n != n || p->og_graph_phase != phase || p->og_graph_mu != step_size ||
            p->og_graph_tol != tol) {
            if (p->og_graph) OIVA_TRY_HIP(hipGraphExecDestroy(p->og_graph));
            p->og_graph = nullptr;
            rc = capture_graph(p->stream, [&] { return epochs(phase, n); }, &p->og_graph, false);
            if (rc) return rc;
            p->og_graph_n = n;
            p->og_graph_phase = phase;
            p->og_graph_mu = step_size;
            p->og_graph_tol = tol;
        }
        OIVA_TRY_HIP(hipGraphLaunch(p->og_graph, p->stream));
    } else if ((rc = epochs(first_epoch, n))) {
        return rc;
    }
    p->wscale_pending = false;
    int after[2] = {0, 0};
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(after, p->og.ctrl, sizeof(after), hipMemcpyDeviceToHost));
    if (epochs_run) *epochs_run = after[1] - before[1];
    if (converged) *converged = after[0];
    if (max_delta) OIVA_TRY_HIP(hipMemcpy(max_delta, p->og.maxdelta, sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

// ---- test-only stage access -----------------------------------------------------------------------
int oiva_test_set_rinv(oiva_plan* p, const float* rinv_host) {
    OIVA_NEED(p && rinv_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    // the device keeps r, not 1/r: store the reciprocal and tell the covariance pass to skip gamma
    std::vector<float> r((size_t)p->T * p->K);
    for (size_t i = 0; i < r.size(); ++i) r[i] = 1.f / rinv_host[i];
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(p->R, r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice));
    p->raw_weights = 1;
    return OIVA_OK;
}

int oiva_test_get_rinv(oiva_plan* p, float* rinv_host, float* wscale_host) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    if (rinv_host) {
        // same formula as oiva::activation_weight on the r the device holds
        const int T = p->T, K = p->K;
        std::vector<float> r((size_t)T * K);
        OIVA_TRY_HIP(hipMemcpy(r.data(), p->R, r.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 0; k < K; ++k) {
            double s = 0.;
            for (int t = 0; t < T; ++t) s += (double)r[(size_t)t * K + k];
            const float ginv = p->raw_weights ? 1.f : 1.f / (float)(s / (double)T);
            for (int t = 0; t < T; ++t) {
                float rn = r[(size_t)t * K + k] * ginv;
                rn = rn < 1e-15f ? 1e-15f : rn;
                rinv_host[(size_t)t * K + k] = 1.f / rn;
            }
        }
    }
    if (wscale_host) OIVA_TRY_HIP(hipMemcpy(wscale_host, p->wscale, (size_t)p->K * sizeof(float), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

int oiva_test_run_weighted_cov(oiva_plan* p) {
    OIVA_NEED(p, OIVA_ERR_ARG, "null plan");
    OIVA_NEED(p->have_x, OIVA_ERR_STATE, "X not set");
    DeviceGuard guard(p->device);
    int rc = ensure_pad(p);
    if (rc) return rc;
    return stage_cov(p);
}

int oiva_test_get_v(oiva_plan* p, void* V_host, int f64) {
    OIVA_NEED(p && V_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    const int F = p->F, M = p->M, K = p->K;
    const long long nfk = (long long)F * K * M * M;
    OIVA_TRY_HIP(launch_sum_parts(p->stream, p->Vpart, p->vpart_f64(), p->cov.nsplit, p->scratch_p, nfk, 1. / (double)p->T));
    OIVA_TRY_HIP(launch_unpack_herm(p->stream, p->scratch_p, p->scratch_c, f64 != 0, (long long)F * K, M));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    const size_t esz = f64 ? sizeof(double2) : sizeof(float2);
    std::vector<char> fk((size_t)nfk * esz);
    OIVA_TRY_HIP(hipMemcpy(fk.data(), p->scratch_c, fk.size(), hipMemcpyDeviceToHost));
    // device order is [F][K][M][M]; the oracle's is (K, F, M, M)
    char* out = (char*)V_host;
    const size_t mm = (size_t)M * M * esz;
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < K; ++k)
            std::memcpy(out + ((size_t)k * F + f) * mm, fk.data() + ((size_t)f * K + k) * mm, mm);
    return OIVA_OK;
}

int oiva_test_run_update(oiva_plan* p) {
    int rc = check_ready(p);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    return stage_update(p, false);
}

int oiva_test_get_what(oiva_plan* p, void* What_host, int f64) {
    OIVA_NEED(p && What_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    std::vector<double2> wh;
    int rc = download_what(p, wh);
    if (rc) return rc;
    if (f64) {
        std::memcpy(What_host, wh.data(), wh.size() * sizeof(double2));
    } else {
        float2* o = static_cast<float2*>(What_host);
        for (size_t i = 0; i < wh.size(); ++i) o[i] = make_float2((float)wh[i].x, (float)wh[i].y);
    }
    return OIVA_OK;
}

int oiva_test_set_what(oiva_plan* p, const void* What_host, int f64) {
    OIVA_NEED(p && What_host, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(p->device);
    std::vector<double2> wh((size_t)p->F * p->M * p->M);
    if (f64) {
        std::memcpy(wh.data(), What_host, wh.size() * sizeof(double2));
    } else {
        const float2* in = static_cast<const float2*>(What_host);
        for (size_t i = 0; i < wh.size(); ++i) wh[i] = make_double2(in[i].x, in[i].y);
    }
    int rc = upload_what(p, wh);
    if (rc) return rc;
    p->have_w = true;
    p->wscale_pending = false;
    return OIVA_OK;
}

int oiva_test_time_stage(oiva_plan* p, int stage, int reps, float* avg_ms) {
    int rc = check_ready(p);
    if (rc) return rc;
    OIVA_NEED(reps >= 1 && avg_ms && stage >= 0 && stage < OIVA_N_STAGES, OIVA_ERR_ARG, "bad arguments");
    DeviceGuard guard(p->device);
    auto run = [&]() -> int {
        switch (stage) {
            case 0: return stage_power(p);
            case 1: return stage_activation(p, p->Ppart, p->pw.nb);
            case 2: return cov_update_applies(p) ? stage_cov_update(p) : stage_cov(p);      // (one launch for both where the plan runs it so)
            default: return cov_update_applies(p) ? OIVA_OK : stage_update(p, false);
        }
    };
    if ((rc = run())) return rc;  // warm
    float ms = 0.f;
    rc = p->stream.elapsed_ms(0, 1, [&] {
        int r = OIVA_OK;
        for (int i = 0; i < reps && r == OIVA_OK; ++i) r = run();
        return r;
    }, &ms);
    if (rc) return rc;
    *avg_ms = ms / reps;
    return OIVA_OK;
}

int oiva_test_run_power(oiva_plan* p, float* p_host) {
    OIVA_NEED(p && p_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(p->have_x && p->have_w, OIVA_ERR_STATE, "X / W not set");
    DeviceGuard guard(p->device);
    int rc = stage_power(p);
    if (rc) return rc;
    const size_t n = (size_t)p->T * p->K;
    OIVA_TRY_HIP(launch_sum_parts(p->stream, p->Ppart, false, p->pw.nb, p->scratch_p, (long long)n, 1.));
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    std::vector<double> sum(n);
    OIVA_TRY_HIP(hipMemcpy(sum.data(), p->scratch_p, n * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) p_host[i] = (float)sum[i];
    return OIVA_OK;
}

int oiva_test_get_ppart(oiva_plan* p, float* parts_host, int* nparts) {
    OIVA_NEED(p && nparts, OIVA_ERR_ARG, "null argument");
    *nparts = p->pw.nb;
    if (!parts_host) return OIVA_OK;
    DeviceGuard guard(p->device);
    OIVA_TRY_HIP(hipStreamSynchronize(p->stream));
    OIVA_TRY_HIP(hipMemcpy(parts_host, p->Ppart, (size_t)p->pw.nb * p->T * p->K * sizeof(float), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

int oiva_test_power_order(int nsplit, int tcp, int cov_splits, int cov_tc, int* order) {
    OIVA_NEED(order && nsplit >= 1 && tcp >= 1 && cov_splits >= 1 && cov_tc >= 1, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(cov_splits <= kPowOrderMaxSplits, OIVA_ERR_ARG, "more covariance splits than the order table holds");
    const PowOrder o = make_pow_order(nsplit, tcp, cov_splits, cov_tc);
    for (int y = 0; y < nsplit; ++y) order[y] = power_chunk_tail_first(y, nsplit, o);
    return OIVA_OK;
}

int oiva_test_x_policy(int T, int F, int M, int cov_tc, int pow_tcp, double budget_mb, int* out, signed char* cov_walk, signed char* pow_walk) {
    OIVA_NEED(out && cov_walk && pow_walk && T >= 1 && F >= 1 && M >= 1 && cov_tc >= 1 && pow_tcp >= 1, OIVA_ERR_ARG, "bad arguments");
    CovGeom cg{};
    cg.tc = cov_tc, cg.nsplit = ceil_div(T, cov_tc);
    PowGeom pg{};
    pg.tcp = pow_tcp, pg.nsplit = ceil_div(T, pow_tcp);
    const XPolicy x = choose_x_policy(budget_mb, T, F, M, false, cg, pg);
    out[0] = x.n16, out[1] = x.nt ? 1 : 0, out[2] = (int)x.why;
    // every frame as the steps of the two kernels meet it: -1 never, 0 plain, 1 nt, 2 more than once or by two policies
    std::fill(cov_walk, cov_walk + T, (signed char)-1);
    std::fill(pow_walk, pow_walk + T, (signed char)-1);
    auto mark = [T](signed char* walk, int t, int frames, bool plain) {
        for (int u = t; u < std::min(T, t + frames); ++u) walk[u] = walk[u] == -1 ? (plain ? 0 : 1) : 2;
    };
    const int xplain = x.xplain();
    for (int t_begin = 0; t_begin < T; t_begin += cov_tc)            // cov_dma_kernel: step i of a split is its frame group i
        for (int i = 0; t_begin + 16 * i < std::min(T, t_begin + cov_tc); ++i)
            mark(cov_walk, t_begin + 16 * i, std::min(16, cov_tc - 16 * i), x_group_plain(kXGroup * i, xplain));
    for (int t_begin = 0; t_begin < T; t_begin += pow_tcp) {         // power_kernel: steps of 4 frames, offsets as the kernel forms them
        const int off0 = t_begin % cov_tc;
        for (int tl = 0; t_begin + tl < std::min(T, t_begin + pow_tcp); tl += 4)
            mark(pow_walk, t_begin + tl, std::min(4, pow_tcp - tl), !x.nt || x_group_plain(x_split_offset(off0, tl, cov_tc), xplain));
    }
    return OIVA_OK;
}

int oiva_test_x_choice(int T, int F, int M, int prec_flags, int cov_kind, int cov_tc, int pow_kind, int pow_tcp, double budget_mb, int from_env, int* out,
                       double* budget_used) {
    OIVA_NEED(out && T >= 1 && F >= 1 && M >= 1 && cov_tc >= 1 && pow_tcp >= 1, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(cov_kind >= 0 && cov_kind < kCovKinds && pow_kind >= 0 && pow_kind < kPowKinds, OIVA_ERR_ARG, "unknown kernel kind");
    if (from_env) {      // what a plan created now would start with
        const char* x = std::getenv("OIVA_X_RESIDENT_MB");
        budget_mb = x && x[0] ? std::atof(x) : kXResidentDefaultMB;
    }
    CovGeom cg{};
    cg.kind = (CovKind)cov_kind, cg.tc = cov_tc, cg.nsplit = ceil_div(T, cov_tc);
    PowGeom pg{};
    pg.kind = (PowKind)pow_kind, pg.tcp = pow_tcp, pg.nsplit = ceil_div(T, pow_tcp);
    const XPolicy x = choose_x_policy(budget_mb, T, F, M, (prec_flags & OIVA_PREC_COV_F64) != 0, cg, pg);
    out[0] = x.n16, out[1] = x.nt ? 1 : 0, out[2] = (int)x.why;
    if (budget_used) *budget_used = budget_mb;
    return OIVA_OK;
}

int oiva_test_cov_rows(int T, int F, int M, int prec_flags, int cov_kind, int cov_tc, int pow_kind, int pow_tcp, double budget_mb, int rows_on, int* rows) {
    OIVA_NEED(rows && T >= 1 && F >= 1 && M >= 1 && cov_tc >= 1 && pow_tcp >= 1, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(cov_kind >= 0 && cov_kind < kCovKinds && pow_kind >= 0 && pow_kind < kPowKinds, OIVA_ERR_ARG, "unknown kernel kind");
    CovGeom cg{};
    cg.kind = (CovKind)cov_kind, cg.tc = cov_tc, cg.nsplit = ceil_div(T, cov_tc);
    PowGeom pg{};
    pg.kind = (PowKind)pow_kind, pg.tcp = pow_tcp, pg.nsplit = ceil_div(T, pow_tcp);
    *rows = cov_rows_form(choose_x_policy(budget_mb, T, F, M, (prec_flags & OIVA_PREC_COV_F64) != 0, cg, pg), rows_on != 0) ? 1 : 0;
    return OIVA_OK;
}

int oiva_test_cov_blocks_per_cu(int M, int kc, int rows, int* n) {
    OIVA_NEED(n && M >= 1 && M <= 8 && kc >= 1, OIVA_ERR_ARG, "bad arguments");
    OIVA_TRY_HIP(cov_blocks_per_cu(M, kc, false, n, rows != 0));
    return OIVA_OK;
}

int oiva_test_kernel_choice(int device, int T, int F, int F_total, int M, int K, int prec_flags, int quad_on, int hmfma_on,
                            int cov_splits_req, int pow_splits_req, int* out) {
    OIVA_NEED(out && T >= 1 && F >= 1 && F_total >= F && M >= 1 && M <= OIVA_MAX_CHANNELS && K >= 1 && K <= M, OIVA_ERR_ARG, "bad arguments");
    OIVA_NEED(cov_splits_req >= 0 && pow_splits_req >= 0, OIVA_ERR_ARG, "bad split count");
    DeviceGuard guard(device);
    oiva_plan p;      // (a plan's fields, nothing allocated: what choice_in reads)
    p.device = device, p.T = T, p.F = F, p.F_total = F_total, p.M = M, p.K = K, p.prec = prec_flags;
    p.cov_quad_on = quad_on != 0, p.cov_hmfma_on = hmfma_on != 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) p.n_cu = prop.multiProcessorCount;
    int asked[2] = {-1, -1};
    const ChoiceIn c = choice_in(&p);
    const CovGeom g = choose_cov(c, device_occupancy(asked), cov_splits_req);
    const PowGeom w = choose_pow(c, device_occupancy(asked), pow_splits_req);
    const int o[18] = {(int)g.kind, g.nsplit, g.tc, g.kc, g.nbg, g.pad, g.part32, partials_f64(g, c.cov_f64) ? 1 : 0, (int)traits(g.kind).unit,
                       (int)w.kind, w.nb, w.nsplit, w.tcp, w.kp, w.rounds, asked[0], asked[1], p.n_cu};
    std::copy(o, o + 18, out);
    return OIVA_OK;
}

int oiva_test_update_choice(int M, int K, int use_double, int vpart_f64, int init_only, int layout, int nsplit, char* name, int n) {
    OIVA_NEED(name && n > 1 && M >= 1 && M <= OIVA_MAX_CHANNELS && K >= 1 && K <= M && nsplit >= 1, OIVA_ERR_ARG, "bad arguments");
    UpdateArgs a{};      // (every pointer null: the launch is captured, never run)
    a.vpart_f64 = vpart_f64 ? 1 : 0, a.nsplit = nsplit, a.T = 16, a.F = 1, a.M = M, a.K = K;
    a.init_only = init_only ? 1 : 0, a.use_double = use_double ? 1 : 0, a.layout = layout ? 1 : 0;
    hipStream_t s = nullptr;
    OIVA_TRY_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    const hipError_t launched = e == hipSuccess ? launch_update(s, a) : e;
    if (e == hipSuccess) e = hipStreamEndCapture(s, &graph);
    if (e == hipSuccess) e = launched;
    std::string mangled;
    size_t kernels = 0;
    if (e == hipSuccess) {
        size_t nodes = 0;
        e = hipGraphGetNodes(graph, nullptr, &nodes);
        std::vector<hipGraphNode_t> node(nodes);
        if (e == hipSuccess && nodes) e = hipGraphGetNodes(graph, node.data(), &nodes);
        for (size_t i = 0; e == hipSuccess && i < nodes; ++i) {
            hipGraphNodeType type;
            hipKernelNodeParams kp{};
            if ((e = hipGraphNodeGetType(node[i], &type)) != hipSuccess || type != hipGraphNodeTypeKernel) continue;
            if ((e = hipGraphKernelNodeGetParams(node[i], &kp)) != hipSuccess) break;
            const char* nm = hipKernelNameRefByPtr(kp.func, s);
            mangled = nm ? nm : "";
            ++kernels;
        }
    }
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipStreamDestroy(s);
    OIVA_TRY_HIP(e);
    OIVA_NEED(kernels == 1 && !mangled.empty(), OIVA_ERR_STATE, "the captured update is not one named kernel launch");
    // the normal form of kernel_choice.h: the demangled name without return type, namespaces and parameter list
    int status = 0;
    char* dem = abi::__cxa_demangle(mangled.c_str(), nullptr, nullptr, &status);
    std::string nm = status == 0 && dem ? dem : mangled;
    std::free(dem);
    for (const char* drop : {"(anonymous namespace)::", "oiva::", "void "})
        for (size_t at; (at = nm.find(drop)) != std::string::npos;) nm.erase(at, std::strlen(drop));
    nm = nm.substr(0, nm.find('('));
    OIVA_NEED((int)nm.size() < n, OIVA_ERR_ARG, "name buffer too small");
    std::memcpy(name, nm.c_str(), nm.size() + 1);
    return OIVA_OK;
}

}  // extern "C"
