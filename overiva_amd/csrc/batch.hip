// C ABI of the batched iteration (oiva_batch_*, include/overiva_hip.h): B problems of one F, M <= 8 and K and of T_b frames each,
// packed along the frames, in the `precise` arithmetic.  Host code only.  Every batch is described by one table of per-problem
// records (RaggedProblem): oiva_batch_create makes the table of B equal lengths, oiva_batch_create_ragged that of the lengths it
// is given, and allocation, X, demix and the grid maxima follow from the table alone.  The two entries differ in the kernels
// of the iteration: a batch of oiva_batch_create runs those of kernels_batch.hip, which take T and the splits of record 0 as
// launch arguments (measured 1-4 % faster per stage than reading the table, CHANGELOG), a batch of oiva_batch_create_ragged
// those of kernels_ragged.hip, which read the table on the device.  The per-bin stages are the single-problem kernels run on
// B*F bins.  Batched OGIVE (oiva_batch_ogive_*) runs on a batch of oiva_batch_create with K = 1, with its own kernels
// (kernels_ogive_batch.hip) and a stopping rule per problem.  Batched ILRMA (oiva_batch_ilrma_*) runs on a batch of
// oiva_batch_create with K = M: its NMF stages and its covariance pass are kernels_ilrma_batch.hip, its per-bin step the update.
// Batched ISS (oiva_batch_iss_*) runs on a batch of either entry with K = M: determined AuxIVA by rank-1 updates of the demixed
// signals, its two stages are kernels_iss_batch.hip, which read the table.
// Batched FIVE (oiva_batch_five_*) runs on a batch of either entry with K = 1: the first three stages of the iteration, then the
// smallest eigenpair of every bin's pencil (V, Cx) in place of the update (kernels_five_batch.hip, which reads the table).
// Batched IP2 (oiva_batch_ip2_*) runs on a batch of either entry with any K <= M: the float64 stages on a complex128 copy of X, then
// the pairwise update of kernels_ip2_batch.hip in place of the IP1 update.
// The PCA front end of auxiva_pca_batch (oiva_batch_set_w_pca,
// _project_dev, _compose_w; kernels_pca_batch.hip) reads the table on the device for every batch.
// A batch of either entry put into the complex128 data path (oiva_batch_set_data_c128, before X is set) holds X as complex128 and
// runs the stages of kernels_batch_c128.hip, which read the table, in float64; the per-bin update stays the shared one.
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "host_io.h"
#include "host_util.h"
#include "oiva_internal.h"

using namespace oiva;

namespace {

constexpr int kBatchMaxChannels = 8;
constexpr int kCovFramesPerSplit = 256;   // frame splits of the covariance pass: ceil(T / 256), a function of T alone
constexpr int kPowFramesPerSplit = 64;    // frame splits of the power pass (each partial power is one workgroup's: any split gives the same bits)
constexpr int kGraphMaxIters = 32;        // longest captured graph: an iterate(n) call is ceil(n / 32) replays
constexpr int kGraphCache = 4;
constexpr int kOgFramesPerSplit = 64;     // frame splits of the OGIVE frame sums: ceil(T / 64), a function of T alone
constexpr int kOgMinGraphEpochs = 8;      // shorter OGIVE chunks run eagerly
constexpr int kIlrmaMaxComponents = 16;
constexpr int kIlrmaStages = OIVA_ILRMA_STAGE_NORMALISE + 1;
constexpr int kIssStages = OIVA_ISS_STAGE_SWEEP + 1;
constexpr int kFiveStages = OIVA_FIVE_STAGE_UPDATE + 1;
constexpr int kIp2Stages = OIVA_IP2_STAGE_UPDATE + 1;

// geometry of the frame-split passes of a problem of T frames: a function of T alone (never of B or of other problems), so a
// problem gets the same bits whatever batch it is in
struct FrameGeom {
    int nsplit, tc;          // covariance pass
    int tcp, pw_nsplit;      // power pass
};
FrameGeom frame_geom(int T) {
    FrameGeom g;
    g.nsplit = ceil_div(T, kCovFramesPerSplit);
    g.tc = ceil_div(T, g.nsplit);
    g.nsplit = ceil_div(T, g.tc);
    g.tcp = round_up(ceil_div(T, ceil_div(T, kPowFramesPerSplit)), 4);
    g.pw_nsplit = ceil_div(T, g.tcp);
    return g;
}

}  // namespace

struct oiva_batch {
    int device = 0;
    int B = 0, T = 0, F = 0, M = 0, K = 0, model = 0;
    HandleStream stream;           // five events: one iteration's four stages (oiva_batch_time_stages), [0] and [1] any bracket
    DeviceArena mem;               // every device buffer below
    const float2* X = nullptr;     // (sum T_b, F, M) packed: (B, T, F, M) when the lengths are equal
    float2* X_owned = nullptr;
    float2* What = nullptr;        // (B*F, M, M) complex64: what the streaming kernels read
    double2* What64 = nullptr;     // (B*F, M, M) complex128: carried between iterations by the float64 update
    double* Cx = nullptr;          // [B*F][M*M] packed, / T
    double* Vpart = nullptr;       // [nsplit][B*F][K][M*M]
    float* Ppart = nullptr;        // problem b's [nb][T_b][K] at probs[b].p_off
    float* R = nullptr;            // problem b's activation buffer of r_buffer_bytes(T_b, K) at probs[b].r_off
    float* wscale = nullptr;       // (B, K)
    float* Spart = nullptr;        // [max stgs nsplit][F][K][3]: projection-back sums of one problem at a time
    float2* Y = nullptr;           // (sum T_b, F, K), allocated on first demix
    double2* Y128 = nullptr;
    // the complex128 data path (oiva_batch_set_data_c128, kernels_batch_c128.hip): X as the caller's complex128 and every stage in
    // float64; these replace X, Ppart, R, wscale and Spart, which are released; Y is Y128
    bool c128 = false;
    const double2* X128 = nullptr; // (sum T_b, F, M) packed
    double2* X128_owned = nullptr;
    double* Ppart64 = nullptr;     // problem b's [nb][T_b][K] at probs[b].p_off (doubles)
    double* Rw64 = nullptr;        // (sum T_b, K): r, then the weights 1 / max(r / gamma, eps)
    double* Gs64 = nullptr;        // [B][rblocks][K]: sums of r over blocks of kBlock frames
    double2* Z128 = nullptr;       // (B*F, K): projection-back scales
    float2* Xr = nullptr;          // (sum T_b, F, K): X projected onto the principal subspace (oiva_batch_project_dev), allocated on first use
    // T is the largest T_b, and nsplit / pw_nsplit / tcp / rblocks the largest over the problems (the grids); every problem's own
    // geometry is in its record (host copy `probs`, device copy `probs_dev`) and stgs[p] is its projection-back statistics
    // geometry (the single-problem plan's for F bins)
    int nsplit = 1;                // covariance pass
    int kp = 1, pw_nsplit = 1, tcp = 4, nb = 1;   // power pass
    int rblocks = 1;               // activation: largest rsum_blocks(T_b)
    size_t frames_total = 0;       // sum of T_b
    std::vector<RaggedProblem> probs;
    std::vector<CovGeom> stgs;
    RaggedProblem* probs_dev = nullptr;
    bool ragged = false;           // made by oiva_batch_create_ragged: the kernels that read the table (dense_args otherwise)
    bool have_x = false, have_cx = false, have_w = false;
    GraphCache graphs{kGraphCache};    // by iterations per replay
    // batched OGIVE (ive.py:33-256): per-bin state of B*F bins and the per-problem stopping rule, allocated by ogive_begin
    OgiveBatchState og{};
    double* Opart = nullptr;       // [osplit][B*F][2M+1] frame-sum partials
    int osplit = 1, otc = 1;
    bool og_ready = false;
    int og_mode = 0, og_model = 0;
    // captured chunk of epochs, cached on (n, phase in the 10-epoch switching cycle, step size, tol) as the single plan's
    hipGraphExec_t og_graph = nullptr;
    int og_graph_n = 0, og_graph_phase = -1;
    double og_graph_mu = 0., og_graph_tol = 0.;
    // batched ILRMA: the NMF state (Tn, Vn), the source models R and the powers P, allocated by ilrma_begin
    IlrmaState il{};
    bool il_ready = false;
    // batched ISS: the group partial powers, the activations r and the weights, allocated by iss_begin
    double* iss_part = nullptr;    // room b's [groups_b][T_b][M] at x_off_b * iss_groups * M
    double* iss_rw = nullptr;      // (sum T_b, M): r
    double* iss_phi = nullptr;     // (sum T_b, M): the weights
    int iss_groups = 0;            // the grid: the most groups of any room
    size_t iss_slab = 0;           // the largest group slab, bytes of dynamic LDS
    bool iss_ready = false;
    // batched FIVE: the reduction of every bin's Cx, formed by five_begin
    double2* five_li = nullptr;    // (B*F, M, M): L^-1 of Cx = L L^H
    double2* five_x128 = nullptr;  // (sum T_b, F, M): X widened to complex128, what the float64 stages of FIVE stream (with
                                   // Ppart64, Rw64 and Gs64, which a complex64 batch does not hold otherwise)
    bool five_ready = false;
    // batched IP2: what its float64 stages stream and leave, allocated by the first oiva_batch_ip2_* call
    double2* ip2_x128 = nullptr;   // (sum T_b, F, M): X widened to complex128
    double* ip2_ppart = nullptr;   // room b's [nb][T_b][K] at probs[b].p_off (doubles)
    double* ip2_rw = nullptr;      // (sum T_b, K): r, then the weights 1 / max(r / gamma, eps)
    double* ip2_gs = nullptr;      // [B][rblocks][K]: sums of r over blocks of kBlock frames
    bool ip2_ready = false;        // ip2_x128 holds the X that is set
};

namespace {

size_t nbins(const oiva_batch* b) { return (size_t)b->B * b->F; }

int drop_graphs(oiva_batch* b) {
    const int rc = b->graphs.clear();
    if (rc) return rc;
    if (b->og_graph) {
        hipGraphExec_t g = b->og_graph;
        b->og_graph = nullptr;
        OIVA_TRY_HIP(hipGraphExecDestroy(g));
    }
    return OIVA_OK;
}

UpdateArgs update_args(oiva_batch* b, bool init_only) {
    UpdateArgs a;
    a.What = b->What;
    a.What64 = b->What64;
    a.Cx = b->Cx;
    a.Vpart = b->Vpart;
    a.vpart_f64 = 1;
    a.wscale = init_only || b->c128 ? nullptr : b->wscale;     // (complex128 data: the scale is applied in float64 by the activation)
    a.nsplit = b->nsplit;
    a.T = b->T;
    a.F = (int)nbins(b);
    a.M = b->M;
    a.K = b->K;
    a.init_only = init_only ? 1 : 0;
    a.use_double = 1;
    a.layout = 0;
    a.wscale_bins = b->F;
    a.ragged = b->ragged || b->c128 ? b->probs_dev : nullptr;
    return a;
}

// what the kernels of equal lengths take as launch arguments: record 0's frame count and splits, and the stride of the
// activation buffers
struct DenseArgs {
    int T, tc, tcp, pw_nsplit, nsplit;
    size_t r_stride;
};
DenseArgs dense_args(const oiva_batch* b) {
    const RaggedProblem& d = b->probs[0];
    return {d.T, d.tc, d.tcp, d.pw_nsplit, d.nsplit, r_buffer_bytes(d.T, b->K) / sizeof(float)};
}

// the four launches of one iteration (overiva.py:138-190); five with complex128 data, whose activation is two
int stage(oiva_batch* b, int s) {
    if (s == 3) {
        OIVA_TRY_HIP(launch_update(b->stream, update_args(b, false)));
    } else if (b->c128) {
        if (s == 0)
            OIVA_TRY_HIP(launch_c128_power(b->stream, b->X128, b->What64, b->Ppart64, b->probs_dev, b->B, b->T, b->F, b->M, b->K));
        else if (s == 1)
            OIVA_TRY_HIP(launch_c128_activation(b->stream, b->Ppart64, b->Rw64, b->Gs64, b->What64, b->What, b->probs_dev, b->B, b->T, b->F,
                                           b->M, b->K, b->model, b->rblocks));
        else
            OIVA_TRY_HIP(launch_c128_cov(b->stream, b->X128, b->Rw64, b->probs_dev, b->Vpart, b->B, b->F, b->M, b->K, b->nsplit));
    } else if (b->ragged) {
        if (s == 0)
            OIVA_TRY_HIP(launch_ragged_power(b->stream, b->X, b->What, b->Ppart, b->probs_dev, b->B, b->F, b->M, b->K, b->kp, b->pw_nsplit,
                                        b->tcp));
        else if (s == 1)
            OIVA_TRY_HIP(launch_ragged_activation(b->stream, b->Ppart, b->nb, b->R, b->probs_dev, b->B, b->K, b->model, b->F, b->rblocks));
        else
            OIVA_TRY_HIP(launch_ragged_cov(b->stream, b->X, b->R, b->probs_dev, b->wscale, b->model, b->Vpart, b->B, b->F, b->M, b->K,
                                      b->nsplit));
    } else {
        const DenseArgs d = dense_args(b);
        if (s == 0)
            OIVA_TRY_HIP(launch_batch_power(b->stream, b->X, b->What, b->Ppart, b->B, d.T, b->F, b->M, b->K, b->kp, d.pw_nsplit, d.tcp));
        else if (s == 1)
            OIVA_TRY_HIP(launch_batch_activation(b->stream, b->Ppart, b->nb, b->R, d.r_stride, b->B, d.T, b->K, b->model, b->F));
        else
            OIVA_TRY_HIP(launch_batch_cov(b->stream, b->X, b->R, d.r_stride, b->wscale, b->model, b->Vpart, b->B, d.T, b->F, b->M, b->K,
                                     d.nsplit, d.tc));
    }
    return OIVA_OK;
}

int one_iteration(oiva_batch* b) {
    for (int s = 0; s < 4; ++s) {
        const int rc = stage(b, s);
        if (rc) return rc;
    }
    return OIVA_OK;
}

// the executable graph of `iters` iterations on the batch's stream: one linear chain of 4 (complex128 data: 5) * iters kernel nodes
int graph_for(oiva_batch* b, int iters, hipGraphExec_t* out) {
    return b->graphs.get(b->stream, iters, [&] {
        int r = OIVA_OK;
        for (int i = 0; i < iters && r == OIVA_OK; ++i) r = one_iteration(b);
        return r;
    }, out);
}

int check_ready(oiva_batch* b) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(b->have_x, OIVA_ERR_STATE, "X not set (oiva_batch_set_x_host/_dev)");
    OIVA_NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    OIVA_NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set (oiva_batch_set_w)");
    return OIVA_OK;
}

// W_hat of every bin in complex128; W (its first K columns) into W_host (B, F, M, K) unless that is nullptr; bad (B): the problems
// whose W holds a non-finite value
int download_w(oiva_batch* b, void* W_host, int f64, std::vector<int>& bad) {
    std::vector<double2> wh(nbins(b) * b->M * b->M);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(wh.data(), b->What64, wh.size() * sizeof(double2), hipMemcpyDeviceToHost));
    bad.assign(b->B, 0);
    for (int p = 0; p < b->B; ++p) bad[p] = !unpack_w(wh, (size_t)p * b->F, (size_t)b->F, b->M, b->K, W_host, f64);
    return OIVA_OK;
}

// Y of every problem into the batch's own device array (allocated on first use), on the batch's stream
int demix_on_device(oiva_batch* b, int proj_back) {
    const int F = b->F, M = b->M, K = b->K;
    const size_t ny = b->frames_total * F * K;
    if (b->c128) {
        if (!b->Y128) OIVA_TRY_HIP(b->mem.take_one(&b->Y128, ny * sizeof(double2)));
        if (proj_back && !b->Z128) OIVA_TRY_HIP(b->mem.take_one(&b->Z128, nbins(b) * K * sizeof(double2)));
        OIVA_TRY_HIP(launch_c128_demix(b->stream, b->X128, b->What64, b->Z128, b->Y128, b->probs_dev, b->B, b->T, F, M, K, proj_back != 0));
        return OIVA_OK;
    }
    if (!b->Y) OIVA_TRY_HIP(b->mem.take_one(&b->Y, ny * sizeof(float2)));
    // overiva.py:192-199 per problem, with the single-problem kernels (projection back against that problem's X[b][:, :, 0]):
    // every problem at its packed frame offset with the statistics geometry of its own T_b
    for (int p = 0; p < b->B; ++p) {
        const int T = b->probs[p].T;
        const size_t t0 = b->probs[p].x_off;
        const CovGeom& stg = b->stgs[p];
        const float2* Xb = b->X + t0 * F * M;
        const float2* Wb = b->What + (size_t)p * F * M * M;
        if (proj_back) OIVA_TRY_HIP(launch_demix_stats(b->stream, Xb, Wb, b->Spart, T, F, M, K, stg));
        OIVA_TRY_HIP(launch_demix_write(b->stream, Xb, Wb, proj_back ? b->Spart : nullptr, stg.nsplit, b->Y + t0 * F * K, T, F, M, K));
    }
    return OIVA_OK;
}

// X of the batch is now the array at X (its own copy or the caller's): captured graphs hold the pointer, Cx is of the old one
int install_x(oiva_batch* b, const void* X) {
    if ((b->c128 ? (const void*)b->X128 : (const void*)b->X) != X) {
        OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
        const int rc = drop_graphs(b);
        if (rc) return rc;
    }
    if (b->c128)
        b->X128 = static_cast<const double2*>(X);
    else
        b->X = static_cast<const float2*>(X);
    b->have_x = true;
    b->have_cx = false;
    b->iss_ready = false;          // (its partial powers are of the old X)
    b->five_ready = false;         // (its reduction is of the old Cx)
    b->ip2_ready = false;          // (its complex128 copy is of the old X)
    return OIVA_OK;
}

// stream, events, the problem table and the buffers of a new batch of frames[p] frames per problem; whatever it made before a
// failure is the caller's to free
int fill_batch(oiva_batch* b, const std::vector<int>& frames, void* stream) {
    const int device = b->device, B = b->B, T = b->T, F = b->F, M = b->M, K = b->K;
    OIVA_TRY_HIP(b->stream.open(stream, 5));
    // every problem's record from its own T_b: functions of T_b, F, M, K alone (never of B); the grids (nsplit, pw_nsplit, tcp,
    // rblocks) take the largest
    b->kp = pow_sources_per_pass(M, K);
    b->nb = ceil_div(F, kBinsPerWave * kWaves);
    b->osplit = ceil_div(T, kOgFramesPerSplit);
    b->otc = ceil_div(T, b->osplit);
    b->osplit = ceil_div(T, b->otc);
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device);
    b->probs.resize(B);
    b->stgs.resize(B);
    int spart_splits = 1;
    size_t x_off = 0, p_off = 0, r_off = 0;
    for (int p = 0; p < B; ++p) {
        const int Tb = frames[p];
        const FrameGeom g = frame_geom(Tb);
        RaggedProblem& d = b->probs[p];
        d.x_off = x_off, d.p_off = p_off, d.r_off = r_off;
        d.inv_T = 1. / (double)Tb;
        d.T = Tb;
        d.tcp = g.tcp, d.pw_nsplit = g.pw_nsplit, d.nsplit = g.nsplit, d.tc = g.tc;
        x_off += Tb;
        p_off += (size_t)b->nb * Tb * K;
        r_off += r_buffer_bytes(Tb, K) / sizeof(float);
        b->stgs[p] = stats_geom(Tb, F, K, n_cu);
        b->nsplit = std::max(b->nsplit, g.nsplit);
        b->pw_nsplit = std::max(b->pw_nsplit, g.pw_nsplit);
        b->tcp = std::max(b->tcp, g.tcp);
        b->rblocks = std::max(b->rblocks, rsum_blocks(Tb));
        spart_splits = std::max(spart_splits, b->stgs[p].nsplit);
    }
    b->frames_total = x_off;
    const size_t ppart_floats = p_off, r_floats = r_off;
    OIVA_TRY_HIP(b->mem.take_one(&b->probs_dev, (size_t)B * sizeof(RaggedProblem)));
    OIVA_TRY_HIP(hipMemcpy(b->probs_dev, b->probs.data(), (size_t)B * sizeof(RaggedProblem), hipMemcpyHostToDevice));
    const size_t MM = (size_t)M * M;
    OIVA_TRY_HIP(b->mem.take_one(&b->What, nbins(b) * MM * sizeof(float2)));
    OIVA_TRY_HIP(b->mem.take_one(&b->What64, nbins(b) * MM * sizeof(double2)));
    OIVA_TRY_HIP(b->mem.take_one(&b->Cx, nbins(b) * MM * sizeof(double)));
    OIVA_TRY_HIP(b->mem.take_one(&b->Vpart, ((size_t)b->nsplit * nbins(b) * K * MM + 2) * sizeof(double)));   // sum_vpart reads idx + 1
    OIVA_TRY_HIP(b->mem.take_one(&b->Ppart, ppart_floats * sizeof(float)));
    OIVA_TRY_HIP(b->mem.take_one(&b->R, r_floats * sizeof(float)));
    OIVA_TRY_HIP(hipMemset(b->R, 0, r_floats * sizeof(float)));      // (the pad rows behind every problem's r)
    OIVA_TRY_HIP(b->mem.take_one(&b->wscale, (size_t)B * K * sizeof(float)));
    OIVA_TRY_HIP(b->mem.take_one(&b->Spart, (size_t)spart_splits * F * K * 3 * sizeof(float)));
    return OIVA_OK;
}

// one stage of an ILRMA epoch (OIVA_ILRMA_STAGE_*); an epoch is the stages in order
int ilrma_stage(oiva_batch* b, int s) {
    const DenseArgs d = dense_args(b);
    switch (s) {
        case OIVA_ILRMA_STAGE_T:
            OIVA_TRY_HIP(launch_ilrma_t(b->stream, b->il, b->B, d.T, b->F, b->K));
            break;
        case OIVA_ILRMA_STAGE_V:
            OIVA_TRY_HIP(launch_ilrma_v(b->stream, b->il, b->B, d.T, b->F, b->K));
            break;
        case OIVA_ILRMA_STAGE_R:
            OIVA_TRY_HIP(launch_ilrma_r(b->stream, b->il, b->B, d.T, b->F, b->K));
            break;
        case OIVA_ILRMA_STAGE_COV:
            OIVA_TRY_HIP(launch_ilrma_cov(b->stream, b->X, b->il, b->Vpart, b->B, d.T, b->F, b->M, d.nsplit, d.tc));
            break;
        case OIVA_ILRMA_STAGE_UPDATE: {
            UpdateArgs a = update_args(b, false);      // IP1 on V = C_s: no pending scale of W
            a.wscale = nullptr;
            OIVA_TRY_HIP(launch_update(b->stream, a));
            break;
        }
        case OIVA_ILRMA_STAGE_POWER:
            OIVA_TRY_HIP(launch_ilrma_power(b->stream, b->X, b->What64, b->il, b->B, d.T, b->F, b->M));
            break;
        case OIVA_ILRMA_STAGE_NORMALISE:
            OIVA_TRY_HIP(launch_ilrma_normalise(b->stream, b->il, b->What, b->What64, b->B, d.T, b->F, b->M));
            break;
        default:
            return fail_with(OIVA_ERR_ARG, "unknown ILRMA stage");
    }
    return OIVA_OK;
}

int check_ilrma(oiva_batch* b, bool begun) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->ragged, OIVA_ERR_ARG, "ILRMA is not supported on a ragged batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "ILRMA is not supported on a complex128 batch");
    const int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(b->K == b->M, OIVA_ERR_ARG, "ILRMA is determined: create the batch with K = M");
    if (begun) OIVA_NEED(b->il_ready, OIVA_ERR_STATE, "call oiva_batch_ilrma_begin first");
    return OIVA_OK;
}

// one stage of an ISS iteration (OIVA_ISS_STAGE_*); the sweep with n_steps of its M rank-1 steps
int iss_stage(oiva_batch* b, int s, int n_steps) {
    if (s == OIVA_ISS_STAGE_ACTIVATION)
        OIVA_TRY_HIP(launch_iss_activation(b->stream, b->iss_part, b->iss_rw, b->iss_phi, b->What64, b->What, b->probs_dev, b->B, b->T, b->F,
                                           b->M, b->model, b->iss_groups));
    else
        OIVA_TRY_HIP(launch_iss_sweep(b->stream, b->X, b->What64, b->What, b->iss_phi, b->iss_part, b->probs_dev, b->B, b->F, b->M,
                                      b->iss_groups, b->iss_slab, n_steps));
    return OIVA_OK;
}

int check_iss(oiva_batch* b, bool begun) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "ISS is not supported on a complex128 batch");
    OIVA_NEED(b->K == b->M, OIVA_ERR_ARG, "ISS is determined: create the batch with K = M");
    for (const RaggedProblem& d : b->probs)
        OIVA_NEED((long long)d.T * b->M <= kIssSlabElems, OIVA_ERR_ARG,
                  "ISS needs T * M <= " + std::to_string(kIssSlabElems) + " in every room (one bin's slab of 128 KiB of LDS)");
    OIVA_NEED(b->have_x, OIVA_ERR_STATE, "X not set (oiva_batch_set_x_host/_dev)");
    OIVA_NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set (oiva_batch_set_w)");
    if (begun) OIVA_NEED(b->iss_ready, OIVA_ERR_STATE, "call oiva_batch_iss_begin first");
    return OIVA_OK;
}

// one stage of a FIVE iteration (OIVA_FIVE_STAGE_*): the float64 stages 0 to 2 of stage() (the complex128 data path's, from the
// problem table) with K = 1 on the widened X, then the per-bin eigenpair in place of the IP1 update (the activation's scale of
// w does not matter: the step forms w afresh)
int five_stage(oiva_batch* b, int s) {
    if (s == OIVA_FIVE_STAGE_POWER)
        OIVA_TRY_HIP(launch_c128_power(b->stream, b->five_x128, b->What64, b->Ppart64, b->probs_dev, b->B, b->T, b->F, b->M, 1));
    else if (s == OIVA_FIVE_STAGE_ACTIVATION)
        OIVA_TRY_HIP(launch_c128_activation(b->stream, b->Ppart64, b->Rw64, b->Gs64, b->What64, b->What, b->probs_dev, b->B, b->T, b->F,
                                            b->M, 1, b->model, b->rblocks));
    else if (s == OIVA_FIVE_STAGE_COV)
        OIVA_TRY_HIP(launch_c128_cov(b->stream, b->five_x128, b->Rw64, b->probs_dev, b->Vpart, b->B, b->F, b->M, 1, b->nsplit));
    else
        OIVA_TRY_HIP(launch_five_update(b->stream, b->Vpart, b->five_li, b->What64, b->What, b->probs_dev, (int)nbins(b), b->F, b->M));
    return OIVA_OK;
}

int check_five(oiva_batch* b, bool begun) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "FIVE is not supported on a complex128 batch");
    OIVA_NEED(b->K == 1, OIVA_ERR_ARG, "FIVE extracts one source: create the batch with K = 1");
    const int rc = check_ready(b);
    if (rc) return rc;
    if (begun) OIVA_NEED(b->five_ready, OIVA_ERR_STATE, "call oiva_batch_five_begin first");
    return OIVA_OK;
}

// one stage of an IP2 iteration (OIVA_IP2_STAGE_*): the float64 stages 0 to 2 of stage() (the complex128 data path's, from the
// problem table) on the widened X, whose activation applies the scale of W in float64; then the schedule of `iteration`
int ip2_stage(oiva_batch* b, int s, int iteration) {
    if (s == OIVA_IP2_STAGE_POWER) {
        OIVA_TRY_HIP(launch_c128_power(b->stream, b->ip2_x128, b->What64, b->ip2_ppart, b->probs_dev, b->B, b->T, b->F, b->M, b->K));
    } else if (s == OIVA_IP2_STAGE_ACTIVATION) {
        OIVA_TRY_HIP(launch_c128_activation(b->stream, b->ip2_ppart, b->ip2_rw, b->ip2_gs, b->What64, b->What, b->probs_dev, b->B, b->T,
                                            b->F, b->M, b->K, b->model, b->rblocks));
    } else if (s == OIVA_IP2_STAGE_COV) {
        OIVA_TRY_HIP(launch_c128_cov(b->stream, b->ip2_x128, b->ip2_rw, b->probs_dev, b->Vpart, b->B, b->F, b->M, b->K, b->nsplit));
    } else {
        UpdateArgs a = update_args(b, false);
        a.wscale = nullptr;                  // (applied by the activation)
        a.ragged = b->probs_dev;             // every room's own T and splits, dense batch or not
        OIVA_TRY_HIP(launch_ip2_update(b->stream, a, iteration));
    }
    return OIVA_OK;
}

// the arguments and the state every oiva_batch_ip2_* entry needs; forms the complex128 copy of X on first use
int prepare_ip2(oiva_batch* b) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "IP2 is not supported on a complex128 batch");
    const int rc = check_ready(b);
    if (rc) return rc;
    if (b->ip2_ready) return OIVA_OK;
    DeviceGuard guard(b->device);
    const size_t nx = b->frames_total * b->F * b->M;
    if (!b->ip2_x128) {                  // (the last of the state: all of it or none)
        DeviceArena& mem = b->mem;
        const size_t before = mem.mark();
        size_t p_doubles = 0;
        for (const RaggedProblem& d : b->probs) p_doubles = std::max(p_doubles, d.p_off + (size_t)b->nb * d.T * b->K);
        mem.take(&b->ip2_ppart, p_doubles * sizeof(double));
        mem.take(&b->ip2_rw, b->frames_total * b->K * sizeof(double));
        mem.take(&b->ip2_gs, (size_t)b->B * b->rblocks * b->K * sizeof(double));
        mem.take(&b->ip2_x128, nx * sizeof(double2));
        if (!mem.ok()) {
            mem.release_to(before);
            b->ip2_ppart = b->ip2_rw = b->ip2_gs = nullptr, b->ip2_x128 = nullptr;
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
        }
    }
    OIVA_TRY_HIP(launch_cast_c64_to_c128(b->stream, b->X, b->ip2_x128, (long long)nx));
    b->ip2_ready = true;
    return OIVA_OK;
}

// the batch of frames[p] frames per problem (T = the largest); arguments checked by the callers
int create_batch(oiva_batch** out, int device, const std::vector<int>& frames, int F, int M, int K, int model, void* stream) {
    DeviceGuard guard(device);
    oiva_batch* b = new oiva_batch;
    b->device = b->mem.device = device;
    b->B = (int)frames.size(), b->T = *std::max_element(frames.begin(), frames.end()), b->F = F, b->M = M, b->K = K, b->model = model;
    const int rc = fill_batch(b, frames, stream);
    if (rc) {
        oiva_batch_destroy(b);
        return rc;
    }
    *out = b;
    return OIVA_OK;
}

}  // namespace

extern "C" {

int oiva_batch_create(oiva_batch** out, int device, int B, int T, int F, int M, int K, int model, void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(B >= 1 && T >= 1 && F >= 1, OIVA_ERR_ARG, "B, T and F must be >= 1");
    OIVA_NEED(M >= 1 && M <= kBatchMaxChannels, OIVA_ERR_ARG, "the batched path runs on 1..8 channels");
    OIVA_NEED(K >= 1 && K <= M, OIVA_ERR_ARG, "number of sources must be in 1..M");
    OIVA_NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    OIVA_NEED((double)B * T * F * M < 4e9, OIVA_ERR_ARG, "batch too large");
    return create_batch(out, device, std::vector<int>((size_t)B, T), F, M, K, model, stream);
}

oiva_status oiva_batch_create_ragged(oiva_batch** out, int device, int B, const int* frames, int F, int M, int K, int model,
                                     void* stream) {
    OIVA_NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    OIVA_NEED(frames != nullptr, OIVA_ERR_ARG, "null frames");
    OIVA_NEED(B >= 1 && F >= 1, OIVA_ERR_ARG, "B and F must be >= 1");
    OIVA_NEED(M >= 1 && M <= kBatchMaxChannels, OIVA_ERR_ARG, "the batched path runs on 1..8 channels");
    OIVA_NEED(K >= 1 && K <= M, OIVA_ERR_ARG, "number of sources must be in 1..M");
    OIVA_NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    double total = 0.;
    int tmax = 0;
    for (int p = 0; p < B; ++p) {
        OIVA_NEED(frames[p] >= 1, OIVA_ERR_ARG, "every problem needs T >= 1 frames (problem " + std::to_string(p) + ")");
        total += frames[p];
        tmax = std::max(tmax, frames[p]);
    }
    OIVA_NEED(total * F * M < 4e9 && (double)B * F * M * M * K * ceil_div(tmax, kCovFramesPerSplit) < 4e9, OIVA_ERR_ARG, "batch too large");
    const int rc = create_batch(out, device, std::vector<int>(frames, frames + B), F, M, K, model, stream);
    if (rc == OIVA_OK) (*out)->ragged = true;
    return rc;
}

int oiva_batch_destroy(oiva_batch* b) {
    if (!b) return OIVA_OK;
    DeviceGuard guard(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    (void)drop_graphs(b);
    b->mem.clear();
    b->stream.close();
    delete b;
    return OIVA_OK;
}

int oiva_batch_set_x_host(oiva_batch* b, const void* X, int f64) {
    OIVA_NEED(b && X, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    const size_t n = b->frames_total * b->F * b->M;
    if (b->c128) {
        // the caller's bits: no conversion pass
        OIVA_NEED(f64, OIVA_ERR_ARG, "a complex128 batch takes complex128 X");
        if (!b->X128_owned) OIVA_TRY_HIP(b->mem.take_one(&b->X128_owned, n * sizeof(double2)));
        OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
        OIVA_TRY_HIP(hipMemcpy(b->X128_owned, X, n * sizeof(double2), hipMemcpyHostToDevice));
        return install_x(b, b->X128_owned);
    }
    if (!b->X_owned) OIVA_TRY_HIP(b->mem.take_one(&b->X_owned, n * sizeof(float2)));
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    if (f64) {
        // converted on the device, through a bounded staging buffer: flat, "rows" of one element
        OIVA_TRY_HIP(staged_copy_c128(true, b->stream, const_cast<void*>(X), 0, b->X_owned, 1, (long long)n, kStageBytes,
                                      b->device, Mem::plain));
    } else {
        OIVA_TRY_HIP(hipMemcpy(b->X_owned, X, n * sizeof(float2), hipMemcpyHostToDevice));
    }
    return install_x(b, b->X_owned);
}

int oiva_batch_set_x_dev(oiva_batch* b, const void* X_dev) {
    OIVA_NEED(b && X_dev, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    return install_x(b, X_dev);
}

int oiva_batch_covariance(oiva_batch* b) {
    OIVA_NEED(b, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(b->have_x, OIVA_ERR_STATE, "X not set");
    DeviceGuard guard(b->device);
    // unit weights, one "source": partials [nsplit][B*F][1][M*M]; problem b's own nsplit_b partials added in split order and
    // divided by T_b (overiva.py:87)
    if (b->c128) {
        OIVA_TRY_HIP(launch_c128_cov(b->stream, b->X128, nullptr, b->probs_dev, b->Vpart, b->B, b->F, b->M, 1, b->nsplit));
        OIVA_TRY_HIP(launch_ragged_sum_parts(b->stream, b->Vpart, b->probs_dev, b->Cx, b->B, b->F, b->M));
    } else if (b->ragged) {
        OIVA_TRY_HIP(launch_ragged_cov(b->stream, b->X, nullptr, b->probs_dev, nullptr, b->model, b->Vpart, b->B, b->F, b->M, 1, b->nsplit));
        OIVA_TRY_HIP(launch_ragged_sum_parts(b->stream, b->Vpart, b->probs_dev, b->Cx, b->B, b->F, b->M));
    } else {
        const DenseArgs d = dense_args(b);
        OIVA_TRY_HIP(launch_batch_cov(b->stream, b->X, nullptr, 0, nullptr, b->model, b->Vpart, b->B, d.T, b->F, b->M, 1, d.nsplit, d.tc));
        OIVA_TRY_HIP(launch_sum_parts(b->stream, b->Vpart, true, d.nsplit, b->Cx, (long long)nbins(b) * b->M * b->M, 1. / (double)d.T));
    }
    b->have_cx = true;
    b->five_ready = false;
    return OIVA_OK;
}

int oiva_batch_set_w(oiva_batch* b, const void* W0, int f64) {
    OIVA_NEED(b, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (needed for the orthogonality constraint)");
    DeviceGuard guard(b->device);
    const int M = b->M, K = b->K;
    const std::vector<double2> wh = pack_what(W0, f64, nbins(b), M, K);
    std::vector<float2> w32(wh.size());
    for (size_t i = 0; i < wh.size(); ++i) w32[i] = make_float2((float)wh[i].x, (float)wh[i].y);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(b->What, w32.data(), w32.size() * sizeof(float2), hipMemcpyHostToDevice));
    OIVA_TRY_HIP(hipMemcpy(b->What64, wh.data(), wh.size() * sizeof(double2), hipMemcpyHostToDevice));
    b->have_w = true;
    if (K < M) OIVA_TRY_HIP(launch_update(b->stream, update_args(b, true)));   // J from the orthogonality constraint, overiva.py:120-121
    return OIVA_OK;
}

int oiva_batch_set_w_eig(oiva_batch* b) {
    OIVA_NEED(b, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    // overiva.py:106-109 per bin, the device eigensolver on B*F bins
    OIVA_TRY_HIP(launch_pca_subspace(b->stream, b->Cx, b->What, b->What64, nullptr, (int)nbins(b), b->M, b->K, true));
    b->have_w = true;
    if (b->K < b->M) OIVA_TRY_HIP(launch_update(b->stream, update_args(b, true)));
    return OIVA_OK;
}

int oiva_batch_iterate(oiva_batch* b, int n) {
    int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(n >= 0, OIVA_ERR_ARG, "n must be >= 0");
    DeviceGuard guard(b->device);
    while (n > 0) {
        const int it = std::min(n, kGraphMaxIters);
        hipGraphExec_t g = nullptr;
        rc = graph_for(b, it, &g);
        if (rc) return rc;
        OIVA_TRY_HIP(hipGraphLaunch(g, b->stream));
        n -= it;
    }
    return OIVA_OK;
}

int oiva_batch_demix(oiva_batch* b, void* Y_host, int f64, int proj_back) {
    OIVA_NEED(Y_host, OIVA_ERR_ARG, "null argument");
    int rc = check_ready(b);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    rc = demix_on_device(b, proj_back);
    if (rc) return rc;
    const size_t ny = b->frames_total * b->F * b->K;
    if (b->c128 && !f64) {
        // the rounded copy of what the device computed in float64
        std::vector<double2> y(ny);
        OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
        OIVA_TRY_HIP(hipMemcpy(y.data(), b->Y128, ny * sizeof(double2), hipMemcpyDeviceToHost));
        float2* out = static_cast<float2*>(Y_host);
        for (size_t i = 0; i < ny; ++i) out[i] = make_float2((float)y[i].x, (float)y[i].y);
        return OIVA_OK;
    }
    if (f64 && !b->c128 && b->five_ready) {
        // FIVE holds X widened to complex128: a complex128 Y is formed in float64 from it, not widened from the complex64 one
        if (!b->Y128) OIVA_TRY_HIP(b->mem.take_one(&b->Y128, ny * sizeof(double2)));
        if (proj_back && !b->Z128) OIVA_TRY_HIP(b->mem.take_one(&b->Z128, nbins(b) * b->K * sizeof(double2)));
        OIVA_TRY_HIP(launch_c128_demix(b->stream, b->five_x128, b->What64, b->Z128, b->Y128, b->probs_dev, b->B, b->T, b->F, b->M, b->K,
                                       proj_back != 0));
    } else if (f64 && !b->c128) {
        if (!b->Y128) OIVA_TRY_HIP(b->mem.take_one(&b->Y128, ny * sizeof(double2)));
        OIVA_TRY_HIP(launch_cast_c64_to_c128(b->stream, b->Y, b->Y128, (long long)ny));
    }
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(Y_host, f64 ? (const void*)b->Y128 : (const void*)b->Y, ny * (f64 ? sizeof(double2) : sizeof(float2)),
                      hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_demix_dev(oiva_batch* b, int proj_back, void** Y_dev) {
    OIVA_NEED(Y_dev != nullptr, OIVA_ERR_ARG, "null argument");
    *Y_dev = nullptr;
    int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "oiva_batch_demix_dev hands out complex64: not on a complex128 batch");
    DeviceGuard guard(b->device);
    rc = demix_on_device(b, proj_back);
    if (rc) return rc;
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    *Y_dev = b->Y;
    return OIVA_OK;
}

int oiva_batch_get_w(oiva_batch* b, void* W_host, int f64) {
    OIVA_NEED(b && W_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(b->device);
    std::vector<int> bad;
    const int rc = download_w(b, W_host, f64, bad);
    if (rc) return rc;
    std::string which;
    for (int p = 0; p < b->B; ++p)
        if (bad[p]) which += (which.empty() ? "" : ", ") + std::to_string(p);
    if (!which.empty())
        return fail_with(OIVA_ERR_NUMERIC, "demixing matrix holds non-finite values (singular W_hat^H V) in problem(s) " + which);
    return OIVA_OK;
}

int oiva_batch_status(oiva_batch* b, int* status) {
    OIVA_NEED(b && status, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(b->device);
    std::vector<int> bad;
    const int rc = download_w(b, nullptr, 0, bad);
    if (rc) return rc;
    std::copy(bad.begin(), bad.end(), status);
    return OIVA_OK;
}

int oiva_batch_time_stages(oiva_batch* b, int n, float* total_ms, float* per_stage_ms) {
    int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && total_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    if (per_stage_ms) {
        double acc[4] = {0., 0., 0., 0.};
        for (int i = 0; i < n; ++i) {
            // (back to back, one wait for the last: not four brackets with a wait each)
            const std::vector<hipEvent_t>& ev = b->stream.events;
            OIVA_TRY_HIP(hipEventRecord(ev[0], b->stream));
            for (int s = 0; s < 4; ++s) {
                rc = stage(b, s);
                if (rc) return rc;
                OIVA_TRY_HIP(hipEventRecord(ev[s + 1], b->stream));
            }
            OIVA_TRY_HIP(hipEventSynchronize(ev[4]));
            for (int s = 0; s < 4; ++s) {
                float ms = 0.f;
                OIVA_TRY_HIP(hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
                acc[s] += ms;
            }
        }
        for (int s = 0; s < 4; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    }
    hipGraphExec_t g = nullptr;
    rc = graph_for(b, std::min(n, kGraphMaxIters), &g);
    if (rc) return rc;
    OIVA_TRY_HIP(hipGraphLaunch(g, b->stream));          // (warm)
    float ms = 0.f;
    rc = b->stream.elapsed_ms(0, 1, [&] { OIVA_TRY_HIP(hipGraphLaunch(g, b->stream)); return (int)OIVA_OK; }, &ms);
    if (rc) return rc;
    *total_ms = ms / (float)std::min(n, kGraphMaxIters);
    return OIVA_OK;
}

// ---- complex128 data (kernels_batch_c128.hip) -------------------------------------------------------------------
oiva_status oiva_batch_set_data_c128(oiva_batch* b) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    if (b->c128) return OIVA_OK;
    OIVA_NEED(!b->have_x, OIVA_ERR_STATE, "the complex128 data path is chosen before X is set");
    DeviceGuard guard(b->device);
    DeviceArena& mem = b->mem;
    const size_t before = mem.mark();
    size_t p_doubles = 0;
    for (const RaggedProblem& d : b->probs) p_doubles = std::max(p_doubles, d.p_off + (size_t)b->nb * d.T * b->K);
    mem.take(&b->Ppart64, p_doubles * sizeof(double));
    mem.take(&b->Rw64, b->frames_total * b->K * sizeof(double));
    mem.take(&b->Gs64, (size_t)b->B * b->rblocks * b->K * sizeof(double));
    if (!mem.ok()) {
        mem.release_to(before);
        return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
    }
    // the float32 stages' buffers are not used on this path
    mem.release(&b->Ppart);
    mem.release(&b->R);
    mem.release(&b->wscale);
    mem.release(&b->Spart);
    b->c128 = true;
    return OIVA_OK;
}

oiva_status oiva_batch_c128_get_weights(oiva_batch* b, double* w) {
    OIVA_NEED(b && w, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(b->c128, OIVA_ERR_ARG, "not a complex128 batch");
    const int rc = check_ready(b);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(w, b->Rw64, b->frames_total * b->K * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_c128_get_cov(oiva_batch* b, void* V) {
    OIVA_NEED(b && V, OIVA_ERR_ARG, "null argument");
    const int rc = check_ready(b);        // (either data path: Vpart has one layout)
    if (rc) return rc;
    DeviceGuard guard(b->device);
    const int M = b->M, K = b->K, MM = M * M;
    const size_t per_split = nbins(b) * K * MM;
    std::vector<double> part((size_t)b->nsplit * per_split);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(part.data(), b->Vpart, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    // every problem's own splits added in order and divided by its T, unpacked from the Hermitian half
    double2* out = static_cast<double2*>(V);
    std::vector<double> acc(MM);
    for (int p = 0; p < b->B; ++p) {
        const RaggedProblem& d = b->probs[p];
        for (size_t fk = (size_t)p * b->F * K; fk < (size_t)(p + 1) * b->F * K; ++fk) {
            for (int e = 0; e < MM; ++e) {
                double s = 0.;
                for (int i = 0; i < d.nsplit; ++i) s += part[(size_t)i * per_split + fk * MM + e];
                acc[e] = s / (double)d.T;
            }
            double2* o = out + fk * MM;
            for (int c = 0; c < M; ++c) {
                o[c * M + c] = make_double2(acc[c], 0.);
                for (int dd = c + 1; dd < M; ++dd) {
                    const int a = herm_pair_index(M, c, dd);
                    o[c * M + dd] = make_double2(acc[a], acc[a + 1]);
                    o[dd * M + c] = make_double2(acc[a], -acc[a + 1]);
                }
            }
        }
    }
    return OIVA_OK;
}

// ---- batched OGIVE (reference ive.py:33-256, one problem per batch entry) -------------------------------------------------
oiva_status oiva_batch_get_cx(oiva_batch* b, void* Cx_host, int f64) {
    OIVA_NEED(b && Cx_host, OIVA_ERR_ARG, "null argument");
    OIVA_NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    const size_t n = nbins(b) * b->M * b->M;
    const size_t bytes = n * (f64 ? sizeof(double2) : sizeof(float2));
    void* full = nullptr;
    ScopedDev scratch;
    OIVA_TRY_HIP(scratch.take_one(&full, bytes));
    OIVA_TRY_HIP(launch_unpack_herm(b->stream, b->Cx, full, f64 != 0, (long long)nbins(b), b->M));
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(Cx_host, full, bytes, hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_ogive_begin(oiva_batch* b, int update_mode, int model) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->ragged, OIVA_ERR_ARG, "OGIVE is not supported on a ragged batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "OGIVE is not supported on a complex128 batch");
    int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(b->K == 1, OIVA_ERR_ARG, "OGIVE extracts one source: create the batch with K = 1");
    OIVA_NEED(update_mode >= OIVA_OGIVE_DEMIX && update_mode <= OIVA_OGIVE_SWITCHING, OIVA_ERR_ARG, "unknown update mode");
    OIVA_NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    DeviceGuard guard(b->device);
    const size_t nb = nbins(b), M = b->M, B = b->B;
    if (!b->Opart) {                     // (the last of the state: all of it or none)
        DeviceArena& mem = b->mem;
        const size_t before = mem.mark();
        alloc_ogive_state(b->og.bin, nb, M, mem);        // (its ctrl / maxdelta: reset by ogive_init_kernel; the batch keeps its own per problem)
        mem.take(&b->og.done, B * sizeof(int));
        mem.take(&b->og.epochs, B * sizeof(int));
        mem.take(&b->og.maxdelta, B * sizeof(double));
        mem.take(&b->og.runmax, B * sizeof(unsigned long long));
        mem.take(&b->og.ticket, B * sizeof(unsigned));
        mem.take(&b->Opart, (size_t)b->osplit * nb * (2 * M + 1) * sizeof(double));
        if (!mem.ok()) {
            mem.release_to(before);
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
        }
    }
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    if (b->og_graph) {                   // captured for the previous update mode / model
        OIVA_TRY_HIP(hipGraphExecDestroy(b->og_graph));
        b->og_graph = nullptr;
    }
    b->og.bin.Cx = b->Cx;
    b->og.bin.What = b->What;
    b->og.bin.What64 = b->What64;
    b->og_mode = update_mode;
    b->og_model = model;
    // Cx^-1, ||Cx||, a from w, the step selection (ive.py:100-102,136-139,173-180) on all B*F bins
    OIVA_TRY_HIP(launch_ogive_init(b->stream, b->og.bin, (int)nb, b->M, update_mode));
    OIVA_TRY_HIP(hipMemsetAsync(b->og.done, 0, B * sizeof(int), b->stream));
    OIVA_TRY_HIP(hipMemsetAsync(b->og.epochs, 0, B * sizeof(int), b->stream));
    OIVA_TRY_HIP(hipMemsetAsync(b->og.maxdelta, 0, B * sizeof(double), b->stream));
    OIVA_TRY_HIP(hipMemsetAsync(b->og.runmax, 0, B * sizeof(unsigned long long), b->stream));
    OIVA_TRY_HIP(hipMemsetAsync(b->og.ticket, 0, B * sizeof(unsigned), b->stream));
    b->og_ready = true;
    return OIVA_OK;
}

oiva_status oiva_batch_ogive_iterate(oiva_batch* b, int first_epoch, int n, double step_size, double tol, int* epochs_run, int* converged,
                                 double* max_delta) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->ragged, OIVA_ERR_ARG, "OGIVE is not supported on a ragged batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "OGIVE is not supported on a complex128 batch");
    int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(b->og_ready, OIVA_ERR_STATE, "call oiva_batch_ogive_begin first");
    OIVA_NEED(n >= 0 && first_epoch >= 0, OIVA_ERR_ARG, "negative epoch count");
    DeviceGuard guard(b->device);
    const int B = b->B;
    std::vector<int> before(B), after(B);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(before.data(), b->og.epochs, B * sizeof(int), hipMemcpyDeviceToHost));
    const int amodel = b->og_model == OIVA_MODEL_LAPLACE ? kModelOgiveLaplace : OIVA_MODEL_GAUSS;
    const DenseArgs d = dense_args(b);
    // one epoch is five launches on the batch's stream (four when the switching criterion does not run)
    auto epochs = [&](int e0, int count) -> int {
        for (int e = e0; e < e0 + count; ++e) {
            if (b->og_mode == OIVA_OGIVE_SWITCHING && e % 10 == 0)
                OIVA_TRY_HIP(launch_batch_ogive_switch(b->stream, b->og, B, b->F, b->M));                     // ive.py:192-193
            OIVA_TRY_HIP(launch_batch_ogive_power(b->stream, b->X, b->What, b->Ppart, b->og.done, B, d.T, b->F, b->M, d.pw_nsplit,
                                             d.tcp));                                                     // ive.py:196, :210/:213
            OIVA_TRY_HIP(launch_batch_ogive_activation(b->stream, b->Ppart, b->nb, b->R, d.r_stride, b->og.done, B, d.T, amodel,
                                                  b->F));                                                 // ive.py:209-217
            OIVA_TRY_HIP(launch_batch_ogive_framesum(b->stream, b->X, b->What64, b->R, d.r_stride, b->og.done, b->Opart, B, d.T, b->F,
                                                b->M, b->osplit, b->otc));                                // ive.py:218-227
            OIVA_TRY_HIP(launch_batch_ogive_step(b->stream, b->og, b->Opart, b->osplit, B, b->F, b->M, step_size, tol));   // ive.py:228-246
        }
        return OIVA_OK;
    };
    if (n >= kOgMinGraphEpochs) {
        // n epochs as one linear graph on the batch's stream, cached while (n, phase, step size, tol) stay the same
        const int phase = first_epoch % 10;
        if (!b->og_graph || b->og_graph_n != n || b->og_graph_phase != phase || b->og_graph_mu != step_size || b->og_graph_tol != tol) {
            if (b->og_graph) OIVA_TRY_HIP(hipGraphExecDestroy(b->og_graph));
            b->og_graph = nullptr;
            rc = capture_graph(b->stream, [&] { return epochs(phase, n); }, &b->og_graph, false);
            if (rc) return rc;
            b->og_graph_n = n;
            b->og_graph_phase = phase;
            b->og_graph_mu = step_size;
            b->og_graph_tol = tol;
        }
        OIVA_TRY_HIP(hipGraphLaunch(b->og_graph, b->stream));
    } else if ((rc = epochs(first_epoch, n))) {
        return rc;
    }
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(after.data(), b->og.epochs, B * sizeof(int), hipMemcpyDeviceToHost));
    if (epochs_run)
        for (int p = 0; p < B; ++p) epochs_run[p] = after[p] - before[p];
    if (converged) OIVA_TRY_HIP(hipMemcpy(converged, b->og.done, B * sizeof(int), hipMemcpyDeviceToHost));
    if (max_delta) OIVA_TRY_HIP(hipMemcpy(max_delta, b->og.maxdelta, B * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

// ---- batched ILRMA (one room per batch entry, determined, eager launches) ------------------------------------------
oiva_status oiva_batch_ilrma_begin(oiva_batch* b, int n_components, const double* T0, const double* V0) {
    int rc = check_ilrma(b, false);
    if (rc) return rc;
    OIVA_NEED(n_components >= 1 && n_components <= kIlrmaMaxComponents, OIVA_ERR_ARG, "n_components must be in 1..16");
    OIVA_NEED(T0 != nullptr && V0 != nullptr, OIVA_ERR_ARG, "null argument");
    const size_t B = b->B, K = b->K, F = b->F, T = b->T, L = n_components;
    const size_t nt = B * K * F * L, nv = B * K * L * T, npr = B * K * F * T;
    for (size_t i = 0; i < nt; ++i) OIVA_NEED(T0[i] > 0. && std::isfinite(T0[i]), OIVA_ERR_ARG, "T0 must be strictly positive");
    for (size_t i = 0; i < nv; ++i) OIVA_NEED(V0[i] > 0. && std::isfinite(V0[i]), OIVA_ERR_ARG, "V0 must be strictly positive");
    DeviceGuard guard(b->device);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    DeviceArena& mem = b->mem;
    IlrmaState& il = b->il;
    if (il.lam && il.L != n_components)                        // (another component count: the state is sized by it)
        for (double** q : {&il.Tn, &il.Vn, &il.P, &il.R, &il.Upart, &il.rowsum, &il.lam}) mem.release(q);
    b->il_ready = false;
    if (!il.lam) {                       // (the last of the state: all of it or none)
        const size_t before = mem.mark();
        il = IlrmaState{};
        il.L = n_components;
        mem.take(&il.Tn, nt * sizeof(double));
        mem.take(&il.Vn, nv * sizeof(double));
        mem.take(&il.P, npr * sizeof(double));
        mem.take(&il.R, npr * sizeof(double));
        mem.take(&il.Upart, 2 * (size_t)ilrma_v_chunks(b->F) * nv * sizeof(double));
        mem.take(&il.rowsum, B * K * F * sizeof(double));
        mem.take(&il.lam, B * K * sizeof(double));
        if (!mem.ok()) {
            mem.release_to(before);
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
        }
    }
    OIVA_TRY_HIP(hipMemcpy(b->il.Tn, T0, nt * sizeof(double), hipMemcpyHostToDevice));
    OIVA_TRY_HIP(hipMemcpy(b->il.Vn, V0, nv * sizeof(double), hipMemcpyHostToDevice));
    OIVA_TRY_HIP(hipMemsetAsync(b->il.lam, 0, B * K * sizeof(double), b->stream));
    // R = Tn Vn and P from the W that is set
    rc = ilrma_stage(b, OIVA_ILRMA_STAGE_R);
    if (rc) return rc;
    rc = ilrma_stage(b, OIVA_ILRMA_STAGE_POWER);
    if (rc) return rc;
    b->il_ready = true;
    return OIVA_OK;
}

oiva_status oiva_batch_ilrma_stage(oiva_batch* b, int stage) {
    const int rc = check_ilrma(b, true);
    if (rc) return rc;
    OIVA_NEED(stage >= 0 && stage < kIlrmaStages, OIVA_ERR_ARG, "unknown ILRMA stage");
    DeviceGuard guard(b->device);
    return ilrma_stage(b, stage);
}

oiva_status oiva_batch_ilrma_iterate(oiva_batch* b, int n) {
    int rc = check_ilrma(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 0, OIVA_ERR_ARG, "n must be >= 0");
    DeviceGuard guard(b->device);
    for (int e = 0; e < n; ++e)
        for (int s = 0; s < kIlrmaStages; ++s)
            if ((rc = ilrma_stage(b, s))) return rc;
    return OIVA_OK;
}

oiva_status oiva_batch_ilrma_get_nmf(oiva_batch* b, double* T, double* V) {
    const int rc = check_ilrma(b, true);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    const size_t BK = (size_t)b->B * b->K, L = b->il.L;
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    if (T) OIVA_TRY_HIP(hipMemcpy(T, b->il.Tn, BK * b->F * L * sizeof(double), hipMemcpyDeviceToHost));
    if (V) OIVA_TRY_HIP(hipMemcpy(V, b->il.Vn, BK * L * b->T * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_ilrma_get_pr(oiva_batch* b, double* P, double* R) {
    const int rc = check_ilrma(b, true);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)b->B * b->K * b->F * b->T;
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    if (P) OIVA_TRY_HIP(hipMemcpy(P, b->il.P, n * sizeof(double), hipMemcpyDeviceToHost));
    if (R) OIVA_TRY_HIP(hipMemcpy(R, b->il.R, n * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_ilrma_get_cov(oiva_batch* b, double* C, double* lambda) {
    const int rc = check_ilrma(b, true);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    if (C) {
        // the frame-split partials of the last covariance stage, added in split order
        const size_t n = nbins(b) * b->K * b->M * b->M;
        const int nsplit = dense_args(b).nsplit;
        std::vector<double> part((size_t)nsplit * n);
        OIVA_TRY_HIP(hipMemcpy(part.data(), b->Vpart, part.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            double s = 0.;
            for (int p = 0; p < nsplit; ++p) s += part[(size_t)p * n + i];
            C[i] = s;
        }
    }
    if (lambda) OIVA_TRY_HIP(hipMemcpy(lambda, b->il.lam, (size_t)b->B * b->K * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_ilrma_time_stages(oiva_batch* b, int n, float* per_stage_ms) {
    int rc = check_ilrma(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && per_stage_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    double acc[kIlrmaStages] = {};
    for (int e = 0; e < n; ++e) {
        for (int s = 0; s < kIlrmaStages; ++s) {
            float ms = 0.f;
            if ((rc = b->stream.elapsed_ms(0, 1, [&] { return ilrma_stage(b, s); }, &ms))) return rc;
            acc[s] += ms;
        }
    }
    for (int s = 0; s < kIlrmaStages; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    return OIVA_OK;
}

// ---- batched ISS (one room per batch entry of either kind, determined, eager launches) -----------------------------
oiva_status oiva_batch_iss_begin(oiva_batch* b) {
    int rc = check_iss(b, false);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    b->iss_ready = false;
    if (!b->iss_phi) {                   // (the last of the state: all of it or none)
        b->iss_groups = 0;
        b->iss_slab = 0;
        for (const RaggedProblem& d : b->probs) {
            b->iss_groups = std::max(b->iss_groups, iss_groups(d.T, b->F, b->M));
            b->iss_slab = std::max(b->iss_slab, (size_t)iss_group_bins(d.T, b->F, b->M) * d.T * b->M * sizeof(double2));
        }
        DeviceArena& mem = b->mem;
        const size_t before = mem.mark();
        mem.take(&b->iss_part, b->frames_total * b->iss_groups * b->M * sizeof(double));
        mem.take(&b->iss_rw, b->frames_total * b->M * sizeof(double));
        mem.take(&b->iss_phi, b->frames_total * b->M * sizeof(double));
        if (!mem.ok()) {
            mem.release_to(before);
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
        }
    }
    OIVA_TRY_HIP(iss_sweep_prepare(b->M));
    // the powers of the W that is set: demix and partial powers, no step
    rc = iss_stage(b, OIVA_ISS_STAGE_SWEEP, 0);
    if (rc) return rc;
    b->iss_ready = true;
    return OIVA_OK;
}

oiva_status oiva_batch_iss_stage(oiva_batch* b, int stage) {
    const int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(stage >= 0 && stage < kIssStages, OIVA_ERR_ARG, "unknown ISS stage");
    DeviceGuard guard(b->device);
    return iss_stage(b, stage, b->M);
}

oiva_status oiva_batch_iss_iterate(oiva_batch* b, int n) {
    int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 0, OIVA_ERR_ARG, "n must be >= 0");
    DeviceGuard guard(b->device);
    for (int e = 0; e < n; ++e)
        for (int s = 0; s < kIssStages; ++s)
            if ((rc = iss_stage(b, s, b->M))) return rc;
    return OIVA_OK;
}

oiva_status oiva_batch_iss_sweep_steps(oiva_batch* b, int n_steps) {
    const int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(n_steps >= 0 && n_steps <= b->M, OIVA_ERR_ARG, "n_steps must be in 0..M");
    DeviceGuard guard(b->device);
    return iss_stage(b, OIVA_ISS_STAGE_SWEEP, n_steps);
}

oiva_status oiva_batch_iss_get_weights(oiva_batch* b, double* phi) {
    const int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(phi != nullptr, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(phi, b->iss_phi, b->frames_total * b->M * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_iss_get_powers(oiva_batch* b, double* p) {
    const int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(p != nullptr, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    const size_t M = b->M;
    std::vector<double> part(b->frames_total * b->iss_groups * M);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(part.data(), b->iss_part, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    // every room's own groups, added as the activation adds them: 16 strided sequences, then those in order
    for (const RaggedProblem& d : b->probs) {
        const int ng = iss_groups(d.T, b->F, b->M);
        const double* base = part.data() + d.x_off * b->iss_groups * M;
        for (size_t i = 0; i < (size_t)d.T * M; ++i) {
            double s = 0.;
            for (int j = 0; j < kIssGroupLanes; ++j) {
                double a = 0.;
                for (int g = j; g < ng; g += kIssGroupLanes) a += base[(size_t)g * d.T * M + i];
                s += a;
            }
            p[d.x_off * M + i] = s;
        }
    }
    return OIVA_OK;
}

oiva_status oiva_batch_iss_time_stages(oiva_batch* b, int n, float* per_stage_ms) {
    int rc = check_iss(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && per_stage_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    double acc[kIssStages] = {};
    for (int e = 0; e < n; ++e) {
        for (int s = 0; s < kIssStages; ++s) {
            float ms = 0.f;
            if ((rc = b->stream.elapsed_ms(0, 1, [&] { return iss_stage(b, s, b->M); }, &ms))) return rc;
            acc[s] += ms;
        }
    }
    for (int s = 0; s < kIssStages; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    return OIVA_OK;
}

// ---- batched FIVE (one room per batch entry of either kind, one source, eager launches) ----------------------------
oiva_status oiva_batch_five_begin(oiva_batch* b) {
    const int rc = check_five(b, false);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    b->five_ready = false;
    const size_t nx = b->frames_total * b->F * b->M;
    if (!b->five_x128) {                 // (the last of the state: all of it or none)
        DeviceArena& mem = b->mem;
        const size_t before = mem.mark();
        size_t p_doubles = 0;
        for (const RaggedProblem& d : b->probs) p_doubles = std::max(p_doubles, d.p_off + (size_t)b->nb * d.T);
        mem.take(&b->five_li, nbins(b) * b->M * b->M * sizeof(double2));
        mem.take(&b->Ppart64, p_doubles * sizeof(double));
        mem.take(&b->Rw64, b->frames_total * sizeof(double));
        mem.take(&b->Gs64, (size_t)b->B * b->rblocks * sizeof(double));
        mem.take(&b->five_x128, nx * sizeof(double2));
        if (!mem.ok()) {
            mem.release_to(before);
            b->five_li = nullptr, b->Ppart64 = b->Rw64 = b->Gs64 = nullptr, b->five_x128 = nullptr;
            return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(mem.status()));
        }
    }
    OIVA_TRY_HIP(launch_cast_c64_to_c128(b->stream, b->X, b->five_x128, (long long)nx));
    OIVA_TRY_HIP(launch_five_begin(b->stream, b->Cx, b->five_li, (int)nbins(b), b->M));
    b->five_ready = true;
    return OIVA_OK;
}

oiva_status oiva_batch_five_stage(oiva_batch* b, int stage) {
    const int rc = check_five(b, true);
    if (rc) return rc;
    OIVA_NEED(stage >= 0 && stage < kFiveStages, OIVA_ERR_ARG, "unknown FIVE stage");
    DeviceGuard guard(b->device);
    return five_stage(b, stage);
}

oiva_status oiva_batch_five_iterate(oiva_batch* b, int n) {
    int rc = check_five(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 0, OIVA_ERR_ARG, "n must be >= 0");
    DeviceGuard guard(b->device);
    for (int e = 0; e < n; ++e)
        for (int s = 0; s < kFiveStages; ++s)
            if ((rc = five_stage(b, s))) return rc;
    return OIVA_OK;
}

oiva_status oiva_batch_five_time_stages(oiva_batch* b, int n, float* per_stage_ms) {
    int rc = check_five(b, true);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && per_stage_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    double acc[kFiveStages] = {};
    for (int e = 0; e < n; ++e) {
        for (int s = 0; s < kFiveStages; ++s) {
            float ms = 0.f;
            if ((rc = b->stream.elapsed_ms(0, 1, [&] { return five_stage(b, s); }, &ms))) return rc;
            acc[s] += ms;
        }
    }
    for (int s = 0; s < kFiveStages; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    return OIVA_OK;
}

oiva_status oiva_batch_five_get_reduction(oiva_batch* b, void* Li) {
    const int rc = check_five(b, true);
    if (rc) return rc;
    OIVA_NEED(Li != nullptr, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    OIVA_TRY_HIP(hipMemcpy(Li, b->five_li, nbins(b) * b->M * b->M * sizeof(double2), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

// ---- batched IP2 (one room per batch entry of either kind, any K <= M, eager launches) ---------------------------------
oiva_status oiva_batch_ip2_stage(oiva_batch* b, int stage, int iteration) {
    const int rc = prepare_ip2(b);
    if (rc) return rc;
    OIVA_NEED(stage >= 0 && stage < kIp2Stages, OIVA_ERR_ARG, "unknown IP2 stage");
    OIVA_NEED(iteration >= 0, OIVA_ERR_ARG, "iteration must be >= 0");
    DeviceGuard guard(b->device);
    return ip2_stage(b, stage, iteration);
}

oiva_status oiva_batch_ip2_iterate(oiva_batch* b, int first_iteration, int n) {
    int rc = prepare_ip2(b);
    if (rc) return rc;
    OIVA_NEED(first_iteration >= 0 && n >= 0, OIVA_ERR_ARG, "first_iteration and n must be >= 0");
    DeviceGuard guard(b->device);
    for (int e = 0; e < n; ++e)
        for (int s = 0; s < kIp2Stages; ++s)
            if ((rc = ip2_stage(b, s, first_iteration + e))) return rc;
    return OIVA_OK;
}

oiva_status oiva_batch_ip2_time_stages(oiva_batch* b, int n, float* per_stage_ms) {
    int rc = prepare_ip2(b);
    if (rc) return rc;
    OIVA_NEED(n >= 1 && per_stage_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    double acc[kIp2Stages] = {};
    for (int e = 0; e < n; ++e) {
        for (int s = 0; s < kIp2Stages; ++s) {
            float ms = 0.f;
            if ((rc = b->stream.elapsed_ms(0, 1, [&] { return ip2_stage(b, s, e); }, &ms))) return rc;
            acc[s] += ms;
        }
    }
    for (int s = 0; s < kIp2Stages; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    return OIVA_OK;
}

// ---- batched PCA front end (reference auxiva_pca.py:63-92, one problem per batch entry) -------------------------------------
oiva_status oiva_batch_set_w_pca(oiva_batch* b, double* evals_host) {
    OIVA_NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "the PCA front end is not supported on a complex128 batch");
    OIVA_NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    // auxiva_pca.py:75-81 per bin, the device eigensolver on B*F bins; the eigenvalues pass through Vpart (free between the
    // covariance and the first iteration, at least B*F*M*M doubles)
    double* evals = evals_host ? b->Vpart : nullptr;
    OIVA_TRY_HIP(launch_pca_subspace(b->stream, b->Cx, b->What, b->What64, evals, (int)nbins(b), b->M, b->K, false));
    b->have_w = true;
    if (evals_host) {
        OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
        OIVA_TRY_HIP(hipMemcpy(evals_host, evals, nbins(b) * b->M * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (b->K < b->M) OIVA_TRY_HIP(launch_update(b->stream, update_args(b, true)));   // J from the orthogonality constraint
    return OIVA_OK;
}

oiva_status oiva_batch_project_dev(oiva_batch* b, void** Xr_dev) {
    OIVA_NEED(Xr_dev != nullptr, OIVA_ERR_ARG, "null argument");
    *Xr_dev = nullptr;
    const int rc = check_ready(b);
    if (rc) return rc;
    OIVA_NEED(!b->c128, OIVA_ERR_ARG, "the PCA front end is not supported on a complex128 batch");
    DeviceGuard guard(b->device);
    if (!b->Xr) OIVA_TRY_HIP(b->mem.take_one(&b->Xr, b->frames_total * b->F * b->K * sizeof(float2)));
    // auxiva_pca.py:79-81 for every problem in one launch, from the problem table
    OIVA_TRY_HIP(launch_pca_project(b->stream, b->X, b->What, b->Xr, b->probs_dev, b->B, b->F, b->M, b->K, b->kp, b->pw_nsplit));
    OIVA_TRY_HIP(hipStreamSynchronize(b->stream));
    *Xr_dev = b->Xr;
    return OIVA_OK;
}

oiva_status oiva_batch_compose_w(oiva_batch* outer, const oiva_batch* inner) {
    OIVA_NEED(outer != nullptr && inner != nullptr, OIVA_ERR_ARG, "null batch");
    OIVA_NEED(outer != inner, OIVA_ERR_ARG, "the reduced batch must be another batch");
    OIVA_NEED(!outer->c128 && !inner->c128, OIVA_ERR_ARG, "the PCA front end is not supported on a complex128 batch");
    OIVA_NEED(inner->B == outer->B && inner->F == outer->F, OIVA_ERR_ARG, "the two batches differ in B or F");
    OIVA_NEED(inner->M == inner->K && inner->K == outer->K, OIVA_ERR_ARG,
              "the reduced batch must be determined on the K channels of the projection");
    OIVA_NEED(inner->device == outer->device, OIVA_ERR_ARG, "the two batches live on different devices");
    OIVA_NEED(outer->have_w && inner->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(outer->device);
    OIVA_TRY_HIP(hipStreamSynchronize(inner->stream));
    OIVA_TRY_HIP(launch_pca_compose(outer->stream, outer->What, outer->What64, inner->What64, (long long)nbins(outer), outer->M, outer->K));
    return OIVA_OK;
}

}  // extern "C"
