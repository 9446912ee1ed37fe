// C ABI of the batched iteration (oiva_batch_*, include/overiva_hip.h): B problems of one F, M <= 8 and K and of T_b frames each,
// packed along the frames, in the `precise` arithmetic.  Host code only.  Every batch is described by one table of per-problem
// records (RaggedProblem): oiva_batch_create makes the table of B equal lengths, oiva_batch_create_ragged that of the lengths it
// is given, and allocation, X, demix and the grid maxima follow from the table alone.  The two entries differ in the kernels
// of the iteration: a batch of oiva_batch_create runs those of kernels_batch.hip, which take T and the splits of record 0 as
// launch arguments (measured 1-4 % faster per stage than reading the table, CHANGELOG), a batch of oiva_batch_create_ragged
// those of kernels_ragged.hip, which read the table on the device.  The per-bin stages are the single-problem kernels run on
// B*F bins.  Batched OGIVE (oiva_batch_ogive_*) runs on a batch of oiva_batch_create with K = 1, with its own kernels
// (kernels_ogive_batch.hip) and a stopping rule per problem.  The PCA front end of auxiva_pca_batch (oiva_batch_set_w_pca,
// _project_dev, _compose_w; kernels_pca_batch.hip) reads the table on the device for every batch.
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "oiva_internal.h"

using namespace oiva;

namespace {

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define NEED(cond, code, msg)                       \
    do {                                            \
        if (!(cond)) return fail_with(code, msg);   \
    } while (0)

int ceil_div(int a, int b) { return (a + b - 1) / b; }
int round_up(int a, int b) { return ceil_div(a, b) * b; }

constexpr int kBatchMaxChannels = 8;
constexpr int kCovFramesPerSplit = 256;   // frame splits of the covariance pass: ceil(T / 256), a function of T alone
constexpr int kPowFramesPerSplit = 64;    // frame splits of the power pass (each partial power is one workgroup's: any split gives the same bits)
constexpr int kGraphMaxIters = 32;        // longest captured graph: an iterate(n) call is ceil(n / 32) replays
constexpr int kGraphCache = 4;
constexpr size_t kStageBytes = (size_t)256 << 20;   // staging of complex128 input
constexpr int kOgFramesPerSplit = 64;     // frame splits of the OGIVE frame sums: ceil(T / 64), a function of T alone
constexpr int kOgMinGraphEpochs = 8;      // shorter OGIVE chunks run eagerly

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

// the single-problem plan's statistics geometry (plan.hip, choose_stats_geom) for F bins: Y as overiva() writes it
CovGeom stats_geom(int T, int F, int K, int n_cu) {
    CovGeom g{};
    g.nbg = ceil_div(F, kBinsPerWave);
    g.kc = 2;
    const int blocks = g.nbg * ceil_div(K, g.kc);
    int ns = std::max(1, n_cu * 4 / std::max(1, blocks));
    ns = std::min(ns, std::max(1, T / 128));
    ns = std::min(16, ns);
    g.tc = round_up(ceil_div(T, ns), 16);
    g.nsplit = ceil_div(T, g.tc);
    return g;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct oiva_batch {
    int device = 0;
    int B = 0, T = 0, F = 0, M = 0, K = 0, model = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
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
    std::vector<std::pair<int, hipGraphExec_t>> graphs;
    hipEvent_t ev[5] = {};
    // batched OGIVE (ive.py:33-256): per-bin state of B*F bins and the per-problem stopping rule, allocated by ogive_begin
    OgiveBatchState og{};
    std::vector<void*> og_bufs;
    double* Opart = nullptr;       // [osplit][B*F][2M+1] frame-sum partials
    int osplit = 1, otc = 1;
    bool og_ready = false;
    int og_mode = 0, og_model = 0;
    // captured chunk of epochs, cached on (n, phase in the 10-epoch switching cycle, step size, tol) as the single plan's
    hipGraphExec_t og_graph = nullptr;
    int og_graph_n = 0, og_graph_phase = -1;
    double og_graph_mu = 0., og_graph_tol = 0.;
};

namespace {

size_t nbins(const oiva_batch* b) { return (size_t)b->B * b->F; }

int drop_graphs(oiva_batch* b) {
    while (!b->graphs.empty()) {
        HIP_TRY(hipGraphExecDestroy(b->graphs.back().second));
        b->graphs.pop_back();
    }
    if (b->og_graph) {
        hipGraphExec_t g = b->og_graph;
        b->og_graph = nullptr;
        HIP_TRY(hipGraphExecDestroy(g));
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
    a.wscale = init_only ? nullptr : b->wscale;
    a.nsplit = b->nsplit;
    a.T = b->T;
    a.F = (int)nbins(b);
    a.M = b->M;
    a.K = b->K;
    a.init_only = init_only ? 1 : 0;
    a.use_double = 1;
    a.layout = 0;
    a.wscale_bins = b->F;
    a.ragged = b->ragged ? b->probs_dev : nullptr;
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

// the four launches of one iteration (overiva.py:138-190)
int stage(oiva_batch* b, int s) {
    if (s == 3) {
        HIP_TRY(launch_update(b->stream, update_args(b, false)));
    } else if (b->ragged) {
        if (s == 0)
            HIP_TRY(launch_ragged_power(b->stream, b->X, b->What, b->Ppart, b->probs_dev, b->B, b->F, b->M, b->K, b->kp, b->pw_nsplit,
                                        b->tcp));
        else if (s == 1)
            HIP_TRY(launch_ragged_activation(b->stream, b->Ppart, b->nb, b->R, b->probs_dev, b->B, b->K, b->model, b->F, b->rblocks));
        else
            HIP_TRY(launch_ragged_cov(b->stream, b->X, b->R, b->probs_dev, b->wscale, b->model, b->Vpart, b->B, b->F, b->M, b->K,
                                      b->nsplit));
    } else {
        const DenseArgs d = dense_args(b);
        if (s == 0)
            HIP_TRY(launch_batch_power(b->stream, b->X, b->What, b->Ppart, b->B, d.T, b->F, b->M, b->K, b->kp, d.pw_nsplit, d.tcp));
        else if (s == 1)
            HIP_TRY(launch_batch_activation(b->stream, b->Ppart, b->nb, b->R, d.r_stride, b->B, d.T, b->K, b->model, b->F));
        else
            HIP_TRY(launch_batch_cov(b->stream, b->X, b->R, d.r_stride, b->wscale, b->model, b->Vpart, b->B, d.T, b->F, b->M, b->K,
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

// the executable graph of `iters` iterations on the batch's stream: one linear chain of 4 * iters kernel nodes
int graph_for(oiva_batch* b, int iters, hipGraphExec_t* out) {
    for (auto& g : b->graphs)
        if (g.first == iters) {
            *out = g.second;
            return OIVA_OK;
        }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
    int r = OIVA_OK;
    for (int i = 0; i < iters && r == OIVA_OK; ++i) r = one_iteration(b);
    hipError_t e = hipStreamEndCapture(b->stream, &graph);
    if (r) {
        if (graph) (void)hipGraphDestroy(graph);
        return r;
    }
    HIP_TRY(e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    HIP_TRY(e);
    HIP_TRY(hipGraphUpload(exec, b->stream));
    if ((int)b->graphs.size() >= kGraphCache) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipGraphExecDestroy(b->graphs.front().second));
        b->graphs.erase(b->graphs.begin());
    }
    b->graphs.emplace_back(iters, exec);
    *out = exec;
    return OIVA_OK;
}

int check_ready(oiva_batch* b) {
    NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    NEED(b->have_x, OIVA_ERR_STATE, "X not set (oiva_batch_set_x_host/_dev)");
    NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set (oiva_batch_set_w)");
    return OIVA_OK;
}

// W_hat of every bin in complex128, and the problems whose W (the first K columns) holds a non-finite value
int download_w(oiva_batch* b, std::vector<double2>& wh, std::vector<int>& bad) {
    const size_t MM = (size_t)b->M * b->M;
    wh.resize(nbins(b) * MM);
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(wh.data(), b->What64, wh.size() * sizeof(double2), hipMemcpyDeviceToHost));
    bad.assign(b->B, 0);
    for (int p = 0; p < b->B; ++p)
        for (size_t f = 0; f < (size_t)b->F && !bad[p]; ++f)
            for (int r = 0; r < b->M; ++r)
                for (int k = 0; k < b->K; ++k) {
                    const double2 v = wh[(((size_t)p * b->F + f) * b->M + r) * b->M + k];
                    if (!std::isfinite(v.x) || !std::isfinite(v.y)) bad[p] = 1;
                }
    return OIVA_OK;
}

// Y of every problem into the batch's own device array (allocated on first use), on the batch's stream
int demix_on_device(oiva_batch* b, int proj_back) {
    const int F = b->F, M = b->M, K = b->K;
    const size_t ny = b->frames_total * F * K;
    if (!b->Y) HIP_TRY(hipMalloc((void**)&b->Y, ny * sizeof(float2)));
    // overiva.py:192-199 per problem, with the single-problem kernels (projection back against that problem's X[b][:, :, 0]):
    // every problem at its packed frame offset with the statistics geometry of its own T_b
    for (int p = 0; p < b->B; ++p) {
        const int T = b->probs[p].T;
        const size_t t0 = b->probs[p].x_off;
        const CovGeom& stg = b->stgs[p];
        const float2* Xb = b->X + t0 * F * M;
        const float2* Wb = b->What + (size_t)p * F * M * M;
        if (proj_back) HIP_TRY(launch_demix_stats(b->stream, Xb, Wb, b->Spart, T, F, M, K, stg));
        HIP_TRY(launch_demix_write(b->stream, Xb, Wb, proj_back ? b->Spart : nullptr, stg.nsplit, b->Y + t0 * F * K, T, F, M, K));
    }
    return OIVA_OK;
}

void free_all(oiva_batch* b) {
    (void)drop_graphs(b);
    for (void* q : {(void*)b->X_owned, (void*)b->What, (void*)b->What64, (void*)b->Cx, (void*)b->Vpart, (void*)b->Ppart, (void*)b->R,
                    (void*)b->wscale, (void*)b->Spart, (void*)b->Y, (void*)b->Y128, (void*)b->Xr, (void*)b->probs_dev})
        if (q) (void)hipFree(q);
    for (void* q : b->og_bufs) (void)hipFree(q);
    for (hipEvent_t& e : b->ev)
        if (e) (void)hipEventDestroy(e);
    if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
}

// the batch of frames[p] frames per problem (T = the largest); arguments checked by the callers
int create_batch(oiva_batch** out, int device, const std::vector<int>& frames, int F, int M, int K, int model, void* stream) {
    const int B = (int)frames.size(), T = *std::max_element(frames.begin(), frames.end());
    DeviceGuard guard(device);
    oiva_batch* b = new oiva_batch;
    b->device = device;
    b->B = B, b->T = T, b->F = F, b->M = M, b->K = K, b->model = model;
    auto bail = [&](int rc) {
        free_all(b);
        delete b;
        return rc;
    };
#define TRY_CREATE(expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return bail(fail_with(OIVA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); \
    } while (0)
    if (stream) {
        b->stream = static_cast<hipStream_t>(stream);
    } else {
        TRY_CREATE(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->own_stream = true;
    }
    for (hipEvent_t& e : b->ev) TRY_CREATE(hipEventCreate(&e));
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
    TRY_CREATE(hipMalloc((void**)&b->probs_dev, (size_t)B * sizeof(RaggedProblem)));
    TRY_CREATE(hipMemcpy(b->probs_dev, b->probs.data(), (size_t)B * sizeof(RaggedProblem), hipMemcpyHostToDevice));
    const size_t MM = (size_t)M * M;
    TRY_CREATE(hipMalloc((void**)&b->What, nbins(b) * MM * sizeof(float2)));
    TRY_CREATE(hipMalloc((void**)&b->What64, nbins(b) * MM * sizeof(double2)));
    TRY_CREATE(hipMalloc((void**)&b->Cx, nbins(b) * MM * sizeof(double)));
    TRY_CREATE(hipMalloc((void**)&b->Vpart, ((size_t)b->nsplit * nbins(b) * K * MM + 2) * sizeof(double)));   // sum_vpart reads idx + 1
    TRY_CREATE(hipMalloc((void**)&b->Ppart, ppart_floats * sizeof(float)));
    TRY_CREATE(hipMalloc((void**)&b->R, r_floats * sizeof(float)));
    TRY_CREATE(hipMemset(b->R, 0, r_floats * sizeof(float)));      // (the pad rows behind every problem's r)
    TRY_CREATE(hipMalloc((void**)&b->wscale, (size_t)B * K * sizeof(float)));
    TRY_CREATE(hipMalloc((void**)&b->Spart, (size_t)spart_splits * F * K * 3 * sizeof(float)));
#undef TRY_CREATE
    *out = b;
    return OIVA_OK;
}

}  // namespace

extern "C" {

int oiva_batch_create(oiva_batch** out, int device, int B, int T, int F, int M, int K, int model, void* stream) {
    NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    NEED(B >= 1 && T >= 1 && F >= 1, OIVA_ERR_ARG, "B, T and F must be >= 1");
    NEED(M >= 1 && M <= kBatchMaxChannels, OIVA_ERR_ARG, "the batched path runs on 1..8 channels");
    NEED(K >= 1 && K <= M, OIVA_ERR_ARG, "number of sources must be in 1..M");
    NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    NEED((double)B * T * F * M < 4e9, OIVA_ERR_ARG, "batch too large");
    return create_batch(out, device, std::vector<int>((size_t)B, T), F, M, K, model, stream);
}

oiva_status oiva_batch_create_ragged(oiva_batch** out, int device, int B, const int* frames, int F, int M, int K, int model,
                                     void* stream) {
    NEED(out != nullptr, OIVA_ERR_ARG, "null out pointer");
    *out = nullptr;
    NEED(frames != nullptr, OIVA_ERR_ARG, "null frames");
    NEED(B >= 1 && F >= 1, OIVA_ERR_ARG, "B and F must be >= 1");
    NEED(M >= 1 && M <= kBatchMaxChannels, OIVA_ERR_ARG, "the batched path runs on 1..8 channels");
    NEED(K >= 1 && K <= M, OIVA_ERR_ARG, "number of sources must be in 1..M");
    NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    double total = 0.;
    int tmax = 0;
    for (int p = 0; p < B; ++p) {
        NEED(frames[p] >= 1, OIVA_ERR_ARG, "every problem needs T >= 1 frames (problem " + std::to_string(p) + ")");
        total += frames[p];
        tmax = std::max(tmax, frames[p]);
    }
    NEED(total * F * M < 4e9 && (double)B * F * M * M * K * ceil_div(tmax, kCovFramesPerSplit) < 4e9, OIVA_ERR_ARG, "batch too large");
    const int rc = create_batch(out, device, std::vector<int>(frames, frames + B), F, M, K, model, stream);
    if (rc == OIVA_OK) (*out)->ragged = true;
    return rc;
}

int oiva_batch_destroy(oiva_batch* b) {
    if (!b) return OIVA_OK;
    DeviceGuard guard(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    free_all(b);
    delete b;
    return OIVA_OK;
}

int oiva_batch_set_x_host(oiva_batch* b, const void* X, int f64) {
    NEED(b && X, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    const size_t n = b->frames_total * b->F * b->M;
    if (!b->X_owned) HIP_TRY(hipMalloc((void**)&b->X_owned, n * sizeof(float2)));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (f64) {
        // converted on the device, through a bounded staging buffer
        const size_t chunk = std::min(n, kStageBytes / sizeof(double2));
        double2* stage_buf = nullptr;
        HIP_TRY(hipMalloc((void**)&stage_buf, chunk * sizeof(double2)));
        hipError_t e = hipSuccess;
        for (size_t i0 = 0; i0 < n && e == hipSuccess; i0 += chunk) {
            const size_t m = std::min(chunk, n - i0);
            e = hipMemcpy(stage_buf, static_cast<const double2*>(X) + i0, m * sizeof(double2), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = launch_cast_c128_to_c64(b->stream, stage_buf, b->X_owned + i0, (long long)m);
            if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
        }
        (void)hipFree(stage_buf);
        HIP_TRY(e);
    } else {
        HIP_TRY(hipMemcpy(b->X_owned, X, n * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (b->X != b->X_owned) {          // captured graphs hold the pointer of X
        const int rc = drop_graphs(b);
        if (rc) return rc;
    }
    b->X = b->X_owned;
    b->have_x = true;
    b->have_cx = false;
    return OIVA_OK;
}

int oiva_batch_set_x_dev(oiva_batch* b, const void* X_dev) {
    NEED(b && X_dev, OIVA_ERR_ARG, "null argument");
    DeviceGuard guard(b->device);
    if (b->X != X_dev) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        const int rc = drop_graphs(b);
        if (rc) return rc;
    }
    b->X = static_cast<const float2*>(X_dev);
    b->have_x = true;
    b->have_cx = false;
    return OIVA_OK;
}

int oiva_batch_covariance(oiva_batch* b) {
    NEED(b, OIVA_ERR_ARG, "null batch");
    NEED(b->have_x, OIVA_ERR_STATE, "X not set");
    DeviceGuard guard(b->device);
    // unit weights, one "source": partials [nsplit][B*F][1][M*M]; problem b's own nsplit_b partials added in split order and
    // divided by T_b (overiva.py:87)
    if (b->ragged) {
        HIP_TRY(launch_ragged_cov(b->stream, b->X, nullptr, b->probs_dev, nullptr, b->model, b->Vpart, b->B, b->F, b->M, 1, b->nsplit));
        HIP_TRY(launch_ragged_sum_parts(b->stream, b->Vpart, b->probs_dev, b->Cx, b->B, b->F, b->M));
    } else {
        const DenseArgs d = dense_args(b);
        HIP_TRY(launch_batch_cov(b->stream, b->X, nullptr, 0, nullptr, b->model, b->Vpart, b->B, d.T, b->F, b->M, 1, d.nsplit, d.tc));
        HIP_TRY(launch_sum_parts(b->stream, b->Vpart, true, d.nsplit, b->Cx, (long long)nbins(b) * b->M * b->M, 1. / (double)d.T));
    }
    b->have_cx = true;
    return OIVA_OK;
}

int oiva_batch_set_w(oiva_batch* b, const void* W0, int f64) {
    NEED(b, OIVA_ERR_ARG, "null batch");
    NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (needed for the orthogonality constraint)");
    DeviceGuard guard(b->device);
    const int M = b->M, K = b->K;
    const size_t nb = nbins(b);
    std::vector<double2> wh(nb * M * M, make_double2(0., 0.));
    for (size_t f = 0; f < nb; ++f) {
        double2* m = wh.data() + f * M * M;
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < K; ++k) {
                const size_t i = (f * M + r) * K + k;
                if (!W0)
                    m[r * M + k] = make_double2(r == k ? 1. : 0., 0.);               // overiva.py:113-114
                else if (f64)
                    m[r * M + k] = static_cast<const double2*>(W0)[i];                // overiva.py:116-117
                else
                    m[r * M + k] = make_double2(static_cast<const float2*>(W0)[i].x, static_cast<const float2*>(W0)[i].y);
            }
        for (int r = K; r < M; ++r) m[r * M + r] = make_double2(-1., 0.);           // overiva.py:122-123
    }
    std::vector<float2> w32(wh.size());
    for (size_t i = 0; i < wh.size(); ++i) w32[i] = make_float2((float)wh[i].x, (float)wh[i].y);
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->What, w32.data(), w32.size() * sizeof(float2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->What64, wh.data(), wh.size() * sizeof(double2), hipMemcpyHostToDevice));
    b->have_w = true;
    if (K < M) HIP_TRY(launch_update(b->stream, update_args(b, true)));   // J from the orthogonality constraint, overiva.py:120-121
    return OIVA_OK;
}

int oiva_batch_set_w_eig(oiva_batch* b) {
    NEED(b, OIVA_ERR_ARG, "null batch");
    NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    // overiva.py:106-109 per bin, the device eigensolver on B*F bins
    HIP_TRY(launch_pca_subspace(b->stream, b->Cx, b->What, b->What64, nullptr, (int)nbins(b), b->M, b->K, true));
    b->have_w = true;
    if (b->K < b->M) HIP_TRY(launch_update(b->stream, update_args(b, true)));
    return OIVA_OK;
}

int oiva_batch_iterate(oiva_batch* b, int n) {
    int rc = check_ready(b);
    if (rc) return rc;
    NEED(n >= 0, OIVA_ERR_ARG, "n must be >= 0");
    DeviceGuard guard(b->device);
    while (n > 0) {
        const int it = std::min(n, kGraphMaxIters);
        hipGraphExec_t g = nullptr;
        rc = graph_for(b, it, &g);
        if (rc) return rc;
        HIP_TRY(hipGraphLaunch(g, b->stream));
        n -= it;
    }
    return OIVA_OK;
}

int oiva_batch_demix(oiva_batch* b, void* Y_host, int f64, int proj_back) {
    NEED(Y_host, OIVA_ERR_ARG, "null argument");
    int rc = check_ready(b);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    rc = demix_on_device(b, proj_back);
    if (rc) return rc;
    const size_t ny = b->frames_total * b->F * b->K;
    if (f64) {
        if (!b->Y128) HIP_TRY(hipMalloc((void**)&b->Y128, ny * sizeof(double2)));
        HIP_TRY(launch_cast_c64_to_c128(b->stream, b->Y, b->Y128, (long long)ny));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(Y_host, f64 ? (const void*)b->Y128 : (const void*)b->Y, ny * (f64 ? sizeof(double2) : sizeof(float2)),
                      hipMemcpyDeviceToHost));
    return OIVA_OK;
}

oiva_status oiva_batch_demix_dev(oiva_batch* b, int proj_back, void** Y_dev) {
    NEED(Y_dev != nullptr, OIVA_ERR_ARG, "null argument");
    *Y_dev = nullptr;
    int rc = check_ready(b);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    rc = demix_on_device(b, proj_back);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    *Y_dev = b->Y;
    return OIVA_OK;
}

int oiva_batch_get_w(oiva_batch* b, void* W_host, int f64) {
    NEED(b && W_host, OIVA_ERR_ARG, "null argument");
    NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(b->device);
    std::vector<double2> wh;
    std::vector<int> bad;
    const int rc = download_w(b, wh, bad);
    if (rc) return rc;
    const int M = b->M, K = b->K;
    const size_t nb = nbins(b);
    for (size_t f = 0; f < nb; ++f)
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < K; ++k) {
                const double2 v = wh[(f * M + r) * M + k];
                const size_t i = (f * M + r) * K + k;
                if (f64)
                    static_cast<double2*>(W_host)[i] = v;
                else
                    static_cast<float2*>(W_host)[i] = make_float2((float)v.x, (float)v.y);
            }
    std::string which;
    for (int p = 0; p < b->B; ++p)
        if (bad[p]) which += (which.empty() ? "" : ", ") + std::to_string(p);
    if (!which.empty())
        return fail_with(OIVA_ERR_NUMERIC, "demixing matrix holds non-finite values (singular W_hat^H V) in problem(s) " + which);
    return OIVA_OK;
}

int oiva_batch_status(oiva_batch* b, int* status) {
    NEED(b && status, OIVA_ERR_ARG, "null argument");
    NEED(b->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(b->device);
    std::vector<double2> wh;
    std::vector<int> bad;
    const int rc = download_w(b, wh, bad);
    if (rc) return rc;
    std::copy(bad.begin(), bad.end(), status);
    return OIVA_OK;
}

int oiva_batch_time_stages(oiva_batch* b, int n, float* total_ms, float* per_stage_ms) {
    int rc = check_ready(b);
    if (rc) return rc;
    NEED(n >= 1 && total_ms, OIVA_ERR_ARG, "n must be >= 1");
    DeviceGuard guard(b->device);
    if (per_stage_ms) {
        double acc[4] = {0., 0., 0., 0.};
        for (int i = 0; i < n; ++i) {
            HIP_TRY(hipEventRecord(b->ev[0], b->stream));
            for (int s = 0; s < 4; ++s) {
                rc = stage(b, s);
                if (rc) return rc;
                HIP_TRY(hipEventRecord(b->ev[s + 1], b->stream));
            }
            HIP_TRY(hipEventSynchronize(b->ev[4]));
            for (int s = 0; s < 4; ++s) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, b->ev[s], b->ev[s + 1]));
                acc[s] += ms;
            }
        }
        for (int s = 0; s < 4; ++s) per_stage_ms[s] = (float)(acc[s] / n);
    }
    hipGraphExec_t g = nullptr;
    rc = graph_for(b, std::min(n, kGraphMaxIters), &g);
    if (rc) return rc;
    HIP_TRY(hipGraphLaunch(g, b->stream));          // (warm)
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    HIP_TRY(hipGraphLaunch(g, b->stream));
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));
    HIP_TRY(hipEventSynchronize(b->ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
    *total_ms = ms / (float)std::min(n, kGraphMaxIters);
    return OIVA_OK;
}

// ---- batched OGIVE (reference ive.py:33-256, one problem per batch entry) -------------------------------------------------
oiva_status oiva_batch_get_cx(oiva_batch* b, void* Cx_host, int f64) {
    NEED(b && Cx_host, OIVA_ERR_ARG, "null argument");
    NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    const size_t n = nbins(b) * b->M * b->M;
    const size_t bytes = n * (f64 ? sizeof(double2) : sizeof(float2));
    void* full = nullptr;
    HIP_TRY(hipMalloc(&full, bytes));
    hipError_t e = launch_unpack_herm(b->stream, b->Cx, full, f64 != 0, (long long)nbins(b), b->M);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(Cx_host, full, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(full);
    HIP_TRY(e);
    return OIVA_OK;
}

oiva_status oiva_batch_ogive_begin(oiva_batch* b, int update_mode, int model) {
    NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    NEED(!b->ragged, OIVA_ERR_ARG, "OGIVE is not supported on a ragged batch");
    int rc = check_ready(b);
    if (rc) return rc;
    NEED(b->K == 1, OIVA_ERR_ARG, "OGIVE extracts one source: create the batch with K = 1");
    NEED(update_mode >= OIVA_OGIVE_DEMIX && update_mode <= OIVA_OGIVE_SWITCHING, OIVA_ERR_ARG, "unknown update mode");
    NEED(model == OIVA_MODEL_LAPLACE || model == OIVA_MODEL_GAUSS, OIVA_ERR_ARG, "unknown model");
    DeviceGuard guard(b->device);
    const size_t nb = nbins(b), M = b->M, B = b->B;
    if (b->og_bufs.empty()) {
        hipError_t e = hipSuccess;
        auto alloc = [&](size_t bytes) -> void* {
            void* ptr = nullptr;
            if (e == hipSuccess) e = hipMalloc(&ptr, bytes);
            if (ptr) b->og_bufs.push_back(ptr);
            return ptr;
        };
        OgiveState& st = b->og.bin;
        st.CxInv = (double2*)alloc(nb * M * M * sizeof(double2));
        st.CxNorm = (double*)alloc(nb * sizeof(double));
        st.A = (double2*)alloc(nb * M * sizeof(double2));
        st.Delta = (double2*)alloc(nb * M * sizeof(double2));
        st.Lambda = (double*)alloc(nb * sizeof(double));
        st.DoA = (int*)alloc(nb * sizeof(int));
        st.DoW = (int*)alloc(nb * sizeof(int));
        st.Dnorm = (double*)alloc(nb * sizeof(double));
        st.ctrl = (int*)alloc(4 * sizeof(int));                 // (reset by ogive_init_kernel; the batch keeps its own per problem)
        st.maxdelta = (double*)alloc(2 * sizeof(double));
        b->og.done = (int*)alloc(B * sizeof(int));
        b->og.epochs = (int*)alloc(B * sizeof(int));
        b->og.maxdelta = (double*)alloc(B * sizeof(double));
        b->og.runmax = (unsigned long long*)alloc(B * sizeof(unsigned long long));
        b->og.ticket = (unsigned*)alloc(B * sizeof(unsigned));
        b->Opart = (double*)alloc((size_t)b->osplit * nb * (2 * M + 1) * sizeof(double));
        if (e != hipSuccess) return fail_with(OIVA_ERR_HIP, std::string("allocation failed: ") + hipGetErrorString(e));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->og_graph) {                   // captured for the previous update mode / model
        HIP_TRY(hipGraphExecDestroy(b->og_graph));
        b->og_graph = nullptr;
    }
    b->og.bin.Cx = b->Cx;
    b->og.bin.What = b->What;
    b->og.bin.What64 = b->What64;
    b->og_mode = update_mode;
    b->og_model = model;
    // Cx^-1, ||Cx||, a from w, the step selection (ive.py:100-102,136-139,173-180) on all B*F bins
    HIP_TRY(launch_ogive_init(b->stream, b->og.bin, (int)nb, b->M, update_mode));
    HIP_TRY(hipMemsetAsync(b->og.done, 0, B * sizeof(int), b->stream));
    HIP_TRY(hipMemsetAsync(b->og.epochs, 0, B * sizeof(int), b->stream));
    HIP_TRY(hipMemsetAsync(b->og.maxdelta, 0, B * sizeof(double), b->stream));
    HIP_TRY(hipMemsetAsync(b->og.runmax, 0, B * sizeof(unsigned long long), b->stream));
    HIP_TRY(hipMemsetAsync(b->og.ticket, 0, B * sizeof(unsigned), b->stream));
    b->og_ready = true;
    return OIVA_OK;
}

oiva_status oiva_batch_ogive_iterate(oiva_batch* b, int first_epoch, int n, double step_size, double tol, int* epochs_run, int* converged,
                                 double* max_delta) {
    NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    NEED(!b->ragged, OIVA_ERR_ARG, "OGIVE is not supported on a ragged batch");
    int rc = check_ready(b);
    if (rc) return rc;
    NEED(b->og_ready, OIVA_ERR_STATE, "call oiva_batch_ogive_begin first");
    NEED(n >= 0 && first_epoch >= 0, OIVA_ERR_ARG, "negative epoch count");
    DeviceGuard guard(b->device);
    const int B = b->B;
    std::vector<int> before(B), after(B);
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(before.data(), b->og.epochs, B * sizeof(int), hipMemcpyDeviceToHost));
    const int amodel = b->og_model == OIVA_MODEL_LAPLACE ? kModelOgiveLaplace : OIVA_MODEL_GAUSS;
    const DenseArgs d = dense_args(b);
    // one epoch is five launches on the batch's stream (four when the switching criterion does not run)
    auto epochs = [&](int e0, int count) -> int {
        for (int e = e0; e < e0 + count; ++e) {
            if (b->og_mode == OIVA_OGIVE_SWITCHING && e % 10 == 0)
                HIP_TRY(launch_batch_ogive_switch(b->stream, b->og, B, b->F, b->M));                     // ive.py:192-193
            HIP_TRY(launch_batch_ogive_power(b->stream, b->X, b->What, b->Ppart, b->og.done, B, d.T, b->F, b->M, d.pw_nsplit,
                                             d.tcp));                                                     // ive.py:196, :210/:213
            HIP_TRY(launch_batch_ogive_activation(b->stream, b->Ppart, b->nb, b->R, d.r_stride, b->og.done, B, d.T, amodel,
                                                  b->F));                                                 // ive.py:209-217
            HIP_TRY(launch_batch_ogive_framesum(b->stream, b->X, b->What64, b->R, d.r_stride, b->og.done, b->Opart, B, d.T, b->F,
                                                b->M, b->osplit, b->otc));                                // ive.py:218-227
            HIP_TRY(launch_batch_ogive_step(b->stream, b->og, b->Opart, b->osplit, B, b->F, b->M, step_size, tol));   // ive.py:228-246
        }
        return OIVA_OK;
    };
    if (n >= kOgMinGraphEpochs) {
        // n epochs as one linear graph on the batch's stream, cached while (n, phase, step size, tol) stay the same
        const int phase = first_epoch % 10;
        if (!b->og_graph || b->og_graph_n != n || b->og_graph_phase != phase || b->og_graph_mu != step_size || b->og_graph_tol != tol) {
            if (b->og_graph) HIP_TRY(hipGraphExecDestroy(b->og_graph));
            b->og_graph = nullptr;
            hipGraph_t graph = nullptr;
            HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
            rc = epochs(phase, n);
            hipError_t e = hipStreamEndCapture(b->stream, &graph);
            if (rc) {
                if (graph) (void)hipGraphDestroy(graph);
                return rc;
            }
            HIP_TRY(e);
            e = hipGraphInstantiate(&b->og_graph, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIP_TRY(e);
            b->og_graph_n = n;
            b->og_graph_phase = phase;
            b->og_graph_mu = step_size;
            b->og_graph_tol = tol;
        }
        HIP_TRY(hipGraphLaunch(b->og_graph, b->stream));
    } else if ((rc = epochs(first_epoch, n))) {
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(after.data(), b->og.epochs, B * sizeof(int), hipMemcpyDeviceToHost));
    if (epochs_run)
        for (int p = 0; p < B; ++p) epochs_run[p] = after[p] - before[p];
    if (converged) HIP_TRY(hipMemcpy(converged, b->og.done, B * sizeof(int), hipMemcpyDeviceToHost));
    if (max_delta) HIP_TRY(hipMemcpy(max_delta, b->og.maxdelta, B * sizeof(double), hipMemcpyDeviceToHost));
    return OIVA_OK;
}

// ---- batched PCA front end (reference auxiva_pca.py:63-92, one problem per batch entry) -------------------------------------
oiva_status oiva_batch_set_w_pca(oiva_batch* b, double* evals_host) {
    NEED(b != nullptr, OIVA_ERR_ARG, "null batch");
    NEED(b->have_cx, OIVA_ERR_STATE, "input covariance not computed (oiva_batch_covariance)");
    DeviceGuard guard(b->device);
    // auxiva_pca.py:75-81 per bin, the device eigensolver on B*F bins; the eigenvalues pass through Vpart (free between the
    // covariance and the first iteration, at least B*F*M*M doubles)
    double* evals = evals_host ? b->Vpart : nullptr;
    HIP_TRY(launch_pca_subspace(b->stream, b->Cx, b->What, b->What64, evals, (int)nbins(b), b->M, b->K, false));
    b->have_w = true;
    if (evals_host) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipMemcpy(evals_host, evals, nbins(b) * b->M * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (b->K < b->M) HIP_TRY(launch_update(b->stream, update_args(b, true)));   // J from the orthogonality constraint
    return OIVA_OK;
}

oiva_status oiva_batch_project_dev(oiva_batch* b, void** Xr_dev) {
    NEED(Xr_dev != nullptr, OIVA_ERR_ARG, "null argument");
    *Xr_dev = nullptr;
    const int rc = check_ready(b);
    if (rc) return rc;
    DeviceGuard guard(b->device);
    if (!b->Xr) HIP_TRY(hipMalloc((void**)&b->Xr, b->frames_total * b->F * b->K * sizeof(float2)));
    // auxiva_pca.py:79-81 for every problem in one launch, from the problem table
    HIP_TRY(launch_pca_project(b->stream, b->X, b->What, b->Xr, b->probs_dev, b->B, b->F, b->M, b->K, b->kp, b->pw_nsplit));
    HIP_TRY(hipStreamSynchronize(b->stream));
    *Xr_dev = b->Xr;
    return OIVA_OK;
}

oiva_status oiva_batch_compose_w(oiva_batch* outer, const oiva_batch* inner) {
    NEED(outer != nullptr && inner != nullptr, OIVA_ERR_ARG, "null batch");
    NEED(outer != inner, OIVA_ERR_ARG, "the reduced batch must be another batch");
    NEED(inner->B == outer->B && inner->F == outer->F, OIVA_ERR_ARG, "the two batches differ in B or F");
    NEED(inner->M == inner->K && inner->K == outer->K, OIVA_ERR_ARG,
         "the reduced batch must be determined on the K channels of the projection");
    NEED(inner->device == outer->device, OIVA_ERR_ARG, "the two batches live on different devices");
    NEED(outer->have_w && inner->have_w, OIVA_ERR_STATE, "demixing matrices not set");
    DeviceGuard guard(outer->device);
    HIP_TRY(hipStreamSynchronize(inner->stream));
    HIP_TRY(launch_pca_compose(outer->stream, outer->What, outer->What64, inner->What64, (long long)nbins(outer), outer->M, outer->K));
    return OIVA_OK;
}

}  // extern "C"
