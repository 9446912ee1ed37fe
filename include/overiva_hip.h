/*
 * overiva_hip.h -- C ABI of liboveriva_hip.so: the MI355X (gfx950) implementation of the
 * AuxIVA / OverIVA iteration hot path of onolab-tmu/overiva.
 *
 * The reference has no FFI: its boundary for this path is the Python call
 *     overiva(X, n_src, n_iter, proj_back, W0, model, init_eig, return_filters, callback)
 * (reference overiva.py:28-38) and auxiva_pca(X, n_src, **kwargs) (auxiva_pca.py:30).
 * The entry points below are what a ctypes binding placed inside those two functions binds;
 * each one names the reference statements it replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative OIVA_ERR_* otherwise;
 *     oiva_last_error() then returns a thread-local message.
 *   - complex arrays are interleaved float32 (re, im) = numpy complex64, C order.
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device memory
 *     on the plan's device.  The caller owns every buffer it passes in; the plan owns
 *     everything it allocates; nothing returned by pointer outlives oiva_plan_destroy.
 *   - one plan = one device + one stream + one contiguous range of frequency bins.
 *     A plan is not thread-safe; distinct plans are independent.
 *   - every entry point restores the calling thread's current device.
 *   - no call synchronises with the host except the ones documented to (copies to host,
 *     oiva_plan_sync, the timing helpers).
 */
#ifndef OVERIVA_HIP_H
#define OVERIVA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define OIVA_OK 0
#define OIVA_ERR_ARG (-1)      /* bad argument / unsupported shape */
#define OIVA_ERR_HIP (-2)      /* a HIP runtime call failed */
#define OIVA_ERR_STATE (-3)    /* call order violated (e.g. iterate before X was set) */
#define OIVA_ERR_NUMERIC (-4)  /* non-finite demixing matrix (numpy raises LinAlgError here) */

#define OIVA_MODEL_LAPLACE 0   /* overiva.py:152-153, :161-163 */
#define OIVA_MODEL_GAUSS 1     /* overiva.py:154-155, :164-167 */

/* Documented limit (the reference has none): at most 32 channels.  1..16 channels run the kernels tuned per shape; 17..32
 * run one generic wide path (kernels_wide.hip), selected by the channel count alone.  oiva_plan_create rejects more with
 * OIVA_ERR_ARG. */
#define OIVA_MAX_CHANNELS 32

/* Arithmetic of a plan (oiva_plan_set_precision).  Device data (X, Y, the W the streaming kernels read) is always
 * complex64; these bits choose where float64 is used on top of it.
 *   0                      : float32 everywhere (fp32 matrix-core chains of 8 frames folded into float64).
 *   OIVA_PREC_UPDATE_F64   : the per-bin algebra (overiva.py:181-190) in float64, W_hat carried in complex128.
 *   OIVA_PREC_COV_F64      : the weighted covariance (overiva.py:179) as float64 sums of exact float64 products (up to 8
 *                            channels: v_fma_f64 on the vector ALU; 9..16: fp64 matrix cores) -- the reference's own
 *                            arithmetic there: its float64 r_inv promotes that product to complex128 even for
 *                            complex64 input (overiva.py:127-128).
 *   OIVA_PREC_PRECISE      : both; what overiva() selects for complex128 input.
 *   OIVA_PREC_UPDATE_ROWS  : lane layout of the per-bin algebra (one lane per matrix row instead of per element). */
#define OIVA_PREC_FAST 0
#define OIVA_PREC_UPDATE_F64 1
#define OIVA_PREC_UPDATE_ROWS 2
#define OIVA_PREC_COV_F64 4
#define OIVA_PREC_PRECISE (OIVA_PREC_UPDATE_F64 | OIVA_PREC_COV_F64)

typedef struct oiva_plan oiva_plan;

/* library */
int oiva_version(void);
const char *oiva_last_error(void);
int oiva_device_count(int *n);

/*
 * Plan life cycle.  T frames, F bins OWNED BY THIS PLAN, M channels, K sources (1 <= K <= M),
 * F_total = number of bins of the whole problem (== F for a single-GPU run; > F when the bins are
 * sharded over several plans/GPUs -- only the gauss model's 1/F (overiva.py:155) depends on it).
 * stream: a hipStream_t to launch on (e.g. the framework's current stream), or NULL for a
 * plan-owned stream.
 */
int oiva_plan_create(oiva_plan **out, int device, int T, int F, int M, int K, int model, int F_total,
                     void *stream);
int oiva_plan_destroy(oiva_plan *p);

/*
 * Input  X (T, F, M) complex64  -- replaces the copy at overiva.py:132 (the transpose there is
 * not needed: kernels read the native (frames, bins, channels) order).
 * _host: copies rows of F*M complex from a host array whose consecutive frames are
 *        row_pitch_bytes apart (pass F_total*M*8 and a pointer to bin f0 to upload a bin shard
 *        of a larger array; 0 means dense).  Synchronous.
 * _dev : borrows a dense device array (no copy); it must stay valid while the plan uses it.
 */
int oiva_plan_set_x_host(oiva_plan *p, const void *X, long long row_pitch_bytes);
int oiva_plan_set_x_dev(oiva_plan *p, const void *X_dev);
/* _host_c128: as _host for a complex128 array (pitch in bytes of complex128 rows); the conversion to the device's
 * complex64 runs on the GPU, so the host never touches the data (reference overiva.py:132 copies X once too). */
int oiva_plan_set_x_host_c128(oiva_plan *p, const void *X, long long row_pitch_bytes);

/*
 * Prologue, step 1: Cx[f] = (1/T) sum_t x x^H  (overiva.py:87).  Must follow set_x.
 */
int oiva_plan_covariance(oiva_plan *p);
/* Cx as (F, M, M) complex64 (f64 = 0) or complex128 (f64 != 0) on the host (used by the host-side init_eig
 * path, overiva.py:106-109, and by auxiva_pca, auxiva_pca.py:71-75). */
int oiva_plan_get_cx(oiva_plan *p, void *Cx_host, int f64);

/*
 * Prologue, step 2: demixing matrix  (overiva.py:89-123).
 * W0_host: (F, M, K) complex64 (f64 = 0) or complex128 (f64 != 0), or NULL for the identity start
 * (overiva.py:113-114).  Builds W_hat = [W | [J; -I]] with J from the orthogonality constraint
 * (overiva.py:96-98,120-123).
 */
int oiva_plan_set_w(oiva_plan *p, const void *W0_host, int f64);

/*
 * n iterations of the loop body overiva.py:138-190 (demix -> activation r -> scale normalisation
 * -> for every source: weighted covariance V, IP1 row solve, normalisation, J update).
 * Only valid when the plan owns all bins (F == F_total).  Asynchronous.
 */
int oiva_plan_iterate(oiva_plan *p, int n);

/*
 * The same iteration cut at its one cross-bin dependency (overiva.py:152-155: r needs all bins),
 * for bin-sharded multi-GPU runs:
 *   oiva_plan_power   : partial powers of THIS plan's bins, one (T, K) float32 part per batch of 64 bins:
 *                       part[b][t,k] = sum over the batch's bins of |w_k^H x|^2.  They live in the device
 *                       buffer returned by oiva_plan_power_buffer, laid out (parts_per_rank, T, K) with the
 *                       parts this plan does not own left at zero (parts_per_rank = the largest batch
 *                       count of any rank, so that every rank contributes an equally sized message).
 *   (caller all-gathers the buffers of all ranks into parts_dev, (G * parts_per_rank, T, K) float32)
 *   oiva_plan_update  : r from the sum over parts in buffer order (rank, then batch: fixed, so every
 *                       rank gets the same bits), then the per-bin part of the iteration
 *                       (overiva.py:158-173 gamma / 1/r, :161-167 W scaling, :176-190).
 */
int oiva_plan_power(oiva_plan *p);
int oiva_plan_power_buffer(oiva_plan *p, int parts_per_rank, void **parts_dev, long long *bytes);
int oiva_plan_update(oiva_plan *p, const void *parts_dev, int nparts);

/*
 * Epilogue: Y = demix(X, W) as (T, F, K) complex64 (overiva.py:192-195), optionally scaled by
 * projection back onto channel 0 (overiva.py:197-199; also the callback payload of :142-148).
 * row_pitch_bytes as in set_x_host (0 = dense).  Synchronous.  Outputs of more than a few MB leave in slabs of frames:
 * slab k is computed while slab k - 1 crosses PCIe into a pinned ring and slab k - 2 is moved into Y_host by a small pool
 * of copy threads ($OIVA_IO_THREADS, default min(8, cores / 2); $OIVA_DEMIX_IO = legacy | ring | register, see
 * csrc/plan.hip demix_to_host).  A Y_host whose pages are already faulted in is served much faster than a fresh
 * allocation: oiva_host_prefault does that, from the pool's threads, e.g. while the iterations run.
 */
int oiva_plan_demix(oiva_plan *p, void *Y_host, long long row_pitch_bytes, int proj_back);
/* Device buffers of >= 16 MB that a destroyed plan owned (its copy of X, Y, staging) stay in a process-wide pool for the next
 * plan of the same shape -- at most $OIVA_POOL_MB (default 2048; 0: nothing is kept).  This releases them to the driver; the
 * library does so itself, and retries, before a device allocation of its own fails for want of memory. */
int oiva_pool_trim(void);
/* Bytes of output per slab of the hand-over above (0: the default, 8 MB).  Test hook. */
int oiva_plan_set_io_slab(oiva_plan *p, long long bytes);
/* Fault the pages of [ptr, ptr + bytes) in for writing, contents unchanged, using the library's copy threads.  Blocking;
 * callable from any thread (overiva() runs it on the array it will return while the queued iterations run on the GPU; beside the
 * upload of X it slowed the upload by as much as it saved: dropped, round 5). */
int oiva_host_prefault(void *ptr, long long bytes);
/* Same, but Y stays on the device: *Y_dev is the plan's own (T, F, K) complex64 buffer, valid until the next demix of
 * this plan or its destruction.  Hand it to oiva_plan_set_x_dev of another plan to chain two solves without a host
 * round trip (the PCA front-end of auxiva_pca.py:79-87).  Synchronous. */
int oiva_plan_demix_dev(oiva_plan *p, int proj_back, void **Y_dev);
/* As oiva_plan_demix, into a complex128 host array (the dtype overiva() returns for complex128 input); converted on
 * the device. */
int oiva_plan_demix_c128(oiva_plan *p, void *Y_host, long long row_pitch_bytes, int proj_back);

/*
 * Push exchange of the per-rank partial powers between the GPUs of one node -- the all-gather in front of the activation
 * (overiva.py:152-155) written for its 100 KB payload: every rank stores its part straight into every rank's gather
 * buffer (fine-grained device memory shared through hipIpcMemHandle, peer stores over xGMI) and signals a counter; a
 * rank's stream waits on its counter with a command-processor wait.  Same result layout as an all-gather (rank-major
 * parts), so oiva_plan_update() takes the buffer as is.  Epochs count the exchanges, from 1, identically on every rank.
 *   create   : allocate this rank's buffer for parts of part_bytes each
 *   export   : OIVA_XCHG_HANDLE_BYTES bytes to hand to every other rank (any host-side transport)
 *   connect  : map the other ranks' buffers; handles = world * OIVA_XCHG_HANDLE_BYTES bytes in rank order
 *   push     : on `stream`, after whatever produced part_dev: store it into slot `rank` everywhere, then signal
 *   wait     : `stream` waits until all `world` parts of this epoch are in this rank's buffer
 *   gathered : the buffer to read after wait (world parts of the padded part size, rank order)
 *   poll     : host-side check with a time-out (used to validate the transport before relying on it)
 *   force    : host store of the value a stream wait of this epoch waits for -- releases a stream whose wait would
 *              never be satisfied (a validation that failed); the exchange must not be used afterwards
 */
#define OIVA_XCHG_MAX_RANKS 16
#define OIVA_XCHG_HANDLE_BYTES 64
typedef struct oiva_xchg oiva_xchg;
int oiva_xchg_create(oiva_xchg **x, int device, int rank, int world, long long part_bytes);
int oiva_xchg_export(oiva_xchg *x, void *handle);
int oiva_xchg_connect(oiva_xchg *x, const void *handles);
int oiva_xchg_push(oiva_xchg *x, void *stream, const void *part_dev, long long part_bytes, int epoch);
int oiva_xchg_wait(oiva_xchg *x, void *stream, int epoch);
int oiva_xchg_gathered(oiva_xchg *x, int epoch, void **gathered);
int oiva_xchg_poll(oiva_xchg *x, int epoch, int timeout_ms, int *arrived);
int oiva_xchg_force(oiva_xchg *x, int epoch);
int oiva_xchg_destroy(oiva_xchg *x);

/*
 * PCA front-end of auxiva_pca (auxiva_pca.py:71-81): W := the eigenvectors of the K largest eigenvalues of the input
 * covariance, in ascending order of the eigenvalue (numpy.linalg.eigh's w[:, :, -K:]), from a Jacobi eigensolver on
 * the device (float64, one wavefront per bin); the orthogonality constraint fills J as in oiva_plan_set_w.  A following
 * demix gives new_X = X conj(w[:, :, -K:]).  The phase of each eigenvector is unspecified (as LAPACK's is a convention);
 * results after projection back do not depend on it.  evals_host: NULL or (F, M) float64, all eigenvalues ascending.
 */
int oiva_plan_set_w_pca(oiva_plan *p, double *evals_host);
/* init_eig of overiva.py:106-109: W := conj of the K principal eigenvectors of the input covariance, each with the
 * phase numpy.linalg.eig (LAPACK zgeev) gives it -- largest component real and positive.  Same eigensolver. */
int oiva_plan_set_w_eig(oiva_plan *p);
/* W (F, M, K) complex64 (f64 = 0) or complex128 (f64 != 0) -- the view returned at overiva.py:201-202.
 * Synchronous.  Returns OIVA_ERR_NUMERIC if W holds a non-finite value (W is still copied out). */
int oiva_plan_get_w(oiva_plan *p, void *W_host, int f64);

int oiva_plan_sync(oiva_plan *p);
/* A copy of the demixing state W_hat on the device, made / brought back on the plan's stream (asynchronous, ordered with the
 * iterations around it): what a caller of the in-kernel exchanges keeps to fall back on when a rank does not deliver. */
int oiva_plan_save_w(oiva_plan *p);
int oiva_plan_restore_w(oiva_plan *p);

/*
 * Measurement.  Runs n iterations bracketed by HIP events on the plan's stream and, when
 * per_kernel_ms is non-NULL, additionally brackets every kernel launch with events (eager
 * launches) and returns the summed time of each stage in per_kernel_ms[0..3]:
 * [0] demix+power pass, [1] source activation (r, gamma, 1/r), [2] weighted-covariance pass,
 * [3] per-bin update.  total_ms = wall time of the n iterations on the device.  Synchronous.
 */
int oiva_plan_iterate_timed(oiva_plan *p, int n, float *total_ms, float *per_kernel_ms);
#define OIVA_N_STAGES 4

/* Launch geometry of the weighted-covariance pass, for roofline accounting and tuning:
 * get/set the number of frame splits (0 = library default). */
int oiva_plan_get_cov_splits(oiva_plan *p, int *nsplit);
int oiva_plan_set_cov_splits(oiva_plan *p, int nsplit);
/* Which kernel takes the covariance pass of a 9..16-channel plan: 1 (default) = the vector-ALU kernels
 * that form the Hermitian half and write float64 partial sums -- float32 products: four lanes per (bin, frame) for up to 4
 * sources (csrc/kernels_cov_quad.hip; 3 and 4 sources only with the float64 per-bin algebra), 32 lanes per (bin, frame) and
 * every source in one pass for 5..16 (csrc/kernels_cov_half16.hip); OIVA_PREC_COV_F64: the float64 form of the latter for
 * 3..16 sources; a plan with 9, 11, 13 or 15 channels runs them on its own copy of X padded by one zero channel per bin
 * ((M + 1) / M of X more device memory, filled by oiva_plan_covariance) -- 0 = the planar matrix-core kernel, which
 * OIVA_PREC_COV_F64 with one or two sources always uses.  *active (may be NULL) receives whether a vector-ALU kernel is what this plan now launches.  Drops captured
 * graphs. */
int oiva_plan_set_cov_quad(oiva_plan *p, int enable, int *active);
/* same for the demix+power pass (0 = library default) */
int oiva_plan_set_pow_splits(oiva_plan *p, int nsplit);
/* 10..16 channels with 9..16 sources: the covariance pass with the sources on the fp32 matrix cores (default, csrc/kernels_cov_hmfma.hip)
 * or on the vector ALU alone (enable = 0; same bits: A/B tests). */
int oiva_plan_set_cov_hmfma(oiva_plan *p, int enable);
/* 8 channels, 2 sources + background, float32 covariance products, four frame splits (the headline shape): the weighted
 * covariance (overiva.py:179) and the per-bin update of the same bins (:181-190) as ONE launch (csrc/kernels_cov_update.hip; same
 * bits as the two launches; measured no faster, so off by default: $OIVA_COV_UPDATE=1 or enable = 1).  enable 1 / 0; -1 only
 * asks.  *active: whether this plan's iterations run it. */
int oiva_plan_set_fuse_cov_update(oiva_plan *p, int enable, int *active);
/* Frame order of the demix+power pass at up to 8 channels (and up to 4 sources beyond): 1 (default; $OIVA_POWER_REVERSE=0 at
 * plan creation: 0) = against the covariance pass -- the frame chunks are handed out from the tail of every covariance split to
 * its head and each is walked descending, so that each of the two passes over X starts on what the other left in the last-level
 * cache; 0 = ascending.  Which chunk a row of the grid takes only matters when the grid runs in several rounds of workgroups
 * (a long frame axis), so only then are the chunks re-ordered; 2 (a test hook, $OIVA_POWER_REVERSE=2) re-orders them in a grid
 * of one round too.  Same bits in every setting (frames are independent in this pass).  Drops captured graphs. */
int oiva_plan_set_power_reverse(oiva_plan *p, int enable);
/* Load policy of X in the two streaming passes at 8 channels, float32 sums (cov_dma_kernel, power_kernel; csrc/kernel_choice.h, DESIGN
 * §3): up to `mb` MB (1e6 bytes) of X -- a fixed set of frame groups, the same in both passes and in every iteration -- are read
 * with plain loads and may stay in the last-level cache; the rest streams with non-temporal loads.  The share is as many
 * sixteenths of X as mb holds; frame by frame it can exceed them, and so mb, by up to 64 frames per covariance split (a split
 * that ends inside a period of 16 groups).  mb <= 0: off, every load plain.  X that fits the budget whole is read plain throughout.  Default: $OIVA_X_RESIDENT_MB at plan creation, else the
 * library's figure.  Same bits in every setting (only the load instructions differ).  Drops captured graphs. */
int oiva_plan_set_x_resident_mb(oiva_plan *p, double mb);
/* What that policy is for the plan's present geometry: *n16 of every 16 frame groups are resident; *nt: the others stream
 * non-temporally (0: every load is plain); *reason: 0 off, 1 X fits the budget whole, 2 the passes run other kernels, 3 the
 * geometry does not keep every load step inside one frame group, 4 a share was chosen. */
int oiva_plan_get_x_resident(oiva_plan *p, int *n16, int *nt, int *reason);
/* Where that policy streams (reason 4), the covariance pass at 8 channels runs the row instantiation of its kernel: every load
 * step requested row by row, resident groups plain and streamed groups non-temporal at the same addresses, through a shorter
 * ring (csrc/kernels_cov.hip).  enable == 0 ($OIVA_COV_ROWS=0 at plan creation) forces the lane-addressed
 * instantiation that every other plan runs: for A/B measurements and for the tests.  Same bits either way.  Drops captured
 * graphs.  oiva_plan_get_cov_rows: *rows = 1 where the next covariance launch takes the row instantiation, else 0. */
int oiva_plan_set_cov_rows(oiva_plan *p, int enable);
int oiva_plan_get_cov_rows(oiva_plan *p, int *rows);
/* Replay the iteration from a captured hipGraph instead of eager launches (default off). */
int oiva_plan_use_graph(oiva_plan *p, int enable);
/* Arithmetic: an OR of OIVA_PREC_* (default OIVA_PREC_FAST).  Call it before oiva_plan_covariance so that the
 * prologue runs in the same arithmetic. */
int oiva_plan_set_precision(oiva_plan *p, int flags);

/*
 * X-resident iteration: the loop body of overiva.py:138-190 (demix + power, activation, weighted covariance, IP1
 * solve + normalisation, orthogonal-constraint update of J) fused into ONE persistent launch per oiva_plan_iterate
 * call, with the plan's slice of X held in the chip's registers + LDS for all n iterations (X leaves HBM once per
 * call instead of twice per iteration).  Applies when the slice fits on chip -- 16 bins x <= 256 frames per compute
 * unit: BASELINE configs[1], one rank's 256-bin shard of the headline shape -- with 4 or 8 channels, 1 or 2 sources
 * (K < M) and a float32 covariance pass; see csrc/resident_kernel.inc.
 *   oiva_plan_set_resident   : enable = 1 turns it on (OIVA_ERR_ARG when the shape does not qualify), 0 off.
 *                              With it on, oiva_plan_iterate is synchronous; a launch whose workgroups could not all
 *                              become resident gives up after the time-out WITHOUT having changed W, the plan falls
 *                              back to the four-launch path for that call and all later ones, and the reason is kept
 *                              (info[8]).
 *   oiva_plan_resident_info  : info[0] shape qualifies, [1] enabled, [2] bin groups, [3] frame splits, [4] frames per
 *                              split, [5] frames per lane, [6] of them in registers, [7] LDS bytes per workgroup,
 *                              [8] give-up code of the last failed launch (0: none), [9] resident launches so far,
 *                              [10] fall-backs so far, [11] the frames of X each compute unit holds, in bytes
 *   oiva_plan_resident_phases: average duration in microseconds, over the iterations of the last resident launch
 *                              (at most 256), of the phases of workgroup 0, from the 100 MHz clock read inside the
 *                              kernel: [0] demix + power, [1] the column's parts (wait + ordered sum), [2] activation,
 *                              [3] weighted covariance: accumulation, [4] its reduction over the frame phases + publication,
 *                              [5] wait for the row's partials, [6] per-bin update chain, [7] wait for the row's
 *                              demixing vectors; *n_iter = iterations covered (0: nothing recorded)
 *   oiva_plan_resident_debug : test hooks -- time-out of a wait in milliseconds (0: default 250, 2000 when sharded over processes), and the index of a
 *                              workgroup that never publishes (-1: none), which makes the launch give up;
 *                              _debug_from: the workgroup stops publishing in that iteration of a launch (0-based)
 *   oiva_plan_resident_loopback: world >= 2: ONE GPU runs the multi-GPU exchange of the kernel against itself -- per
 *                              frame split a leader workgroup gathers the rank's parts and stores the sums of all
 *                              `world` slots (its own, exact zeros for the others) into a gather buffer of the same kind
 *                              of memory the ranks of a sharded run map from each other, every workgroup adds the
 *                              slots in rank order: the leader hop and the world-slot sum of bench.py --gpus N on one
 *                              GPU (everything but the flight over xGMI), with the result of world = 1.  0 / 1: off.
 *                              Call it while resident is off; the plan must own all bins.
 */
struct oiva_xchg;
#define OIVA_RESIDENT_INFO 12
#define OIVA_RESIDENT_PHASES 8
int oiva_plan_set_resident(oiva_plan *p, int enable);
int oiva_plan_resident_info(oiva_plan *p, int *info /* OIVA_RESIDENT_INFO ints */);
int oiva_plan_resident_phases(oiva_plan *p, double *phase_us /* OIVA_RESIDENT_PHASES */, int *n_iter);
int oiva_plan_resident_debug(oiva_plan *p, int timeout_ms, int stall_block);
int oiva_plan_resident_debug_from(oiva_plan *p, int timeout_ms, int stall_block, int first_stalled_iteration);
int oiva_plan_resident_loopback(oiva_plan *p, int world);
/* Diagnostics: with enable != 0 the next resident launches (of at most 64 iterations) record the timestamps of EVERY
 * workgroup; stamps_host (NULL: just switch) receives [n_wg][n_iter][OIVA_RESIDENT_STAMPS] 100 MHz ticks of the last one. */
#define OIVA_RESIDENT_STAMPS 16
int oiva_plan_resident_trace(oiva_plan *p, int enable, unsigned long long *stamps_host, int *n_wg, int *n_iter);
/* Bins sharded over the GPUs of a node: give the plan of a shard a connected oiva_xchg (below) whose slot is
 * frame_splits * frames_per_split * K * 4 bytes; the resident kernel then exchanges the ranks' partial source powers
 * (overiva.py:152-155) itself -- one workgroup per frame split stores the rank's sums into every rank's buffer (peer
 * stores over xGMI), every workgroup adds the ranks' sums in rank order -- and oiva_plan_iterate works on a shard
 * (F < F_total).  Every rank must call oiva_plan_iterate with the same counts.  A launch that gives up returns
 * OIVA_ERR_STATE (nothing written).  x = NULL disconnects. */
int oiva_plan_resident_connect(oiva_plan *p, struct oiva_xchg *x);
/*
 * The same exchange for shards that do NOT fit on chip (2 and 4 GPUs at the headline shape), inside the four-launch
 * iteration: give the plan a connected oiva_xchg whose slot is T * K * 8 bytes; the ACTIVATION kernel then adds its rank's
 * 64-bin parts, stores the sum of every (frame, source) -- one 8-byte {value, epoch} word -- into its slot of every other
 * rank's buffer (peer stores over xGMI), polls its own buffer for the other ranks' words and adds the ranks' sums in rank
 * order (overiva.py:152-155; the same bits of r on every rank).  No collective, no stream wait, no host in the loop:
 * oiva_plan_iterate works on a shard (F < F_total) and replays captured graphs of four kernels per iteration.  Every rank
 * must run the same number of iterations.  Connecting zeroes the rank's own gather buffer and restarts the epochs: the ranks
 * must rendezvous (any barrier of the host side) between their connects and their first iteration.  A wait that gives
 * up (default 2 s) is reported by the next oiva_plan_sync / oiva_plan_get_w / oiva_plan_demix* (OIVA_ERR_STATE); the demixing
 * matrices of the iterations since are undefined: oiva_plan_save_w before, oiva_plan_restore_w after.  x = NULL disconnects
 * and clears the condition.
 *   oiva_plan_fused_loopback: world >= 2: ONE GPU runs that exchange against itself (own buffer, the other ranks' sums are
 *                             zeros: the result is the single-GPU one up to the association of the sum); 0 / 1: off.
 *   oiva_plan_fused_debug   : test hooks -- time-out of a wait in milliseconds (0: default); stall != 0: in loop-back the other
 *                             ranks' words are never stored (a rank that does not deliver)
 */
int oiva_plan_fused_connect(oiva_plan *p, struct oiva_xchg *x);
int oiva_plan_fused_loopback(oiva_plan *p, int world);
int oiva_plan_fused_debug(oiva_plan *p, int timeout_ms, int stall);
/* Number of frame splits of the resident grid (0: the library's choice).  The ranks of a sharded run must use one
 * geometry: they agree on the smallest count any of them chose (uneven shards).  Call it while resident is off. */
int oiva_plan_set_resident_splits(oiva_plan *p, int nsplit);

/*
 * Test-only stage access (per-kernel parity tests call these through the same ABI).
 * Stages run on the plan's current state; getters synchronise.
 */
int oiva_test_set_rinv(oiva_plan *p, const float *rinv_host /* (T,K) */);
int oiva_test_get_rinv(oiva_plan *p, float *rinv_host /* (T,K) */, float *wscale_host /* (K) */);
int oiva_test_run_weighted_cov(oiva_plan *p);                 /* overiva.py:179 for all K sources */
int oiva_test_get_v(oiva_plan *p, void *V_host /* (K,F,M,M) complex64 | complex128 */, int f64);
int oiva_test_run_update(oiva_plan *p);                       /* overiva.py:181-190 for s = 0..K-1 */
int oiva_test_get_what(oiva_plan *p, void *What_host /* (F,M,M) complex64 | complex128 */, int f64);
int oiva_test_set_what(oiva_plan *p, const void *What_host, int f64);
int oiva_test_run_power(oiva_plan *p, float *p_host /* (T,K) summed over this plan's bins */);
/* the partial powers of the last power pass as they lie on the device: *nparts 64-bin parts of (T, K) floats (parts_host NULL:
 * only the count) */
int oiva_test_get_ppart(oiva_plan *p, float *parts_host, int *nparts);
/* host only: order[y] = the frame chunk that row y of the power pass's grid takes (nsplit chunks of tcp frames) against a
 * covariance pass of cov_splits splits of cov_tc frames */
int oiva_test_power_order(int nsplit, int tcp, int cov_splits, int cov_tc, int *order);
/* average duration of `reps` back-to-back launches of one stage (0 power, 1 activation, 2 covariance,
 * 3 update) on the plan's current state, HIP events on the plan's stream */
int oiva_test_time_stage(oiva_plan *p, int stage, int reps, float *avg_ms);
/* Test hook: device and pinned buffers the library has handed to its handles and temporaries and not yet taken back, and their
 * bytes, over all handles of the process.  A large buffer resting in the pool (oiva_pool_trim) counts as taken back. */
int oiva_test_live_buffers(long long *count, long long *bytes);
/* host only: the load policy of X (oiva_plan_set_x_resident_mb) for T frames of F bins x M channels, covariance splits of cov_tc
 * frames, power chunks of pow_tcp frames and a budget: out (3) = n16, nt, reason; cov_walk / pow_walk (T each): every frame as
 * the load steps of the covariance / power kernel meet it -- -1 never, 0 plain, 1 nt, 2 more than once */
int oiva_test_x_policy(int T, int F, int M, int cov_tc, int pow_tcp, double budget_mb, int *out, signed char *cov_walk, signed char *pow_walk);
/* host only: the policy a plan with these kernels and this geometry chooses (kinds as oiva_test_kernel_choice reports them):
 * out (3) = n16, nt, reason.  from_env != 0: the budget a plan created now starts with ($OIVA_X_RESIDENT_MB, else the library's
 * default) instead of budget_mb; *budget_used (may be NULL) receives the budget applied. */
int oiva_test_x_choice(int T, int F, int M, int prec_flags, int cov_kind, int cov_tc, int pow_kind, int pow_tcp, double budget_mb, int from_env,
                       int *out, double *budget_used);
/* host only: which instantiation of the 8-channel covariance kernel a plan with these kernels, this geometry, this budget and
 * this setting of oiva_plan_set_cov_rows launches (arguments as oiva_test_x_choice): *rows = 1 the row form, 0 the lane form */
int oiva_test_cov_rows(int T, int F, int M, int prec_flags, int cov_kind, int cov_tc, int pow_kind, int pow_tcp, double budget_mb, int rows_on,
                       int *rows);
/* Test hook: workgroups of cov_dma_kernel<M, kc> (rows != 0: of its row instantiation) that one CU of the current device holds */
int oiva_test_cov_blocks_per_cu(int M, int kc, int rows, int *n);
/* Test hook: the kernels and geometry a plan of this shape and these settings would run on `device` (csrc/kernel_choice.h), by
 * the functions a plan chooses with; nothing is allocated.  prec_flags: OIVA_PREC_*; quad_on / hmfma_on: the switches of
 * oiva_plan_set_cov_quad / _hmfma; *_splits_req: 0 or the splits asked for.  out (18): covariance kind, nsplit, tc, kc, nbg, pad,
 * part32, partials are float64, kind of the unit-weights pass; power kind, nb, nsplit, tcp, kp, rounds; the two occupancy
 * figures the choice asked the device for (covariance, power; -1: not asked, 0: the query failed); the device's CU count.
 * Kinds count from 0 in the order of CovKind / PowKind. */
int oiva_test_kernel_choice(int device, int T, int F, int F_total, int M, int K, int prec_flags, int quad_on, int hmfma_on,
                            int cov_splits_req, int pow_splits_req, int *out);
/* Test hook: the per-bin update kernel that is LAUNCHED for these fields of the update's arguments (channels, sources, float64
 * arithmetic, float64 partials, J initialisation only, row layout, covariance splits) and the process's switches ($OIVA_UPDATE_GRAM,
 * $OIVA_UPDATE_DET, $OIVA_DET16_INVERSE, $OIVA_DET16_ROWS).  The launch of one bin with null pointers is captured on a stream of
 * its own, so nothing runs and nothing is allocated; name (n bytes) receives the captured kernel node's function in the normal
 * form of csrc/kernel_choice.h, e.g. "update_sq_kernel<8, double, 8, 2>". */
int oiva_test_update_choice(int M, int K, int use_double, int vpart_f64, int init_only, int layout, int nsplit, char *name, int n);

/*
 * OGIVE -- orthogonally constrained independent vector extraction of ONE source by gradient steps, the reference's
 * ive.py::ogive(X, n_iter, step_size, tol, update, proj_back, W0, model, init_eig, return_filters, callback)
 * (ive.py:33-256; called at overiva_sim.py:313-315).  Runs on a plan created with K = 1 after oiva_plan_covariance
 * and oiva_plan_set_w (w = column 0: identity start ive.py:129-130, or W0 / the principal eigenvector from the host):
 *   oiva_plan_ogive_begin   : Cx^-1, ||Cx||, a from w, step selection                       ive.py:100-102,136-139,173-180
 *   oiva_plan_ogive_iterate : up to n epochs of ive.py:190-246 starting at epoch index first_epoch (the switching
 *                             criterion runs when the index is a multiple of 10).  The stopping rule max ||delta|| < tol
 *                             is evaluated on the device after every epoch; once met the state is frozen and the
 *                             remaining epochs of the call are no-ops.  Synchronous: returns the number of epochs that
 *                             changed the state and whether the rule was met.
 * The result is read with oiva_plan_demix / oiva_plan_get_w as for the other algorithms.
 */
#define OIVA_OGIVE_DEMIX 0
#define OIVA_OGIVE_MIX 1
#define OIVA_OGIVE_SWITCHING 2
int oiva_plan_ogive_begin(oiva_plan *p, int update_mode, int model);
int oiva_plan_ogive_iterate(oiva_plan *p, int first_epoch, int n, double step_size, double tol, int *epochs_run,
                            int *converged, double *max_delta);

/*
 * Batched OverIVA: B independent problems of one shape (T frames, F bins, M <= 8 channels, K sources) per set of launches
 * (kernels_batch.hip).  The life cycle mirrors a plan's; every stage serves all B problems at once and the iteration is four
 * launches whatever B (demix+power, activation, weighted covariance, per-bin update), replayed from one captured graph.
 * Arithmetic: always OIVA_PREC_PRECISE.  A problem's result does not depend on B or on its place in the batch: every sum is
 * ordered by the bin and frame within its own problem.
 *   X (B, T, F, M): host complex64 or complex128 (converted on the device), or a borrowed dense complex64 device array.
 *   W0 (B, F, M, K) complex64 or (f64) complex128, or NULL for the identity (overiva.py:113-117).
 *   Y (B, T, F, K) complex64 or complex128; W (B, F, M, K).
 *   oiva_batch_get_w copies W out even when it returns OIVA_ERR_NUMERIC (some problem's W holds non-finite values; the
 *   message names them); oiva_batch_status fills status[B] with 1 for such a problem, else 0 (both synchronise).
 *   oiva_batch_time_stages: n eager iterations with events around every stage; per_stage_ms[4] (demix_power, activation,
 *   weighted_cov, ip_update) per iteration, total_ms per iteration of a replay of the captured graph of n iterations.
 */
typedef struct oiva_batch oiva_batch;
int oiva_batch_create(oiva_batch **out, int device, int B, int T, int F, int M, int K, int model, void *stream);
int oiva_batch_destroy(oiva_batch *b);
int oiva_batch_set_x_host(oiva_batch *b, const void *X_host, int f64);
int oiva_batch_set_x_dev(oiva_batch *b, const void *X_dev);
int oiva_batch_covariance(oiva_batch *b);
int oiva_batch_set_w(oiva_batch *b, const void *W0_host, int f64);
int oiva_batch_set_w_eig(oiva_batch *b);
int oiva_batch_iterate(oiva_batch *b, int n);
int oiva_batch_demix(oiva_batch *b, void *Y_host, int f64, int proj_back);
int oiva_batch_get_w(oiva_batch *b, void *W_host, int f64);
int oiva_batch_status(oiva_batch *b, int *status);
int oiva_batch_time_stages(oiva_batch *b, int n, float *total_ms, float *per_stage_ms);

/*
 * Batched OGIVE: ive.py::ogive on B problems of one shape (M <= 8 channels) per set of launches, each problem with its own
 * stopping rule (kernels_ogive_batch.hip).  Runs on a batch created with K = 1, after oiva_batch_covariance and
 * oiva_batch_set_w (w = column 0: identity, W0, or the principal eigenvector from the host, read through oiva_batch_get_cx):
 *   oiva_batch_get_cx        : the input covariance Cx (B, F, M, M), complex64 or (f64) complex128                ive.py:96
 *   oiva_batch_ogive_begin   : Cx^-1, ||Cx||, a from w, step selection on every bin; every problem running,
 *                              0 epochs                                                        ive.py:100-102,136-139,173-180
 *   oiva_batch_ogive_iterate : up to n epochs of ive.py:190-246 starting at epoch index first_epoch (the switching criterion
 *                              runs when the index is a multiple of 10), replayed from one linear captured graph.  Problem p
 *                              stops at the first epoch whose max ||delta|| < tol; its state is then frozen and later epochs
 *                              skip it.  Synchronous; fills, per problem, epochs_run[B] (epochs of this call that changed its
 *                              state), converged[B] (rule met) and max_delta[B] (max ||delta|| of its last epoch).
 * Arithmetic: OIVA_PREC_PRECISE.  x_psi is formed from float64 frame sums of rinv x conj(y) (ive.py:221-227), so a problem
 * matches oiva_plan_ogive_* to rounding; its bits and its epoch count do not depend on B, on its place in the batch or on
 * which other problems have stopped.  The result is read with oiva_batch_demix / oiva_batch_get_w / oiva_batch_status.
 * oiva_status is int, the status code every entry point returns.
 */
typedef int oiva_status;
oiva_status oiva_batch_get_cx(oiva_batch *b, void *Cx_host, int f64);
oiva_status oiva_batch_ogive_begin(oiva_batch *b, int update_mode, int model);
oiva_status oiva_batch_ogive_iterate(oiva_batch *b, int first_epoch, int n, double step_size, double tol, int *epochs_run,
                                     int *converged, double *max_delta);

/*
 * Ragged batch: B problems of one F, M <= 8 and K but of frames[b] = T_b >= 1 frames each (rooms of different lengths).
 * oiva_batch_create_ragged checks its arguments before any device call (OIVA_ERR_ARG: null frames, B < 1, a T_b < 1, F < 1,
 * M outside 1..8, K outside 1..M, sizes that overflow) and returns an ordinary oiva_batch: every oiva_batch_* entry above
 * works on it, with these layouts:
 *   X (sum T_b, F, M) PACKED: problem b holds frames [off_b, off_b + T_b), off_b = T_0 + ... + T_{b-1}; host complex64 /
 *   complex128 (oiva_batch_set_x_host) or a borrowed packed complex64 device array (oiva_batch_set_x_dev).
 *   Y (sum T_b, F, K) packed the same way (oiva_batch_demix).
 *   W0, W (B, F, M, K), Cx (B, F, M, M), status[B]: as a dense batch's.
 * Problem b gets the bits of a dense batch of its own T_b frames (oiva_batch_create with B = 1, T = T_b): every order of summation
 * and every split is a function of (bin, frame, T_b).  The iteration is still four launches whatever B, replayed from one
 * linear captured graph.  oiva_batch_ogive_begin and oiva_batch_ogive_iterate return OIVA_ERR_ARG on a ragged batch.
 */
oiva_status oiva_batch_create_ragged(oiva_batch **out, int device, int B, const int *frames, int F, int M, int K, int model,
                                     void *stream);

/*
 * Complex128 data (opt-in): X is held as the caller's complex128 and every stage -- demix and powers, r, gamma
 * and the weights, the scale of W, both covariances, the per-bin algebra, Y and the projection back -- runs in float64
 * (kernels_batch_c128.hip; the per-bin update is the shared float64 one).  A batch of either create call.
 *   oiva_batch_set_data_c128    : puts a fresh batch into the mode; OIVA_ERR_STATE once X is set.  Afterwards
 *                                 oiva_batch_set_x_host takes complex128 only (f64 = 1, copied as it is: OIVA_ERR_ARG otherwise),
 *                                 oiva_batch_set_x_dev borrows a packed complex128 device array, oiva_batch_demix with f64 = 1
 *                                 returns what the device computed and with f64 = 0 its rounded copy; _covariance, _set_w,
 *                                 _set_w_eig, _iterate (five launches per iteration whatever B), _get_w, _status, _get_cx and
 *                                 _time_stages work unchanged.  OGIVE, ILRMA, the PCA entry points and oiva_batch_demix_dev return
 *                                 OIVA_ERR_ARG ("complex128").
 *   oiva_batch_c128_get_weights : test hook: the activation weights 1 / max(r / gamma, eps) of the last iteration, (sum T_b, K)
 *   oiva_batch_c128_get_cov     : test hook: the weighted covariances of the last iteration, every problem's frame splits added
 *                                 in order and divided by its T_b, (B*F, K, M, M) complex128; the partials have one layout on
 *                                 both data paths, so it also reads a complex64 batch (the FIVE tests: DESIGN.md 3.16)
 * A room's bits do not depend on B, on its place in the batch or on the other rooms' lengths.
 */
oiva_status oiva_batch_set_data_c128(oiva_batch *b);
oiva_status oiva_batch_c128_get_weights(oiva_batch *b, double *w);
oiva_status oiva_batch_c128_get_cov(oiva_batch *b, void *V);

/*
 * Batched PCA + determined AuxIVA (auxiva_pca.py:63-92 on B problems; overiva_amd/pca_batch.py, auxiva_pca_batch): the outer
 * batch (M channels, K < M sources) finds every bin's principal subspace and projects X onto it on the device, an inner batch
 * of the same B, F and frames with M = K runs the determined iteration on the projected X, and the composed filters demix the
 * original X.  Dense and ragged batches alike: the projection is driven from the problem table.
 *   oiva_batch_set_w_pca   : after oiva_batch_covariance: W = [the eigenvectors of the K largest eigenvalues of Cx, ascending |
 *                            [0; -I]] per bin (auxiva_pca.py:75-81, w[:, :, -K:]), as oiva_plan_set_w_pca for one problem;
 *                            evals_host (B, F, M) ascending, or NULL
 *   oiva_batch_project_dev : Xr[t,f,k] = sum_m conj(W[b,f,m,k]) X[t,f,m] for all problems in one launch (auxiva_pca.py:79-81),
 *                            (B, T, F, K) or packed (sum T_b, F, K) complex64 in a device array of the batch that is NOT the one
 *                            oiva_batch_demix_dev returns; every element is the float32 chain of oiva_batch_demix without
 *                            projection back.  Synchronous; *Xr_dev is valid until the next projection on the batch or its
 *                            destruction: hand it to the inner batch's oiva_batch_set_x_dev
 *   oiva_batch_compose_w   : columns 0..K-1 of the outer W <- P W_red in float64 per (problem, bin), P = those columns and W_red
 *                            the inner batch's K x K W; OIVA_ERR_ARG unless B and F agree and inner M == inner K == outer K.
 *                            Waits for the inner batch's stream.  A non-finite W_red propagates: oiva_batch_get_w / _status of the
 *                            outer batch name the problem.  oiva_batch_demix(outer, proj_back = 1) then gives auxiva_pca.py:89-90
 */
oiva_status oiva_batch_set_w_pca(oiva_batch *b, double *evals_host);
oiva_status oiva_batch_project_dev(oiva_batch *b, void **Xr_dev);
oiva_status oiva_batch_compose_w(oiva_batch *outer, const oiva_batch *inner);

/*
 * Batched ILRMA: independent low-rank matrix analysis on B rooms of one shape per set of launches (kernels_ilrma_batch.hip;
 * DESIGN.md 3.9 states the algorithm, which is the contract: parity with pra.bss.ilrma is not pinned).  Determined: the batch is
 * made by oiva_batch_create with K = M <= 8; a ragged batch gets OIVA_ERR_ARG ("ragged").  Source model r[s,f,t] = (Tn[s] Vn[s])[f,t]
 * with n_components columns; all state is float64, W is carried in complex128 as by oiva_batch_iterate.
 *   oiva_batch_ilrma_begin   : after oiva_batch_set_x_*, oiva_batch_covariance and oiva_batch_set_w; 1 <= n_components <= 16;
 *                              T0 (B, K, F, L) and V0 (B, K, L, T) host float64, strictly positive.  Allocates the state and
 *                              forms R = T0 V0 and P = |y|^2 from the W that is set.
 *   oiva_batch_ilrma_stage   : one stage of an epoch (OIVA_ILRMA_STAGE_*), eager on the batch's stream
 *   oiva_batch_ilrma_iterate : n epochs = n times the stages in order
 *   oiva_batch_ilrma_get_nmf : Tn (B, K, F, L), Vn (B, K, L, T); either may be NULL
 *   oiva_batch_ilrma_get_pr  : test hook: P, R (B, K, F, T); either may be NULL
 *   oiva_batch_ilrma_get_cov : test hook: C (B, F, K, M*M), the packed Hermitian frame-split partials of the last covariance
 *                              stage added in split order (sum_t x x^H / r, not divided by T; M real diagonals, then (re, im)
 *                              of every entry c < d, row-major), and lambda (B, K) of the last normalisation; either may be NULL
 *   oiva_batch_ilrma_time_stages : n epochs with events around every stage: per_stage_ms[7], ms per epoch by stage
 * A room's bits do not depend on B or on its place in the batch.  The result is read with oiva_batch_demix / _get_w / _status.
 */
enum {
    OIVA_ILRMA_STAGE_T = 0,         /* Tn of every source from P and R, then its rows of R */
    OIVA_ILRMA_STAGE_V = 1,         /* Vn of every source */
    OIVA_ILRMA_STAGE_R = 2,         /* R = Tn Vn */
    OIVA_ILRMA_STAGE_COV = 3,       /* C_s = (1/T) sum_t x x^H / r[s,f,t], as frame-split partials */
    OIVA_ILRMA_STAGE_UPDATE = 4,    /* IP1 per bin, the sources in sequence */
    OIVA_ILRMA_STAGE_POWER = 5,     /* P from the new W */
    OIVA_ILRMA_STAGE_NORMALISE = 6  /* lambda_s = sqrt(mean P[s]); W / lambda, P, R and Tn / lambda^2 */
};
oiva_status oiva_batch_ilrma_begin(oiva_batch *b, int n_components, const double *T0, const double *V0);
oiva_status oiva_batch_ilrma_stage(oiva_batch *b, int stage);
oiva_status oiva_batch_ilrma_iterate(oiva_batch *b, int n);
oiva_status oiva_batch_ilrma_get_nmf(oiva_batch *b, double *T, double *V);
oiva_status oiva_batch_ilrma_get_pr(oiva_batch *b, double *P, double *R);
oiva_status oiva_batch_ilrma_get_cov(oiva_batch *b, double *C, double *lambda);
oiva_status oiva_batch_ilrma_time_stages(oiva_batch *b, int n, float *per_stage_ms);

/*
 * Batched ISS: determined AuxIVA by iterative source steering (rank-1 updates of the demixed signals; Scheibler & Ono, ICASSP
 * 2020) on B rooms per set of launches (kernels_iss_batch.hip; DESIGN.md 3.15 states the algorithm, which is the contract).  The
 * batch is made by oiva_batch_create or oiva_batch_create_ragged with K = M <= 8, and every room must satisfy T_b * M <= 8192
 * (one bin's complex128 slab of 128 KiB of LDS): otherwise OIVA_ERR_ARG, as on a complex128 batch (oiva_batch_set_data_c128).
 * X stays complex64; every stage is float64 and W is carried in complex128 as by oiva_batch_iterate.  The source model and the
 * auxiliary weights are oiva_batch_iterate's (the batch's model); no covariance is formed and no linear system solved.
 *   oiva_batch_iss_begin       : after oiva_batch_set_x_* and oiva_batch_set_w / _set_w_eig.  Allocates the state and forms the
 *                                source powers of the W that is set (the sweep with no step)
 *   oiva_batch_iss_stage       : one stage of an iteration (OIVA_ISS_STAGE_*), eager on the batch's stream
 *   oiva_batch_iss_iterate     : n iterations = n times the stages in order (three launches per iteration whatever B)
 *   oiva_batch_iss_time_stages : n iterations with events around every stage: per_stage_ms[2], ms per iteration by stage
 *   oiva_batch_iss_sweep_steps : test hook: the sweep with its first n_steps rank-1 steps only, 0 <= n_steps <= M
 *   oiva_batch_iss_get_weights : test hook: the weights 1 / max(r / gamma, eps) of the last activation, (sum T_b, M) float64
 *   oiva_batch_iss_get_powers  : test hook: the source powers sum_f |y|^2 the last sweep left, (sum T_b, M) float64
 * All but _begin return OIVA_ERR_STATE before _begin.  A room's bits do not depend on B, on its place in the batch or on the
 * lengths of the other rooms.  The result is read with oiva_batch_demix / _demix_dev / _get_w / _status.
 */
enum {
    OIVA_ISS_STAGE_ACTIVATION = 0,  /* r, gamma and the weights from the group powers; the columns of W scaled (two launches) */
    OIVA_ISS_STAGE_SWEEP = 1        /* demix, the M rank-1 steps in LDS, the new W and the group powers (one launch) */
};
oiva_status oiva_batch_iss_begin(oiva_batch *b);
oiva_status oiva_batch_iss_stage(oiva_batch *b, int stage);
oiva_status oiva_batch_iss_iterate(oiva_batch *b, int n);
oiva_status oiva_batch_iss_time_stages(oiva_batch *b, int n, float *per_stage_ms);
oiva_status oiva_batch_iss_sweep_steps(oiva_batch *b, int n_steps);
oiva_status oiva_batch_iss_get_weights(oiva_batch *b, double *phi);
oiva_status oiva_batch_iss_get_powers(oiva_batch *b, double *p);

/*
 * Batched FIVE: single-source extraction by iterative SINR maximisation (Scheibler & Ono, "Fast independent vector extraction by
 * iterative SINR maximization", ICASSP 2020) on B rooms per set of launches (kernels_five_batch.hip; DESIGN.md 3.16 states the
 * algorithm, which is the contract).  The batch is made by oiva_batch_create or oiva_batch_create_ragged with K = 1 and M <= 8:
 * otherwise OIVA_ERR_ARG, as on a complex128 batch (oiva_batch_set_data_c128).  An iteration is the demix and power pass, the
 * activation and the weighted covariance with K = 1 (the batch's model) in float64 -- the stages of the complex128 data path, on
 * a complex128 copy of the batch's complex64 X that _begin makes --, then the new per-bin step: the
 * eigenpair (lambda, u) of V_f u = lambda Cx_f u with the smallest lambda in float64, w_f = u / sqrt(u^H V_f u).
 *   oiva_batch_five_begin         : after oiva_batch_set_x_*, oiva_batch_covariance and oiva_batch_set_w / _set_w_eig.  Forms,
 *                                   once per call, the complex128 copy of X and the reduction Li = L^-1 of Cx_f = L L^H of every bin (Li Cx_f Li^H = I); a
 *                                   Cx_f that is not positive definite gives a non-finite Li and the room ends non-finite
 *   oiva_batch_five_stage         : one stage of an iteration (OIVA_FIVE_STAGE_*), eager on the batch's stream
 *   oiva_batch_five_iterate       : n iterations = n times the stages in order (four launches per iteration whatever B)
 *   oiva_batch_five_time_stages   : n iterations with events around every stage: per_stage_ms[4], ms per iteration by stage
 *   oiva_batch_five_get_reduction : test hook: Li, (B, F, M, M) complex128
 * All but _begin return OIVA_ERR_STATE before _begin.  A room's bits do not depend on B, on its place in the batch or on the
 * lengths of the other rooms.  The result is read with oiva_batch_demix / _demix_dev / _get_w / _status; once _begin has run,
 * oiva_batch_demix with f64 = 1 forms Y in float64 from the complex128 copy of X (f64 = 0 and _demix_dev: the complex64 path).
 */
enum {
    OIVA_FIVE_STAGE_POWER = 0,       /* y = w^H x and the powers sum_f |y|^2 */
    OIVA_FIVE_STAGE_ACTIVATION = 1,  /* r from the powers */
    OIVA_FIVE_STAGE_COV = 2,         /* V_f = mean_t x x^H / max(r_t / mean r, eps), as frame-split partials */
    OIVA_FIVE_STAGE_UPDATE = 3       /* the smallest eigenpair of (V_f, Cx_f) per bin, the new w */
};
oiva_status oiva_batch_five_begin(oiva_batch *b);
oiva_status oiva_batch_five_stage(oiva_batch *b, int stage);
oiva_status oiva_batch_five_iterate(oiva_batch *b, int n);
oiva_status oiva_batch_five_time_stages(oiva_batch *b, int n, float *per_stage_ms);
oiva_status oiva_batch_five_get_reduction(oiva_batch *b, void *Li);

/*
 * Batched IP2: OverIVA / AuxIVA whose demixing vectors are updated two at a time by the exact minimiser of the surrogate over the
 * pair (Ono, "Fast stereo independent vector analysis and its implementation on mobile phone", IWAENC 2012; Scheibler & Ono's
 * OverIVA-IP2) on B rooms per set of launches (kernels_ip2_batch.hip; DESIGN.md 3.17 states the algorithm, which is the
 * contract).  The batch is made by oiva_batch_create or oiva_batch_create_ragged with 1 <= K <= M <= 8; a complex128 batch
 * (oiva_batch_set_data_c128) is refused with OIVA_ERR_ARG.  Needs X, the covariance and W (OIVA_ERR_STATE otherwise).  An
 * iteration is the demix and power pass, the activation (which scales W) and the weighted covariances of all K sources in
 * float64 -- the stages of the complex128 data path, on a complex128 copy of the batch's complex64 X made on first use --, then
 * the per-bin schedule of the iteration's index n, counted from the start of the separation:
 *     n even: (0,1), (2,3), ..., then (K-1) alone if K is odd;   n odd and K > 2: (0) alone, (1,2), ..., then (K-1) alone if K
 *     is even;   K = 2: (0,1) always;   K = 1: (0) alone.   A single step is IP1; J follows every step when K < M.
 *   oiva_batch_ip2_iterate     : iterations first_iteration .. first_iteration + n - 1 (five launches each whatever B); the index
 *                                is explicit, so the result does not depend on how a run is cut into calls
 *   oiva_batch_ip2_stage       : one stage (OIVA_IP2_STAGE_*) of iteration `iteration`, eager on the batch's stream
 *   oiva_batch_ip2_time_stages : iterations 0 .. n - 1 with events around every stage: per_stage_ms[4], ms per iteration by stage
 * A room's bits do not depend on B, on its place in the batch or on the lengths of the other rooms.  The result is read with
 * oiva_batch_demix / _demix_dev / _get_w / _status.
 */
enum {
    OIVA_IP2_STAGE_POWER = 0,       /* y = W^H x and the powers sum_f |y|^2 */
    OIVA_IP2_STAGE_ACTIVATION = 1,  /* r, gamma and the weights from the powers; the columns of W scaled */
    OIVA_IP2_STAGE_COV = 2,         /* V_s = mean_t x x^H / max(r_ts / gamma_s, eps) for every source, as frame-split partials */
    OIVA_IP2_STAGE_UPDATE = 3       /* the schedule of pair and single steps per bin */
};
oiva_status oiva_batch_ip2_iterate(oiva_batch *b, int first_iteration, int n);
oiva_status oiva_batch_ip2_stage(oiva_batch *b, int stage, int iteration);
oiva_status oiva_batch_ip2_time_stages(oiva_batch *b, int n, float *per_stage_ms);

/*
 * STFT analysis / synthesis on the GPU (hipFFT): time-domain audio in and out next to the solver.
 * Replaces, in the reference's drivers, pra.transform.analysis(mics_signals.T, framesize, framesize // 2, win=win_a)
 * (overiva_oneshot.py:293-295, overiva_sim.py:206-207) and pra.transform.synthesis(Y, framesize, framesize // 2,
 * win=win_s) (overiva_oneshot.py:371-379).  Those are third-party pyroomacoustics calls whose source is absent from
 * the reference: parity unpinned; the block-processing convention restated here: every frame holds `hop` new
 * samples behind `frame - hop` old ones, zeros before the first sample, n_frames = n_samples / hop.
 *   x (n_samples, n_chan) float32, C order  ->  X (n_frames, frame/2 + 1, n_chan) complex64
 *   Y (n_frames, frame/2 + 1, k) complex64  ->  y (n_frames * hop, k) float32      (k <= n_chan)
 * win_a / win_s: analysis / synthesis windows of `frame` floats, or NULL for a rectangular window.
 * oiva_stft_analysis copies X to X_host when that is not NULL and returns, through X_dev when that is not NULL, the
 * device array holding it (valid until the next analysis/synthesis on this handle): hand it to
 * oiva_plan_set_x_dev to run the solver without a host round trip.  All calls are synchronous.
 */
typedef struct oiva_stft oiva_stft;
int oiva_stft_create(oiva_stft **out, int device, int n_samples, int n_chan, int frame, int hop, const float *win_a,
                     const float *win_s);
int oiva_stft_destroy(oiva_stft *p);
int oiva_stft_shape(oiva_stft *p, int *n_frames, int *n_freq);
int oiva_stft_analysis(oiva_stft *p, const float *x_host, void *X_host, void **X_dev);
int oiva_stft_synthesis(oiva_stft *p, const void *Y_host, int n_chan, float *y_host);

/*
 * Audio in, audio out for a batch (overiva_amd/separate.py, separate_batch): the STFT of B rooms of different lengths in one
 * set of launches, X written on the device in the layout of the batched solvers, Y read from the batch's device array.
 *   packed audio x (sum n_b, M) float32, host: room b holds samples [s_b, s_b + n_b), s_b = n_0 + ... + n_{b-1}
 *   X (sum T_b, F, M) complex64, device, T_b = n_b / hop, F = frame / 2 + 1: the packed layout oiva_batch_set_x_dev borrows for a
 *     ragged batch of frames T_b, and a dense batch's (B, T, F, M) when all T_b agree
 *   packed y (sum T_b * hop, K) float32, host
 * Framing convention and arithmetic are oiva_stft's, room by room: zeros before EACH room's first sample, no frame and no
 * overlap-add across a room boundary.  win_a / win_s: `frame` floats or NULL (rectangular).  stream: NULL (the handle owns one) or
 * a hipStream_t to run on.  Every entry checks its arguments before any device call (OIVA_ERR_ARG: null pointers, B < 1, a room
 * shorter than one hop, odd frame, hop outside 1..frame, M outside 1..8, K outside 1..M, 2^31 elements or more in a room's
 * buffers, 2^63 bytes or more in all) and is synchronous.
 *   oiva_bstft_analysis      : upload, framing + window, one batched R2C, transpose; *X_dev is valid until the next analysis on
 *                              the handle or its destruction
 *   oiva_bstft_synthesis_dev : Y_dev (sum T_b, F, K) complex64 on the device -> packed y on the host
 *   oiva_bstft_phase_ms      : ms[8] of the last analysis (upload, framing, R2C, transpose) and the last synthesis (transpose, C2R,
 *                              overlap-add, download), from events on the handle's stream; 0 for a call not made yet
 *   oiva_batch_demix_dev     : oiva_batch_demix with Y left on the device, (B, T, F, K) or packed (sum T_b, F, K) complex64;
 *                              *Y_dev is valid until the next demix on the batch or its destruction
 *   oiva_device_to_host      : plain copy of `bytes` bytes of a device array of this process (tests read X and Y with it)
 */
typedef struct oiva_bstft oiva_bstft;
oiva_status oiva_bstft_create(oiva_bstft **out, int device, int B, const int *n_samples, int M, int frame, int hop,
                              const float *win_a, const float *win_s, void *stream);
oiva_status oiva_bstft_destroy(oiva_bstft *p);
oiva_status oiva_bstft_shape(oiva_bstft *p, int *frames, int *n_freq);
oiva_status oiva_bstft_analysis(oiva_bstft *p, const float *x_host_packed, void **X_dev);
oiva_status oiva_bstft_synthesis_dev(oiva_bstft *p, const void *Y_dev, int K, float *y_host_packed);
oiva_status oiva_bstft_phase_ms(oiva_bstft *p, float *ms);
oiva_status oiva_batch_demix_dev(oiva_batch *b, int proj_back, void **Y_dev);
oiva_status oiva_device_to_host(void *host, const void *dev, long long bytes);

/*
 * BSS Eval on the device (bsseval.hip, kernels_bsseval.hip): SDR, SIR and SAR of B rooms of N sources (1..8) with
 * a filter of filter_length taps (1..512), rooms of their own lengths, all arithmetic in float64.  One handle = one
 * (lengths, N, filter_length).  With diag_only only the pairs (estimate k, reference k) are evaluated.  max_group: 0, or the most
 * rooms whose two copies of the Gram matrix may be held at once (the handle halves the group by itself when the allocation
 * fails); a room's bits do not depend on B, on its place, on the other rooms' lengths or on the grouping.
 *   ref / est packed (sum_b N * n_b) float64: room b's (N, n_b) signals, row-major, room after room.
 *   oiva_bsseval_stage       : stage 0 correlate (lag sums), 1 factor (assembly + Cholesky of G and of its N diagonal blocks),
 *                              2 solve, 3 criteria; in order; stages 1..3 need all rooms in one group (OIVA_ERR_STATE otherwise)
 *   oiva_bsseval_run         : all four stages, group by group
 *   oiva_bsseval_get_gram    : G (B, N Lf, N Lf) (after factor; may be NULL), D (B, N, N Lf), E (B, N) (after correlate)
 *   oiva_bsseval_get_filters : C (B, N, N Lf) = G^-1 D_k and c (B, N[j], N[k], Lf) = G_jj^-1 D_k[j]
 *   oiva_bsseval_get_criteria: sdr, sir, sar (B, N, N) indexed [room][estimate][reference], NaN where not evaluated; copies them
 *                              out even when it returns OIVA_ERR_NUMERIC (a room's factorisation met a pivot that is not finite
 *                              or <= N Lf eps max_diag(G); the message names the rooms as "problem(s) ...")
 *   oiva_bsseval_status      : status[B], 1 for a flagged room
 *   oiva_bsseval_time_stages : n full runs with events around every stage: per_stage_ms[4], ms per run
 * Every entry checks its arguments before any device call and is synchronous.
 */
typedef struct oiva_bsseval oiva_bsseval;
oiva_status oiva_bsseval_create(oiva_bsseval **out, int device, int B, const int *n_samples, int N, int filter_length,
                                int diag_only, int max_group, void *stream);
oiva_status oiva_bsseval_destroy(oiva_bsseval *p);
oiva_status oiva_bsseval_groups(oiva_bsseval *p, int *rooms_per_group);
oiva_status oiva_bsseval_set_signals(oiva_bsseval *p, const double *ref_host_packed, const double *est_host_packed);
oiva_status oiva_bsseval_stage(oiva_bsseval *p, int stage);
oiva_status oiva_bsseval_run(oiva_bsseval *p);
oiva_status oiva_bsseval_get_gram(oiva_bsseval *p, double *G_host, double *D_host, double *E_host);
oiva_status oiva_bsseval_get_filters(oiva_bsseval *p, double *C_host, double *c_host);
oiva_status oiva_bsseval_get_criteria(oiva_bsseval *p, double *sdr, double *sir, double *sar);
oiva_status oiva_bsseval_status(oiva_bsseval *p, int *status);
oiva_status oiva_bsseval_time_stages(oiva_bsseval *p, int n, float *per_stage_ms);

/*
 * BSS Eval of many estimate sets against one set of references (bsseval.hip, kernels_bsseval.hip): the half of
 * oiva_bsseval that depends on the references alone -- their lag sums, the Gram matrix G, its Cholesky factor and the factors of
 * its N diagonal blocks -- is made once (prepare) and up to max_sets estimate sets are evaluated against it, any number of them
 * per set of launches (evaluate).  One handle = one (lengths, N, filter_length, max_sets), limits as oiva_bsseval_create and
 * max_sets >= 1; all B rooms are resident at once (no internal grouping: when the buffers do not fit, creation fails with the
 * allocation message and leaves nothing behind).  For every room and set the results have the bits oiva_bsseval gives on the same
 * signals; they do not depend on max_sets, on the sets evaluated together, on the set's place among them, on B or on the room's
 * place.
 *   ref / est packed as for oiva_bsseval_set_signals; set e is one such est.
 *   oiva_bsssets_set_references: the references, host -> device; drops the preparation and every set's results
 *   oiva_bsssets_set_estimates : the estimates of set e (0 .. max_sets - 1), host -> device
 *   oiva_bsssets_take          : device to device from an oiva_bsseval handle that is as oiva_bsseval_set_signals leaves it (the
 *                                caller sees to that): its estimates into set e, with_references its references too.  The handles
 *                                must agree in device, B, lengths, N and filter_length (OIVA_ERR_ARG names what differs)
 *   oiva_bsssets_prepare       : the reference half; the same pivot rule as oiva_bsseval, so the same rooms are flagged
 *   oiva_bsssets_evaluate      : sets e0 .. e0 + n_sets - 1: lag sums with the estimates, right-hand sides, substitutions, quadratic
 *                                forms, ratios.  OIVA_ERR_STATE before prepare (or after new references) and for a set whose
 *                                estimates were never given.  Flagged rooms are skipped, the others run on
 *   oiva_bsssets_get_criteria  : sdr, sir, sar (B, n_sets, N, N) indexed [room][set][estimate][reference], NaN where not evaluated;
 *                                copies them out even when it returns OIVA_ERR_NUMERIC (the message names the flagged rooms as
 *                                "problem(s) ...")
 *   oiva_bsssets_status        : status[B], 1 for a flagged room (after prepare)
 *   oiva_bsssets_get_gram      : test hook: G (B, N Lf, N Lf) (may be NULL), D (B, N, N Lf) and E (B, N) of the evaluated set e
 *   oiva_bsssets_get_filters   : test hook: C (B, N, N Lf) and c (B, N[j], N[k], Lf) of the evaluated set e
 *   oiva_bsssets_counts        : preparations and sets evaluated since creation
 *   oiva_bsssets_phase_ms      : ms[4]: device ms of the last prepare, and of the lag sums, the substitutions (with the right-hand
 *                                sides) and the criteria of the last evaluate (OIVA_ERR_STATE until both have run)
 * Every entry checks its arguments before any device call and is synchronous.
 */
typedef struct oiva_bsssets oiva_bsssets;
oiva_status oiva_bsssets_create(oiva_bsssets **out, int device, int B, const int *n_samples, int N, int filter_length,
                                int diag_only, int max_sets, void *stream);
oiva_status oiva_bsssets_destroy(oiva_bsssets *p);
oiva_status oiva_bsssets_set_references(oiva_bsssets *p, const double *ref_host_packed);
oiva_status oiva_bsssets_set_estimates(oiva_bsssets *p, int e, const double *est_host_packed);
oiva_status oiva_bsssets_take(oiva_bsssets *p, oiva_bsseval *from, int e, int with_references);
oiva_status oiva_bsssets_prepare(oiva_bsssets *p);
oiva_status oiva_bsssets_evaluate(oiva_bsssets *p, int e0, int n_sets);
oiva_status oiva_bsssets_get_criteria(oiva_bsssets *p, int e0, int n_sets, double *sdr, double *sir, double *sar);
oiva_status oiva_bsssets_status(oiva_bsssets *p, int *status);
oiva_status oiva_bsssets_get_gram(oiva_bsssets *p, int e, double *G_host, double *D_host, double *E_host);
oiva_status oiva_bsssets_get_filters(oiva_bsssets *p, int e, double *C_host, double *c_host);
oiva_status oiva_bsssets_counts(oiva_bsssets *p, long long *preparations, long long *sets_evaluated);
oiva_status oiva_bsssets_phase_ms(oiva_bsssets *p, float *ms);

/*
 * Shoebox rooms by the image-source method on the device (room.hip, kernels_room.hip): impulse responses, premix
 * (every source convolved with its response at every microphone) and mix-down of B rooms of S sources (1..16) and M microphones
 * (1..32), all arithmetic in float64.  One handle = one set of geometries; fs, c and max_order (0..32) are the batch's.
 *   room_dim (B, 3), sources (B, S, 3), mics (B, M, 3), absorption6 (B, 6): energy absorption in [0, 1) of the walls x=0, x=Lx,
 *   y=0, y=Ly, z=0, z=Lz.  rir_length: 0 = room b gets k_max,b + 81 samples, else that many for every room (<= 65536).
 *   oiva_room_compute_rir : k_max of every room, then every impulse response (once per handle)
 *   oiva_room_rir_lengths : lengths[B] (may be NULL) and the number of images (may be NULL)
 *   oiva_room_get_rir     : packed (sum_b S M Lr_b): room b's (S, M, Lr_b), row-major, room after room
 *   oiva_room_set_signals : n_samples[B] and the packed signals (sum_b S n_b): room b's (S, n_b); max_group: 0, or the most rooms
 *                           whose premix may be held at once (the handle halves the group by itself when the allocation fails)
 *   oiva_room_groups      : rooms per group; a group is named by its first room g0 = 0, group, 2 group, ...
 *   oiva_room_convolve    : the premix of group g0: room b's (S, M, n_b + Lr_b - 1), the full linear convolution.  One premix
 *                           buffer: convolving a group gives up the premix and the mix of the group before
 *   oiva_room_get_premix  : packed premix of group g0, room after room
 *   oiva_room_mix         : group g0 (convolved): every source divided by its population standard deviation at ref_mic, targets
 *                           s < K scaled by sqrt(sources_var[s]) (NULL: ones), the others by sigma_i, background = their sum +
 *                           sigma_n * noise (packed (n_out_b, M) of the group's rooms, NULL: none); K == S needs sinr = +inf
 *   oiva_room_get_mix     : packed mix (n_out_b, M) and ref (K + 1, n_out_b, M) of group g0, room after room
 *   oiva_room_time_stages : n full runs (unit sources_var, no noise) with events around every stage: per_stage_ms[4] = k_max,
 *                           impulse responses, convolution, mix-down; ms per run
 * A room's bits do not depend on B, on its place in the batch, on the other rooms or on the grouping.  Every entry checks its
 * arguments before any device call and is synchronous.
 */
typedef struct oiva_room oiva_room;
oiva_status oiva_room_create(oiva_room **out, int device, int B, int S, int M, double fs, double c, int max_order,
                             const double *room_dim, const double *sources, const double *mics, const double *absorption6,
                             int rir_length, void *stream);
oiva_status oiva_room_destroy(oiva_room *p);
oiva_status oiva_room_compute_rir(oiva_room *p);
oiva_status oiva_room_rir_lengths(oiva_room *p, int *lengths, int *images);
oiva_status oiva_room_get_rir(oiva_room *p, double *rir_host_packed);
oiva_status oiva_room_set_signals(oiva_room *p, const int *n_samples, const double *signals_host_packed, int max_group);
oiva_status oiva_room_groups(oiva_room *p, int *rooms_per_group);
oiva_status oiva_room_convolve(oiva_room *p, int g0);
oiva_status oiva_room_get_premix(oiva_room *p, int g0, double *premix_host_packed);
oiva_status oiva_room_mix(oiva_room *p, int g0, int K, double sinr, double snr, int ref_mic, const double *sources_var,
                          const double *noise_host_packed);
oiva_status oiva_room_get_mix(oiva_room *p, int g0, double *mix_host_packed, double *ref_host_packed);
oiva_status oiva_room_time_stages(oiva_room *p, int n, int K, double sinr, double snr, int ref_mic, float *per_stage_ms);

/*
 * One step of the Monte-Carlo sweep with every hand-over on the device (sweep.hip, kernels_sweep.hip; DESIGN.md 3.12;
 * overiva_amd/sweep.py, sweep_batch): the mix of an oiva_room group goes into the batched STFT without leaving the device, and
 * the synthesis of a solver's Y goes into an oiva_bsseval handle's ref and est without leaving it.
 *   oiva_bstft_analysis_dev   : oiva_bstft_analysis with the packed (sum n_b, M) audio already on the device: float32 (f64 = 0, a
 *                               device-to-device copy) or float64 (f64 = 1, cast to float32 round-to-nearest-even, what
 *                               ndarray.astype(float32) does); the "upload" phase of oiva_bstft_phase_ms times that step
 *   oiva_bstft_synthesis_keep : oiva_bstft_synthesis_dev without the download: *y_dev is the handle's packed (sum T_b hop, K)
 *                               float32 audio, valid until the next call on the handle; the "download" phase reads 0
 * One oiva_sweep handle = the rooms of one group of an oiva_room: B, their output lengths n_out[b], M microphones (1..8), K
 * targets (1..min(M, 7)), (frame, hop) of the STFT, ref_mic and the filter_length of the evaluation.  Of room b the samples
 * [0, m_b), m_b = T_b hop - (frame - hop), T_b = n_out[b] / hop, are evaluated; m_b < 1 is refused (OIVA_ERR_ARG naming the room).
 *   oiva_sweep_set_filler : packed (sum m_b) float64: row K of every room's estimates, what is held against the background
 *   oiva_sweep_take_mix   : group g0 of `room` must be mixed (OIVA_ERR_STATE otherwise) with K targets and be this handle's rooms;
 *                           runs oiva_bstft_analysis_dev on its float64 mix where it lies and remembers where its ref lies;
 *                           *X_dev as oiva_bstft_analysis.  No audio crosses to the host
 *   oiva_sweep_evaluate   : Y_dev (sum T_b, F, C) complex64, K <= C <= M: oiva_bstft_synthesis_keep; the population standard
 *                           deviation of every channel over all T_b hop samples (float64, two passes); order = the channels by
 *                           descending standard deviation, ties to the lower index (reorder = 0: the identity); then, into the
 *                           device buffers of `bsseval` (created with N = K + 1, lengths m_b and this filter_length):
 *                             est[b, k, i] = y[b, i, order[b, k]] (k < K), est[b, K, i] = filler[b, i],
 *                             ref[b, j, i] = room_ref[b, j, i, ref_mic] (j <= K)
 *                           exact gathers; the handle is left as after oiva_bsseval_set_signals, the caller runs
 *                           oiva_bsseval_run.  filler_dev: NULL (the handle's own) or packed (sum m_b) float64 on the device
 *   oiva_sweep_phase_ms   : device ms of the kernels of the last evaluate behind its synthesis
 *   oiva_sweep_get_order  : test hook: order and std of the last evaluate, (B, C) each
 *   oiva_sweep_get_signals: test hook: the packed ref and est the last evaluate left in `bsseval`
 * Every entry checks its arguments before any device call and is synchronous.  The room handle must stay alive and its group
 * mixed between take_mix and the last evaluate.
 */
typedef struct oiva_sweep oiva_sweep;
oiva_status oiva_bstft_analysis_dev(oiva_bstft *p, const void *x_dev, int f64, void **X_dev);
oiva_status oiva_bstft_synthesis_keep(oiva_bstft *p, const void *Y_dev, int K, void **y_dev);
oiva_status oiva_sweep_create(oiva_sweep **out, int device, int B, const int *n_out, int M, int K, int frame, int hop, int ref_mic,
                              int filter_length, void *stream);
oiva_status oiva_sweep_destroy(oiva_sweep *p);
oiva_status oiva_sweep_set_filler(oiva_sweep *p, const double *filler_host_packed);
oiva_status oiva_sweep_take_mix(oiva_sweep *p, oiva_room *room, int g0, oiva_bstft *bstft, void **X_dev);
oiva_status oiva_sweep_evaluate(oiva_sweep *p, oiva_bstft *bstft, const void *Y_dev, int C, int reorder, oiva_bsseval *bsseval,
                                const double *filler_dev);
oiva_status oiva_sweep_phase_ms(oiva_sweep *p, float *ms);
oiva_status oiva_sweep_get_order(oiva_sweep *p, int *order, double *std);
oiva_status oiva_sweep_get_signals(oiva_sweep *p, oiva_bsseval *bsseval, double *ref_host_packed, double *est_host_packed);

/*
 * Seeded standard normals on the device (rng.hip, kernels_rng.hip; overiva_amd/rng.py): the sensor noise of the
 * room simulation and the filler row of the sweep, drawn where they are used.  The generator is Philox-4x64-10: block j of a
 * stream is the ten rounds on the counter (j, purpose, 0, 0) under the stream's key (key0, key1) -- what
 * numpy.random.Philox(key=[key0, key1], counter=(j, purpose, 0, 0) - 1).random_raw(4) returns -- and every word w of it becomes
 * u = ((w >> 12) + 0.5) 2^-52; words 0, 1 give z0 = r cos(2 pi u1), z1 = r sin(2 pi u1) with r = sqrt(-2 ln u0), words 2, 3 give
 * z2, z3 likewise.  Element n of a stream is z[n mod 4] of block n / 4, so a stream is a prefix of every longer one with its key
 * and purpose.  purpose: 0 for sensor noise, 1 for the filler row, other values are the caller's.  A value depends on (key,
 * purpose, n) alone, not on the other streams of a handle or on the stream's place among them.
 * One oiva_rng handle = n_streams streams of counts[i] elements (1..2^40 in all), packed stream after stream in float64.
 *   oiva_rng_fill     : draws every stream, stream i under (key0[i], key1[i]); n_streams keys each
 *   oiva_rng_fill_ms  : device ms of the kernel of the last fill
 *   oiva_rng_get      : the packed values on the host (OIVA_ERR_STATE before the first fill)
 *   oiva_rng_ptr      : where they lie on the device: valid until the next fill or the handle's end; with counts m_b it is a
 *                       filler_dev of oiva_sweep_evaluate
 *   oiva_rng_raw      : test hook: words (n_blocks, 4) of blocks first_block .. first_block + n_blocks - 1 (n_blocks <= 2^20)
 *   oiva_rng_room_mix : oiva_room_mix with the noise of group g0 drawn into the room handle's own noise buffer instead of copied
 *                       from the host: room g0 + i is the row-major (n_out, M) array of its stream under (key0[i], key1[i]),
 *                       purpose 0; as many keys as the group has rooms.  Arguments, errors and the mix-down are oiva_room_mix's
 * Every entry checks its arguments before any device call and is synchronous.
 */
typedef struct oiva_rng oiva_rng;
oiva_status oiva_rng_create(oiva_rng **out, int device, int n_streams, const long long *counts, void *stream);
oiva_status oiva_rng_destroy(oiva_rng *p);
oiva_status oiva_rng_fill(oiva_rng *p, const unsigned long long *key0, const unsigned long long *key1, unsigned long long purpose);
oiva_status oiva_rng_fill_ms(oiva_rng *p, float *ms);
oiva_status oiva_rng_get(oiva_rng *p, double *host_packed);
oiva_status oiva_rng_ptr(oiva_rng *p, void **dev_packed);
oiva_status oiva_rng_raw(int device, unsigned long long key0, unsigned long long key1, unsigned long long purpose,
                         unsigned long long first_block, int n_blocks, unsigned long long *words_host);
oiva_status oiva_rng_room_mix(oiva_room *room, int g0, int K, double sinr, double snr, int ref_mic, const double *sources_var,
                              const unsigned long long *key0, const unsigned long long *key1);

/*
 * Decay curve and reverberation time of many impulse responses on the device (decay.hip, kernels_decay.hip; DESIGN.md 3.14;
 * overiva_amd/acoustics.py), all arithmetic in float64.  For a response h[0..L-1]: the Schroeder integral
 * E[n] = sum_{k >= n} h[k]^2, summed in an order that is a function of (n, L) alone; theta_a = E[0] 10^(-start_db / 10) and
 * theta_b = E[0] 10^(-(start_db + decay_db) / 10), both factors formed once on the host; i_a, i_b = the smallest n with
 * E[n] <= theta_a, theta_b (-1: none, and both -1 for an all-zero response); sum_d, sum_nd = the sums of D[n] = 10 log10(E[n] / E[0])
 * and of n D[n] over theta_b < E[n] <= theta_a.  The estimates follow on the host: (60 / decay_db) (i_b - i_a) / fs, and
 * -60 / (m fs) with m the least-squares slope of D over [i_a, i_b).
 * One oiva_decay handle = n_resp responses (1..2^22) of lengths[i] samples (1..2^24), packed one after the other.
 *   oiva_decay_set_host  : the packed samples (sum lengths) from the host
 *   oiva_decay_set_dev   : ... where they lie on the device: borrowed, must stay valid until the run
 *   oiva_decay_set_room  : ... the room handle's own impulse responses, S M responses of Lr_b samples per room as
 *                          oiva_room_get_rir lays them out; no copy.  OIVA_ERR_STATE before oiva_room_compute_rir (or after new
 *                          absorptions), OIVA_ERR_ARG when device or table of lengths are not this handle's
 *   oiva_decay_run       : fs > 0, start_db >= 0, decay_db > 0 (finite); keep_curve != 0 also writes every E[n]
 *   oiva_decay_get       : e0, i_a, i_b, sum_d, sum_nd (n_resp each; each may be NULL) of the last run
 *   oiva_decay_get_curve : the packed curves (sum lengths); OIVA_ERR_STATE unless the last run kept them
 *   oiva_decay_ms        : device ms of the kernel of the last run
 *   oiva_decay_room_set_absorption : new wall absorptions (B, 6) for a room handle: its impulse responses become stale, so
 *                          oiva_room_compute_rir may run again on the same handle (k_max, the lengths and the device buffers are
 *                          kept: they do not depend on the absorption); any convolved or mixed group is dropped, and
 *                          oiva_room_convolve returns OIVA_ERR_STATE until the responses are computed.  Without this call a room
 *                          handle computes its responses once, as before
 * A response's results do not depend on the other responses, on its place in the handle or on the launch.  Every entry checks its
 * arguments before any device call and is synchronous.
 */
typedef struct oiva_decay oiva_decay;
oiva_status oiva_decay_create(oiva_decay **out, int device, int n_resp, const int *lengths, void *stream);
oiva_status oiva_decay_destroy(oiva_decay *p);
oiva_status oiva_decay_set_host(oiva_decay *p, const double *host_packed);
oiva_status oiva_decay_set_dev(oiva_decay *p, const void *dev_packed);
oiva_status oiva_decay_set_room(oiva_decay *p, oiva_room *room);
oiva_status oiva_decay_run(oiva_decay *p, double fs, double start_db, double decay_db, int keep_curve);
oiva_status oiva_decay_get(oiva_decay *p, double *e0, int *i_a, int *i_b, double *sum_d, double *sum_nd);
oiva_status oiva_decay_get_curve(oiva_decay *p, double *curve_host_packed);
oiva_status oiva_decay_ms(oiva_decay *p, float *ms);
oiva_status oiva_decay_room_set_absorption(oiva_room *room, const double *absorption6);

#ifdef __cplusplus
}
#endif
#endif /* OVERIVA_HIP_H */
