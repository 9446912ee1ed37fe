// Which kernel runs the covariance pass and the power pass of a plan, and on what geometry: the one table of what each kernel
// family supports and needs (kCovTraits, kPowTraits) and the two functions that choose from it (choose_cov, choose_pow).
// Everything else -- the launchers' switches, the partial type, the unit-weights pass, the switches of the C ABI -- reads the
// table.  Host only, header only, standard C++: no HIP type and no device query in here (the two occupancy figures the choice
// needs come in as callables), so a plain program can replay any choice (tests/helpers/kernel_choice_main.cpp).
// Behind them, the same for the third stage: which per-bin update kernel launch_update runs (kUpdTraits, choose_update; replayed by
// tests/helpers/update_choice_main.cpp), and the shape rule of the fused covariance + update launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <functional>
#include <string>

#include "overiva_hip.h"

namespace oiva {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// channel counts of the kernels tuned per shape (1..kNarrowMax: register arrays sized by it) and of the generic wide path
// (kNarrowMax + 1 .. kWideMax = OIVA_MAX_CHANNELS, kernels_wide.hip), chosen by the channel count alone
constexpr int kNarrowMax = 16;
constexpr int kWideMax = OIVA_MAX_CHANNELS;

// ---- lane geometry shared by the streaming kernels -------------------------------------------
// A wave is 16 bins x 4 frame phases: lane l -> bin (l & 15), phase (l >> 4).  The 16 bins of one
// frame are 16*M*8 contiguous bytes of the native (T, F, M) complex64 tensor, so one wave touches
// four contiguous runs per step and every byte of every cache line it opens is consumed.
constexpr int kBinsPerWave = 16;
constexpr int kPhasesPerWave = 4;
constexpr int kBlock = 256;  // 4 waves
constexpr int kWaves = kBlock / 64;

// The covariance kernel families.  Lane: one lane per (bin, frame), cov_kernel / cov_dma_kernel (which of the two is
// dispatch_kc's business, kernels_cov.hip); Pair32 / Pair64: 8 channels, two lanes per (bin, frame); Quad: four lanes, few
// sources; Half16 / Half16F64: 32 lanes, many sources, float32 / float64 sums; Hmfma / Hmfma64: the same with the sources on the
// fp32 matrix cores; Mfma: the planar matrix-core kernel; Wide: 17..32 channels.
enum class CovKind { Lane, Pair32, Pair64, Quad, Half16, Hmfma, Half16F64, Hmfma64, Mfma, Wide };
// The power kernels.  Lane: power_kernel (kernels_demix.hip); Mfma: power_mfma_kernel, any bin count, ragged ones included; Lds:
// power_lds_kernel, X staged through the LDS (both kernels_power_mfma.hip); Wide: 17..32 channels.
enum class PowKind { Lane, Mfma, Lds, Wide };
constexpr int kCovKinds = 10, kPowKinds = 4;
static_assert((int)CovKind::Wide + 1 == kCovKinds && (int)PowKind::Wide + 1 == kPowKinds, "one traits row per kind");

struct CovGeom {
    int nsplit;   // frame splits (grid.y)
    int tc;       // frames per split (multiple of the kind's quantum)
    int kc;       // sources per pass (template KC)
    int nbg;      // bin groups (grid.x of the kernels that take it from here)
    CovKind kind = CovKind::Lane;
    int pad = 0;  // odd channel count of 9..15: the kinds that read the padded X read the copy of X padded to M + 1 channels
    int part32 = 0; // Hmfma: the partial blocks leave as float32 (each the float64 sum of its chains, rounded once)
    int xplain = 16; // cov_dma_kernel: the frame groups g of a split with g % 16 < xplain are loaded plain, the others nt (XPolicy)
    int rows = 0;    // cov_dma_kernel: its row instantiation (cov_rows_form below), filled in at launch time like xplain
};
// Which frame chunk the y-th dispatched row of power_kernel's grid takes when the pass runs against the covariance pass
// (DESIGN §3).  The covariance pass walks `cs` splits of `ctc` frames ascending and side by side, so the X it read last -- what
// the Infinity Cache still holds -- is the TAIL of every split.  The n chunks of tcp frames are therefore handed out tail
// first: chunk c belongs to the split that holds its last frame (split s owns chunks [first[s], first[s + 1]), first[s] = the
// chunk that holds frame s * ctc), row 0 of the order is the last chunk of every split, row 1 the one before it, and so on
// down to the heads, which the next covariance pass reads first.  A bijection of [0, n) for any n, tcp, cs, ctc >= 1 (a split
// may own no chunk at all).  The table is made on the host and travels by value in the kernel's arguments (the divisions of the
// closed form cost every workgroup 1-2 us in front of its first load: measured); uniform scalar work in the kernel
// (power_chunk_tail_first, oiva_internal.h).
constexpr int kPowOrderMaxSplits = 64;
struct PowOrder {
    int cs = 0;                              // covariance splits (0: no order, chunk = row)
    int q = 0;                               // chunks EVERY split owns: the rows of the order that hold all cs splits
    int first[kPowOrderMaxSplits + 1] = {};  // first chunk of split s; first[cs] = n
};
inline PowOrder make_pow_order(int n, int tcp, int cs, int ctc) {
    PowOrder o;
    if (cs < 1 || cs > kPowOrderMaxSplits || ctc < 1 || tcp < 1 || n < 1) return o;      // (more splits than the table holds: chunk = row)
    o.cs = cs;
    for (int s = 0; s < cs; ++s) {
        const long long c = (long long)s * ctc / tcp;
        o.first[s] = c < n ? (int)c : n;
    }
    o.first[cs] = n;
    o.q = n;
    for (int s = 0; s < cs; ++s) o.q = o.first[s + 1] - o.first[s] < o.q ? o.first[s + 1] - o.first[s] : o.q;
    return o;
}
struct PowGeom {
    int nb;       // bin batches of 64 (grid.x)
    int nsplit;   // frame splits (grid.y)
    int tcp;      // frames per split (multiple of 4, <= kPowMaxFrames)
    int kp;       // sources per pass
    PowKind kind = PowKind::Lane;
    // the frame order of power_kernel: rev = every chunk from its last step to its first, ord = which chunk a row of the grid
    // takes (both: against the covariance pass, kernels_demix.hip).  Filled in at launch time (stage_power).
    int rev = 0;
    PowOrder ord{};
    int rounds = 1;   // rounds of resident workgroups the grid of power_kernel takes (choose_pow)
    // the load policy of X (XPolicy below), filled in at launch time like the order: frames in groups of 16 counted from the
    // start of their covariance split of xctc frames, groups g with g % 16 < xplain loaded plain, the others nt
    int xplain = 16;
    int xctc = 0;
};
constexpr int kPowMaxFrames = 512;

// ---- one load policy per byte of X, the same in both streaming passes and in every iteration ---------------------
// The frames of every covariance split are counted off in groups of kXGroup from the split's first frame; of every kXPeriod
// consecutive groups the first n16 are RESIDENT: both passes read them with plain loads, so they may stay in the Infinity Cache
// from pass to pass, and read the other groups with non-temporal loads (8 channels: cov_dma_kernel<8, KC>, power_kernel<8, KP>).
// A covariance step (16 frames) is one group; a power load step (4 frames) lies inside one group because splits and chunks
// start on multiples of 4 frames.
constexpr int kXGroup = 16, kXPeriod = 16;
constexpr bool x_group_plain(int frame_in_split, int xplain) { return ((frame_in_split / kXGroup) % kXPeriod) < xplain; }
// frame-in-split of the frame `tl` frames behind one at `off0` in its split, for walks that cross at most one split boundary
constexpr int x_split_offset(int off0, int tl, int ctc) { return off0 + tl >= ctc ? off0 + tl - ctc : off0 + tl; }
enum class XReason { Off, Fits, Kernels, Geometry, Share };
constexpr double kXResidentDefaultMB = 268.;      // MB of X that may stay resident: the 256 MiB of the Infinity Cache
struct XPolicy {
    int n16 = 0;                     // resident groups of every 16
    bool nt = false;                 // the other groups stream non-temporally (false: every load of X is plain, as before)
    XReason why = XReason::Off;
    int xplain() const { return nt ? n16 : kXPeriod; }      // what the kernels take
};
// budget_mb: what may stay resident ($OIVA_X_RESIDENT_MB, oiva_plan_set_x_resident_mb; <= 0: the policy is off).  The share is
// n16 sixteenths of X, as many as the budget holds.  Counted frame by frame the resident bytes can EXCEED the budget: a split that
// ends inside a period has up to n16 (16 - n16) <= 64 resident frames more than its sixteenths (headline, 200 MB: 201.3 MB).  All plain, as before: X fits the budget whole (Fits); a pass is not cov_dma_kernel /
// power_kernel (Kernels); the geometry does not keep every step inside one group (Geometry).
inline XPolicy choose_x_policy(double budget_mb, int T, int F, int M, bool cov_f64, const CovGeom& cg, const PowGeom& pg) {
    XPolicy x;
    if (!(budget_mb > 0.)) return x;
    const double frame_bytes = (double)F * M * 8., budget = budget_mb * 1e6;
    x.why = XReason::Fits, x.n16 = kXPeriod;
    if (frame_bytes * T <= budget) return x;
    x.why = XReason::Kernels, x.n16 = 0;
    if (cg.kind != CovKind::Lane || pg.kind != PowKind::Lane || cov_f64 || M != 8) return x;
    x.why = XReason::Geometry;
    if (cg.tc % kXGroup != 0 || pg.tcp % 4 != 0 || pg.tcp > cg.tc) return x;
    x.why = XReason::Share, x.nt = true;
    x.n16 = std::min(kXPeriod - 1, (int)(budget * kXPeriod / (frame_bytes * T)));
    return x;
}

// Which instantiation of cov_dma_kernel<8, KC> a launch takes: the row form (every step requested row by row, plain or nt, through
// a ring of kCovRowStages stages: kernels_cov.hip) exactly where the policy streams, the lane-addressed form everywhere else --
// X that fits the budget, the policy off, other kernels, other geometries -- and wherever the switch is off ($OIVA_COV_ROWS=0,
// oiva_plan_set_cov_rows: for A/B and for the tests).  Same bits either way.
constexpr bool cov_rows_form(const XPolicy& x, bool rows_on) { return rows_on && x.nt; }

// ---- the traits ----------------------------------------------------------------------------------------------------------------
enum class Partials { F64, Acc, F32IfPart32 };      // float64 always | the accumulator's type | float32 when CovGeom::part32
struct CovTraits {
    bool (*supported)(int M, int K);   // on the channel count the kernel sees (the padded one where padded_x)
    int (*sources)(int K);             // sources per pass over X (nullptr: lane_sources_per_pass, by the register budget)
    int bins;                          // bins per group of CovGeom::nbg: the kernel's workgroup (the matrix-core kinds run one bin
                                       // per workgroup and do not read nbg; it keeps their vector-ALU sibling's groups)
    int quantum;                       // frames per step of a workgroup: tc is a multiple of it
    Partials partials;
    int launches;                      // per pass: 1, or 2 with a weights pre-pass in front of the kernel
    bool padded_x;                     // reads the padded copy of X at 9 / 11 / 13 / 15 channels
    bool quad_switch;                  // oiva_plan_set_cov_quad governs it (a vector-ALU kernel of 9..16 channels)
    bool fusable;                      // the fused covariance + update launch may replace it (kernels_cov_update.hip)
    bool update_arith;                 // which kernel or how many splits also depends on OIVA_PREC_UPDATE_F64: a change of that bit
                                       // chooses again (Wide: nothing does; it chooses again all the same, as it always has)
    CovKind unit;                      // the kind that runs the unit-weights pass (K = 1, R == nullptr) on the same splits
};
// shape -> kernel -> lanes -> sources per pass: DESIGN §3.  The numbers behind the predicates are in the kernel files.
constexpr CovTraits kCovTraits[kCovKinds] = {
    /* Lane      */ {[](int M, int K) { return M >= 1 && M <= 8 && K >= 1 && K <= M; }, nullptr, kBinsPerWave, 16, Partials::F64, 1, false, false, true, false, CovKind::Lane},
    // float32 kernel for 8 channels and three or more sources, FOUR per pass over X (kernels_cov_pair32.hip)
    /* Pair32    */ {[](int M, int K) { return M == 8 && K >= 3; }, [](int) { return 4; }, 32, 8, Partials::F64, 2, false, false, false, true, CovKind::Pair32},
    // float64 vector-ALU kernel for 8 channels (kernels_cov_pair64.hip)
    /* Pair64    */ {[](int M, int) { return M == 8; }, [](int K) { return K >= 2 ? 2 : 1; }, 32, 8, Partials::F64, 2, false, false, false, false, CovKind::Pair64},
    // vector-ALU kernel for 10, 12, 14, 16 channels and K <= 4 sources, float32 arithmetic (kernels_cov_quad.hip)
    /* Quad      */ {[](int M, int K) { return M >= 10 && M <= 16 && M % 2 == 0 && K >= 1 && K <= 4; }, [](int K) { return K >= 2 ? 2 : 1; }, kBinsPerWave, 8, Partials::F64, 2, true, true, false, true, CovKind::Quad},
    // float32 vector-ALU kernel for 10, 12, 14, 16 channels and up to 16 sources in ONE pass (kernels_cov_half16.hip)
    /* Half16    */ {[](int M, int K) { return M >= 10 && M <= 16 && M % 2 == 0 && K >= 1 && K <= 16; }, [](int K) { return K <= 8 ? 8 : (K <= 12 ? 12 : 16); }, 2, 16, Partials::F64, 2, true, true, false, true, CovKind::Half16},
    // 9..16 sources on 10/12/14/16 channels (odd counts: the padded copy of X), kernels_cov_hmfma.hip
    /* Hmfma     */ {[](int M, int K) { return M >= 10 && M <= 16 && M % 2 == 0 && K >= 9 && K <= 16; }, [](int K) { return K <= 8 ? 8 : (K <= 12 ? 12 : 16); }, 2, 32, Partials::F32IfPart32, 2, true, true, false, true, CovKind::Half16},
    // float64 sums (the `precise` arithmetic): 4 or 8 sources per pass.
    // (one or two sources stay on the fp64 matrix-core kernel: a two-source instantiation of this one measured 523-590 us against
    //  474 at 2048 bins x 4000 frames x 16 channels -- the 34 conversion and product instructions per lane and frame are then
    //  two thirds of the work; three or four sources: 692 against 836 us, five to eight 1.06 against 1.57 ms, sixteen 2.08 against 3.10)
    /* Half16F64 */ {[](int M, int K) { return M >= 10 && M <= 16 && M % 2 == 0 && K >= 3 && K <= 16; }, [](int K) { return K <= 4 ? 4 : 8; }, 2, 16, Partials::F64, 2, true, true, false, true, CovKind::Mfma},
    // float64 sums (`precise`): exactly 16 channels (15: the padded copy of X), 9..16 sources
    /* Hmfma64   */ {[](int M, int K) { return M == 16 && K >= 9 && K <= 16; }, [](int K) { return K <= 4 ? 4 : 8; }, 2, 32, Partials::F64, 2, true, true, false, true, CovKind::Mfma},
    // planar matrix-core kernel for 9..16 channels (one wave per (bin, split), four sources per wave: kc stays 1 and is not read)
    /* Mfma      */ {[](int M, int K) { return M >= 9 && M <= 16 && K >= 1 && K <= M; }, [](int) { return 1; }, kBinsPerWave, 4, Partials::Acc, 2, false, false, false, true, CovKind::Mfma},
    // 17..32 channels (kernels_wide.hip): float64 sums of exact float64 products whatever the arithmetic mode
    /* Wide      */ {[](int M, int K) { return M > kNarrowMax && M <= kWideMax && K >= 1 && K <= M; }, [](int K) { return std::min(K, 2); }, 1, 4, Partials::F64, 2, false, false, false, true, CovKind::Wide},
};
constexpr const CovTraits& traits(CovKind k) { return kCovTraits[(int)k]; }
// element type of the covariance partials a pass of kind g.kind leaves
constexpr bool partials_f64(const CovGeom& g, bool cov_f64) {
    return traits(g.kind).partials == Partials::F64 || (traits(g.kind).partials == Partials::Acc ? cov_f64 : !g.part32);
}

struct PowTraits {
    bool (*supported)(int M, int K);
    int (*sources)(int K);             // sources per pass over X (the matrix-core kernels take all in one pass and do not read kp)
    int bins;                          // bins per workgroup (one part of Ppart)
    int quantum;                       // tcp is a multiple of it
    bool padded_x;                     // reads the padded copy of X where the plan holds a current one
    bool occupancy;                    // the rounds of its grid are counted from an occupancy query
};
constexpr int pow_sources_per_pass(int /*M*/, int K) {
    // (round 5, measured and dropped: all of 5..8 sources in ONE pass, power_kernel<M, 8> -- 2049 x 235: 5 / 5 10.3 -> 11.7 us,
    //  6 / 6 11.9 -> 12.8, 7 / 7 13.5 -> 14.5, 8 / 8 17.8 -> 18.9; 2048 x 4000: 8 / 8 121 -> 129, 5 / 5 75 -> 76, only 8 / 5
    //  140 -> 111: eight demixing products per frame make the pass arithmetic-bound, two passes of four overlap)
    return K >= 3 ? 4 : (K >= 2 ? 2 : 1);
}
// the (channels, sources per pass) that rule can ask for with K <= M: the launchers of the lane power kernels (plan, batch, ragged
// batch, PCA projection) instantiate these and no others (tests/test_kernel_census.py)
constexpr bool pow_kp_reachable(int M, int kp) { return kp == 1 || (kp == 2 && M >= 2) || (kp == 4 && M >= 3); }
constexpr PowTraits kPowTraits[kPowKinds] = {
    /* Lane */ {[](int M, int K) { return M >= 1 && M <= kNarrowMax && K >= 1 && K <= M && (M <= 8 || K <= 4); }, [](int K) { return pow_sources_per_pass(0, K); }, kBinsPerWave * kWaves, 4, false, true},
    // more than 4 sources would take several VALU passes over X (register budget): one MFMA pass instead
    // (measured at 16 channels: 16 sources 770 -> 325 us; 2 sources 191 us VALU vs 332 us MFMA); an odd channel count
    // reads the copy of X padded by one zero channel (16-byte loads instead of 8-byte ones)
    /* Mfma */ {[](int M, int K) { return M > 8 && M <= kNarrowMax && K > 4 && K <= M; }, [](int K) { return pow_sources_per_pass(0, K); }, kBinsPerWave * kWaves, 4, true, false},
    // 16 channels, at least 64 bins: X staged through LDS in 2 KB runs (power_lds_kernel); $OIVA_POWER_LDS=0: off
    /* Lds  */ {[](int M, int K) { return M == 16 && K > 4 && K <= M; }, [](int K) { return pow_sources_per_pass(0, K); }, kBinsPerWave * kWaves, 4, false, false},
    /* Wide */ {[](int M, int K) { return M > kNarrowMax && M <= kWideMax && K >= 1 && K <= M; }, [](int K) { return K >= 3 ? 4 : K; }, kBinsPerWave * kWaves, 4, false, false},
};
constexpr const PowTraits& traits(PowKind k) { return kPowTraits[(int)k]; }

// ---- the choice ------------------------------------------------------------------------------------------------------------------
struct ChoiceIn {
    int T, F, F_total, M, K;
    int n_cu;
    bool cov_f64, upd_f64;     // OIVA_PREC_COV_F64, OIVA_PREC_UPDATE_F64: the two precision bits the choice depends on
    bool cov_quad_on = true;   // oiva_plan_set_cov_quad
    bool cov_hmfma_on = true;  // oiva_plan_set_cov_hmfma
    bool part32 = false;       // $OIVA_HMFMA_PART32=1: float32 partials where the kind can leave them
    bool kc_wide = true;       // $OIVA_COV_KC_WIDE
    bool power_lds = true;     // $OIVA_POWER_LDS
    double x_resident_mb = 0.; // the budget of the load policy of X (XPolicy): where X streams, the power pass takes other chunks
};
// the only device queries the choice makes: workgroups of an instantiation one CU holds at once (< 1: the query failed)
struct Occupancy {
    std::function<int(int M, int kc, bool f64)> cov_blocks_per_cu;
    std::function<int(int M, int kp, int tcp)> pow_blocks_per_cu;
};

// sources handled per pass over X by the Lane kernels
inline int lane_sources_per_pass(int M, int K, bool f64, bool short_axis, bool kc_wide) {
    const int regs = M * M * (f64 ? 2 : 1);   // as many as fit the accumulator budget (KC * M^2 <= 144 registers)
    int kc = 1;
    if (K >= 2 && regs * 2 <= 144) kc = 2;
    if (K >= 3 && regs * 4 <= 144) kc = 4;
    // 7 channels / 3+ sources and 5 / 5: a third / fifth source per pass (147 / 125 accumulators: two waves per SIMD instead of
    // three, a pass of 7 channels 100 us instead of 75 at 2048 x 4000) where that saves a whole pass over X.  Measured (covariance
    // pass, iteration): 2048 x 4000 x 7 / 3 162 -> 105 us (239 -> 198), 5 / 5 121 -> 93 (203 -> 181), 2049 x 235 x 7 / 3 22.0 ->
    // 16.5 (51.8 -> 47.6), 7 / 7 34.0 -> 27.2 (73.8 -> 66.6); not 7 / 4 (two passes either way: 21.8 -> 23.4) and 7 / 7 only on
    // a short frame axis (2048 x 4000: three passes of three 294 us, four of two 283).  $OIVA_COV_KC_WIDE=0: off.
    if (!f64 && kc_wide) {
        if (M == 7 && (K == 3 || K == 5 || K == 6 || (K == 7 && short_axis))) kc = 3;
        if (M == 5 && K >= 5) kc = 5;
    }
    return kc;
}

// Frame splits are chosen so that the grid is a whole number of "rounds" of what the chip holds at
// once (CUs x resident workgroups per CU): a grid of 1.5 rounds runs as long as one of 2.
inline int pick_splits(int capacity, int blocks_per_split, int T, int min_frames) {
    int ns = std::max(1, capacity / std::max(1, blocks_per_split));
    ns = std::min(ns, std::max(1, T / std::max(1, min_frames)));   // every split keeps >= min_frames frames
    return ns;
}

// Kernels with four frame phases per workgroup, float64 per-bin algebra behind them (`mixed`): 8 frame splits on a long
// frame axis, 4 on a short one (their float32 chains are then T / 32 resp. T / 16 frames); on a short axis never more than
// one round of workgroups (a workgroup's fixed costs dominate there) or splits of fewer than 16 frames.
inline int mixed_min_splits(int capacity, int blocks_per_split, int T) {
    if (T >= 1024) return 8;       // (a second round of workgroups costs little there: +18 us of 270 at 2048 x 4000 x 16 / 2)
    const int one_round = std::max(1, capacity / std::max(1, blocks_per_split));
    return std::max(1, std::min(std::min(4, one_round), T / 16));
}

// 9, 11, 13, 15 channels: the plan holds a copy of X padded by one zero channel (oiva_plan_create), which the vector-ALU
// kernels of 10..16 channels read
constexpr bool padded_channels(int M) { return M > 8 && M <= kNarrowMax && M % 2 == 1; }

// the kind by priority: the first whose predicate and condition hold
inline CovKind choose_cov_kind(const ChoiceIn& c) {
    const int M = c.M, K = c.K;
    if (M > kNarrowMax) return CovKind::Wide;
    if (M <= 8) {
        // float64, 8 channels: two lanes per (bin, frame), 32 bins per workgroup (kernels_cov_pair64.hip); else 16 bins
        // (same geometry, float32: 8 channels with three or more sources, four per pass -- kernels_cov_pair32.hip)
        if (!c.cov_f64 && traits(CovKind::Pair32).supported(M, K)) return CovKind::Pair32;
        if (c.cov_f64 && traits(CovKind::Pair64).supported(M, K)) return CovKind::Pair64;
        return CovKind::Lane;
    }
    // few sources: the Hermitian half on the vector ALU, four lanes per (bin, frame).  One or two sources are one pass
    // over X and faster than the matrix-core kernel in any mode; three or four are two passes, slower than its float32
    // form (measured 486-517 against 459 us at 2048 x 4000 x 16) but with float64 partial sums of short float32 chains,
    // which is what the float64 per-bin algebra of the `mixed` mode needs -- and 1.8 times faster than the float64
    // matrix-core pass that mode would otherwise have to be replaced by
    // (9, 11, 13, 15 channels: the same kernels on the copy of X padded by one zero channel, plan_covariance)
    const int Mc = M + (padded_channels(M) ? 1 : 0);
    if (!c.cov_f64 && c.cov_quad_on && traits(CovKind::Quad).supported(Mc, K) && (K <= 2 || c.upd_f64)) return CovKind::Quad;
    // many sources (5..16): the Hermitian half over 32 lanes per (bin, frame), every source in one pass; a wave's float32
    // chain is T / (4 nsplit) frames: <= 256 in `fast`, <= 128 with the float64 per-bin algebra behind it
    // (float64 sums, `precise`, 3..16 sources: the same lanes with four or eight sources per pass; splits only to fill the chip)
    if (c.cov_quad_on && (c.cov_f64 ? traits(CovKind::Half16F64).supported(Mc, K) : K > 4 && traits(CovKind::Half16).supported(Mc, K))) {
        // nine and more sources: the weighted sums of all sources as one small GEMM per bin on the fp32 matrix cores, the
        // Hermitian products on the vector ALU beside it (kernels_cov_hmfma.hip; on by default)
        const CovKind hm = c.cov_f64 ? CovKind::Hmfma64 : CovKind::Hmfma;
        if (c.cov_hmfma_on && traits(hm).supported(Mc, K)) return hm;
        return c.cov_f64 ? CovKind::Half16F64 : CovKind::Half16;
    }
    return CovKind::Mfma;
}

inline CovGeom choose_cov(const ChoiceIn& c, const Occupancy& occ, int nsplit_req) {
    CovGeom g{};
    g.kind = choose_cov_kind(c);
    const CovTraits& t = traits(g.kind);
    const int T = c.T, F = c.F, K = c.K, n_cu = c.n_cu;
    g.pad = padded_channels(c.M) ? 1 : 0;
    g.nbg = ceil_div(F, t.bins);
    g.kc = t.sources ? t.sources(K) : lane_sources_per_pass(c.M, K, c.cov_f64, T < 1024, c.kc_wide);
    int nsplit = nsplit_req;
    switch (g.kind) {
        case CovKind::Wide:
            // 17..32 channels (kernels_wide.hip): one workgroup per (bin, split, pass of sources), float64 sums in every mode;
            // splits only to fill the chip with two workgroups per CU
            if (nsplit <= 0) {
                // (counted on F_total, not on this plan's bins: every rank of a bin-sharded run then groups the frames of a bin
                //  into the same splits as one plan over all bins does, and its float64 partials add up to the same bits)
                const int groups = c.F_total * ceil_div(K, g.kc);
                nsplit = 1;
                while (groups * nsplit < 2 * n_cu && ceil_div(T, nsplit + 1) >= 128) ++nsplit;
            }
            break;
        case CovKind::Quad:
            // one round of two workgroups per CU
            if (nsplit <= 0) {
                const int blocks = g.nbg * ceil_div(K, g.kc);
                nsplit = std::min(32, pick_splits(n_cu * 2, blocks, T, T >= 1024 ? 128 : 64));
                // only 4 frame phases per workgroup: a lane's float32 chain is T / (4 nsplit) frames, four times that of the
                // 8-channel kernel at equal splits, and the error of the result grows linearly with it (measured against
                // the reference's own complex64 floor, 16 channels / 2 sources x 20 iterations: T = 4000: 4 splits 0.8-1.0
                // floors, 8 splits 0.5-0.6, 16 splits 0.3; T = 163: 1 split 1.4, 4 splits 0.8, 8 splits 0.6).  With the
                // float64 per-bin algebra (`mixed`, the default arithmetic of these shapes) the chains are what is left of
                // the error, so that mode takes 8 splits (+18 us on the pass, +8 us in the update at 2048 x 4000 x 16 / 2).
                // ... as long as that is still one round of workgroups (few frames: 4 splits = chains of T / 16, 0.8 floors)
                if (c.upd_f64) nsplit = std::max(nsplit, mixed_min_splits(n_cu * 2, blocks, T));
            }
            break;
        case CovKind::Half16:
        case CovKind::Hmfma:
        case CovKind::Half16F64:
        case CovKind::Hmfma64: {
            const bool hm = g.kind == CovKind::Hmfma || g.kind == CovKind::Hmfma64;
            if (nsplit <= 0) {
                // (float64: no chain to bound; the four-source form runs a little faster in two rounds of workgroups -- 2048 x 4000
                //  x 16 / 4: 1 split 744 us, 2 splits 691, 4 splits 693; the eight-source form does not care)
                // (the matrix-core kernel: one bin per workgroup and eight float32 chains -- half the splits for the same chain)
                const int chains = hm ? 8 : 4;
                nsplit = c.cov_f64 ? (!hm && g.kc == 4 && T >= 1024 ? 2 : 1) : ceil_div(T, chains * (c.upd_f64 ? 128 : 256));
                const int per_cu = hm ? (c.cov_f64 ? 2 : 3) : c.cov_f64 && g.kc == 4 ? 4 : 2;      // workgroups a CU holds (registers / launch bounds)
                const int groups = hm ? F : g.nbg * ceil_div(K, g.kc);
                while (groups * nsplit < per_cu * n_cu && ceil_div(T, nsplit + 1) >= 64) ++nsplit;
            }
            // (round 6, opt-in: $OIVA_HMFMA_PART32=1, read whenever the geometry is chosen) the float32 matrix-core kernel hands its
            // partial blocks over as float32 -- half the bytes the per-bin update is bound by at 16 x 16 (update 66 -> 50 us, iteration
            // 931 -> 903 us) for one more rounding per block: W moves by 1e-8 on i.i.d. input and by 3e-6 .. 1e-5 (0.3-0.5 reference
            // floors) on a 16-source mixture at full size, and the fixtures of <= 1024 frames land up to twice as far from the
            // complex128 result (tools/r6/part32_ab.py, tools/r6/NOTES.md).  Not the default: parity first.
            if (t.partials == Partials::F32IfPart32) g.part32 = c.part32 ? 1 : 0;
            break;
        }
        case CovKind::Mfma:
            // planar matrix-core path: one wave per (bin, split); splits bound the length of the fp32
            // accumulation chain (<= 512 frames) and keep >= 2 waves per SIMD when there are few bins
            if (nsplit <= 0) {
                nsplit = ceil_div(T, 512);
                const int waves = F * ceil_div(K, 4);
                while (waves * nsplit < 2 * 4 * n_cu && ceil_div(T, nsplit + 1) >= 64) ++nsplit;
            }
            break;
        case CovKind::Lane:
        case CovKind::Pair32:
        case CovKind::Pair64:
            if (nsplit <= 0) {
                const int nz = ceil_div(K, g.kc);
                int bpc = 2;      // (the pair kernels: two workgroups per CU)
                if (g.kind == CovKind::Lane && (bpc = occ.cov_blocks_per_cu(c.M, g.kc, c.cov_f64)) < 1) bpc = 2;
                // one round: the grid is what the chip holds at once (CUs x resident workgroups); every workgroup pays a
                // fixed cost (gamma prologue, ring fill, epilogue), so fewer, longer workgroups win as long as the chip
                // is full, and 1.5 rounds run as long as 2
                // (on a short frame axis at least 64 frames per split instead of 128: at the reference's 160-235 frames the floor of
                //  128 left the chip to one split -- 2049 x 235 x 8 / 2: 1 split 18.9 / 29.2 us (float32 / float64), 3 splits 14.7 /
                //  16.8.  On a long axis the floor of 128 stays: a 256-bin shard of 4000 frames takes 28 splits in 20.4 us, 32 splits
                //  -- exactly the chip's 512 workgroup slots, which the dispatcher does not fill evenly -- 26.3)
                nsplit = pick_splits(n_cu * bpc, g.nbg * nz, T, T >= 1024 ? 128 : 64);
                // a grid that fills the chip's workgroup slots EXACTLY runs slower than one an eighth short of it (the dispatcher does
                // not fill the CUs evenly): 512 bins x 4000 frames, 16 splits = 512 workgroups 31.4 us, 14 splits 29.5 us; 256 bins: 32
                // splits 26.3 us, 28 splits 20.4 us
                if (nsplit >= 12 && g.nbg * nz * nsplit >= n_cu * bpc) nsplit = nsplit * 7 / 8;
                // the update kernel adds the nsplit partials of every matrix element in one round of loads per 16 splits
                // (sum_vpart); more than 32 splits cost more there than the fuller grid saves here (measured on a
                // 256-bin shard: 16 splits 25.2 + 8.0 us, 28 splits 21.4 + 9.2 us, 42 splits 25.5 + 10.3 us)
                // ... unless 32 splits would leave most of the chip idle (few bins, very long frame axis): then the
                // streaming pass dominates and up to 64 splits are allowed
                const int cap = (g.nbg * nz * 32 >= n_cu) ? 32 : 64;
                nsplit = std::min(nsplit, cap);
                // four frame phases per workgroup instead of 16: float32 chains four times as long at equal splits; with the
                // float64 per-bin algebra behind it the pass takes at least 8 splits (see the 10..16-channel kernel above)
                // (round 5: on a short frame axis the bound is the chain itself -- T / (4 nsplit) <= 64 frames, what 4 splits give just below
                //  1024 frames -- not 4 splits whatever T: at the reference's 2049 bins x 235 frames the forced fourth split cost 8 / 4
                //  sources 26.8 against 21.2 us on the pass (iteration 74.4 -> 69.2 us), 8 / 3 23.0 against 19.2 (63.5 -> 59.4))
                if (g.kind == CovKind::Pair32 && c.upd_f64) {
                    const int by_chain = T >= 1024 ? 8 : std::min(4, ceil_div(T, 256));
                    nsplit = std::max(nsplit, std::min(by_chain, mixed_min_splits(n_cu * bpc, g.nbg * nz, T)));
                }
            }
            break;
    }
    g.tc = round_up(ceil_div(T, nsplit), t.quantum);
    g.nsplit = ceil_div(T, g.tc);
    return g;
}

inline PowKind choose_pow_kind(const ChoiceIn& c) {
    if (c.M > kNarrowMax) return PowKind::Wide;
    if (!traits(PowKind::Mfma).supported(c.M, c.K)) return PowKind::Lane;
    // (power_lds_kernel: whole 64-bin batches of 16 unpadded channels, at least one tile of 16 frames)
    if (c.power_lds && traits(PowKind::Lds).supported(c.M, c.K) && c.F >= kBinsPerWave * kWaves && c.T >= 16) return PowKind::Lds;
    return PowKind::Mfma;
}

// Does the load policy of X stream some group of this shape, as far as budget, size and kernels decide it?  (The geometry has
// the last word: choose_x_policy on the splits and chunks that were chosen.)
inline bool x_streams_by_kernels(const ChoiceIn& c, PowKind pk) {
    CovGeom cg{};
    cg.kind = choose_cov_kind(c), cg.tc = kXGroup;
    PowGeom pg{};
    pg.kind = pk, pg.tcp = 4;
    return choose_x_policy(c.x_resident_mb, c.T, c.F, c.M, c.cov_f64, cg, pg).nt;
}

inline PowGeom choose_pow(const ChoiceIn& c, const Occupancy& occ, int nsplit_req) {
    PowGeom g{};
    g.kind = choose_pow_kind(c);
    const PowTraits& t = traits(g.kind);
    const int T = c.T, n_cu = c.n_cu;
    g.nb = ceil_div(c.F, t.bins);
    g.kp = t.sources(c.K);
    int nsplit = nsplit_req;
    if (g.kind == PowKind::Wide) {
        // 17..32 channels (kernels_wide.hip): one lane per bin of a 64-bin batch; about four workgroups per CU
        const int groups = g.nb * ceil_div(c.K, g.kp);
        if (nsplit <= 0) nsplit = pick_splits(n_cu * 4, groups, T, 16);
        g.tcp = round_up(ceil_div(T, nsplit), t.quantum);
        g.nsplit = ceil_div(T, g.tcp);
        return g;
    }
    if (nsplit <= 0) {
        // Workgroups so that about 48 KB of X are in flight per CU: a wave keeps two steps (2 x 4 frames x 16 bins x 8M
        // bytes) in flight, i.e. 12 / M workgroups per CU -- 1.5 at 8 channels, 3 at 4, 0.75 at 16.  Measured at 2048 bins
        // x 4000 frames on the kernel itself and on the pure-read form of its geometry (tools/membench.hip, pattern P):
        // 8 channels 12 splits (384 workgroups) 88-90 us, 16: 91, 24: 92, 8: 106 (four steps in flight and 24 splits, as in
        // round 1: 94-96 us); 4 channels 24 splits 40.7 us, 12: 46; 2 channels 24 splits 21.8, 12: 35; 16 channels / 2
        // sources 6 splits 172 us, 12: 234.  More resident waves thrash the 32 KB L1, fewer expose HBM latency.  Each
        // workgroup loads its W first (256-bin shard: 62 splits 13.5 us, 167 splits 15.9 us).
        // (counted per source pass: with 8 sources in two passes, 12 splits 112 us, 6 splits 127-137 us)
        // ONE source per pass halves the arithmetic per byte and a wave runs through its two steps in flight before the next
        // ones arrive: twice the workgroups (8 channels / 1 source: 12 splits 111 us, 24 splits 92.5; with 2-4 sources 24
        // splits measure the same as 12)
        // (not beyond 8 channels: 16 channels / 1 source 6 splits 226 us, 12 splits -- 1.5 rounds of workgroups -- 276)
        const int per_cu_x12 = (g.kp == 1 && c.M <= 8) ? 24 : 12;
        // (at least 32 frames per workgroup: with 64, 2049 x 235 x 8 / 2 ran 3 splits in 16.0 us where 6-8 take 11.9-12.1,
        //  2049 x 160 x 4 / 2 2 splits in 12.0 us where 5-8 take 8.2-8.4)
        nsplit = pick_splits(std::max(n_cu / 2, n_cu * per_cu_x12 / std::max(c.M, 1)), g.nb, T, 32);
        // The instantiation that STREAMS X (8 channels, two sources per pass): ONE workgroup per CU where the grid can be that.
        // Its steps are whole 1-KB rows past the L1, so the reasoning above does not carry over, and more requests in flight make
        // it slower, not faster: 2048 x 4000 x 8 / 2, 268 MB resident, chunks through oiva_plan_set_pow_splits, power stage /
        // iteration in us: 8 chunks (256 workgroups of 500 frames) 77.6 / 177.9, 10 (1.25 workgroups per CU: the last quarter
        // runs alone) 89.5 / 191.1, 12: 84.8 / 186.4, 16: 85.0 / 186.7, 20: 85.0 / 187.0, 24: 82.5 / 184.9, 32: 95.4 / 198.0
        // (profiles/pow_splits_nt.log; the pure-read form says the same of deeper request queues: tools/mallbench.hip rows "e",
        // DESIGN §7).  Where the cap of tcp or the number of bin batches leaves no grid of 7/8 .. 1 workgroups per CU (2049 bins:
        // 33 x 8 = 264) the chunks above stay; one source per pass was not measured and keeps them too.
        if (g.kind == PowKind::Lane && g.kp == 2 && x_streams_by_kernels(c, g.kind)) {
            const int one = pick_splits(n_cu, g.nb, T, 32);
            const int tcp1 = std::min(std::max(round_up(ceil_div(T, one), t.quantum), 4), kPowMaxFrames);
            const long long grid = (long long)g.nb * ceil_div(T, tcp1);
            if (grid <= n_cu && grid * 8 >= (long long)n_cu * 7) nsplit = one;
        }
    }
    int tcp = round_up(ceil_div(T, nsplit), t.quantum);
    tcp = std::min(std::max(tcp, 4), kPowMaxFrames);
    g.tcp = tcp;
    g.nsplit = ceil_div(T, tcp);
    // rounds of workgroups the grid runs in (a long frame axis: tcp is capped, so the chunks outnumber the chip's slots)
    if (t.occupancy) {
        const int bpc = occ.pow_blocks_per_cu(c.M, g.kp, g.tcp);
        if (bpc > 0) g.rounds = (int)((((long long)g.nb * g.nsplit * ceil_div(c.K, g.kp)) + (long long)bpc * n_cu - 1) / ((long long)bpc * n_cu));
    }
    return g;
}

// ---- the per-bin update ------------------------------------------------------------------------------------------------------
// Which kernel launch_update runs (kernels_update.hip), for the plan, every batch, ILRMA and the PCA front end: one kind per kernel
// family, the table of what each is launched with (kUpdTraits), and the one function that chooses (choose_update).  The launchers
// behind launch_update only turn the integers of an UpdChoice into template arguments.
//   Sq .. Det: square layout, 1..8 channels, MP x MP lanes per bin (update_sq_kernel, update_bg_kernel, update_gram_kernel,
//   update_det_kernel); Rows: update_kernel, the row layout, SG lanes per bin (all kernels_update.hip); Wave16, Det16: one wavefront
//   per bin of 9..16 channels (update_wave16_kernel, update_det16_kernel: kernels_update16.hip); Det16Rows: update_det16r_kernel,
//   one matrix row per lane, three waves per four bins (kernels_update16r.hip); Wide: wide_update_kernel, 17..32 channels.
enum class UpdKind { Sq, Bg, Gram, Det, Rows, Wave16, Det16, Det16Rows, Wide };
constexpr int kUpdKinds = 9;
static_assert((int)UpdKind::Wide + 1 == kUpdKinds, "one traits row per kind");

// what the choice reads of the update's arguments (UpdateArgs, oiva_internal.h)
struct UpdIn {
    int M, K;
    bool use_double;   // per-bin algebra in float64
    bool vpart_f64;    // the covariance partials are float64
    bool init_only;    // only the J initialisation of the prologue
    int layout;        // 0: square (one lane per matrix element up to 8 channels), 1: one lane per matrix row
    int nsplit;        // covariance splits behind V (a ragged batch: the largest)
};
// the process's switches (update_switches(), host_util.hip): $OIVA_UPDATE_GRAM (0: off, 2: measurement only, every K through the
// Gram form), $OIVA_UPDATE_DET=0, $OIVA_DET16_INVERSE=1, $OIVA_DET16_ROWS=0
struct UpdSwitches {
    int gram = 1;
    bool det = true, det16_inverse = false, det16_rows = true;
};
struct UpdChoice {
    bool ok = false;               // false: no kernel takes these arguments
    UpdKind kind = UpdKind::Sq;
    int mp = 0;                    // Sq .. Det: MP, the padded channel count; Rows: SG, the lanes per bin
    int mt = 0, kt = 0;            // channel and source count as compile-time constants (0: taken at run time)
    bool f64 = false;              // arithmetic type (Gram, Det, Det16, Det16Rows, Wide: float64 always, not a template argument)
    bool vpart_f64 = false;        // partial type (a template argument of the 9..16-channel kernels only)
    bool flag = false;             // Wave16: OVER (K < M); Det16: INVERSE
    int block = 0;                 // lanes per workgroup
    int bins_per_block = 0;        // the grid is ceil_div(F, bins_per_block) workgroups
};

struct UpdTraits {
    const char* kernel;
    int m_lo, m_hi;                // channel counts
    int block;
    int bins;                      // bins per workgroup; 0: block / lanes per bin (MP x MP resp. SG of the choice)
    int max_splits;                // covariance splits the kernel adds (0: any number)
};
constexpr UpdTraits kUpdTraits[kUpdKinds] = {
    /* Sq        */ {"update_sq_kernel", 1, 8, kBlock, 0, 0},
    /* Bg        */ {"update_bg_kernel", 3, 8, kBlock, 0, 0},
    /* Gram      */ {"update_gram_kernel", 3, 8, kBlock, 0, 0},
    /* Det       */ {"update_det_kernel", 2, 8, kBlock, 0, 0},
    /* Rows      */ {"update_kernel", 1, kNarrowMax, kBlock, 0, 0},
    /* Wave16    */ {"update_wave16_kernel", 9, kNarrowMax, 64, 1, 0},
    /* Det16     */ {"update_det16_kernel", 9, kNarrowMax, 64, 1, 0},
    // frame splits the eliminating waves add, two in flight at a time (more: the one-matrix-per-wave kernel)
    /* Det16Rows */ {"update_det16r_kernel", 9, kNarrowMax, 192, 4, 4},
    /* Wide      */ {"wide_update_kernel", kNarrowMax + 1, kWideMax, kBlock, 1, 0},
};
constexpr const UpdTraits& traits(UpdKind k) { return kUpdTraits[(int)k]; }

// The instantiations there are of the 1..8-channel kernels: what choose_update can ask of the launcher of kernels_update.hip.
// Channel count MT (MP / 2 < MT <= MP) as a compile-time constant, and with it the source counts the reference's own sweeps use
// (overiva_sim_config.json: 2..8 microphones, 1..4 targets, determined AuxIVA): 1, 2, 3, 4, MT; other source counts (5 .. MT - 1)
// at run time; one channel: the run-time-shape kernel.
constexpr int upd_padded(int M) { return M <= 2 ? 2 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16)); }
constexpr bool upd_instantiated(UpdKind k, int mp, int mt, int kt) {
    const bool shape = mt >= 2 && mt <= 8 && mp == upd_padded(mt);
    const bool few = kt >= 1 && kt <= 4 && kt < mt, rest = kt == 0 && mt >= 6;
    switch (k) {
        case UpdKind::Sq: return (mp == 2 && mt == 0 && kt == 0) || (shape && (kt == mt || few || rest));
        case UpdKind::Bg: return shape && mp >= 4 && few && kt <= 2;
        case UpdKind::Gram: return shape && mp >= 4 && (few || rest);
        case UpdKind::Det: return shape && kt == mt;
        case UpdKind::Rows: return mt == 0 && kt == 0 && (mp == 2 || mp == 4 || mp == 8 || mp == 16);
        default: return true;
    }
}

// the rules, by priority: the first that holds
inline UpdChoice choose_update(const UpdIn& u, const UpdSwitches& sw) {
    UpdChoice c{};
    const int M = u.M, K = u.K;
    if (M < 1 || M > kWideMax || K < 1 || K > M) return c;
    c.f64 = u.use_double, c.vpart_f64 = u.vpart_f64;
    auto chosen = [&c](UpdKind k, int mp, int mt, int kt, bool flag = false) {
        const UpdTraits& t = traits(k);
        c.ok = true, c.kind = k, c.mp = mp, c.mt = mt, c.kt = kt, c.flag = flag;
        c.block = t.block;
        c.bins_per_block = t.bins ? t.bins : t.block / (k == UpdKind::Rows ? mp : mp * mp);
        return c;
    };
    // 17..32 channels, either layout: the matrices live in LDS; float64 in every arithmetic mode (use_double is not consulted)
    if (M > kNarrowMax) return chosen(UpdKind::Wide, 0, 0, 0);
    // the row layout.  Run-time M and K only: folding them as constants made this variant slower (the fully unrolled source
    // loop spills: 16 channels / 16 sources 0.89 -> 1.67 ms)
    if (u.layout != 0) return chosen(UpdKind::Rows, upd_padded(M), 0, 0);
    const bool det_case = K == M && u.use_double && !u.init_only;      // determined, float64, a whole update
    if (M > 8) {      // 9..16 channels, square layout: one wavefront per bin ...
        // ... or, determined in float64 on at most four splits, one matrix row per lane ($OIVA_DET16_ROWS=0: the kernels below)
        if (sw.det16_rows && det_case && u.nsplit <= traits(UpdKind::Det16Rows).max_splits) return chosen(UpdKind::Det16Rows, 0, 0, 0);
        if (sw.det && det_case) return chosen(UpdKind::Det16, 0, 0, 0, sw.det16_inverse);
        return chosen(UpdKind::Wave16, 0, 0, 0, K < M);
    }
    // square layout, up to 8 channels: one lane per matrix element
    const int mp = upd_padded(M);
    if (M == 1) return chosen(UpdKind::Sq, mp, 0, 0);
    // 1 or 2 sources with background channels: the structured chain with closed-form K x K solves; 3 and more (float64): the
    // Gram form (update_gram_kernel).  2049 x 235, float64, update stage, generic kernel -> this dispatch: 8 / 3 23.0 -> 21.9 us,
    // 6 / 3 20.2 -> 16.6, 5 / 3 18.7 -> 15.4, 8 / 4 39.5 -> 28.4, 6 / 4 37.8 -> 22.2, 8 / 6 64.2 -> 37.3; with one or two sources the
    // Gram form is on a par with the structured chain (8 / 2 15.4 against 13.7 us, 6 / 2 11.2 / 11.9, 8 / 1 8.6 / 7.7), which
    // the X-resident kernel shares.  (The J initialisation of the prologue keeps the generic kernel.)
    if (mp >= 4 && !u.init_only && K < M) {
        if (sw.gram == 2 && u.use_double && K <= 2) return chosen(UpdKind::Gram, mp, M, K);      // (measurement only: every K through the Gram form)
        if (K <= 2) return chosen(UpdKind::Bg, mp, M, K);
        if (sw.gram && u.use_double) return chosen(UpdKind::Gram, mp, M, K <= 4 ? K : 0);
    }
    // determined: one elimination for the inverse of W_hat^H, a rank-one step per source
    // (float64 only: in float32 the explicit inverses cost accuracy -- 8 / 8 mixture, 20 iterations: 6.5 reference floors
    //  against 2.8 with the elimination per source -- and `fast` keeps the latter)
    if (sw.det && det_case) return chosen(UpdKind::Det, mp, M, M);
    return chosen(UpdKind::Sq, mp, M, K == M || K <= 4 ? K : 0);
}

// the normal form of a choice: the kernel with its template arguments as a demangler prints them, `update_sq_kernel<8, double, 8, 2>`
inline std::string update_kernel_name(const UpdChoice& c) {
    const std::string r = c.f64 ? "double" : "float", v = c.vpart_f64 ? "double" : "float", b = c.flag ? "true" : "false";
    const std::string mp = std::to_string(c.mp), mt = std::to_string(c.mt), kt = std::to_string(c.kt);
    std::string args;
    switch (c.kind) {
        case UpdKind::Sq:
        case UpdKind::Bg:
        case UpdKind::Rows: args = mp + ", " + r + ", " + mt + ", " + kt; break;
        case UpdKind::Gram: args = mp + ", " + mt + ", " + kt; break;
        case UpdKind::Det: args = mp + ", double, " + mt; break;
        case UpdKind::Wave16: args = r + ", " + v + ", " + b; break;
        case UpdKind::Det16: args = v + ", " + b; break;
        case UpdKind::Det16Rows: args = v; break;
        case UpdKind::Wide: return traits(c.kind).kernel;
    }
    return std::string(traits(c.kind).kernel) + "<" + args + ">";
}

// ---- the fused covariance + update launch (kernels_cov_update.hip) -----------------------------------------------------------
constexpr int kCovUpdateBins = 4;      // bins per workgroup = waves (one per bin in the update)
// eligible: 8 channels, 2 sources, four frame splits of a whole number of 16-frame steps (what the plan chooses at the headline
// shape)
inline bool cov_update_supported(int M, int K, int T, int F, int nsplit, int tc) {
    // (32-bit buffer offsets; whole steps: every split, and with it T, a multiple of 16 frames)
    return M == 8 && K == 2 && nsplit == kWaves && tc % 16 == 0 && T % 16 == 0 && T > (kWaves - 1) * tc && F >= kCovUpdateBins &&
           (size_t)T * F * M * 8 < ((size_t)1 << 31);       // (buffer addressing of X: 32-bit offsets)
}

}  // namespace oiva
