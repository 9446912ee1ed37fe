"""Small plans and batches that really RUN every per-bin update kernel family (csrc/kernel_choice.h: UpdKind) at the smallest shapes
at which a launcher can still go wrong: one bin, and one bin more than a workgroup holds (a ragged last workgroup), 40..70 frames.
Shared by tests/test_update_choice_gpu.py and tools/ab_plan_bits.py / ab_batch_bits.py (``--update-cases``), which recorded
tests/golden/update_parent_bits.json on the build before choose_update existed."""
import hashlib

import numpy as np

MODES = ("fast", "mixed", "precise")
SQUARE = [(1, 1), (2, 1), (2, 2), (3, 2), (4, 3), (4, 4), (5, 3), (6, 4), (7, 6), (8, 1), (8, 2), (8, 5), (8, 8)]
ROWS = [(3, 2), (8, 8), (12, 3)]


def padded(M):
    return 2 if M <= 2 else 4 if M <= 4 else 8 if M <= 8 else 16


def _plans():
    """(M, K, mode, row layout, T, F, covariance splits asked for (0: the plan's own), matrix-core covariance pass)"""
    cases, n = [], 0

    def add(M, K, mode, rows, F, splits=0):
        nonlocal n
        # (70 frames in steps of 4 are 4 splits of 20 and 5 splits of 16; the other plans take what the rule gives them)
        cases.append((M, K, mode, rows, 70 if splits else 40 + (7 * n) % 31, F, splits, splits > 0))
        n += 1

    for M, K in SQUARE:      # MP x MP lanes per bin, 256 lanes per workgroup
        for i, mode in enumerate(MODES):
            add(M, K, mode, False, 256 // padded(M) ** 2 + 1)
        add(M, K, MODES[n % 3], False, 1)
    for M, K in ROWS:        # SG lanes per bin
        for mode in MODES:
            add(M, K, mode, True, 256 // padded(M) + 1)
        add(M, K, MODES[n % 3], True, 1)
    # determined, 9..16 channels, float64: four splits, four bins per wave (Det16Rows); five splits, one bin per wave (Det16)
    for M in (16, 9):
        for mode in MODES[1:]:
            for F in (5, 9):
                add(M, M, mode, False, F, 4)
            for F in (1, 2):
                add(M, M, mode, False, F, 5)
    for M, K in ((16, 16), (12, 3), (16, 2)):      # one wavefront per bin (Wave16): determined in float32, K < M in any arithmetic
        for mode in MODES if K < M else MODES[:1]:
            add(M, K, mode, False, 2)
        add(M, K, "fast", False, 1)
    for mode in MODES[:2]:                          # 17..32 channels (Wide)
        add(17, 3, mode, False, 2)
    add(17, 3, "precise", False, 1)
    return cases


PLAN_CASES = _plans()
# (entry point, M, K, B, F, frames): B x F bins in one launch, a ragged last workgroup
BATCH_CASES = [(kind, M, K, 3, F, frames) for M, K, F in ((4, 2, 11), (6, 6, 3))
               for kind, frames in (("dense", (55,) * 3), ("ragged", (40, 70, 55)), ("c128", (47,) * 3))]


def plan_id(c):
    M, K, mode, rows, T, F, splits, _ = c
    return f"plan M{M}K{K}-{mode}" + ("-rows" if rows else "") + f"-T{T}F{F}" + (f"-splits{splits}" if splits else "")


def batch_id(c):
    kind, M, K, B, F, frames = c
    return f"batch {kind} M{M}K{K}-B{B}F{F}-T" + "+".join(str(t) for t in sorted(set(frames)))


def table_row(c):
    """the (M, K, use_double, init_only, layout, nsplit) of a plan case's iterations as tests/golden/update_choice.json has them"""
    M, K, mode, rows, T, F, splits, _ = c
    return M, K, int(mode != "fast"), 0, int(rows), splits if 9 <= M <= 16 and K == M and splits else 1


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def combined(parts):
    """one digest over the digests of W after one iteration, W after three and Y: what the golden file holds per case"""
    return hashlib.sha256((parts["W1"] + parts["W3"] + parts["Y"]).encode()).hexdigest()


def run_plan(oa, orc, c):
    """digests of W after one and after three iterations and of Y"""
    M, K, mode, rows, T, F, splits, matrix_core = c
    X = orc.synth_iid(T, F, M, seed=1000 * M + 10 * K + F)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode, row_layout=rows)
        if matrix_core:      # (its frame quantum of 4 leaves 4 and 5 splits of 40..70 frames as asked)
            p.set_cov_quad(False)
        if splits:
            p.set_cov_splits(splits)
            assert p.cov_splits() == splits, (plan_id(c), p.cov_splits())
        p.set_x(X)
        p.covariance()
        p.set_w()            # (K < M: the J initialisation, init_only)
        out = {}
        p.iterate(1)
        out["W1"] = digest(p.get_w(np.complex128))
        p.iterate(2)
        out["W3"] = digest(p.get_w(np.complex128))
        out["Y"] = digest(p.demix(proj_back=True))
    return out


def run_batch(oa, orc, c):
    kind, M, K, B, F, frames = c
    Xs = [orc.synth_iid(T, F, M, seed=2000 * M + 10 * K + b) for b, T in enumerate(frames)]
    if kind == "c128":
        Xs = [x.astype(np.complex128) for x in Xs]
    out = {}
    for n_iter in (1, 3):
        if kind == "ragged":
            Y, W = oa.overiva_batch_ragged(Xs, n_src=K, n_iter=n_iter, return_filters=True)
            Y = np.concatenate([y.ravel() for y in Y])
        else:
            Y, W = oa.overiva_batch(np.stack(Xs), n_src=K, n_iter=n_iter, return_filters=True,
                                    data="complex128" if kind == "c128" else "complex64")
        out[f"W{n_iter}"] = digest(W)
    out["Y"] = digest(Y)
    return out
