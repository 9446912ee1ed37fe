"""five_batch() / five() on the GPU: the reduction and one per-bin step from a known state against the NumPy
restatement (tests/helpers/five_oracle.py), iterated results under the restatement's own yardstick, bits that do not depend on
the batch, the public calls, a room whose input covariance is singular, and a mixture out of which a source comes.

Every figure is printed before it is asserted (DESIGN.md 3.16 has the measured ones).
"""
import os
import sys

import numpy as np
import pytest
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import five_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12        # float64 stages, of the largest entry: the bound test_ilrma_gpu.py and test_iss_gpu.py hold them to
TOL_P = 1e-10      # the defining properties of the step


def open_plan(X, model="laplace", W0=None, init_eig=True):
    """a plan with FIVE begun on X: (B, T, F, M), or a list of (T_b, F, M) rooms"""
    from overiva_amd import BatchPlan, RaggedBatchPlan

    if isinstance(X, list):
        F, M = X[0].shape[1:]
        plan = RaggedBatchPlan([x.shape[0] for x in X], F, M, 1, model)
    else:
        B, T, F, M = X.shape
        plan = BatchPlan(B, T, F, M, 1, model)
    plan.set_x(X)
    plan.covariance()
    if W0 is None and init_eig:
        plan.set_w_eig()
    else:
        plan.set_w(W0)
    plan.five_begin()
    return plan


def quad(w, A):
    """w^H A w per bin: w (F, M), A (F, M, M)"""
    return np.einsum("fm,fmn,fn->f", np.conj(w), A, w)


def new_seen():
    return dict(norm=0.0, residual=0.0, rho=0.0, w=0.0, yardstick=np.inf, d_form=0.0, d_move=0.0, gap=np.inf, margin=0.0)


def check_update(X, w_prev, V, Cx, w, model, seen):
    """one room's update from the device's own V and Cx (w_prev: the w the stages before it ran on): the figures of the step into
    ``seen``; the restatement's gap is asserted before anything is compared"""
    wa, lam = fo.step_whitened(V, Cx)
    wb, _ = fo.step_pencil(V, Cx)
    seen["gap"] = min(seen["gap"], float(fo.gaps(lam).min()))
    assert seen["gap"] >= fo.MIN_GAP, seen["gap"]
    d_form = fo.wdist(wb, wa)
    d_move = fo.wdist(fo.one_step(fo.perturbed(X), w_prev, model)[0], fo.one_step(X, w_prev, model)[0])
    tol = 10.0 * max(d_form, d_move)
    Vw = np.einsum("fmn,fn->fm", V, w)
    Cw = np.einsum("fmn,fn->fm", Cx, w)
    rho = (quad(w, V) / quad(w, Cx)).real
    lam_min = np.array([scipy.linalg.eigh(V[f], Cx[f], eigvals_only=True)[0] for f in range(V.shape[0])])
    d_w = fo.wdist(w, wa)
    seen["norm"] = max(seen["norm"], float(np.max(np.abs(quad(w, V) - 1.0))))
    seen["residual"] = max(seen["residual"], float(np.max(np.linalg.norm(Vw - rho[:, None] * Cw, axis=1) / np.linalg.norm(Vw, axis=1))))
    seen["rho"] = max(seen["rho"], float(np.max(np.abs(rho - lam_min) / lam_min)))
    seen["d_form"], seen["d_move"] = max(seen["d_form"], d_form), max(seen["d_move"], d_move)
    seen["w"], seen["yardstick"] = max(seen["w"], d_w), min(seen["yardstick"], tol)
    seen["margin"] = max(seen["margin"], d_w / tol)


# ---- 1. the reduction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fo.SHAPES + ["ragged"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_the_reduction_whitens_cx(shape):
    """Li Cx Li^H = I to 1e-12 with the restatement's Cx, Li lower triangular with a positive diagonal"""
    X = fo.ragged_rooms() if shape == "ragged" else fo.rooms(shape)
    with open_plan(X) as plan:
        Li = plan.get_five_reduction()
        Cx_dev = plan.get_cx()
    worst = worst_cx = 0.0
    for b in range(len(X)):
        Cx = fo.covariance(X[b])
        M = Cx.shape[-1]
        worst_cx = max(worst_cx, fo.dist(Cx_dev[b], Cx))
        E = Li[b] @ Cx @ np.conj(np.swapaxes(Li[b], 1, 2)) - np.eye(M)
        worst = max(worst, float(np.max(np.abs(E))))
        assert np.all(np.triu(Li[b], 1) == 0) and np.all(np.diagonal(Li[b], axis1=1, axis2=2).real > 0)
    print(f"five reduction {shape}: |Li Cx Li^H - I| {worst:.2e}, Cx against the restatement {worst_cx:.2e}")
    assert worst <= TOL and worst_cx <= TOL


# ---- 2. one update from a known state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.CASES, ids=fo.case_id)
def test_one_update_from_the_device_s_own_v(case):
    """stages 0 to 2 on the device, its V and Cx read back, then the update: w^H V w = 1 and V w = rho Cx w to 1e-10, rho the
    smallest generalized eigenvalue to 1e-10 relative, w within the yardstick of the restatement's w on that V and Cx
    (phase-free), and the complex64 copy the streaming passes read is the rounded float64 w"""
    shape, model = case
    X = fo.rooms(shape)
    with open_plan(X, model) as plan:
        w0 = plan.get_w(np.complex128)[..., 0]
        for s in ("power", "activation", "cov"):
            plan.five_stage(s)
        V = plan.get_weighted_cov()[:, :, 0]
        Cx = plan.get_cx()
        plan.five_stage("update")
        w = plan.get_w(np.complex128)[..., 0]
        assert np.array_equal(plan.get_w(np.complex64)[..., 0], w.astype(np.complex64))
    seen = new_seen()
    for b in range(shape[0]):
        check_update(X[b], w0[b], V[b], Cx[b], w[b], model, seen)
    print(f"five update {fo.case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in seen.items()))
    assert seen["norm"] <= TOL_P and seen["residual"] <= TOL_P and seen["rho"] <= TOL_P, seen
    assert seen["margin"] <= 1.0, seen


@pytest.mark.parametrize("case", fo.CASES, ids=fo.case_id)
def test_every_iterate_follows_from_the_device_s_own_v(case):
    """ten iterations stage by stage: every update is held to the bounds of the test above on the V the device formed for it, so
    an iterated run can leave the float64 restatement only through the stages in front of the update"""
    shape, model = case
    X = fo.rooms(shape)
    seen = new_seen()
    with open_plan(X, model) as plan:
        Cx = plan.get_cx()
        w = plan.get_w(np.complex128)[..., 0]
        for _ in range(10):
            w_prev = w
            for s in ("power", "activation", "cov"):
                plan.five_stage(s)
            V = plan.get_weighted_cov()[:, :, 0]
            plan.five_stage("update")
            w = plan.get_w(np.complex128)[..., 0]
            for b in range(shape[0]):
                check_update(X[b], w_prev[b], V[b], Cx[b], w[b], model, seen)
    print(f"five ten updates {fo.case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in seen.items()))
    assert seen["norm"] <= TOL_P and seen["residual"] <= TOL_P and seen["rho"] <= TOL_P, seen
    assert seen["margin"] <= 1.0, seen


# ---- 3. iterated -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.CASES, ids=fo.case_id)
def test_iterated_against_the_restatement(case):
    """1, 3 and 10 iterations of five_iterate from the device's own start: w (phase-free) and the projected-back Y against the
    restatement run from that start, each under the case's yardstick at that iteration count (10 times the larger of the distance
    between the restatement's two formulations and its move under a 1e-13 relative change of X).  Y is asked for in complex128: the plan then forms it in
    float64 from the widened X (the complex64 Y of the same W carries float32's 6e-8 and is held to that in the public calls)"""
    shape, model = case
    X = fo.rooms(shape)
    got = {}
    with open_plan(X, model) as plan:
        w0 = plan.get_w(np.complex128)[..., 0]
        done = 0
        for n in fo.ITER_COUNTS:
            plan.five_iterate(n - done)
            done = n
            got[n] = (plan.get_w(np.complex128)[..., 0], plan.demix(True, np.complex128)[..., 0])
    worst = {}
    for b in range(shape[0]):
        ref = fo.yardstick(X[b], w0[b], model)
        assert ref["min_gap"] >= fo.MIN_GAP, ref["min_gap"]
        for n in fo.ITER_COUNTS:
            d_w, d_y = fo.wdist(got[n][0][b], ref[n]["w"]), fo.dist(got[n][1][b], ref[n]["y"])
            print(f"five iterated {fo.case_id(case)} room {b} n = {n}: w {d_w:.2e} (yardstick {ref[n]['tol_w']:.2e}), "
                  f"Y {d_y:.2e} (yardstick {ref[n]['tol_y']:.2e})")
            worst[n] = max(worst.get(n, 0.0), d_w / ref[n]["tol_w"], d_y / ref[n]["tol_y"])
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 4. a room's bits do not depend on the batch ---------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch():
    """room b of a dense batch, of the batch in another order, of the ragged batch (in two orders) and alone: W and Y equal bit
    for bit"""
    import overiva_amd as oa

    n = 3
    dense = fo.rooms((3, fo.RAGGED_FRAMES[0], fo.RAGGED_F, fo.RAGGED_M))
    ragged = fo.ragged_rooms()
    assert np.array_equal(dense[0], ragged[0])
    alone = [oa.five_batch(x[None], n_iter=n, return_filters=True) for x in list(dense) + ragged[1:]]
    Yd, Wd = oa.five_batch(dense, n_iter=n, return_filters=True)
    Yp, Wp = oa.five_batch(dense[::-1], n_iter=n, return_filters=True)
    for b in range(3):
        for Y, W in ((Yd[b], Wd[b]), (Yp[2 - b], Wp[2 - b])):
            assert np.array_equal(Y, alone[b][0][0]) and np.array_equal(W, alone[b][1][0])
    ref = [alone[0]] + alone[3:]
    order = [2, 0, 3, 1]
    Yr, Wr = oa.five_batch(ragged, n_iter=n, return_filters=True)
    Yq, Wq = oa.five_batch([ragged[i] for i in order], n_iter=n, return_filters=True)
    for b in range(4):
        assert np.array_equal(Yr[b], ref[b][0][0]) and np.array_equal(Wr[b], ref[b][1][0])
        assert np.array_equal(Yq[b], ref[order[b]][0][0]) and np.array_equal(Wq[b], ref[order[b]][1][0])
    assert all(np.all(np.isfinite(a[1])) for a in alone)


# ---- 5. the public calls ---------------------------------------------------------------------------------------------------------
def test_five_is_five_batch_of_one_room():
    import overiva_amd as oa

    T, F, M = 70, 17, 3
    X = fo.rooms((1, T, F, M))[0]
    one = oa.five(X, n_iter=4, return_filters=True)
    bat = oa.five_batch(X[None], n_iter=4, return_filters=True)
    assert one[0].shape == (T, F, 1) and one[0].dtype == np.complex64 and one[1].shape == (F, M, 1)
    assert bat[0].shape == (1, T, F, 1) and bat[1].shape == (1, F, M, 1)
    assert np.array_equal(one[0], bat[0][0]) and np.array_equal(one[1], bat[1][0])
    assert np.array_equal(oa.five(X, n_iter=4), one[0])                         # Y alone
    assert np.array_equal(oa.five(X, n_iter=4, n_src=1), one[0])
    info = oa.last_batch_info()
    assert info["algorithm"] == "five" and info["batched"] == 1 and info["shape"] == (T, F, M, 1)
    # the default start is the plan's eigenvector start; the identity column and a W0 are the other two
    with open_plan(X[None]) as plan:
        plan.five_iterate(4)
        assert np.array_equal(plan.get_w(np.complex64)[0], one[1]) and np.array_equal(plan.demix(True)[0], one[0])
    e0 = np.zeros((F, M, 1))
    e0[:, 0, 0] = 1.0
    Yi = oa.five(X, n_iter=1, init_eig=False)
    assert np.array_equal(Yi, oa.five(X, n_iter=1, W0=e0))
    assert not np.array_equal(Yi, oa.five(X, n_iter=1))
    # complex128 in, complex128 out
    Y128, W128 = oa.five_batch(X[None].astype(np.complex128), n_iter=4, return_filters=True)
    assert Y128.dtype == W128.dtype == np.complex128 and np.array_equal(W128.astype(np.complex64), bat[1])
    # (complex128 out is formed in float64 from the same w; the complex64 Y carries float32's rounding)
    assert fo.dist(bat[0].astype(np.complex128), Y128) <= 1e-5 and not np.array_equal(Y128, bat[0].astype(np.complex128))


def test_a_list_of_rooms_returns_a_list():
    import overiva_amd as oa

    Xs = fo.ragged_rooms()
    Ys, W = oa.five_batch(Xs, n_iter=3, return_filters=True)
    assert isinstance(Ys, list) and [y.shape for y in Ys] == [x.shape[:2] + (1,) for x in Xs] and W.shape == (4, fo.RAGGED_F, fo.RAGGED_M, 1)
    info = oa.last_batch_info()
    assert info["algorithm"] == "five" and info["ragged"] and info["frames"] == list(fo.RAGGED_FRAMES)


def test_callback_epochs():
    import overiva_amd as oa

    B, T, F, M = 2, 70, 17, 2
    X = fo.rooms((B, T, F, M))
    got = []
    Y = oa.five_batch(X, n_iter=12, callback=lambda Y: got.append(Y.copy()))
    assert len(got) == 2 and all(g.shape == (B, T, F, 1) for g in got)          # epochs 0 and 10
    assert np.array_equal(got[0], oa.five_batch(X, n_iter=0))
    assert np.array_equal(got[1], oa.five_batch(X, n_iter=10))
    assert np.array_equal(Y, oa.five_batch(X, n_iter=12))                       # the callback does not change the result


def _audio(seed, n, M):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 64 + 1, M)), 64, axis=0)[:n]
    A = rng.standard_normal((M, M)) + 2 * np.eye(M)
    return ((env * rng.standard_normal((n, M))) @ A.T).astype(np.float32)


def test_separate_batch_is_the_composed_path():
    """separate_batch(algorithm="five") against stft.analysis -> five_batch on the list -> stft.synthesis per room, bit for bit,
    on two rooms of different lengths with 64-sample frames"""
    import overiva_amd as oa
    from overiva_amd import stft

    L, HOP, M = 64, 32, 3
    wa = stft.hann(L)
    ws = stft.compute_synthesis_window(wa, HOP)
    xs = [_audio(3, 4096, M), _audio(4, 2777, M)]
    Xc = [stft.analysis(x, L, HOP, win=wa) for x in xs]
    Yc, Wc = oa.five_batch(Xc, n_iter=5, init_eig=True, return_filters=True)
    yc = [stft.synthesis(Y, L, HOP, win=ws) for Y in Yc]
    yb, Wb = oa.separate_batch(xs, L, HOP, n_iter=5, algorithm="five", init_eig=True, return_filters=True)
    assert oa.last_batch_info()["algorithm"] == "five"
    assert np.array_equal(Wb.astype(np.complex64), Wc)
    for a, b in zip(yb, yc):
        assert a.shape == b.shape and a.shape[1] == 1 and np.array_equal(a, b)


def test_refusals_of_the_plan():
    """K != 1, complex128 data, every entry before begin, a stage that does not exist"""
    import overiva_amd as oa

    X = fo.rooms((1, 33, 5, 3))
    with oa.BatchPlan(1, 33, 5, 3, 2) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w()
        with pytest.raises(ValueError, match="one source"):
            plan.five_begin()
    with oa.BatchPlan(1, 33, 5, 3, 1, data="complex128") as plan:
        with pytest.raises(ValueError, match="complex128"):
            plan.five_begin()
    with oa.BatchPlan(1, 33, 5, 3, 1) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w()
        for call in (lambda: plan.five_iterate(1), lambda: plan.five_stage("update"), plan.get_five_reduction):
            with pytest.raises(RuntimeError, match="five_begin"):
                call()
        plan.five_begin()
        with pytest.raises(ValueError):
            plan.five_stage(4)
        plan.covariance()                    # a new Cx: the reduction is of the old one
        with pytest.raises(RuntimeError, match="five_begin"):
            plan.five_iterate(1)


# ---- 6. a bad room ---------------------------------------------------------------------------------------------------------------
def test_a_singular_room_is_named_and_leaves_the_others_alone():
    """room 1 has an all-zero channel, so its Cx is singular: it ends non-finite and status() names it; the other rooms keep the
    bits of a batch without it"""
    B, T, F, M = 3, 70, 17, 3
    X = fo.rooms((B, T, F, M))
    X[1, :, :, 2] = 0
    with open_plan(X) as plan:
        plan.five_iterate(3)
        bad = plan.status()
        W = plan.get_w(np.complex128, check=False)
        with pytest.raises(np.linalg.LinAlgError, match="1"):
            plan.get_w(np.complex128)
    print(f"five singular room: status {bad.tolist()}, room 1 finite {bool(np.all(np.isfinite(W[1])))}")
    assert not bad[0] and not bad[2] and bad[1] and not np.all(np.isfinite(W[1]))
    keep = [0, 2]
    with open_plan(X[keep]) as plan:
        plan.five_iterate(3)
        Wk = plan.get_w(np.complex128)
    assert np.all(np.isfinite(Wk)) and np.array_equal(W[keep], Wk)


# ---- 7. it extracts a source -----------------------------------------------------------------------------------------------------
def test_it_extracts_the_super_gaussian_source():
    """one super-Gaussian source (a shared frame envelope) in a Gaussian background of the same power at 4 microphones: after 10
    iterations the output correlates better with the source's image at channel 0 than channel 0 itself does"""
    import overiva_amd as oa

    T, F, M = 300, 16, 4
    rng = np.random.default_rng(5)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    env = rng.gamma(0.3, 1.0, (T, 1))
    s = env / np.sqrt(np.mean(env ** 2)) * cn(T, F)
    a = cn(F, M)
    image = s[:, :, None] * a[None]
    Hn = cn(F, M, M)
    noise = np.einsum("fmn,tfn->tfm", Hn, cn(T, F, M)) / np.sqrt(M)
    X = (image + noise).astype(np.complex64)
    Y = oa.five(X, n_iter=10)[:, :, 0]

    def corr(y):
        return float(np.abs(np.vdot(image[:, :, 0], y)) / (np.linalg.norm(image[:, :, 0]) * np.linalg.norm(y)))

    print(f"five extraction: correlation with the source image {corr(Y):.3f}, of channel 0 {corr(X[:, :, 0]):.3f}")
    assert corr(Y) > corr(X[:, :, 0])
