"""auxiva_iss_batch() / auxiva_iss() on the GPU: every stage against the NumPy restatement
(tests/helpers/iss_oracle.py) from a known state, a room with an all-zero channel, iterated results where the restatement is
itself reproducible, the cost along the device path, bits that do not depend on the batch, and the public calls.

Every figure is printed before it is asserted (DESIGN.md 3.15 has the measured ones).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import iss_oracle as iso  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12        # float64 stages, of the largest entry: the bound test_ilrma_gpu.py holds them to
TOL_P = 1e-10      # the two defining properties of a rank-1 step


def dist(a, b):
    """maximum absolute difference over the maximum magnitude"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def rooms(kind, B, T, F, M, seed=iso.SEED):
    return np.stack([iso.make_x(kind, T, F, M, seed=seed + b) for b in range(B)])


def random_w0(B, F, M, seed):
    """well conditioned: the identity plus a small complex perturbation"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, F, M, M)) + 1j * rng.standard_normal((B, F, M, M))
    return np.eye(M)[None, None] + 0.3 / np.sqrt(M) * g


def open_plan(X, W0=None, model="laplace"):
    """a plan with ISS begun on X: (B, T, F, M), or a list of (T_b, F, M) rooms"""
    from overiva_amd import BatchPlan, RaggedBatchPlan

    if isinstance(X, list):
        F, M = X[0].shape[1:]
        plan = RaggedBatchPlan([x.shape[0] for x in X], F, M, M, model)
    else:
        B, T, F, M = X.shape
        plan = BatchPlan(B, T, F, M, M, model)
    plan.set_x(X)
    plan.covariance()
    plan.set_w(W0)
    plan.iss_begin()
    return plan


def run_device(X, n, model="laplace", W0=None):
    """n iterations through the plan: (W complex128, Y complex64 without projection back)"""
    with open_plan(X, W0, model) as plan:
        plan.iss_iterate(n)
        return plan.get_w(np.complex128), plan.demix(False)


# ---- 1. one stage at a time from a known state ---------------------------------------------------------------------------------
# (B, T, F, M): the frame stride of 64 below, at and above a multiple; bin groups that end inside F (17 = 2 x 8 + 1, 65, 9, 33, 20),
# one bin, every channel instantiation, two rooms of T = 257, and the LDS limit T M = 8192 with one bin per group
STAGE_SHAPES = [((3, 70, 17, 2), m) for m in iso.MODELS] + [((2, 33, 65, 3), m) for m in iso.MODELS] \
    + [((2, 64, 1, 5), m) for m in iso.MODELS] + [((1, 65, 5, 1), m) for m in iso.MODELS] + [((2, 128, 9, 4), m) for m in iso.MODELS] \
    + [((1, 130, 33, 6), m) for m in iso.MODELS] + [((1, 100, 20, 7), m) for m in iso.MODELS] + [((2, 257, 20, 8), m) for m in iso.MODELS] \
    + [((1, 1024, 3, 8), "laplace")]


@pytest.mark.parametrize("shape,model", STAGE_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_stages_against_numpy(shape, model):
    """p of the head-only pass, phi, the scaled W, then W after 1, 2, ..., M steps, each from the state the device itself holds
    (its scaled W and its phi); after every step the two properties in NumPy from get_w and X"""
    B, T, F, M = shape
    X = rooms("mix", B, T, F, M)
    X128 = X.astype(np.complex128)
    W0 = random_w0(B, F, M, seed=3)
    seen = {}

    def check(name, dev, ref):
        seen[name] = max(seen.get(name, 0.0), dist(dev, ref))

    with open_plan(X, W0, model) as plan:
        p = np.stack([iso.powers(iso.demix(X128[b], W0[b])) for b in range(B)])
        check("p head", plan.get_iss_powers(), p)
        plan.iss_stage("activation")
        act = [iso.activation(p[b], F, model) for b in range(B)]
        check("phi", plan.get_iss_weights(), np.stack([a[0] for a in act]))
        Wa = plan.get_w(np.complex128)
        check("W scaled", Wa, np.stack([W0[b] / act[b][1][None, None, :] for b in range(B)]))
        phi = plan.get_iss_weights()                                   # the known state of the sweep: the device's own
        Y = np.stack([iso.demix(X128[b], Wa[b]) for b in range(B)])
        Wref = Wa.copy()
        worst_orth = worst_norm = 0.0
        for n in range(1, M + 1):
            k = n - 1
            yk = Y[:, :, :, k].copy()
            for b in range(B):
                iso.step(Y[b], Wref[b], phi[b], k)
            plan.set_w(Wa)
            plan.iss_sweep_steps(n)
            Wn = plan.get_w(np.complex128)
            check(f"W after {n}", Wn, Wref)
            # the properties of step k, from the device's W: y' = X conj(W_n), y_k the channel before the step
            Yn = np.stack([iso.demix(X128[b], Wn[b]) for b in range(B)])
            d = np.einsum("btm,btf->bfm", phi, yk.real ** 2 + yk.imag ** 2)
            c = np.abs(np.einsum("btm,btfm,btf->bfm", phi, Yn, np.conj(yk)))
            nn = np.einsum("btm,btfm->bfm", phi, Yn.real ** 2 + Yn.imag ** 2)
            orth = np.delete(c / np.sqrt(nn * d), k, axis=2)
            worst_orth = max(worst_orth, float(orth.max()) if orth.size else 0.0)
            worst_norm = max(worst_norm, float(np.max(np.abs(nn[:, :, k] / T - 1.0))))
        check("p swept", plan.get_iss_powers(), np.stack([iso.powers(Y[b]) for b in range(B)]))
        # the complex64 copy the output path reads is the rounded W
        assert np.array_equal(plan.get_w(np.complex64), Wn.astype(np.complex64))
    seen["orthogonality"], seen["normalisation"] = worst_orth, worst_norm
    print(f"iss stages {shape} {model}: " + ", ".join(f"{k} {v:.2e}" for k, v in seen.items()))
    for name, v in seen.items():
        assert v <= (TOL_P if name in ("orthogonality", "normalisation") else TOL), (name, v)


def test_a_zero_channel_takes_the_zero_branch_and_leaves_the_others_alone():
    """room 1 has an all-zero channel: its d_m are zero (or not a number) and v = 0 there; the room ends finite or is named by
    status(), and the other rooms have the bits of a batch without it"""
    B, T, F, M = 3, 70, 17, 3
    X = rooms("mix", B, T, F, M)
    X[1, :, :, 2] = 0
    with open_plan(X) as plan:
        plan.iss_iterate(3)
        bad = plan.status()
        W = plan.get_w(np.complex128, check=False)
    print(f"iss zero channel: status {bad.tolist()}, room 1 finite {bool(np.all(np.isfinite(W[1])))}")
    assert not bad[0] and not bad[2]
    assert bool(bad[1]) != bool(np.all(np.isfinite(W[1])))
    keep = [0, 2]
    Wk, _ = run_device(X[keep], 3)
    assert np.all(np.isfinite(Wk)) and np.array_equal(W[keep], Wk)
    # a zero channel that meets finite weights: one step from a known state
    Xz = rooms("mix", 1, T, F, M)
    with open_plan(Xz) as plan:
        plan.iss_stage("activation")
        Wa = plan.get_w(np.complex128)
        Wz = Wa.copy()
        Wz[:, :, :, 1] = 0                    # y_1 = 0: d_m = 0 for every m in step 1
        plan.set_w(Wz)
        plan.iss_sweep_steps(2)
        W2 = plan.get_w(np.complex128)
        plan.set_w(Wz)
        plan.iss_sweep_steps(1)
        W1 = plan.get_w(np.complex128)
    assert np.all(np.isfinite(W2)) and np.array_equal(W1, W2)      # step 1 changed nothing


# ---- 2. iterated results, where the oracle is reproducible -----------------------------------------------------------------------
@pytest.mark.parametrize("case", iso.ITERATED, ids=iso.case_id)
def test_iterated_parity(case):
    """delta: how far a 1e-13 relative perturbation of X moves the oracle's own W.  The device, whose sums round in another order,
    must stay within 10 delta after 1, 5 and 20 iterations: W, and Y = X conj(W) with and without projection back (formed in
    float64 from the device's W: the batch's own output path demixes in float32, checked against the same Y at float32's bound
    and bit for bit against a plan of that W in test_the_output_path_is_the_batch_s_own).  complex64 and complex128 input give
    the same W."""
    import overiva_amd as oa

    kind, (T, F, M), model = case
    o = iso.oracle_run(case)
    X = o["X"]
    X128 = X.astype(np.complex128)
    done = 0
    with open_plan(X[None], None, model) as plan:
        for n in iso.ITER_COUNTS:
            delta = o[n]["delta"]
            assert 10 * delta <= 1e-8, delta          # (asserted for every case by test_iss_host.py: nothing is skipped)
            plan.iss_iterate(n - done)
            done = n
            W = plan.get_w(np.complex128)[0]
            dW = iso.rel(W, o[n]["W"])
            Yd, Yo = iso.demix(X128, W), iso.demix(X128, o[n]["W"])
            dY, dYp = iso.rel(Yd, Yo), iso.rel(iso.projected(X128, Yd), iso.projected(X128, Yo))
            Y32 = plan.demix(False)[0]
            # float32's bound: with S = sum_m |x_m| |w_m| and u = 2^-24, either part of y is a sum of 2 M products (error
            # <= 2 M u S in any order), of a W rounded to complex64 (u S) and is rounded once more (u S); the two parts together
            # sqrt(2) times that; one more u S for the second-order terms
            room = np.sqrt(2.0) * (2 * M + 3) * 2.0 ** -24 * np.einsum("tfm,fmk->tfk", np.abs(X128), np.abs(W))
            over = float(np.max(np.abs(Y32 - Yd) / room))
            print(f"iss iterated {iso.case_id(case)} n={n}: delta {delta:.2e} device W {dW:.2e} Y {dY:.2e} Y projected {dYp:.2e}; "
                  f"float32 output over its bound {over:.2f}")
            assert dW <= 10 * delta and dY <= 10 * delta and dYp <= 10 * delta
            assert over <= 1.0
            if n == 5:
                W5 = W
    a = oa.auxiva_iss_batch(X[None], n_iter=5, model=model, return_filters=True)
    b = oa.auxiva_iss_batch(X128[None], n_iter=5, model=model, return_filters=True)
    assert a[1].dtype == np.complex64 and b[1].dtype == np.complex128 and b[0].dtype == np.complex128
    assert np.array_equal(b[1][0], W5) and np.array_equal(a[1][0], W5.astype(np.complex64))
    assert np.array_equal(a[0], b[0].astype(np.complex64))


# ---- 3. the cost along the device path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", iso.COST_CASES, ids=iso.case_id)
def test_cost_does_not_rise_across_a_sweep_on_the_device(case):
    """20 iterations stage by stage; J in NumPy from get_w after the activation and after the sweep: no sweep raises it by more
    than 1e-12 of |J| at its start"""
    kind, (B, T, F, M), model = case
    X = rooms(kind, B, T, F, M)

    def cost(plan):
        W = plan.get_w(np.complex128)
        return np.array([iso.cost(X[b], W[b], model) for b in range(B)])

    rise, first = -np.inf, None
    with open_plan(X, None, model) as plan:
        for _ in range(20):
            plan.iss_stage("activation")
            before = cost(plan)
            first = before if first is None else first          # (J at the start of the first sweep, as the host test takes it)
            plan.iss_stage("sweep")
            after = cost(plan)
            rise = max(rise, float(((after - before) / np.abs(before)).max()))
    print(f"iss cost {iso.case_id(case)}: largest relative rise across a sweep {rise:.2e}, J {first} -> {after}")
    assert np.all(np.isfinite(after)) and np.all(after < first)
    assert rise <= 1e-12


# ---- 4. bits do not depend on the batch ------------------------------------------------------------------------------------------
BITS = [(F, M, model) for F in (17, 65) for M in (2, 3, 8) for model in iso.MODELS]


@pytest.mark.parametrize("F,M,model", BITS, ids=lambda v: str(v))
def test_bits_do_not_depend_on_the_batch(F, M, model):
    B, T = 5, 70
    X = rooms("mix", B, T, F, M)
    full = run_device(X, 5, model)
    perm = [3, 0, 4, 2, 1]
    shuffled = run_device(X[perm], 5, model)
    for b in range(B):
        alone = run_device(X[b:b + 1], 5, model)
        for name, a, f, p in zip(("W", "Y"), alone, full, shuffled):
            assert np.all(np.isfinite(a)), name
            assert np.array_equal(a[0], f[b]), (name, b)
            assert np.array_equal(a[0], p[perm.index(b)]), (name, b)


@pytest.mark.parametrize("F,M,model", BITS, ids=lambda v: str(v))
def test_rooms_of_different_lengths_have_the_bits_of_a_batch_of_one(F, M, model):
    lengths = [16, 63, 64, 65, 147, 168, 257]
    Xs = [iso.make_x("mix", T, F, M, seed=iso.SEED + b) for b, T in enumerate(lengths)]
    W, Ys = run_device(Xs, 5, model)
    for b, x in enumerate(Xs):
        Wb, Yb = run_device(x[None], 5, model)
        assert np.all(np.isfinite(Wb))
        assert np.array_equal(Wb[0], W[b]) and np.array_equal(Yb[0], Ys[b]), b


# ---- 5. the public calls ---------------------------------------------------------------------------------------------------------
def test_auxiva_iss_is_auxiva_iss_batch_of_one_room():
    import overiva_amd as oa

    T, F, M = 70, 17, 3
    X = iso.make_x("mix", T, F, M)
    one = oa.auxiva_iss(X, n_iter=4, return_filters=True)
    bat = oa.auxiva_iss_batch(X[None], n_iter=4, return_filters=True)
    assert one[0].shape == (T, F, M) and one[0].dtype == np.complex64 and one[1].shape == (F, M, M)
    assert np.array_equal(one[0], bat[0][0]) and np.array_equal(one[1], bat[1][0])
    assert np.array_equal(oa.auxiva_iss(X, n_iter=4), one[0])                    # Y alone
    assert np.array_equal(oa.auxiva_iss(X, n_src=M, n_iter=4), one[0])
    # W0 given as the identity is the default
    eye = np.tile(np.eye(M), (F, 1, 1))
    assert np.array_equal(oa.auxiva_iss(X, n_iter=4, W0=eye), one[0])
    assert np.array_equal(oa.auxiva_iss_batch(X[None], n_iter=4, W0=eye[None]), bat[0])
    info = oa.last_batch_info()
    assert info["algorithm"] == "auxiva_iss" and info["batched"] == 1
    assert info["precision"] == "precise" and info["shape"] == (T, F, M, M)
    # the eigenvector start is the plan's
    Ye, We = oa.auxiva_iss(X, n_iter=2, init_eig=True, return_filters=True)
    with oa.BatchPlan(1, T, F, M, M) as plan:
        plan.set_x(X[None])
        plan.covariance()
        plan.set_w_eig()
        plan.iss_begin()
        plan.iss_iterate(2)
        assert np.array_equal(plan.get_w(np.complex64)[0], We) and np.array_equal(plan.demix(True)[0], Ye)
    assert not np.array_equal(Ye, oa.auxiva_iss(X, n_iter=2))


def test_a_list_of_rooms_returns_a_list():
    import overiva_amd as oa

    Xs = [iso.make_x("mix", T, 17, 2, seed=iso.SEED + b) for b, T in enumerate((40, 70, 33))]
    Ys, W = oa.auxiva_iss_batch(Xs, n_iter=3, return_filters=True)
    assert isinstance(Ys, list) and [y.shape for y in Ys] == [x.shape for x in Xs] and W.shape == (3, 17, 2, 2)
    info = oa.last_batch_info()
    assert info["algorithm"] == "auxiva_iss" and info["ragged"] and info["frames"] == [40, 70, 33]
    for b, x in enumerate(Xs):
        Yb, Wb = oa.auxiva_iss_batch(x[None], n_iter=3, return_filters=True)
        assert np.array_equal(Yb[0], Ys[b]) and np.array_equal(Wb[0], W[b])


def test_callback_epochs():
    import overiva_amd as oa

    B, T, F, M = 2, 70, 17, 2
    X = rooms("iid", B, T, F, M)
    got = []
    Y = oa.auxiva_iss_batch(X, n_iter=22, callback=lambda Y: got.append(Y.copy()))
    assert len(got) == 3 and all(g.shape == (B, T, F, M) for g in got)          # epochs 0, 10 and 20
    assert np.array_equal(got[0], oa.auxiva_iss_batch(X, n_iter=0))
    assert np.array_equal(got[1], oa.auxiva_iss_batch(X, n_iter=10))
    assert np.array_equal(got[2], oa.auxiva_iss_batch(X, n_iter=20))
    assert np.array_equal(Y, oa.auxiva_iss_batch(X, n_iter=22))                 # the callback does not change the result


def test_the_output_path_is_the_batch_s_own():
    import overiva_amd as oa

    B, T, F, M = 2, 70, 17, 3
    X = rooms("mix", B, T, F, M).astype(np.complex128)          # complex128 in: W comes back in complex128
    Y0, W = oa.auxiva_iss_batch(X, n_iter=3, proj_back=False, return_filters=True)
    Y1 = oa.auxiva_iss_batch(X, n_iter=3, proj_back=True)
    assert Y0.dtype == Y1.dtype == W.dtype == np.complex128
    with oa.BatchPlan(B, T, F, M, M) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(W)
        assert np.array_equal(plan.demix(False, np.complex128), Y0)
        assert np.array_equal(plan.demix(True, np.complex128), Y1)
    assert not np.array_equal(Y0, Y1)


def _audio(seed, n, M):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 512 + 1, M)), 512, axis=0)[:n]
    A = rng.standard_normal((M, M)) + 2 * np.eye(M)
    return ((env * rng.standard_normal((n, M))) @ A.T).astype(np.float32)


def test_separate_batch_is_the_composed_path():
    """separate_batch(algorithm="auxiva_iss") against stft.analysis -> auxiva_iss_batch -> stft.synthesis per room, bit for bit,
    for an array and for a list of rooms"""
    import overiva_amd as oa
    from overiva_amd import stft

    L, HOP, M = 512, 256, 4                   # the transform of test_separate_gpu.test_agreement_with_the_composed_path
    wa = stft.hann(L)
    ws = stft.compute_synthesis_window(wa, HOP)
    for xs in (np.stack([_audio(s, 25600, M) for s in (1, 2)]), [_audio(s, n, M) for s, n in ((3, 25600), (4, 17741), (5, 38400))]):
        Xc = [stft.analysis(x, L, HOP, win=wa) for x in xs]
        Yc, Wc = oa.auxiva_iss_batch(Xc if isinstance(xs, list) else np.stack(Xc), n_iter=6, return_filters=True)
        yc = [stft.synthesis(Y, L, HOP, win=ws) for Y in Yc]
        yb, Wb = oa.separate_batch(xs, L, HOP, n_iter=6, algorithm="auxiva_iss", return_filters=True)
        assert oa.last_batch_info()["algorithm"] == "auxiva_iss"
        assert np.array_equal(Wb.astype(np.complex64), Wc)
        for a, b in zip(yb, yc):
            assert a.shape == b.shape and np.array_equal(a, b)


def test_refusals_of_the_c_entries():
    """K != M, complex128 data, T M over the limit, and every entry before begin"""
    import ctypes

    import overiva_amd as oa
    from overiva_amd import _lib

    lib = _lib.load()
    X = rooms("iid", 1, 20, 5, 3)
    out = (ctypes.c_double * 4096)()
    with oa.BatchPlan(1, 20, 5, 3, 2) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(None)
        with pytest.raises(ValueError, match="K = M"):
            plan.iss_begin()
    with oa.BatchPlan(1, 20, 5, 3, 3, data="complex128") as plan:
        assert lib.oiva_batch_iss_begin(plan.h) == _lib.ERR_ARG and b"complex128" in lib.oiva_last_error()
        with pytest.raises(ValueError, match="complex128"):
            plan.iss_begin()
    with oa.BatchPlan(1, 1025, 2, 8, 8) as plan:
        assert lib.oiva_batch_iss_begin(plan.h) == _lib.ERR_ARG and b"8192" in lib.oiva_last_error()
    with oa.RaggedBatchPlan([16, 2734], 2, 3, 3) as plan:
        assert lib.oiva_batch_iss_begin(plan.h) == _lib.ERR_ARG and b"8192" in lib.oiva_last_error()
    with oa.BatchPlan(1, 20, 5, 3, 3) as plan:
        assert lib.oiva_batch_iss_begin(plan.h) == _lib.ERR_STATE              # X not set
        plan.set_x(X)
        plan.covariance()
        plan.set_w(None)
        for call in (lambda: lib.oiva_batch_iss_stage(plan.h, 0), lambda: lib.oiva_batch_iss_stage(plan.h, 1),
                     lambda: lib.oiva_batch_iss_iterate(plan.h, 1), lambda: lib.oiva_batch_iss_sweep_steps(plan.h, 1),
                     lambda: lib.oiva_batch_iss_get_weights(plan.h, out), lambda: lib.oiva_batch_iss_get_powers(plan.h, out),
                     lambda: lib.oiva_batch_iss_time_stages(plan.h, 1, (ctypes.c_float * 2)())):
            assert call() == _lib.ERR_STATE
        with pytest.raises(RuntimeError, match="iss_begin"):
            plan.iss_iterate(1)
        plan.iss_begin()
        assert lib.oiva_batch_iss_stage(plan.h, 2) == _lib.ERR_ARG
        assert lib.oiva_batch_iss_sweep_steps(plan.h, 4) == _lib.ERR_ARG
        plan.iss_iterate(1)
        ms = plan.iss_time_stages(1)
        assert set(ms) == {"activation", "sweep"} and all(v > 0 for v in ms.values())
        assert np.all(np.isfinite(plan.get_w()))
        plan.set_x(X)                                                           # new X: begin again
        assert lib.oiva_batch_iss_iterate(plan.h, 1) == _lib.ERR_STATE
