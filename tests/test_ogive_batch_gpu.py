"""ogive_batch() on the GPU: parity with the real reference (tests/golden/ogive_batch.npz), the same result as one ogive() call
per problem, a stopping rule per problem, bit-for-bit independence of a problem's result from the batch around it, isolation of
a non-finite problem, and one batch of the reference's own size."""
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ogive_batch.npz")
TOL = 1e-5
SAME = 1e-9          # batched against single calls (both `precise`)
AMP_LIMIT = 1e3      # as conftest.chaotic


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _single(oa, X, **kw):
    oa.set_precision("precise")
    try:
        return oa.ogive(X, **kw)
    finally:
        oa.set_precision("auto")


def _max_delta_series(oa, X, n, update="demix", model="laplace", step_size=0.1):
    """max ||delta|| of every epoch of the single-problem plan (precise), tol = 0"""
    T, F, M = X.shape
    out = []
    with oa.Plan(T, F, M, 1, model) as p:
        p.set_precision("precise")
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.ogive_begin(update, model)
        for e in range(n):
            out.append(p.ogive_iterate(e, 1, step_size, 0.0)[2])
    return np.array(out)


def _mix(T, F, M, seed):
    return orc.synth_mixture(T, F, M, 1, seed=seed)


# ---- 1. reference parity ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as d:
        g = {k: d[k] for k in d.files}
    T, F, M, S = (int(g[k]) for k in ("T", "F", "M", "S"))
    X = np.stack([orc.synth_iid(T, F, M, seed=int(s)) if fam == "iid" else orc.synth_mixture(T, F, M, S, seed=int(s))
                  for fam, s in zip(g["family"], g["seed"])])
    assert np.allclose([x.astype(np.complex128).sum() for x in X], g["X_sum"], rtol=0, atol=1e-9)
    return g, X.astype(np.complex128)


@pytest.mark.parametrize("update", ["demix", "mix", "switching"])
@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_ogive_batch_reference_parity(oa, gold, update, model):
    g, X = gold
    key = f"{update}_{model}"
    n = int(g["n_iter"])
    Y, w = oa.ogive_batch(X, n_iter=n, tol=0.0, update=update, model=model, proj_back=False, return_filters=True)
    assert Y.dtype == np.complex128 and w.shape == g[f"W_{key}"].shape
    assert oa.last_batch_info()["epochs"] == [n] * len(X)
    checked = 0
    for b in range(len(X)):
        amp = float(g[f"amp_{key}"][b])
        if amp > AMP_LIMIT:          # the reference itself is chaotic here: finite and equal to the problem run alone
            w1 = oa.ogive_batch(X[b:b + 1], n_iter=n, tol=0.0, update=update, model=model, proj_back=False, return_filters=True)[1]
            assert np.all(np.isfinite(w[b])) and np.array_equal(w1[0], w[b])
            continue
        floor = float(np.nan_to_num(g[f"floor_{key}"][b]))
        e = orc.rel_err(w[b], g[f"W_{key}"][b])
        assert e < max(TOL * max(1.0, amp / 10.0), 0.1 * floor), (b, e, amp, floor)
        checked += 1
    assert checked >= 2


def test_ogive_batch_reference_early_stop(oa, gold):
    g, X = gold
    _, w = oa.ogive_batch(X, n_iter=int(g["stop_n_iter"]), tol=float(g["stop_tol"]), proj_back=False, return_filters=True)
    info = oa.last_batch_info()
    assert info["epochs"] == g["stop_epochs"].tolist()
    assert info["converged"] == [int(e) < int(g["stop_n_iter"]) for e in g["stop_epochs"]]
    for b in range(len(X)):
        assert orc.rel_err(w[b], g["W_stop"][b]) < TOL * max(1.0, float(g["amp_stop"][b]) / 10.0)


# ---- 2. the same result as one ogive() call per problem --------------------------------------------------------------------
W0_MODES = ("identity", "shared", "per_problem", "init_eig")


def _sweep():
    out = []
    i = 0
    for M in range(1, 9):
        for update in ("demix", "mix", "switching"):
            out.append((M, update, ("laplace", "gauss")[i % 2], W0_MODES[i % 4], (np.complex64, np.complex128)[(i // 2) % 2]))
            i += 1
    return out


@pytest.mark.parametrize("M, update, model, w0, dtype", _sweep(), ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_ogive_batch_matches_single_calls(oa, M, update, model, w0, dtype):
    B, T, F, n = 3, 80, 37, 120
    X = np.stack([orc.synth_iid(T, F, M, seed=300 * M + b) for b in range(B)]).astype(dtype)
    rng = np.random.default_rng(M)
    W0 = None
    if w0 == "shared":
        W0 = np.eye(M, 1)[None] + 0.1 * (rng.standard_normal((F, M, 1)) + 1j * rng.standard_normal((F, M, 1)))
    elif w0 == "per_problem":
        W0 = np.eye(M, 1)[None, None] + 0.1 * (rng.standard_normal((B, F, M, 1)) + 1j * rng.standard_normal((B, F, M, 1)))
    kw = dict(n_iter=n, tol=0.0, update=update, model=model, init_eig=w0 == "init_eig", return_filters=True)
    got = []
    Y, w = oa.ogive_batch(X, W0=W0, callback=lambda y: got.append(np.array(y)), **kw)
    assert Y.dtype == dtype and w.dtype == dtype and Y.shape == (B, T, F, 1) and w.shape == (B, F, M, 1)
    info = oa.last_batch_info()
    assert info["batched"] == B and info["precision"] == "precise" and info["epochs"] == [n] * B
    assert len(got) == 2 and got[0].shape == (B, T, F, 1)
    tol = SAME if dtype == np.complex128 else 1e-6       # (complex64 output: the rounding of the result itself)
    for b in range(B):
        sgot = []
        Ys, ws = _single(oa, X[b], W0=W0[b] if w0 == "per_problem" else W0, callback=lambda y: sgot.append(np.array(y)), **kw)
        assert orc.rel_err(w[b], ws) < tol, (b, orc.rel_err(w[b], ws))
        assert orc.rel_err(Y[b], Ys) < tol, (b, orc.rel_err(Y[b], Ys))
        assert len(sgot) == 2
        for e in range(2):
            assert orc.rel_err(got[e][b], sgot[e]) < tol


# 9 to 16 parts of 64 bins (520 bins: a short fifth block of two; 1024 bins: 8 full blocks), as test_batch_gpu.py
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("F", [520, 1024])
def test_ogive_batch_matches_single_calls_at_9_to_16_parts(oa, F, model):
    B, T, M, n = 2, 64, 2, 120
    X = np.stack([orc.synth_iid(T, F, M, seed=1200 + F + b) for b in range(B)]).astype(np.complex128)
    kw = dict(n_iter=n, tol=0.0, model=model, return_filters=True)
    Y, w = oa.ogive_batch(X, **kw)
    info = oa.last_batch_info()
    assert info["batched"] == B and info["precision"] == "precise" and info["epochs"] == [n] * B
    for b in range(B):
        Ys, ws = _single(oa, X[b], **kw)
        ew, eY = orc.rel_err(w[b], ws), orc.rel_err(Y[b], Ys)
        print(f"ogive batch F={F} {model} problem {b}: w {ew:.2e}, Y {eY:.2e} of the single call's")
        assert ew < SAME and eY < SAME, (b, ew, eY)


# ---- 3. a stopping rule per problem ------------------------------------------------------------------------------------------
def test_ogive_batch_stops_each_problem_at_its_own_epoch(oa):
    T, F, M, n = 96, 45, 4, 300
    X = np.stack([_mix(T, F, M, 11), orc.synth_iid(T, F, M, seed=12), _mix(T, F, M, 13), _mix(T, F, M, 14),
                  orc.synth_iid(T, F, M, seed=15)]).astype(np.complex128)
    series = [_max_delta_series(oa, x, n) for x in X]
    # a tolerance no epoch's max ||delta|| comes within 1e-6 (relative) of, under which the problems stop at different epochs
    # and at least one never stops
    chosen = None
    for tol in np.geomspace(0.2, 1e-3, 60):
        if min(np.min(np.abs(s - tol)) / tol for s in series) < 1e-6:
            continue
        stop = [int(np.argmax(s < tol)) + 1 if np.any(s < tol) else n for s in series]
        never = [not np.any(s < tol) for s in series]
        if any(never) and len(set(s for s, nv in zip(stop, never) if not nv)) >= 2:
            chosen = (tol, stop, never)
            break
    assert chosen is not None, [s[:5] for s in series]
    tol, stop, never = chosen
    print(f"\n[ogive_batch] tol {tol:.4g}: stop epochs {stop}, never {never}")
    Y, w = oa.ogive_batch(X, n_iter=n, tol=tol, return_filters=True)
    info = oa.last_batch_info()
    assert info["epochs"] == stop and info["converged"] == [not v for v in never]
    for b in range(len(X)):
        Ys, ws = _single(oa, X[b], n_iter=n, tol=tol, return_filters=True)
        assert orc.rel_err(w[b], ws) < SAME and orc.rel_err(Y[b], Ys) < SAME, (b, orc.rel_err(w[b], ws))
    # the problems that stop: more epochs after all of them have stopped change nothing
    idx = [b for b in range(len(X)) if not never[b]]
    Y1, w1 = oa.ogive_batch(X[idx], n_iter=max(stop[b] for b in idx), tol=tol, return_filters=True)
    Y2, w2 = oa.ogive_batch(X[idx], n_iter=n + 100, tol=tol, return_filters=True)
    assert np.array_equal(Y1, Y2) and np.array_equal(w1, w2)
    assert oa.last_batch_info()["epochs"] == [stop[b] for b in idx]
    with oa.BatchPlan(len(idx), T, F, M, 1) as p:
        p.set_x(X[idx])
        p.covariance()
        p.set_w(None)
        p.ogive_begin("demix", "laplace")
        ran, conv, _ = p.ogive_iterate(0, n, 0.1, tol)
        assert ran.tolist() == [stop[b] for b in idx] and conv.all()
        wa = p.get_w()
        ran, conv, _ = p.ogive_iterate(n, 20, 0.1, tol)
        assert ran.tolist() == [0] * len(idx) and conv.all() and np.array_equal(p.get_w(), wa)


# ---- 4. bitwise batch invariance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, F, M", [(64, 2049, 4), (90, 37, 6), (64, 520, 2)])
def test_ogive_batch_bits_do_not_depend_on_the_batch(oa, T, F, M):
    B = 8
    X = np.stack([orc.synth_iid(T, F, M, seed=7 * b + M) if b % 2 else _mix(T, F, M, 7 * b + M) for b in range(B)])
    kw = dict(n_iter=60, tol=3e-2, return_filters=True)
    Yall, wall = oa.ogive_batch(X, **kw)
    eall = oa.last_batch_info()["epochs"]
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    Yp, wp = oa.ogive_batch(X[perm], **kw)
    ep = oa.last_batch_info()["epochs"]
    for b in (0, 3, 6):
        Y1, w1 = oa.ogive_batch(X[b:b + 1], **kw)
        assert np.array_equal(Y1[0], Yall[b]) and np.array_equal(w1[0], wall[b])
        assert oa.last_batch_info()["epochs"] == [eall[b]]
    for i, b in enumerate(perm):
        assert np.array_equal(Yp[i], Yall[b]) and np.array_equal(wp[i], wall[b]) and ep[i] == eall[b]


# ---- 5. isolation of a non-finite problem ------------------------------------------------------------------------------------
def test_ogive_batch_nan_flags_only_its_problem(oa):
    B, T, F, M, n, tol = 4, 80, 70, 4, 60, 3e-2
    X = np.stack([_mix(T, F, M, 40 + b) if b % 2 else orc.synth_iid(T, F, M, seed=40 + b) for b in range(B)])
    Xbad = X.copy()
    Xbad[2, 5, 3, 1] = np.nan
    Yc, wc = oa.ogive_batch(X, n_iter=n, tol=tol, return_filters=True)
    ec = oa.last_batch_info()["epochs"]
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 2$"):
        oa.ogive_batch(Xbad, n_iter=n, tol=tol)
    eb = oa.last_batch_info()["epochs"]
    assert eb[2] == n and not oa.last_batch_info()["converged"][2]
    with oa.BatchPlan(B, T, F, M, 1) as p:
        p.set_x(Xbad)
        p.covariance()
        p.set_w(None)
        p.ogive_begin("demix", "laplace")
        p.ogive_iterate(0, n, 0.1, tol)
        wb, sb = p.get_w(np.complex64, check=False), p.status()
    assert sb.tolist() == [False, False, True, False]
    for b in (0, 1, 3):
        assert np.array_equal(wb[b], wc[b]) and eb[b] == ec[b]


# ---- 6. the reference's own call size ----------------------------------------------------------------------------------------
def test_ogive_batch_user_sized(oa):
    B, T, F, M = 16, 235, 2049, 8
    X = np.stack([orc.synth_iid(T, F, M, seed=900 + b) if b % 4 else _mix(T, F, M, 900 + b) for b in range(B)])
    kw = dict(n_iter=4000, step_size=0.1, tol=1e-3, update="demix", return_filters=True)
    Y, w = oa.ogive_batch(X, **kw)
    info = oa.last_batch_info()
    print(f"\n[ogive_batch] 16 x 2049 x 235 x 8, sweep settings: epochs {info['epochs']}")
    assert np.all(np.isfinite(w))
    for b in (0, 5):
        Ys, ws = _single(oa, X[b], **kw)
        assert orc.rel_err(w[b], ws) < 1e-5, (b, orc.rel_err(w[b], ws))     # (complex64 results of up to 4000 epochs)
        assert orc.rel_err(Y[b], Ys) < 1e-5
