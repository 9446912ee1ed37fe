"""overiva_batch() on the GPU: parity with the real reference (tests/golden/batch_*.npz), the same result as one overiva() call
per problem, bit-for-bit independence of a problem's result from the batch around it, isolation of a non-finite problem, and
one batch of the reference's own size."""
import glob
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "batch_*.npz")))
TOL = 1e-5
SAME = 1e-9          # batched against single calls (both `precise`)
AMP_LIMIT = 1e3      # as conftest.chaotic


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _golden_x(g):
    T, F, M, K = (int(g[k]) for k in ("T", "F", "M", "K"))
    X = np.stack([orc.synth_iid(T, F, M, seed=int(s)) if fam == "iid" else orc.synth_mixture(T, F, M, max(K, 1), seed=int(s))
                  for fam, s in zip(g["family"], g["seed"])])
    assert np.allclose([x.astype(np.complex128).sum() for x in X], g["X_sum"], rtol=0, atol=1e-9)
    return X, K


def _single(oa, X, **kw):
    oa.set_precision("precise")
    try:
        return oa.overiva(X, **kw)
    finally:
        oa.set_precision("auto")


# ---- 1. reference parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_batch_reference_parity(oa, path):
    with np.load(path) as d:
        g = {k: d[k] for k in d.files}
    X, K = _golden_x(g)
    Y, W = oa.overiva_batch(X.astype(np.complex128), n_src=K, n_iter=20, proj_back=False, return_filters=True)
    assert Y.dtype == np.complex128 and W.shape == g["W_c128"].shape
    for b, fam in enumerate(g["family"]):
        Wr = g["W_c128"][b]
        if g["amp"][b] > AMP_LIMIT:        # the reference itself is chaotic here: finite and repeatable
            Y2, W2 = oa.overiva_batch(X[b:b + 1].astype(np.complex128), n_src=K, n_iter=20, proj_back=False, return_filters=True)
            assert np.all(np.isfinite(W[b])) and np.array_equal(W2[0], W[b])
            continue
        tol = TOL if fam == "iid" else max(TOL, 1.5 * orc.rel_err(g["W_c64"][b], Wr))
        assert orc.rel_err(W[b], Wr) < tol, (b, fam, orc.rel_err(W[b], Wr), tol)
        if b < len(g["Y_c128"]):
            assert orc.rel_err(Y[b], g["Y_c128"][b]) < tol


# ---- 2. the same result as one overiva() call per problem ------------------------------------------------------------------
W0_MODES = ("identity", "shared", "per_problem", "init_eig")


def _sweep():
    out = []
    i = 0
    for M in range(1, 9):
        for K in range(1, M + 1):
            out.append((M, K, ("laplace", "gauss")[i % 2], bool((i // 2) % 2), W0_MODES[i % 4],
                        (np.complex64, np.complex128)[(i // 3) % 2]))
            i += 1
    return out


@pytest.mark.parametrize("M, K, model, proj_back, w0, dtype", _sweep(),
                         ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_batch_matches_single_calls(oa, M, K, model, proj_back, w0, dtype):
    B, T, F = 3, 96, 67
    X = np.stack([orc.synth_iid(T, F, M, seed=100 * M + 10 * K + b) for b in range(B)]).astype(dtype)
    rng = np.random.default_rng(M * K)
    W0 = None
    if w0 == "shared":
        W0 = np.eye(M, K)[None] + 0.1 * (rng.standard_normal((F, M, K)) + 1j * rng.standard_normal((F, M, K)))
    elif w0 == "per_problem":
        W0 = np.eye(M, K)[None, None] + 0.1 * (rng.standard_normal((B, F, M, K)) + 1j * rng.standard_normal((B, F, M, K)))
    kw = dict(n_src=K, n_iter=12, proj_back=proj_back, model=model, init_eig=w0 == "init_eig", return_filters=True)
    got = []
    Y, W = oa.overiva_batch(X, W0=W0, callback=lambda y: got.append(np.array(y)), **kw)
    assert Y.dtype == dtype and W.dtype == dtype and Y.shape == (B, T, F, K) and W.shape == (B, F, M, K)
    assert oa.last_solver_info()["batched"] == B and oa.last_solver_info()["precision"] == "precise"
    assert len(got) == 2 and got[0].shape == (B, T, F, K)
    for b in range(B):
        w0b = W0[b] if w0 == "per_problem" else W0
        sgot = []
        Ys, Ws = _single(oa, X[b], W0=w0b, callback=lambda y: sgot.append(np.array(y)), **kw)
        tol = SAME if dtype == np.complex128 else 1e-6       # (complex64 output: the rounding of the result itself)
        assert orc.rel_err(W[b], Ws) < tol, (b, orc.rel_err(W[b], Ws))
        assert orc.rel_err(Y[b], Ys) < tol, (b, orc.rel_err(Y[b], Ys))
        for e in range(2):
            assert orc.rel_err(got[e][b], sgot[e]) < tol
    if w0 != "init_eig":
        # against the oracle (the reference's algorithm in complex128)
        Wr = orc.overiva_faithful(X[0].astype(np.complex128), n_src=K, n_iter=12, proj_back=False, model=model,
                                  W0=W0[0] if w0 == "per_problem" else W0, return_filters=True)[1]
        assert orc.rel_err(W[0], Wr) < 1e-5


# 9 to 16 parts of 64 bins: the activation sums them 16 at a time in blocks of two.  520 bins are 9 parts with a short fifth
# block, 1024 bins are 16 parts in 8 full blocks.  A wrong canonical order of that float32 sum moves r by about 1e-8 relative.
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("F", [520, 1024])
def test_batch_matches_single_calls_at_9_to_16_parts(oa, F, model):
    B, T, M, K = 2, 64, 2, 2
    X = np.stack([orc.synth_iid(T, F, M, seed=1000 + F + b) for b in range(B)]).astype(np.complex128)
    kw = dict(n_src=K, n_iter=12, proj_back=False, model=model, return_filters=True)
    Y, W = oa.overiva_batch(X, **kw)
    assert Y.dtype == np.complex128 and Y.shape == (B, T, F, K) and W.shape == (B, F, M, K)
    assert oa.last_solver_info()["batched"] == B and oa.last_solver_info()["precision"] == "precise"
    for b in range(B):
        Ys, Ws = _single(oa, X[b], **kw)
        eW, eY = orc.rel_err(W[b], Ws), orc.rel_err(Y[b], Ys)
        print(f"batch F={F} {model} problem {b}: W {eW:.2e}, Y {eY:.2e} of the single call's")
        assert eW < SAME and eY < SAME, (b, eW, eY)


# ---- 3. bitwise batch invariance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, F, M, K", [(64, 2049, 4, 2), (100, 40, 6, 3), (48, 7, 8, 8), (64, 520, 2, 2)])
def test_batch_bits_do_not_depend_on_the_batch(oa, T, F, M, K):
    B = 8
    X = np.stack([orc.synth_iid(T, F, M, seed=7 * b + M) if b % 2 else orc.synth_mixture(T, F, M, K, seed=7 * b + M)
                  for b in range(B)])
    run = lambda Xb: oa.overiva_batch(Xb, n_src=K, n_iter=5, return_filters=True)
    Yall, Wall = run(X)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    Yp, Wp = run(X[perm])
    for b in (0, 3, 7):
        Y1, W1 = run(X[b:b + 1])
        assert np.array_equal(Y1[0], Yall[b]) and np.array_equal(W1[0], Wall[b])
    for i, b in enumerate(perm):
        assert np.array_equal(Yp[i], Yall[b]) and np.array_equal(Wp[i], Wall[b])


# ---- 4. isolation of a non-finite problem ------------------------------------------------------------------------------------
def test_batch_nan_flags_only_its_problem(oa):
    B, T, F, M, K = 4, 80, 70, 4, 2
    X = np.stack([orc.synth_iid(T, F, M, seed=40 + b) for b in range(B)])
    Xbad = X.copy()
    Xbad[2, 5, 3, 1] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 2$"):
        oa.overiva_batch(Xbad, n_src=K, n_iter=4)

    def w_and_status(Xin):
        with oa.BatchPlan(B, T, F, M, K) as p:
            p.set_x(Xin)
            p.covariance()
            p.set_w(None)
            p.iterate(4)
            return p.get_w(check=False), p.status()

    Wc, sc = w_and_status(X)
    Wb, sb = w_and_status(Xbad)
    assert not sc.any() and sb.tolist() == [False, False, True, False]
    assert not np.all(np.isfinite(Wb[2]))
    for b in (0, 1, 3):
        assert np.array_equal(Wb[b], Wc[b])


# ---- 5. the reference's own call size ----------------------------------------------------------------------------------------
def test_batch_user_sized(oa):
    B, T, F, M, K = 16, 235, 2049, 8, 4
    X = np.stack([orc.synth_iid(T, F, M, seed=900 + b) if b % 4 else orc.synth_mixture(T, F, M, K, seed=900 + b)
                  for b in range(B)])
    Y, W = oa.overiva_batch(X, n_src=K, n_iter=20, return_filters=True)
    for b in range(0, B, 3):
        if b % 4 == 0:
            continue           # (mixture rows: covered by the golden parity; here the i.i.d. ones against single calls)
        Ys, Ws = _single(oa, X[b].astype(np.complex128), n_src=K, n_iter=20, return_filters=True)
        assert orc.rel_err(W[b].astype(np.complex128), Ws) < 1e-6      # (W returned in complex64, the dtype of X)
    with oa.BatchPlan(B, T, F, M, K) as p:
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.iterate(20)
        W64 = p.get_w(np.complex128)
    for b in range(1, B, 4):
        Ws = _single(oa, X[b].astype(np.complex128), n_src=K, n_iter=20, proj_back=False, return_filters=True)[1]
        assert orc.rel_err(W64[b], Ws) < SAME, (b, orc.rel_err(W64[b], Ws))
