"""overiva_batch_ragged() on the GPU: problem b of a ragged batch gets the bits of the dense batch of its own length, whatever the
other problems; the same result as one overiva() call per problem; parity with the real reference (tests/golden/ragged.npz);
isolation of a non-finite problem; one batch of the reference's own room lengths; packed device input and the refusal of OGIVE."""
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ragged.npz")
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
        return oa.overiva(X, **kw)
    finally:
        oa.set_precision("auto")


def _problems(frames, F, M, K, seed, mix=()):
    return [orc.synth_mixture(T, F, M, K, seed=seed + b) if b in mix else orc.synth_iid(T, F, M, seed=seed + b)
            for b, T in enumerate(frames)]


# ---- 1. the bits of the dense batch of the problem's own length ---------------------------------------------------------------
# frame counts across every boundary of the geometry: 1..3 covariance splits (256), power splits (64), activation blocks (256)
BIT_CASES = [
    # F, M, K, model, dtype, frames, proj_back, init_eig
    (7, 1, 1, "laplace", np.complex64, (16, 63, 64, 65, 147, 160, 168, 235, 256, 257, 300, 520), True, False),
    (67, 2, 2, "gauss", np.complex128, (16, 64, 257, 520), False, False),
    (2049, 4, 2, "laplace", np.complex64, (147, 160, 168, 235, 300), True, False),
    (67, 6, 3, "gauss", np.complex64, (63, 65, 256, 300), True, True),
    (7, 8, 4, "laplace", np.complex128, (16, 65, 160, 520), False, False),
    (67, 8, 8, "gauss", np.complex128, (16, 147, 257), True, False),
    (520, 2, 2, "gauss", np.complex128, (64, 65, 100), False, False),          # 9 parts of 64 bins: summed 16 at a time
]


@pytest.mark.parametrize("F, M, K, model, dtype, frames, proj_back, init_eig", BIT_CASES,
                         ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_ragged_bits_match_the_dense_batch(oa, F, M, K, model, dtype, frames, proj_back, init_eig):
    Xs = [x.astype(dtype) for x in _problems(frames, F, M, K, seed=300 * M + K, mix=(1,) if model == "laplace" else ())]
    kw = dict(n_src=K, n_iter=8, proj_back=proj_back, model=model, init_eig=init_eig, return_filters=True)
    Ys, W = oa.overiva_batch_ragged(Xs, **kw)
    info = oa.last_batch_info()
    assert info["ragged"] is True and info["frames"] == list(frames) and info["batched"] == len(frames)
    assert W.shape == (len(frames), F, M, K) and W.dtype == dtype
    for b, X in enumerate(Xs):
        assert Ys[b].shape == (frames[b], F, K) and Ys[b].dtype == dtype
        Yd, Wd = oa.overiva_batch(X[None], **kw)
        assert np.array_equal(Ys[b], Yd[0]), (b, frames[b], orc.rel_err(Ys[b], Yd[0]))
        assert np.array_equal(W[b], Wd[0]), (b, frames[b], orc.rel_err(W[b], Wd[0]))


# ---- 2. bitwise batch invariance ----------------------------------------------------------------------------------------------
def test_ragged_bits_do_not_depend_on_the_batch(oa):
    frames, F, M, K = (65, 300, 16, 257, 147, 64), 67, 4, 2
    Xs = _problems(frames, F, M, K, seed=55, mix=(1, 4))
    run = lambda xs: oa.overiva_batch_ragged(xs, n_src=K, n_iter=6, return_filters=True)
    Yall, Wall = run(Xs)
    perm = [4, 1, 5, 0, 3, 2]
    Yp, Wp = run([Xs[i] for i in perm])
    for i, b in enumerate(perm):
        assert np.array_equal(Yp[i], Yall[b]) and np.array_equal(Wp[i], Wall[b])
    for subset in ([0, 2], [3], [5, 1, 4]):
        Ys, Ws = run([Xs[i] for i in subset])
        for i, b in enumerate(subset):
            assert np.array_equal(Ys[i], Yall[b]) and np.array_equal(Ws[i], Wall[b])
    # equal lengths take the ragged path and still give the dense bits
    Ye, We = run([Xs[0], Xs[0]])
    Yd, Wd = oa.overiva_batch(np.stack([Xs[0], Xs[0]]), n_src=K, n_iter=6, return_filters=True)
    assert np.array_equal(We, Wd) and all(np.array_equal(Ye[b], Yd[b]) for b in range(2))


# ---- 3. the same result as one overiva() call per problem ---------------------------------------------------------------------
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
def test_ragged_matches_single_calls(oa, M, K, model, proj_back, w0, dtype):
    frames, F = (80, 96, 150), 67       # (lengths at which no case of the sweep is chaotic in the reference itself)
    B = len(frames)
    Xs = [orc.synth_iid(T, F, M, seed=100 * M + 10 * K + b + 1).astype(dtype) for b, T in enumerate(frames)]
    rng = np.random.default_rng(M * K + 1)
    W0 = None
    if w0 == "shared":
        W0 = np.eye(M, K)[None] + 0.1 * (rng.standard_normal((F, M, K)) + 1j * rng.standard_normal((F, M, K)))
    elif w0 == "per_problem":
        W0 = np.eye(M, K)[None, None] + 0.1 * (rng.standard_normal((B, F, M, K)) + 1j * rng.standard_normal((B, F, M, K)))
    kw = dict(n_src=K, n_iter=12, proj_back=proj_back, model=model, init_eig=w0 == "init_eig", return_filters=True)
    got = []
    Ys, W = oa.overiva_batch_ragged(Xs, W0=W0, callback=lambda ys: got.append([np.array(y) for y in ys]), **kw)
    assert isinstance(Ys, list) and len(Ys) == B and W.dtype == dtype and W.shape == (B, F, M, K)
    assert oa.last_solver_info()["batched"] == B and oa.last_solver_info()["precision"] == "precise"
    assert len(got) == 2 and [g.shape for g in got[0]] == [(T, F, K) for T in frames]
    tol = SAME if dtype == np.complex128 else 1e-6       # (complex64 output: the rounding of the result itself)
    for b in range(B):
        w0b = W0[b] if w0 == "per_problem" else W0
        sgot = []
        Y1, W1 = _single(oa, Xs[b], W0=w0b, callback=lambda y: sgot.append(np.array(y)), **kw)
        assert Ys[b].dtype == dtype
        assert orc.rel_err(W[b], W1) < tol, (b, orc.rel_err(W[b], W1))
        assert orc.rel_err(Ys[b], Y1) < tol, (b, orc.rel_err(Ys[b], Y1))
        for e in range(2):
            assert orc.rel_err(got[e][b], sgot[e]) < tol


# 9 to 16 parts of 64 bins (520 bins: a short fifth block of two; 1024 bins: 8 full blocks), as test_batch_gpu.py
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("F", [520, 1024])
def test_ragged_matches_single_calls_at_9_to_16_parts(oa, F, model):
    frames, M, K = (64, 65), 2, 2
    Xs = [orc.synth_iid(T, F, M, seed=1100 + F + b).astype(np.complex128) for b, T in enumerate(frames)]
    kw = dict(n_src=K, n_iter=12, proj_back=False, model=model, return_filters=True)
    Ys, W = oa.overiva_batch_ragged(Xs, **kw)
    assert oa.last_solver_info()["batched"] == len(frames) and oa.last_solver_info()["precision"] == "precise"
    for b, X in enumerate(Xs):
        Y1, W1 = _single(oa, X, **kw)
        eW, eY = orc.rel_err(W[b], W1), orc.rel_err(Ys[b], Y1)
        print(f"ragged F={F} {model} problem {b}: W {eW:.2e}, Y {eY:.2e} of the single call's")
        assert eW < SAME and eY < SAME, (b, eW, eY)


# ---- 4. reference parity --------------------------------------------------------------------------------------------------------
def _golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _golden_input(g, p):
    T, F, M, K = int(g["T"][p]), int(g["F"]), int(g["M"][p]), int(g["K"][p])
    seed = int(g["seed"][p])
    X = orc.synth_iid(T, F, M, seed=seed) if g["family"][p] == "iid" else orc.synth_mixture(T, F, M, K, seed=seed)
    assert abs(X.astype(np.complex128).sum() - g["X_sum"][p]) < 1e-9
    return X


@pytest.mark.parametrize("group", range(4))
def test_ragged_reference_parity(oa, group):
    g = _golden()
    ps = [p for p in range(len(g["T"])) if int(g["group"][p]) == group]
    M, K, model = int(g["M"][ps[0]]), int(g["K"][ps[0]]), str(g["model"][ps[0]])
    n_iter = int(g["n_iter"])
    Xs = [_golden_input(g, p).astype(np.complex128) for p in ps]
    assert len({x.shape[0] for x in Xs}) == len(Xs)          # a ragged batch
    Ys, W = oa.overiva_batch_ragged(Xs, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True)
    for i, p in enumerate(ps):
        Wr = g["W_c128"][p][:, :M, :K]
        if g["amp"][p] > AMP_LIMIT:        # the reference itself is chaotic here: finite and repeatable
            Y2, W2 = oa.overiva_batch_ragged(Xs[i:i + 1], n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True)
            assert np.all(np.isfinite(W[i])) and np.array_equal(W2[0], W[i])
            continue
        W64 = g["W_c64"][p][:, :M, :K].astype(np.complex128)
        tol = TOL if g["family"][p] == "iid" else max(TOL, 1.5 * orc.rel_err(W64, Wr))
        assert orc.rel_err(W[i], Wr) < tol, (p, orc.rel_err(W[i], Wr), tol)
        if p == int(g["Y_index"]):
            assert orc.rel_err(Ys[i], g["Y_c128"]) < tol


# ---- 5. isolation of a non-finite problem ---------------------------------------------------------------------------------------
def test_ragged_nan_flags_only_its_problem(oa):
    frames, F, M, K = (80, 130, 50, 300), 70, 4, 2
    Xs = _problems(frames, F, M, K, seed=40)
    bad = [x.copy() for x in Xs]
    bad[2][5, 3, 1] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 2$"):
        oa.overiva_batch_ragged(bad, n_src=K, n_iter=4)

    def w_and_status(xs):
        with oa.RaggedBatchPlan(frames, F, M, K) as p:
            p.set_x(xs)
            p.covariance()
            p.set_w(None)
            p.iterate(4)
            return p.get_w(check=False), p.status()

    Wc, sc = w_and_status(Xs)
    Wb, sb = w_and_status(bad)
    assert not sc.any() and sb.tolist() == [False, False, True, False]
    assert not np.all(np.isfinite(Wb[2]))
    for b in (0, 1, 3):
        assert np.array_equal(Wb[b], Wc[b])


# ---- 6. the reference's own room lengths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, K", [(4, 2), (8, 4)])
def test_ragged_user_sized(oa, M, K):
    B, F = 32, 2049
    frames = [int(t) for t in np.random.default_rng(147 + M).integers(147, 169, size=B)]
    assert len(set(frames)) > 5
    Xs = [orc.synth_iid(T, F, M, seed=1200 + 37 * M + b) if b % 4 else orc.synth_mixture(T, F, M, K, seed=1200 + 37 * M + b)
          for b, T in enumerate(frames)]
    with oa.RaggedBatchPlan(frames, F, M, K) as p:
        p.set_x(Xs)
        p.covariance()
        p.set_w(None)
        p.iterate(20)
        W64 = p.get_w(np.complex128)
        Ys = p.demix(True)
    assert [y.shape for y in Ys] == [(T, F, K) for T in frames] and all(np.all(np.isfinite(y)) for y in Ys)
    for b in (1, 14, 31):
        # the dense batch of the room's own length, bit for bit; a single call (at 4 / 2 overiva() takes the X-resident kernel,
        # whose float64 sums run in another order: agreement to 1e-7 there) to rounding
        with oa.BatchPlan(1, frames[b], F, M, K) as d:
            d.set_x(Xs[b][None])
            d.covariance()
            d.set_w(None)
            d.iterate(20)
            assert np.array_equal(d.get_w(np.complex128)[0], W64[b]) and np.array_equal(d.demix(True)[0], Ys[b])
        Ws = _single(oa, Xs[b].astype(np.complex128), n_src=K, n_iter=20, proj_back=False, return_filters=True)[1]
        assert orc.rel_err(W64[b], Ws) < 1e-6, (b, orc.rel_err(W64[b], Ws))


# ---- 7. packed device input, and the ABI's refusal of OGIVE --------------------------------------------------------------------
def test_ragged_device_input_and_ogive_refusal(oa):
    import torch

    frames, F, M, K = (90, 270, 33), 65, 4, 2
    Xs = _problems(frames, F, M, K, seed=77)
    packed = np.concatenate(Xs).astype(np.complex64)

    def run(setter):
        with oa.RaggedBatchPlan(frames, F, M, K, model="gauss") as p:
            setter(p)
            p.covariance()
            p.set_w(None)
            p.iterate(5)
            return p.demix(True), p.get_w()

    Yh, Wh = run(lambda p: p.set_x(Xs))
    Yp, Wp = run(lambda p: p.set_x(packed))
    t = torch.from_numpy(packed).to(f"cuda:{oa.get_device()}")
    torch.cuda.synchronize()
    Yd, Wd = run(lambda p: p.set_x_device(t.data_ptr(), keepalive=t))
    assert np.array_equal(Wh, Wd) and np.array_equal(Wh, Wp)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(Yh, Yd, Yp))

    from overiva_amd import _lib

    with oa.RaggedBatchPlan(frames, F, M, 1) as p:
        p.set_x(Xs)
        p.covariance()
        p.set_w(None)
        assert p.lib.oiva_batch_ogive_begin(p.h, 0, 0) == _lib.ERR_ARG
        assert b"ragged" in p.lib.oiva_last_error()
        assert p.lib.oiva_batch_ogive_iterate(p.h, 0, 1, 0.1, 1e-3, None, None, None) == _lib.ERR_ARG
        with pytest.raises(ValueError, match="ragged"):
            p.ogive_begin()
