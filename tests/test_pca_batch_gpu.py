"""auxiva_pca_batch() on the GPU: the batched projection gives the bits of the epilogue's demix; the eigensolver on B * F bins
against numpy.linalg.eigh; the composed filters against np.matmul; a problem's bits do not depend on the batch; parity with the
real reference (tests/golden) and with the oracle at every channel / source count; isolation of a non-finite room; audio in,
audio out through separate_batch."""
import numpy as np
import pytest

from conftest import golden_files
from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

PCA_CASES = [(2, 1), (4, 2), (5, 2), (8, 2), (8, 7)]
# frame counts on both sides of the 64-frame power split and the 256-frame covariance split; 67 bins leave a last bin batch of 3
FRAMES, F_BITS = (16, 63, 65, 147, 257), 67
TOL = 1e-5


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _problems(frames, F, M, K, seed, mix=()):
    return [orc.synth_mixture(T, F, M, K, seed=seed + b) if b in mix else orc.synth_iid(T, F, M, seed=seed + b)
            for b, T in enumerate(frames)]


def _outer(oa, Xs, M, K, dense=False):
    """the outer plan after set_x and covariance: ragged on the list Xs, or dense on its stack"""
    if dense:
        X = np.stack(Xs)
        plan = oa.BatchPlan(X.shape[0], X.shape[1], X.shape[2], M, K)
        plan.set_x(X)
    else:
        plan = oa.RaggedBatchPlan([x.shape[0] for x in Xs], Xs[0].shape[1], M, K)
        plan.set_x(Xs)
    plan.covariance()
    return plan


def _inner(oa, outer, new_X, model="laplace"):
    K = outer.K
    inner = oa.BatchPlan(outer.B, outer.T, outer.F, K, K, model) if outer.dense else oa.RaggedBatchPlan(outer.frames, outer.F, K, K, model)
    inner.set_x_device(new_X.ptr, keepalive=new_X)
    inner.covariance()
    return inner


def _staged(oa, plan, n_iter, model="laplace"):
    """the stages of auxiva_pca_batch on an outer plan whose covariance is computed, one plan method each"""
    plan.set_w_pca()
    with _inner(oa, plan, plan.project_device(), model) as inner:
        inner.set_w(None)
        inner.iterate(n_iter)
        plan.compose_w(inner)


# ---- 1. the projection is the epilogue's demix, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
@pytest.mark.parametrize("M, K", PCA_CASES)
def test_projection_bits(oa, M, K, dense):
    frames = (65, 65, 65) if dense else FRAMES
    Xs = _problems(frames, F_BITS, M, K, seed=10 * M + K, mix=(1,))
    with _outer(oa, Xs, M, K, dense) as plan:
        plan.set_w_pca()
        new_X = plan.project_device()
        assert new_X.owner is plan and new_X.n_chan == K and new_X.frames == list(frames) and new_X.dense == dense
        got = new_X.get_x()
        want = plan.demix(proj_back=False)
        again = new_X.get_x()                  # (the projection does not live in the array demix writes)
    for b, T in enumerate(frames):
        assert got[b].shape == (T, F_BITS, K) and got[b].dtype == np.complex64
        assert np.all(np.isfinite(got[b]))
        assert np.array_equal(got[b], want[b]), (b, T, orc.rel_err(got[b], want[b]))
        assert np.array_equal(again[b], got[b])


# ---- 2. eigenvalues and principal subspace against LAPACK ---------------------------------------------------------------------
@pytest.mark.parametrize("M, K", PCA_CASES)
def test_eigenvalues_and_subspace(oa, M, K):
    Xs = _problems(FRAMES, F_BITS, M, K, seed=10 * M + K, mix=(1,))
    with _outer(oa, Xs, M, K) as plan:
        Cx = plan.get_cx(np.complex128)
        ev = plan.set_w_pca(return_eigenvalues=True)
        P = plan.get_w(np.complex128)
        assert plan.set_w_pca() is None
    assert ev.shape == (len(FRAMES), F_BITS, M) and P.shape == (len(FRAMES), F_BITS, M, K)
    for b in range(len(FRAMES)):
        lam, vec = np.linalg.eigh(Cx[b])
        assert np.max(np.abs(ev[b] - lam)) <= 1e-12 * np.max(np.abs(lam)), b
        gap = np.min(np.diff(lam, axis=1)) / np.max(lam)
        tol = 1e-11 / max(gap, 1e-6)
        Pr = vec[:, :, -K:]
        proj = P[b] @ np.conj(P[b].swapaxes(1, 2))
        want = Pr @ np.conj(Pr.swapaxes(1, 2))
        assert np.max(np.abs(proj - want)) < tol, (b, np.max(np.abs(proj - want)), gap)


# ---- 3. the composed filters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
@pytest.mark.parametrize("M, K", PCA_CASES)
def test_compose(oa, M, K, dense):
    frames = (65, 65, 65) if dense else FRAMES
    Xs = _problems(frames, F_BITS, M, K, seed=10 * M + K)
    with _outer(oa, Xs, M, K, dense) as plan:
        plan.set_w_pca()
        P = plan.get_w(np.complex128)
        with _inner(oa, plan, plan.project_device()) as inner:
            inner.set_w(None)
            inner.iterate(3)
            W_red = inner.get_w(np.complex128)
            plan.compose_w(inner)
        W = plan.get_w(np.complex128)
        W32 = plan.get_w(np.complex64)
        with oa.BatchPlan(len(frames), 65, F_BITS + 1, K, K) as other:       # another F
            with pytest.raises(ValueError):
                plan.compose_w(other)
            assert plan.lib.oiva_batch_compose_w(plan.h, other.h) == oa._lib.ERR_ARG          # (the library checks too)
        assert plan.lib.oiva_batch_compose_w(plan.h, plan.h) == oa._lib.ERR_ARG
        assert np.array_equal(plan.get_w(np.complex128), W)
    want = np.matmul(P, W_red)
    assert W.shape == want.shape == (len(frames), F_BITS, M, K)
    for b in range(len(frames)):
        # at most 8 terms of float64 products per element: worst-case rounding about 4e-15
        assert orc.rel_err(W[b], want[b]) < 1e-13, (b, orc.rel_err(W[b], want[b]))
    assert np.array_equal(W32, W.astype(np.complex64))


# ---- 4. bitwise batch invariance ----------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(oa):
    frames, F, M, K = (65, 300, 16, 257, 147, 64), 67, 6, 2
    Xs = _problems(frames, F, M, K, seed=55, mix=(1, 4))
    run = lambda xs: oa.auxiva_pca_batch(xs, n_src=K, n_iter=6, return_filters=True)
    Yall, Wall = run(Xs)
    info = oa.last_batch_info()
    assert info["algorithm"] == "auxiva_pca" and info["reduced"] == K and info["ragged"] is True and info["frames"] == list(frames)
    assert Wall.shape == (len(frames), F, M, K)
    assert all(y.shape == (T, F, K) and np.all(np.isfinite(y)) for y, T in zip(Yall, frames))
    perm = [4, 1, 5, 0, 3, 2]
    Yp, Wp = run([Xs[i] for i in perm])
    for i, b in enumerate(perm):
        assert np.array_equal(Yp[i], Yall[b]) and np.array_equal(Wp[i], Wall[b]), b
    for subset in ([0, 2], [3], [5, 1, 4]):
        Ys, Ws = run([Xs[i] for i in subset])
        for i, b in enumerate(subset):
            assert np.array_equal(Ys[i], Yall[b]) and np.array_equal(Ws[i], Wall[b]), (subset, b)
    # a list of equal lengths takes the ragged plans and still gives the bits of the dense call
    Ye, We = run([Xs[0], Xs[0]])
    Yd, Wd = run(np.stack([Xs[0], Xs[0]]))
    assert "ragged" not in oa.last_batch_info()
    assert isinstance(Yd, np.ndarray) and Yd.shape == (2, frames[0], F, K)
    assert np.array_equal(We, Wd) and all(np.array_equal(Ye[b], Yd[b]) for b in range(2))
    assert np.array_equal(Ye[0], Yall[0]) and np.array_equal(Yd[1], Yall[0])


def test_determined_is_overiva_batch(oa):
    T, F, M = 65, 67, 4
    X = np.stack(_problems((T, T, T), F, M, M, seed=77, mix=(1,)))
    Y, W = oa.auxiva_pca_batch(X, n_src=M, n_iter=6, proj_back=False, return_filters=True)
    info = oa.last_batch_info()
    assert info["algorithm"] == "auxiva_pca" and info["reduced"] == M
    Yo, Wo = oa.overiva_batch(X, n_src=None, n_iter=6, proj_back=True, return_filters=True)
    assert np.array_equal(Y, Yo) and np.array_equal(W, Wo)
    Yn = oa.auxiva_pca_batch(X, n_iter=6)                  # n_src=None: determined
    assert np.array_equal(Yn, Yo)
    Yr = oa.auxiva_pca_batch(list(X), n_src=M, n_iter=6)
    Yor = oa.overiva_batch_ragged(list(X), n_src=None, n_iter=6, proj_back=True)
    assert all(np.array_equal(a, b) for a, b in zip(Yr, Yor))


# ---- 5. parity with the real reference ----------------------------------------------------------------------------------------
def _pca_golden():
    out = []
    for path in golden_files():
        with np.load(path) as d:
            if "Ypca_c128_laplace_5" in d.files and int(d["M"]) <= 8:
                out.append(path)
    return out


@pytest.mark.parametrize("path", _pca_golden(), ids=lambda p: p.split("overiva_")[-1][:-len(".npz")])
def test_reference_parity(oa, path):
    with np.load(path) as d:
        X, K, want = d["X"].astype(np.complex128), int(d["K"]), d["Ypca_c128_laplace_5"]
        amp = max(1.0, float(d["amp_laplace_5"])) if "amp_laplace_5" in d.files else 1.0
    T, F, M = X.shape
    rooms = [orc.synth_iid(T + 7, F, M, seed=1).astype(np.complex128), X, orc.synth_iid(T - 5, F, M, seed=2).astype(np.complex128)]
    Ys = oa.auxiva_pca_batch(rooms, n_src=K, n_iter=5, proj_back=True, model="laplace")
    assert Ys[1].shape == want.shape and Ys[1].dtype == np.complex128
    e = orc.rel_err(Ys[1], want)
    print(f"\n[pca_batch] {path.split('overiva_')[-1]} auxiva_pca 5 its: Y err {e:.2e}")
    assert e < 2 * TOL * max(1.0, amp / 10.0)      # the bound test_auxiva_pca holds the single call to


def test_reference_fixtures_are_there():
    assert len(_pca_golden()) >= 12


# ---- 6. every channel and source count against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("M, K", [(M, K) for M in range(2, 9) for K in range(1, M)])
def test_oracle_sweep(oa, M, K):
    frames, F, n_iter = (80, 96, 150), 33, 8
    model = ("laplace", "gauss")[(10 * M + K) % 2]
    X64 = [orc.synth_iid(T, F, M, seed=100 * M + 10 * K + b + 1) for b, T in enumerate(frames)]
    X128 = [x.astype(np.complex128) for x in X64]
    want = [orc.auxiva_pca_faithful(x, n_src=K, n_iter=n_iter, proj_back=True, model=model) for x in X128]
    for Xs, dtype in ((X128, np.complex128), (X64, np.complex64)):
        Ys = oa.auxiva_pca_batch(Xs, n_src=K, n_iter=n_iter, model=model)
        for b, T in enumerate(frames):
            assert Ys[b].shape == (T, F, K) and Ys[b].dtype == dtype
            e = orc.rel_err(Ys[b], want[b])
            print(f"\n[pca_batch] {M}/{K} {model} {np.dtype(dtype).name} problem {b}: Y err {e:.2e}")
            assert e < 2e-5, (b, e)


# ---- 7. isolation of a non-finite room ----------------------------------------------------------------------------------------
def test_zero_room_flags_only_itself(oa):
    frames, F, M, K = (80, 130, 50, 300), 70, 4, 2
    Xs = _problems(frames, F, M, K, seed=40)
    bad = [x.copy() for x in Xs]
    bad[2][:] = 0
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 2$"):
        oa.auxiva_pca_batch(bad, n_src=K, n_iter=4)
    with _outer(oa, bad, M, K) as plan:
        _staged(oa, plan, 4)
        assert list(plan.status()) == [False, False, True, False]
        Yb = plan.demix(True)
        Wb = plan.get_w(np.complex128, check=False)
    Y, W = oa.auxiva_pca_batch(Xs, n_src=K, n_iter=4, return_filters=True)
    for b in (0, 1, 3):                          # the finite rooms: the bits they have without the zero room
        assert np.array_equal(Yb[b], Y[b]) and np.array_equal(Wb[b].astype(W.dtype), W[b]), b


# ---- 8. audio in, audio out -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(640, 640, 640), (640, 512, 333)], ids=["dense", "ragged"])
def test_separate_batch(oa, lens):
    from overiva_amd import separate

    M, K, frame, hop, n_iter = 4, 2, 64, 32, 5
    rng = np.random.default_rng(8)
    rooms = [rng.standard_normal((n, M)).astype(np.float32) for n in lens]
    dense = len(set(lens)) == 1
    x = np.stack(rooms) if dense else rooms
    y, W = oa.separate_batch(x, frame, hop, n_src=K, n_iter=n_iter, algorithm="auxiva_pca", return_filters=True)
    info = oa.last_batch_info()
    assert info["audio"] is True and info["algorithm"] == "auxiva_pca" and info["reduced"] == K
    wa, ws = separate._windows(frame, hop, None, None)
    with oa.BatchSTFT(lens[0] if dense else list(lens), M, frame, hop, win_a=wa, win_s=ws, B=len(lens) if dense else None) as st:
        Xd = st.analysis_device(x)
        F = frame // 2 + 1
        plan = oa.BatchPlan(len(lens), st.frames[0], F, M, K) if dense else oa.RaggedBatchPlan(st.frames, F, M, K)
        with plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            _staged(oa, plan, n_iter)
            want = st.synthesis_device(plan.demix_device(True))
            Wwant = plan.get_w(np.complex128)
    assert np.array_equal(W, Wwant) and W.shape == (len(lens), F, M, K)
    for b, n in enumerate(lens):
        assert y[b].shape == (n // hop * hop, K) and y[b].dtype == np.float32 and np.all(np.isfinite(y[b]))
        assert np.array_equal(y[b], want[b]), b
    with pytest.raises(ValueError):
        oa.separate_batch(x, frame, hop, n_src=K, algorithm="auxiva_pca", step_size=0.1)
