"""The wide path (17..32 channels, csrc/kernels_wide.hip) stage by stage and end to end against the oracle: the weighted and
the input covariance, the partial powers, one per-bin update and the J initialisation, whole runs of overiva() and
auxiva_pca(), and the narrow-only entry points refusing a wide plan."""
import ctypes
import glob
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

WIDE = [17, 18, 23, 24, 31, 32]


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


def _random_what(F, M, seed):
    rng = np.random.default_rng(seed)
    return np.eye(M)[None] + 0.3 * (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M)))


# ---- covariance -----------------------------------------------------------------------------------------------------------
def _cov_cases():
    out = []
    for M in WIDE:
        for K in sorted({k for k in (1, 2, 3, 4, 8, 16, M) if k <= M}):
            out.append((M, K))
    return out


@pytest.mark.parametrize("mode", ["fast", "mixed", "precise"])
@pytest.mark.parametrize("case", _cov_cases(), ids=lambda c: f"{c[0]}ch{c[1]}src")
def test_wide_covariance(oa, case, mode):
    M, K = case
    T, F = 71 + 3 * M, 37 - M // 2          # ragged frames and bins
    X = orc.synth_mixture(T, F, M, min(K, 4), seed=100 * M + K)
    rinv = np.random.default_rng(M + 17 * K).gamma(2.0, 1.0, (T, K)).astype(np.float32)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_x(X)
        p.covariance()
        Cx = p.get_cx(np.complex128)
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
    w = 1.0 / (np.float32(1) / rinv).astype(np.float64) if mode == "precise" else rinv.astype(np.float64)
    eV = orc.rel_err(V, orc.weighted_cov_all(X, w))
    eC = orc.rel_err(Cx, orc.input_covariance(X.astype(np.complex128)))
    tol = 1e-10 if mode == "precise" else 3e-7
    assert eV < tol and eC < max(tol, 1e-7), (eV, eC)
    assert np.array_equal(V, np.conj(np.swapaxes(V, -1, -2)))


# ---- power ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 63, 65, 130])
@pytest.mark.parametrize("M, K", [(17, 1), (24, 2), (32, 3), (31, 7), (32, 32)])
def test_wide_power(oa, M, K, F):
    T = 53
    X = orc.synth_iid(T, F, M, seed=F + M)
    What = _random_what(F, M, seed=F * M + K)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.t_set_what(What)
        pw = p.t_run_power()
    assert orc.rel_err(pw, orc.demix_power(X, What.astype(np.complex64)[:, :, :K])) < 2e-6


# ---- one update, J initialisation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [17, 24, 32])
@pytest.mark.parametrize("kind", ["1", "2", "3", "M"])
def test_wide_update(oa, M, kind):
    K = M if kind == "M" else int(kind)
    T, F = 150, 9
    X = orc.synth_iid(T, F, M, seed=M + K)
    rinv = np.random.default_rng(K).gamma(2.0, 1.0, (T, K)).astype(np.float32)
    W_in = _random_what(F, M, seed=3 * M + K)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("precise")
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.t_set_what(W_in)
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        p.t_run_update()
        W_out = p.t_get_what(np.complex128)
    w = 1.0 / (np.float32(1) / rinv).astype(np.float64)
    V = orc.weighted_cov_all(X, w)
    ref = orc.ip_update_bin(W_in, V, orc.input_covariance(X.astype(np.complex128)), K)
    assert orc.rel_err(W_out[:, :, :K], ref[:, :, :K]) < 1e-9
    assert orc.rel_err(W_out, ref) < 1e-9


@pytest.mark.parametrize("mode", ["fast", "precise"])
@pytest.mark.parametrize("M, K", [(17, 2), (24, 5), (32, 1)])
def test_wide_init_j(oa, M, K, mode):
    T, F = 120, 7
    X = orc.synth_iid(T, F, M, seed=M * K)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        W = p.t_get_what(np.complex128)
    ref = orc.init_demixing(orc.input_covariance(X.astype(np.complex128)), K)
    assert orc.rel_err(W, ref) < (1e-9 if mode == "precise" else 1e-4)


# ---- end to end, against the real reference's results (tests/golden/wide_*.npz, make_wide_golden.py) ---------------------------
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_*.npz")))
TOL = 1e-5
FAST_FLOORS = 6.0         # as tests/test_gpu_parity.py
AMP_LIMIT = 1e3           # as conftest.chaotic


def _load(path):
    with np.load(path) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("n_iter", [1, 5, 20])
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[5:-4])
def test_wide_end_to_end(oa, path, n_iter, model):
    g = _load(path)
    X, K = g["X"], int(g["K"])
    X128 = X.astype(np.complex128)
    run = lambda Xin: oa.overiva(Xin, n_src=K, n_iter=n_iter, model=model, proj_back=False, return_filters=True)
    if float(g[f"amp_{model}_{n_iter}"]) > AMP_LIMIT:
        # the reference itself is chaotic here: nothing to pin; the run is finite and repeatable
        Y1, W1 = run(X)
        Y2, W2 = run(X)
        assert np.all(np.isfinite(W1)) and np.array_equal(W1, W2) and np.array_equal(Y1, Y2)
        return
    Wr = g[f"W_c128_{model}_{n_iter}"]
    # complex128 in -> `precise`, complex128 out: 1e-5 from the reference's complex128 result
    Y, W = run(X128)
    assert Y.dtype == np.complex128 and W.dtype == np.complex128
    assert orc.rel_err(W, Wr) < TOL
    if f"Y_c128_{model}_{n_iter}" in g:
        assert orc.rel_err(Y, g[f"Y_c128_{model}_{n_iter}"]) < TOL
    # complex64 in -> `mixed`: max(1e-5, 1.5 floors) from the reference's complex64 result, floor = its distance from complex128
    Wf = g[f"W_c64_{model}_{n_iter}"]
    floor = orc.rel_err(Wf, Wr)
    Y, W = run(X)
    assert Y.dtype == np.complex64
    assert orc.rel_err(W, Wf) < max(TOL, 1.5 * floor), (orc.rel_err(W, Wf), floor)
    # `fast`: within FAST_FLOORS reference floors of the complex128 result
    oa.set_precision("fast")
    try:
        Y, W = run(X)
    finally:
        oa.set_precision("auto")
    assert orc.rel_err(W, Wr) < max(TOL, FAST_FLOORS * floor), (orc.rel_err(W, Wr), floor)


def _phase_aligned(W, ref):
    """W with every column's phase turned onto ref's (eigenvector phases are a convention)"""
    ph = np.sum(np.conj(W) * ref, axis=1, keepdims=True)
    return W * ph / np.maximum(np.abs(ph), 1e-300)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[5:-4])
def test_wide_options(oa, path):
    """W0, init_eig, proj_back with the callback payloads at epochs 0 and 10, auxiva_pca -- against the real reference"""
    g = _load(path)
    X128, K = g["X"].astype(np.complex128), int(g["K"])
    W = oa.overiva(X128, n_src=K, n_iter=3, proj_back=False, W0=g["W0"], return_filters=True)[1]
    assert orc.rel_err(W, g["W_w0_c128_laplace_3"]) < TOL
    W = oa.overiva(X128, n_src=K, n_iter=3, proj_back=False, init_eig=True, return_filters=True)[1]
    assert orc.rel_err(_phase_aligned(W, g["W_eig_c128_laplace_3"]), g["W_eig_c128_laplace_3"]) < TOL
    if "Ypb_c128_laplace_12" in g:
        got = []
        Y = oa.overiva(X128, n_src=K, n_iter=12, proj_back=True, callback=lambda y: got.append(np.array(y)))
        assert orc.rel_err(Y, g["Ypb_c128_laplace_12"]) < TOL
        assert len(got) == 2
        assert orc.rel_err(got[0], g["cb0_c128_laplace"]) < TOL and orc.rel_err(got[1], g["cb10_c128_laplace"]) < TOL
    if "Ypca_c128_laplace_5" in g:
        Y = oa.auxiva_pca(X128, n_src=K, n_iter=5, proj_back=True, model="laplace")
        assert orc.rel_err(Y, g["Ypca_c128_laplace_5"]) < TOL


@pytest.mark.parametrize("M, K", [(32, 2), (24, None)])
def test_wide_auxiva_pca(oa, M, K):
    T, F = 200, 7
    X = orc.synth_mixture(T, F, M, 2, seed=M).astype(np.complex128)
    Yr = orc.auxiva_pca_faithful(X, n_src=K, proj_back=True, n_iter=5)
    Y = oa.auxiva_pca(X, n_src=K, proj_back=True, n_iter=5)
    assert Y.shape == Yr.shape
    assert orc.rel_err(Y, Yr) < 1e-5


def test_wide_full_size_ragged_bins(oa):
    """2049 bins (a ragged last batch of 64) x 400 frames x 32 channels / 2 sources, `mixed`, 5 iterations: max(1e-5, 1.5 floors)
    from the oracle's complex64 result (the reference's own arithmetic), floor = its distance from the complex128 result"""
    T, F, M, K = 400, 2049, 32, 2
    X = orc.synth_mixture(T, F, M, K, seed=11)
    Yr, Wr = orc.overiva_faithful(X.astype(np.complex128), n_src=K, n_iter=5, return_filters=True)
    Yf, Wf = orc.overiva_faithful(X, n_src=K, n_iter=5, return_filters=True)
    floor = max(orc.rel_err(Wf, Wr), orc.rel_err(Yf, Yr))
    Y, W = oa.overiva(X, n_src=K, n_iter=5, return_filters=True)
    tol = max(TOL, 1.5 * floor)
    assert orc.rel_err(W, Wf) < tol and orc.rel_err(Y, Yf) < tol, (orc.rel_err(W, Wf), floor)


def test_wide_non_finite_raises(oa):
    X = np.zeros((64, 5, 20), np.complex64)      # V = 0: W_hat^H V is singular
    with pytest.raises(np.linalg.LinAlgError):
        oa.overiva(X, n_src=2, n_iter=2, return_filters=True)


def test_narrow_only_entry_points_refuse_a_wide_plan(oa):
    T, F, M = 96, 5, 24
    X = orc.synth_iid(T, F, M, seed=3)
    with oa.Plan(T, F, M, 1, "laplace") as p:
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        lib = p.lib
        assert lib.oiva_plan_ogive_begin(p.h, 0, 0) == -1
        assert lib.oiva_plan_set_resident(p.h, 1) == -1
        active = ctypes.c_int(-1)
        assert lib.oiva_plan_set_fuse_cov_update(p.h, 1, ctypes.byref(active)) == 0 and active.value == 0
        active = ctypes.c_int(-1)
        assert lib.oiva_plan_set_cov_quad(p.h, 1, ctypes.byref(active)) == 0 and active.value == 0
        p.iterate(2)                       # the plan still runs on the wide path
        assert np.all(np.isfinite(p.get_w()))
