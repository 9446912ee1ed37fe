"""The complex128 data path of the batched solver on the GPU (``data="complex128"``, csrc/kernels_batch_c128.hip): parity with the
real reference's complex128 results to 1e-9 on the committed fixtures and on full-precision input (tests/golden/c128_*.npz), every
stage against the oracle's stage functions to 1e-12, bits that do not depend on the batch, device input, isolation of a non-finite
room and the callback.  Every figure is printed before it is asserted."""
import ctypes
import os

import numpy as np
import pytest

from conftest import chaotic, golden_files
from oracle import overiva_oracle as orc
from helpers.c128_cases import GOLDEN, admitted, load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9           # against the real reference: the bound tests/test_oracle_golden.py holds the float64 oracle to
STAGE_TOL = 1e-12    # float64 sums against the oracle's stages (test_weighted_covariance's bound)
C128 = "complex128"


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _trajectory(oa, X, K, model, data, W0=None, init_eig=False, stops=(1, 5, 12, 20)):
    """one room through the plan: W after 1, 5 and 20 iterations, Y with projection back after 12 and without after 20"""
    T, F, M = X.shape
    out = {}
    with oa.BatchPlan(1, T, F, M, K, model, **({} if data is None else {"data": data})) as p:
        p.set_x(X[None])
        p.covariance()
        if init_eig:
            p.set_w_eig()
        else:
            p.set_w(W0)
        done = 0
        for n in stops:
            p.iterate(n - done)
            done = n
            if n == 12:
                out["Ypb_12"] = p.demix(True, np.complex128)[0]
            else:
                out[f"W_{n}"] = p.get_w(np.complex128, check=False)[0]
        out["Y"] = p.demix(False, np.complex128)[0]
        assert p.info()["data"] == (data or "complex64")
    return out


def _small_golden():
    out = []
    for path in golden_files():
        with np.load(path) as d:
            if int(d["M"]) <= 8:
                out.append(path)
    return out


# ---- 1. against the real reference, committed fixtures -----------------------------------------------------------------------
@pytest.mark.parametrize("path", _small_golden(), ids=lambda p: os.path.basename(p)[8:-4])
def test_reference_parity_on_the_committed_fixtures(oa, path):
    with np.load(path) as d:
        g = {k: d[k] for k in d.files}
    X, K = g["X"].astype(np.complex128), int(g["K"])
    errs, gots = {}, {}
    for model in orc.MODELS:
        got = gots[model] = _trajectory(oa, X, K, model, C128)
        for n in (1, 5, 20):
            if f"W_c128_{model}_{n}" in g and not chaotic(g, model, n):
                errs[f"W_{model}_{n}"] = orc.rel_err(got[f"W_{n}"], g[f"W_c128_{model}_{n}"])
        if f"Y_c128_{model}_20" in g and not chaotic(g, model, 20):
            errs[f"Y_{model}_20"] = orc.rel_err(got["Y"], g[f"Y_c128_{model}_20"])
        if f"Ypb_c128_{model}_12" in g and not chaotic(g, model, 12):
            errs[f"Ypb_{model}_12"] = orc.rel_err(got["Ypb_12"], g[f"Ypb_c128_{model}_12"])
    if "Ypb_frame0_c128_laplace_12" in g and not chaotic(g, "laplace", 12):
        errs["Ypb_frame0_laplace_12"] = orc.rel_err(gots["laplace"]["Ypb_12"][0], g["Ypb_frame0_c128_laplace_12"])
    if "W0" in g:
        errs["W_w0_3"] = orc.rel_err(_trajectory(oa, X, K, "laplace", C128, W0=g["W0"], stops=(3,))["W_3"], g["W_w0_c128_laplace_3"])
        errs["W_det_2"] = orc.rel_err(_trajectory(oa, X, X.shape[2], "laplace", C128, stops=(2,))["W_2"], g["W_det_c128_laplace_2"])
        # (eigenvector phases are LAPACK's: magnitudes, as tests/test_oracle_golden.py compares them)
        Ye = _trajectory(oa, X, K, "laplace", C128, init_eig=True, stops=(3,))["Y"]
        errs["absY_eig_3"] = orc.rel_err(np.abs(Ye), np.abs(g["Y_eig_c128_laplace_3"]))
    print(f"\n[c128 parity] {os.path.basename(path)}", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs and max(errs.values()) < TOL, {k: v for k, v in errs.items() if not v < TOL}


# ---- 2. full-precision input: the reference's complex128 numbers, which the default path cannot reach ----------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[5:-4])
def test_full_precision_input(oa, path):
    g, X, K = load_case(path)
    rows = g["rows"]
    new, old = {}, {}
    for model in orc.MODELS:
        for data, errs in ((C128, new), (None, old)):
            got = _trajectory(oa, X, K, model, data)
            for n in (1, 5, 20):
                if admitted(g, model, n):
                    errs[f"W_{model}_{n}"] = orc.rel_err(got[f"W_{n}"], g[f"W_{model}_{n}"])
            if admitted(g, model, 20):
                errs[f"Y_{model}_20"] = orc.rel_err(got["Y"][rows], g[f"Yrows_{model}_20"])
            if admitted(g, model, 12):
                errs[f"Ypb_{model}_12"] = orc.rel_err(got["Ypb_12"][rows], g[f"Ypbrows_{model}_12"])
    print(f"\n[c128 full precision] {os.path.basename(path)}")
    for k in new:
        print(f"    {k}: complex128 path {new[k]:.2e}, default path {old[k]:.2e}")
    assert len(new) >= 8
    assert max(new.values()) < TOL, {k: v for k, v in new.items() if not v < TOL}
    assert all(old[k] >= 10 * new[k] for k in new), {k: (new[k], old[k]) for k in new if not old[k] >= 10 * new[k]}


def test_the_public_calls_return_complex128(oa):
    g, X, K = load_case(GOLDEN[0])
    Y, W = oa.overiva_batch(X[None], n_src=K, n_iter=5, proj_back=False, return_filters=True, data=C128)
    assert Y.dtype == np.complex128 and W.dtype == np.complex128
    assert oa.last_batch_info()["data"] == C128
    e = orc.rel_err(W[0], g["W_laplace_5"])
    Ys, Ws = oa.overiva_batch_ragged([X, X[:40]], n_src=K, n_iter=5, proj_back=False, return_filters=True, data=C128)
    assert Ys[1].dtype == np.complex128 and oa.last_batch_info()["data"] == C128 and oa.last_batch_info()["ragged"]
    print(f"\n[c128 public] W {e:.2e}")
    assert e < TOL and np.array_equal(Ws[0], W[0]) and np.array_equal(Ys[0], Y[0])
    oa.overiva_batch(X[None].astype(np.complex64), n_src=K, n_iter=1)
    assert oa.last_batch_info()["data"] == "complex64"
    with oa.BatchPlan(1, *X.shape, K, data=C128) as p:       # the rounded copy, and the refusals of the library itself
        p.set_x(X[None])
        p.covariance()
        p.set_w()
        p.iterate(2)
        assert np.array_equal(p.demix(True, np.complex64), p.demix(True, np.complex128).astype(np.complex64))
        dev = ctypes.c_void_p()
        assert p.lib.oiva_batch_demix_dev(p.h, 1, ctypes.byref(dev)) == oa._lib.ERR_ARG
        assert b"complex128" in p.lib.oiva_last_error()
        assert p.lib.oiva_batch_ogive_begin(p.h, 0, 0) == oa._lib.ERR_ARG and b"complex128" in p.lib.oiva_last_error()
        assert p.lib.oiva_batch_set_w_pca(p.h, None) == oa._lib.ERR_ARG and b"complex128" in p.lib.oiva_last_error()
        assert p.lib.oiva_batch_ilrma_iterate(p.h, 1) == oa._lib.ERR_ARG and b"complex128" in p.lib.oiva_last_error()
        assert p.lib.oiva_batch_set_x_host(p.h, oa._lib.ptr(X[None].astype(np.complex64)), 0) == oa._lib.ERR_ARG
        total, stages = p.time_stages(2)
        assert total > 0 and all(v > 0 for v in stages.values())
    with oa.BatchPlan(1, *X.shape, K) as p:                   # the mode is chosen before X is set
        p.set_x(X[None])
        assert p.lib.oiva_batch_set_data_c128(p.h) == oa._lib.ERR_STATE


# ---- 3. stage by stage from a known state against the oracle's stage functions ----------------------------------------------------
@pytest.mark.parametrize("model", orc.MODELS)
@pytest.mark.parametrize("shape", [(70, 17, 2, 1), (257, 20, 8, 4), (64, 130, 4, 2), (129, 16, 7, 3)], ids=lambda s: "x".join(map(str, s)))
def test_stages_against_the_oracle(oa, shape, model):
    T, F, M, K = shape
    rng = np.random.default_rng(sum(shape))
    X = rng.standard_normal((T, F, M)) + 1j * rng.standard_normal((T, F, M))
    zero_frame = 5 if (model == "laplace" and shape == (257, 20, 8, 4)) else None
    if zero_frame is not None:
        X[zero_frame] = 0.
    W0 = np.eye(M, K)[None] + 0.1 * (rng.standard_normal((F, M, K)) + 1j * rng.standard_normal((F, M, K)))
    with oa.BatchPlan(1, T, F, M, K, model, data=C128) as p:
        p.set_x(X[None])
        p.covariance()
        Cx = p.get_cx(np.complex128)[0]
        p.set_w(W0)
        p.iterate(1)
        w = p.get_weights()[0]
        V = np.moveaxis(p.get_weighted_cov()[0], 1, 0)          # (K, F, M, M)
        W1 = p.get_w(np.complex128)[0]
    e = {"Cx": orc.rel_err(Cx, orc.input_covariance(X))}
    r_inv, wscale = orc.finalize_activation(orc.demix_power(X, W0), F, model)
    live = np.ones(T, bool)
    if zero_frame is not None:
        live[zero_frame] = False
        assert np.all(r_inv[zero_frame] == 1. / orc.EPS_R)
        assert np.all(w[zero_frame] == 1. / orc.EPS_R), w[zero_frame]       # the eps floor: exactly 1 / eps
    e["weights"] = orc.rel_err(w[live], r_inv[live])
    e["weights_max"] = float(np.max(np.abs(w[live] - r_inv[live]) / r_inv[live]))
    Vo = orc.weighted_cov_all(X, r_inv)
    e["V"] = max(orc.rel_err(V[k], Vo[k]) for k in range(K))
    # one per-bin update from the state the device held: its own Cx and V, W scaled as overiva.py:161-167
    W_hat = orc.init_demixing(Cx, K, W0=W0)
    W_hat[:, :, :K] /= wscale[None, None, :]
    e["update"] = orc.rel_err(W1, orc.ip_update_bin(W_hat, V, Cx, K)[:, :, :K])
    print(f"\n[c128 stages] {shape} {model}", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) < STAGE_TOL, e


# ---- 4. bits do not depend on the batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [17, 130])
def test_bits_do_not_depend_on_the_batch(oa, F):
    T, M, K, B = 70, 4, 2, 5
    rng = np.random.default_rng(F)
    X = rng.standard_normal((B, T, F, M)) + 1j * rng.standard_normal((B, T, F, M))
    kw = dict(n_src=K, n_iter=5, return_filters=True, data=C128)
    Y, W = oa.overiva_batch(X, **kw)
    perm = np.array([3, 0, 4, 2, 1])
    Yp, Wp = oa.overiva_batch(X[perm], **kw)
    assert np.array_equal(Yp, Y[perm]) and np.array_equal(Wp, W[perm])
    for b in (0, 2, 4):
        Y1, W1 = oa.overiva_batch(X[b:b + 1], **kw)
        assert np.array_equal(Y1[0], Y[b]) and np.array_equal(W1[0], W[b]), b
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(Y))


@pytest.mark.parametrize("model", orc.MODELS)
def test_ragged_rooms_get_the_bits_of_their_own_dense_batch(oa, model):
    frames, F, M, K = (70, 257, 64, 70), 17, 3, 2
    rng = np.random.default_rng(7)
    Xs = [rng.standard_normal((T, F, M)) + 1j * rng.standard_normal((T, F, M)) for T in frames]
    kw = dict(n_src=K, n_iter=5, model=model, return_filters=True, data=C128)
    Ys, W = oa.overiva_batch_ragged(Xs, **kw)
    for b, x in enumerate(Xs):
        Yd, Wd = oa.overiva_batch(x[None], **kw)
        assert Ys[b].dtype == np.complex128 and np.array_equal(Ys[b], Yd[0]) and np.array_equal(W[b], Wd[0]), b


# ---- 5. device input ------------------------------------------------------------------------------------------------------------
def test_set_x_device_gives_the_bits_of_set_x(oa):
    import torch

    B, T, F, M, K = 2, 70, 17, 4, 2
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, T, F, M)) + 1j * rng.standard_normal((B, T, F, M))
    res = []
    for dev in (False, True):
        with oa.BatchPlan(B, T, F, M, K, data=C128) as p:
            if dev:
                t = torch.from_numpy(X).cuda()
                assert t.dtype == torch.complex128 and t.is_contiguous()
                torch.cuda.synchronize()
                p.set_x_device(t.data_ptr(), keepalive=t)
            else:
                p.set_x(X)
            p.covariance()
            p.set_w()
            p.iterate(5)
            res.append((p.get_w(), p.demix(True, np.complex128)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- 6. a room of zeros ---------------------------------------------------------------------------------------------------------
def test_a_room_of_zeros_is_named_and_leaves_the_others_alone(oa):
    B, T, F, M, K = 3, 70, 17, 4, 2
    rng = np.random.default_rng(6)
    X = rng.standard_normal((B, T, F, M)) + 1j * rng.standard_normal((B, T, F, M))
    Yg, Wg = oa.overiva_batch(X, n_src=K, n_iter=5, return_filters=True, data=C128)
    X[1] = 0.
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1$"):
        oa.overiva_batch(X, n_src=K, n_iter=5, data=C128)
    with oa.BatchPlan(B, T, F, M, K, data=C128) as p:
        p.set_x(X)
        p.covariance()
        p.set_w()
        p.iterate(5)
        assert list(p.status()) == [False, True, False]
        W = p.get_w(check=False)
        Y = p.demix(True, np.complex128)
    assert not np.all(np.isfinite(W[1]))
    for b in (0, 2):
        assert np.array_equal(W[b], Wg[b]) and np.array_equal(Y[b], Yg[b]), b


# ---- 7. the callback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj_back", [False, True])
def test_callback_receives_complex128_estimates(oa, proj_back):
    B, T, F, M, K = 2, 64, 20, 3, 2
    rng = np.random.default_rng(9)
    X = rng.standard_normal((B, T, F, M)) + 1j * rng.standard_normal((B, T, F, M))
    got = []
    oa.overiva_batch(X, n_src=K, n_iter=12, proj_back=proj_back, callback=lambda y: got.append(np.array(y)), data=C128)
    assert len(got) == 2 and all(y.dtype == np.complex128 and y.shape == (B, T, F, K) for y in got)
    for y, n in zip(got, (0, 10)):
        assert np.array_equal(y, oa.overiva_batch(X, n_src=K, n_iter=n, proj_back=proj_back, data=C128)), n
