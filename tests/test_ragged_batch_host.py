"""overiva_batch_ragged() without a GPU: argument validation raises before the library is touched, the ragged ABI entry is
declared, bound and exported and checks its arguments before any device call, and the oracle reproduces the ragged golden
fixture (tests/golden/ragged.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import overiva_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
GOLDEN = os.path.join(HERE, "golden", "ragged.npz")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _xs(frames=(16, 24, 9), F=5, M=4, dtype=np.complex64):
    return [(np.ones((t, F, M)) + 1j).astype(dtype) for t in frames]


@pytest.mark.parametrize("bad", [
    dict(Xs=[]),                                                      # empty
    dict(Xs=_xs()[:1] + _xs(F=6)[1:]),                                # F differs
    dict(Xs=_xs()[:1] + _xs(M=3)[1:]),                                # M differs
    dict(Xs=_xs()[:2] + _xs(dtype=np.complex128)[2:]),                # mixed dtypes
    dict(Xs=_xs(frames=(16, 0, 9))),                                  # T_b = 0
    dict(Xs=_xs(M=9)),                                                # 9 channels
    dict(Xs=[x[0] for x in _xs()]),                                   # a problem of ndim 2
    dict(Xs=_xs(), n_src=5),
    dict(Xs=_xs(), n_src=0),
    dict(Xs=_xs(), model="student"),
    dict(Xs=_xs(), W0=np.ones((5, 4, 3))),                            # K = 4 (default): wrong K
    dict(Xs=_xs(), n_src=2, W0=np.ones((2, 5, 4, 2))),                # wrong B
    dict(Xs=_xs(), n_src=2, W0=np.ones((3, 6, 4, 2))),                # wrong F
    dict(Xs=_xs(), n_iter=-1),
])
def test_ragged_validation_before_device(no_device, bad):
    Xs = bad.pop("Xs")
    with pytest.raises(ValueError):
        no_device.overiva_batch_ragged(Xs, **bad)


def test_ragged_accepts_the_documented_w0_shapes():
    from overiva_amd import batch

    Xs = _xs()
    for W0 in (np.ones((5, 4, 2)), np.ones((4, 2)), np.ones((5, 1, 2)), np.ones((3, 5, 4, 2))):
        batch._check_ragged_args(Xs, 2, "laplace", W0, 3)
    batch._check_ragged_args(_xs(frames=(8, 8)), 2, "laplace", None, 3)       # equal lengths: legal


def test_ragged_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.overiva_batch_ragged(_xs(), n_src=2)


def test_ragged_is_public():
    import overiva_amd

    assert "overiva_batch_ragged" in overiva_amd.__all__ and callable(overiva_amd.overiva_batch_ragged)
    assert "RaggedBatchPlan" in overiva_amd.__all__ and issubclass(overiva_amd.RaggedBatchPlan, overiva_amd.BatchPlan)


def test_ragged_symbol_declared_and_bound():
    from overiva_amd import _lib

    txt = open(HEADER).read()
    assert re.search(r"\boiva_status\s+oiva_batch_create_ragged\s*\(", txt)
    assert not re.search(r"\bint\s+\**\s*oiva_batch_create_ragged\s*\(", txt)
    assert "oiva_batch_create_ragged" in _lib.SIGNATURES


def _built_lib():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    return _lib.load()


def test_ragged_symbol_exported():
    lib = _built_lib()
    assert hasattr(lib, "oiva_batch_create_ragged")


@pytest.mark.parametrize("B, frames, F, M, K", [
    (3, None, 5, 4, 2),                 # null frames
    (0, [8], 5, 4, 2),                  # B < 1
    (3, [8, 0, 8], 5, 4, 2),            # a T_b < 1
    (3, [8, -3, 8], 5, 4, 2),
    (2, [8, 8], 0, 4, 2),               # F < 1
    (2, [8, 8], 5, 9, 2),               # M > 8
    (2, [8, 8], 5, 0, 1),               # M < 1
    (2, [8, 8], 5, 4, 5),               # K > M
    (2, [8, 8], 5, 4, 0),               # K < 1
    (2, [2_000_000_000, 2_000_000_000], 2049, 8, 4),      # sizes that overflow
])
def test_ragged_create_checks_arguments_before_device_use(B, frames, F, M, K):
    """on a machine without a GPU any device call fails with OIVA_ERR_HIP: OIVA_ERR_ARG shows the check came first"""
    from overiva_amd import _lib

    lib = _built_lib()
    h = ctypes.c_void_p()
    fr = None if frames is None else (ctypes.c_int * len(frames))(*frames)
    rc = lib.oiva_batch_create_ragged(ctypes.byref(h), 0, B, fr, F, M, K, 0, None)
    assert rc == _lib.ERR_ARG, (rc, lib.oiva_last_error())
    assert not h.value


def test_oracle_reproduces_ragged_golden():
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN) as d:
        g = {k: d[k] for k in d.files}
    F = int(g["F"])
    # one oracle run per (M, K, model) group is enough to pin the fixture; the first problem of every group
    seen = set()
    for p in range(len(g["T"])):
        T, M, K, model = int(g["T"][p]), int(g["M"][p]), int(g["K"][p]), str(g["model"][p])
        X = _golden_input(g, p)
        assert abs(X.astype(np.complex128).sum() - g["X_sum"][p]) < 1e-9
        if (M, K, model) in seen:
            continue
        seen.add((M, K, model))
        W = orc.overiva_faithful(X.astype(np.complex128), n_src=K, n_iter=int(g["n_iter"]), proj_back=False, model=model,
                                 return_filters=True)[1]
        Wr = g["W_c128"][p][:, :M, :K]
        assert orc.rel_err(W, Wr) < 1e-9 * max(1.0, float(g["amp"][p])), (p, orc.rel_err(W, Wr))


def _golden_input(g, p):
    T, F, M, K = int(g["T"][p]), int(g["F"]), int(g["M"][p]), int(g["K"][p])
    seed = int(g["seed"][p])
    return orc.synth_iid(T, F, M, seed=seed) if g["family"][p] == "iid" else orc.synth_mixture(T, F, M, K, seed=seed)
