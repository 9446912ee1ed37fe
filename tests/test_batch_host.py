"""overiva_batch() without a GPU: argument validation raises before the library is touched, the batch ABI is declared and
exported, and the oracle reproduces the batched golden fixtures (tests/golden/batch_*.npz)."""
import glob
import os
import re

import numpy as np
import pytest

from oracle import overiva_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "batch_*.npz")))
BATCH_SYMBOLS = ("oiva_batch_create", "oiva_batch_destroy", "oiva_batch_set_x_host", "oiva_batch_set_x_dev", "oiva_batch_covariance",
                 "oiva_batch_set_w", "oiva_batch_set_w_eig", "oiva_batch_iterate", "oiva_batch_demix", "oiva_batch_get_w",
                 "oiva_batch_status", "oiva_batch_time_stages")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _x(B=2, T=16, F=5, M=4):
    return (np.ones((B, T, F, M)) + 1j).astype(np.complex64)


@pytest.mark.parametrize("bad", [
    dict(X=_x()[0]),                                    # ndim 3
    dict(X=_x()[None]),                                 # ndim 5
    dict(X=_x(M=9)),                                    # 9 channels
    dict(X=_x(), n_src=5),
    dict(X=_x(), n_src=0),
    dict(X=_x(), model="student"),
    dict(X=_x(), W0=np.ones((5, 4, 3))),                # K = 4 (default): wrong K
    dict(X=_x(), W0=np.ones((3, 5, 4, 4))),             # wrong B
    dict(X=_x(), n_src=2, W0=np.ones((2, 6, 4, 2))),    # wrong F
])
def test_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.overiva_batch(X, **bad)


def test_batch_accepts_the_documented_w0_shapes(monkeypatch):
    from overiva_amd import batch

    X = _x()
    for W0 in (np.ones((5, 4, 2)), np.ones((4, 2)), np.ones((5, 1, 2)), np.ones((2, 5, 4, 2))):
        batch._check_args(X, 2, "laplace", W0, 3)


def test_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.overiva_batch(_x(), n_src=2)


def test_batch_is_public():
    import overiva_amd

    assert "overiva_batch" in overiva_amd.__all__ and callable(overiva_amd.overiva_batch)
    assert "BatchPlan" in overiva_amd.__all__


def test_batch_symbols_declared_and_bound():
    from overiva_amd import _lib

    txt = open(HEADER).read()
    declared = set(re.findall(r"\bint\s+\**\s*(oiva_batch_\w+)\s*\(", txt))
    assert declared == set(BATCH_SYMBOLS), declared ^ set(BATCH_SYMBOLS)
    assert set(BATCH_SYMBOLS) <= set(_lib.SIGNATURES)


def test_batch_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in BATCH_SYMBOLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[6:-4])
def test_oracle_reproduces_batch_golden(path):
    with np.load(path) as d:
        g = {k: d[k] for k in d.files}
    T, F, M, K = (int(g[k]) for k in ("T", "F", "M", "K"))
    assert os.path.getsize(path) < 1 << 20
    for b, (fam, seed) in enumerate(zip(g["family"], g["seed"])):
        X = orc.synth_iid(T, F, M, seed=int(seed)) if fam == "iid" else orc.synth_mixture(T, F, M, max(K, 1), seed=int(seed))
        assert abs(X.astype(np.complex128).sum() - g["X_sum"][b]) < 1e-9
        Y, W = orc.overiva_faithful(X.astype(np.complex128), n_src=K, n_iter=20, proj_back=False, return_filters=True)
        assert orc.rel_err(W, g["W_c128"][b]) < 1e-9
        if b < len(g["Y_c128"]):
            assert orc.rel_err(Y, g["Y_c128"][b]) < 1e-9
