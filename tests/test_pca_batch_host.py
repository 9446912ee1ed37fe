"""auxiva_pca_batch() without a GPU: argument validation raises before the library is touched, the three new ABI entries are
declared as oiva_status, bound and exported and check their arguments before any device call, compose_w refuses plans that do not
fit, and separate_batch knows the new algorithm."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
NEW_SYMBOLS = ("oiva_batch_set_w_pca", "oiva_batch_project_dev", "oiva_batch_compose_w")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _x(B=2, T=8, F=5, M=4, dtype=np.complex64):
    return np.ones((B, T, F, M), dtype)


def _xs(frames=(8, 9), F=5, M=4, dtype=np.complex64):
    return [np.ones((t, F, M), dtype) for t in frames]


@pytest.mark.parametrize("bad", [
    dict(X=_x(M=9), n_src=2),                                            # 9 channels
    dict(X=_xs(M=9), n_src=2),
    dict(X=_x(), n_src=0),
    dict(X=_x(), n_src=5),                                               # M + 1
    dict(X=_xs(), n_src=0),
    dict(X=_xs(), n_src=5),
    dict(X=_x(), n_src=2, model="student"),
    dict(X=_xs(), n_src=2, model="student"),
    dict(X=_x(), n_src=2, n_iter=-1),
    dict(X=_xs()[:1] + _xs(dtype=np.complex128)[1:], n_src=2),           # mixed dtypes
    dict(X=_xs()[:1] + _xs(F=6)[1:], n_src=2),                           # mixed F
    dict(X=_xs()[:1] + _xs(M=3)[1:], n_src=2),                           # mixed M
    dict(X=[], n_src=2),
    dict(X=_x()[0], n_src=2),                                            # ndim 3
    dict(X=_x(), n_src=2, W0=np.ones((5, 4, 2))),                        # (F, M, K) instead of (F, K, K)
    dict(X=_xs(), n_src=2, W0=np.ones((5, 4, 2))),
    dict(X=_x(), n_src=2, W0=np.ones((3, 5, 2, 2))),                     # wrong B
])
def test_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.auxiva_pca_batch(X, **bad)


def test_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.auxiva_pca_batch(_x(), n_src=2)
    with pytest.raises(ValueError, match="sharding"):
        no_device.auxiva_pca_batch(_xs(), n_src=2)


def test_no_callback_and_no_unknown_keywords(no_device):
    with pytest.raises(TypeError):
        no_device.auxiva_pca_batch(_x(), n_src=2, callback=lambda y: None)
    with pytest.raises(TypeError):
        no_device.auxiva_pca_batch(_x(), n_src=2, step_size=0.1)


def test_is_public():
    import overiva_amd

    assert "auxiva_pca_batch" in overiva_amd.__all__ and callable(overiva_amd.auxiva_pca_batch)
    for cls in (overiva_amd.BatchPlan, overiva_amd.RaggedBatchPlan):
        for method in ("set_w_pca", "project_device", "compose_w"):
            assert callable(getattr(cls, method)), (cls, method)


def test_new_symbols_declared_and_bound():
    from overiva_amd import _lib

    txt = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\boiva_status\s+" + name + r"\s*\(", txt), name
        assert not re.search(r"\bint\s+\**\s*" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name


def _built_lib():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    return _lib.load()


def test_new_symbols_exported():
    lib = _built_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_null_arguments_are_argument_errors():
    """on a machine without a GPU any device call fails with OIVA_ERR_HIP: OIVA_ERR_ARG shows the check came first"""
    from overiva_amd import _lib

    lib = _built_lib()
    dev = ctypes.c_void_p()
    ev = (ctypes.c_double * 8)()
    assert lib.oiva_batch_set_w_pca(None, None) == _lib.ERR_ARG
    assert lib.oiva_batch_set_w_pca(None, ev) == _lib.ERR_ARG
    assert lib.oiva_batch_project_dev(None, ctypes.byref(dev)) == _lib.ERR_ARG
    assert lib.oiva_batch_project_dev(None, None) == _lib.ERR_ARG
    assert lib.oiva_batch_compose_w(None, None) == _lib.ERR_ARG
    assert not dev.value


def _fake_plan(cls, B, F, M, K):
    """a plan object without device state: what compose_w compares before it calls the library"""
    p = object.__new__(cls)
    p.B, p.F, p.M, p.K, p.h = B, F, M, K, None
    return p


@pytest.mark.parametrize("inner", [(2, 5, 2, 2), (3, 6, 2, 2), (3, 5, 3, 3), (3, 5, 3, 2), (3, 5, 4, 2), (3, 5, 1, 1)],
                         ids=["B", "F", "K", "not determined", "M", "K=1"])
def test_compose_w_refuses_plans_that_do_not_fit(no_device, inner):
    outer = _fake_plan(no_device.BatchPlan, 3, 5, 4, 2)
    with pytest.raises(ValueError):
        outer.compose_w(_fake_plan(no_device.RaggedBatchPlan, *inner))
    with pytest.raises(ValueError):
        outer.compose_w(outer)
    with pytest.raises(ValueError):
        outer.compose_w(None)


def test_separate_batch_knows_the_algorithm(no_device):
    from overiva_amd import separate

    rooms = [np.ones((n, 4), np.float32) for n in (640, 512, 333)]
    for x in (rooms, np.ones((2, 640, 4), np.float32)):
        r = separate._check_separate_args(x, 64, None, 2, 20, "auxiva_pca", "laplace", None, None, None, {})
        assert len(r) == 9 and r[3:6] == (4, 32, 2)
        separate._check_separate_args(x, 64, None, 2, 20, "auxiva_pca", "laplace", None, None, np.ones((33, 2, 2)), {})   # (F, K, K)
    with pytest.raises(ValueError):
        no_device.separate_batch(rooms, 64, n_src=2, algorithm="fastica")
    with pytest.raises(ValueError):
        no_device.separate_batch(rooms, 64, n_src=2, algorithm="auxiva_pca", step_size=0.1)
    with pytest.raises(ValueError):
        no_device.separate_batch(rooms, 64, n_src=2, algorithm="auxiva_pca", W0=np.ones((33, 4, 2)))        # (F, M, K)
    with pytest.raises(ValueError):
        no_device.separate_batch(rooms, 64, n_src=5, algorithm="auxiva_pca")
