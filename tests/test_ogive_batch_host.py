"""ogive_batch() without a GPU: argument validation raises before the library is touched, the function is public, the batched
OGIVE ABI is declared and bound, and the golden fixture (tests/golden/ogive_batch.npz) is what its generator describes."""
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
GOLDEN = os.path.join(HERE, "golden", "ogive_batch.npz")
OGIVE_BATCH_SYMBOLS = ("oiva_batch_get_cx", "oiva_batch_ogive_begin", "oiva_batch_ogive_iterate")


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
    dict(X=_x(), update="both"),
    dict(X=_x(), update="Demix"),
    dict(X=_x(), model="cauchy"),
    dict(X=_x(), n_iter=-1),
    dict(X=_x(), W0=np.ones((5, 4, 2))),                # two columns
    dict(X=_x(), W0=np.ones((6, 4, 1))),                # wrong F
    dict(X=_x(), W0=np.ones((3, 5, 4, 1))),             # wrong B
    dict(X=_x(), W0=np.ones((2, 5, 3, 1))),             # wrong M
])
def test_ogive_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.ogive_batch(X, **bad)


def test_ogive_batch_has_no_source_count(no_device):
    with pytest.raises(TypeError):
        no_device.ogive_batch(_x(), n_src=1)


def test_ogive_batch_accepts_the_documented_w0_shapes():
    from overiva_amd import batch

    X = _x()
    for W0 in (np.ones((5, 4, 1)), np.ones((4, 1)), np.ones((5, 1, 1)), np.ones((2, 5, 4, 1)), None):
        batch._check_ogive_args(X, "demix", "laplace", W0, 3)


def test_ogive_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.ogive_batch(_x())


def test_ogive_batch_is_public():
    import overiva_amd

    assert "ogive_batch" in overiva_amd.__all__ and callable(overiva_amd.ogive_batch)
    assert "last_batch_info" in overiva_amd.__all__


def test_ogive_batch_symbols_declared_and_bound():
    from overiva_amd import _lib

    txt = open(HEADER).read()
    for name in OGIVE_BATCH_SYMBOLS:
        assert f" {name}(" in txt, name
        assert name in _lib.SIGNATURES, name


def test_ogive_batch_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in OGIVE_BATCH_SYMBOLS:
        assert hasattr(lib, name), name


def test_ogive_batch_golden_fixture():
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN) as d:
        g = {k: d[k] for k in d.files}
    T, F, M, S = (int(g[k]) for k in ("T", "F", "M", "S"))
    B = len(g["family"])
    assert 4 <= B <= 6 and set(g["family"]) == {"iid", "mix"}
    for b, (fam, seed) in enumerate(zip(g["family"], g["seed"])):
        X = orc.synth_iid(T, F, M, seed=int(seed)) if fam == "iid" else orc.synth_mixture(T, F, M, S, seed=int(seed))
        assert abs(X.astype(np.complex128).sum() - g["X_sum"][b]) < 1e-9
    for update in ("demix", "mix", "switching"):
        for model in ("laplace", "gauss"):
            assert g[f"W_{update}_{model}"].shape == (B, F, M, 1)
            assert g[f"amp_{update}_{model}"].shape == g[f"floor_{update}_{model}"].shape == (B,)
    assert g["W_stop"].shape == (B, F, M, 1)
    assert np.all((g["stop_epochs"] >= 1) & (g["stop_epochs"] <= int(g["stop_n_iter"])))
    assert len(set(g["stop_epochs"].tolist())) >= 2          # the problems stop at different epochs
    assert np.all(g["stop_margin"] > 1e-6)                   # no epoch's max ||delta|| sits on the tolerance
