"""The complex128 data path of the batched solver (``data="complex128"``) without a GPU: the new symbols are declared, bound and
exported, every refusal comes before the library is touched, the new kernels use no scratch memory, the oracle reproduces the
new fixtures (tests/golden/c128_*.npz) -- so they are the reference's and not the oracle's --, and the cap on skipped rows holds."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import overiva_oracle as orc

from helpers.c128_cases import GOLDEN, HEADER, admitted, load_case, mk

SYMBOLS = ("oiva_batch_set_data_c128", "oiva_batch_c128_get_weights", "oiva_batch_c128_get_cov")
KERNELS = ("c128_power_kernel", "c128_activation_kernel", "c128_finalize_kernel", "c128_cov_kernel", "c128_projback_kernel",
           "c128_demix_kernel")
TOL = 1e-9


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def test_symbols_declared_bound_and_exported():
    import ctypes

    from overiva_amd import _lib, build

    build.build_library()
    header = open(HEADER).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in SYMBOLS:
        assert re.search(r"oiva_status\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
        assert hasattr(lib, sym), sym
    assert "kernels_batch_c128.hip" in build.SOURCES
    loaded = _lib.load()
    for sym in SYMBOLS:         # a null batch is an argument error, not a crash
        assert getattr(loaded, sym)(*([None] * len(_lib.SIGNATURES[sym]))) == _lib.ERR_ARG, sym


def test_new_kernels_use_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_batch_c128",))
    for k in KERNELS:
        assert any(k in name for name in usage), (k, sorted(usage))
    assert all(any(k in name for k in KERNELS) for name in usage), sorted(usage)
    assert [name for name, u in usage.items() if u["scratch"] != 0] == []


@pytest.mark.parametrize("dtype", [np.complex64, np.float64, np.float32])
def test_complex128_data_needs_complex128_input(no_device, dtype):
    X = np.ones((2, 16, 5, 4), dtype)
    with pytest.raises(ValueError, match=np.dtype(dtype).name):
        no_device.overiva_batch(X, n_src=2, data="complex128")
    with pytest.raises(ValueError, match=np.dtype(dtype).name):
        no_device.overiva_batch_ragged([X[0], X[1, :9]], n_src=2, data="complex128")


def test_unknown_data_mode_and_the_usual_checks_come_first(no_device):
    X = np.ones((2, 16, 5, 4), np.complex128)
    for bad in ("float64", "c128", None, 128):
        with pytest.raises(ValueError, match="data must be"):
            no_device.overiva_batch(X, n_src=2, data=bad)
        with pytest.raises(ValueError, match="data must be"):
            no_device.overiva_batch_ragged(list(X), n_src=2, data=bad)
        with pytest.raises(ValueError, match="data must be"):
            no_device.BatchPlan(2, 16, 5, 4, 2, data=bad)
        with pytest.raises(ValueError, match="data must be"):
            no_device.RaggedBatchPlan([16, 9], 5, 4, 2, data=bad)
    with pytest.raises(ValueError):
        no_device.overiva_batch(X, n_src=5, data="complex128")
    with pytest.raises(ValueError):
        no_device.overiva_batch(np.ones((2, 16, 5, 9), np.complex128), data="complex128")


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


@pytest.mark.parametrize("ragged", [False, True])
def test_plan_refusals_come_before_the_library(ragged):
    """OGIVE, ILRMA, the PCA entry points and demix_device say "complex128" on a complex128 plan; set_x names the dtype"""
    from overiva_amd import batch

    cls = batch.RaggedBatchPlan if ragged else batch.BatchPlan
    p = cls.__new__(cls)
    p.lib, p.h, p.data = _Untouchable(), None, "complex128"
    p.frames, p.offsets = [16, 16], np.array([0, 16, 32])
    p.B, p.T, p.F, p.M, p.K = 2, 16, 5, 4, 4
    other = cls.__new__(cls)
    other.lib, other.h, other.data, other.B, other.T, other.F, other.M, other.K = _Untouchable(), None, "complex64", 2, 16, 5, 4, 4
    other.frames = [16, 16]
    calls = [lambda: p.set_w_pca(), lambda: p.project_device(), lambda: p.compose_w(other), lambda: other.compose_w(p),
             lambda: p.demix_device()]
    if not ragged:        # (a ragged plan refuses these for being ragged)
        calls += [lambda: p.ogive_begin(), lambda: p.ogive_iterate(0, 1), lambda: p.ilrma_begin(np.ones((2, 4, 5, 2)), np.ones((2, 4, 2, 16))),
                  lambda: p.ilrma_iterate(), lambda: p.ilrma_stage(0)]
    for call in calls:
        with pytest.raises(ValueError, match="complex128"):
            call()
    X = np.ones(p.shape, np.complex64)
    with pytest.raises(ValueError, match="complex64"):
        p.set_x(X)
    if ragged:
        with pytest.raises(ValueError, match="complex64"):
            p.set_x([X[:16], X[16:]])
    assert p.info()["data"] == "complex128" and other.info()["data"] == "complex64"


def test_documents_speak_of_the_mode():
    import overiva_amd
    from overiva_amd import batch

    for doc in (batch.__doc__, batch.BatchPlan.__doc__, sys.modules[overiva_amd.overiva.__module__].__doc__):
        assert 'data="complex128"' in doc
    for doc in (batch.overiva_batch.__doc__, batch.overiva_batch_ragged.__doc__):
        assert '"complex128"' in doc


def test_the_cap_on_skipped_rows_holds():
    """every laplace row and every gauss row at 1, 5 (and 12) iterations is admitted: only gauss at 20 may drop out"""
    assert len(GOLDEN) == 13
    dropped = []
    for path in GOLDEN:
        assert os.path.getsize(path) < 1 << 20
        with np.load(path) as d:
            g = {k: d[k] for k in d.files}
        for model in mk.MODELS:
            for n in (1, 5, 12, 20):
                if not admitted(g, model, n):
                    dropped.append((os.path.basename(path), model, n))
    print(dropped)
    assert all(model == "gauss" and n == 20 for _, model, n in dropped), dropped
    assert sorted(d[0] for d in dropped) == ["c128_100x65x3x2_mix.npz", "c128_129x16x7x3_iid.npz", "c128_257x20x8x4_mix.npz",
                                             "c128_64x130x4x2_mix.npz"], dropped


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[5:-4])
def test_oracle_reproduces_the_fixtures(path):
    g, X, K = load_case(path)
    rows = g["rows"]
    for model in mk.MODELS:
        for n in mk.N_ITERS:
            if not admitted(g, model, n):
                continue
            Y, W = orc.overiva_faithful(X, n_src=K, n_iter=n, proj_back=False, model=model, return_filters=True)
            assert orc.rel_err(W, g[f"W_{model}_{n}"]) < TOL, (model, n)
            if n == 20:
                assert orc.rel_err(Y[rows], g[f"Yrows_{model}_20"]) < TOL, model
        if admitted(g, model, 12):
            Y = orc.overiva_faithful(X, n_src=K, n_iter=12, proj_back=True, model=model)
            assert orc.rel_err(Y[rows], g[f"Ypbrows_{model}_12"]) < TOL, model
        # rounding X to complex64 moves the reference's own result past the bound (2.8e-9 at the least): the fixture separates the two paths
        assert orc.rel_err(g[f"W_rounded_{model}_20"], g[f"W_{model}_20"]) > 2 * TOL
