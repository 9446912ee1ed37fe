"""CPU-side checks of the wide path (17..32 channels): the public limit, the errors raised before any device call, and the
arithmetic each channel count resolves to.  No GPU needed."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "overiva_hip.h")


def test_header_limit_is_32_channels():
    txt = open(HEADER).read()
    m = re.search(r"#define\s+OIVA_MAX_CHANNELS\s+(\d+)", txt)
    assert m and int(m.group(1)) == 32


def test_python_limit_matches_header():
    from overiva_amd.overiva import MAX_CHANNELS

    assert MAX_CHANNELS == 32


def _no_device(monkeypatch):
    """any attempt to reach the library fails the test"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", boom)


def test_overiva_33_channels_raises_before_any_device_call(monkeypatch):
    import overiva_amd as oa

    _no_device(monkeypatch)
    X = np.zeros((8, 3, 33), np.complex64)
    with pytest.raises(ValueError, match="1..32 channels"):
        oa.overiva(X, n_src=2, n_iter=1)
    with pytest.raises(ValueError, match="1..32 channels"):
        oa.overiva(X)


def test_auxiva_pca_33_channels_raises_before_any_device_call(monkeypatch):
    import overiva_amd as oa

    _no_device(monkeypatch)
    X = np.zeros((8, 3, 33), np.complex64)
    with pytest.raises(ValueError, match="1..32 channels"):
        oa.auxiva_pca(X, n_src=2, proj_back=True, n_iter=1)


def test_ogive_17_channels_raises_before_any_device_call(monkeypatch):
    import overiva_amd as oa

    _no_device(monkeypatch)
    X = np.zeros((8, 3, 17), np.complex64)
    with pytest.raises(ValueError, match="1..16 channels"):
        oa.ogive(X, n_iter=1)


@pytest.mark.parametrize("M", [17, 18, 23, 24, 31, 32])
def test_resolve_precision_wide(M):
    from overiva_amd.overiva import resolve_precision

    for T in (16, 235, 4000):
        assert resolve_precision(np.complex64, M, mode="auto", n_frames=T) == "mixed"
        assert resolve_precision(np.complex128, M, mode="auto", n_frames=T) == "precise"


WIDE_GOLDEN = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "wide_*.npz")))
AMP_LIMIT = 1e3          # as conftest.chaotic: where the reference itself amplifies a 1e-12 perturbation more, nothing is pinned


def test_wide_fixtures_exist():
    assert len(WIDE_GOLDEN) >= 5
    for path in WIDE_GOLDEN:
        assert os.path.getsize(path) < 1 << 20, path
        with np.load(path) as g:
            assert 17 <= int(g["M"]) <= 32


@pytest.mark.parametrize("path", WIDE_GOLDEN, ids=os.path.basename)
def test_oracle_reproduces_wide_fixtures(path):
    """oracle.overiva_faithful / auxiva_pca_faithful against the REAL reference's results at 17..32 channels
    (tests/golden/make_wide_golden.py): complex128 to 1e-9 wherever the reference is not chaotic, complex64 within its floor"""
    from oracle import overiva_oracle as orc

    with np.load(path) as d:
        g = {k: d[k] for k in d.files}
    X, K = g["X"], int(g["K"])
    X128 = X.astype(np.complex128)
    compared = 0
    for model in ("laplace", "gauss"):
        for n_iter in (1, 5, 20):
            if float(g[f"amp_{model}_{n_iter}"]) > AMP_LIMIT:
                continue
            for dt, Xin in (("c128", X128), ("c64", X)):
                key = f"{dt}_{model}_{n_iter}"
                if key in g["nonfinite"].tolist():
                    continue
                Y, W = orc.overiva_faithful(Xin, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True)
                if dt == "c128":
                    tol = 1e-9
                else:       # (complex64: as tests/test_oracle_golden.py -- within the distance of either complex64 run from
                    #          the complex128 result, the meaningful floor; BLAS paths differ in the last bits)
                    tol = max(2e-6, 4 * orc.rel_err(g[f"W_{key}"], g[f"W_c128_{model}_{n_iter}"]))
                assert orc.rel_err(W, g[f"W_{key}"]) < tol, key
                if f"Y_{key}" in g:
                    assert orc.rel_err(Y, g[f"Y_{key}"]) < tol, key
                compared += 1
    assert compared >= 8
    W = orc.overiva_faithful(X128, n_src=K, n_iter=3, proj_back=False, W0=g["W0"], return_filters=True)[1]
    assert orc.rel_err(W, g["W_w0_c128_laplace_3"]) < 1e-9
    if "Ypb_c128_laplace_12" in g:
        got = []
        Y = orc.overiva_faithful(X128, n_src=K, n_iter=12, proj_back=True, callback=lambda y: got.append(np.array(y)))
        assert orc.rel_err(Y, g["Ypb_c128_laplace_12"]) < 1e-9
        assert orc.rel_err(got[0], g["cb0_c128_laplace"]) < 1e-9 and orc.rel_err(got[1], g["cb10_c128_laplace"]) < 1e-9
    if "Ypca_c128_laplace_5" in g:
        Y = orc.auxiva_pca_faithful(X128, n_src=K, n_iter=5, proj_back=True, model="laplace")
        assert orc.rel_err(Y, g["Ypca_c128_laplace_5"]) < 1e-9
