"""separate_batch() / BatchSTFT without a GPU: argument validation raises before the library is touched, the new ABI entries are
declared as oiva_status, bound and exported, and check their arguments before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
NEW_SYMBOLS = ("oiva_bstft_create", "oiva_bstft_destroy", "oiva_bstft_shape", "oiva_bstft_analysis", "oiva_bstft_synthesis_dev",
               "oiva_bstft_phase_ms", "oiva_batch_demix_dev", "oiva_device_to_host")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _rooms(lens=(640, 512, 333), M=4, dtype=np.float32):
    return [np.ones((n, M), dtype) for n in lens]


def _dense(B=2, n=640, M=4, dtype=np.float32):
    return np.ones((B, n, M), dtype)


@pytest.mark.parametrize("bad", [
    dict(x=_dense(), frame=63),                                          # odd frame
    dict(x=_dense(), frame=0),
    dict(x=_dense(), frame=64, hop=65),                                  # hop > frame
    dict(x=_dense(), frame=64, hop=0),
    dict(x=_dense(), frame=64.0),
    dict(x=_rooms(lens=(640, 31, 333)), frame=64),                       # a room shorter than one hop
    dict(x=_dense(n=31), frame=64),
    dict(x=_rooms()[:2] + _rooms(M=3)[2:], frame=64),                    # rooms of different M
    dict(x=_rooms()[:2] + _rooms(dtype=np.float64)[2:], frame=64),       # mixed dtypes
    dict(x=_dense(dtype=np.complex64), frame=64),                        # complex input
    dict(x=_rooms(dtype=np.complex128), frame=64),
    dict(x=_dense(M=9), frame=64),                                       # 9 channels
    dict(x=_rooms(M=9), frame=64),
    dict(x=_rooms(), frame=64, algorithm="ogive"),                       # OGIVE with a sequence
    dict(x=_dense(), frame=64, algorithm="fastica"),                     # unknown algorithm
    dict(x=_dense(), frame=64, algorithm="ogive", n_src=2),
    dict(x=_dense(), frame=64, algorithm="ogive", update="both"),
    dict(x=_dense(), frame=64, step_size=0.1),                           # an OGIVE argument to overiva
    dict(x=_dense(), frame=64, algorithm="ogive", momentum=1.0),
    dict(x=[], frame=64),
    dict(x=_dense()[0], frame=64),                                       # ndim 2
    dict(x=[r[:, 0] for r in _rooms()], frame=64),                       # a room of ndim 1
    dict(x=_dense(), frame=64, n_src=5),
    dict(x=_dense(), frame=64, n_src=0),
    dict(x=_dense(), frame=64, model="student"),
    dict(x=_dense(), frame=64, n_iter=-1),
    dict(x=_dense(), frame=64, win_a=np.ones(32)),                       # window lengths
    dict(x=_dense(), frame=64, win_s=np.ones(65)),
    dict(x=_dense(), frame=64, W0=np.ones((33, 4, 3))),                  # K = 4 (default): wrong K
    dict(x=_dense(), frame=64, n_src=2, W0=np.ones((3, 33, 4, 2))),      # wrong B
    dict(x=_rooms(), frame=64, n_src=2, W0=np.ones((3, 32, 4, 2))),      # wrong F
])
def test_separate_validation_before_device(no_device, bad):
    x = bad.pop("x")
    with pytest.raises(ValueError):
        no_device.separate_batch(x, **bad)


def test_separate_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.separate_batch(_dense(), 64, n_src=2)


def test_separate_accepts_the_documented_arguments():
    """the checker alone (no library): defaults of hop and the windows, the W0 shapes, float64 and integer audio"""
    from overiva_amd import separate, stft

    r = separate._check_separate_args(_rooms(), 64, None, 2, 20, "overiva", "laplace", None, None, None, {})
    rooms, ragged, lens, M, hop, K, wa, ws, out_dtype = r
    assert ragged and lens == [640, 512, 333] and (M, hop, K) == (4, 32, 2) and out_dtype == np.float32
    assert np.allclose(wa, stft.hann(64)) and np.allclose(ws, stft.compute_synthesis_window(stft.hann(64), 32))
    r = separate._check_separate_args(_dense(dtype=np.float64), 64, 64, None, 5, "ogive", "gauss", None, None, np.ones((2, 33, 4, 1)),
                                      dict(step_size=0.05, tol=1e-4, update="switching"))
    assert not r[1] and r[5] == 1 and r[6] is None and r[7] is None and r[8] == np.float64      # rectangular when hop == frame
    for W0 in (np.ones((33, 4, 2)), np.ones((4, 2)), np.ones((3, 33, 4, 2))):
        separate._check_separate_args(_rooms(), 64, 32, 2, 3, "overiva", "laplace", None, None, W0, {})
    separate._check_separate_args(_rooms(lens=(32, 32)), 64, 32, 2, 3, "overiva", "laplace", None, None, None, {})   # exactly one hop


@pytest.mark.parametrize("bad", [
    dict(n_samples=640, M=4, frame=64, hop=32),                          # an int without B
    dict(n_samples=640, M=4, frame=64, hop=32, B=0),
    dict(n_samples=[640, 640], M=4, frame=64, hop=32, B=3),
    dict(n_samples=[640, 31], M=4, frame=64, hop=32),
    dict(n_samples=[640], M=9, frame=64, hop=32),
    dict(n_samples=[640], M=4, frame=63, hop=32),
    dict(n_samples=[640], M=4, frame=64, hop=32, win_a=np.ones(63)),
    dict(n_samples=[], M=4, frame=64, hop=32),
])
def test_batch_stft_validation_before_device(no_device, bad):
    with pytest.raises(ValueError):
        no_device.BatchSTFT(**bad)


def test_separate_is_public():
    import overiva_amd

    for name in ("separate_batch", "BatchSTFT"):
        assert name in overiva_amd.__all__ and callable(getattr(overiva_amd, name))
    assert callable(overiva_amd.BatchPlan.demix_device) and callable(overiva_amd.RaggedBatchPlan.demix_device)


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


@pytest.mark.parametrize("B, n_samples, M, frame, hop", [
    (2, None, 4, 64, 32),                       # null n_samples
    (0, [640], 4, 64, 32),                      # B < 1
    (-1, [640], 4, 64, 32),
    (2, [640, 31], 4, 64, 32),                  # a room shorter than a hop
    (2, [640, 0], 4, 64, 32),
    (1, [640], 4, 63, 32),                      # odd frame
    (1, [640], 4, 0, 1),
    (1, [640], 4, 64, 0),                       # hop outside 1..frame
    (1, [640], 4, 64, 65),
    (1, [640], 0, 64, 32),                      # M outside 1..8
    (1, [640], 9, 64, 32),
    (1, [2_000_000_000], 8, 64, 32),            # 2^31 elements of audio in a room
    (1, [1 << 30], 1, 4096, 1),                 # 2^31 elements of frames in a room (2^42 floats)
    (2, [640, 1 << 30], 1, 4096, 1),
])
def test_bstft_create_checks_arguments_before_device_use(B, n_samples, M, frame, hop):
    """on a machine without a GPU any device call fails with OIVA_ERR_HIP: OIVA_ERR_ARG shows the check came first"""
    from overiva_amd import _lib

    lib = _built_lib()
    h = ctypes.c_void_p()
    ns = None if n_samples is None else (ctypes.c_int * len(n_samples))(*n_samples)
    rc = lib.oiva_bstft_create(ctypes.byref(h), 0, B, ns, M, frame, hop, None, None, None)
    assert rc == _lib.ERR_ARG, (rc, lib.oiva_last_error())
    assert not h.value
    assert lib.oiva_bstft_create(None, 0, 1, (ctypes.c_int * 1)(640), 4, 64, 32, None, None, None) == _lib.ERR_ARG    # null out


def test_null_handles_and_pointers_are_argument_errors():
    from overiva_amd import _lib

    lib = _built_lib()
    buf = (ctypes.c_float * 8)()
    dev = ctypes.c_void_p()
    n = ctypes.c_int()
    assert lib.oiva_bstft_shape(None, None, ctypes.byref(n)) == _lib.ERR_ARG
    assert lib.oiva_bstft_analysis(None, buf, ctypes.byref(dev)) == _lib.ERR_ARG
    assert lib.oiva_bstft_synthesis_dev(None, buf, 1, buf) == _lib.ERR_ARG
    assert lib.oiva_bstft_phase_ms(None, buf) == _lib.ERR_ARG
    assert lib.oiva_batch_demix_dev(None, 1, ctypes.byref(dev)) == _lib.ERR_ARG
    assert lib.oiva_batch_demix_dev(None, 1, None) == _lib.ERR_ARG
    assert lib.oiva_device_to_host(None, buf, 8) == _lib.ERR_ARG
    assert lib.oiva_device_to_host(buf, None, 8) == _lib.ERR_ARG
    assert lib.oiva_device_to_host(buf, buf, -1) == _lib.ERR_ARG
    assert lib.oiva_bstft_destroy(None) == _lib.OK
