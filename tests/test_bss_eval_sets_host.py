"""bss_eval_sets_batch() / bss_eval_sets() / BssEvalSets without a GPU: every refusal comes before the library is touched (in
Python) or before a device call (in the library: without a GPU any device call gives ERR_HIP, so ERR_ARG shows the order), the ABI
is declared, bound and exported, and the kernels use no scratch memory."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import bss_sets_cases as sets_cases  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_bsssets_create", "oiva_bsssets_destroy", "oiva_bsssets_set_references", "oiva_bsssets_set_estimates",
           "oiva_bsssets_take", "oiva_bsssets_prepare", "oiva_bsssets_evaluate", "oiva_bsssets_get_criteria", "oiva_bsssets_status",
           "oiva_bsssets_get_gram", "oiva_bsssets_get_filters", "oiva_bsssets_counts", "oiva_bsssets_phase_ms")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import _lib

    return _lib.load()


def _ref(B=2, N=2, n=50, seed=0):
    return np.random.default_rng(seed).standard_normal((B, N, n))


def _est(B=2, E=2, N=2, n=50, seed=1):
    return np.random.default_rng(seed).standard_normal((B, E, N, n))


def _with(a, index, value):
    a = a.copy()
    a[index] = value
    return a


@pytest.mark.parametrize("bad", [
    dict(ref=_ref(), est=_est()[:, 0]),                                   # rank 3 estimates
    dict(ref=_ref(), est=_est()[None]),                                   # rank 5
    dict(ref=_ref(), est=_est(E=0)),                                      # n_sets = 0
    dict(ref=list(_ref()), est=[_est()[0], _est(E=3)[1]]),                # set counts differ between rooms
    dict(ref=_ref(), est=_est(n=49)),                                     # a set whose shape disagrees with the references
    dict(ref=_ref(), est=_est(N=3)),
    dict(ref=_ref(), est=_est(B=3)),
    dict(ref=_ref(N=9), est=_est(N=9)),                                   # 9 sources
    dict(ref=_ref(), est=_est(), filter_length=0),
    dict(ref=_ref(), est=_est(), filter_length=513),
    dict(ref=_ref(), est=_est(), filter_length=32.0),
    dict(ref=_ref().astype(np.complex128), est=_est()),                   # complex
    dict(ref=_ref(), est=_est() + 0j),
    dict(ref=_with(_ref(), (1, 0, 7), np.nan), est=_est()),               # non-finite
    dict(ref=_ref(), est=_with(_est(), (0, 1, 1, 3), np.inf)),
    dict(ref=_ref(), est=_with(_est(), (0, 1, 0), 0.0)),                  # an all-zero estimate in set 1 only
    dict(ref=_ref(B=0), est=_est(B=0)),                                   # empty batch
    dict(ref=[], est=[]),
    dict(ref=_ref(), est=list(_est())),                                   # an array given against a sequence
    dict(ref=list(_ref()), est=_est()),
    dict(ref=_ref(), est=_est(), max_group=-1),
    dict(ref=_ref(), est=_est(), max_group=1.0),
])
def test_validation_before_device(no_device, bad):
    ref, est = bad.pop("ref"), bad.pop("est")
    with pytest.raises(ValueError):
        no_device.bss_eval_sets_batch(ref, est, **bad)


def test_the_set_is_named_in_the_refusal(no_device):
    with pytest.raises(ValueError, match=r"^set 1: room 0: estimated source\(s\) 0 are all zeros"):
        no_device.bss_eval_sets_batch(_ref(), _with(_est(), (0, 1, 0), 0.0))


@pytest.mark.parametrize("bad", [
    dict(ref=_ref(), est=_est()),                                         # a batch given to the one-room call
    dict(ref=_ref()[0], est=_est()[0][0]),                                # one set without the set axis
    dict(ref=_ref()[0], est=_est()[0], filter_length=0),
    dict(ref=_ref()[0], est=_est(n=40)[0]),
])
def test_one_room_validation_before_device(no_device, bad):
    ref, est = bad.pop("ref"), bad.pop("est")
    with pytest.raises(ValueError):
        no_device.bss_eval_sets(ref, est, **bad)


def test_refused_under_bin_sharding(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: object())
    with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
        no_device.bss_eval_sets_batch(_ref(), _est())


def test_the_helper_shares_references_and_varies_the_sets():
    refs, sets = sets_cases.make_rooms("ar", 3, [300, 301], 3)
    assert [r.shape for r in refs] == [(3, 300), (3, 301)] and [s.shape for s in sets] == [(3, 3, 300), (3, 3, 301)]
    again = sets_cases.make_rooms("ar", 3, [300, 301], 3)
    assert all(sets_cases.same_bits(a, b) for a, b in zip(sets, again[1]))
    assert not np.array_equal(sets[0][0], sets[0][1]) and not np.array_equal(sets[0][1], sets[0][2])


def test_symbols_declared_bound_and_exported(lib):
    import overiva_amd
    from overiva_amd import _lib, build, metrics

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"oiva_status\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
        assert getattr(lib, sym).restype is C.c_int
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_bsssets_")} == set(SYMBOLS)
    assert "kernels_bsseval.hip" in build.SOURCES and "bsseval.hip" in build.SOURCES
    for name in ("BssEvalSets", "bss_eval_sets_batch", "bss_eval_sets"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(metrics, name)
        assert name in overiva_amd.__doc__
    assert issubclass(metrics.BssEvalSets, _lib.Handle)
    for method in ("set_references", "set_estimates", "take", "prepare", "evaluate", "get_criteria", "status", "get_gram",
                   "get_filters", "counts", "phase_ms", "info"):
        assert callable(getattr(metrics.BssEvalSets, method))


def test_sets_kernels_use_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_bsseval",))
    names = " ".join(usage)
    for kernel in ("bss_lag_kernel", "bss_lag_sum_kernel", "bss_assemble_kernel", "bss_init_rhs_kernel", "bss_trsv_kernel",
                   "bss_quad_kernel", "bss_criteria_kernel", "bss_chol_diag_kernel", "bss_chol_panel_kernel", "bss_chol_update_kernel"):
        assert kernel in names, kernel
    # the eight lag instantiations, forward and backward substitution, the large and the small quadratic forms
    assert len(usage) == 8 + 1 + 1 + 1 + 2 + 2 + 1 + 3
    for name, u in usage.items():
        assert u["scratch"] == 0, (name, u)


def test_null_handles_and_pointers(lib):
    from overiva_amd import _lib

    x = np.zeros(4)
    p = _lib.ptr(x)
    out = C.c_void_p()
    one = C.c_void_p(8)           # a handle that is not null: never followed, a null argument is met first
    ns = (C.c_int * 2)(50, 50)
    ll = C.c_longlong()
    assert lib.oiva_bsssets_destroy(None) == _lib.OK
    assert lib.oiva_bsssets_create(None, 0, 2, ns, 2, 8, 0, 1, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_create(C.byref(out), 0, 2, None, 2, 8, 0, 1, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_set_references(None, p) == lib.oiva_bsssets_set_references(one, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_set_estimates(None, 0, p) == lib.oiva_bsssets_set_estimates(one, 0, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_take(None, one, 0, 0) == lib.oiva_bsssets_take(one, None, 0, 0) == _lib.ERR_ARG
    assert lib.oiva_bsssets_prepare(None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_evaluate(None, 0, 1) == _lib.ERR_ARG
    assert lib.oiva_bsssets_get_criteria(None, 0, 1, p, p, p) == _lib.ERR_ARG
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.oiva_bsssets_get_criteria(one, 0, 1, *args) == _lib.ERR_ARG
    assert lib.oiva_bsssets_status(None, (C.c_int * 2)()) == lib.oiva_bsssets_status(one, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_get_gram(None, 0, p, p, p) == _lib.ERR_ARG
    assert lib.oiva_bsssets_get_gram(one, 0, p, None, p) == lib.oiva_bsssets_get_gram(one, 0, p, p, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_get_filters(None, 0, p, p) == _lib.ERR_ARG
    assert lib.oiva_bsssets_get_filters(one, 0, None, p) == lib.oiva_bsssets_get_filters(one, 0, p, None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_counts(None, C.byref(ll), C.byref(ll)) == _lib.ERR_ARG
    assert lib.oiva_bsssets_counts(one, None, C.byref(ll)) == lib.oiva_bsssets_counts(one, C.byref(ll), None) == _lib.ERR_ARG
    assert lib.oiva_bsssets_phase_ms(None, (C.c_float * 4)()) == lib.oiva_bsssets_phase_ms(one, None) == _lib.ERR_ARG


def test_create_checks_its_arguments_before_the_device(lib):
    from conftest import has_gpu
    from overiva_amd import _lib

    h = C.c_void_p()
    ns = (C.c_int * 2)(50, 60)
    good = dict(B=2, ns=ns, N=2, Lf=8, max_sets=3)
    for change in (dict(B=0), dict(N=0), dict(N=9), dict(Lf=0), dict(Lf=513), dict(max_sets=0), dict(max_sets=-1),
                   dict(max_sets=65536), dict(ns=(C.c_int * 2)(50, 0)), dict(ns=(C.c_int * 2)(50, 2 ** 31 - 1))):
        a = dict(good, **change)
        rc = lib.oiva_bsssets_create(C.byref(h), 0, a["B"], a["ns"], a["N"], a["Lf"], 0, a["max_sets"], None)
        assert rc == _lib.ERR_ARG and not h.value, change
    if not has_gpu():      # the control: arguments in order reach the device, which is not there
        assert lib.oiva_bsssets_create(C.byref(h), 0, 2, ns, 2, 8, 0, 3, None) == _lib.ERR_HIP and not h.value


def test_the_handle_checks_its_arguments_before_the_library(no_device):
    from overiva_amd.metrics import BssEvalSets

    for args, kw in ((([], 2), {}), (([50, 0], 2), {}), (([50], 9), {}), (([50], 0), {}), (([50], 2), dict(filter_length=513)),
                     (([50], 2), dict(filter_length=0)), (([50], 2), dict(max_sets=0))):
        with pytest.raises(ValueError):
            BssEvalSets(*args, **kw)
