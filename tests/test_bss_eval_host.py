"""bss_eval_batch() / bss_eval_sources() without a GPU: every refusal comes before the library is touched, the ABI is declared, bound
and exported, the permutation rule holds on hand-made SIR matrices, and the NumPy restatement the GPU tests compare against
(tests/helpers/bss_eval_oracle.py) agrees with itself on every case closely enough to be the yardstick."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import bss_eval_cases as cases  # noqa: E402
import bss_eval_oracle as bso  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_bsseval_create", "oiva_bsseval_destroy", "oiva_bsseval_groups", "oiva_bsseval_set_signals", "oiva_bsseval_stage",
           "oiva_bsseval_run", "oiva_bsseval_get_gram", "oiva_bsseval_get_filters", "oiva_bsseval_get_criteria", "oiva_bsseval_status",
           "oiva_bsseval_time_stages")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _sig(B=2, N=2, n=50, seed=0):
    return np.random.default_rng(seed).standard_normal((B, N, n))


def _with(a, index, value):
    a = a.copy()
    a[index] = value
    return a


@pytest.mark.parametrize("bad", [
    dict(ref=_sig()[0], est=_sig()[0]),                                  # rank 2 given to the batched call
    dict(ref=_sig()[None], est=_sig()[None]),                            # rank 4
    dict(ref=_sig(), est=_sig(n=49)),                                    # mismatched lengths
    dict(ref=_sig(), est=_sig(N=3)),                                     # mismatched source counts
    dict(ref=_sig(), est=_sig(B=3)),                                     # mismatched batches
    dict(ref=_sig(), est=list(_sig())),                                  # an array against a sequence
    dict(ref=_sig(N=9), est=_sig(N=9)),                                  # 9 sources
    dict(ref=_sig(N=0), est=_sig(N=0)),                                  # no source
    dict(ref=_sig(), est=_sig(), filter_length=0),
    dict(ref=_sig(), est=_sig(), filter_length=513),
    dict(ref=_sig(), est=_sig(), filter_length=True),
    dict(ref=_sig(), est=_sig(), filter_length=32.0),
    dict(ref=_sig().astype(np.complex128), est=_sig()),                  # complex
    dict(ref=_sig(), est=_sig() + 0j),
    dict(ref=_with(_sig(), (1, 0, 7), np.nan), est=_sig()),              # non-finite
    dict(ref=_sig(), est=_with(_sig(), (0, 1, 3), np.inf)),
    dict(ref=_with(_sig(), (1, 1), 0.0), est=_sig()),                    # an all-zero reference
    dict(ref=_sig(), est=_with(_sig(), (0, 0), 0.0)),                    # an all-zero estimate
    dict(ref=_sig(B=0), est=_sig(B=0)),                                  # empty batch
    dict(ref=[], est=[]),
    dict(ref=_sig(n=0), est=_sig(n=0)),                                  # no samples
    dict(ref=[_sig()[0], _sig(N=3)[0]], est=[_sig()[0], _sig(N=3)[0]]),  # source counts differ between rooms
    dict(ref=[_sig()[0], _sig()[0][0]], est=[_sig()[0], _sig()[0][0]]),  # a room of rank 1
])
def test_validation_before_device(no_device, bad):
    ref, est = bad.pop("ref"), bad.pop("est")
    with pytest.raises(ValueError):
        no_device.bss_eval_batch(ref, est, **bad)


@pytest.mark.parametrize("bad", [
    dict(ref=_sig(), est=_sig()),                                        # a batch given to the one-room call
    dict(ref=_sig()[0], est=_sig()[0], filter_length=0),
    dict(ref=_sig()[0], est=_sig(n=40)[0]),
    dict(ref=_with(_sig()[0], (0,), 0.0), est=_sig()[0]),
])
def test_one_room_validation_before_device(no_device, bad):
    ref, est = bad.pop("ref"), bad.pop("est")
    with pytest.raises(ValueError):
        no_device.bss_eval_sources(ref, est, **bad)


def test_refused_under_bin_sharding(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: object())
    with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
        no_device.bss_eval_batch(_sig(), _sig())


def test_symbols_declared_bound_and_exported():
    import overiva_amd
    from overiva_amd import _lib, build, metrics

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_bsseval_")} == set(SYMBOLS)
    assert "kernels_bsseval.hip" in build.SOURCES and "bsseval.hip" in build.SOURCES
    for name in ("bss_eval_batch", "bss_eval_sources"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(metrics, name)
    assert "not pinned" in metrics.__doc__
    assert "lstsq" in metrics.bss_eval_batch.__doc__
    assert issubclass(metrics.BssEval, _lib.Handle)
    for method in ("set_signals", "correlate", "factor", "solve", "criteria", "get_gram", "get_filters", "status", "time_stages"):
        assert callable(getattr(metrics.BssEval, method))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_restatement_is_a_yardstick(case):
    """its two forms agree, it is reproducible, and 10 x its spread is <= 1e-6 dB on every room of every case"""
    kind, B, N, n, Lf = case
    run = cases.oracle_run(case)
    ref, est = cases.make_case(case)
    assert np.array_equal(ref, run["ref"]) and np.array_equal(est, run["est"])
    again = bso.bss_eval_td(ref[0], est[0], Lf)
    for a, b in zip(again, run["rooms"][0]["td"]):
        assert np.array_equal(a, b)
    for b, room in enumerate(run["rooms"]):
        print(f"{cases.case_id(case)} room {b}: delta {room['delta']:.2e} dB, forms {room['forms']:.2e} dB")
        assert room["yardstick"] > 0.0
        assert cases.FACTOR * room["yardstick"] <= cases.ADMIT_DB
        assert np.all(np.isfinite(room["td"][0])) and np.all(np.isfinite(room["td"][2]))


def test_one_source_has_infinite_sir():
    ref, est = cases.make_room("white", 1, 300, 3)
    for form in (bso.bss_eval_td, bso.bss_eval_gram):
        sdr, sir, sar = form(ref, est, 8)
        assert np.isposinf(sir).all() and np.isfinite(sdr).all() and np.isfinite(sar).all()


@pytest.mark.parametrize("sir,want", [
    ([[10., 0.], [0., 10.]], [0, 1]),
    ([[0., 10.], [10., 0.]], [1, 0]),
    ([[5., 5.], [5., 5.]], [0, 1]),                                       # a tie: the first permutation
    ([[1., 9., 0.], [0., 1., 9.], [9., 0., 1.]], [2, 0, 1]),              # perm[j] = the estimate of reference j
    ([[3., 3., 0.], [3., 3., 0.], [0., 0., 3.]], [0, 1, 2]),              # a tie between (0,1,2) and (1,0,2)
    ([[9., 0., 0.], [0., 2., 4.], [0., 4., 2.]], [0, 2, 1]),
    ([[np.inf]], [0]),
])
def test_permutation_rule(sir, want):
    from overiva_amd.metrics import best_permutation

    sir = np.array(sir)
    got = best_permutation(sir)
    assert list(got) == want
    assert list(bso.best_permutation(sir)) == want
    N = len(want)
    import itertools

    means = [np.mean(sir[list(p), np.arange(N)]) for p in itertools.permutations(range(N))]
    assert np.mean(sir[got, np.arange(N)]) == max(means)
    assert list(itertools.permutations(range(N)))[int(np.argmax(means))] == tuple(want)
