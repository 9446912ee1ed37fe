"""ilrma_batch() / ilrma() without a GPU: every refusal comes before the library is touched, the ABI is declared and bound, the
default start is reproducible from ``seed``, and the NumPy restatement the GPU tests compare against (tests/helpers/ilrma_oracle.py)
has the two properties those tests lean on: a cost that never rises, and the same result stage-wise and interleaved per source."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import ilrma_cases as cases  # noqa: E402
import ilrma_oracle as ilo  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
ILRMA_SYMBOLS = ("oiva_batch_ilrma_begin", "oiva_batch_ilrma_iterate", "oiva_batch_ilrma_stage", "oiva_batch_ilrma_get_nmf",
                 "oiva_batch_ilrma_get_pr")


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _x(B=2, T=16, F=5, M=3):
    return (np.ones((B, T, F, M)) + 1j).astype(np.complex64)


def _pos(*shape):
    return np.full(shape, 0.5)


def _with(a, index, value):
    a = a.copy()
    a[index] = value
    return a


@pytest.mark.parametrize("bad", [
    dict(X=_x()[0]),                                        # ndim 3
    dict(X=_x()[None]),                                     # ndim 5
    dict(X=_x(M=9)),                                        # 9 channels
    dict(X=_x().real),                                      # not complex
    dict(X=_x(), n_src=2),                                  # overdetermined
    dict(X=_x(), n_src=4),
    dict(X=_x(), n_src=True),
    dict(X=_x(), n_iter=-1),
    dict(X=_x(), n_components=0),
    dict(X=_x(), n_components=17),
    dict(X=_x(), n_components=2.0),
    dict(X=_x(), W0=np.ones((5, 3, 2))),                    # K != M
    dict(X=_x(), W0=np.ones((6, 3, 3))),                    # wrong F
    dict(X=_x(), W0=np.ones((3, 5, 3, 3))),                 # wrong B
    dict(X=_x(), T0=_pos(2, 3, 5, 3)),                      # L = 3 against n_components = 2
    dict(X=_x(), T0=_pos(3, 5, 2)),                         # no batch axis
    dict(X=_x(), V0=_pos(2, 3, 2, 15)),                     # wrong T
    dict(X=_x(), T0=_with(_pos(2, 3, 5, 2), (1, 2, 4, 1), 0.0)),
    dict(X=_x(), T0=_with(_pos(2, 3, 5, 2), (0, 0, 0, 0), -1.0)),
    dict(X=_x(), V0=_with(_pos(2, 3, 2, 16), (1, 0, 1, 7), np.nan)),
    dict(X=_x(), V0=_with(_pos(2, 3, 2, 16), (1, 0, 1, 7), np.inf)),
])
def test_ilrma_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises((ValueError, TypeError)):
        no_device.ilrma_batch(X, **bad)


@pytest.mark.parametrize("bad", [
    dict(X=_x()),                                           # a batch given to the one-room call
    dict(X=_x()[0], n_src=2),
    dict(X=_x()[0], W0=np.ones((1, 5, 3, 3))),              # a batch of starts
    dict(X=_x()[0], T0=_pos(2, 3, 5, 2)),                   # a batch axis on T0
    dict(X=_x()[0], V0=_pos(3, 2, 15)),
])
def test_ilrma_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.ilrma(X, **bad)


def test_ilrma_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.ilrma_batch(_x())


def test_ragged_plan_refuses_ilrma_before_the_library():
    """the refusal is the class's: no handle is needed to get it"""
    from overiva_amd import RaggedBatchPlan

    plan = RaggedBatchPlan.__new__(RaggedBatchPlan)
    for call in (lambda: plan.ilrma_begin(None, None), lambda: plan.ilrma_iterate(1), lambda: plan.ilrma_stage(0), plan.get_nmf,
                 plan.get_pr):
        with pytest.raises(ValueError, match="ragged"):
            call()


def test_ilrma_is_public():
    import overiva_amd

    for name in ("ilrma_batch", "ilrma"):
        assert name in overiva_amd.__all__ and callable(getattr(overiva_amd, name))
    # the contract is the algorithm as the project states it, and the module says so
    assert "not pinned" in sys.modules["overiva_amd.ilrma"].__doc__


def test_ilrma_symbols_declared_and_bound():
    from overiva_amd import _lib

    txt = open(HEADER).read()
    for name in ILRMA_SYMBOLS:
        assert f" {name}(" in txt, name
        assert name in _lib.SIGNATURES, name


def test_ilrma_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ILRMA_SYMBOLS:
        assert hasattr(lib, name), name


def test_stage_names_follow_the_header():
    """``BatchPlan.ilrma_stage`` takes the names of ``ILRMA_STAGES``: their order is the header's enumeration"""
    import re

    from overiva_amd import batch

    txt = open(HEADER).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"OIVA_ILRMA_STAGE_([A-Z]+) = (\d+)", txt)}
    assert values == {"T": 0, "V": 1, "R": 2, "COV": 3, "UPDATE": 4, "POWER": 5, "NORMALISE": 6}
    assert batch.ILRMA_STAGES == ("t_update", "v_update", "r_rewrite", "weighted_cov", "ip_update", "power", "normalise")


def test_default_init_is_the_documented_recipe():
    from overiva_amd.ilrma import default_nmf_init

    B, T, F, M, L = 3, 7, 5, 2, 4
    T0, V0 = default_nmf_init(B, T, F, M, L, seed=5)
    rng = np.random.RandomState(5)
    assert np.array_equal(T0, 0.1 + 0.9 * rng.rand(B, M, F, L))
    assert np.array_equal(V0, 0.1 + 0.9 * rng.rand(B, M, L, T))
    again = default_nmf_init(B, T, F, M, L, seed=5)
    assert np.array_equal(T0, again[0]) and np.array_equal(V0, again[1])
    other = default_nmf_init(B, T, F, M, L, seed=6)
    assert not np.array_equal(T0, other[0])
    assert T0.min() >= 0.1 and T0.max() < 1.0 and V0.min() >= 0.1 and V0.max() < 1.0
    # the oracle's helper is the same recipe
    assert all(np.array_equal(a, b) for a, b in zip((T0, V0), ilo.default_init(B, T, F, M, L, seed=5)))


def _longest_cases():
    """every (kind, shape) of the iterated comparisons at its largest epoch count"""
    longest = {}
    for kind, shape, n in cases.ITERATED:
        longest[(kind, shape)] = max(n, longest.get((kind, shape), 0))
    return sorted(longest)


@pytest.mark.parametrize("kind,shape", _longest_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_oracle_cost_never_rises(kind, shape):
    """Q = sum(P / R + log R) - 2 T sum_f log|det W_f| over 20 epochs at the shapes of the iterated tests: no step 1 (NMF) or
    step 3 (IP1) raises it by more than 1e-12 relative, and step 4 (the normalisation) moves it by at most that either way"""
    T, F, M, L = shape
    X = cases.make_x(kind, T, F, M)
    T0, V0 = cases.make_nmf(T, F, M, L)
    trace = []
    ilo.ilrma(X, 20, T0[0], V0[0], observe=lambda step, P, R, W: trace.append((step, ilo.cost(P, R, W))))
    assert len(trace) == 1 + 3 * 20 and all(np.isfinite(q) for _, q in trace)
    for (_, before), (step, after) in zip(trace[:-1], trace[1:]):
        change = (after - before) / abs(before)
        assert change <= 1e-12, (step, change)
        if step == 4:
            assert abs(change) <= 1e-12, change
    assert trace[-1][1] < trace[0][1]


@pytest.mark.parametrize("kind,shape", _longest_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_oracle_orderings_agree(kind, shape):
    """steps 1-3 interleaved per source (as pra writes them) against stage-wise: step 1 of source s reads only P[s] and R[s], and
    P is not refreshed inside an epoch, so the two are the same arithmetic"""
    T, F, M, L = shape
    X = cases.make_x(kind, T, F, M)
    T0, V0 = cases.make_nmf(T, F, M, L)
    a = ilo.ilrma(X, 5, T0[0], V0[0])
    b = ilo.ilrma(X, 5, T0[0], V0[0], interleaved=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("case", cases.ITERATED, ids=cases.case_id)
def test_oracle_is_reproducible_on_the_iterated_cases(case):
    """the condition under which the GPU test compares iterated results: a 1e-13 relative perturbation of X moves the oracle's
    own W by delta with 10 delta <= 1e-8 (measured: delta <= 2.8e-13 on every case)"""
    o = cases.oracle_run(case)
    assert np.all(np.isfinite(o["W"])) and 10 * o["delta"] <= 1e-8 and 10 * o["delta_R"] <= 1e-8, (o["delta"], o["delta_R"])
