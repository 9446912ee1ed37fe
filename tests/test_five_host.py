"""five_batch() / five() without a GPU: every refusal comes before the library is touched, the names are public, the ABI is
declared, bound and exported, the new kernels use no scratch memory, and the NumPy restatement the GPU tests compare against
(tests/helpers/five_oracle.py) has the properties those tests lean on: its two formulations agree, its w satisfies w^H V w = 1
and V w = lambda Cx w, and every compared iterate of every case has a relative eigen-gap of at least 0.005."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import five_oracle as fo  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
FIVE_SYMBOLS = ("oiva_batch_five_begin", "oiva_batch_five_stage", "oiva_batch_five_iterate", "oiva_batch_five_time_stages",
                "oiva_batch_five_get_reduction")


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


@pytest.mark.parametrize("bad", [
    dict(X=_x(), n_src=2),                                  # one source only
    dict(X=_x(), n_src=True),
    dict(X=_x(M=9)),                                        # 9 channels
    dict(X=_x(), W0=np.ones((5, 3, 3))),                    # a start of three columns
    dict(X=_x(), W0=np.ones((6, 3, 1))),                    # wrong F
    dict(X=_x(), W0=np.ones((3, 5, 3, 1))),                 # wrong B
    dict(X=[_x()[0], _x(F=6)[0]]),                          # rooms whose F differ
    dict(X=[_x()[0], _x(M=4)[0]]),                          # rooms whose M differ
    dict(X=[_x()[0], _x()[0].astype(np.complex128)]),       # mixed dtypes
    dict(X=[]),
    dict(X=_x()[0]),                                        # ndim 3
    dict(X=_x().real),                                      # not complex
    dict(X=_x(), model="student"),
    dict(X=_x(), n_iter=-1),
    dict(X=_x(), n_iter=2.5),
])
def test_five_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises((ValueError, TypeError)):
        no_device.five_batch(X, **bad)


def test_the_messages_name_what_is_wrong(no_device):
    with pytest.raises(ValueError, match="one source"):
        no_device.five_batch(_x(), n_src=2)
    with pytest.raises(ValueError, match="1..8 channels"):
        no_device.five_batch(_x(M=9))
    with pytest.raises(ValueError, match="W0 has shape"):
        no_device.five_batch(_x(), W0=np.ones((5, 3, 3)))
    with pytest.raises(ValueError, match="F and M must agree"):
        no_device.five_batch([_x()[0], _x(F=6)[0]])


@pytest.mark.parametrize("method,args", [("five_begin", ()), ("five_iterate", (1,)), ("five_stage", ("update",)),
                                         ("get_five_reduction", ()), ("five_time_stages", (1,))])
def test_a_complex128_plan_is_refused_before_device(no_device, method, args):
    """the refusal names "complex128" and is raised before the handle is used (this plan has none)"""
    plan = object.__new__(no_device.BatchPlan)
    plan.data = "complex128"
    with pytest.raises(ValueError, match="complex128"):
        getattr(plan, method)(*args)


@pytest.mark.parametrize("bad", [
    dict(X=_x()),                                           # a batch given to the one-room call
    dict(X=_x()[0], n_src=2),
    dict(X=_x()[0], W0=np.ones((1, 5, 3, 1))),              # a batch of starts
])
def test_five_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.five(X, **bad)


def test_five_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.five_batch(_x())


def test_separate_batch_refuses_before_device(no_device):
    x = np.ones((2, 300, 3), np.float32)
    with pytest.raises(ValueError, match="one source"):
        no_device.separate_batch(x, frame=8, hop=4, algorithm="five", n_src=2)
    with pytest.raises(ValueError, match="unknown arguments"):
        no_device.separate_batch(x, frame=8, hop=4, algorithm="five", step_size=0.1)
    with pytest.raises(ValueError, match="'five'"):
        no_device.separate_batch(x, frame=8, hop=4, algorithm="six")


def test_five_is_public():
    import overiva_amd

    for name in ("five_batch", "five"):
        assert name in overiva_amd.__all__ and callable(getattr(overiva_amd, name))
    for name in ("five_begin", "five_iterate", "five_stage", "get_five_reduction", "five_time_stages"):
        assert callable(getattr(overiva_amd.BatchPlan, name))
        assert getattr(overiva_amd.RaggedBatchPlan, name) is getattr(overiva_amd.BatchPlan, name)     # inherited: a ragged plan runs FIVE
    assert "DESIGN.md 3.16" in sys.modules["overiva_amd.five"].__doc__


def test_five_symbols_declared_and_bound():
    from overiva_amd import _lib, build

    txt = open(HEADER).read()
    for name in FIVE_SYMBOLS:
        assert f" {name}(" in txt, name
        assert name in _lib.SIGNATURES, name
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_batch_five_")} == set(FIVE_SYMBOLS)
    assert "kernels_five_batch.hip" in build.SOURCES


def test_five_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in FIVE_SYMBOLS:
        assert hasattr(lib, name), name


def test_stage_names_follow_the_header():
    import re

    from overiva_amd import batch

    txt = open(HEADER).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"OIVA_FIVE_STAGE_([A-Z]+) = (\d+)", txt)}
    assert values == {"POWER": 0, "ACTIVATION": 1, "COV": 2, "UPDATE": 3}
    assert batch.FIVE_STAGES == tuple(name.lower() for name, _ in sorted(values.items(), key=lambda kv: kv[1]))


def test_five_kernels_use_no_scratch_memory():
    """a bin's matrices live in LDS tiles and a lane holds a handful of entries: neither kernel may spill"""
    from overiva_amd import build

    if not os.path.exists(os.path.join(build.OBJ, "kernels_five_batch.usage.txt")):
        pytest.fail("no resource remarks of kernels_five_batch.hip (build() writes them)")
    usage = build.kernel_usage(("kernels_five_batch",))
    for kernel in ("five_begin_kernel", "five_update_kernel"):
        assert len([1 for name in usage if kernel in name]) == 4, (kernel, sorted(usage))     # 2, 4, 6 and 8 padded channels
    assert len(usage) == 8 and all(u["scratch"] == 0 for u in usage.values()), usage


# ---- the restatement's invariants: they fix the cases before any GPU is involved --------------------------------------------------
@pytest.mark.parametrize("case", fo.CASES, ids=fo.case_id)
def test_the_two_formulations_agree_and_w_solves_the_pencil(case):
    """one iteration from the eigenvector start, every room: the two formulations within 1e-10 (phase-free), and for both
    |w^H V w - 1| <= 1e-12, ||V w - lambda_1 Cx w|| / ||V w|| <= 1e-10, lambda_1 the smallest of scipy's generalized eigenvalues"""
    shape, model = case
    for X in fo.rooms(shape):
        Cx = fo.covariance(X)
        V = fo.weighted_cov(X, fo.weights(X, fo.start(Cx), model))
        wa, la = fo.step_whitened(V, Cx)
        wb, lb = fo.step_pencil(V, Cx)
        assert fo.wdist(wa, wb) <= 1e-10
        assert np.max(np.abs(la - lb) / lb) <= 1e-10
        for w in (wa, wb):
            Vw = np.einsum("fmn,fn->fm", V, w)
            Cw = np.einsum("fmn,fn->fm", Cx, w)
            assert np.max(np.abs(np.sum(np.conj(w) * Vw, axis=1) - 1.0)) <= 1e-12
            res = np.linalg.norm(Vw - lb[:, :1] * Cw, axis=1) / np.linalg.norm(Vw, axis=1)
            assert res.max() <= 1e-10, res.max()


@pytest.mark.parametrize("case", fo.CASES, ids=fo.case_id)
def test_every_compared_iterate_has_a_gap(case):
    """the condition under which the GPU tests compare: (lambda_2 - lambda_1) / lambda_2 >= 0.005 on every bin of each of the
    ten iterations, both formulations and the perturbed input; and the yardsticks that follow are of the order 1e-11"""
    shape, model = case
    for X in fo.rooms(shape):
        y = fo.yardstick(X, None, model)
        assert y["min_gap"] >= fo.MIN_GAP, y["min_gap"]
        for n in fo.ITER_COUNTS:
            assert y[n]["tol_w"] <= 1e-9 and y[n]["tol_y"] <= 1e-9, (n, y[n]["tol_w"], y[n]["tol_y"])


def test_the_ragged_rooms_have_a_gap():
    for X in fo.ragged_rooms():
        assert fo.five(X, 10, "laplace")["min_gap"] >= fo.MIN_GAP


def test_the_phase_free_distance_ignores_a_phase_per_bin():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((7, 4)) + 1j * rng.standard_normal((7, 4))
    ph = np.exp(2j * np.pi * rng.random((7, 1)))
    assert fo.wdist(w * ph, w) <= 1e-15
    assert fo.wdist(w * ph * (1 + 1e-6), w) > 1e-7
