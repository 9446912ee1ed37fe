"""auxiva_iss_batch() / auxiva_iss() without a GPU: every refusal comes before the library is touched, the names are public, the
ABI is declared, bound and exported, and the NumPy restatement the GPU tests compare against (tests/helpers/iss_oracle.py) has
the properties those tests lean on: after every rank-1 step the steered channels are orthogonal to the old y_k under their
weights and y_k has unit weighted power, the signals kept by rank-1 updates are X conj(W), the cost never rises across a sweep on
the cost cases, and every iterated case is one where the restatement is itself reproducible."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import iss_oracle as iso  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
ISS_SYMBOLS = ("oiva_batch_iss_begin", "oiva_batch_iss_iterate", "oiva_batch_iss_stage", "oiva_batch_iss_time_stages",
               "oiva_batch_iss_sweep_steps", "oiva_batch_iss_get_weights", "oiva_batch_iss_get_powers")


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
    dict(X=_x()[0]),                                        # ndim 3
    dict(X=_x().real),                                      # not complex
    dict(X=_x(), n_src=2),                                  # overdetermined
    dict(X=_x(), n_src=4),
    dict(X=_x(), n_src=True),
    dict(X=_x(M=9)),                                        # 9 channels
    dict(X=_x(B=1, T=1025, F=2, M=8)),                      # T M = 8200
    dict(X=_x(B=1, T=8200, F=2, M=1)),
    dict(X=[_x()[0], _x(T=1640, M=5)[0]]),                  # mixed channel counts
    dict(X=[_x(T=20)[0], _x(T=2734)[0]]),                   # a list whose second room has T M = 8202
    dict(X=_x(), model="student"),
    dict(X=_x(), n_iter=-1),
    dict(X=_x(), W0=np.ones((5, 3, 2))),                    # K != M
    dict(X=_x(), W0=np.ones((6, 3, 3))),                    # wrong F
    dict(X=_x(), W0=np.ones((3, 5, 3, 3))),                 # wrong B
    dict(X=[_x()[0], _x(F=6)[0]]),                          # mixed list shapes
    dict(X=[_x()[0], _x()[0].astype(np.complex128)]),       # mixed dtypes
    dict(X=[]),
])
def test_iss_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises((ValueError, TypeError)):
        no_device.auxiva_iss_batch(X, **bad)


def test_the_messages_name_what_is_wrong(no_device):
    with pytest.raises(ValueError, match="determined"):
        no_device.auxiva_iss_batch(_x(), n_src=2)
    with pytest.raises(ValueError, match="8192"):
        no_device.auxiva_iss_batch(_x(B=1, T=1025, F=2, M=8))
    with pytest.raises(ValueError, match="1..8 channels"):
        no_device.auxiva_iss_batch(_x(M=9))


@pytest.mark.parametrize("bad", [
    dict(X=_x()),                                           # a batch given to the one-room call
    dict(X=_x()[0], n_src=2),
    dict(X=_x()[0], W0=np.ones((1, 5, 3, 3))),              # a batch of starts
])
def test_iss_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.auxiva_iss(X, **bad)


def test_iss_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.auxiva_iss_batch(_x())
    with pytest.raises(ValueError, match="sharding"):
        no_device.auxiva_iss_batch([_x()[0], _x(T=9)[0]])


@pytest.mark.parametrize("bad", [
    dict(n_src=2),                                          # ISS is determined
    dict(n_src=True),
    dict(frame=8, hop=1),                                   # 3000 frames x 3 channels = 9000
])
def test_separate_batch_refuses_before_device(no_device, bad):
    x = np.ones((2, 3000, 3), np.float32)
    kw = dict(frame=8, hop=4, algorithm="auxiva_iss")
    kw.update(bad)
    with pytest.raises(ValueError, match="determined|8192"):
        no_device.separate_batch(x, **kw)


def test_iss_is_public():
    import overiva_amd

    for name in ("auxiva_iss_batch", "auxiva_iss"):
        assert name in overiva_amd.__all__ and callable(getattr(overiva_amd, name))
    for name in ("iss_begin", "iss_iterate", "iss_stage", "iss_sweep_steps", "get_iss_weights", "get_iss_powers", "iss_time_stages"):
        assert callable(getattr(overiva_amd.BatchPlan, name))
        assert getattr(overiva_amd.RaggedBatchPlan, name) is getattr(overiva_amd.BatchPlan, name)       # inherited: a ragged plan runs ISS
    assert "DESIGN.md 3.15" in sys.modules["overiva_amd.iss"].__doc__


def test_iss_symbols_declared_and_bound():
    from overiva_amd import _lib, build

    txt = open(HEADER).read()
    for name in ISS_SYMBOLS:
        assert f" {name}(" in txt, name
        assert name in _lib.SIGNATURES, name
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_batch_iss_")} == set(ISS_SYMBOLS)
    assert "kernels_iss_batch.hip" in build.SOURCES


def test_iss_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ISS_SYMBOLS:
        assert hasattr(lib, name), name


def test_stage_names_follow_the_header():
    import re

    from overiva_amd import batch

    txt = open(HEADER).read()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"OIVA_ISS_STAGE_([A-Z]+) = (\d+)", txt)}
    assert values == {"ACTIVATION": 0, "SWEEP": 1}
    assert batch.ISS_STAGES == ("activation", "sweep")


def test_iss_kernels_use_no_scratch_memory():
    """the sweep keeps 3 M sums and a column of W in registers through M unrolled steps: none of it may end in scratch memory"""
    from overiva_amd import build

    if not os.path.exists(os.path.join(build.OBJ, "kernels_iss_batch.usage.txt")):
        pytest.fail("no resource remarks of kernels_iss_batch.hip (build() writes them)")
    usage = build.kernel_usage(("kernels_iss_batch",))
    sweeps = [u for name, u in usage.items() if "iss_sweep_kernel" in name]
    assert len(sweeps) == 8, sorted(usage)
    for kernel in ("iss_activation_kernel", "iss_finalize_kernel"):
        assert len([1 for name in usage if kernel in name]) == 1, (kernel, sorted(usage))
    assert len(usage) == 10 and all(u["scratch"] == 0 for u in usage.values()), usage


# ---- the oracle's invariants: they fix the cases before any GPU is involved -------------------------------------------------------
def _watch(X, model, n_iter, seen):
    """runs the oracle and records the worst of the three per-step figures into ``seen``"""
    X128 = X.astype(np.complex128)
    T = X.shape[0]

    def observe(it, k, Y, W, phi, yk):
        if k < 0:
            return
        d = np.einsum("tm,tf->fm", phi, yk.real ** 2 + yk.imag ** 2)
        c = np.abs(np.einsum("tm,tfm,tf->fm", phi, Y, np.conj(yk)))
        n = np.einsum("tm,tfm->fm", phi, Y.real ** 2 + Y.imag ** 2)
        orth = np.delete(c / np.sqrt(n * d), k, axis=1)
        seen["orth"] = max(seen.get("orth", 0.0), float(orth.max()) if orth.size else 0.0)
        seen["norm"] = max(seen.get("norm", 0.0), float(np.max(np.abs(n[:, k] / T - 1.0))))
        ref = iso.demix(X128, W)
        seen["kept"] = max(seen.get("kept", 0.0), float(np.max(np.abs(Y - ref)) / np.max(np.abs(ref))))

    return iso.iss(X, n_iter, model, observe=observe)


@pytest.mark.parametrize("case", iso.ITERATED, ids=iso.case_id)
def test_oracle_steps_have_their_properties(case):
    """over 20 iterations: |sum_t phi_m y_m' conj(y_k)| / sqrt(sum_t phi_m |y_m'|^2 d_m) <= 1e-13 for m != k (y_k the old one),
    |sum_t phi_k |y_k'|^2 / T - 1| <= 1e-13, and the Y kept by rank-1 updates equals X conj(W) to 1e-12"""
    kind, (T, F, M), model = case
    seen = {}
    out = _watch(iso.make_x(kind, T, F, M), model, 20, seen)
    assert np.all(np.isfinite(out["W"]))
    assert seen["orth"] <= 1e-13 and seen["norm"] <= 1e-13 and seen["kept"] <= 1e-12, seen


@pytest.mark.parametrize("case", iso.ITERATED, ids=iso.case_id)
def test_oracle_is_reproducible_on_the_iterated_cases(case):
    """the condition under which the GPU test compares iterated results: a 1e-13 relative perturbation of X moves the oracle's own
    W by delta with 10 delta <= 1e-8, after 1, 5 and 20 iterations.  No case is skipped by it on the GPU: one that fails here is
    replaced."""
    o = iso.oracle_run(case)
    for n in iso.ITER_COUNTS:
        assert np.all(np.isfinite(o[n]["W"])) and 10 * o[n]["delta"] <= 1e-8, (n, o[n]["delta"])


@pytest.mark.parametrize("case", iso.COST_CASES, ids=iso.case_id)
def test_oracle_cost_never_rises_across_a_sweep(case):
    """J after the M steps against J after the activation, 20 iterations, every room of the case: no sweep raises it by more than
    1e-12 of |J|.  (The gauss case is kept because this holds on it: the eps floor of the weights stays inactive there.)"""
    kind, (B, T, F, M), model = case
    for b in range(B):
        X = iso.make_x(kind, T, F, M, seed=iso.SEED + b)
        trace = []

        def observe(it, k, Y, W, phi, yk):
            if k in (-1, M - 1):
                trace.append((k, iso.cost(X, W, model), float(phi.max())))

        iso.iss(X, 20, model, observe=observe)
        assert len(trace) == 40
        for (k0, before, top), (k1, after, _) in zip(trace[0::2], trace[1::2]):
            assert (k0, k1) == (-1, M - 1) and np.isfinite(after)
            assert (after - before) / abs(before) <= 1e-12, (before, after)
            assert top < 1.0 / iso.EPS                    # the floor is inactive
        assert trace[-1][1] < trace[0][1]
