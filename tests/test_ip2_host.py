"""overiva_ip2_batch() / overiva_ip2() without a GPU: the schedule, the NumPy restatement the GPU tests compare against
(tests/helpers/ip2_oracle.py) and the properties those tests lean on, every refusal before the library is touched, the names
public, the ABI declared, bound and exported, and every iterated case one where the restatement is itself reproducible."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import ip2_cases as cases  # noqa: E402
import ip2_oracle as ipo  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
IP2_SYMBOLS = ("oiva_batch_ip2_iterate", "oiva_batch_ip2_stage", "oiva_batch_ip2_time_stages")
# (T, F, M, K) of the oracle's own checks: determined and over-determined, odd and even K
ORACLE_SHAPES = [(70, 9, 2, 2), (70, 9, 3, 3), (130, 9, 4, 4), (70, 9, 4, 2), (70, 5, 8, 2), (130, 5, 6, 3), (130, 5, 6, 5), (70, 5, 3, 1)]


@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


# ---------------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("which", ["product", "oracle"])
def test_every_source_is_in_exactly_one_step(which):
    from overiva_amd import ip2

    fn = ip2.schedule if which == "product" else ipo.schedule
    for K in range(1, 9):
        for n in (0, 1, 2, 3):
            steps = fn(K, n)
            assert sorted(s for step in steps for s in step) == list(range(K)), (K, n, steps)
            assert all(len(step) in (1, 2) for step in steps)
            assert all(len(step) == 1 or step[1] == step[0] + 1 for step in steps)
            assert sum(len(step) == 1 for step in steps) <= 2
            assert [tuple(s) for s in steps] == [tuple(s) for s in ipo.schedule(K, n)]


def test_the_schedule_rows_hold_literally():
    from overiva_amd.ip2 import schedule

    assert schedule(1, 0) == schedule(1, 1) == [(0,)]
    assert schedule(2, 0) == schedule(2, 1) == schedule(2, 7) == [(0, 1)]
    assert schedule(3, 0) == [(0, 1), (2,)] and schedule(3, 1) == [(0,), (1, 2)]
    assert schedule(4, 0) == [(0, 1), (2, 3)] and schedule(4, 1) == [(0,), (1, 2), (3,)]
    assert schedule(5, 2) == [(0, 1), (2, 3), (4,)] and schedule(5, 3) == [(0,), (1, 2), (3, 4)]
    assert schedule(8, 0) == [(0, 1), (2, 3), (4, 5), (6, 7)] and schedule(8, 1) == [(0,), (1, 2), (3, 4), (5, 6), (7,)]
    for bad in ((0, 0), (2, -1), (True, 0), (2.0, 0)):
        with pytest.raises(ValueError):
            schedule(*bad)


# ------------------------------------------------------------------------------------------------------------------ oracle
def _start(T, F, M, K, model="laplace", seed=5):
    """a room, its Cx, a W_hat away from the identity and the V of that W_hat"""
    X = cases.make_x("mix", T, F, M, K, seed=seed).astype(np.complex128)
    Cx = ipo.input_covariance(X)
    W_hat = ipo.init_w_hat(Cx, K, cases.random_w0(1, F, M, K, seed=seed, amp=0.3)[0])
    r_inv, scale = ipo.weights(X, W_hat, K, model)
    W_hat[:, :, :K] /= scale
    return X, Cx, W_hat, ipo.weighted_cov(X, r_inv)


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("parity", [0, 1])
def test_oracle_steps_have_their_defining_properties(shape, parity):
    T, F, M, K = shape
    X, Cx, W_hat, V = _start(*shape)
    worst = {"step": 0.0, "j": 0.0}
    before = [ipo.surrogate(W_hat, V, K)]

    def observe(step, phase, W):
        if phase == "step":
            d = (ipo.pair_properties(W, V[:, step[0]], V[:, step[1]], *step) if len(step) == 2 else
                 ipo.single_properties(W, V[:, step[0]], step[0]))
            worst["step"] = max(worst["step"], d)
        else:
            worst["j"] = max(worst["j"], ipo.j_orthogonality(W, Cx, K))
            if K == M:
                now = ipo.surrogate(W, V, K)
                assert np.all(now <= before[-1] + 1e-12 * np.abs(before[-1])), step       # the surrogate never rises
                before.append(now)

    ipo.update(W_hat, V, Cx, K, parity, observe=observe)
    print(f"ip2 oracle {shape} parity {parity}: properties {worst['step']:.2e}, J orthogonality {worst['j']:.2e}")
    assert worst["step"] <= 1e-10 and worst["j"] <= 1e-10


def _near_proportional(F, eps, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((F, 2, 2)) + 1j * rng.standard_normal((F, 2, 2))
    Ub = A @ ipo.herm(A) + 0.1 * np.eye(2)
    E = rng.standard_normal((F, 2, 2)) + 1j * rng.standard_normal((F, 2, 2))
    E = E @ ipo.herm(E)
    return (1.0 + rng.random((F, 1, 1))) * Ub + eps * E, Ub


@pytest.mark.parametrize("eps", [1.0, 1e-3, 1e-6, 1e-9])
def test_the_closed_form_matches_eigh_up_to_a_phase(eps):
    """also where U_a is nearly a multiple of U_b: the eigenvalues, the two normalisations and both cross-orthogonalities; the
    vectors themselves only while the eigenvalue gap keeps them defined"""
    Ua, Ub = _near_proportional(200, eps)
    ha, hb = ipo.rotate(Ua, Ub)
    ga, gb = ipo.rotate_eigh(Ua, Ub)
    q = lambda x, U, y: np.einsum("fi,fij,fj->f", np.conj(x), U, y)      # noqa: E731
    lam_hi, lam_lo = q(ha, Ua, ha).real / q(ha, Ub, ha).real, q(hb, Ua, hb).real / q(hb, Ub, hb).real
    ref_hi, ref_lo = q(ga, Ua, ga).real / q(ga, Ub, ga).real, q(gb, Ua, gb).real / q(gb, Ub, gb).real
    assert np.all(lam_hi >= lam_lo)
    np.testing.assert_allclose(lam_hi, ref_hi, rtol=1e-12)
    np.testing.assert_allclose(lam_lo, ref_lo, rtol=1e-12)
    np.testing.assert_allclose(q(ha, Ua, ha).real, 1.0, rtol=1e-12)
    np.testing.assert_allclose(q(hb, Ub, hb).real, 1.0, rtol=1e-12)
    scale_a, scale_b = np.sqrt(q(hb, Ua, hb).real), np.sqrt(q(ha, Ub, ha).real)
    assert np.max(np.abs(q(hb, Ua, ha)) / scale_a) <= 1e-10 and np.max(np.abs(q(ha, Ub, hb)) / scale_b) <= 1e-10
    if eps >= 1e-3:
        for x, g in ((ha, ga), (hb, gb)):
            ph = np.einsum("fi,fi->f", np.conj(g), x)
            ph /= np.abs(ph)
            assert np.max(np.abs(g * ph[:, None] - x)) <= 1e-9 * np.max(np.abs(x))


@pytest.mark.parametrize("shape", ORACLE_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_the_pair_step_through_eigh_gives_the_same_vectors_up_to_a_phase(shape):
    T, F, M, K = shape
    X, Cx, W_hat, V = _start(*shape)
    W1 = ipo.update(W_hat, V, Cx, K, 0)
    W2 = ipo.update(W_hat, V, Cx, K, 0, rotation=ipo.rotate_eigh)
    ph = np.einsum("fik,fik->fk", np.conj(W2[:, :, :K]), W1[:, :, :K])
    ph /= np.abs(ph)
    assert np.max(np.abs(W2[:, :, :K] * ph[:, None, :] - W1[:, :, :K])) <= 1e-10 * np.max(np.abs(W1))


@pytest.mark.parametrize("shape", [(70, 9, 2, 2), (70, 9, 3, 3), (130, 9, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_a_pair_step_is_no_worse_than_two_ip1_steps(shape):
    """K = M: from the same start and with the same V, the surrogate after the pair (a, b) is no higher than after IP1 on a then b"""
    T, F, M, K = shape
    X, Cx, W_hat, V = _start(*shape)
    for a in range(K - 1):
        pair = np.array(W_hat)
        ipo.pair_step(pair, V[:, a], V[:, a + 1], a, a + 1)
        two = ipo.update_ip1(W_hat, V, Cx, K, sources=(a, a + 1))
        s2, s1 = ipo.surrogate(pair, V, K), ipo.surrogate(two, V, K)
        assert np.all(s2 <= s1 + 1e-12 * np.abs(s1)), (a, np.max(s2 - s1))
        assert np.all(s2 <= ipo.surrogate(W_hat, V, K) + 1e-12)


@pytest.mark.parametrize("shape", [(130, 17, 2, 2), (130, 17, 3, 3), (130, 17, 4, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("model", cases.MODELS)
def test_the_cost_is_monotone_without_the_scale_normalisation(shape, model):
    T, F, M, K = shape
    X = cases.make_x("mix", T, F, M, K, seed=5)
    costs = []
    ipo.iterate(X, K, 10, model, normalise=False, costs=costs)
    steps = np.diff(costs)
    assert np.all(steps <= 1e-12 * np.abs(costs[0])), steps.max()
    assert costs[-1] < costs[0]


def test_chunked_iteration_equals_one_call():
    T, F, M, K = 70, 9, 5, 3
    X = cases.make_x("mix", T, F, M, K, seed=5)
    whole = ipo.iterate(X, K, 5)
    part = ipo.iterate(X, K, 3)
    part = ipo.iterate(X, K, 2, first=3, W_hat=part)
    assert np.array_equal(whole, part)
    wrong = ipo.iterate(X, K, 2, first=0, W_hat=ipo.iterate(X, K, 3))     # (the index matters: odd K alternates its schedule)
    assert not np.array_equal(whole, wrong)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _x(B=2, T=16, F=5, M=3):
    return (np.ones((B, T, F, M)) + 1j).astype(np.complex64)


@pytest.mark.parametrize("bad", [
    dict(X=_x()[0]),                                        # ndim 3
    dict(X=_x().real),                                      # not complex
    dict(X=_x(), n_src=0),
    dict(X=_x(), n_src=4),
    dict(X=_x(), n_src=True),
    dict(X=_x(M=9)),                                        # 9 channels
    dict(X=[_x()[0], _x(M=5)[0]]),                          # mixed channel counts
    dict(X=_x(), model="student"),
    dict(X=_x(), n_iter=-1),
    dict(X=_x(), n_iter=2.5),
    dict(X=_x(), n_src=2, W0=np.ones((5, 3, 3))),           # K columns expected
    dict(X=_x(), W0=np.ones((6, 3, 3))),                    # wrong F
    dict(X=_x(), W0=np.ones((3, 5, 3, 3))),                 # wrong B
    dict(X=[_x()[0], _x(F=6)[0]]),                          # mixed list shapes
    dict(X=[_x()[0], _x()[0].astype(np.complex128)]),       # mixed dtypes
    dict(X=[]),
    dict(X=_x().astype(np.complex128), data="complex128"),  # no complex128 data path
])
def test_ip2_batch_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises((ValueError, TypeError)):
        no_device.overiva_ip2_batch(X, **bad)


def test_the_messages_name_what_is_wrong(no_device):
    with pytest.raises(ValueError, match="n_src must be in 1..3"):
        no_device.overiva_ip2_batch(_x(), n_src=4)
    with pytest.raises(ValueError, match="1..8 channels"):
        no_device.overiva_ip2_batch(_x(M=9))
    with pytest.raises(ValueError, match="model"):
        no_device.overiva_ip2_batch(_x(), model="student")


@pytest.mark.parametrize("bad", [
    dict(X=_x()),                                           # a batch given to the one-room call
    dict(X=_x()[0], n_src=4),
    dict(X=_x()[0], W0=np.ones((1, 5, 3, 3))),              # a batch of starts
])
def test_ip2_validation_before_device(no_device, bad):
    X = bad.pop("X")
    with pytest.raises(ValueError):
        no_device.overiva_ip2(X, **bad)


def test_ip2_batch_refuses_an_active_sharding_group(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: ("group",))
    with pytest.raises(ValueError, match="sharding"):
        no_device.overiva_ip2_batch(_x())
    with pytest.raises(ValueError, match="sharding"):
        no_device.overiva_ip2_batch([_x()[0], _x(T=9)[0]])
    with pytest.raises(ValueError, match="sharding"):
        no_device.separate_batch(np.ones((2, 300, 3), np.float32), frame=8, algorithm="overiva_ip2")


def test_a_complex128_plan_refuses_ip2_before_the_library(no_device):
    plan = object.__new__(no_device.BatchPlan)
    plan.data = "complex128"
    for call in (lambda: plan.ip2_iterate(0, 1), lambda: plan.ip2_stage("update", 0), lambda: plan.ip2_time_stages(1)):
        with pytest.raises(ValueError, match="complex128"):
            call()


@pytest.mark.parametrize("bad", [
    dict(step_size=0.1),                                    # OGIVE's arguments
    dict(tol=1e-3),
    dict(n_src=4),
    dict(n_src=True),
    dict(model="student"),
    dict(n_iter=-1),
])
def test_separate_batch_refuses_before_device(no_device, bad):
    x = np.ones((2, 300, 3), np.float32)
    kw = dict(frame=8, hop=4, algorithm="overiva_ip2")
    kw.update(bad)
    with pytest.raises(ValueError):
        no_device.separate_batch(x, **kw)
    with pytest.raises(ValueError, match="overiva_ip2"):
        no_device.separate_batch(x, frame=8, algorithm="ip2")          # an unknown name; the message lists the known ones
    with pytest.raises(ValueError, match="1..8"):
        no_device.separate_batch(np.ones((1, 300, 9), np.float32), frame=8, algorithm="overiva_ip2")


def test_sweep_entries_are_checked_before_device(no_device):
    from overiva_amd import sweep

    assert "overiva_ip2" in sweep.OVERDET_ALGOS and "auxiva_ip2" not in sweep.OVERDET_ALGOS
    block = {"a": {"algo": "auxiva_ip2", "kwargs": {"n_iter": 30}}, "o": {"algo": "overiva_ip2", "kwargs": {"n_iter": 25, "model": "gauss"}},
             "i": {"algo": "overiva", "kwargs": {"n_iter": 25}}}
    got = {e["name"]: e for e in sweep._check_algorithms(block, 2, [1100, 1100], 3, 64, 32, None, None, sweep.OVERDET_ALGOS)}
    assert got["a"]["n_src"] == 3 and got["a"]["reorder"] and got["o"]["n_src"] == 2 and not got["o"]["reorder"]
    assert got["o"]["model"] == "gauss" and got["a"]["n_iter"] == 30
    assert sweep.checkpoints("overiva_ip2", 25, True) == sweep.checkpoints("overiva", 25, True) == [0, 10, 20, 25]
    assert sweep.checkpoints("auxiva_ip2", 20, True) == sweep.checkpoints("auxiva", 20, True)
    assert sweep.checkpoints("auxiva_ip2", 20) == [0, 20]
    for bad in ({"x": {"algo": "ilrma"}}, {"x": {"algo": "ip2"}}, {"x": {"algo": "overiva_ip2", "kwargs": {"step_size": 0.1}}},
                {"x": {"algo": "auxiva_ip2", "kwargs": {"model": "student"}}}):
        with pytest.raises(ValueError):
            sweep._check_algorithms(bad, 2, [1100, 1100], 3, 64, 32, None, None, sweep.OVERDET_ALGOS)
    with pytest.raises(ValueError):
        sweep._check_algorithms({"x": {"algo": "overiva_ip2"}}, 2, [1100, 1100], 9, 64, 32, None, None, sweep.OVERDET_ALGOS)


# --------------------------------------------------------------------------------------------------------------------- names
def test_ip2_is_public():
    import overiva_amd

    for name in ("overiva_ip2_batch", "overiva_ip2"):
        assert name in overiva_amd.__all__ and callable(getattr(overiva_amd, name))
    for name in ("ip2_iterate", "ip2_stage", "ip2_time_stages"):
        assert callable(getattr(overiva_amd.BatchPlan, name))
        assert getattr(overiva_amd.RaggedBatchPlan, name) is getattr(overiva_amd.BatchPlan, name)       # inherited: a ragged plan runs IP2
    mod = sys.modules["overiva_amd.ip2"]
    assert "DESIGN.md 3.17" in mod.__doc__
    for name in ("schedule", "run_ip2", "overiva_ip2_batch", "overiva_ip2"):
        assert callable(getattr(mod, name))


def test_ip2_symbols_declared_and_bound():
    from overiva_amd import _lib, build

    txt = open(HEADER).read()
    for name in IP2_SYMBOLS:
        assert f" {name}(" in txt, name
        assert name in _lib.SIGNATURES, name
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_batch_ip2_")} == set(IP2_SYMBOLS)
    assert set(re.findall(r"\b(oiva_batch_ip2_\w+)\(", txt)) == set(IP2_SYMBOLS)
    assert "kernels_ip2_batch.hip" in build.SOURCES


def test_ip2_symbols_exported():
    from overiva_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built (build() makes it)")
    import ctypes

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in IP2_SYMBOLS:
        assert hasattr(lib, name), name


def test_stage_names_follow_the_header():
    from overiva_amd import batch

    txt = open(HEADER).read()
    for idx, name in enumerate(batch.IP2_STAGES):
        assert re.search(rf"OIVA_IP2_STAGE_{name.upper()}\s*=\s*{idx}\b", txt), name
    assert len(re.findall(r"OIVA_IP2_STAGE_\w+\s*=", txt)) == len(batch.IP2_STAGES)


# ----------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("case", cases.ITERATED, ids=cases.case_id)
def test_cases_are_reproducible(case):
    """delta: how far a 1e-13 relative perturbation of X moves the restatement's own W.  The GPU file holds the device to
    max(1e-12, 10 delta); a case belongs there only if that bound means something"""
    run = cases.oracle_run(case)
    for n in cases.counts(case):
        print(f"ip2 {cases.case_id(case)} n={n}: delta {run[n]['delta']:.2e}")
        assert np.all(np.isfinite(run[n]["W"]))
        assert 10 * run[n]["delta"] <= 1e-8, (n, run[n]["delta"])


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=cases.update_id)
def test_update_cases_are_well_conditioned(case):
    """the UPDATE stage alone is held to 1e-12 of the largest entry of W.  On every case the GPU file runs, a relative change of
    2e-16 (one rounding) of the V and W_hat the restatement is fed moves its own result by less than a tenth of that"""
    (B, T, F, M, K), model = case
    X, W0 = cases.update_inputs(case)
    worst = 0.0
    for b in range(B):
        rng = np.random.default_rng(b)
        Xb = X[b].astype(np.complex128)
        Cx = ipo.input_covariance(Xb)
        W_hat = ipo.init_w_hat(Cx, K, W0[b])
        r_inv, scale = ipo.weights(Xb, W_hat, K, model)
        W_hat[:, :, :K] /= scale
        V = ipo.weighted_cov(Xb, r_inv)
        V2 = V * (1.0 + 2e-16 * rng.standard_normal(V.shape))
        V2 = 0.5 * (V2 + ipo.herm(V2))
        W2 = W_hat * (1.0 + 2e-16 * rng.standard_normal(W_hat.shape))
        for parity in (0, 1):
            a, c = ipo.update(W_hat, V, Cx, K, parity), ipo.update(W2, V2, Cx, K, parity)
            worst = max(worst, float(np.max(np.abs(c - a)) / np.max(np.abs(a))))
    print(f"ip2 update case {cases.update_id(case)}: the restatement moves {worst:.2e} under one rounding of its inputs")
    assert 10 * worst <= 1e-12
