"""The kernel choice (csrc/kernel_choice.h) on the device.  The library's choice on every row of the recorded table
(tests/golden/kernel_choice_256cu.json: the choices of the commit before the table existed, tools/kernel_choice_table.py), and
small plans of every covariance and power kernel kind (tests/helpers/kernel_choice_cases.py) that really run what the choice says:
their splits and the quad switch's answer are the choice's, and the weighted covariance, the input covariance, two iterations
and the demixed output pass the comparisons of the parity tests at these shapes (their helpers and tolerances)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from oracle import overiva_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
from kernel_choice_cases import PLAN_CASES, QUAD_GOVERNED, case_id  # noqa: E402
from test_gpu_parity import FAST_FLOORS, TOL, _c64_floor  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = os.path.join(GOLDEN_DIR, "kernel_choice_256cu.json")


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


@pytest.fixture
def part32_env():
    saved = os.environ.get("OIVA_HMFMA_PART32")
    yield
    if saved is None:
        os.environ.pop("OIVA_HMFMA_PART32", None)
    else:
        os.environ["OIVA_HMFMA_PART32"] = saved


def test_every_recorded_row(oa, part32_env):
    import kernel_choice_table as kct
    from overiva_amd import _lib
    from overiva_amd.plan import kernel_choice

    table = json.load(open(TABLE))
    n_in = len(kct.INPUTS)
    assert table["columns"] == kct.INPUTS + kct.OUTPUTS and [tuple(r[:n_in]) for r in table["rows"]] == kct.sweep()
    n_cu = kernel_choice(70, 5, 3, 2)["n_cu"]
    if n_cu != table["n_cu"]:
        pytest.skip(f"the table was recorded on {table['n_cu']} CUs, this device has {n_cu}")
    lib = _lib.load()
    bad = [(r[:n_in], r[n_in:], got) for r in table["rows"] for got in [kct.choose(lib, r[:n_in])] if got != r[n_in:]]
    assert not bad, (len(bad), bad[:5])


def _check_against_oracle(oa, X, K, mode, p):
    """two iterations from the identity and the demixed output against the complex128 oracle, as
    test_gpu_parity.test_odd_shapes_against_oracle and test_fast_mode_accuracy bound them"""
    p.set_w()
    p.iterate(2)
    W, Y = p.get_w(np.complex128), p.demix(proj_back=True)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(Y))
    Yr, Wr = orc.overiva_staged(X, n_src=K, n_iter=2, proj_back=True, model="laplace", return_filters=True)
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    bound = TOL
    if mode != "precise" and max(eW, eY / 2) >= TOL:
        floor = _c64_floor(lambda: orc.overiva_faithful(X, n_src=K, n_iter=2, proj_back=True, model="laplace", return_filters=True)[1], Wr)
        if not floor < 1e-2:
            return          # the reference's own complex64 arithmetic is chaotic here: nothing to pin (finite, above)
        bound = max(TOL, (1.5 if mode == "mixed" else FAST_FLOORS) * floor)
    print(f"\n[kernel choice] 2 its ({mode}): W err {eW:.2e} Y err {eY:.2e} (bound {bound:.1e})")
    assert eW < bound and eY < 2 * bound


@pytest.mark.parametrize("case", PLAN_CASES, ids=case_id)
def test_plan_runs_the_chosen_kernels(oa, case, part32_env):
    from overiva_amd.plan import kernel_choice

    T, F, M, K, mode, quad, hm, p32, cov_kind, pow_kind = case
    os.environ["OIVA_HMFMA_PART32"] = "1" if p32 else "0"
    choice = kernel_choice(T, F, M, K, mode, cov_quad=quad, cov_hmfma=hm)
    assert (choice["cov_kind"], choice["pow_kind"], choice["part32"]) == (cov_kind, pow_kind, int(p32))
    X = orc.synth_iid(T, F, M, seed=T + F + 10 * M + K)
    rinv = np.random.default_rng(M + 17 * K).gamma(2.0, 1.0, (T, K)).astype(np.float32)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_cov_hmfma(hm)
        assert p.set_cov_quad(quad) == (choice["cov_kind"] in QUAD_GOVERNED)
        assert p.cov_splits() == choice["nsplit"]
        p.set_x(X)
        p.covariance()
        Cx = p.get_cx()
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
        # the comparisons of test_cov_dispatch_gpu (1..16 channels) and test_wide_gpu.test_wide_covariance (17..32)
        w = 1.0 / (np.float32(1) / rinv).astype(np.float64) if mode == "precise" else rinv.astype(np.float64)
        eV = orc.rel_err(V, orc.weighted_cov_all(X, w))
        eC = orc.rel_err(Cx, orc.input_covariance(X.astype(np.complex128)))
        if M > 16:
            tol = 1e-10 if mode == "precise" else 3e-7
            assert eV < tol and eC < max(tol, 1e-7), (eV, eC)
        else:
            tol = (1e-12 if M <= 8 else 2e-7) if mode == "precise" else 3e-7
            assert eV < tol and eC < tol, (eV, eC)
        assert np.array_equal(V, np.conj(np.swapaxes(V, -1, -2)))
        _check_against_oracle(oa, X, K, mode, p)
