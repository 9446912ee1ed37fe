"""Single-room plan kernels that a public call with default switches reaches and no test launched (tools/kernel_census.py), at the
smallest shapes at which their launchers can go wrong, each against the float64 reference of the same operation.

* the per-bin update in float32 at 5, 6 and 7 channels (update_bg_kernel<8, float, 5|7, KT>, update_sq_kernel<8, float, MT, KT>, the
  J initialisation among them) and the row layout at 1 and 2 channels (update_kernel<2, float|double, 0, 0>): one update from a given
  W_hat and the device's own V and Cx (tests/helpers/census_update_cases.py).  Bounds: float32 per-bin algebra, the 2e-5 of
  test_ip_update; float64, the rule of test_determined_update_on_ill_conditioned_covariances (4 reference sensitivities + 1e-12);
  the J initialisation, the 1e-5 of test_j_initialisation (all tests/test_gpu_parity.py);
* the vector-ALU power pass at 10..15 channels with up to four sources (power_kernel<10..15, KP, false>): TOL_KERNEL of
  test_demix_power."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import census_update_cases as cu  # noqa: E402
from oracle import overiva_oracle as orc  # noqa: E402
from test_update_forms import reference_sensitivity  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_KERNEL = 3e-6        # tests/test_gpu_parity.py: one float32 pass, no iteration feedback
TOL_UPDATE_F32 = 2e-5    # tests/test_gpu_parity.py::test_ip_update
TOL_J_INIT = 1e-5        # tests/test_gpu_parity.py::test_j_initialisation, up to 8 channels


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    return overiva_amd


@pytest.mark.parametrize("case", cu.DEFAULT_CASES, ids=cu.case_id)
def test_default_update_against_the_oracle(oa, case):
    M, K, mode, T, F, splits, rows = case
    got = cu.run_case(oa, orc, case)
    e_init = orc.rel_err(got["W_init"], orc.init_demixing(got["Cx"], K))
    sens, ref = reference_sensitivity(got["W_in"].astype(np.complex128), got["V"], got["Cx"], K)
    e = orc.rel_err(got["W_out"], ref)
    moved = orc.rel_err(got["W_out"], got["W_in"])
    print(f"\n[census] {cu.case_id(case)}: update {e:.2e} (reference sensitivity {sens:.1e}; moved W_hat by {moved:.1e}), J initialisation {e_init:.2e}")
    assert e_init < TOL_J_INIT
    assert moved > 1e-3                                       # the update ran
    assert e < (TOL_UPDATE_F32 if mode == "fast" else 4 * sens + 1e-12)


# (T, F, M, K): 64 bins per workgroup + 1, frames no multiple of the 4 of a load step; K -> 1, 2 or 4 sources per pass
POWER_SHAPES = [(50, 65, 10, 3), (43, 65, 11, 1), (50, 1, 12, 1), (37, 65, 13, 2), (50, 66, 14, 4), (41, 65, 15, 1)]


@pytest.mark.parametrize("before_covariance", [False, True], ids=["padded-copy", "caller-X"])
@pytest.mark.parametrize("shape", POWER_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_power_pass_at_10_to_15_channels_with_few_sources(oa, shape, before_covariance):
    """overiva.py:140 + :153; odd channel counts on the plan's zero-padded copy of X once the covariance pass has filled it, and on
    the caller's X before"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=30 + M)
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(X)
        if not before_covariance:
            p.covariance()
        p.t_set_what(What)
        pw = p.t_run_power()
    e = orc.rel_err(pw, orc.demix_power(X, What[:, :, :K]))
    print(f"\n[census] power pass {shape}: {e:.2e}")
    assert e < TOL_KERNEL
