"""The per-bin update kernels that only a switch of the process selects, against the oracle's chain.

tools/kernel_census.py found them launched by no test: tests/test_update_choice_gpu.py holds their rows of the choice table by
CAPTURING the launch (nothing executes), and the plans that run compare default switches only.  $OIVA_UPDATE_GRAM, $OIVA_UPDATE_DET
and $OIVA_DET16_INVERSE are documented (INTEGRATION.md "switches"), so a user can run this arithmetic.

The library reads its switches once per process: every set of tests/helpers/census_update_cases.py runs in one fresh child process,
all four side by side, started once per module.  A child runs one update per case from a given W_hat and hands back W_hat before and
after and the device's own V and Cx in complex128; the comparison is made here, against ``orc.ip_update_bin`` on those V and Cx.

Bound: the rule of test_determined_update_on_ill_conditioned_covariances (tests/test_gpu_parity.py), float64 per-bin algebra from
the device's own V: 4 of the reference's own moves under a last-bit change of V, + 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import census_update_cases as cu  # noqa: E402
from oracle import overiva_oracle as orc  # noqa: E402
from test_update_forms import reference_sensitivity  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(n, c) for n, s in enumerate(cu.SETS) for c in s[2]]


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{set: what its child saved}; the four children run side by side (at most 6 at a time is the rule)"""
    assert len(cu.SETS) <= 6
    d = tmp_path_factory.mktemp("census_update")
    script = os.path.join(HERE, "helpers", "census_update_cases.py")
    procs = [subprocess.Popen([sys.executable, script, str(n), str(d / f"{n}.npz")], env=cu.set_env(n), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for n in range(len(cu.SETS))]
    out = {}
    for n, p in enumerate(procs):
        text, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (cu.SETS[n][0], p.returncode, text[-3000:])
        with np.load(d / f"{n}.npz") as z:
            out[n] = {k: z[k] for k in z.files}
    return out


@pytest.mark.parametrize("n,case", CASES, ids=[f"{cu.SETS[n][0]}-{cu.case_id(c)}" for n, c in CASES])
def test_switched_update_against_the_oracle(children, n, case):
    M, K, mode, T, F, splits, rows = case
    got = {k: children[n][f"{cu.case_id(case)}/{k}"] for k in ("W_in", "V", "Cx", "W_out", "splits")}
    assert not splits or int(got["splits"]) == splits        # (9..16 channels: the one-matrix-per-wave kernels need five)
    assert got["V"].shape == (K, F, M, M) and got["W_out"].shape == (F, M, M)
    sens, ref = reference_sensitivity(got["W_in"], got["V"], got["Cx"], K)
    e = orc.rel_err(got["W_out"], ref)
    moved = orc.rel_err(got["W_out"], got["W_in"])
    print(f"\n[census] {cu.SETS[n][0]} {cu.case_id(case)}: {e:.2e} (reference sensitivity {sens:.1e}; the update moved W_hat by {moved:.1e})")
    assert moved > 1e-3                                       # the update ran
    assert e < 4 * sens + 1e-12
