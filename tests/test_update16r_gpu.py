"""update_det16r_kernel (csrc/kernels_update16r.hip; reference overiva.py:176-190 for determined AuxIVA at 9..16 channels, float64:
one matrix row per lane, four bins per workgroup, two waves eliminating V_s with recorded multipliers, one running the chain)
against the kernel it replaced (update_det16_kernel, $OIVA_DET16_ROWS=0, itself held against the oracle by tests/test_gpu_parity.py
and tests/test_update_forms.py) and against the oracle directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {repo!r})
import overiva_amd as oa
from oracle import overiva_oracle as orc
out = {{}}
for (T, F, M, splits) in {cases!r}:
    X = orc.synth_mixture(T, F, M, M, seed=T + F + M) if F % 2 else orc.synth_iid(T, F, M, seed=T + F + M)
    with oa.Plan(T, F, M, M, "laplace") as p:
        p.set_precision("mixed")
        p.set_x(X); p.covariance(); p.set_w(None)
        if splits: p.set_cov_splits(splits)
        p.iterate(1)
        out[f"{{T}}_{{F}}_{{M}}_{{splits}}_1"] = p.get_w(np.complex128)
        p.iterate(2)
        out[f"{{T}}_{{F}}_{{M}}_{{splits}}_3"] = p.get_w(np.complex128)
np.savez({path!r}, **out)
"""

CASES = [(256, 6, 16, 0), (256, 7, 13, 0), (300, 9, 12, 0), (1024, 64, 16, 0), (1024, 65, 16, 2), (2048, 33, 15, 4), (2048, 4, 10, 3), (96, 8, 16, 1),
         (640, 130, 9, 0), (512, 12, 11, 0), (512, 5, 14, 2)]


@pytest.fixture(scope="module")
def both_forms(tmp_path_factory):
    """W after three iterations of every case through each kernel (the switch is read once per process: two children)"""
    d = tmp_path_factory.mktemp("det16r")
    res = {}
    for rows in ("0", "1"):
        path = str(d / f"w_rows{rows}.npz")
        env = dict(os.environ, OIVA_DET16_ROWS=rows)
        subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, cases=CASES, path=path)], check=True, env=env, timeout=600)
        res[rows] = dict(np.load(path))
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_rows_kernel_against_the_one_matrix_per_wave_kernel(both_forms, case):
    """the same mathematics in another lane layout (and fused multiply-adds where the old kernel multiplies and adds): the results
    agree to rounding -- ragged bin counts (workgroups of four bins with dead groups), every channel count 9..16 (identity
    padding, odd counts: partial blocks of odd length), 1..4 frame splits"""
    T, F, M, splits = case
    key = f"{T}_{F}_{M}_{splits}"
    e = {}
    for its in (1, 3):
        W0, W1 = both_forms["0"][f"{key}_{its}"], both_forms["1"][f"{key}_{its}"]
        assert np.all(np.isfinite(W1)) and W1.shape == (F, M, M)
        e[its] = orc.rel_err(W1, W0)
    print(f"\n[det16r] {case}: rows vs one-matrix-per-wave after 1 iteration {e[1]:.2e}, after 3 {e[3]:.2e}")
    # one iteration: the two kernels on the same covariances -- rounding of float64 chains of a different association.  Three: the
    # difference has been through the float32 power pass twice, which re-quantises it to float32 rounding noise times the
    # problem's conditioning (measured on the 16 x 16 mixture: 3e-14, 1e-8, 2e-7): far below any parity bound all the same
    assert e[1] < 1e-11 and e[3] < 1e-5


@pytest.mark.parametrize("case", [c for c in CASES if c[1] >= 64], ids=lambda c: "x".join(str(v) for v in c))
def test_rows_kernel_at_64_bins_and_more_against_the_oracle(both_forms, case):
    """the cases with whole 64-bin batches of the power pass (one batch, one + a ragged bin, two + two bins at 9 channels) against
    the oracle itself, not only against the kernel's predecessor: W after three iterations of the row kernel's run within the
    north star's 1e-5 of the oracle's complex128 result on the i.i.d. cases (even bin counts), within max(1e-5, 1.5 floors) on
    the mixture-like one (odd), floor = the reference's own complex64 arithmetic against its complex128 one"""
    T, F, M, splits = case
    mixture = F % 2 == 1
    X = orc.synth_mixture(T, F, M, M, seed=T + F + M) if mixture else orc.synth_iid(T, F, M, seed=T + F + M)      # as the child
    kw = dict(n_src=M, n_iter=3, proj_back=False, model="laplace", return_filters=True)
    _, Wr = orc.overiva_staged(X, **kw)
    bound = 1e-5
    if mixture:
        with np.errstate(all="ignore"):
            floor = orc.rel_err(orc.overiva_faithful(X, **kw)[1], Wr)
        bound = max(bound, 1.5 * floor)
    e = orc.rel_err(both_forms["1"][f"{T}_{F}_{M}_{splits}_3"], Wr)
    print(f"\n[det16r] {case}: rows vs oracle after 3 iterations {e:.2e} (bound {bound:.1e})")
    assert e < bound


@pytest.mark.parametrize("shape", [(200, 10, 16), (160, 7, 12), (320, 5, 9)], ids=lambda s: "x".join(str(v) for v in s))
def test_rows_kernel_against_the_oracle(oa, shape):
    """end to end through overiva() (the default kernel of these shapes) against the oracle's complex128 arithmetic"""
    T, F, M = shape
    X = orc.synth_iid(T, F, M, seed=3)
    Y, W = oa.overiva(X.astype(np.complex128), n_iter=3, proj_back=False, return_filters=True)
    Yr, Wr = orc.overiva_staged(X, n_src=M, n_iter=3, proj_back=False, return_filters=True)
    assert orc.rel_err(W, Wr) < 1e-6 and orc.rel_err(Y, Yr) < 1e-6


def test_rows_kernel_more_than_four_splits_falls_back(oa):
    """few bins and a long frame axis: the covariance pass fills the chip with frame splits -- up to 4 the row kernel adds them (two
    in flight at a time, the rest of its registers are the matrices), beyond that the one-matrix-per-wave kernel serves; same
    results to the rounding of the partials"""
    T, F, M = 4096, 8, 16
    X = orc.synth_iid(T, F, M, seed=9)
    W = {}
    for splits in (4, 8, 32):
        with oa.Plan(T, F, M, M, "laplace") as p:
            p.set_precision("mixed")
            p.set_x(X); p.covariance(); p.set_w(None)
            p.set_cov_splits(splits)
            assert p.cov_splits() == splits
            p.iterate(2)
            W[splits] = p.get_w(np.complex128)
    for splits in (8, 32):
        assert np.all(np.isfinite(W[splits])) and orc.rel_err(W[splits], W[4]) < 1e-5


def test_float32_partial_blocks_opt_in(oa, monkeypatch):
    """$OIVA_HMFMA_PART32=1 (read when a plan chooses its geometry): cov_hmfma_kernel stores its partial blocks as float32 -- each value
    the float64 sum of its chains rounded once -- and both forms of the update add them in float64: W after three iterations within
    1e-6 of the float64-block run on i.i.d. input, with 1, 2 and 4 frame splits and an odd channel count (blocks of odd length)"""
    for (T, F, M, splits) in ((512, 12, 16, 1), (2048, 9, 16, 2), (4096, 5, 16, 4), (1024, 6, 13, 2)):
        X = orc.synth_iid(T, F, M, seed=T + M)
        W = {}
        for part in ("0", "1"):
            monkeypatch.setenv("OIVA_HMFMA_PART32", part)
            with oa.Plan(T, F, M, M, "laplace") as p:
                p.set_precision("mixed")
                p.set_x(X); p.covariance(); p.set_w(None)
                p.set_cov_splits(splits)
                p.iterate(3)
                W[part] = p.get_w(np.complex128)
        e = orc.rel_err(W["1"], W["0"])
        print(f"\n[float32 partial blocks] {T}x{F}x{M}, {splits} splits: W vs float64 blocks {e:.1e}")
        assert np.all(np.isfinite(W["1"])) and 0 < e < 1e-6
