"""The partial powers of the power pass, part by part and from every position of a batch in the launch.

reference overiva.py:140 + :152-155: the per-frame power of the demixed signal is summed over bins; it leaves the device as one
float32 PART per 64-bin batch (csrc/kernels_misc.hip adds the parts in canonical blocks).  The bin-sharded path rests on one
promise: a plan that holds whole batches of the bins -- ``Plan(..., F_total=)`` -- produces the same parts, bit
for bit, as the plan that holds all bins, wherever its first batch lies in the whole.  Checked here for every power kernel
(PowKind Lane with 1, 2 and 4 sources per pass, Mfma, Lds, Wide):

* every shard's parts are ``array_equal`` to the single plan's parts of the same batches -- shards whose first batch is batch
  0, 1, 2, 3 and 5 of the whole, two of them with the ragged last batch (17 bins: two 16-bin sub-batches in power_lds_kernel);
* every part of the single plan alone is within the single-kernel bound of the oracle's power over that batch's bins (the sum
  over parts, which the other tests compare, would not notice a bin booked to the neighbouring part);
* ``kernel_choice`` reports the kind the case is named for, for the whole and for every shard.

70 frames: two 64-frame workgroup rows of power_lds_kernel, a cut 16-frame tile, no multiple of 4.  Needs an MI355X: run with ``-m gpu``.
"""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL_KERNEL = 3e-6   # single-kernel bound (one fp32 pass, no iteration feedback), as tests/test_gpu_parity.py
T, F_TOTAL = 70, 401                 # six whole batches of 64 bins + a ragged one of 17
SHARDS = [(0, 256), (64, 192), (128, 256), (192, 401), (320, 401)]      # first batches 0, 1, 2, 3, 5
BATCH = 64

CASES = [("Lane", 4, 1), ("Lane", 8, 2), ("Lane", 6, 3), ("Lane", 8, 8), ("Lane", 12, 3), ("Lane", 16, 2),
         ("Mfma", 10, 6), ("Mfma", 13, 7), ("Mfma", 12, 12), ("Mfma", 15, 15),
         ("Lds", 16, 5), ("Lds", 16, 9), ("Lds", 16, 16),
         ("Wide", 20, 3), ("Wide", 24, 5)]


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


def _parts(oa, X, What, K, F_total):
    T_, F, M = X.shape
    with oa.Plan(T_, F, M, K, "laplace", F_total=F_total) as p:
        p.set_x(np.ascontiguousarray(X))
        p.covariance()
        p.t_set_what(np.ascontiguousarray(What))
        total = p.t_run_power()
        parts = p.t_get_ppart()
    return parts, total


@pytest.mark.parametrize("kind,M,K", CASES, ids=[f"{k}-{m}x{s}" for k, m, s in CASES])
def test_parts_are_the_same_bits_from_every_position_and_each_is_its_own_bins(oa, kind, M, K):
    from overiva_amd import plan

    X = orc.synth_iid(T, F_TOTAL, M, seed=100 * M + K)
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F_TOTAL, M, M)) + 1j * rng.standard_normal((F_TOTAL, M, M))).astype(np.complex64)

    choice = plan.kernel_choice(T, F_TOTAL, M, K, F_total=F_TOTAL)
    assert choice["pow_kind"] == kind
    if kind == "Lane":
        assert choice["kp"] == (4 if K >= 3 else K)      # sources per pass: 1, 2 and 4 all appear among the cases
    single, total = _parts(oa, X, What, K, F_TOTAL)
    nparts = -(-F_TOTAL // BATCH)
    assert single.shape == (nparts, T, K)

    # each part against the oracle on that batch's bins alone
    worst = 0.0
    for b in range(nparts):
        lo, hi = b * BATCH, min((b + 1) * BATCH, F_TOTAL)
        e = orc.rel_err(single[b], orc.demix_power(X[:, lo:hi], What[lo:hi, :, :K]))
        worst = max(worst, e)
        assert e < TOL_KERNEL, (b, e)
    assert orc.rel_err(total, orc.demix_power(X, What[:, :, :K])) < TOL_KERNEL
    print(f"\n[parts] {kind} {M}x{K}: worst part vs oracle {worst:.2e}")

    # every shard: the bits of the single plan's parts of the same batches
    differ = []
    for lo, hi in SHARDS:
        assert plan.kernel_choice(T, hi - lo, M, K, F_total=F_TOTAL)["pow_kind"] == kind, (lo, hi)
        shard, _ = _parts(oa, X[:, lo:hi], What[lo:hi], K, F_TOTAL)
        want = single[lo // BATCH:-(-hi // BATCH)]
        assert shard.shape == want.shape, (lo, hi)
        if not np.array_equal(shard, want):
            differ.append((lo, hi, [int(b) for b in np.flatnonzero(np.any(shard != want, axis=(1, 2)))], orc.rel_err(shard, want)))
    assert not differ, f"shards (lo, hi, parts that differ, distance): {differ}"
