"""The bin-sharded product path on ONE MI355X: several plans with F_total > F on the same device, their partial
power buffers concatenated by a device copy (what the RCCL all-gather of overiva_amd/sharded.py delivers), against
the single-plan run.  Reference coupling: overiva.py:152-155 (r needs all bins) is the only exchange.

Checked: oiva_plan_power / oiva_plan_power_buffer / oiva_plan_update, the parts-per-rank layout with zero-padded
parts, the fixed part order of the sum, F_total in the gauss model's 1/F, plans running on a caller-provided
stream.  EQUAL shards on 64-bin batches must give the SAME BITS as the single plan (the sum over the parts is associated
in the same canonical blocks, csrc/kernels_misc.hip); other boundaries the same result to rounding (the zero parts that pad
unequal shards to one message size shift the blocks).  Needs an MI355X: run with ``-m gpu``.
"""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

T, F, M, K = 300, 448, 8, 2          # 7 batches of 64 bins


def _run_single(oa, X, model, mode, n_iter, MK=(M, K), splits=0):
    """-> W, Y, r_inv after the last iteration, the plan's covariance frame splits (``splits``: asked for; 0: the plan's own choice)"""
    F = X.shape[1]
    with oa.Plan(T, F, MK[0], MK[1], model) as p:
        p.set_precision(mode)
        if splits:
            p.set_cov_splits(splits)
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.iterate(n_iter)
        return p.get_w(np.complex128), p.demix(True), p.t_get_rinv()[0], p.cov_splits()


def _run_sharded(oa, X, model, mode, n_iter, bounds, MK=(M, K), splits=0):
    """-> concatenated W and Y, every plan's r_inv after the last iteration, every plan's covariance frame splits"""
    import torch

    from overiva_amd.sharded import HipEngine

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    world = len(bounds) - 1
    F = X.shape[1]
    with torch.cuda.stream(stream):
        engines = [HipEngine(T, bounds[r + 1] - bounds[r], MK[0], MK[1], model, F, 0, precision=mode) for r in range(world)]
        assert all(e.stream.cuda_stream == stream.cuda_stream for e in engines)       # one stream orders everything
        if splits:
            for e in engines:
                e.plan.set_cov_splits(splits)
        ppr = max(e.power_parts(bounds[r + 1] - bounds[r]) for r, e in enumerate(engines))
        local = [e.exchange_buffer(ppr) for e in engines]
        gathered = engines[0].new_gather_buffer(world)
        for r, e in enumerate(engines):
            e.set_x(X, bounds[r])
            e.covariance()
            e.set_w(None)
        rows = ppr * T
        for _ in range(n_iter):
            for e in engines:
                e.power()
            for r in range(world):                       # the all-gather: rank-major concatenation
                gathered[r * rows:(r + 1) * rows].copy_(local[r], non_blocking=True)
            for e in engines:
                e.update(gathered)
        W = np.concatenate([e.plan.get_w(np.complex128) for e in engines], axis=0)
        Y = np.concatenate([e.demix(True) for e in engines], axis=1)
        rinv = [e.plan.t_get_rinv()[0] for e in engines]
        got = [e.plan.cov_splits() for e in engines]
        for e in engines:
            e.close()
    return W, Y, rinv, got


@pytest.mark.parametrize("mode", ["precise", "fast"])
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("bounds", [(0, 256, 512), (0, 128, 256, 384, 512), (0, 128, 256, 384, 512, 640, 768, 896, 1024), (0, 576, 1152)],
                         ids=["2-equal", "4-equal", "8-equal", "2-equal-9-parts-each"])
def test_equal_aligned_shards_are_bitwise_equal_to_the_single_plan(bounds, model, mode):
    """W and Y are the same bits only where every plan splits the frame axis alike (the partial covariances of a bin are then the
    same sums): at these shapes every plan chooses the same number of covariance frame splits by itself -- asserted here, not
    assumed (test_every_kernel_family_... below sets the count instead)"""
    import overiva_amd as oa

    X = orc.synth_mixture(T, bounds[-1], M, K, seed=21)
    W1, Y1, _, s1 = _run_single(oa, X, model, mode, 6)
    W2, Y2, _, s2 = _run_sharded(oa, X, model, mode, 6, list(bounds))
    assert all(s == s1 for s in s2), (s1, s2)
    assert np.all(np.isfinite(W1))
    assert np.array_equal(W1, W2)
    assert np.array_equal(Y1, Y2)


# (channels, sources), arithmetic, the covariance and the power kernel the row is there for (csrc/kernel_choice.h)
FAMILIES = [((16, 16), "mixed", "Hmfma", "Lds"), ((16, 16), "precise", "Hmfma64", "Lds"), ((16, 9), "mixed", "Hmfma", "Lds"),
            ((16, 5), "fast", "Half16", "Lds"), ((12, 12), "mixed", "Hmfma", "Mfma"), ((15, 15), "mixed", "Hmfma", "Mfma"),
            ((12, 2), "mixed", "Quad", "Lane"), ((8, 4), "mixed", "Pair32", "Lane"), ((8, 8), "precise", "Pair64", "Lane"),
            ((4, 4), "fast", "Lane", "Lane")]
_single_runs = {}


@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("bounds", [tuple(range(0, 513, 128)), tuple(range(0, 513, 64))], ids=["4-equal", "8-equal"])
@pytest.mark.parametrize("MK,mode,cov_kind,pow_kind", FAMILIES, ids=[f"{mk[0]}x{mk[1]}-{mode}-{ck}-{pk}" for mk, mode, ck, pk in FAMILIES])
def test_every_kernel_family_gives_the_single_plans_bits_on_equal_shards(MK, mode, cov_kind, pow_kind, bounds, model):
    """512 bins as 4 shards of 128 and 8 shards of 64 (every shard whole canonical blocks of the sum over parts; first batches that
    are no multiple of 4), 3 iterations, every covariance and power kernel family: the activations r -- all that crosses between
    the shards, reference overiva.py:152-155 -- are the SAME BITS on every shard as on the single plan.  So are W and Y once
    every plan splits the frame axis alike, which this test establishes itself: the single plan's own split count is set on
    every shard (left alone, a 128-bin plan of 16 x 16 takes 4 splits where the 512-bin one takes fewer) and kernel_choice
    must report the same kernels and frames per split for the shard and the whole."""
    import overiva_amd as oa
    from overiva_amd import plan

    Fa = bounds[-1]
    whole = plan.kernel_choice(T, Fa, MK[0], MK[1], mode, F_total=Fa)
    assert (whole["cov_kind"], whole["pow_kind"]) == (cov_kind, pow_kind)
    splits = whole["nsplit"]
    for r in range(len(bounds) - 1):
        shard = plan.kernel_choice(T, bounds[r + 1] - bounds[r], MK[0], MK[1], mode, F_total=Fa, cov_splits=splits)
        assert all(shard[k] == whole[k] for k in ("cov_kind", "tc", "nsplit", "pow_kind")), (shard, whole)
    key = (MK, mode, model)
    if key not in _single_runs:
        if any(k[:2] != key[:2] for k in _single_runs):      # (the single plan's run is shared by a row's cases, not kept beyond them)
            _single_runs.clear()
        X = orc.synth_iid(T, Fa, MK[0], seed=21 + 16 * MK[0] + MK[1])
        _single_runs[key] = (X,) + _run_single(oa, X, model, mode, 3, MK, splits)
    X, W1, Y1, r1, s1 = _single_runs[key]
    W2, Y2, r2, s2 = _run_sharded(oa, X, model, mode, 3, list(bounds), MK, splits)
    assert s1 == splits and all(s == splits for s in s2), (splits, s1, s2)
    assert np.all(np.isfinite(W1)) and np.all(np.isfinite(r1))
    off = [r for r, ri in enumerate(r2) if not np.array_equal(ri, r1)]
    assert not off, f"r_inv differs from the single plan's on shards {off}"
    assert np.array_equal(W1, W2)
    assert np.array_equal(Y1, Y2)


@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("bounds", [(0, 128, 448), (0, 192, 256, 448)], ids=["2-uneven", "3-uneven"])
def test_unequal_aligned_shards_agree_to_rounding(bounds, model):
    """unequal shards are padded with zero parts to one message size, which shifts the blocks of the canonical sum"""
    import overiva_amd as oa

    X = orc.synth_mixture(T, F, M, K, seed=21)
    W1, Y1 = _run_single(oa, X, model, "precise", 6)[:2]
    W2, Y2 = _run_sharded(oa, X, model, "precise", 6, list(bounds))[:2]
    assert orc.rel_err(W2, W1) < 1e-5 and orc.rel_err(Y2, Y1) < 1e-5


@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_unaligned_shards_agree_to_rounding(model):
    """boundaries inside a 64-bin batch (what shard_bounds gives for world sizes that do not divide the batches)"""
    import overiva_amd as oa
    from overiva_amd.sharded import shard_bounds

    X = orc.synth_mixture(T, F, M, K, seed=22)
    W1, Y1 = _run_single(oa, X, model, "precise", 6)[:2]
    W2, Y2 = _run_sharded(oa, X, model, "precise", 6, shard_bounds(F, 3))[:2]
    assert orc.rel_err(W2, W1) < 1e-5 and orc.rel_err(Y2, Y1) < 1e-5
    _, Wr = orc.overiva_staged(X, n_src=K, n_iter=6, proj_back=False, model=model, return_filters=True)
    assert orc.rel_err(W2, Wr) < 1e-5
