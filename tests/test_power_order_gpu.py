"""The power pass walks X against the covariance pass (csrc/kernels_demix.hip): its frame chunks are handed out from
the tail of every covariance split to its head and each chunk is walked descending.  Frames are independent in this pass (the
sums run over bins), so the order may change nothing: every word of the partial powers, and everything computed from them, keeps
its bits whether the switch (``Plan.set_power_reverse`` / ``$OIVA_POWER_REVERSE``) is on or off.  Needs an MI355X."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL_KERNEL = 3e-6   # the bound of test_gpu_parity.test_demix_power (one fp32 pass)


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


_INPUTS = {}


def _inputs(shape):
    """X, two different W_hat and the oracle's powers for the first: computed once per shape, never modified"""
    if shape not in _INPUTS:
        T, F, M, K = shape
        X = orc.synth_iid(T, F, M, seed=11)
        rng = np.random.default_rng(6)
        What = (rng.standard_normal((2, F, M, M)) + 1j * rng.standard_normal((2, F, M, M))).astype(np.complex64)
        ref = orc.demix_power(X, What[0][:, :, :K])
        for a in (X, What, ref):
            a.setflags(write=False)
        _INPUTS[shape] = (X, What, ref)
    return _INPUTS[shape]


ON = [1, 2]      # 1: the default; 2: the chunks tail first even where the grid is one round (these shapes all are)


def _ppart_on_off(oa, shape, cov_splits=0, on=1):
    T, F, M, K = shape
    X, What, ref = _inputs(shape)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("fast")
        p.set_x(X)
        p.covariance()
        if cov_splits:
            p.set_cov_splits(cov_splits)
            assert p.cov_splits() == cov_splits
        p.set_power_reverse(on)
        p.t_set_what(What[0])
        pw_on = p.t_run_power()
        on = p.t_get_ppart()
        # another W in between: the second run of What[0] cannot pass on what the first left in the buffer
        p.t_set_what(What[1])
        p.t_run_power()
        other = p.t_get_ppart()
        p.set_power_reverse(False)
        p.t_set_what(What[0])
        p.t_run_power()
        off = p.t_get_ppart()
    assert on.shape == (-(-F // 64), T, K)
    assert not np.array_equal(on, other)
    return on, off, pw_on, ref


@pytest.mark.parametrize("shape", [(203, 64, 8, 2), (64, 64, 8, 2), (1000, 80, 8, 2), (300, 128, 4, 1)],
                         ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("on", ON)
def test_partial_powers_keep_their_bits(oa, shape, on):
    """ragged last chunk; one chunk; a bin count that is no multiple of the 64 of a part; 4 channels / 1 source (24 workgroups per
    CU's worth of chunks, one source per pass)"""
    on, off, _, _ = _ppart_on_off(oa, shape, on=on)
    assert np.all(np.isfinite(on))
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


@pytest.mark.parametrize("on", ON)
@pytest.mark.parametrize("cov_splits", [1, 2, 4])
def test_partial_powers_keep_their_bits_at_every_covariance_split_count(oa, cov_splits, on):
    """the chunk order follows the covariance geometry the plan runs with, not a fixed 4 x 1000"""
    on, off, _, _ = _ppart_on_off(oa, (517, 128, 8, 2), cov_splits, on=on)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


@pytest.mark.parametrize("on", ON)
def test_reversed_pass_matches_the_oracle(oa, on):
    """overiva.py:140 + :153: the parts summed, against the oracle, to test_demix_power's bound"""
    on, _, pw_on, ref = _ppart_on_off(oa, (203, 64, 8, 2), on=on)
    e_parts = orc.rel_err(on.astype(np.float64).sum(axis=0), ref)
    e_sum = orc.rel_err(pw_on, ref)
    print(f"\n[power order] 203x64x8/2 reversed pass against the oracle: parts summed {e_parts:.2e}, device sum {e_sum:.2e}")
    assert e_parts < TOL_KERNEL and e_sum < TOL_KERNEL


@pytest.mark.parametrize("mode", ["mixed", "fast"])
def test_w_keeps_its_bits_eager_and_from_a_graph(oa, mode):
    """three iterations at 517 x 128 x 8 / 2: the same W with the switch on and off, launched eagerly and replayed from a
    captured graph (toggling the switch drops the captured graphs: a stale one would replay the old order -- harmless for the
    bits, so the eager / graph legs are also compared with each other)"""
    T, F, M, K = 517, 128, 8, 2
    X, _, _ = _inputs((T, F, M, K))
    W = {}
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_resident(False)
        p.set_x(X)
        p.covariance()
        for graph in (False, True):
            p.use_graph(graph)
            for rev in (1, 2, 0):
                p.set_power_reverse(rev)
                p.set_w(None)
                p.iterate(3)
                W[graph, rev] = p.get_w()
    first = W[False, 1]
    assert np.all(np.isfinite(first.view(np.float32)))
    assert not np.array_equal(first[:, :K, :], np.broadcast_to(np.eye(K, dtype=first.dtype), (F, K, K)))      # it iterated
    for key, w in W.items():
        assert np.array_equal(w.view(np.uint32), first.view(np.uint32)), key
