"""The load policy of X in the two streaming passes (csrc/kernel_choice.h::choose_x_policy): a share of the frame
groups is read with plain loads, the rest streams non-temporally and row by row through LDS (cov_dma_kernel's ring, the landing
area of power_kernel).  Only the load instructions and their addressing differ, so every word keeps its bits whatever the share
(``Plan.set_x_resident_mb`` / ``$OIVA_X_RESIDENT_MB``).  The shapes are far below any cache size: they test the addressing and
the choice of the policy per step, not speed.  Needs an MI355X."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
# (frames, bins, channels, sources): a bin count that is no multiple of 16 or 64; one source per pass; 4 channels (the other
# instantiations of the two kernels, which keep their plain loads) with a ragged last bin group; several periods of 16 groups per split
SHAPES = [(70, 401, 8, 2), (300, 64, 8, 1), (333, 33, 4, 2), (1040, 48, 8, 2)]
SPLITS = [1, 2, 4]
N16 = [0, 1, 8, 15, 16]


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


_X = {}


def _x(shape):
    if shape not in _X:
        T, F, M, K = shape
        X = orc.synth_iid(T, F, M, seed=23)
        X.setflags(write=False)
        _X[shape] = X
    return _X[shape]


def _budget_mb(shape, n16):
    """the budget that holds n16 sixteenths of X and not one more; n16 = 16: X whole"""
    T, F, M, _ = shape
    return (n16 + 0.5) / 16 * T * F * M * 8 / 1e6


def _force(p, shape, n16):
    """... and the rule's answer: that share, unless a power chunk is longer than a covariance split (70 frames in 3 splits of 32
    against chunks of 36: a chunk could cross two split boundaries), where it must say so and stream nothing"""
    from overiva_amd.plan import kernel_choice

    p.set_x_resident_mb(_budget_mb(shape, n16))
    c = kernel_choice(*shape, mode=p.mode, cov_splits=p.splits_asked)
    want = (16, False, "fits") if n16 == 16 else (n16, True, "share") if c["tcp"] <= c["tc"] else (0, False, "geometry")
    if shape[2] != 8 and n16 < 16:
        want = (0, False, "kernels")      # the streamed form of the two passes exists at 8 channels: 4 keep their plain loads
    assert p.x_resident() == want
    c = kernel_choice(*shape, mode=p.mode, cov_splits=p.splits_asked, x_resident_mb=_budget_mb(shape, n16))
    assert (c["x_n16"], c["x_nt"], c["x_why"]) == want      # the choice without a plan says the same


def _plan(oa, shape, mode, splits):
    T, F, M, K = shape
    p = oa.Plan(T, F, M, K, "laplace")
    p.mode, p.splits_asked = mode, splits
    p.set_precision(mode)
    p.set_resident(False)
    p.set_x(_x(shape))
    p.covariance()
    p.set_cov_splits(splits)
    tc = -(-(-(-T // splits)) // 16) * 16      # splits are whole steps of 16 frames: 70 frames asked into 4 make 3 of 32
    assert p.cov_splits() == -(-T // tc)
    return p


def _one_iteration(p):
    p.set_w(None)
    p.iterate(1)
    rinv, _ = p.t_get_rinv()
    return p.t_get_ppart(), rinv, p.t_get_v(np.complex128)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_iteration_keeps_its_bits_at_every_share(oa, shape, splits):
    """the partial powers, the activations and the weighted covariances of one iteration"""
    with _plan(oa, shape, "fast", splits) as p:
        p.set_x_resident_mb(0)
        assert p.x_resident() == (0, False, "off")
        off = _one_iteration(p)
        assert all(np.all(np.isfinite(a.view(np.float64) if a.dtype == np.complex128 else a)) for a in off)
        assert np.abs(off[2]).max() > 0
        for n16 in N16:
            _force(p, shape, n16)
            on = _one_iteration(p)
            for name, a, b in zip(("Ppart", "r_inv", "V"), on, off):
                assert np.array_equal(_bits(a), _bits(b)), (name, n16)


@pytest.mark.parametrize("mode", ["mixed", "fast"])
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_w_keeps_its_bits_eager_and_from_a_graph(oa, shape, splits, mode):
    """three iterations, launched eagerly and replayed from a captured graph (the setter drops the captured graphs)"""
    T, F, M, K = shape
    W = {}
    with _plan(oa, shape, mode, splits) as p:
        for graph in (False, True):
            p.use_graph(graph)
            for n16 in [None] + N16:
                if n16 is None:
                    p.set_x_resident_mb(0)
                else:
                    _force(p, shape, n16)
                p.set_w(None)
                p.iterate(3)
                W[graph, n16] = p.get_w()
    first = W[False, None]
    assert np.all(np.isfinite(first.view(np.float32)))
    assert not np.array_equal(first[:, :K, :], np.broadcast_to(np.eye(K, dtype=first.dtype), (F, K, K)))      # it iterated
    for key, w in W.items():
        assert np.array_equal(_bits(w), _bits(first)), key


def test_policy_follows_kernels_and_geometry(oa):
    """the passes of other shapes keep their plain loads; a budget that holds X whole streams nothing"""
    with oa.Plan(64, 32, 6, 2, "laplace") as p:
        p.set_x_resident_mb(0.001)
        assert p.x_resident() == (0, False, "kernels")
    with oa.Plan(300, 64, 8, 2, "laplace") as p:
        assert p.x_resident() == (16, False, "fits")      # the default budget
        p.set_precision("precise")
        p.set_x_resident_mb(0.001)
        assert p.x_resident() == (0, False, "kernels")


def test_streamed_passes_match_the_oracle(oa):
    """half of X streamed: the power pass (overiva.py:140 + :153) and three iterations (:140-190) against the oracle"""
    shape = (300, 64, 8, 2)
    T, F, M, K = shape
    X = _x(shape)
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
    _, Wr = orc.overiva_staged(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)
    with _plan(oa, shape, "mixed", 2) as p:
        _force(p, shape, 8)
        p.set_w(None)
        p.t_set_what(What)
        pw = p.t_run_power()
        parts = p.t_get_ppart()
        p.set_w(None)
        p.iterate(3)
        W = p.get_w()
    ref = orc.demix_power(X, What[:, :, :K])
    e_parts, e_sum, e_w = orc.rel_err(parts.astype(np.float64).sum(axis=0), ref), orc.rel_err(pw, ref), orc.rel_err(W, Wr)
    print(f"\n[x cache policy] 300x64x8/2, n16 = 8 against the oracle: power parts summed {e_parts:.2e}, device sum {e_sum:.2e}, "
          f"W after 3 iterations {e_w:.2e}")
    assert e_parts < TOL and e_sum < TOL and e_w < TOL
