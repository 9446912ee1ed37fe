"""The row instantiation of the 8-channel covariance kernel (csrc/kernels_cov.hip, cov_dma_kernel<8, KC, true>: every load step
requested row by row, plain or non-temporal at the same addresses, through a shorter ring), launched exactly where the load
policy of X streams.  Only the load instructions, their addressing and the ring differ from the lane-addressed instantiation,
which ``Plan.set_cov_rows(False)`` forces: every word keeps its bits.  The shapes are the smallest at which the loop can go
wrong -- splits shorter than the ring, every remainder of the unrolled loop, frames past the end inside a step, a ragged bin
group -- and far below any cache size.  Needs an MI355X.

Three sources on 8 channels are not a case of this kernel: the plan takes them to the pair kernel (four sources per pass,
kernels_cov_pair32.hip), the policy answers ``kernels`` and nothing streams.  The cases are kept: the plan must then report the
lane form, whatever the switch says.  So no plan launches the row instantiation with more than one pass along z (``gridDim.z``
> 1 needs more sources than a pass takes, and two sources are one pass of KC = 2): that geometry is unreachable for the row
form, and no test here covers it."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
M = 8
BINS = [17, 48]                              # a ragged second bin group (its clamped bins requested, never stored); whole groups
SOURCES = [1, 2, 3]                          # KC = 1, KC = 2, two launches along z
SHORT = [1, 15, 17, 33, 49, 65, 81]          # 1 .. 6 steps of 16 frames in one split, the last one ragged
LONG, LONG_SPLITS = 1040, [1, 2, 4]          # several periods of 16 groups; splits of 272 and 528 frames end inside a period
N16 = [1, 8, 15]


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


_X = {}


def _x(T, F):
    if (T, F) not in _X:
        X = orc.synth_iid(T, F, M, seed=31)
        X.setflags(write=False)
        _X[T, F] = X
    return _X[T, F]


def _plan(oa, T, F, K, mode, splits):
    p = oa.Plan(T, F, M, K, "laplace")
    p.set_precision(mode)
    p.set_resident(False)
    p.set_x(_x(T, F))
    p.covariance()
    p.set_cov_splits(splits)
    tc = -(-(-(-T // splits)) // 16) * 16
    assert p.cov_splits() == -(-T // tc)
    p.tc = tc
    return p


def _force(p, n16):
    """a budget of n16 sixteenths of X (tests/test_x_cache_policy_gpu.py::_force); where the rule's power chunks are longer than a
    covariance split, chunks that fit.  Returns whether the policy streams: always, but for the pair kernel's three sources."""
    p.set_pow_splits(0)
    p.set_x_resident_mb((n16 + 0.5) / 16 * p.T * p.F * M * 8 / 1e6)
    if p.x_resident()[2] == "geometry":
        p.set_pow_splits(-(-p.T // (p.tc // 4 * 4)))
    if p.K >= 3:
        assert p.x_resident() == (0, False, "kernels")
        return False
    assert p.x_resident() == (n16, True, "share")
    return True


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _one_iteration(p):
    p.set_w(None)
    p.iterate(1)
    _, wscale = p.t_get_rinv()
    return p.t_get_v(np.complex128), wscale


def _both_forms(p, streams, what):
    """`what(p)` under the row form and under the forced lane form, from the same start; the plan says which one runs"""
    out = []
    for rows in (True, False):
        p.set_cov_rows(rows)
        assert p.cov_rows() == (rows and streams)
        out.append(what(p))
    p.set_cov_rows(True)
    return out


def _check_one_iteration(p, streams, tag):
    (v_rows, s_rows), (v_lane, s_lane) = _both_forms(p, streams, _one_iteration)
    assert np.all(np.isfinite(v_lane.view(np.float64))) and np.abs(v_lane).max() > 0, tag
    assert np.array_equal(_bits(v_rows), _bits(v_lane)), ("V", tag)
    assert np.array_equal(_bits(s_rows), _bits(s_lane)), ("wscale", tag)


def _three_iterations(p):
    p.set_w(None)
    p.iterate(3)
    # (fewer frames than channels: singular covariances, which get_w refuses; the state as it lies on the device, same bits still)
    return p.get_w() if p.T >= 2 * M else p.t_get_what(np.complex128)


def _check_w(p, streams, tag):
    W = {}
    for graph in (False, True):
        p.use_graph(graph)
        W[graph, True], W[graph, False] = _both_forms(p, streams, _three_iterations)
    p.use_graph(False)
    first = W[False, False]
    if p.T >= 2 * M:
        assert np.all(np.isfinite(first.view(np.float32))), tag
        assert not np.array_equal(first[:, :p.K, :], np.broadcast_to(np.eye(p.K, dtype=first.dtype), (p.F, p.K, p.K))), tag      # it iterated
    for key, w in W.items():
        assert np.array_equal(_bits(w), _bits(first)), (key, tag)


@pytest.mark.parametrize("mode", ["mixed", "fast"])
@pytest.mark.parametrize("K", SOURCES)
@pytest.mark.parametrize("F", BINS)
def test_short_splits_keep_their_bits(oa, F, K, mode):
    """one split of 1 .. 6 steps: V and wscale after one iteration, W after three, eager and from a captured graph"""
    for T in SHORT:
        with _plan(oa, T, F, K, mode, 1) as p:
            for n16 in N16:
                streams = _force(p, n16)
                _check_one_iteration(p, streams, (T, n16))
                _check_w(p, streams, (T, n16))


@pytest.mark.parametrize("mode", ["mixed", "fast"])
@pytest.mark.parametrize("splits", LONG_SPLITS)
@pytest.mark.parametrize("K", SOURCES)
def test_long_splits_keep_their_bits(oa, K, splits, mode):
    """1040 frames in 1, 2 and 4 splits: whole periods of 16 groups and splits that end inside one"""
    for F in BINS:
        with _plan(oa, LONG, F, K, mode, splits) as p:
            for n16 in N16:
                streams = _force(p, n16)
                _check_one_iteration(p, streams, (F, n16))
                _check_w(p, streams, (F, n16))


def test_form_follows_the_policy(oa):
    """the row form exactly where the policy answers `share`; the lane form under `fits`, `off` and the switch"""
    with _plan(oa, 81, 17, 2, "mixed", 1) as p:
        assert p.x_resident() == (16, False, "fits") and not p.cov_rows()      # the default budget
        p.set_x_resident_mb(0)
        assert p.x_resident() == (0, False, "off") and not p.cov_rows()
        assert _force(p, 8) and p.cov_rows()
        p.set_cov_rows(False)
        assert p.x_resident() == (8, True, "share") and not p.cov_rows()
        p.set_cov_rows(True)
        assert p.cov_rows()
        p.set_precision("precise")                                              # float64 sums: another kernel
        assert p.x_resident()[2] == "kernels" and not p.cov_rows()
    with oa.Plan(333, 33, 4, 2, "laplace") as p:                                # 4 channels keep their one instantiation
        p.set_x_resident_mb(0.001)
        assert p.x_resident() == (0, False, "kernels") and not p.cov_rows()


def test_both_forms_hold_two_workgroups_per_cu(oa):
    """the geometry is chosen on the lane form's occupancy (cov_blocks_per_cu); the row form must hold as many"""
    import ctypes as C

    from overiva_amd import _lib

    for kc in (1, 2):
        n = {}
        for rows in (0, 1):
            v = C.c_int()
            _lib.check(_lib.load().oiva_test_cov_blocks_per_cu(M, kc, rows, C.byref(v)))
            n[rows] = v.value
        assert n[0] == 2 and n[1] >= 2, (kc, n)


@pytest.mark.parametrize("K", [1, 2])
def test_weighted_covariance_matches_a_float64_sum(oa, K):
    """V_k[f] = sum_t w[t, k] x x^H (overiva.py:179) of the row form, five steps and a ragged bin group, half of X streamed"""
    T, F = 81, 17
    rinv = np.random.default_rng(5 + K).gamma(2.0, 1.0, (T, K)).astype(np.float32)
    with _plan(oa, T, F, K, "mixed", 1) as p:
        assert _force(p, 8) and p.cov_rows()
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
    e = orc.rel_err(V, orc.weighted_cov_all(_x(T, F), rinv.astype(np.float64)))
    print(f"\n[cov rows] 81x17x8/{K}, n16 = 8 against the float64 sum: V {e:.2e}")
    assert e < TOL
