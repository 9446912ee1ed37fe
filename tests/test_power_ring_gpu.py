"""The streamed instantiation of the power pass (csrc/kernels_demix.hip, power_kernel<8, KP, true>) and the chunk rule that
goes with it (csrc/kernel_choice.h::choose_pow).  Every load step goes HBM -> LDS row by row into a two-stage ring per wave, the
wave waits with a counted vmcnt for the step it consumes and stores the step's sums to LDS out of the compiler's sight; where X
streams the pass takes one workgroup per CU.  Only the way X reaches the registers and the chunking differ from the plain
instantiation at the policy's "off", so every word of Ppart keeps its bits against the same plan with
``Plan.set_x_resident_mb(0)``, whatever the share, the walk and the chunk count.  The shapes are far below any cache size: they
test the ring's bookkeeping (chunks shorter than the ring, ragged ends, requests past the end, the policy per step across
periods and split boundaries, chunks at the cap of 512 frames handed out by the host-made table), not speed.
Needs an MI355X."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N16 = [0, 1, 8, 15]
REV = [1, 0]


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


_INPUTS = {}


def _inputs(shape):
    """X and a W_hat: computed once per shape, never modified"""
    if shape not in _INPUTS:
        T, F, M, K = shape
        X = orc.synth_iid(T, F, M, seed=29)
        rng = np.random.default_rng(8)
        What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
        for a in (X, What):
            a.setflags(write=False)
        _INPUTS[shape] = (X, What)
    return _INPUTS[shape]


def _plan(oa, shape, mode, cov_splits):
    T, F, M, K = shape
    p = oa.Plan(T, F, M, K, "laplace")
    p.set_precision(mode)
    p.set_resident(False)
    p.set_x(_inputs(shape)[0])
    p.covariance()
    p.set_cov_splits(cov_splits)
    return p


def _share(p, shape, n16):
    """the budget that holds n16 sixteenths of X and not one more: the pass must stream, not fall back to plain"""
    T, F, M, _ = shape
    p.set_x_resident_mb((n16 + 0.5) / 16 * T * F * M * 8 / 1e6)
    assert p.x_resident() == (n16, True, "share")


def _ppart(p, What):
    p.t_set_what(What)
    pw = p.t_run_power()
    return p.t_get_ppart(), pw


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_all_shares(oa, shape, cov_splits, pow_splits=0, revs=REV, n16s=N16):
    X, What = _inputs(shape)
    with _plan(oa, shape, "fast", cov_splits) as p:
        if pow_splits:
            p.set_pow_splits(pow_splits)
        p.set_x_resident_mb(0)
        assert p.x_resident() == (0, False, "off")
        p.set_power_reverse(0)
        off, _ = _ppart(p, What)
        assert np.all(np.isfinite(off)) and np.abs(off).max() > 0
        for rev in revs:
            p.set_power_reverse(rev)
            for n16 in n16s:
                _share(p, shape, n16)
                # zeros in between: a pass that skipped a word cannot pass on what the last one left there
                p.t_set_what(np.zeros_like(What))
                p.t_run_power()
                on, _ = _ppart(p, What)
                assert np.array_equal(_bits(on), _bits(off)), (rev, n16)


@pytest.mark.parametrize("T", [8, 12])
def test_a_chunk_shorter_than_the_ring(oa, T):
    """two and three steps: the prologue, one turn of the loop, the odd step behind it, requests past the end"""
    _check_all_shares(oa, (T, 64, 8, 2), 1)


@pytest.mark.parametrize("cov_splits", [1, 2])
def test_ragged_frames_and_bins(oa, cov_splits):
    """T no multiple of 4, a short last chunk, a bin count that is no multiple of 16 or 64"""
    _check_all_shares(oa, (70, 401, 8, 2), cov_splits)


def test_one_source_per_pass(oa):
    _check_all_shares(oa, (300, 64, 8, 1), 2)


@pytest.mark.parametrize("cov_splits", [1, 2, 4])
def test_several_periods_and_a_chunk_across_a_split_boundary(oa, cov_splits):
    _check_all_shares(oa, (1040, 48, 8, 2), cov_splits)


@pytest.mark.parametrize("pow_splits", [1, 2, 7])
def test_chunk_counts(oa, pow_splits):
    """one chunk of 300 frames, two of 152 and 148, seven of 44"""
    _check_all_shares(oa, (300, 64, 8, 1), 1, pow_splits=pow_splits, n16s=[0, 8])


def test_capped_chunks_in_the_host_made_order(oa):
    """1100 frames asked into one chunk: tcp at its cap of 512, three chunks (the last of 76 frames), the middle one across the
    boundary of the two covariance splits of 560; reverse = 2: the chunks are handed out by the host-made table"""
    _check_all_shares(oa, (1100, 64, 8, 2), 2, pow_splits=1, revs=[2, 1, 0], n16s=[1, 8])


def test_streamed_power_pass_matches_the_oracle(oa):
    """overiva.py:140 + :153: the parts summed and the device's own sum against the oracle"""
    shape = (70, 401, 8, 2)
    X, What = _inputs(shape)
    with _plan(oa, shape, "mixed", 2) as p:
        _share(p, shape, 8)
        parts, pw = _ppart(p, What)
    ref = orc.demix_power(X, What[:, :, :shape[3]])
    e_parts, e_sum = orc.rel_err(parts.astype(np.float64).sum(axis=0), ref), orc.rel_err(pw, ref)
    print(f"\n[streamed power pass] 70x401x8/2, n16 = 8 against the oracle: parts summed {e_parts:.2e}, device sum {e_sum:.2e}")
    assert e_parts < TOL and e_sum < TOL


@pytest.mark.parametrize("mode", ["mixed", "fast"])
def test_w_keeps_its_bits_eager_and_from_a_graph(oa, mode):
    """three iterations with the policy off and at two shares, launched eagerly and replayed from a captured graph"""
    shape = (1040, 48, 8, 2)
    T, F, M, K = shape
    W = {}
    with _plan(oa, shape, mode, 2) as p:
        for graph in (False, True):
            p.use_graph(graph)
            for n16 in (None, 0, 8):
                if n16 is None:
                    p.set_x_resident_mb(0)
                else:
                    _share(p, shape, n16)
                p.set_w(None)
                p.iterate(3)
                W[graph, n16] = p.get_w()
    first = W[False, None]
    assert np.all(np.isfinite(first.view(np.float32)))
    assert not np.array_equal(first[:, :K, :], np.broadcast_to(np.eye(K, dtype=first.dtype), (F, K, K)))      # it iterated
    for key, w in W.items():
        assert np.array_equal(_bits(w), _bits(first)), key


def test_chunks_where_x_streams(oa):
    """the rule: one workgroup per CU where X streams at 8 channels / two sources and such a grid exists; everything else keeps
    the chunks it had (2049 bins: 33 x 8 workgroups are more than one per CU; `precise` and the shards do not stream)"""
    from overiva_amd.plan import kernel_choice

    c = kernel_choice(4000, 2048, 8, 2, "mixed")
    if c["n_cu"] != 256:
        pytest.skip(f"the figures are those of 256 CUs, this device has {c['n_cu']}")
    assert (c["pow_nsplit"], c["tcp"], c["rounds"]) == (8, 500, 1) and (c["x_nt"], c["x_why"]) == (True, "share")
    assert c["nb"] * c["pow_nsplit"] == c["n_cu"]
    c = kernel_choice(4000, 2049, 8, 2, "fast")
    assert (c["pow_nsplit"], c["tcp"]) == (11, 364) and c["x_nt"]
    c = kernel_choice(4000, 2048, 8, 2, "precise")
    assert (c["pow_nsplit"], c["tcp"]) == (12, 336) and c["x_why"] == "kernels"
    c = kernel_choice(4000, 1024, 8, 2, "mixed")
    assert (c["pow_nsplit"], c["tcp"]) == (24, 168) and c["x_why"] == "fits"
    c = kernel_choice(4000, 2048, 8, 1, "mixed")
    assert (c["pow_nsplit"], c["tcp"]) == (24, 168)      # one source per pass: not measured, as before
    c = kernel_choice(4000, 2048, 4, 2, "mixed")
    assert (c["pow_nsplit"], c["tcp"]) == (24, 168) and c["x_why"] == "fits"

