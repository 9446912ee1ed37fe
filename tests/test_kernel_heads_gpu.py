"""The head of the power pass (csrc/demix_arith.h::load_w_raw): how W is LOADED changed, no floating-point operation did.  So every
word must equal what the build before that change computed: ``tests/golden/kernel_heads_parent.json`` holds SHA-256 digests
recorded on that build by tools/record_kernel_heads_golden.py, of the demixing matrix after the prologue's update (``wscale``
null), of the partial powers, the activations, ``wscale``, the weighted covariances and W_hat after one iteration, and of W after
1 and 3 iterations; the three iterations once more from a captured graph.  The shapes are the smallest that take every path of
the new loads: one ragged 64-bin part, one source in the two-source instantiation and a second launch with a lone source, 16- and
8-byte loads of W (7 channels: unaligned rows), the three arithmetic modes, the streamed and the plain power pass.  The frame
counts (1, 2, 10 and 16 block sums behind gamma, short last blocks) and the dense and the ragged batch (the per-problem ``wscale``
and table of the structured per-bin update) are there for the heads of the covariance and update kernels: the same change to
them was tried and is not in the build, and whoever tries again has these digests to meet.  Needs an MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_heads_parent.json")
TOL = 1e-5      # tests/test_x_cache_policy_gpu.py

# (frames, bins, channels, sources, mode, half of X streamed)
CASES = [
    (70, 48, 8, 2, "fast", False),
    (70, 48, 8, 2, "mixed", True),
    (300, 48, 8, 1, "mixed", False),
    (300, 48, 8, 1, "fast", True),
    (300, 48, 8, 3, "mixed", True),
    (300, 48, 8, 3, "fast", False),
    (300, 48, 8, 2, "mixed", True),
    (300, 48, 8, 2, "precise", False),
    (300, 48, 4, 2, "fast", False),
    (300, 48, 4, 1, "mixed", False),
    (300, 48, 6, 2, "mixed", False),
    (300, 48, 6, 3, "fast", False),
    (300, 48, 7, 2, "mixed", False),
    (300, 48, 7, 3, "fast", False),
    (2309, 48, 8, 2, "mixed", True),
    (2309, 48, 8, 2, "fast", False),
    (2309, 48, 6, 2, "precise", False),
    (4000, 16, 8, 2, "mixed", True),
    (4000, 16, 8, 2, "fast", False),
    (4000, 16, 7, 1, "precise", False),
]
# (bins, channels, sources, frames of every problem): a dense batch of two and a ragged batch of two lengths
BATCH_CASES = [(48, 8, 2, (300, 300)), (48, 8, 2, (300, 70)), (48, 6, 1, (2309, 300))]


def case_id(case):
    T, F, M, K, mode, stream = case
    return f"T{T}F{F}M{M}K{K}-{mode}-{'streamed' if stream else 'plain'}"


def batch_id(case):
    F, M, K, frames = case
    return f"batch F{F}M{M}K{K}-" + "+".join(str(t) for t in frames)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_X = {}


def _x(T, F, M, seed=41):
    if (T, F, M, seed) not in _X:
        X = orc.synth_iid(T, F, M, seed=seed)
        X.setflags(write=False)
        _X[T, F, M, seed] = X
    return _X[T, F, M, seed]


def _plan(oa, case):
    T, F, M, K, mode, stream = case
    p = oa.Plan(T, F, M, K, "laplace")
    p.set_precision(mode)
    p.set_resident(False)
    p.set_x(_x(T, F, M))
    p.covariance()
    # half of X (8 of 16 frame groups) within the budget, or every load plain
    p.set_x_resident_mb(8.5 / 16 * T * F * M * 8 / 1e6 if stream else 0)
    return p


def run_case(oa, case, graph=False):
    """the digests of one plan: launched eagerly every stage's output, from a graph the three iterations alone"""
    out = {}
    with _plan(oa, case) as p:
        p.use_graph(graph)
        out["x_resident"] = list(p.x_resident())
        p.set_w(None)
        if not graph:
            out["W0"] = digest(p.get_w(np.complex128))
            p.iterate(1)
            r, wscale = p.t_get_rinv()
            out["Ppart"], out["r"], out["wscale"] = digest(p.t_get_ppart()), digest(r), digest(wscale)
            out["V"], out["What"] = digest(p.t_get_v(np.complex128)), digest(p.t_get_what(np.complex128))
            out["W1"] = digest(p.get_w(np.complex128))
            p.set_w(None)
        p.iterate(3)
        W = p.get_w(np.complex128)
        assert np.all(np.isfinite(W.view(np.float64)))
        out["W3"] = digest(W)
    return out


def run_batch(oa, case):
    F, M, K, frames = case
    Xs = [_x(T, F, M, seed=50 + b) for b, T in enumerate(frames)]
    if len(set(frames)) == 1:
        Y, W = oa.overiva_batch(np.stack(Xs), n_src=K, n_iter=3, return_filters=True)
        Ys = list(Y)
    else:
        Ys, W = oa.overiva_batch_ragged(Xs, n_src=K, n_iter=3, return_filters=True)
    return {"Y": [digest(y) for y in Ys], "W": digest(W)}


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_stage_keeps_the_bits_of_the_parent_build(oa, golden, case):
    got, want = run_case(oa, case), golden[case_id(case)]
    assert got["x_resident"] == want["x_resident"]
    for name in ("W0", "Ppart", "r", "wscale", "V", "What", "W1", "W3"):
        assert got[name] == want[name], name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_iterations_from_a_graph_keep_the_bits(oa, golden, case):
    assert run_case(oa, case, graph=True)["W3"] == golden[case_id(case)]["W3"]


@pytest.mark.parametrize("case", BATCH_CASES, ids=batch_id)
def test_batches_keep_the_bits_of_the_parent_build(oa, golden, case):
    assert run_batch(oa, case) == golden[batch_id(case)]


def test_the_cases_take_both_power_instantiations(golden):
    """the streamed cases really stream (8 of 16 frame groups non-temporally) wherever the geometry allows it, the others never"""
    streamed = [golden[case_id(c)]["x_resident"] for c in CASES if c[5]]
    assert sum(1 for x in streamed if x == [8, True, "share"]) >= 5
    assert all(x[1] is False for x in (golden[case_id(c)]["x_resident"] for c in CASES if not c[5]))


def test_streamed_case_matches_the_oracle(oa):
    """three iterations of a streamed case (overiva.py:140-190) against the oracle"""
    case = (300, 48, 8, 2, "mixed", True)
    T, F, M, K = case[:4]
    _, Wr = orc.overiva_staged(_x(T, F, M), n_src=K, n_iter=3, proj_back=False, return_filters=True)
    with _plan(oa, case) as p:
        assert p.x_resident() == (8, True, "share")
        p.set_w(None)
        p.iterate(3)
        W = p.get_w()
    e_w = orc.rel_err(W, Wr)
    print(f"\n[kernel heads] 300x48x8/2 mixed, half of X streamed, W after 3 iterations against the oracle: {e_w:.2e}")
    assert e_w < TOL
