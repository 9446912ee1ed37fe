"""bss_eval_sets_batch() / BssEvalSets on the GPU against bss_eval_batch() / BssEval on every set alone.

There is no tolerance here: for every room and set the new path must give the bits of the existing one (NaN patterns included),
which tests/test_bss_eval_gpu.py holds to the NumPy restatement of DESIGN.md 3.10.  Both paths run the same chains of additions
(csrc/bss_arith.h); the set is an axis of the grid.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import bss_eval_cases as cases  # noqa: E402
import bss_sets_cases as sets_cases  # noqa: E402
from bss_sets_cases import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


def _single(ref_b, est_be, Lf, **kw):
    """what bss_eval_batch gives on one room and one set: the seven outputs, without the batch axis"""
    from overiva_amd import bss_eval_batch

    return tuple(o[0] for o in bss_eval_batch(ref_b[None], est_be[None], filter_length=Lf, return_matrices=True, **kw))


def _assert_equals_single_calls(out, refs, sets, Lf, rooms=None, **kw):
    E = sets[0].shape[0]
    for b in (range(len(refs)) if rooms is None else rooms):
        for e in range(E):
            one = _single(refs[b], sets[b][e], Lf, **kw)
            for name, got, want in zip(("sdr", "sir", "sar", "perm", "SDR", "SIR", "SAR"), out, one):
                assert same_bits(got[b][e], want), (name, b, e, got[b][e], want)


@pytest.mark.parametrize("case", sets_cases.CASES, ids=cases.case_id)
def test_sets_equal_single_calls(case):
    from overiva_amd import bss_eval_sets_batch, last_batch_info

    kind, B, N, n, Lf = case
    refs, sets = sets_cases.make_rooms(kind, N, [n] * B, 3)
    out = bss_eval_sets_batch(np.stack(refs), np.stack(sets), filter_length=Lf, return_matrices=True)
    info = last_batch_info()
    assert info["algorithm"] == "bss_eval_sets" and info["n_sets"] == 3 and info["reference_preparations"] == 1
    assert info["batched"] == B and info["n_sources"] == N and info["filter_length"] == Lf and info["n_samples"] == n
    assert [o.shape for o in out] == [(B, 3, N)] * 4 + [(B, 3, N, N)] * 3
    _assert_equals_single_calls(out, refs, sets, Lf)
    if N == 1:
        assert np.isposinf(out[1]).all()


def test_sets_equal_single_calls_without_the_permutation():
    from overiva_amd import bss_eval_sets_batch

    kind, B, N, n, Lf = sets_cases.CASES[1]
    refs, sets = sets_cases.make_rooms(kind, N, [n] * B, 3)
    out = bss_eval_sets_batch(np.stack(refs), np.stack(sets), compute_permutation=False, filter_length=Lf, return_matrices=True)
    _assert_equals_single_calls(out, refs, sets, Lf, compute_permutation=False)
    assert np.isnan(out[4][:, :, ~np.eye(N, dtype=bool)]).all() and np.isfinite(out[4][:, :, np.eye(N, dtype=bool)]).all()
    assert (out[3] == np.arange(N)).all()


def test_ragged_rooms():
    from overiva_amd import bss_eval_sets_batch, last_batch_info

    lens, N, Lf = [2048, 2049, 1000], 4, 16
    refs, sets = sets_cases.make_rooms("white", N, lens, 2)
    out = bss_eval_sets_batch(refs, sets, filter_length=Lf, return_matrices=True)
    info = last_batch_info()
    assert info["ragged"] is True and info["lengths"] == lens and info["batched"] == 3 and "n_samples" not in info
    _assert_equals_single_calls(out, refs, sets, Lf)


def test_a_sets_bits_depend_on_nothing_but_the_set():
    from overiva_amd import bss_eval_sets_batch
    from overiva_amd.metrics import BssEvalSets

    N, Lf, n, B, E = 3, 20, 900, 2, 4
    refs, sets = sets_cases.make_rooms("ar", N, [n] * B, E)
    ref, est = np.stack(refs), np.stack(sets)
    together = bss_eval_sets_batch(ref, est, filter_length=Lf, return_matrices=True)
    order = [2, 0, 3, 1]
    permuted = bss_eval_sets_batch(ref, est[:, order], filter_length=Lf, return_matrices=True)
    grouped = bss_eval_sets_batch(ref, est, filter_length=Lf, return_matrices=True, max_group=1)
    for e in range(E):
        alone = bss_eval_sets_batch(ref, est[:, e:e + 1], filter_length=Lf, return_matrices=True)
        for t, a, p, g in zip(together, alone, permuted, grouped):
            assert same_bits(t[:, e], a[:, 0]), e
            assert same_bits(t[:, e], p[:, order.index(e)]), e
            assert same_bits(t[:, e], g[:, e]), e
    # on the handle: all four sets in one evaluate, and one evaluate per set
    with BssEvalSets([n] * B, N, Lf, max_sets=E) as ev:
        ev.set_references(refs)
        ev.prepare()
        for e in range(E):
            ev.set_estimates(e, [s[e] for s in sets])
        ev.evaluate(0, E)
        at_once = ev.get_criteria(0, E)
        for e in (3, 1, 0, 2):
            ev.evaluate(e, 1)
        one_by_one = ev.get_criteria(0, E)
        assert ev.counts() == (1, 2 * E)
    for t, a, o in zip(together[4:], at_once, one_by_one):
        assert same_bits(t, a) and same_bits(t, o)


def test_staged_handle():
    from overiva_amd import _lib
    from overiva_amd.metrics import BssEval, BssEvalSets

    N, Lf, lens = 2, 33, [700, 655]
    refs, sets = sets_cases.make_rooms("white", N, lens, 2)
    with BssEvalSets(lens, N, Lf, max_sets=2) as ev:
        with pytest.raises(RuntimeError, match="references not set"):
            ev.prepare()
        ev.set_references(refs)
        ev.set_estimates(0, [s[0] for s in sets])
        with pytest.raises(RuntimeError, match="prepare has not run"):
            ev.evaluate(0, 1)
        assert ev.lib.oiva_bsssets_evaluate(ev.h, 0, 1) == _lib.ERR_STATE
        ev.prepare()
        with pytest.raises(RuntimeError, match="the estimates of set 1 are not set"):
            ev.evaluate(0, 2)
        with pytest.raises(ValueError):
            ev.evaluate(1, 2)
        for rnd in range(2):
            est = [s[rnd] for s in sets]
            ev.set_estimates(0, est)
            with pytest.raises(RuntimeError, match="has not been evaluated"):
                ev.get_criteria(0, 1)
            ev.evaluate(0, 1)
            assert not ev.status().any()
            with BssEval(lens, N, Lf) as fresh:
                fresh.set_signals(refs, est)
                fresh.run()
                want = fresh.get_gram() + fresh.get_filters() + fresh.get_criteria()
            got = ev.get_gram(0) + ev.get_filters(0) + tuple(m[:, 0] for m in ev.get_criteria(0, 1))
            for name, g, w in zip(("G", "D", "E", "C", "c", "sdr", "sir", "sar"), got, want):
                assert same_bits(g, w), (rnd, name)
        assert ev.counts() == (1, 2)
        ms = ev.phase_ms()
        assert list(ms) == ["prepare", "correlate", "solve", "criteria"] and all(v > 0.0 for v in ms.values())
        info = ev.info()
        assert info["algorithm"] == "bss_eval_sets" and info["reference_preparations"] == 1 and info["sets_evaluated"] == 2
        # new references drop the preparation
        ev.set_references([r[::-1].copy() for r in refs])
        with pytest.raises(RuntimeError, match="prepare has not run"):
            ev.evaluate(0, 1)
        ev.prepare()
        ev.evaluate(0, 1)
        assert ev.counts() == (2, 3)


def test_take_from_a_bss_eval_handle():
    from overiva_amd import _lib
    from overiva_amd.metrics import BssEval, BssEvalSets

    N, Lf, lens = 3, 20, [900, 640]
    refs, sets = sets_cases.make_rooms("ar", N, lens, 1)
    est = [s[0] for s in sets]
    with BssEval(lens, N, Lf) as ev, BssEvalSets(lens, N, Lf, max_sets=2) as st:
        ev.set_signals(refs, est)
        st.take(ev, 1, with_references=True)
        st.prepare()
        st.evaluate(1, 1)
        got = tuple(m[:, 0] for m in st.get_criteria(1, 1))
        ev.run()
        for g, w in zip(got, ev.get_criteria()):
            assert same_bits(g, w)
        # estimates alone keep the preparation
        st.take(ev, 0)
        st.evaluate(0, 1)
        for g, w in zip(st.get_criteria(0, 1), got):
            assert same_bits(g[:, 0], w)
        assert st.counts() == (1, 2)
        for other, what in ((dict(lengths=[900, 641]), "length of room 1"), (dict(N=2), "differ in N"),
                            (dict(filter_length=21), "filter_length"), (dict(lengths=[900]), "differ in B")):
            a = dict(lengths=lens, N=N, filter_length=Lf)
            a.update(other)
            with BssEvalSets(a["lengths"], a["N"], a["filter_length"]) as wrong:
                assert wrong.lib.oiva_bsssets_take(wrong.h, ev.h, 0, 1) == _lib.ERR_ARG
                with pytest.raises(ValueError, match=what):
                    wrong.take(ev, 0, with_references=True)
        with pytest.raises(ValueError):
            st.take(ev, 2)


def test_flagged_room():
    from overiva_amd import bss_eval_sets_batch
    from overiva_amd.metrics import BssEvalSets

    N, Lf, n, E = 2, 33, 700, 2
    rooms = [cases.make_room("white", N, n, 600 + b) for b in range(3)]
    ref = np.stack([r for r, _ in rooms])
    ref[1, 1] = ref[1, 0]                                 # room 1: two identical references
    sets = [sets_cases.make_sets(ref[b], E, 650 + b) for b in range(3)]
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1$"):
        bss_eval_sets_batch(ref, np.stack(sets), filter_length=Lf)
    with BssEvalSets([n] * 3, N, Lf, max_sets=E) as ev:
        ev.set_references(list(ref))
        ev.prepare()
        for e in range(E):
            ev.set_estimates(e, [s[e] for s in sets])
        ev.evaluate(0, E)
        assert list(ev.status()) == [False, True, False] and int(ev.status().sum()) == 1
        with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1$"):
            ev.get_criteria(0, E)
        mats = ev.get_criteria(0, E, check=False)
    for m in mats:
        assert np.isnan(m[1]).all()
    for b in (0, 2):
        for e in range(E):
            one = _single(ref[b], sets[b][e], Lf)
            for m, w in zip(mats, one[4:]):
                assert same_bits(m[b, e], w), (b, e)


def test_one_room_call():
    from overiva_amd import bss_eval_sets, bss_eval_sources

    N, Lf, n = 2, 33, 700
    refs, sets = sets_cases.make_rooms("white", N, [n], 2)
    out = bss_eval_sets(refs[0], sets[0], filter_length=Lf)
    assert [o.shape for o in out] == [(2, N)] * 4
    for e in range(2):
        one = bss_eval_sources(refs[0], sets[0][e], filter_length=Lf)
        for o, w in zip(out, one):
            assert same_bits(o[e], w)


def test_the_sweep_prepares_the_references_once_per_group():
    """the bit equality of the sweep with the chain is tests/test_sweep_gpu.py; here: what the sweep's evaluations cost"""
    import overiva_amd as oa
    import sweep_chain as sc

    args = sc.scene("ragged", 2)
    args = sc.sweep_args(sc.with_noise(args, sc.out_lengths(args)))
    block = {"o": {"algo": "overiva", "kwargs": {"n_iter": 12}}, "a": {"algo": "auxiva", "kwargs": {"n_iter": 25}}}
    marks = [oa.sweep.checkpoints("overiva", 12, True), oa.sweep.checkpoints("auxiva", 25, True)]
    assert marks == [[0, 10, 12], [0, 10, 20, 25]]
    got = oa.sweep_batch(algorithms=block, monitor_convergence=True, **args)
    assert [r["checkpoints"] for r in got] == marks
    info = oa.last_batch_info()
    assert info["groups"] == [3] and info["evaluation"] == "bss_eval_sets" and info["groups_without_sets"] == 0
    assert info["reference_preparations"] == 1 and info["sets_evaluated"] == 3 + 4
    oa.sweep_batch(algorithms=block, monitor_convergence=True, max_group=1, **args)
    info = oa.last_batch_info()
    assert info["groups"] == [1, 1, 1] and info["reference_preparations"] == 3 and info["sets_evaluated"] == 3 * (3 + 4)
    # without monitoring: the shared evaluation of the unprocessed microphones and one final state per entry
    oa.sweep_batch(algorithms=block, **args)
    info = oa.last_batch_info()
    assert info["reference_preparations"] == 1 and info["sets_evaluated"] == 1 + 2
