"""BSS Eval behind one set of kernel wrappers and one host core (csrc/kernels_bsseval.hip, csrc/bsseval.hip): the wrappers, the
buffer layouts and the host code changed, no floating-point operation did (csrc/bss_arith.h is untouched).  The equalities of
test_bss_eval_gpu.py and test_bss_eval_sets_gpu.py (sets against single calls, ragged against alone, grouped against ungrouped)
compare two users of the same wrappers, so here every word is compared with what the build BEFORE the merge computed:
``tests/golden/bss_eval_parent.json`` holds SHA-256 digests recorded on that build by tools/record_bss_parent_golden.py.

The cases: ``bss_eval_batch`` on the shapes of bss_sets_cases.CASES (two rooms; a second segment of one sample; 8 right-hand sides
and 72 vectors; one live lag in the second 256-lag workgroup; whole blocks; one source) and once on the diagonal pairs alone, whose
NaN pattern is part of the digest; the staged handle's G, D, E, C, c and matrices; five rooms in groups of two (a group offset > 0
and a short last group); a ragged batch; three estimate sets evaluated at once and in two calls; a flagged room next to a healthy
one.  The inputs are those of tests/helpers/bss_eval_cases.py and bss_sets_cases.py.  The GPU tests need an MI355X."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import bss_eval_cases as cases  # noqa: E402
import bss_sets_cases as sets  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "bss_eval_parent.json")

# (kind, B, N, n, Lf)
BATCH_CASES = list(sets.CASES)
STAGED_CASES = BATCH_CASES[:2]
N_SETS = 3


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(names, arrays):
    return {name: digest(a) for name, a in zip(names, arrays)}


MATS = ("sdr", "sir", "sar")


def run_batch(case, compute_permutation=True):
    from overiva_amd import bss_eval_batch

    ref, est = cases.make_case(case)
    out = bss_eval_batch(ref, est, compute_permutation=compute_permutation, filter_length=case[4], return_matrices=True)
    return _digests(("sdr_j", "sir_j", "sar_j", "perm") + MATS, [out[0], out[1], out[2], out[3].astype(np.int64), *out[4:]])


def run_staged(case):
    from overiva_amd.metrics import BssEval

    kind, B, N, n, Lf = case
    ref, est = cases.make_case(case)
    with BssEval([n] * B, N, Lf) as ev:
        ev.set_signals(list(ref), list(est))
        ev.correlate()
        ev.factor()
        out = _digests(("G", "D", "E"), ev.get_gram())
        ev.solve()
        out.update(_digests(("C", "c"), ev.get_filters()))
        ev.criteria()
        out.update(_digests(MATS, ev.get_criteria()))
    return out


def _rooms(kind, N, lens, seed0):
    rooms = [cases.make_room(kind, N, n, seed0 + 100 * b) for b, n in enumerate(lens)]
    return [r for r, _ in rooms], [e for _, e in rooms]


def run_grouped():
    from overiva_amd.metrics import BssEval

    lens = [900] * 5
    ref, est = _rooms("ar", 3, lens, cases.SEED)
    with BssEval(lens, 3, 20, max_group=2) as ev:
        assert ev.group == 2
        ev.set_signals(ref, est)
        ev.run()
        out = _digests(MATS, ev.get_criteria())
        out.update(_digests(("C", "c"), ev.get_filters()))
    return out


def run_ragged():
    from overiva_amd import bss_eval_batch

    ref, est = _rooms("ar", 4, [2048, 2049, 1000], cases.SEED)
    out = bss_eval_batch(ref, est, filter_length=16, return_matrices=True)
    return _digests(("sdr_j", "sir_j", "sar_j", "perm") + MATS, [out[0], out[1], out[2], out[3].astype(np.int64), *out[4:]])


def run_sets(case, split):
    """three sets through one handle, evaluated as (0, 3) or as (0, 1) then (1, 2): the matrices of all sets, D, E, C, c of set 1"""
    from overiva_amd.metrics import BssEvalSets

    kind, B, N, n, Lf = case
    refs, ests = sets.make_rooms(kind, N, [n] * B, N_SETS)
    with BssEvalSets([n] * B, N, Lf, max_sets=N_SETS) as ev:
        ev.set_references(refs)
        ev.prepare()
        for e in range(N_SETS):
            ev.set_estimates(e, [s[e] for s in ests])
        if split:
            ev.evaluate(0, 1)
            ev.evaluate(1, 2)
        else:
            ev.evaluate(0, N_SETS)
        out = _digests(MATS, ev.get_criteria(0, N_SETS))
        out.update(_digests(("D", "E"), ev.get_gram(1, with_g=False)[1:]))
        out.update(_digests(("C", "c"), ev.get_filters(1)))
    return out


def run_flagged():
    """room 0 has two identical references (test_bss_eval_gpu.py::test_flagged_room), room 1 is healthy"""
    from overiva_amd.metrics import BssEval

    N, Lf, n = 2, 8, 700
    rooms = [cases.make_room("white", N, n, 600 + b) for b in range(2)]
    ref, est = np.stack([r for r, _ in rooms]), np.stack([e for _, e in rooms])
    ref[0, 1] = ref[0, 0]
    with BssEval([n] * 2, N, Lf) as ev:
        ev.set_signals(list(ref), list(est))
        ev.run()
        status = ev.status()
        assert list(status) == [True, False]
        out = _digests(MATS, ev.get_criteria(check=False))
    out["status"] = digest(status.astype(np.uint8))
    return out


# case id -> what computes its digests
RUNS = {}
for _case in BATCH_CASES:
    RUNS["batch " + cases.case_id(_case)] = (run_batch, (_case,))
    RUNS["sets " + cases.case_id(_case)] = (run_sets, (_case, False))
    RUNS["sets split " + cases.case_id(_case)] = (run_sets, (_case, True))
RUNS["batch diagonal " + cases.case_id(BATCH_CASES[0])] = (run_batch, (BATCH_CASES[0], False))
for _case in STAGED_CASES:
    RUNS["staged " + cases.case_id(_case)] = (run_staged, (_case,))
RUNS["grouped ar-B5-N3-n900-Lf20-group2"] = (run_grouped, ())
RUNS["ragged ar-N4-Lf16-2048+2049+1000"] = (run_ragged, ())
RUNS["flagged white-B2-N2-n700-Lf8"] = (run_flagged, ())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUNS))
def test_keeps_the_bits_of_the_parent_build(golden, name):
    fn, args = RUNS[name]
    got, want = fn(*args), golden[name]
    assert sorted(got) == sorted(want)
    for key in got:
        assert got[key] == want[key], key


def test_the_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(RUNS)


def test_no_two_cases_share_their_digests(golden):
    """a recorder that ran one case under several names would pass the comparison: different inputs give different digest sets.
    (Evaluating three sets at once or in two calls gives the same bits by design: those two cases of a shape count as one.)"""
    seen = {}
    for name, d in golden.items():
        inputs = name.replace("sets split ", "sets ")
        assert seen.setdefault(json.dumps(d, sort_keys=True), inputs) == inputs, name
    assert len(seen) == len(RUNS) - len(BATCH_CASES)
