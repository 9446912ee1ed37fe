"""The per-bin update behind one choice (csrc/kernel_choice.h: choose_update; launch_update and the launchers of the four update
files only turn the choice into template arguments): the same kernel is LAUNCHED for every input as before the choice was one
function, and the kernels compute the same bits.

``tests/golden/update_choice.json`` (tools/update_choice_table.py) and ``tests/golden/update_parent_bits.json``
(tools/ab_plan_bits.py / ab_batch_bits.py ``--update-cases``: per case one SHA-256 over those of W after one and three
iterations and of Y) were recorded on the build BEFORE choose_update existed, the first
through the same captured launch that ``overiva_amd.plan.update_choice`` reads.  The library reads its switches once per process,
so the rows of every non-default switch are swept by one child process each (they load the library with ctypes alone and run side
by side).  The GPU tests need an MI355X; the others check the fixtures themselves."""
import collections
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import update_choice_cases as uc  # noqa: E402
import update_choice_table as table  # noqa: E402

KINDS = ("update_sq_kernel", "update_bg_kernel", "update_gram_kernel", "update_det_kernel", "update_kernel", "update_wave16_kernel",
         "update_det16_kernel", "update_det16r_kernel", "wide_update_kernel")


@pytest.fixture(scope="module")
def choice_rows():
    return table.load(os.path.join(HERE, "golden", "update_choice.json"))


@pytest.fixture(scope="module")
def parent_bits():
    with open(os.path.join(HERE, "golden", "update_parent_bits.json")) as f:
        return json.load(f)


def test_the_table_holds_the_whole_sweep_and_every_kind(choice_rows):
    want = [r for n in range(len(table.SETS)) for r in table.set_rows(n)]
    assert sorted(r[:-1] for r in choice_rows) == sorted(want)
    assert {r[-1].split("<")[0] for r in choice_rows} == set(KINDS)


def test_the_cases_run_every_kind(choice_rows, parent_bits):
    """by the recorded table, the plans of update_choice_cases.py reach all nine kernel families (and the J initialisation), and
    the golden file holds exactly the cases"""
    default = [table.DEFAULTS[s] for s in table.SWITCHES]
    by_input = {tuple(r[:7]): r[-1] for r in choice_rows if r[7:11] == default}
    seen = collections.Counter()
    for c in uc.PLAN_CASES:
        M, K, dbl, init, layout, nsplit = uc.table_row(c)
        for v64 in (0, 1):
            seen[by_input[(M, K, dbl, v64, init, layout, nsplit)].split("<")[0]] += 1
        if K < M:
            seen["init " + by_input[(M, K, dbl, 1, 1, layout, 1)].split("<")[0]] += 1
    assert all(seen[k] for k in KINDS), seen
    assert all(seen["init " + k] for k in ("update_sq_kernel", "update_kernel", "update_wave16_kernel", "wide_update_kernel")), seen
    assert sorted(parent_bits) == sorted([uc.plan_id(c) for c in uc.PLAN_CASES] + [uc.batch_id(c) for c in uc.BATCH_CASES])
    assert len(set(parent_bits.values())) == len(parent_bits)      # no case recorded twice


@pytest.mark.gpu
def test_every_row_launches_the_recorded_kernel(choice_rows):
    """the captured launch of every row -- nothing executes -- names the kernel the parent build launched; the default switches in
    this process through the Python entry, every other set in a process of its own"""
    from overiva_amd.plan import update_choice

    children = [(n, table.spawn(n)) for n in range(1, len(table.SETS))]
    got_rows = [r + [update_choice(r[0], r[1], use_double=r[2], vpart_f64=r[3], init_only=r[4], layout=r[5], nsplit=r[6])]
                for r in table.set_rows(0)]
    for n, proc in children:
        got_rows += table.collect(proc, n)
    want = {tuple(r[:-1]): r[-1] for r in choice_rows}
    assert len(got_rows) == len(want) == len(choice_rows)
    bad = [(g, want[tuple(g[:-1])]) for g in got_rows if g[-1] != want[tuple(g[:-1])]]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("case", uc.PLAN_CASES, ids=uc.plan_id)
def test_plans_keep_the_bits_of_the_parent_build(parent_bits, case):
    import overiva_amd as oa
    from oracle import overiva_oracle as orc

    got = uc.run_plan(oa, orc, case)
    assert uc.combined(got) == parent_bits[uc.plan_id(case)], got


@pytest.mark.gpu
@pytest.mark.parametrize("case", uc.BATCH_CASES, ids=uc.batch_id)
def test_batches_keep_the_bits_of_the_parent_build(parent_bits, case):
    import overiva_amd as oa
    from oracle import overiva_oracle as orc

    got = uc.run_batch(oa, orc, case)
    assert uc.combined(got) == parent_bits[uc.batch_id(case)], got
