"""tests/golden/kernel_census.json (tools/kernel_census.py) against the build: every compiled ``__global__`` instantiation is in
the census, and the census names a GPU test file whose traced run launched it.

What this test cannot notice: a test that later STOPS launching a kernel.  The file says what the traced runs of the day it was
recorded launched; only recording it again (tools/README.md, "Kernel census") shows a kernel that has lost its test.  What it does
notice: a new or renamed instantiation (not in the file), and a census recorded while a kernel had no test."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))

import kernel_census as kc  # noqa: E402


@pytest.fixture(scope="module")
def census():
    with open(kc.CENSUS) as f:
        return json.load(f)


def test_names_are_brought_to_one_form():
    """what the demangler of the build prints and what a dispatch trace holds"""
    want = "update_bg_kernel<8, double, 8, 2>"
    for raw in ("void oiva::update_bg_kernel<8, double, 8, 2>(oiva::UpdateArgs)",
                "void oiva::(anonymous namespace)::update_bg_kernel<8, double, 8, 2>(oiva::UpdateArgs) [clone .kd]",
                "oiva::update_bg_kernel<8,double,8,2>(oiva::UpdateArgs).kd",
                '"void oiva::update_bg_kernel<(int)8, double, (int)8, (int)2>(oiva::UpdateArgs)"'):
        assert kc.normalise(raw) == want, raw
    assert kc.normalise("void oiva::cov_kernel<3, 1, (bool)0, double>(float const*, HIP_vector_type<float, 2u>*)") == "cov_kernel<3, 1, false, double>"
    assert kc.normalise("void oiva::push_kernel<HIP_vector_type<float, 4u> >(void*)") == "push_kernel<HIP_vector_type<float, 4>>"
    assert kc.normalise("oiva::room_std_kernel(float*, int)") == "room_std_kernel"
    assert kc.family("cov_kernel<3, 1, false, double>") == "cov_kernel"


def test_the_census_holds_exactly_the_compiled_kernels(census):
    """a new or renamed instantiation fails here until the census is recorded again"""
    compiled = kc.compiled_sources()
    if len(compiled) < 100:
        pytest.skip("resource remarks not available (library built without them)")
    have = census["kernels"]
    assert sorted(set(compiled) - set(have)) == [], "compiled, not in the census: record it again (tools/README.md)"
    assert sorted(set(have) - set(compiled)) == [], "in the census, no longer compiled: record it again (tools/README.md)"
    assert {k: v["source"] for k, v in have.items()} == compiled


def test_every_kernel_names_a_test_file(census):
    """no exemption list: a kernel that cannot get a test is one that nothing can launch, and is deleted instead (of the 92
    instantiations the suite did not launch when the census was first taken, 60 got a test and 32 were deleted: DESIGN.md §4.1)"""
    files = census["files"]
    never = sorted(k for k, v in census["kernels"].items() if not v["tests"])
    assert never == [], (len(never), never[:20])
    for k, v in census["kernels"].items():
        for t in v["tests"]:
            assert t in files and os.path.exists(os.path.join(REPO, t)), (k, t)


def test_the_trust_check_is_recorded(census):
    """three kernels that run only from a replayed graph and three that run only in a child process were looked for in the trace;
    a file whose trace missed its kernels is marked, with the reason"""
    t = census["trust_check"]
    for key in ("graph_replay", "child_process"):
        assert len(t[key]["kernels"]) >= 3 and isinstance(t[key]["seen"], bool) and t[key]["how"], key
        assert all(k in census["kernels"] for k in t[key]["kernels"]), key
    for f in kc.CHILD_FILES:
        assert f in census["files"]
    for f, e in census["files"].items():
        assert e["traced"] is True or e.get("reason"), f
        if f in kc.CHILD_FILES and e["traced"]:
            assert e["processes"] >= 2, f
    if not t["graph_replay"]["seen"]:
        assert not any(e["traced"] for e in census["files"].values())
