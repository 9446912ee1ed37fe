"""Host-side checks of the row instantiation of the 8-channel covariance kernel (csrc/kernels_cov.hip): the launch rule
(csrc/kernel_choice.h::cov_rows_form, through the host-only hook oiva_test_cov_rows) and what the compiler made of the
instantiation (the resource remarks the build keeps next to the objects).  No GPU needed.  That ``cov_blocks_per_cu`` still answers
2 is an occupancy query and needs a device: tests/test_cov_rows_gpu.py::test_both_forms_hold_two_workgroups_per_cu asks it; here
the remarks are checked for what that answer follows from (registers, scratch, LDS, waves per SIMD)."""
import ctypes as C
import os
import re

import pytest

from test_x_cache_policy_host import F, GEOMS, M, REASONS, _x_mb

LANE, PREC_COV_F64 = 0, 4      # CovKind::Lane / PowKind::Lane; OIVA_PREC_COV_F64


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import build, _lib

    build.build_library()
    assert _lib.PREC_COV_F64 == PREC_COV_F64
    return _lib.load()


def _rows(lib, T, ctc, tcp, budget_mb, on=1, M=M, prec=0, cov_kind=LANE, pow_kind=LANE):
    rows = C.c_int(-1)
    assert lib.oiva_test_cov_rows(T, F, M, prec, cov_kind, ctc, pow_kind, tcp, float(budget_mb), on, C.byref(rows)) == 0
    return rows.value


def _nt(lib, T, ctc, tcp, budget_mb, M=M, prec=0, cov_kind=LANE, pow_kind=LANE):
    out = (C.c_int * 3)()
    assert lib.oiva_test_x_choice(T, F, M, prec, cov_kind, ctc, pow_kind, tcp, float(budget_mb), 0, out, None) == 0
    return bool(out[1]), REASONS[out[2]]


@pytest.mark.parametrize("T,ctc,tcp", GEOMS)
def test_row_form_exactly_where_the_policy_streams(lib, T, ctc, tcp):
    for share in (0.03, 0.3, 0.5, 0.97):
        assert _nt(lib, T, ctc, tcp, share * _x_mb(T)) == (True, "share")
        assert _rows(lib, T, ctc, tcp, share * _x_mb(T)) == 1
        assert _rows(lib, T, ctc, tcp, share * _x_mb(T), on=0) == 0      # the switch
    for budget, why in ((0., "off"), (-1., "off"), (_x_mb(T), "fits"), (1e6, "fits")):
        assert _nt(lib, T, ctc, tcp, budget) == (False, why)
        assert _rows(lib, T, ctc, tcp, budget) == 0


@pytest.mark.parametrize("T,ctc,tcp,M_,prec,kinds,why", [
    (4000, 1000, 336, 8, 0, (LANE, LANE), "geometry"),     # splits that do not start on a group
    (4000, 144, 336, 8, 0, (LANE, LANE), "geometry"),      # a chunk that crosses more than one split boundary
    (4000, 1008, 336, 4, 0, (LANE, LANE), "kernels"),      # 4 channels keep their one instantiation
    (4000, 1008, 336, 6, 0, (LANE, LANE), "kernels"),
    (4000, 1008, 336, 8, PREC_COV_F64, (LANE, LANE), "kernels"),
    (4000, 1008, 336, 8, 0, (1, LANE), "kernels"),         # the pair kernel (three and more sources)
    (4000, 1008, 336, 8, 0, (LANE, 1), "kernels"),
])
def test_every_other_plan_keeps_the_lane_form(lib, T, ctc, tcp, M_, prec, kinds, why):
    budget = 0.3 * _x_mb(T, M=M_)
    assert _nt(lib, T, ctc, tcp, budget, M=M_, prec=prec, cov_kind=kinds[0], pow_kind=kinds[1]) == (False, why)
    assert _rows(lib, T, ctc, tcp, budget, M=M_, prec=prec, cov_kind=kinds[0], pow_kind=kinds[1]) == 0


def test_bad_arguments_are_refused(lib):
    rows = C.c_int()
    assert lib.oiva_test_cov_rows(0, F, M, 0, LANE, 16, LANE, 4, 1., 1, C.byref(rows)) != 0
    assert lib.oiva_test_cov_rows(16, F, M, 0, 99, 16, LANE, 4, 1., 1, C.byref(rows)) != 0
    assert lib.oiva_test_cov_rows(16, F, M, 0, LANE, 16, LANE, 4, 1., 1, None) != 0


def _remarks():
    """{kernel name: {field: value}} of kernels_cov.hip, from the remarks of the last build"""
    from overiva_amd import build

    path = os.path.join(build.OBJ, "kernels_cov.usage.txt")
    if not os.path.exists(path):
        build.build_library(force=True)          # objects came from a build without remarks
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_row_instantiations_hold_two_workgroups_per_cu(lib):
    """cov_blocks_per_cu answers for the lane form and the geometry is chosen on that answer (2: tests/golden/
    kernel_choice_256cu.json): the row form must hold the same two workgroups of four waves -- two waves per SIMD: at most 256
    registers, no scratch -- and two rings in a CU's 160 KB of LDS.  Its ring is 32 KB per stage pair, never more than the lane
    form's four stages."""
    usage = _remarks()
    rows = {n: u for n, u in usage.items() if re.search(r"cov_dma_kernelILi8ELi[12]ELb1ELi\d+E", n)}
    lane = {n: u for n, u in usage.items() if re.search(r"cov_dma_kernelILi8ELi[12]ELb0ELi4E", n)}
    assert len(rows) == 2 and len(lane) == 2, sorted(usage)
    for name, u in list(rows.items()) + list(lane.items()):
        assert u["VGPRs"] <= 256 and u["AGPRs"] == 0, (name, u)
        assert u["ScratchSize"] == 0, (name, u)
        assert u["Occupancy"] >= 2, (name, u)
        assert 2 * u["LDS Size"] <= 160 * 1024, (name, u)
    stages = {int(re.search(r"ELb1ELi(\d+)E", n).group(1)) for n in rows}
    assert len(stages) == 1 and 2 <= stages.pop() <= 4
    for name, u in rows.items():
        assert u["LDS Size"] % (16 * 1024) == 0 and 32 * 1024 <= u["LDS Size"] <= 64 * 1024, (name, u)
