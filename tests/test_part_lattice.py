"""The partitioned GROUP BY's lattice member in the host simulation: the real kernels_part.hip compiled for the CPU
(tests/helpers.py hostsim_lib(real_fast=True), as tests/test_hostsim_real_kernels.py runs the rest of the family) behind the
real api.cpp / plan.cpp, every case of tests/part_lattice_cases.py against the oracle, with the member and with
MI355Q_OPT_NO_LATTICE_PART, and the two against each other."""
import ctypes as C

import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import test_hostsim_flow as flow
from tests.helpers import check_probe_invariant, compare_rows, hostsim_lib

SIM_PARTITIONS = 16   # P of a 40 K-entry table on the simulation's 8 "CUs"
CASES = plc.build_cases(SIM_PARTITIONS, plc.SIM_ROWS)


@pytest.fixture(scope="module")
def sim():
    lib = capi.load_library(hostsim_lib(real_fast=True))
    lib.hostsim_configure.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32]
    lib.hostsim_configure.restype = None
    saved = capi._lib
    capi._lib = lib
    lib.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    yield lib
    capi._lib = saved


def check_trace(lc, err):
    """the stderr marks of a MI355Q_OPT_TRACE step name the phase-2 member that ran"""
    if lc.member == "idx":
        assert plc.TRACE_IDX in err and plc.TRACE_GAVE_UP not in err, err
    elif lc.member == "gave_up":
        assert plc.TRACE_IDX in err and plc.TRACE_GAVE_UP in err, err
    elif lc.member == "plain":
        assert plc.TRACE_PLAIN in err and plc.TRACE_IDX not in err and plc.TRACE_GAVE_UP not in err, err


def units_in_trace(err):
    """P of the lattice member's TRACE line: `... lattice points, P units of E entries)`"""
    return int(err.split(plc.TRACE_IDX, 1)[1].split(" units of ", 1)[0].rsplit(" ", 1)[1])


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_lattice_member_against_the_oracle_and_the_plain_member(sim, oracle, capfd, lc):
    capfd.readouterr()
    rs = flow._check(oracle, lc.case, flags=capi.OPT_TRACE, **lc.opts)
    err = capfd.readouterr().err
    check_trace(lc, err)
    if lc.member is not None:
        assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
        assert rs.report.n_launches >= lc.min_launches, rs.report.n_launches
        assert rs.report.rows_scanned == plc.SIM_ROWS
    if lc.name == "few_points_per_unit":
        assert units_in_trace(err) == SIM_PARTITIONS, err
    if lc.max_groups is not None:
        assert rs.rowCount() < lc.max_groups, rs.rowCount()
    check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
    plain = flow._check(oracle, lc.case, flags=capi.OPT_TRACE | capi.OPT_NO_LATTICE_PART, **lc.opts)
    err = capfd.readouterr().err
    assert plc.TRACE_IDX not in err and plc.TRACE_GAVE_UP not in err, err
    check_probe_invariant(plain.getQueryMemDesc(), plain.getStorage())
    assert plain.report.kernel_name == rs.report.kernel_name and plain.report.variant == rs.report.variant
    compare_rows(rs.getQueryMemDesc(), plain.fetch(), rs.fetch(), lc.case.fp_rtol)
