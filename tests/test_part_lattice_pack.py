"""The lattice member's packed records in the host simulation: the real kernels_part.hip compiled for the CPU behind the
real api.cpp / plan.cpp (as tests/test_part_lattice.py runs the member itself), every case of
tests/part_lattice_pack_cases.py three ways — packed (the default), MI355Q_OPT_NO_LATTICE_PACK (the 16-byte records) and
the oracle — both library runs against the oracle and against each other.  The simulation has 8 "CUs": P = 16, a staged
line of 64 segments = 768 packed records."""
import ctypes as C

import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import part_lattice_pack_cases as ppc
from tests import test_hostsim_flow as flow
from tests.helpers import check_probe_invariant, compare_rows, hostsim_lib
from tests.test_part_lattice import check_trace

SIM_PARTITIONS = 16   # P of a 40 K-entry table on the simulation's 8 "CUs"
CASES = ppc.build_cases(SIM_PARTITIONS, plc.SIM_ROWS)


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


def check_record_format(lc, err, packed):
    """the record format has a TRACE line of its own whenever the lattice member started"""
    if lc.member in ("idx", "gave_up"):
        want, other = (ppc.TRACE_PACKED, ppc.TRACE_UNPACKED) if packed else (ppc.TRACE_UNPACKED, ppc.TRACE_PACKED)
        assert want in err and other not in err, err


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_packed_records_against_the_oracle_and_the_16_byte_records(sim, oracle, capfd, lc):
    capfd.readouterr()
    rs = flow._check(oracle, lc.case, flags=capi.OPT_TRACE, **lc.opts)
    err = capfd.readouterr().err
    check_trace(lc, err)
    check_record_format(lc, err, True)
    assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
    assert rs.report.n_launches >= lc.min_launches, rs.report.n_launches
    assert rs.report.rows_scanned == plc.SIM_ROWS
    if lc.max_groups is not None:
        assert rs.rowCount() < lc.max_groups, rs.rowCount()
    check_probe_invariant(rs.getQueryMemDesc(), rs.getStorage())
    wide = flow._check(oracle, lc.case, flags=capi.OPT_TRACE | capi.OPT_NO_LATTICE_PACK, **lc.opts)
    err = capfd.readouterr().err
    check_trace(lc, err)
    check_record_format(lc, err, False)
    check_probe_invariant(wide.getQueryMemDesc(), wide.getStorage())
    assert wide.report.kernel_name == rs.report.kernel_name and wide.report.variant == rs.report.variant
    assert wide.report.n_launches == rs.report.n_launches and wide.report.rows_scanned == rs.report.rows_scanned
    assert wide.rowCount() == rs.rowCount()
    compare_rows(rs.getQueryMemDesc(), wide.fetch(), rs.fetch(), lc.case.fp_rtol)
