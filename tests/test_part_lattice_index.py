"""The lattice member's exact-division index in the host simulation: the real kernels_part.hip compiled for the CPU behind
the real api.cpp / plan.cpp, every case of tests/part_lattice_index_cases.py at 250 K rows three ways — packed records (the
default), MI355Q_OPT_NO_LATTICE_PACK (the 16-byte records) and the oracle — both library runs against the oracle and
against each other; the TRACE lines say whether the member ran or gave up."""
import ctypes as C

import pytest

from heavydb_amd import capi
from tests import part_lattice_cases as plc
from tests import part_lattice_index_cases as pic
from tests import test_hostsim_flow as flow
from tests.helpers import check_probe_invariant, compare_rows, hostsim_lib
from tests.test_part_lattice import check_trace
from tests.test_part_lattice_pack import check_record_format

CASES = pic.build_cases(plc.SIM_ROWS)


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


@pytest.mark.parametrize("lc", CASES, ids=[c.name for c in CASES])
def test_exact_division_index_against_the_oracle_packed_and_unpacked(sim, oracle, capfd, lc):
    capfd.readouterr()
    rs = flow._check(oracle, lc.case, flags=capi.OPT_TRACE, **lc.opts)
    err = capfd.readouterr().err
    check_trace(lc, err)
    check_record_format(lc, err, True)
    assert rs.report.kernel_name.decode() == "k_part_scatter" and rs.report.variant == 2, (rs.report.kernel_name, rs.report.variant)
    assert rs.report.rows_scanned == plc.SIM_ROWS
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
