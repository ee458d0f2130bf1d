"""Grouped steps over a ONE-TO-MANY join on the CPU: the real k_join_expand_count / _scan / _write of kernels_proj.hip compiled for
the host (tests/hostsim) under the host code of api_routes.cpp execute_join_expand, against the oracle's restatement of the
reference's join loop around the row function's body — and against the same step in the row kernel (OPT_NO_JOIN_EXPAND).  The
same cases run on the device in tests/test_zz_gpu_join_expand.py."""
import copy

import pytest

from heavydb_amd import capi
from heavydb_amd.executor import ExpressionRange, Executor
from tests import cases as cases_mod
from tests import join_expand_cases as jx
from tests import test_hostsim_flow as flow
from tests.helpers import compare_buffers
from tests.test_hostsim_flow import sim  # noqa: F401  (the fixture)

CASES = jx.build_cases()
IDS = [ec.case.name for ec in CASES]


def route_of(ec, flags=0, make_join=flow._build_join):
    hj, keep = make_join(ec.case)
    ec.case.ra.join_table = hj
    try:
        return Executor(0).explain(ec.case.ra, [len(f[0]) for f in ec.case.frags], kernel_variant=2, flags=flags)
    finally:
        ec.case.ra.join_table = None


def check_route(ec, route):
    if ec.case.ra.exprs:
        assert route.startswith("k_project") and jx.ROUTE_NOTE in route, route
    else:
        assert route.startswith(jx.ROUTE_NOTE), route


def check_report(ec, rs):
    """count + scan, and per pass the write kernel and at least one launch of the derived step (whose kernel the report
    names: a fast family's, or the row kernel's over the dense columns where the plan is the row kernel's)"""
    assert rs.report.n_launches >= 2 + 2 * ec.passes, rs.report.n_launches


def check_row_kernel(ec, rs, rs_row, route_row):
    """the same step with OPT_NO_JOIN_EXPAND: the row kernel's result at the parity bar"""
    q = rs.getQueryMemDesc()
    compare_buffers(q, rs_row.getStorage(), rs.getStorage(), ec.case.fp_rtol)
    assert rs_row.rowCount() == rs.rowCount()
    assert jx.ROUTE_NOTE not in route_row, route_row
    assert rs_row.report.kernel_name.decode() == "k_generic", rs_row.report.kernel_name


@pytest.mark.parametrize("ec", CASES, ids=IDS)
def test_join_expand_on_the_host_simulation(sim, oracle, ec):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    rs = flow._check(oracle, ec.case, kernel_variant=2, **ec.opts)   # the oracle: keys, counts, integer sums, MIN / MAX exact; fp 1e-9
    check_route(ec, route_of(ec))
    check_report(ec, rs)
    if ec.nothing_joins:
        assert rs.rowCount() == 0
    else:
        assert rs.rowCount() >= 150
    hj, keep = flow._build_join(ec.case)
    ec.case.ra.join_table = hj
    try:
        rs_row = Executor(0).executeWorkUnit(ec.case.ra, flow._fetch_result(ec.case), allow_retry=False, kernel_variant=2,
                                             flags=capi.OPT_NO_JOIN_EXPAND, **ec.opts)
    finally:
        ec.case.ra.join_table = None
    check_row_kernel(ec, rs, rs_row, route_of(ec, capi.OPT_NO_JOIN_EXPAND))


def test_joined_rows_of_the_cases_are_what_the_docstring_says():
    """the shapes the kernels are aimed at: a hot key beyond a workgroup's lanes, fragments at the tile edges, three passes"""
    for ec in CASES:
        rows2 = jx.joined_rows_per_fragment(ec)
        if ec.nothing_joins:
            assert sum(rows2) == 0
            continue
        assert sum(rows2) > jx.N_ROWS and max(rows2) < 2**31
        assert jx.passes_of(rows2, ec.opts.get("pass_rows", 0) or sum(rows2)) == ec.passes, (ec.case.name, rows2)


def planned_route(groups, flags=0, make_join=flow._build_join):
    """the planner's own choice, no launch: cases.py's join_1n_perfect_groupby_int32_key over 1 B outer rows"""
    case = next(c for c in cases_mod.build_cases() if c.name == "join_1n_perfect_groupby_int32_key")
    ra = copy.deepcopy(case.ra)
    ra.input_col_descs[3].range = ExpressionRange(True, 0, groups - 1)
    hj, keep = make_join(case)
    ra.join_table = hj
    try:
        return Executor(0).explain(ra, [250_000_000] * 4, flags=flags)
    finally:
        ra.join_table = None


def test_the_planner_takes_the_route_for_a_large_input_and_a_table_beyond_lds(sim):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    assert planned_route(20_000).startswith(jx.ROUTE_NOTE)
    assert not planned_route(30).startswith(jx.ROUTE_NOTE)            # (a table of <= 64 KB: the row kernel's LDS copy)
    assert jx.ROUTE_NOTE not in planned_route(20_000, capi.OPT_NO_JOIN_EXPAND)
