"""Grouped steps over a ONE-TO-MANY join on the device (k_join_expand_count / _scan / _write and the step without the join,
through the C-ABI): every case of tests/join_expand_cases.py — what tests/test_join_expand.py runs through the host simulation —
against the oracle at the parity bar (keys, counts, integer sums, MIN / MAX bit for bit; DOUBLE sums / AVG within 1e-9 relative;
baseline tables as key -> slots) and against the same step in the row kernel (OPT_NO_JOIN_EXPAND), with the route, the
launch count and the planner's own choice asserted.  The largest case lays down about 120 000 joined rows."""
from __future__ import annotations

import pytest

from heavydb_amd import capi
from tests import join_expand_cases as jx
from tests.helpers import compare_buffers, compare_rows, qmd_equal
from tests.test_gpu_parity import _build_join, _fetch_result, _oracle_join, _upload, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from tests.test_join_expand import check_report, check_route, check_row_kernel, planned_route, route_of

pytestmark = pytest.mark.gpu
CASES = jx.build_cases()


@pytest.mark.parametrize("ec", CASES, ids=[ec.case.name for ec in CASES])
def test_join_expand_on_the_device(torch_cuda, oracle, ec):
    from heavydb_amd.executor import Executor
    torch, case = torch_cuda, ec.case
    q, want, code = oracle.execute(case.ra.to_plan(), case.frags, case.inner, _oracle_join(oracle, case), n_threads=2)
    assert code == 0
    frag_t, inner_t = _upload(torch, case)
    make_join = lambda c: _build_join(torch, c)  # noqa: E731
    hj, keep = make_join(case)
    case.ra.join_table = hj
    try:
        ex = Executor(0)
        fr = _fetch_result(case, frag_t, inner_t)
        rs = ex.executeWorkUnit(case.ra, fr, allow_retry=False, kernel_variant=2, **ec.opts)
        qmd_equal(q, rs.getQueryMemDesc())
        compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
        assert rs.rowCount() == oracle.row_count(q, want)
        compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
        rs_row = ex.executeWorkUnit(case.ra, fr, allow_retry=False, kernel_variant=2, flags=capi.OPT_NO_JOIN_EXPAND, **ec.opts)
    finally:
        case.ra.join_table = None
    check_report(ec, rs)
    assert rs.rowCount() == 0 if ec.nothing_joins else rs.rowCount() >= 150
    check_route(ec, route_of(ec, make_join=make_join))
    check_row_kernel(ec, rs, rs_row, route_of(ec, capi.OPT_NO_JOIN_EXPAND, make_join=make_join))


def test_the_planner_takes_the_route_for_a_large_input_and_a_table_beyond_lds_on_the_device(torch_cuda):
    make_join = lambda c: _build_join(torch_cuda, c)  # noqa: E731
    assert planned_route(20_000, make_join=make_join).startswith(jx.ROUTE_NOTE)
    assert not planned_route(30, make_join=make_join).startswith(jx.ROUTE_NOTE)
    assert jx.ROUTE_NOTE not in planned_route(20_000, capi.OPT_NO_JOIN_EXPAND, make_join=make_join)
