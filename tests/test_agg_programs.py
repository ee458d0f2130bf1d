"""Non-grouped aggregates of expressions in the scan's registers (route `aggregate arguments as register programs`, kernel
k_scan_agg_prog) on the CPU: api_routes.cpp / regprog.h / the real kernels_filter.hip compiled for the host (tests/hostsim,
both simulations) against the oracle.  The same cases run on the device in tests/test_zz_gpu_agg_programs.py."""
import ctypes as C

import numpy as np
import pytest

from heavydb_amd import capi
from tests import agg_prog_cases as ap
from tests.helpers import compare_buffers, compare_rows, hostsim_lib, qmd_equal

TAKEN = ap.taken_cases()
ERRORS = ap.error_cases()
NOT_TAKEN = ap.not_taken_cases()


@pytest.fixture(scope="module", params=[False, True], ids=["hostsim", "hostsim_real"])
def sim(request):
    lib = capi.load_library(hostsim_lib(request.param))
    lib.hostsim_live_allocations.restype = C.c_int
    saved = capi._lib
    capi._lib = lib
    yield lib
    capi._lib = saved


def _executor():
    from heavydb_amd.executor import Executor
    return Executor(0)


def _frag_rows(case):
    return [len(cols[0]) for cols in case.frags]


def run_case(oracle, case, fetch_result, flags=0):
    """the step against the oracle; returns the ResultSet (None where the case expects an error, which is then checked)"""
    q, want, code = ap.reference(oracle, case)
    ex = _executor()
    if case.expect_error is not None:
        assert code == case.expect_error
        with pytest.raises(capi.Mi355qError) as ei:
            ex.executeWorkUnit(case.ra, fetch_result, allow_retry=False, flags=flags)
        assert ei.value.code == case.expect_error
        return None
    assert code == 0
    rs = ex.executeWorkUnit(case.ra, fetch_result, allow_retry=False, flags=flags)
    qmd_equal(q, rs.getQueryMemDesc())
    compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
    compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
    return rs


def assert_taken(case, rs=None):
    route = _executor().explain(case.ra, _frag_rows(case))
    assert ap.KERNEL in route and ap.ROUTE in route and "k_project" not in route, route
    if rs is not None:
        assert rs.report.kernel_name == ap.KERNEL.encode(), rs.report.kernel_name
        assert rs.report.variant == 0 and rs.report.n_launches == 1
        assert rs.report.rows_scanned == sum(_frag_rows(case))


def assert_not_taken(case, rs=None):
    route = _executor().explain(case.ra, _frag_rows(case))
    assert ap.KERNEL not in route and "k_project" in route, route
    if rs is not None:
        assert rs.report.kernel_name != ap.KERNEL.encode()


@pytest.mark.parametrize("case", TAKEN, ids=[c.name for c in TAKEN])
def test_taken_cases_match_the_oracle(sim, oracle, case):
    rs = run_case(oracle, case, ap.host_fetch_result(case))
    assert_taken(case, rs)
    # rows x the widths of the distinct physical columns the plan reads
    plan = case.ra.to_plan()
    used = set()
    for e in case.ra.exprs:
        used |= {n.arg for n in e.nodes if n.op == capi.EX_COL}
    used |= {q.col for q in case.ra.simple_quals} | {t.col for t in case.ra.target_exprs if 0 <= t.col < plan.n_cols}
    width = {capi.INT8: 1, capi.INT16: 2, capi.INT32: 4, capi.INT64: 8, capi.DOUBLE: 8, capi.FLOAT: 4}
    assert rs.report.algorithmic_bytes == sum(_frag_rows(case)) * sum(width[case.ra.input_col_descs[c].type] for c in used)


@pytest.mark.parametrize("case", ERRORS, ids=[c.name for c in ERRORS])
def test_errors_count_only_for_rows_that_pass(sim, oracle, case):
    rs = run_case(oracle, case, ap.host_fetch_result(case))
    assert_taken(case, rs)


@pytest.mark.parametrize("case", NOT_TAKEN, ids=[c.name for c in NOT_TAKEN])
def test_not_taken_cases_keep_the_projection_pass(sim, oracle, case):
    rs = run_case(oracle, case, ap.host_fetch_result(case))
    assert_not_taken(case, rs)


def test_a_misaligned_chunk_keeps_the_projection_pass(sim, oracle):
    """mi355q_explain assumes aligned chunks (it is given none), so the route shows in the step's report"""
    case = TAKEN[0]
    rs = run_case(oracle, case, ap.host_fetch_result(case, misalign_col=ap.B))
    assert rs.report.kernel_name != ap.KERNEL.encode(), rs.report.kernel_name


@pytest.mark.parametrize("name", ["expr_double_arith_nongrouped", "expr_overflow_is_an_error", "expr_overflow_only_in_filtered_rows"])
def test_the_matrix_cases_take_the_route(sim, oracle, name):
    from tests.cases import build_cases
    case = next(c for c in build_cases() if c.name == name)
    case.name = "matrix_" + name
    rs = run_case(oracle, case, ap.host_fetch_result(case))
    assert_taken(case, rs)


@pytest.mark.parametrize("name", ["i32_product_all_kinds", "i64_difference", "double_arith_nullable_operand", "four_arguments_four_columns"])
def test_both_routes_agree(sim, oracle, name):
    case = next(c for c in TAKEN if c.name == name)
    new = run_case(oracle, case, ap.host_fetch_result(case))
    old = run_case(oracle, case, ap.host_fetch_result(case), flags=capi.OPT_NO_AGG_PROGRAMS)
    assert_taken(case, new)
    route = _executor().explain(case.ra, _frag_rows(case), flags=capi.OPT_NO_AGG_PROGRAMS)
    assert "k_project" in route and ap.KERNEL not in route, route
    assert old.report.kernel_name != ap.KERNEL.encode()
    q = new.getQueryMemDesc()
    a, b = np.asarray(new.getStorage()).reshape(-1), np.asarray(old.getStorage()).reshape(-1)
    for t in range(q.n_targets):
        s = q.target_slot[t]
        if q.target_arg_is_fp[t]:   # DOUBLE SUM / MIN / MAX / AVG's sum: the project's 1e-9 bar (its count slot is exact)
            x, y = a[s:s + 1].view(np.float64)[0], b[s:s + 1].view(np.float64)[0]
            assert abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (t, x, y)
            if q.target_agg[t] == capi.AVG:
                assert a[s + 1] == b[s + 1]
        else:
            n = 2 if q.target_agg[t] == capi.AVG else 1
            assert (a[s:s + n] == b[s:s + n]).all(), (t, a[s:s + n], b[s:s + n])


def test_reserve_then_execute_leaves_nothing_behind(sim, oracle):
    """mi355q_reserve_workspace holds everything the step needs: the step itself allocates its result and nothing else"""
    import gc
    case = TAKEN[0]
    ex = _executor()
    fr = ap.host_fetch_result(case)
    gc.collect()   # (results of earlier tests)
    assert capi._lib.mi355q_release_workspace(0) == 0
    base = sim.hostsim_live_allocations()
    ex.reserveWorkspace(case.ra, fr)
    reserved = sim.hostsim_live_allocations()
    assert reserved > base
    rs = run_case(oracle, case, fr)
    assert_taken(case, rs)
    assert sim.hostsim_live_allocations() == reserved + 1   # the result's buffer
    del rs
    gc.collect()
    assert sim.hostsim_live_allocations() == reserved
