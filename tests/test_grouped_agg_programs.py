"""Few-groups GROUP BY over aggregates of expressions, evaluated beside the LDS table (route `grouped aggregate arguments
as register programs`, kernel k_groupby_lds_prog) on the CPU: api_routes.cpp / regprog.h / lds_args.h against the oracle on
both host simulations — the real kernels_lds.hip compiled for the host (512 cooperative fibers per workgroup), and the
stand-in that runs the lowered plan's row function over the arguments' values.  The same cases run on the device in
tests/test_zz_gpu_grouped_agg_programs.py."""
import ctypes as C

import numpy as np
import pytest

from heavydb_amd import capi
from tests import grouped_agg_prog_cases as gp
from tests.helpers import compare_buffers, compare_rows, hostsim_lib, qmd_equal

TAKEN = gp.taken_cases()
ERRORS = gp.error_cases()
NOT_TAKEN = gp.not_taken_cases()


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


def run_case(oracle, case, fetch_result, flags=None):
    """the step against the oracle; returns the ResultSet (None where the case expects an error, which is then checked)"""
    q, want, code = gp.reference(oracle, case)
    variant, case_flags = gp.options(case)
    flags = case_flags if flags is None else flags
    ex = _executor()
    if case.expect_error is not None:
        assert code == case.expect_error
        with pytest.raises(capi.Mi355qError) as ei:
            ex.executeWorkUnit(case.ra, fetch_result, allow_retry=False, kernel_variant=variant, flags=flags)
        assert ei.value.code == case.expect_error
        return None
    assert code == 0
    rs = ex.executeWorkUnit(case.ra, fetch_result, allow_retry=False, kernel_variant=variant, flags=flags)
    qmd_equal(q, rs.getQueryMemDesc())
    compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
    compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
    return rs


def _route(case, flags=None):
    variant, case_flags = gp.options(case)
    return _executor().explain(case.ra, _frag_rows(case), kernel_variant=variant, flags=case_flags if flags is None else flags)


def assert_taken(case, rs=None):
    route = _route(case)
    assert gp.KERNEL in route and gp.ROUTE in route and "k_project" not in route, route
    if rs is not None:
        assert rs.report.kernel_name == gp.KERNEL.encode(), rs.report.kernel_name
        assert rs.report.variant == gp.VARIANT.get(case.name, rs.report.variant) and rs.report.variant in (6, 7)
        assert rs.report.n_launches == 1
        assert rs.report.rows_scanned == sum(_frag_rows(case))


def assert_not_taken(case, rs=None):
    route = _route(case)
    assert gp.KERNEL not in route and "k_project" in route, route
    if rs is not None:
        assert rs.report.kernel_name != gp.KERNEL.encode()


@pytest.mark.parametrize("case", TAKEN, ids=[c.name for c in TAKEN])
def test_taken_cases_match_the_oracle(sim, oracle, case):
    rs = run_case(oracle, case, gp.host_fetch_result(case))
    assert_taken(case, rs)
    # rows x the widths of the distinct physical columns the plan reads
    plan = case.ra.to_plan()
    used = set(case.ra.groupby_exprs)
    for e in case.ra.exprs:
        used |= {n.arg for n in e.nodes if n.op == capi.EX_COL}
    used |= {q.col for q in case.ra.simple_quals} | {t.col for t in case.ra.target_exprs if t.agg != capi.PROJECT_KEY and 0 <= t.col < plan.n_cols}
    width = {capi.INT8: 1, capi.INT16: 2, capi.INT32: 4, capi.INT64: 8, capi.DOUBLE: 8, capi.FLOAT: 4}
    assert rs.report.algorithmic_bytes == sum(_frag_rows(case)) * sum(width[case.ra.input_col_descs[c].type] for c in used)


@pytest.mark.parametrize("case", ERRORS, ids=[c.name for c in ERRORS])
def test_errors_count_only_for_rows_that_pass(sim, oracle, case):
    rs = run_case(oracle, case, gp.host_fetch_result(case))
    assert_taken(case, rs)


def test_a_key_outside_its_range_is_out_of_slots_on_both_routes(sim, oracle):
    case = next(c for c in ERRORS if c.name == "key_outside_its_declared_range")
    assert case.expect_error == capi.ERR_OUT_OF_SLOTS
    run_case(oracle, case, gp.host_fetch_result(case))
    run_case(oracle, case, gp.host_fetch_result(case), flags=capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    assert gp.KERNEL not in _route(case, capi.OPT_NO_GROUPED_AGG_PROGRAMS)


@pytest.mark.parametrize("case", NOT_TAKEN, ids=[c.name for c in NOT_TAKEN])
def test_not_taken_cases_keep_the_projection_pass(sim, oracle, case):
    rs = run_case(oracle, case, gp.host_fetch_result(case))
    assert_not_taken(case, rs)


def test_past_the_size_threshold_the_class_rule_keeps_the_projection_pass(sim):
    """2^20 rows is where the route's size rule would admit a step on its own; no class of arguments beat the two-pass route
    when measured (INT32 11.4 ms against 7.9 ms per 1 B rows, BIGINT 13.5 against 10.0, DOUBLE 12.5 against 11.0), so at the
    default variant every step stays on k_project, and kernel_variant 2 reaches the route"""
    for name in ("i32_product_all_kinds", "cast_bigint_product", "double_program"):
        case = next(c for c in TAKEN if c.name == name)
        route = _executor().explain(case.ra, [2_000_003], kernel_variant=0)
        assert gp.KERNEL not in route and "k_project" in route, route
        route = _executor().explain(case.ra, [2_000_003], kernel_variant=2)
        assert gp.KERNEL in route and "k_project" not in route, route


def test_a_misaligned_operand_chunk_keeps_the_projection_pass(sim, oracle):
    """mi355q_explain assumes aligned chunks (it is given none), so the route shows in the step's report"""
    case = TAKEN[0]
    rs = run_case(oracle, case, gp.host_fetch_result(case, misalign_col=gp.B))
    assert rs.report.kernel_name != gp.KERNEL.encode(), rs.report.kernel_name


@pytest.mark.parametrize("name", ["i32_product_all_kinds", "two_keys_three_arguments", "double_program"])
def test_both_routes_agree(sim, oracle, name):
    case = next(c for c in TAKEN if c.name == name)
    new = run_case(oracle, case, gp.host_fetch_result(case))
    old = run_case(oracle, case, gp.host_fetch_result(case), flags=capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    assert_taken(case, new)
    route = _route(case, capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    assert "k_project" in route and gp.KERNEL not in route, route
    assert old.report.kernel_name != gp.KERNEL.encode()
    gp.slots_agree(new, old)


def test_reserve_then_execute_leaves_nothing_behind(sim, oracle):
    """mi355q_reserve_workspace holds everything the step needs: the step itself allocates its result and nothing else"""
    import gc
    case = TAKEN[0]
    ex = _executor()
    fr = gp.host_fetch_result(case)
    gc.collect()   # (results of earlier tests)
    assert capi._lib.mi355q_release_workspace(0) == 0
    base = sim.hostsim_live_allocations()
    ex.reserveWorkspace(case.ra, fr, kernel_variant=2)
    reserved = sim.hostsim_live_allocations()
    assert reserved > base
    rs = run_case(oracle, case, fr)
    assert_taken(case, rs)
    assert sim.hostsim_live_allocations() == reserved + 1   # the result's buffer
    del rs
    gc.collect()
    assert sim.hostsim_live_allocations() == reserved
