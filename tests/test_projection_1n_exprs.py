"""Projection steps with expressions through a ONE-TO-MANY join on the CPU: the real kernels_proj.hip (k_proj_join_1n's
expression-carrying member) compiled for the host (tests/hostsim) against the oracle's restatement of the reference's join
loop around the row function's body.  The same cases run on the device in tests/test_zz_gpu_projection_1n_exprs.py."""
import pytest

from heavydb_amd import capi
from tests import proj_1n_expr_cases
from tests.test_projection import check_projection, host_fetch_result, sim  # noqa: F401  (sim: the fixture)

CASES = proj_1n_expr_cases.build_cases()
ROUTE_NOTE = "k_proj_compact (one-to-many join, expressions in registers)"
# report.variant of the one-to-many member with expressions: the evaluator's stack and values in LDS / row at a time, private stack
IN_LDS, ROW_AT_A_TIME = 32, 33
# the row-at-a-time evaluator: both layouts, an expression in a qual, a LIMIT inside a run, every error rule, the deepest programs
ROW_AT_A_TIME_CASES = [c for c in CASES if c.name in (
    "x1n_targets_inner_perfect", "x1n_targets_left_keyed_filtered_columnar", "x1n_expr_qual_left_nullable_int32_key",
    "x1n_scan_limit_inside_a_run", "x1n_div_by_zero_in_unmatched_rows_inner", "x1n_div_by_zero_in_unmatched_rows_left",
    "x1n_div_by_zero_in_a_matched_row", "x1n_div_by_zero_past_the_limit", "x1n_div_by_zero_dropped_by_a_qual",
    "x1n_overflow_in_an_emitted_row", proj_1n_expr_cases.SEVEN_DEEP)]
assert len(ROW_AT_A_TIME_CASES) == 11


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_projection_1n_with_expressions_on_the_host_simulation(sim, oracle, case):
    """key sequence entry by entry, the rows of every run of equal keys as a multiset, the error code (check_projection)"""
    rs = check_projection(oracle, case, host_fetch_result)
    if rs is not None:
        assert rs.report.kernel_name.decode() == "k_proj_compact" and rs.report.variant == IN_LDS, rs.report.variant
        assert rs.rowCount() >= (50 if case.ra.scan_limit else 10_000)


@pytest.mark.parametrize("case", ROW_AT_A_TIME_CASES, ids=[c.name for c in ROW_AT_A_TIME_CASES])
def test_projection_1n_with_expressions_row_at_a_time_on_the_host_simulation(sim, oracle, case):
    """The member's other evaluator: eval_exprs with its private stack, which it takes when the LDS area has no room.

    The launch sizes the area as MAX_EXPRS x MAX_EXPR_NODES x sizeof(XNode) + (deepest - 1 + n) x 4 x 256 x 8 bytes
    = 3 072 + (deepest - 1 + n) x 8 192 and keeps the LDS form up to 156 KB = 159 744 bytes: room for 19 levels.  Seven
    expressions would need a 14-deep stack to go beyond it, and a plan's stack is at most MI355Q_MAX_EXPR_STACK = 8 values
    deep (deeper programs are refused as invalid plans): the widest area a plan can ask of this member — which has no output
    image in LDS — is 3 072 + (7 + 8) x 8 192 = 125 952 bytes.  So no plan reaches the fallback through the sizing; pass_rows = -4
    switches the area off.  Checked through report.variant: 33 ran here, 32 in the test above (the seven-expression case with
    8-deep stacks, 117 760 bytes of LDS, included)."""
    rs = check_projection(oracle, case, host_fetch_result, pass_rows=-4)
    if rs is not None:
        assert rs.report.variant == ROW_AT_A_TIME, rs.report.variant


def test_projection_1n_with_expressions_is_explained(sim):
    from heavydb_amd.executor import Executor
    from tests.test_hostsim_flow import _build_join
    case = next(c for c in CASES if c.name == "x1n_expr_qual_inner_perfect")
    hj, keep = _build_join(case)
    case.ra.join_table = hj
    route = Executor(0).explain(case.ra, [len(f[0]) for f in case.frags])
    assert ROUTE_NOTE in route, route


def test_projection_1n_without_expressions_keeps_its_member_and_note(sim, oracle):
    """the plain one-to-many step: the member without expressions (report.variant 1 / 2, as before), the join's route note"""
    from heavydb_amd.executor import Executor
    from tests import proj_cases
    case = next(c for c in proj_cases.build_join_cases() if c.name == "join_1n_inner_perfect")
    rs = check_projection(oracle, case, host_fetch_result)
    assert rs.report.variant in (1, 2)
    route = Executor(0).explain(case.ra, [len(f[0]) for f in case.frags])
    assert "k_proj_compact (join probe per row)" in route and ROUTE_NOTE not in route, route
