"""Projection steps with expressions through a ONE-TO-MANY join on the device (k_proj_join_1n's expression-carrying member
through the C-ABI): every case of tests/proj_1n_expr_cases.py against the oracle — the key sequence entry by entry, the rows
of every run of equal keys as a multiset, the error code — and, for the cases without error or limit, against SQLite's
JOIN / LEFT JOIN over the same tables (tests/test_sqlite_semantics._sql_for states the expressions as columns of a view)."""
from __future__ import annotations

import pytest

from tests import proj_1n_expr_cases
from tests.test_projection import check_projection
from tests.test_projection_1n_exprs import IN_LDS, ROUTE_NOTE, ROW_AT_A_TIME, ROW_AT_A_TIME_CASES
from tests.test_zz_gpu_projection import device_fetch_result, torch_cuda  # noqa: F401  (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
CASES = proj_1n_expr_cases.build_cases()
_PLAIN = [c for c in CASES if c.expect_error is None and not c.ra.scan_limit]


def _check(torch, oracle, case, **opts):
    from tests.test_gpu_parity import _build_join
    return check_projection(oracle, case, lambda c: device_fetch_result(torch, c), make_join=lambda c: _build_join(torch, c), **opts)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_projection_1n_with_expressions_on_the_device(torch_cuda, oracle, case):
    rs = _check(torch_cuda, oracle, case)
    if rs is not None:
        assert rs.report.kernel_name.decode() == "k_proj_compact" and rs.report.variant == IN_LDS, rs.report.variant
        assert rs.rowCount() >= (50 if case.ra.scan_limit else 10_000)


@pytest.mark.parametrize("case", ROW_AT_A_TIME_CASES, ids=[c.name for c in ROW_AT_A_TIME_CASES])
def test_projection_1n_with_expressions_row_at_a_time_on_the_device(torch_cuda, oracle, case):
    """the member's row-at-a-time evaluator (private stack), forced with pass_rows = -4: no plan's programs are deep enough to
    push this member's LDS area beyond the cap (the arithmetic: tests/test_projection_1n_exprs.py).  report.variant 33 ran."""
    rs = _check(torch_cuda, oracle, case, pass_rows=-4)
    if rs is not None:
        assert rs.report.variant == ROW_AT_A_TIME, rs.report.variant


@pytest.mark.parametrize("case", _PLAIN, ids=[c.name for c in _PLAIN])
def test_projection_1n_with_expressions_on_the_device_agrees_with_sqlite(torch_cuda, case):
    """the DEVICE's rows against SQLite's: a pin of the joined rows and of the expressions' values that owes nothing to the oracle"""
    from heavydb_amd.executor import Executor
    from tests.test_gpu_parity import _build_join
    from tests.test_sqlite_semantics import _key, projection_rows_sqlite, rows_agree
    hj, keep = _build_join(torch_cuda, case)
    case.ra.join_table = hj
    try:
        rs = Executor(0).executeWorkUnit(case.ra, device_fetch_result(torch_cuda, case), allow_retry=False)
    finally:
        case.ra.join_table = None
    q = rs.getQueryMemDesc()
    iv, dv, nu = rs.fetch()
    fp = [bool(q.target_is_fp[t]) for t in range(q.n_targets)]
    cols = [[None if n_ else float(d) if fp[t] else int(i) for i, d, n_ in zip(iv[:, t].tolist(), dv[:, t].tolist(), nu[:, t].tolist())]
            for t in range(q.n_targets)]
    got = sorted(zip(*cols), key=_key)
    want = sorted((tuple(float(v) if f and v is not None else v for v, f in zip(r, fp)) for r in projection_rows_sqlite(case)), key=_key)
    rows_agree(case, q, want, got)


def test_projection_1n_with_expressions_is_explained_on_the_device(torch_cuda):
    from heavydb_amd.executor import Executor
    from tests.test_gpu_parity import _build_join
    case = next(c for c in CASES if c.name == "x1n_expr_qual_inner_perfect")
    hj, keep = _build_join(torch_cuda, case)
    case.ra.join_table = hj
    try:
        route = Executor(0).explain(case.ra, [len(f[0]) for f in case.frags])
    finally:
        case.ra.join_table = None
    assert ROUTE_NOTE in route, route
