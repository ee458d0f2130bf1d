"""Non-grouped aggregates of expressions in the scan's registers (k_scan_agg_prog) on the device: the cases of
tests/agg_prog_cases.py — what tests/test_agg_programs.py runs through the host simulation — through the C-ABI against the
oracle, with the route and the kernel name asserted, one case of 2 000 003 rows (every workgroup of the grid takes several
tiles) and one comparison of the route with the two-pass route behind MI355Q_OPT_NO_AGG_PROGRAMS."""
from __future__ import annotations

import numpy as np
import pytest

from heavydb_amd import capi
from tests import agg_prog_cases as ap
from tests.helpers import compare_buffers, compare_rows, qmd_equal

pytestmark = pytest.mark.gpu

TAKEN = ap.taken_cases()
ERRORS = [c for c in ap.error_cases() if c.name in ("i32_overflow_in_a_passing_row", "i32_overflow_only_in_dropped_rows",
                                                    "i32_overflow_in_the_last_partial_quads_row", "i64_product_overflow",
                                                    "narrowing_cast_overflow")]
NOT_TAKEN = [c for c in ap.not_taken_cases() if c.name in ("division",)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    capi.load_library()
    return torch


def _run(torch, oracle, case, flags=0):
    from heavydb_amd.executor import Executor, FetchResult
    q, want, code = ap.reference(oracle, case)
    frags = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cols] for cols in case.frags]
    fr = FetchResult([[int(t.data_ptr()) for t in cols] for cols in frags], [len(cols[0]) for cols in case.frags], keepalive=[frags])
    ex = Executor(0)
    if case.expect_error is not None:
        assert code == case.expect_error
        with pytest.raises(capi.Mi355qError) as ei:
            ex.executeWorkUnit(case.ra, fr, allow_retry=False, flags=flags)
        assert ei.value.code == case.expect_error
        return None
    assert code == 0
    rs = ex.executeWorkUnit(case.ra, fr, allow_retry=False, flags=flags)
    qmd_equal(q, rs.getQueryMemDesc())
    compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
    compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
    return rs


def _route(case, flags=0):
    from heavydb_amd.executor import Executor
    return Executor(0).explain(case.ra, [len(cols[0]) for cols in case.frags], flags=flags)


def _assert_taken(case, rs):
    route = _route(case)
    assert ap.KERNEL in route and ap.ROUTE in route and "k_project" not in route, route
    if rs is not None:
        assert rs.report.kernel_name == ap.KERNEL.encode(), rs.report.kernel_name
        assert rs.report.variant == 0 and rs.report.n_launches == 1


@pytest.mark.parametrize("case", TAKEN, ids=[c.name for c in TAKEN])
def test_taken_cases_on_the_device(torch_cuda, oracle, case):
    _assert_taken(case, _run(torch_cuda, oracle, case))


def test_two_million_rows_on_the_device(torch_cuda, oracle):
    case = ap.large_case()
    _assert_taken(case, _run(torch_cuda, oracle, case))


@pytest.mark.parametrize("case", ERRORS, ids=[c.name for c in ERRORS])
def test_errors_on_the_device(torch_cuda, oracle, case):
    _assert_taken(case, _run(torch_cuda, oracle, case))


@pytest.mark.parametrize("case", NOT_TAKEN, ids=[c.name for c in NOT_TAKEN])
def test_not_taken_cases_on_the_device(torch_cuda, oracle, case):
    rs = _run(torch_cuda, oracle, case)
    route = _route(case)
    assert ap.KERNEL not in route and "k_project" in route, route
    assert rs.report.kernel_name != ap.KERNEL.encode()


def test_both_routes_agree_on_the_device(torch_cuda, oracle):
    """integer slots bit for bit, DOUBLE sums within the project's 1e-9"""
    for name in ("i32_product_all_kinds", "double_arith_nullable_operand"):
        case = next(c for c in TAKEN if c.name == name)
        new = _run(torch_cuda, oracle, case)
        old = _run(torch_cuda, oracle, case, flags=capi.OPT_NO_AGG_PROGRAMS)
        _assert_taken(case, new)
        route = _route(case, capi.OPT_NO_AGG_PROGRAMS)
        assert "k_project" in route and ap.KERNEL not in route, route
        assert old.report.kernel_name != ap.KERNEL.encode()
        q = new.getQueryMemDesc()
        a, b = np.asarray(new.getStorage()).reshape(-1), np.asarray(old.getStorage()).reshape(-1)
        for t in range(q.n_targets):
            s = q.target_slot[t]
            if q.target_arg_is_fp[t]:
                x, y = a[s:s + 1].view(np.float64)[0], b[s:s + 1].view(np.float64)[0]
                assert abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (t, x, y)
                if q.target_agg[t] == capi.AVG:
                    assert a[s + 1] == b[s + 1]
            else:
                n = 2 if q.target_agg[t] == capi.AVG else 1
                assert (a[s:s + n] == b[s:s + n]).all(), (t, a[s:s + n], b[s:s + n])
