"""Few-groups GROUP BY over aggregates of expressions (k_groupby_lds_prog) on the device: the cases of
tests/grouped_agg_prog_cases.py — what tests/test_grouped_agg_programs.py runs through the host simulations — through the
C-ABI against the oracle, with the route, the kernel name and the variant (6: one window, 7: several) asserted; one case of
2 000 003 rows (every workgroup takes several tiles) — taken with kernel_variant 2, left to the projection pass at the
default variant, where the class rule of the route holds it back —; and the route against the two-pass route behind
MI355Q_OPT_NO_GROUPED_AGG_PROGRAMS.  Every case runs twice: the LDS atomics make the order of the updates differ from run
to run."""
from __future__ import annotations

import numpy as np
import pytest

from heavydb_amd import capi
from tests import grouped_agg_prog_cases as gp

pytestmark = pytest.mark.gpu

TAKEN = gp.taken_cases()
ERRORS = gp.error_cases()
NOT_TAKEN = [c for c in gp.not_taken_cases() if c.name in ("division",)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    capi.load_library()
    return torch


def _run(torch, oracle, case, flags=None):
    from heavydb_amd.executor import Executor, FetchResult
    from tests.helpers import compare_buffers, compare_rows, qmd_equal
    q, want, code = gp.reference(oracle, case)
    variant, case_flags = gp.options(case)
    flags = case_flags if flags is None else flags
    frags = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cols] for cols in case.frags]
    fr = FetchResult([[int(t.data_ptr()) for t in cols] for cols in frags], [len(cols[0]) for cols in case.frags], keepalive=[frags])
    ex = Executor(0)
    rs = None
    for _ in range(2):
        if case.expect_error is not None:
            assert code == case.expect_error
            with pytest.raises(capi.Mi355qError) as ei:
                ex.executeWorkUnit(case.ra, fr, allow_retry=False, kernel_variant=variant, flags=flags)
            assert ei.value.code == case.expect_error
            continue
        assert code == 0
        rs = ex.executeWorkUnit(case.ra, fr, allow_retry=False, kernel_variant=variant, flags=flags)
        qmd_equal(q, rs.getQueryMemDesc())
        compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
        compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), case.fp_rtol)
    return rs


def _route(case, flags=None):
    from heavydb_amd.executor import Executor
    variant, case_flags = gp.options(case)
    return Executor(0).explain(case.ra, [len(cols[0]) for cols in case.frags], kernel_variant=variant,
                               flags=case_flags if flags is None else flags)


def _assert_taken(case, rs):
    route = _route(case)
    assert gp.KERNEL in route and gp.ROUTE in route and "k_project" not in route, route
    if rs is not None:
        assert rs.report.kernel_name == gp.KERNEL.encode(), rs.report.kernel_name
        assert rs.report.variant == gp.VARIANT.get(case.name, rs.report.variant) and rs.report.variant in (6, 7)
        assert rs.report.n_launches == 1


@pytest.mark.parametrize("case", TAKEN, ids=[c.name for c in TAKEN])
def test_taken_cases_on_the_device(torch_cuda, oracle, case):
    _assert_taken(case, _run(torch_cuda, oracle, case))


def test_two_million_rows_on_the_device(torch_cuda, oracle):
    case = gp.large_case()
    assert gp.options(case) == (2, 0)
    _assert_taken(case, _run(torch_cuda, oracle, case))


def test_two_million_rows_at_the_default_variant_keep_the_projection_pass(torch_cuda, oracle):
    """past the size threshold, but no class of arguments beat the two-pass route when measured: the route is not a default"""
    case = gp.large_case(variant=0)
    assert gp.options(case) == (0, 0)
    rs = _run(torch_cuda, oracle, case)
    route = _route(case)
    assert gp.KERNEL not in route and "k_project" in route, route
    assert rs.report.kernel_name != gp.KERNEL.encode()


@pytest.mark.parametrize("case", ERRORS, ids=[c.name for c in ERRORS])
def test_errors_on_the_device(torch_cuda, oracle, case):
    _assert_taken(case, _run(torch_cuda, oracle, case))


def test_a_key_outside_its_range_is_out_of_slots_on_both_routes(torch_cuda, oracle):
    case = next(c for c in ERRORS if c.name == "key_outside_its_declared_range")
    _run(torch_cuda, oracle, case, flags=capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    assert gp.KERNEL not in _route(case, capi.OPT_NO_GROUPED_AGG_PROGRAMS)


@pytest.mark.parametrize("case", NOT_TAKEN, ids=[c.name for c in NOT_TAKEN])
def test_not_taken_cases_on_the_device(torch_cuda, oracle, case):
    rs = _run(torch_cuda, oracle, case)
    route = _route(case)
    assert gp.KERNEL not in route and "k_project" in route, route
    assert rs.report.kernel_name != gp.KERNEL.encode()


@pytest.mark.parametrize("name", ["i32_product_all_kinds", "two_keys_three_arguments", "double_program"])
def test_both_routes_agree_on_the_device(torch_cuda, oracle, name):
    """group by group: integer slots bit for bit, DOUBLE sums within the project's 1e-9"""
    case = next(c for c in TAKEN if c.name == name)
    new = _run(torch_cuda, oracle, case)
    old = _run(torch_cuda, oracle, case, flags=capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    _assert_taken(case, new)
    route = _route(case, capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    assert "k_project" in route and gp.KERNEL not in route, route
    assert old.report.kernel_name != gp.KERNEL.encode()
    gp.slots_agree(new, old)
