"""Star joins on the CPU: join steps whose quals and group columns name columns of the dimension (capi.INNER_COL), run through the
library's host code on the host simulation (tests/hostsim) — plan.cpp flatten_inner_refs, api_routes.cpp execute_inner_refs, the
real k_join_gather / k_join_expand_* — against the oracle on a flattened plan the test builds itself with numpy and against
SQLite on the query text (tests/star_join_cases.py).  The same cases run on the device in tests/test_zz_gpu_star_join.py."""
import copy
import ctypes as C

import numpy as np
import pytest

from heavydb_amd import capi
from heavydb_amd.executor import Executor, ExpressionRange, FetchResult, Qual, TargetExpr, inner
from tests import star_join_cases as sx
from tests import test_hostsim_flow as flow
from tests.helpers import qmd_equal
from tests.test_hostsim_flow import sim  # noqa: F401  (the fixture)

CASES = sx.build_cases()
RUNS = [(sc, vid, opts, star_runs) for sc in CASES for vid, opts, star_runs in sx.variants(sc)]
RUN_IDS = [f"{sc.name}-{vid}" for sc, vid, _, _ in RUNS]


def _unaligned(a):
    """a copy of the array 4 bytes past a 64-byte boundary"""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 128, np.uint8)
    off = (-raw.ctypes.data) % 64 + 4
    out = raw[off:off + a.nbytes].view(a.dtype)
    out[...] = a
    return out


def fetch_result(sc):
    if not sc.unaligned:
        return flow._fetch_result(sc.case)
    frags = [[_unaligned(a) for a in cols] for cols in sc.case.frags]
    inn = [flow._aligned(a) for a in sc.case.inner]
    return FetchResult([[a.ctypes.data for a in cols] for cols in frags], [len(cols[0]) for cols in frags], [a.ctypes.data for a in inn],
                       len(inn[0]), 0, [frags, inn])


def route_of(sc, opts, make_join=flow._build_join):
    hj, keep = make_join(sc.case)
    sc.case.ra.join_table = hj
    try:
        return Executor(0).explain(sc.case.ra, [len(f[0]) for f in sc.case.frags], inner_rows=len(sc.case.inner[0]), **opts)
    finally:
        sc.case.ra.join_table = None


def run_one(oracle, sc, opts, star_runs, make_join=flow._build_join, make_fetch=fetch_result):
    """one case one way: the descriptor, the result (or the error code) against both references, the report, the route"""
    q, want, code = sx.oracle_reference(oracle, sc)
    hj, keep = make_join(sc.case)
    sc.case.ra.join_table = hj
    try:
        # mi355q_qmd_init of the stated plan = the flattened plan's descriptor
        qmd_equal(q, Executor(0).initQueryMemoryDescriptor(sc.case.ra))
        fr = make_fetch(sc)
        if sc.case.expect_error is not None:
            assert code == sc.case.expect_error
            with pytest.raises(capi.Mi355qError) as ei:
                Executor(0).executeWorkUnit(sc.case.ra, fr, allow_retry=False, **opts)
            assert ei.value.code == sc.case.expect_error, ei.value.code
            return
        rs = Executor(0).executeWorkUnit(sc.case.ra, fr, allow_retry=False, **opts)
    finally:
        sc.case.ra.join_table = None
    sx.check_result(oracle, sc, rs, star_runs)
    if not sc.unaligned:   # (mi355q_explain assumes aligned chunks)
        sx.check_route(sc, route_of(sc, opts, make_join), star_runs)


@pytest.mark.parametrize("sc,vid,opts,star_runs", RUNS, ids=RUN_IDS)
def test_star_join_on_the_host_simulation(sim, oracle, sc, vid, opts, star_runs):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    run_one(oracle, sc, opts, star_runs)


def test_the_cases_cover_what_their_docstring_says(oracle):
    star = [sc for sc in CASES if sc.star and sc.case.expect_error is None]
    qs = [sx.oracle_reference(oracle, sc)[0] for sc in star]
    assert {bool(q.keyless) for q in qs} == {True, False}
    assert all(q.desc_type == capi.GROUP_BY_PERFECT_HASH for q in qs)
    assert min(q.entry_count for q in qs) <= 8 and max(q.entry_count for q in qs) >= 300
    assert {sc.case.ra.join_kind for sc in star} == {capi.JOIN_INNER, capi.JOIN_LEFT}
    assert {len(sc.case.ra.groupby_exprs) for sc in star} == {1, 2, 3}
    assert sum(sc.sql is not None for sc in CASES) >= 6
    base = [sx.oracle_reference(oracle, sc)[0] for sc in CASES if "baseline" in sc.name]
    assert base and all(q.desc_type == capi.GROUP_BY_BASELINE_HASH for q in base)
    # the rows the LEFT ... IS NULL case keeps are exactly the unmatched ones
    sc = next(c for c in CASES if c.name == "star_left_qual_is_null_keeps_unmatched")
    q, want, _ = sx.oracle_reference(oracle, sc)
    iv, dv, nu = oracle.fetch_rows(q, want)
    unmatched = sum(int((hi == lo).sum()) for cols in sc.case.frags for _, lo, hi in [sx._match(sc.case, cols[sx.DID])])
    assert iv.shape[0] == 1 and nu[0, 0] and iv[0, 1] == unmatched and unmatched > 1000


def _plan(ra):
    hj, keep = flow._build_join(CASES[0].case)
    ra.join_table = hj
    return ra.to_plan(), (hj, keep)


def test_refusals_return_their_documented_codes(sim):
    """no launch: mi355q_qmd_init and mi355q_explain answer for the plan alone"""
    lib = capi.load_library()
    base = CASES[0].case.ra

    def code_of(mutate, with_join=True):
        ra = copy.deepcopy(base)
        keep = None
        if with_join:
            p, keep = _plan(ra)
        else:
            ra.join_outer_col = -1
            p = ra.to_plan()
        mutate(p)
        q = capi.QMD()
        rc = lib.mi355q_qmd_init(C.byref(p), C.byref(q))
        ra.join_table = None
        return rc

    def set_(field, i, sub, v):
        def m(p):
            setattr(getattr(p, field)[i], sub, v)
        return m

    assert code_of(lambda p: None) == 0
    # an inner reference where none is accepted
    def cond_ref(p):
        p.targets[1].agg = capi.COUNT_IF
        p.targets[1].cond.col = capi.INNER_COL(sx.D_SEG)
        p.targets[1].cond.op = capi.EQ
    assert code_of(cond_ref) == capi.ERR_INVALID_PLAN
    def key_ref(p):
        p.join_outer_col = capi.INNER_COL(sx.D_REGION)
    assert code_of(key_ref) == capi.ERR_INVALID_PLAN
    def expr_arg_ref(p):      # (no other inner reference in the plan: the expression's own check answers)
        p.n_quals = 0
        p.group_cols[0] = sx.Q
        p.n_exprs = 1
        p.exprs[0].n_nodes = 1
        p.exprs[0].nodes[0].op = capi.EX_COL
        p.exprs[0].nodes[0].arg = capi.INNER_COL(sx.D_SEG)
    assert code_of(expr_arg_ref) == capi.ERR_INVALID_PLAN
    # ... with n_exprs > 0
    def with_expr(p):
        p.n_exprs = 1
        p.exprs[0].n_nodes = 1
        p.exprs[0].nodes[0].op = capi.EX_COL
        p.exprs[0].nodes[0].arg = sx.AMT
    assert code_of(with_expr) == capi.ERR_UNSUPPORTED
    # a Projection step with an inner reference in a qual
    def projection(p):
        p.n_group_cols = 0
        p.n_targets = 1
        p.targets[0].agg = capi.PROJECT
        p.targets[0].col = sx.AMT
    assert code_of(projection) == capi.ERR_UNSUPPORTED
    # without a join; an index >= n_inner_cols; a hostile n_inner_cols
    assert code_of(lambda p: None, with_join=False) == capi.ERR_INVALID_PLAN
    assert code_of(set_("quals", 0, "col", capi.INNER_COL(len(base.inner_col_descs)))) == capi.ERR_INVALID_PLAN
    assert code_of(set_("quals", 0, "col", 2**31 - 1)) == capi.ERR_INVALID_PLAN
    def no_inner_cols(p):
        p.n_inner_cols = 0
    assert code_of(no_inner_cols) == capi.ERR_INVALID_PLAN
    for hostile in (-1, 17, 1 << 20, 2**31 - 1):
        def bad_n(p, v=hostile):
            p.n_inner_cols = v
        assert code_of(bad_n) == capi.ERR_INVALID_PLAN
    # an encoded inner column; more columns than the flattened plan may have
    def encoded(p):
        p.inner_cols[sx.D_SEG].encoding = capi.ENC_DICT
    assert code_of(encoded) == capi.ERR_UNSUPPORTED
    def full(p):
        for c in range(p.n_cols, capi.MAX_COLS - 1):
            p.cols[c] = p.cols[sx.Q]
        p.n_cols = capi.MAX_COLS - 1          # + d.region, d.segment and the matched flag: 18 columns
    assert code_of(full) == capi.ERR_UNSUPPORTED


def test_explain_and_reserve_answer_like_execute_for_a_refused_plan(sim):
    """an encoded inner column: every entry point that meets the plan refuses it alike"""
    sc = CASES[0]
    ra = copy.deepcopy(sc.case.ra)
    ra.inner_col_descs[sx.D_SEG].encoding = capi.ENC_DICT
    hj, keep = flow._build_join(sc.case)
    ra.join_table = hj
    fr = flow._fetch_result(sc.case)
    for call in (lambda: Executor(0).initQueryMemoryDescriptor(ra), lambda: Executor(0).explain(ra, [1000], inner_rows=1000),
                 lambda: Executor(0).reserveWorkspace(ra, fr), lambda: Executor(0).executeWorkUnit(ra, fr, allow_retry=False)):
        with pytest.raises(capi.Mi355qError) as ei:
            call()
        assert ei.value.code == capi.ERR_UNSUPPORTED


def test_the_asynchronous_call_completes_the_step_inside_the_call(sim, oracle):
    sc = CASES[0]
    hj, keep = flow._build_join(sc.case)
    sc.case.ra.join_table = hj
    try:
        rs, pending = Executor(0).executeWorkUnitAsync(sc.case.ra, flow._fetch_result(sc.case))
        pending.wait()
    finally:
        sc.case.ra.join_table = None
    q, want, code = sx.oracle_reference(oracle, sc)
    from tests.helpers import compare_buffers
    compare_buffers(q, want, rs.getStorage(), sc.case.fp_rtol)


def planned_route(flags=0, groups=100, dim_slots=1_000_000, make_join=flow._build_join):
    """the planner's own choice for 1 B fact rows, no launch"""
    sc = CASES[0]
    ra = copy.deepcopy(sc.case.ra)
    ra.inner_col_descs[sx.D_REGION].range = ExpressionRange(True, 0, groups - 1)
    hj, keep = make_join(sc.case)
    ra.join_table = hj
    return Executor(0).explain(ra, [250_000_000] * 4, inner_rows=dim_slots, flags=flags)


def test_the_planner_takes_the_star_member_for_a_billion_rows_and_the_flag_removes_it(sim):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    assert sx.STAR_NOTE in planned_route()
    route = planned_route(capi.OPT_NO_STAR_GROUPBY)
    assert sx.STAR_NOTE not in route and route.startswith(sx.FLAT_NOTE + "k_join_gather"), route
