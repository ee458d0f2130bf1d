"""SEMI and ANTI join levels on the CPU: the cases of tests/semi_join_cases.py through the library's host code on the host
simulation (tests/hostsim) — plan.cpp exists_join_plans, api_routes.cpp execute_exists_join, the real k_join_exists_mask members —
against the oracle on a masked joinless plan the cases file builds with numpy alone and against SQLite on the query text.  The same
cases run on the device in tests/test_zz_gpu_semi_join.py (and, with MI355Q_HOSTSIM=real, on the simulation that compiles
every kernel file for the host)."""
import copy
import ctypes as C

import numpy as np
import pytest

from heavydb_amd import capi
from heavydb_amd.executor import Executor, FetchResult, Qual, TargetExpr
from tests import semi_join_cases as sj
from tests import test_hostsim_flow as flow
from tests.test_hostsim_flow import sim  # noqa: F401  (the fixture)
from tests.test_star_join import _unaligned

RUNS = [(sc, kind, vid, opts) for sc in sj.CASES for _, kind in sj.KINDS for vid, opts in sj.variants()]
RUN_IDS = [f"{sc.name}-{'semi' if kind == capi.JOIN_SEMI else 'anti'}-{vid}" for sc, kind, vid, _ in RUNS]


def host_fetch(sc, case):
    frags = [[(_unaligned if sc.unaligned else flow._aligned)(a) for a in cols] for cols in case.frags]
    return FetchResult([[a.ctypes.data for a in cols] for cols in frags], [len(cols[0]) for cols in frags], [], 0, 0, [frags])


def run_one(oracle, sc, kind, opts, make_join=flow._build_join, make_fetch=host_fetch):
    """one case one way: the descriptor, the route, the result (or the error code) against both references"""
    case = sj.stated(sc, kind)
    hj, keep = make_join(case)
    case.ra.join_table = hj
    ex = Executor(0)
    # mi355q_qmd_init of the stated plan = the joinless plan's descriptor, bit for bit
    assert bytes(ex.initQueryMemoryDescriptor(case.ra)) == bytes(ex.initQueryMemoryDescriptor(sj.joinless(sc)))
    route = ex.explain(case.ra, [len(f[0]) for f in case.frags], kernel_variant=opts.get("kernel_variant", 0))
    assert route.startswith(sj.NOTE[kind]) and sj.KERNEL in route, route
    if sc.dim.name != "empty":   # (mi355q_explain assumes aligned chunks: the unaligned case is planned like its aligned twin)
        assert ("(fast member)" in route) == (not sc.general) and ("(general member)" in route) == sc.general, route
    fr = make_fetch(sc, case)
    if sc.small_buffer:
        with pytest.raises(capi.Mi355qError) as ei:
            ex.executeWorkUnit(case.ra, fr, allow_retry=False, **opts)
        # (the oracle's code is negative too; the library's carries the count the caller needs for the retry)
        assert sj.oracle_reference(oracle, sc, kind)[2] < 0 and ei.value.code == -sj.passing_rows(sc, kind), ei.value.code
        return None
    rs = ex.executeWorkUnit(case.ra, fr, allow_retry=False, **opts)
    sj.check_result(oracle, sc, kind, rs)
    return rs


@pytest.mark.parametrize("sc,kind,vid,opts", RUNS, ids=RUN_IDS)
def test_semi_and_anti_joins_on_the_host_simulation(sim, oracle, sc, kind, vid, opts):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    run_one(oracle, sc, kind, opts)


def _case(name):
    return next(sc for sc in sj.CASES if sc.name == name)


def _count(oracle, sc, kind, join_kind=None, **opts):
    """COUNT(*) of a non-grouped case through the library"""
    case = sj.stated(sc, kind)
    if join_kind is not None:
        case.ra.join_kind = join_kind
    hj, keep = flow._build_join(case)
    case.ra.join_table = hj
    rs = Executor(0).executeWorkUnit(case.ra, host_fetch(sc, case), allow_retry=False, **opts)
    return rs


def test_semi_counts_a_row_once_however_many_inner_rows_match(sim, oracle):
    """SEMI over the one-to-many table = SEMI over its de-duplicated one-to-one table, table for table; the INNER join over the
    one-to-many table counts a fact row once per match"""
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    assert set(sj.DIMS["many"].keys) == set(sj.DIMS["one"].keys) and len(sj.DIMS["many"].keys) > len(sj.DIMS["one"].keys)
    for step in ("non_grouped", "few_groups"):
        many = _count(oracle, _case(f"many_{step}"), capi.JOIN_SEMI)
        one = _count(oracle, _case("non_grouped_count_sum" if step == "non_grouped" else "few_groups"), capi.JOIN_SEMI)
        assert bytes(many.getQueryMemDesc()) == bytes(one.getQueryMemDesc())
        a, b = many.getStorage(), one.getStorage()
        if step == "non_grouped":
            assert (a == b).all()
        else:   # (an AVG slot's DOUBLE sum may differ in its last bits between two runs)
            from tests.helpers import compare_buffers
            compare_buffers(one.getQueryMemDesc(), b, a, 1e-9)
    semi = int(_count(oracle, _case("many_non_grouped"), capi.JOIN_SEMI).fetch()[0][0, 0])
    inner = int(_count(oracle, _case("many_non_grouped"), capi.JOIN_SEMI, join_kind=capi.JOIN_INNER).fetch()[0][0, 0])
    every = np.concatenate([cols[sj.DID] for cols in sj.FRAGS])
    per_key = {int(k): int(c) for k, c in zip(*np.unique(sj.DIMS["many"].keys, return_counts=True))}
    want_inner = sum(per_key.get(int(k), 0) for k in every)
    assert semi == sj.passing_rows(_case("many_non_grouped"), capi.JOIN_SEMI)
    assert inner == want_inner and inner > semi, (semi, inner)
    assert (semi, inner) == (35208, 56170)     # fact rows whose key the dimension has / joined rows


def test_the_general_member_agrees_with_the_fast_member(sim, oracle):
    """OPT_LDS_GENERIC_MEMBER (the typed members' A/B switch) sends a fast-member shape to the general member"""
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    for name in ("few_groups", "many_non_grouped", "int32_key"):
        for _, kind in sj.KINDS:
            sc = _case(name)
            case = sj.stated(sc, kind)
            hj, keep = flow._build_join(case)
            case.ra.join_table = hj
            rs = Executor(0).executeWorkUnit(case.ra, host_fetch(sc, case), allow_retry=False, flags=capi.OPT_LDS_GENERIC_MEMBER)
            sj.check_result(oracle, sc, kind, rs)


def test_several_passes_fold_to_the_same_result(sim, oracle):
    sim.hostsim_configure(flow.ALL_ROUTES, 0, 0, 0)
    # (a Projection folded from several passes is an appended result: its entry count is the passes' sum, as for every
    # derived route over the pass loop)
    for name in ("few_groups", "non_grouped_count_sum", "baseline_bigint_key"):
        run_one(oracle, _case(name), capi.JOIN_ANTI, {"pass_rows": 16390})


def test_reserve_workspace_holds_the_mask_region(sim):
    """mi355q_reserve_workspace reports (and allocates) the passes' mask region beside the derived step's scratch"""
    sc = _case("baseline_bigint_key")
    case = sj.stated(sc, capi.JOIN_SEMI)
    hj, keep = flow._build_join(case)
    case.ra.join_table = hj
    fr = host_fetch(sc, case)
    # the derived step alone (the cases file's masked joinless plan: one more column), then the SEMI step
    ref = sj.reference_case(sc, capi.JOIN_SEMI)
    frags = [[flow._aligned(a) for a in cols] for cols in ref.frags]
    fr_ref = FetchResult([[a.ctypes.data for a in cols] for cols in frags], [len(cols[0]) for cols in frags], [], 0, 0, [frags])
    held_derived = Executor(0).reserveWorkspace(ref.ra, fr_ref, kernel_variant=2)
    held = Executor(0).reserveWorkspace(case.ra, fr, kernel_variant=2)
    assert held >= held_derived + sj.N_ROWS, (held, held_derived)     # one byte per row


# ------------------------------------------------------------------------------- the refusals
def _entry_points(ra, sc, case):
    fr = host_fetch(sc, case)
    rows = [len(f[0]) for f in case.frags]
    return [lambda: Executor(0).initQueryMemoryDescriptor(ra), lambda: Executor(0).explain(ra, rows),
            lambda: Executor(0).reserveWorkspace(ra, fr), lambda: Executor(0).executeWorkUnit(ra, fr, allow_retry=False)]


def _refused(ra, sc, case, code, skip_qmd=False):
    for i, call in enumerate(_entry_points(ra, sc, case)):
        if skip_qmd and i == 0:
            continue
        with pytest.raises(capi.Mi355qError) as ei:
            call()
        assert ei.value.code == code, (i, ei.value.code)


@pytest.mark.parametrize("kind", [k for _, k in sj.KINDS], ids=[n for n, _ in sj.KINDS])
def test_refusals_return_their_documented_codes_at_every_entry_point(sim, kind):
    from heavydb_amd.executor import Expr, InputColDescriptor, ExpressionRange, inner
    sc = _case("few_groups")
    case = sj.stated(sc, kind)
    hj, keep = flow._build_join(case)

    def plan(**changes):
        ra = copy.copy(case.ra)
        ra.join_table = hj
        for k, v in changes.items():
            setattr(ra, k, v)
        return ra

    inner_desc = [InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 6))]
    # the inner side is not readable: a target with table = 1, an inner reference in a qual / a group column, no join table
    _refused(plan(target_exprs=list(case.ra.target_exprs[:2]) + [TargetExpr(capi.SUM, 0, 1)], inner_col_descs=inner_desc), sc, case,
             capi.ERR_INVALID_PLAN)
    _refused(plan(simple_quals=[Qual(inner(0), capi.EQ, 3)], inner_col_descs=inner_desc), sc, case, capi.ERR_INVALID_PLAN)
    _refused(plan(groupby_exprs=[inner(0)], inner_col_descs=inner_desc), sc, case, capi.ERR_INVALID_PLAN)
    _refused(plan(join_table=None), sc, case, capi.ERR_INVALID_PLAN)
    # expressions; no room for the mask column / its qual
    e = Expr.col(sj.AMT)
    _refused(plan(exprs=[e]), sc, case, capi.ERR_UNSUPPORTED)
    full_cols = list(case.ra.input_col_descs) + [case.ra.input_col_descs[sj.Q]] * (capi.MAX_COLS - len(case.ra.input_col_descs))
    ra = plan(input_col_descs=full_cols)
    wide = sj.Case("wide", ra, [list(cols) + [cols[sj.Q]] * (capi.MAX_COLS - len(cols)) for cols in case.frags])
    _refused(ra, sc, wide, capi.ERR_UNSUPPORTED)
    _refused(plan(simple_quals=[Qual(sj.V32, capi.GT, -2000)] * capi.MAX_QUALS), sc, case, capi.ERR_UNSUPPORTED)
    # ... while one column and one qual fewer are accepted
    ok = plan(input_col_descs=full_cols[:-1], simple_quals=[Qual(sj.V32, capi.GT, -2000)] * (capi.MAX_QUALS - 1))
    assert sj.KERNEL in Executor(0).explain(ok, [1000])


def test_a_join_kind_the_library_does_not_know_stays_unsupported(sim):
    sc = _case("few_groups")
    case = sj.stated(sc, capi.JOIN_SEMI)
    hj, keep = flow._build_join(case)
    ra = copy.copy(case.ra)
    ra.join_table = hj
    ra.join_kind = 4
    # (mi355q_qmd_init has no opinion on the kind of a join whose inner side the plan does not read)
    _refused(ra, sc, case, capi.ERR_UNSUPPORTED, skip_qmd=True)


def test_the_asynchronous_call_completes_the_step_inside_the_call(sim, oracle):
    sc = _case("few_groups")
    case = sj.stated(sc, capi.JOIN_ANTI)
    hj, keep = flow._build_join(case)
    case.ra.join_table = hj
    rs, pending = Executor(0).executeWorkUnitAsync(case.ra, host_fetch(sc, case))
    pending.wait()
    sj.check_result(oracle, sc, capi.JOIN_ANTI, rs)
    # ... and a refused plan is refused inside the call
    ra = copy.copy(case.ra)
    ra.join_table = None
    with pytest.raises(capi.Mi355qError) as ei:
        Executor(0).executeWorkUnitAsync(ra, host_fetch(sc, case))
    assert ei.value.code == capi.ERR_INVALID_PLAN


def test_abi_values():
    assert (capi.JOIN_INNER, capi.JOIN_LEFT, capi.JOIN_SEMI, capi.JOIN_ANTI) == (0, 1, 2, 3)
    assert capi.ABI_VERSION == 7
