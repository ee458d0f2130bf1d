"""Cases of the few-groups GROUP BY whose aggregate arguments are expressions evaluated beside the LDS table
(k_groupby_lds_prog, route `grouped aggregate arguments as register programs`): the plans the route takes, the errors it
must raise or must not raise, and the plans it must leave to the projection pass.  Shared by
tests/test_grouped_agg_programs.py (host simulation) and tests/test_zz_gpu_grouped_agg_programs.py (device).

The table of tests/agg_prog_cases.py (without its FLOAT / INT16 / encoded columns) — 50 001 rows in fragments [1, 0, 16 385, 5, 3, rest]: an empty fragment, fragments
shorter than a quad, a quad remainder, tail rows, several tiles of the kernel (2048 rows each) — plus four key columns.
Every case runs with kernel_variant 2 (the route's size rule admits a small table only then) unless OPTIONS says otherwise.
DOUBLE data is positive as in agg_prog_cases, so the 1e-9 bar holds for any order of summation."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Tuple

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import AVG, COUNT, DOUBLE, GE, GT, INT32, INT64, LT, MAX, MIN, PROJECT_KEY, SUM
from heavydb_amd.executor import Expr, Qual, TargetExpr
from tests import agg_prog_cases as apc
from tests.agg_prog_cases import A, B, CQ, P, Q, T8, X, Y, C, L32, aligned, host_fetch_result  # noqa: F401
from tests.cases import NP, NULLS, Case

N = apc.N
ROUTE = "grouped aggregate arguments as register programs"
KERNEL = "k_groupby_lds_prog"

# A .. T8 as in agg_prog_cases; its FLOAT / INT16 / encoded columns are left out (a plan holds 16 columns, expressions
# included, and only that module's refused shapes read them); then Z and the key columns.  NC: the first expression's column
# in the lowered plan
Z, G100, G3N, G64, GW = range(apc.T8 + 1, apc.T8 + 6)
NC = GW + 1

# per case: (kernel_variant, flags); the default is (2, 0)
OPTIONS: Dict[str, Tuple[int, int]] = {}


def options(case: Case) -> Tuple[int, int]:
    return OPTIONS.get(case.name, (2, 0))


def _columns(rng, n: int) -> List[tuple]:
    cols = apc._columns(rng, n)
    cols = cols[:apc.T8 + 1] + [cols[apc.Z]]
    g3n = rng.integers(-1, 2, n).astype(np.int32)
    g3n[rng.random(n) < 0.07] = NP[INT32](NULLS[INT32])
    return cols + [
        (INT32, False, rng.integers(0, 100, n).astype(np.int32), 0, 0),        # G100
        (INT32, True, g3n, 0, 0),                                              # G3N: three groups and the NULL group
        (INT64, False, rng.integers(10, 30, n).astype(np.int64), 0, 0),        # G64
        (INT32, False, rng.integers(0, 20_000, n).astype(np.int32), 0, 0),     # GW: a table of several windows
    ]


def _keys(n: int) -> List[TargetExpr]:
    return [TargetExpr(PROJECT_KEY, k) for k in range(n)]


def all_kinds(col: int, n_keys: int = 1) -> List[TargetExpr]:
    return _keys(n_keys) + apc.all_kinds(col)


def taken_cases(n: int = N, seed: int = 177) -> List[Case]:
    rng = np.random.default_rng(seed)
    descs, frags = apc._table(_columns(rng, n), n)
    u = lambda *a, **k: apc._unit(descs, frags, *a, **k)   # noqa: E731
    ab = C(A).mul(C(B), INT32)
    xy = C(X).sub(C(Y), INT64)
    dbl = C(P).mul(Expr.lit(DOUBLE, 2.5), DOUBLE).sub(C(Q), DOUBLE)
    half = [Qual(CQ, LT, 50)]
    return [
        Case("i32_product_all_kinds", u([ab], all_kinds(NC), half, group=[G100]), frags),
        Case("nullable_key_three_groups", u([ab], all_kinds(NC), half, group=[G3N]), frags),
        Case("two_keys_three_arguments", u([ab, xy], _keys(2) + [TargetExpr(SUM, NC), TargetExpr(SUM, NC + 1), TargetExpr(MIN, NC + 1),
                                                                 TargetExpr(MAX, Y), TargetExpr(COUNT)], half, group=[G100, G64]), frags),
        Case("double_program", u([dbl], _keys(1) + [TargetExpr(SUM, NC), TargetExpr(MIN, NC), TargetExpr(MAX, NC), TargetExpr(AVG, NC)],
                                 half, group=[G100]), frags),
        Case("key_is_operand_and_qual_column", u([ab], _keys(1) + [TargetExpr(SUM, NC), TargetExpr(COUNT)], [Qual(B, LT, 500)], group=[B]), frags),
        Case("cast_bigint_product", u([C(A).cast(INT64).mul(C(Y), INT64)], all_kinds(NC), half + [Qual(T8, GT, -50)], group=[G100]), frags),
        Case("no_qual", u([ab], all_kinds(NC), group=[G100]), frags),
        Case("two_quals_on_one_column", u([ab], all_kinds(NC), [Qual(CQ, GE, 10), Qual(CQ, LT, 60)], group=[G100]), frags),
        Case("quals_on_three_columns_one_bigint", u([ab], all_kinds(NC), [Qual(CQ, LT, 80), Qual(Y, LT, 500_000), Qual(B, LT, 900)],
                                                    group=[G64]), frags),
        Case("filter_passes_no_row", u([ab], all_kinds(NC), [Qual(CQ, LT, -5)], group=[G100]), frags),
        Case("all_null_operand", u([C(Z).mul(C(B), INT32)], all_kinds(NC), half, group=[G100]), frags),
        # sum, min, max (8 bytes each), rows and the non-NULL count (4 each): 32 bytes x 20 000 entries = 640 KB, several LDS
        Case("windowed_table", u([xy], all_kinds(NC), half, group=[GW]), frags),
        Case("one_window", u([xy], all_kinds(NC), half, group=[G100]), frags),
    ]


# report.variant: 6 with one window, 7 with several
VARIANT = {"windowed_table": 7, "one_window": 6}


def large_case(n: int = 2_000_003, variant: int = 2) -> Case:
    """every workgroup of the device's grid takes several tiles.  The table is past the route's size threshold (2^20 rows),
    but the class rule keeps the step on the projection pass at the default variant (INT32 arguments lost to the two-pass
    route when measured: 11.4 ms against 7.9 ms per 1 B rows): variant 2 takes the route, variant 0 must not"""
    c = taken_cases(n, seed=178)[0]
    c.name = "i32_product_all_kinds_2m" + ("" if variant == 2 else "_default_variant")
    OPTIONS[c.name] = (variant, 0)
    return c


def error_cases(seed: int = 179) -> List[Case]:
    """a small table per case: the row that overflows is placed by hand"""
    n = N
    fs = apc.frag_sizes(n)
    first_of_last = sum(fs[:-1])
    out = []

    def case(name, mutate, exprs, targets, quals, expect, group, late=None):
        rng = np.random.default_rng(seed)
        cols = _columns(rng, n)
        arrs = [a for _, _, a, _, _ in cols]
        arrs[A][arrs[A] == NULLS[INT32]] = 1   # (the rows placed below must not be NULL by accident)
        mutate(arrs)
        descs, frags = apc._table(cols, n)
        unit = apc._unit(descs, frags, exprs, targets, quals, group=group)
        if late:   # after the columns' ranges have been declared
            late(arrs)
            _, frags = apc._table(cols, n)
        out.append(Case(name, unit, frags, expect_error=expect))

    ab = [C(A).mul(C(B), INT32)]
    tg = _keys(1) + [TargetExpr(SUM, NC), TargetExpr(COUNT)]
    half = [Qual(CQ, LT, 50)]
    OVF = capi.ERR_OVERFLOW_OR_UNDERFLOW

    def put(row, passes):
        def m(arrs):
            arrs[A][row] = 70_000
            arrs[B][row] = 70_000
            arrs[CQ][row] = 7 if passes else 77
        return m
    mid = 1 + 5_000   # a row inside the third fragment's tiles
    case("i32_overflow_in_a_passing_row", put(mid, True), ab, tg, half, OVF, [G100])
    case("i32_overflow_only_in_dropped_rows", put(mid, False), ab, tg, half, None, [G100])
    case("i32_overflow_in_the_last_partial_quads_row", put(n - 1, True), ab, tg, half, OVF, [G100])
    # the last row of the 5-row fragment is its partial quad's only valid row: dropped by the qual, and the three copies of it
    # that fill the quad's registers are no rows at all
    case("i32_overflow_behind_a_fragments_end_never_raises", put(1 + 16_385 + 4, False), ab, tg, half, None, [G100])

    def big64(arrs):
        arrs[X][first_of_last + 9] = 2**40
        arrs[Y][first_of_last + 9] = 2**40
        arrs[CQ][first_of_last + 9] = 3
    case("i64_product_overflow", big64, [C(X).mul(C(Y), INT64)], _keys(1) + [TargetExpr(MAX, NC), TargetExpr(COUNT)], half, OVF, [G100])

    def wide(arrs):
        arrs[Y][mid] = 2**40
        arrs[CQ][mid] = 3
    case("narrowing_cast_overflow", wide, [C(Y).cast(INT32)], tg, half, OVF, [G100])

    def stray_key(arrs):
        arrs[G100][mid] = 5_000
        arrs[CQ][mid] = 3
    case("key_outside_its_declared_range", lambda arrs: None, ab, tg, half, capi.ERR_OUT_OF_SLOTS, [G100], late=stray_key)
    return out


def not_taken_cases(seed: int = 180) -> List[Case]:
    rng = np.random.default_rng(seed)
    descs, frags = apc._table(_columns(rng, N), N)
    u = lambda *a, **k: apc._unit(descs, frags, *a, **k)   # noqa: E731
    ab = C(A).mul(C(B), INT32)
    xy = C(X).sub(C(Y), INT64)
    half = [Qual(CQ, LT, 50)]
    s = lambda c: _keys(1) + [TargetExpr(SUM, c), TargetExpr(COUNT)]   # noqa: E731
    taken = u([ab], s(NC), half, group=[G100])
    cases = [
        Case("division", u([C(A).div(L32(7), INT32)], s(NC), half, group=[G100]), frags),
        Case("case_when", u([Expr.case(C(B).cmp(capi.EX_LT, L32(500)), C(A), C(B), INT32)], s(NC), half, group=[G100]), frags),
        # (nearly every row a group of its own: the baseline table gets room for them)
        Case("double_key_is_a_baseline_layout", dataclasses.replace(u([ab], s(NC), half, group=[Q]), max_groups_buffer_entry_guess=1 << 17), frags),
        Case("wide_range_key_is_a_baseline_layout", dataclasses.replace(u([ab], s(NC), half, group=[X]), max_groups_buffer_entry_guess=1 << 17), frags),
        Case("expression_key", u([C(A).add(C(B), INT32), ab], s(NC + 1), half, group=[NC]), frags),
        Case("four_arguments", u([ab, C(A).add(C(B), INT32), C(A).sub(C(B), INT32)],
                                 _keys(1) + [TargetExpr(SUM, NC), TargetExpr(SUM, NC + 1), TargetExpr(SUM, NC + 2), TargetExpr(SUM, B)], half,
                                 group=[G100]), frags),
        Case("expression_read_by_a_qual", u([C(A).add(C(B), INT32)], s(NC), [Qual(NC, GT, 500)], group=[G100]), frags),
        Case("count_if_target", u([ab], _keys(1) + [TargetExpr(SUM, NC), TargetExpr(capi.COUNT_IF, cond=Qual(B, LT, 500))], half, group=[G100]), frags),
        Case("output_columnar_hint", dataclasses.replace(u([ab], s(NC), half, group=[G100]), output_columnar_hint=capi.OUTPUT_COLUMNAR), frags),
        # three arguments over 20 000 entries: 7 x 8 bytes of sums / minima / maxima + rows + two non-NULL counts = 68 bytes per
        # entry, 1.36 MB against 8 windows x 152 KB
        Case("table_beyond_eight_windows", u([ab, xy, C(P).mul(Expr.lit(DOUBLE, 2.5), DOUBLE)],
                                             _keys(1) + [TargetExpr(SUM, NC), TargetExpr(MIN, NC), TargetExpr(MAX, NC), TargetExpr(SUM, NC + 1),
                                                         TargetExpr(MIN, NC + 1), TargetExpr(SUM, NC + 2), TargetExpr(MIN, NC + 2)], half, group=[GW]), frags),
        # operand columns A and B, the key, and two columns read for the filter alone: five columns under range quals, one more
        # than the member holds
        Case("quals_on_five_columns", u([ab], s(NC), [Qual(A, GE, 0), Qual(B, LT, 950), Qual(G100, LT, 99), Qual(CQ, LT, 80), Qual(T8, GT, -100)],
                                        group=[G100]), frags),
        Case("small_table_at_the_default_variant", taken, frags),
        Case("opted_out", taken, frags),
    ]
    OPTIONS["small_table_at_the_default_variant"] = (0, 0)
    OPTIONS["opted_out"] = (2, capi.OPT_NO_GROUPED_AGG_PROGRAMS)
    return cases


_REFERENCE: Dict[str, tuple] = {}


def reference(oracle, case: Case):
    """the oracle's answer for a case, computed once (a cache of its own: agg_prog_cases names some of its cases alike)"""
    if case.name not in _REFERENCE:
        _REFERENCE[case.name] = apc.reference(oracle, dataclasses.replace(case, name="grouped/" + case.name))
    return _REFERENCE[case.name]


def slots_agree(new, old):
    """both routes, group by group: key quads and integer slots bit for bit, DOUBLE sums / minima / maxima within the
    project's 1e-9"""
    q = new.getQueryMemDesc()
    a, b = np.asarray(new.getStorage()).reshape(-1).view(np.int64), np.asarray(old.getStorage()).reshape(-1).view(np.int64)
    row = q.row_size // 8
    first = row - q.slot_count   # the key quads come first
    assert a.size == b.size == q.entry_count * row
    for e in range(q.entry_count):
        ra, rb = a[e * row:(e + 1) * row], b[e * row:(e + 1) * row]
        assert (ra[:first] == rb[:first]).all(), (e, ra[:first], rb[:first])
        for t in range(q.n_targets):
            if q.target_slot[t] < 0:
                continue
            s = first + q.target_slot[t]
            if q.target_arg_is_fp[t] and q.target_agg[t] != capi.PROJECT_KEY:
                x, y = ra[s:s + 1].view(np.float64)[0], rb[s:s + 1].view(np.float64)[0]
                assert x == y or abs(x - y) <= 1e-9 * max(abs(x), abs(y)), (e, t, x, y)
                if q.target_agg[t] == capi.AVG:
                    assert ra[s + 1] == rb[s + 1], (e, t)
            else:
                n = 2 if q.target_agg[t] == capi.AVG else 1
                assert (ra[s:s + n] == rb[s:s + n]).all(), (e, t, ra[s:s + n], rb[s:s + n])
