"""Cases of the non-grouped aggregates whose arguments are expressions evaluated in the scan's registers (k_scan_agg_prog,
route `aggregate arguments as register programs`): the plans the route takes, the errors it must raise or must not raise,
and the plans it must leave to the projection pass.  Shared by tests/test_agg_programs.py (host simulation) and
tests/test_zz_gpu_agg_programs.py (device).

The table: about 50 000 rows in fragments [1, 0, 16 385, 5, 3, rest] — an empty fragment, fragments shorter than a quad, a
quad remainder, tail rows (the last fragment's row count is 3 mod 4) and several tiles of the kernel (2048 rows each).
DOUBLE data is chosen so that every `p * 2.5 - q` is positive: the sums do not cancel, and the 1e-9 bar holds for any
order of summation (about 5e4 additions of 2^-53 relative error each: below 1e-11)."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import AVG, COUNT, DOUBLE, GE, GT, INT8, INT16, INT32, INT64, LT, MAX, MIN, SUM
from heavydb_amd.executor import Expr, FetchResult, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests.cases import NP, NULLS, Case, col_range, expr_range, split

N = 50_001
ROUTE = "aggregate arguments as register programs"
KERNEL = "k_scan_agg_prog"

# columns
A, B, CQ, X, Y, P, Q, T8, F32, S16, ENC, Z, NC = range(13)


def frag_sizes(n: int) -> List[int]:
    head = [1, 0, 16_385, 5, 3]
    return head + [n - sum(head)]


def _columns(rng, n: int) -> List[tuple]:
    """(type, nullable, values, encoding, logical type)"""
    def nulls(a, t, frac=0.07):
        a = a.copy()
        a[rng.random(n) < frac] = NP[t](NULLS[t])
        return a
    return [
        (INT32, True, nulls(rng.integers(0, 1000, n).astype(np.int32), INT32), 0, 0),             # A
        (INT32, False, rng.integers(0, 1000, n).astype(np.int32), 0, 0),                          # B
        (INT32, False, rng.integers(0, 100, n).astype(np.int32), 0, 0),                           # CQ: the usual qual column
        (INT64, True, nulls(rng.integers(-10**9, 10**9, n).astype(np.int64), INT64), 0, 0),       # X
        (INT64, False, rng.integers(-10**6, 10**6, n).astype(np.int64), 0, 0),                    # Y
        (DOUBLE, True, nulls(100.0 + rng.random(n) * 900.0, DOUBLE), 0, 0),                       # P: p * 2.5 >= 250
        (DOUBLE, False, rng.random(n) * 100.0, 0, 0),                                             # Q: q < 100
        (INT8, False, rng.integers(-100, 100, n).astype(np.int8), 0, 0),                          # T8
        (capi.FLOAT, False, rng.random(n).astype(np.float32) * 10, 0, 0),                         # F32
        (INT16, False, rng.integers(-3000, 3000, n).astype(np.int16), 0, 0),                      # S16
        (INT16, False, rng.integers(-3000, 3000, n).astype(np.int16), capi.ENC_FIXED, INT32),     # ENC: FIXED(16) of an INT
        (INT32, True, np.full(n, NULLS[INT32], np.int32), 0, 0),                                  # Z: all NULL
    ]


def _table(cols, n: int):
    fs = frag_sizes(n)
    descs = []
    for t, nullable, a, enc, logical in cols:
        descs.append(InputColDescriptor(t, nullable, col_range([a], t, nullable), enc, logical))
    per_col = [split(a, fs) for _, _, a, _, _ in cols]
    frags = [[per_col[c][f] for c in range(len(cols))] for f in range(len(fs))]
    return descs, frags


def _unit(descs, frags, exprs, targets, quals=(), group=()):
    xs = [e.with_range(expr_range(e, descs, frags, exprs[:i])) for i, e in enumerate(exprs)]
    return RelAlgExecutionUnit(list(descs), list(targets), list(quals), list(group), max_groups_buffer_entry_guess=16384, exprs=xs)


C = Expr.col
L32 = lambda v: Expr.lit(INT32, v)   # noqa: E731


def all_kinds(col: int) -> List[TargetExpr]:
    return [TargetExpr(SUM, col), TargetExpr(MIN, col), TargetExpr(MAX, col), TargetExpr(AVG, col), TargetExpr(COUNT, col), TargetExpr(COUNT)]


def taken_cases(n: int = N, seed: int = 77) -> List[Case]:
    rng = np.random.default_rng(seed)
    descs, frags = _table(_columns(rng, n), n)
    u = lambda *a, **k: _unit(descs, frags, *a, **k)   # noqa: E731
    ab = C(A).mul(C(B), INT32)
    half = [Qual(CQ, LT, 50)]
    cases = [
        Case("i32_product_all_kinds", u([ab], all_kinds(NC), half), frags),
        Case("cast_bigint_product", u([C(A).cast(INT64).mul(C(Y), INT64)], all_kinds(NC), half), frags),
        Case("i64_difference", u([C(X).sub(C(Y), INT64)], all_kinds(NC), half), frags),
        Case("literal_first", u([L32(100).sub(C(A), INT32)], all_kinds(NC), half), frags),
        Case("negated_sum", u([C(A).add(C(B), INT32).neg(INT32)], all_kinds(NC), half), frags),
        Case("double_arith_nullable_operand", u([C(P).mul(Expr.lit(DOUBLE, 2.5), DOUBLE).sub(C(Q), DOUBLE)], all_kinds(NC), half), frags),
        Case("program_beside_plain_columns", u([ab], [TargetExpr(SUM, NC), TargetExpr(SUM, CQ), TargetExpr(MAX, Y), TargetExpr(COUNT)], half), frags),
        Case("two_programs_share_a_column", u([ab, C(A).add(C(B), INT32)],
                                              [TargetExpr(SUM, NC), TargetExpr(SUM, NC + 1), TargetExpr(MIN, NC + 1), TargetExpr(COUNT, NC)], half), frags),
        Case("four_arguments_four_columns", u([ab, C(X).sub(C(Y), INT64)],
                                              [TargetExpr(SUM, NC), TargetExpr(MIN, NC + 1), TargetExpr(MAX, B), TargetExpr(AVG, Y), TargetExpr(COUNT)],
                                              half), frags),
        Case("no_qual", u([ab], all_kinds(NC)), frags),
        Case("two_quals_on_one_column", u([ab], all_kinds(NC), [Qual(CQ, GE, 10), Qual(CQ, LT, 60)]), frags),
        Case("quals_on_three_columns_one_bigint", u([ab], all_kinds(NC), [Qual(CQ, LT, 80), Qual(T8, GT, -50), Qual(Y, LT, 500_000)]), frags),
        Case("quals_on_the_operand_columns", u([C(X).sub(C(Y), INT64)], all_kinds(NC), [Qual(X, GT, 0), Qual(Y, LT, 0), Qual(T8, LT, 50)]), frags),
        Case("filter_passes_no_row", u([ab], all_kinds(NC), [Qual(CQ, LT, -5)]), frags),
        Case("all_null_operand", u([C(Z).mul(C(B), INT32)], all_kinds(NC), half), frags),
        Case("double_no_qual_is_not_null", u([C(P).mul(Expr.lit(DOUBLE, 2.5), DOUBLE).sub(C(Q), DOUBLE)],
                                             [TargetExpr(SUM, NC), TargetExpr(AVG, NC), TargetExpr(MAX, Q)], [Qual(A, capi.IS_NOT_NULL)]), frags),
    ]
    return cases


def large_case(n: int = 2_000_003) -> Case:
    """every workgroup of the device's grid takes several tiles"""
    c = taken_cases(n, seed=78)[0]
    c.name = "i32_product_all_kinds_2m"
    return c


def error_cases(seed: int = 79) -> List[Case]:
    """a small table per case: the row that overflows is placed by hand"""
    n = N
    fs = frag_sizes(n)
    first_of_last = sum(fs[:-1])
    out = []

    def table(mutate):
        rng = np.random.default_rng(seed)
        cols = _columns(rng, n)
        arrs = [a for _, _, a, _, _ in cols]
        arrs[A][arrs[A] == NULLS[INT32]] = 1   # (the rows placed below must not be NULL by accident)
        mutate(arrs)
        return _table(cols, n)

    def case(name, mutate, exprs, targets, quals, expect):
        descs, frags = table(mutate)
        out.append(Case(name, _unit(descs, frags, exprs, targets, quals), frags, expect_error=expect))

    ab = [C(A).mul(C(B), INT32)]
    tg = [TargetExpr(SUM, NC), TargetExpr(COUNT)]
    half = [Qual(CQ, LT, 50)]
    OVF = capi.ERR_OVERFLOW_OR_UNDERFLOW

    def put(row, passes):
        def m(arrs):
            arrs[A][row] = 70_000
            arrs[B][row] = 70_000
            arrs[CQ][row] = 7 if passes else 77
        return m
    mid = 1 + 5_000   # a row inside the third fragment's tiles
    case("i32_overflow_in_a_passing_row", put(mid, True), ab, tg, half, OVF)
    case("i32_overflow_only_in_dropped_rows", put(mid, False), ab, tg, half, None)
    case("i32_overflow_in_the_last_partial_quads_row", put(n - 1, True), ab, tg, half, OVF)
    # the last row of the 5-row fragment is its partial quad's only valid row: dropped by the qual, and the three copies of it
    # that fill the quad's registers are no rows at all
    case("i32_overflow_behind_a_fragments_end_never_raises", put(1 + 16_385 + 4, False), ab, tg, half, None)

    def big64(arrs):
        arrs[X][first_of_last + 9] = 2**40
        arrs[Y][first_of_last + 9] = 2**40
        arrs[CQ][first_of_last + 9] = 3
    case("i64_product_overflow", big64, [C(X).mul(C(Y), INT64)], [TargetExpr(MAX, NC), TargetExpr(COUNT)], half, OVF)

    def wide(arrs):
        arrs[Y][mid] = 2**40
        arrs[CQ][mid] = 3
    case("narrowing_cast_overflow", wide, [C(Y).cast(INT32)], [TargetExpr(SUM, NC), TargetExpr(COUNT)], half, OVF)
    return out


def not_taken_cases(seed: int = 80) -> List[Case]:
    rng = np.random.default_rng(seed)
    descs, frags = _table(_columns(rng, N), N)
    u = lambda *a, **k: _unit(descs, frags, *a, **k)   # noqa: E731
    ab = C(A).mul(C(B), INT32)
    half = [Qual(CQ, LT, 50)]
    s = lambda c: [TargetExpr(SUM, c), TargetExpr(COUNT)]   # noqa: E731
    return [
        Case("division", u([C(A).div(L32(7), INT32)], s(NC), half), frags),
        Case("modulo", u([C(A).mod(L32(7), INT32)], s(NC), half), frags),
        Case("case_when", u([Expr.case(C(B).cmp(capi.EX_LT, L32(500)), C(A), C(B), INT32)], s(NC), half), frags),
        Case("float_operand", u([C(F32).cast(DOUBLE).mul(Expr.lit(DOUBLE, 2.0), DOUBLE)], s(NC), half), frags),
        Case("int16_operand", u([C(S16).cast(INT32).add(C(B), INT32)], s(NC), half), frags),
        Case("encoded_operand", u([C(ENC).add(C(B), INT32)], s(NC), half), frags),
        Case("expression_read_by_a_qual", u([C(A).add(C(B), INT32)], s(NC), [Qual(NC, GT, 500)]), frags),
        Case("expression_reads_an_expression", u([C(A).add(C(B), INT32), C(NC).mul(L32(2), INT32)], [TargetExpr(SUM, NC), TargetExpr(SUM, NC + 1)], half), frags),
        Case("grouped", u([ab], [TargetExpr(capi.PROJECT_KEY), TargetExpr(SUM, NC), TargetExpr(COUNT)], half, group=[CQ]), frags),
        Case("five_arguments", u([ab, C(A).add(C(B), INT32), C(A).sub(C(B), INT32)],
                                 [TargetExpr(SUM, NC), TargetExpr(SUM, NC + 1), TargetExpr(SUM, NC + 2), TargetExpr(SUM, B), TargetExpr(SUM, CQ)], half), frags),
        Case("count_if_target", u([ab], [TargetExpr(SUM, NC), TargetExpr(capi.COUNT_IF, cond=Qual(B, LT, 500))], half), frags),
    ]


def aligned(a: np.ndarray, offset: int = 0) -> np.ndarray:
    """a copy of `a` whose first byte sits `offset` bytes behind a 64-byte boundary (empty arrays included)"""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 128, np.uint8)
    off = (-raw.ctypes.data) % 64 + offset
    out = raw[off:off + a.nbytes].view(a.dtype)
    out[...] = a
    return out


def host_fetch_result(case: Case, misalign_col: int = -1) -> FetchResult:
    keep = [[aligned(a, 4 if c == misalign_col else 0) for c, a in enumerate(cols)] for cols in case.frags]
    return FetchResult([[a.ctypes.data for a in cols] for cols in keep], [len(cols[0]) for cols in keep], [], 0, 0, [keep])


_REFERENCE: Dict[str, tuple] = {}


def reference(oracle, case: Case):
    """the oracle's answer for a case, computed once"""
    if case.name not in _REFERENCE:
        _REFERENCE[case.name] = oracle.execute(case.ra.to_plan(), case.frags, n_threads=8)
    return _REFERENCE[case.name]
