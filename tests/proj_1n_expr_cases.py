"""Projection steps with EXPRESSIONS through a ONE-TO-MANY join (k_proj_join_1n's expression-carrying member), shared by
the host-simulation tests (tests/test_projection_1n_exprs.py) and the device tests (tests/test_zz_gpu_projection_1n_exprs.py):

    SELECT t.a + 5, d.w, CAST(t.f AS DOUBLE) * 2.5, ... FROM t JOIN d ON t.k = d.k WHERE t.f + 1 < 500 ...

The dimension is the `dup` construction of proj_cases.build_join_cases (keys with 1 to 4 matches, 50 keys with none, outer
keys partly outside the range).  The outer table has 50 000 rows in fragments [1, 16384, 16385, 5, rest]: a tile is 16 384
rows, so there are fragments of several tiles, a tile boundary one row into a fragment, ragged ends, and a look-back across
tiles whose entry counts differ."""
from __future__ import annotations

from typing import List

import numpy as np

from heavydb_amd import capi
from heavydb_amd.executor import Expr, ExprNode, ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests.proj_cases import INT_NULL, ProjCase, _split

N_ROWS = 50_000
FRAG_SIZES = [1, 16384, 16385, 5, N_ROWS - 32775]
N_PHYS = 5   # outer columns: k, a, f, k32 (nullable), g — expression j is outer column N_PHYS + j
SEVEN_DEEP = "x1n_seven_expressions_eight_deep"


def build_cases() -> List[ProjCase]:
    rng = np.random.default_rng(1777)
    D, R = InputColDescriptor, ExpressionRange
    I32, I64, F64 = capi.INT32, capi.INT64, capi.DOUBLE
    C_, L = Expr.col, Expr.lit
    m, n = 700, N_ROWS
    dk = rng.permutation(m).astype(np.int64)
    dup = np.concatenate([dk[:m - 50], dk[:50], dk[:20], dk[5:8]])        # keys with 1, 2, 3 and 4 matches; 50 keys with none
    m2 = len(dup)
    inner = [dup, rng.integers(-1000, 1000, m2).astype(np.int64), rng.random(m2), rng.random(m2).astype(np.float32),
             np.where(np.arange(m2) % 9 == 0, INT_NULL[capi.INT16], rng.integers(-100, 100, m2)).astype(np.int16)]
    inner_descs = [D(I64, False, R(True, 0, m - 1)), D(I64, False, R(True, -1000, 999)), D(F64), D(capi.FLOAT),
                   D(capi.INT16, True, R(True, -100, 99, True))]
    k = rng.integers(-60, m + 60, n).astype(np.int64)                     # some keys miss
    kz, kz2 = int(dk[0]), int(dk[1])                                      # kz: a key with several matches, absent from the first half
    k[:n // 2][k[:n // 2] == kz] = kz2
    assert (k[n // 2:] == kz).any() and (k == -10).any() and kz != 0
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    f = rng.integers(0, 1000, n).astype(np.int32)
    assert (f == 0).any()
    k32 = rng.integers(0, m + 40, n).astype(np.int32)
    k32[::11] = INT_NULL[I32]                                             # a NULL key matches nothing
    g = f.copy()
    g[n // 2:] = 2**31 - 3                                                # g + 5 overflows INT32 in the second half
    descs = [D(I64, False, R(True, -60, m + 59)), D(I64), D(I32, False, R(True, 0, 999)), D(I32, True, R(True, 0, m + 39, True)), D(I32)]
    frags = _split([k, a, f, k32, g], FRAG_SIZES)

    cases: List[ProjCase] = []

    def add(name, exprs, targets, quals=(), outer_col=0, kind=capi.JOIN_INNER, keyed=False, guess=3 * n, **kw):
        err = kw.pop("expect_error", None)
        ra = RelAlgExecutionUnit(list(descs), [TargetExpr(capi.PROJECT, c, t) for c, t in targets], list(quals),
                                 inner_col_descs=list(inner_descs), join_outer_col=outer_col, join_kind=kind,
                                 max_groups_buffer_entry_guess=guess, exprs=list(exprs), **kw)
        cases.append(ProjCase(name, ra, frags, err, 0, list(inner), dup, I64, R(True, 0, m - 1), keyed, 1, False))

    X = N_PHYS
    e_add = C_(1).add(L(I64, 5), I64)                                      # INT64 column + literal
    e_mul = C_(2).cast(F64).mul(L(F64, 2.5), F64)                          # CAST(INT32 AS DOUBLE) * literal
    e_case = Expr.case(C_(2).cmp(capi.EX_NE, L(I32, 0)), C_(1).div(C_(2).cast(I64), I64), L(I64, 0), I64)   # a guarded division
    e_reads = C_(X).sub(C_(0), I64)                                        # reads expression 0: (a + 5) - k
    four = [e_add, e_mul, e_case, e_reads]
    beside = [(X, 0), (1, 1), (X + 1, 0), (4, 1), (X + 2, 0), (X + 3, 0)]  # expressions beside d.w and d.s (nullable INT16)
    # 1. expression targets of each kind beside inner columns: INNER / LEFT, perfect / keyed, row-wise / columnar
    add("x1n_targets_inner_perfect", four, beside)
    add("x1n_targets_left_perfect", four, beside, kind=capi.JOIN_LEFT)
    add("x1n_targets_inner_keyed_columnar", four, beside + [(3, 1)], keyed=True, output_columnar_hint=capi.OUTPUT_COLUMNAR)
    add("x1n_targets_left_keyed_filtered_columnar", four, beside + [(3, 1), (2, 0)], [Qual(2, capi.LT, 700)], kind=capi.JOIN_LEFT, keyed=True,
        output_columnar_hint=capi.OUTPUT_COLUMNAR)
    # 2. WHERE f + 1 < 500 (a BOOLEAN expression = 1) AND a > 0, an expression target; the nullable INT32 join key
    cond = C_(2).add(L(I32, 1), I32).cmp(capi.EX_LT, L(I32, 500))
    add("x1n_expr_qual_inner_perfect", [cond, e_add], [(X + 1, 0), (1, 1), (1, 0)], [Qual(X, capi.EQ, 1), Qual(1, capi.GT, 0)])
    add("x1n_expr_qual_left_keyed_columnar", [cond, e_add], [(X + 1, 0), (1, 1), (2, 1)], [Qual(X, capi.EQ, 1), Qual(1, capi.GT, 0)],
        kind=capi.JOIN_LEFT, keyed=True, output_columnar_hint=capi.OUTPUT_COLUMNAR)
    add("x1n_expr_qual_left_nullable_int32_key", [cond, e_mul], [(0, 0), (X + 1, 0), (1, 1), (4, 1)], [Qual(X, capi.EQ, 1), Qual(1, capi.GT, 0)],
        outer_col=3, kind=capi.JOIN_LEFT)
    add("x1n_expr_qual_inner_nullable_int32_key_keyed", [cond, e_mul], [(X + 1, 0), (1, 1)], [Qual(X, capi.EQ, 1)], outer_col=3, keyed=True)
    # 3. expressions only: no inner column among the targets (the matches still multiply the rows)
    add("x1n_expressions_only", [e_add, e_mul], [(X, 0), (X + 1, 0)])
    add("x1n_expressions_only_left_columnar", [e_add, e_mul], [(X + 1, 0), (X, 0)], kind=capi.JOIN_LEFT, output_columnar_hint=capi.OUTPUT_COLUMNAR)
    # 4. a LIMIT that cuts inside one row's run of matches, in the third fragment's first tile (the tiles behind it write nothing)
    in_dim = (k >= 0) & (k < m)
    cnt = np.where(in_dim, np.bincount(dup, minlength=m)[np.clip(k, 0, m - 1)], 0)
    first = np.cumsum(cnt) - cnt
    row = int(np.nonzero((np.arange(n) > 24_000) & (cnt >= 3))[0][0])
    limit = int(first[row]) + 2
    assert first[row] < limit < first[row] + cnt[row]
    add("x1n_scan_limit_inside_a_run", four, beside, scan_limit=limit)
    cnt_left = np.maximum(cnt, 1)
    first_left = np.cumsum(cnt_left) - cnt_left
    add("x1n_scan_limit_inside_a_run_left_keyed_columnar", four, beside, kind=capi.JOIN_LEFT, keyed=True, scan_limit=int(first_left[row]) + 1,
        output_columnar_hint=capi.OUTPUT_COLUMNAR)
    # 5. the buffer is too small and there is no limit: minus the joined-row count
    add("x1n_buffer_full", [e_add], [(X, 0), (1, 1)], guess=500, expect_error=-1)
    # 6. errors follow the reference's loop nest: the body — and with it a target's expression — runs once per joined row
    div_miss = C_(1).div(C_(0).add(L(I64, 10), I64), I64)                  # a / (k + 10): zero at k = -10, which has no match
    div_hit = C_(1).div(C_(0).sub(L(I64, kz), I64), I64)                   # a / (k - kz): zero at k = kz, which has matches
    add("x1n_div_by_zero_in_unmatched_rows_inner", [div_miss], [(X, 0), (1, 1)])
    add("x1n_div_by_zero_in_unmatched_rows_left", [div_miss], [(X, 0), (1, 1)], kind=capi.JOIN_LEFT, expect_error=capi.ERR_DIV_BY_ZERO)
    add("x1n_div_by_zero_in_a_matched_row", [div_hit], [(X, 0), (1, 1)], expect_error=capi.ERR_DIV_BY_ZERO)
    add("x1n_div_by_zero_in_a_matched_row_keyed_columnar", [div_hit], [(X, 0), (1, 1)], keyed=True, output_columnar_hint=capi.OUTPUT_COLUMNAR,
        expect_error=capi.ERR_DIV_BY_ZERO)
    add("x1n_div_by_zero_past_the_limit", [div_hit], [(X, 0), (1, 1)], scan_limit=50)
    add("x1n_div_by_zero_dropped_by_a_qual", [div_hit], [(X, 0), (1, 1)], [Qual(0, capi.NE, kz)])
    add("x1n_overflow_in_an_emitted_row", [C_(4).add(L(I32, 5), I32)], [(X, 0), (1, 1)], expect_error=capi.ERR_OVERFLOW_OR_UNDERFLOW)
    # 7. seven expressions, each with the deepest stack a plan may have (8 values: a a a a a a a a + + + + + + +) plus j
    deep = [Expr([ExprNode(capi.EX_COL, 0, 1)] * 8 + [ExprNode(capi.EX_ADD, I64)] * 7).add(L(I64, j), I64) for j in range(7)]
    add(SEVEN_DEEP, deep, [(X + j, 0) for j in range(7)] + [(1, 1)])
    return cases
