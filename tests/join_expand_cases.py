"""Grouped steps over a ONE-TO-MANY join (k_join_expand_count / _scan / _write + the step without the join, api_routes.cpp
execute_join_expand), shared by the host-simulation tests (tests/test_join_expand.py) and the device tests
(tests/test_zz_gpu_join_expand.py):

    SELECT f.g, COUNT(*), COUNT(d.x), SUM(d.w), MIN(d.x), MAX(d.x), AVG(d.fd), SUM(f.v) FROM f [LEFT] JOIN d ON f.k = d.k GROUP BY f.g

Every shape is the smallest at which the expansion can go wrong.  The outer table has 50 000 rows in fragments
[1, 16384, 16385, 5, rest]: a tile is 16 384 rows and a lane's quad four, so there are a one-row fragment, a fragment of exactly
one tile, a tile boundary one row into a fragment, a partial quad, and a fragment of several tiles with a ragged end.  The
dimension has 3 300 keys with 0 - 3 rows each (about 5 000 rows) plus ONE hot key with 3 000 rows: an outer row with the hot key
has more joined rows than a workgroup has lanes (its entries span a dozen store steps, written by every lane) and its sub-tile's
total exceeds the 256 entries of one step.  Outer keys miss on both sides of the key range, 3 % of them are NULL, and the
inner column d.x is nullable and holds NULLs."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import AVG, COUNT, COUNT_IF, DOUBLE, INT16, INT32, INT64, MAX, MIN, PROJECT_KEY, SUM, SUM_IF
from heavydb_amd.executor import Expr, ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests.cases import NULLS, Case, col_range

N_ROWS = 50_000
FRAG_SIZES = [1, 16384, 16385, 5, N_ROWS - 32775]
N_KEYS = 3300
HOT_ROWS = 3000
ROUTE_NOTE = "k_join_expand"
# outer columns
K, G, V, K32, G2, GW, G20K, X, GFX = range(9)
N_PHYS = 9
# inner columns
D_K, D_W, D_FD, D_X = range(4)


@dataclass
class ExpandCase:
    case: Case
    opts: Dict[str, int] = field(default_factory=dict)   # beside kernel_variant = 2
    passes: int = 1                                       # passes the route must run
    nothing_joins: bool = False


def _split(cols, sizes):
    out, at = [], 0
    for s in sizes:
        out.append([c[at:at + s] for c in cols])
        at += s
    assert at == len(cols[0])
    return out


def build_cases() -> List[ExpandCase]:
    rng = np.random.default_rng(4242)
    D, R = InputColDescriptor, ExpressionRange
    n, m = N_ROWS, N_KEYS
    # ---- the dimension: every key 0 - 3 times, the hot key HOT_ROWS times, shuffled
    reps = rng.integers(0, 4, m)
    hot = int(m // 2)
    reps[hot] = HOT_ROWS
    dk = np.repeat(np.arange(m, dtype=np.int64), reps)
    rng.shuffle(dk)
    md = len(dk)
    assert 7500 <= md <= 8500 and (reps == 0).sum() > 500
    d_w = rng.integers(-1000, 1000, md).astype(np.int64)
    d_fd = rng.random(md)
    d_x = rng.integers(-100, 100, md).astype(np.int32)
    d_x[rng.random(md) < 0.11] = NULLS[INT32]
    inner = [dk, d_w, d_fd, d_x]
    inner_descs = [D(INT64, False, R(True, 0, m - 1)), D(INT64, False, col_range([d_w], INT64, False)),
                   D(DOUBLE, False, col_range([d_fd], DOUBLE, False)), D(INT32, True, col_range([d_x], INT32, True))]
    join_rng = R(True, 0, m - 1)
    # ---- the fact table
    k = rng.integers(-60, m + 60, n).astype(np.int64)
    k[rng.random(n) < 0.03] = NULLS[INT64]
    k32 = rng.integers(0, m + 40, n).astype(np.int32)
    k32[rng.random(n) < 0.03] = NULLS[INT32]
    assert 5 <= (k == hot).sum() <= 40 and 5 <= (k32 == hot).sum() <= 40
    g = rng.integers(0, 200, n).astype(np.int32)
    v = rng.integers(-10**6, 10**6, n).astype(np.int64)
    g2 = rng.integers(0, 10, n).astype(np.int32)
    g20k = rng.integers(0, 20_000, n).astype(np.int32)
    gw = g20k.astype(np.int64) * 1_000_003_000_003 - 7
    x = rng.integers(-500, 500, n).astype(np.int64)
    x[rng.random(n) < 0.1] = NULLS[INT64]
    gfx = rng.integers(0, 300, n).astype(np.int16)
    cols = [k, g, v, k32, g2, gw, g20k, x, gfx]
    descs = [D(INT64, True, col_range([k], INT64, True)), D(INT32, False, R(True, 0, 199)), D(INT64, False, col_range([v], INT64, False)),
             D(INT32, True, col_range([k32], INT32, True)), D(INT32, False, R(True, 0, 9)), D(INT64, False, col_range([gw], INT64, False)),
             D(INT32, False, R(True, 0, 19_999)), D(INT64, True, col_range([x], INT64, True)),
             D(INT16, False, R(True, 0, 299), capi.ENC_FIXED, INT64)]
    frags = _split(cols, FRAG_SIZES)

    KEY = TargetExpr(PROJECT_KEY)
    FULL = [KEY, TargetExpr(COUNT), TargetExpr(COUNT, D_X, 1), TargetExpr(SUM, D_W, 1), TargetExpr(MIN, D_X, 1), TargetExpr(MAX, D_X, 1),
            TargetExpr(AVG, D_FD, 1), TargetExpr(SUM, V)]
    out: List[ExpandCase] = []

    # the same table with a key column that never matches: every key below the dimension's range, or NULL
    k_miss = np.where(k == NULLS[INT64], k, -1 - (np.abs(k) % 50)).astype(np.int64)
    miss_descs = [D(INT64, True, col_range([k_miss], INT64, True))] + descs[1:]
    miss_frags = _split([k_miss] + cols[1:], FRAG_SIZES)

    def add(name, targets, group, quals=(), outer_col=K, kind=capi.JOIN_INNER, keyed=False, guess=16384, exprs=(), opts=None, passes=1,
            nothing_joins=False):
        ra = RelAlgExecutionUnit(list(miss_descs if nothing_joins else descs), list(targets), list(quals), list(group),
                                 inner_col_descs=list(inner_descs), join_outer_col=outer_col, join_kind=kind,
                                 max_groups_buffer_entry_guess=guess, exprs=list(exprs))
        out.append(ExpandCase(Case(name, ra, miss_frags if nothing_joins else frags, list(inner), dk, INT64, join_rng, keyed, join_one_to_many=2),
                              dict(opts or {}), passes, nothing_joins))

    # 1. INNER and LEFT x perfect and keyed tables, every kind of target
    for kind, ktag in [(capi.JOIN_INNER, "inner"), (capi.JOIN_LEFT, "left")]:
        for keyed, ttag in [(False, "perfect"), (True, "keyed")]:
            add(f"expand_{ktag}_{ttag}_all_targets", FULL, [G], kind=kind, keyed=keyed)
    # 2. a nullable INT32 join key (decode_int path: no quads)
    add("expand_inner_perfect_nullable_int32_key", FULL, [G], outer_col=K32)
    add("expand_left_keyed_nullable_int32_key", FULL, [G], outer_col=K32, kind=capi.JOIN_LEFT, keyed=True)
    # 3. two group columns
    add("expand_left_perfect_two_group_columns",
        [TargetExpr(PROJECT_KEY, 0), TargetExpr(PROJECT_KEY, 1), TargetExpr(COUNT), TargetExpr(SUM, D_W, 1), TargetExpr(AVG, D_FD, 1),
         TargetExpr(MAX, D_X, 1)], [G, G2], kind=capi.JOIN_LEFT)
    # 4. a baseline layout (a wide BIGINT key) and a perfect layout of 20 000 groups
    add("expand_inner_keyed_baseline_wide_key", [KEY, TargetExpr(COUNT), TargetExpr(SUM, D_W, 1), TargetExpr(MIN, D_X, 1), TargetExpr(SUM, V)],
        [GW], keyed=True, guess=65536)
    add("expand_left_perfect_20000_groups", [KEY, TargetExpr(COUNT), TargetExpr(COUNT, D_X, 1), TargetExpr(SUM, D_W, 1), TargetExpr(AVG, D_FD, 1)],
        [G20K], kind=capi.JOIN_LEFT)
    # 5. quals on outer columns; x IS NOT NULL on an aggregated column changes the layout (constrained_not_null)
    add("expand_inner_perfect_quals_not_null_aggregate",
        [KEY, TargetExpr(COUNT), TargetExpr(SUM, X), TargetExpr(MIN, X), TargetExpr(SUM, D_W, 1), TargetExpr(AVG, D_FD, 1)], [G],
        quals=[Qual(X, capi.IS_NOT_NULL), Qual(V, capi.GT, -500_000), Qual(G2, capi.LT, 8)])
    add("expand_left_keyed_quals", FULL, [G], quals=[Qual(V, capi.LE, 250_000), Qual(G, capi.GE, 20)], kind=capi.JOIN_LEFT, keyed=True)
    # 6. conditional aggregates
    add("expand_left_perfect_count_if_sum_if",
        [KEY, TargetExpr(COUNT_IF, cond=Qual(V, capi.GT, 0)), TargetExpr(SUM_IF, V, cond=Qual(X, capi.LT, 100)), TargetExpr(SUM, D_W, 1),
         TargetExpr(COUNT)], [G], kind=capi.JOIN_LEFT)
    # 7. a kENCODING_FIXED group key (INT16 chunks of a BIGINT column): copied as stored
    add("expand_inner_keyed_fixed_encoded_group_key", [KEY, TargetExpr(COUNT), TargetExpr(SUM, D_W, 1), TargetExpr(MAX, D_X, 1), TargetExpr(SUM, V)],
        [GFX], keyed=True)
    # 8. three passes: pass_rows = derived rows per pass (the fragments are never split)
    add("expand_left_perfect_three_passes", FULL, [G], kind=capi.JOIN_LEFT, passes=3)
    rows2 = joined_rows_per_fragment(out[-1])
    out[-1].opts["pass_rows"] = max(rows2) + rows2[0] + rows2[3]   # the three large fragments never share a pass
    assert passes_of(rows2, out[-1].opts["pass_rows"]) == 3, rows2
    # 9. an INNER join in which nothing matches (every key misses): the initialised layout comes back
    add("expand_inner_perfect_nothing_matches", [KEY, TargetExpr(COUNT), TargetExpr(SUM, D_W, 1), TargetExpr(AVG, D_FD, 1)], [G], nothing_joins=True)
    # 10. an expression target: lowered by k_project, then expanded (k_project > k_join_expand > ...)
    add("expand_inner_perfect_expression_target",
        [KEY, TargetExpr(COUNT), TargetExpr(SUM, N_PHYS), TargetExpr(SUM, D_W, 1)], [G], exprs=[Expr.col(V).add(Expr.lit(INT64, 5), INT64)])
    return out


def passes_of(rows2: List[int], pass_rows: int) -> int:
    """the pass loop's cut: a pass holds at least one fragment; the next one joins while the pass stays within pass_rows"""
    pass_rows = max(pass_rows, max(rows2))
    passes, held = 0, None
    for r in rows2:
        if held is None or held + r > pass_rows:
            passes, held = passes + 1, r
        else:
            held += r
    return passes


def joined_rows_per_fragment(ec: ExpandCase) -> List[int]:
    """numpy restatement of the count: joined rows of every outer fragment"""
    c = ec.case
    col = c.ra.join_outer_col
    cnt = np.bincount(c.join_keys, minlength=N_KEYS)
    left = c.ra.join_kind == capi.JOIN_LEFT
    out = []
    for cols in c.frags:
        kk = cols[col].astype(np.int64)
        null = kk == NULLS[c.ra.input_col_descs[col].type]
        inside = (~null) & (kk >= 0) & (kk < N_KEYS)
        per = np.where(inside, cnt[np.clip(kk, 0, N_KEYS - 1)], 0)
        if left:
            per = np.maximum(per, 1)
        out.append(int(per.sum()))
    return out
