"""Star joins: a join step whose WHERE and GROUP BY name columns of the DIMENSION (capi.INNER_COL / executor.inner), shared by the
host-simulation tests (tests/test_star_join.py) and the device tests (tests/test_zz_gpu_star_join.py):

    SELECT d.region, COUNT(*), SUM(f.amount) FROM fact f JOIN dim d ON f.did = d.id WHERE d.segment BETWEEN 2 AND 5 GROUP BY d.region

The oracle cannot state an inner reference.  The references are (1) the oracle on the FLATTENED plan `flatten()` builds here
with numpy alone — the join done with searchsorted, the inner columns gathered into outer columns (NULL sentinels for the
unmatched rows a LEFT join keeps), an INT32 `matched` column and the qual `matched = 1` for INNER joins, np.repeat for a
one-to-many table — and (2) SQLite on the query text itself (StarCase.sql: tables f(c0 ..) and d(k0, i0 ..)).  Nothing here calls the library's own rewrite.

The fact table has 50 000 rows in fragments [1, 16384, 16385, 5, rest] (a tile is 16 384 rows, a lane's quad four: a one-row
fragment, exactly one tile, a tile boundary one row into a fragment, a partial quad, several tiles with a ragged end); the
dimension has 1 000 rows whose keys leave holes inside [100, 1399]; fact keys miss below and above that range and 3 % of the
nullable key column is NULL."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import AVG, COUNT, DOUBLE, INT8, INT32, INT64, MAX, MIN, PROJECT_KEY, SUM
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr, inner
from tests.cases import NP, NULLS, Case, col_range

N_ROWS = 50_000
FRAG_SIZES = [1, 16384, 16385, 5, N_ROWS - 32775]
N_DIM = 1000
KEY_MIN, KEY_MAX = 100, 1399
STAR_NOTE = "k_join_group_code + k_star_groupby_lds"
FLAT_NOTE = "inner columns flattened: "
# outer columns
DID, DID32, AMT, V32, FD, Q = range(6)
# inner columns
D_REGION, D_R300, D_SEG, D_NATT, D_F, D_N8, D_OOR, D_OOR2 = range(8)   # (the key column d.id is the join table's)


@dataclass
class StarCase:
    case: Case                       # the stated plan (inner references) and its tables
    star: bool                       # the star member's shape: default and kernel_variant 2 take it, the flag leaves it
    flat_kernel: str                 # the pre-pass the flattened route names: "k_join_gather" / "k_join_expand"
    sql: Optional[str] = None        # the query text for SQLite (tables f(c0..), d(k0, i0..)), where one is compared
    unaligned: bool = False          # the fact chunks sit 4 bytes off a 16-byte boundary
    empty: bool = False              # no row passes

    @property
    def name(self):
        return self.case.name


def _split(cols, sizes):
    out, at = [], 0
    for s in sizes:
        out.append([c[at:at + s] for c in cols])
        at += s
    assert at == len(cols[0])
    return out


def build_cases() -> List[StarCase]:
    rng = np.random.default_rng(777)
    D, R = InputColDescriptor, ExpressionRange
    n, m = N_ROWS, N_DIM
    # ---- the dimension: 1 000 of the 1 300 keys of [100, 1399], shuffled; the range's ends are present
    keys = np.sort(rng.choice(np.arange(KEY_MIN + 1, KEY_MAX), m - 2, replace=False))
    keys = np.concatenate([[KEY_MIN], keys, [KEY_MAX]]).astype(np.int64)
    rng.shuffle(keys)
    lonely = int(keys[17])           # a dimension row no fact row matches
    d_region = rng.integers(0, 7, m).astype(np.int32)
    d_r300 = rng.integers(0, 300, m).astype(np.int32)
    d_seg = rng.integers(0, 10, m).astype(np.int32)
    d_seg[rng.random(m) < 0.1] = NULLS[INT32]
    d_natt = rng.integers(0, 4, m).astype(np.int32)
    d_natt[rng.random(m) < 0.15] = NULLS[INT32]
    d_n8 = rng.integers(0, 5, m).astype(np.int8)      # a TINYINT attribute: not the star member's key type
    d_n8[rng.random(m) < 0.1] = NULLS[INT8]
    d_f = np.round(rng.random(m) * 50) / 4            # a DOUBLE attribute with a few dozen distinct values
    d_oor = d_region.copy()
    d_oor[33] = 9                    # outside its declared range [0, 6], on a row fact rows match
    d_oor2 = d_region.copy()
    d_oor2[17] = 9                   # ... on the row nothing matches
    inner_cols = [d_region, d_r300, d_seg, d_natt, d_f, d_n8, d_oor, d_oor2]
    inner_descs = [D(INT32, False, R(True, 0, 6)), D(INT32, False, R(True, 0, 299)),
                   D(INT32, True, R(True, 0, 9, True)), D(INT32, True, R(True, 0, 3, True)), D(DOUBLE, False, col_range([d_f], DOUBLE, False)),
                   D(INT8, True, R(True, 0, 4, True)), D(INT32, False, R(True, 0, 6)), D(INT32, False, R(True, 0, 6))]
    join_rng = R(True, KEY_MIN, KEY_MAX)
    # ---- the fact table
    did = rng.integers(KEY_MIN - 40, KEY_MAX + 41, n).astype(np.int64)
    did[did == lonely] = int(keys[33])
    did[rng.random(n) < 0.03] = NULLS[INT64]
    did32 = rng.integers(KEY_MIN - 40, KEY_MAX + 41, n).astype(np.int32)
    did32[did32 == lonely] = int(keys[33])
    assert (did == keys[33]).sum() > 0 and (did32 == keys[33]).sum() > 0 and (did < KEY_MIN).sum() > 500 and (did > KEY_MAX).sum() > 500
    amt = rng.integers(-10**6, 10**6, n).astype(np.int64)
    v32 = rng.integers(-1000, 1000, n).astype(np.int32)
    fd = rng.random(n) * 100 - 50
    q = rng.integers(0, 100, n).astype(np.int32)
    cols = [did, did32, amt, v32, fd, q]
    descs = [D(INT64, True, col_range([did], INT64, True)), D(INT32, False, col_range([did32], INT32, False)),
             D(INT64, False, col_range([amt], INT64, False)), D(INT32, False, col_range([v32], INT32, False)),
             D(DOUBLE, False, col_range([fd], DOUBLE, False)), D(INT32, False, R(True, 0, 99))]
    frags = _split(cols, FRAG_SIZES)
    # ---- a one-to-many dimension: every key of the first 400 rows twice more, with other attributes
    dup = np.arange(400)
    many_rows = np.concatenate([np.arange(m), dup, dup[::2]])
    rng.shuffle(many_rows)
    many_cols = [c[many_rows].copy() for c in inner_cols]
    many_keys = keys[many_rows].copy()
    many_cols[D_REGION] = rng.integers(0, 7, len(many_rows)).astype(np.int32)

    KEY = TargetExpr(PROJECT_KEY)
    out: List[StarCase] = []

    def add(name, group, targets, quals=(), kind=capi.JOIN_INNER, key=DID, star=True, keyed=False, many=False, sql=None, error=None,
            unaligned=False, empty=False):
        ra = RelAlgExecutionUnit(list(descs), list(targets), list(quals), [inner(g) for g in group], inner_col_descs=list(inner_descs),
                                 join_outer_col=key, join_kind=kind)
        inn = many_cols if many else inner_cols
        case = Case(name, ra, frags, list(inn), many_keys if many else keys, INT64, join_rng, keyed, join_one_to_many=2 if many else 0, expect_error=error)
        out.append(StarCase(case, star, "k_join_expand" if many else "k_join_gather", sql, unaligned, empty))

    BETWEEN = [Qual(inner(D_SEG), capi.GE, 2), Qual(inner(D_SEG), capi.LE, 5)]
    # 1. the query the feature exists for
    add("star_inner_region_count_sum_where_segment_between", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], BETWEEN,
        sql="SELECT d.i0, COUNT(*), SUM(f.c2) FROM f JOIN d ON f.c0 = d.k0 WHERE d.i2 BETWEEN 2 AND 5 GROUP BY d.i0")
    # 2. LEFT, 7 groups (+ the NULL group of the unmatched rows), three value columns of the three types, AVG / MIN / MAX
    add("star_left_region_three_value_columns", [D_REGION],
        [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(AVG, FD), TargetExpr(MIN, V32), TargetExpr(MAX, V32), TargetExpr(MAX, FD)],
        kind=capi.JOIN_LEFT,
        sql="SELECT d.i0, COUNT(*), SUM(f.c2), AVG(f.c4), MIN(f.c3), MAX(f.c3), MAX(f.c4) FROM f LEFT JOIN d ON f.c0 = d.k0 GROUP BY d.i0")
    # 3. 300 groups: several replicas; an INT32 NOT NULL join key
    add("star_inner_300_groups_int32_key", [D_R300], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(MAX, FD), TargetExpr(AVG, V32)],
        key=DID32)
    add("star_left_300_groups", [D_R300], [KEY, TargetExpr(COUNT), TargetExpr(MIN, AMT), TargetExpr(SUM, FD)], kind=capi.JOIN_LEFT)
    # 4. two and three inner keys, one of them nullable with NULL attributes
    add("star_left_two_keys_one_nullable", [D_REGION, D_NATT],
        [TargetExpr(PROJECT_KEY, 0), TargetExpr(PROJECT_KEY, 1), TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(AVG, FD)], kind=capi.JOIN_LEFT,
        sql="SELECT d.i0, d.i3, COUNT(*), SUM(f.c2), AVG(f.c4) FROM f LEFT JOIN d ON f.c0 = d.k0 GROUP BY d.i0, d.i3")
    add("star_inner_three_keys", [D_REGION, D_SEG, D_NATT],
        [TargetExpr(PROJECT_KEY, 0), TargetExpr(PROJECT_KEY, 1), TargetExpr(PROJECT_KEY, 2), TargetExpr(COUNT), TargetExpr(MAX, AMT)])
    # 5. COUNT(*) alone
    add("star_inner_count_only", [D_REGION], [TargetExpr(COUNT)])
    add("star_left_key_and_count", [D_SEG], [KEY, TargetExpr(COUNT)], kind=capi.JOIN_LEFT)
    # ... and a KEYED layout: no slot tells a touched entry from an untouched one (SUMs whose ranges span 0)
    add("star_left_keyed_layout_sums_only", [D_REGION, D_NATT], [TargetExpr(PROJECT_KEY, 1), TargetExpr(SUM, AMT), TargetExpr(SUM, FD)],
        kind=capi.JOIN_LEFT)
    add("star_inner_keyed_layout_sum_only", [D_R300], [KEY, TargetExpr(SUM, V32)], [Qual(inner(D_SEG), capi.NE, 0)])
    # 6. the inner quals: =, IS NULL, IS NOT NULL, one that rejects every row
    add("star_inner_qual_eq", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, V32)], [Qual(inner(D_SEG), capi.EQ, 3)],
        sql="SELECT d.i0, COUNT(*), SUM(f.c3) FROM f JOIN d ON f.c0 = d.k0 WHERE d.i2 = 3 GROUP BY d.i0")
    add("star_inner_qual_is_null", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], [Qual(inner(D_SEG), capi.IS_NULL)])
    add("star_inner_qual_is_not_null", [D_SEG], [KEY, TargetExpr(COUNT), TargetExpr(MIN, FD)], [Qual(inner(D_SEG), capi.IS_NOT_NULL)])
    add("star_inner_qual_rejects_every_row", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], [Qual(inner(D_REGION), capi.GT, 100)],
        empty=True)
    # 7. LEFT: d.attr IS NULL keeps exactly the unmatched rows, d.attr = k drops them
    add("star_left_qual_is_null_keeps_unmatched", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)],
        [Qual(inner(D_REGION), capi.IS_NULL)], kind=capi.JOIN_LEFT,
        sql="SELECT d.i0, COUNT(*), SUM(f.c2) FROM f LEFT JOIN d ON f.c0 = d.k0 WHERE d.i0 IS NULL GROUP BY d.i0")
    add("star_left_qual_eq_drops_unmatched", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)],
        [Qual(inner(D_SEG), capi.EQ, 4)], kind=capi.JOIN_LEFT,
        sql="SELECT d.i0, COUNT(*), SUM(f.c2) FROM f LEFT JOIN d ON f.c0 = d.k0 WHERE d.i2 = 4 GROUP BY d.i0")
    # 8. an outer qual together with an inner qual
    add("star_inner_outer_and_inner_qual", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(AVG, FD)],
        [Qual(Q, capi.LT, 50), Qual(inner(D_SEG), capi.GE, 2), Qual(AMT, capi.GT, -900_000)],
        sql="SELECT d.i0, COUNT(*), SUM(f.c2), AVG(f.c4) FROM f JOIN d ON f.c0 = d.k0 WHERE f.c5 < 50 AND d.i2 >= 2 AND f.c2 > -900000 "
            "GROUP BY d.i0")
    # 9. an attribute outside its declared range: an error where a fact row reaches it, none where nothing does
    add("star_inner_attribute_out_of_range_matched", [D_OOR], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], error=capi.ERR_OUT_OF_SLOTS)
    add("star_left_attribute_out_of_range_unmatched", [D_OOR2], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], kind=capi.JOIN_LEFT)
    # ---- the flattened route alone
    add("flat_inner_unaligned_fragments", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], BETWEEN, star=False, unaligned=True)
    add("flat_left_keyed_table", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(MAX, D_F, 1)], BETWEEN,
        kind=capi.JOIN_LEFT, star=False, keyed=True)
    add("flat_inner_one_to_many_table", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], [Qual(inner(D_SEG), capi.LT, 7)],
        star=False, many=True)
    add("flat_left_one_to_many_table", [D_REGION, D_NATT],
        [TargetExpr(PROJECT_KEY, 0), TargetExpr(PROJECT_KEY, 1), TargetExpr(COUNT), TargetExpr(SUM, AMT)], kind=capi.JOIN_LEFT, star=False, many=True)
    add("flat_inner_non_grouped_sum", [], [TargetExpr(SUM, AMT), TargetExpr(COUNT)], [Qual(inner(D_SEG), capi.LT, 5)], star=False,
        sql="SELECT SUM(f.c2), COUNT(*) FROM f JOIN d ON f.c0 = d.k0 WHERE d.i2 < 5")
    add("flat_left_baseline_double_key", [D_F], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], kind=capi.JOIN_LEFT, star=False)
    add("flat_inner_baseline_double_key_inner_qual", [D_F], [KEY, TargetExpr(COUNT), TargetExpr(MIN, V32)], [Qual(inner(D_REGION), capi.NE, 2)],
        star=False)
    # a TINYINT attribute as a key (not the star member's), and as a qual column beside a star-shaped key (the member's)
    add("flat_left_tinyint_key", [D_REGION, D_N8], [TargetExpr(PROJECT_KEY, 0), TargetExpr(PROJECT_KEY, 1), TargetExpr(COUNT), TargetExpr(SUM, AMT)],
        kind=capi.JOIN_LEFT, star=False)
    add("star_inner_tinyint_qual", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], [Qual(inner(D_N8), capi.LE, 2)])
    add("flat_inner_or_group_of_inner_quals", [D_REGION], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)],
        [Qual(inner(D_SEG), capi.EQ, 1, or_group=1), Qual(inner(D_NATT), capi.IS_NULL, or_group=1), Qual(Q, capi.GE, 10)], star=False,
        sql="SELECT d.i0, COUNT(*), SUM(f.c2) FROM f JOIN d ON f.c0 = d.k0 WHERE (d.i2 = 1 OR d.i3 IS NULL) AND f.c5 >= 10 GROUP BY d.i0")
    return out


def _match(case: Case, fk: np.ndarray):
    """the join in numpy: per fact row the dimension rows it matches (lo, hi into `order`)"""
    jk = np.asarray(case.join_keys)
    order = np.argsort(jk, kind="stable")
    sk = jk[order]
    null = fk == NULLS[case.ra.input_col_descs[case.ra.join_outer_col].type]
    fk = fk.astype(np.int64)
    lo = np.searchsorted(sk, fk, "left")
    hi = np.searchsorted(sk, fk, "right")
    hi = np.where(null, lo, hi)
    return order, lo, hi


def flatten(sc: StarCase) -> Case:
    """the joinless plan over the joined rows, and those rows"""
    case, ra = sc.case, sc.case.ra
    left = ra.join_kind == capi.JOIN_LEFT
    nc = len(ra.input_col_descs)
    new_of = {}          # inner column -> outer column of the flattened plan

    def outer_of(c):
        if c not in new_of:
            new_of[c] = nc + len(new_of)
        return new_of[c]

    targets = [TargetExpr(t.agg, outer_of(t.col), 0) if t.table and t.agg != PROJECT_KEY else TargetExpr(t.agg, t.col, 0) for t in ra.target_exprs]
    quals = [Qual(outer_of(capi.INNER_COL_INDEX(q.col)), q.op, q.literal, q.or_group) if capi.IS_INNER_COL(q.col) else q for q in ra.simple_quals]
    group = [outer_of(capi.INNER_COL_INDEX(g)) if capi.IS_INNER_COL(g) else g for g in ra.groupby_exprs]
    descs = list(ra.input_col_descs)
    for c in new_of:     # (insertion order = column order)
        d = ra.inner_col_descs[c]
        r = d.range
        if left:
            r = ExpressionRange(r.valid, r.min, r.max, True, r.fp_min, r.fp_max, r.bucket)
        descs.append(InputColDescriptor(d.type, d.nullable or left, r, d.encoding, d.logical_type))
    if not left:
        descs.append(InputColDescriptor(INT32, False, ExpressionRange(True, 0, 1)))
        quals.append(Qual(len(descs) - 1, capi.EQ, 1))
    frags = []
    for cols in case.frags:
        order, lo, hi = _match(case, cols[ra.join_outer_col])
        cnt = hi - lo
        per = np.maximum(cnt, 1)              # an unmatched row stays once: NULLs under LEFT, matched = 0 under INNER
        rep = np.repeat(np.arange(len(cnt)), per)
        first = np.cumsum(per) - per
        within = np.arange(len(rep)) - first[rep]
        matched = cnt[rep] > 0
        rowid = order[np.minimum(lo[rep] + within, len(order) - 1)] if len(order) else np.zeros(len(rep), np.int64)
        new_cols = [c[rep] for c in cols]
        for c in new_of:
            t = ra.inner_col_descs[c].type
            new_cols.append(np.where(matched, case.inner[c][rowid], NP[t](NULLS[t])).astype(NP[t]))
        if not left:
            new_cols.append(matched.astype(np.int32))
        frags.append(new_cols)
    ra2 = RelAlgExecutionUnit(descs, targets, quals, group, max_groups_buffer_entry_guess=ra.max_groups_buffer_entry_guess,
                              bigint_count=ra.bigint_count, output_columnar_hint=ra.output_columnar_hint, num_tuples=ra.num_tuples)
    return Case(case.name + "_flattened", ra2, frags, expect_error=case.expect_error, fp_rtol=case.fp_rtol)


# ------------------------------------------------------------------------------- the checks both test files run
def sql_rows(sc: StarCase):
    """SQLite's answer to the query text: rows as tuples (None = NULL)"""
    from tests.test_sqlite_semantics import _load
    return _load(sc.case).execute(sc.sql).fetchall()


def result_rows(q, fetched):
    iv, dv, nu = fetched
    return [tuple(None if nu[r, t] else (float(dv[r, t]) if q.target_is_fp[t] else int(iv[r, t])) for t in range(q.n_targets))
            for r in range(iv.shape[0])]


def rows_agree_with_sqlite(sc: StarCase, q, fetched, rtol=1e-9):
    import math
    from tests.test_sqlite_semantics import _key
    fp = [bool(q.target_is_fp[t]) for t in range(q.n_targets)]
    want = sorted((tuple(float(v) if f and v is not None else v for v, f in zip(r, fp)) for r in sql_rows(sc)), key=_key)
    got = sorted(result_rows(q, fetched), key=_key)
    assert len(want) == len(got), (sc.sql, len(want), len(got))
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            if a is None or b is None:
                assert a is None and b is None, (sc.sql, w, g)
            elif isinstance(a, float) or isinstance(b, float):
                assert math.isclose(float(a), float(b), rel_tol=rtol, abs_tol=1e-9), (sc.sql, w, g)
            else:
                assert a == b, (sc.sql, w, g)


def oracle_reference(oracle, sc: StarCase):
    """(descriptor, buffer, code) of the oracle on the flattened plan; computed once per case"""
    if getattr(sc, "_ref", None) is None:
        flat = flatten(sc)
        sc._ref = oracle.execute(flat.ra.to_plan(), flat.frags, [], None, n_threads=2)
    return sc._ref


def variants(sc: StarCase):
    """(id, options, the star member runs): every star-shaped case three ways, the others two"""
    if sc.star:
        return [("default", {}, True), ("no_star_flag", {"flags": capi.OPT_NO_STAR_GROUPBY}, False), ("variant2", {"kernel_variant": 2}, True)]
    return [("default", {}, False), ("variant2", {"kernel_variant": 2}, False)]


def check_route(sc: StarCase, route: str, star_runs: bool):
    if star_runs:
        assert STAR_NOTE in route and FLAT_NOTE not in route, route
    else:
        assert FLAT_NOTE + sc.flat_kernel in route and STAR_NOTE not in route, route


def check_result(oracle, sc: StarCase, rs, star_runs: bool):
    """the parity bar against the oracle on the flattened plan, SQLite where the case has a query text, the report"""
    from tests.helpers import compare_buffers, compare_rows, qmd_equal
    q, want, code = oracle_reference(oracle, sc)
    assert code == 0
    qmd_equal(q, rs.getQueryMemDesc())
    compare_buffers(q, want, rs.getStorage(), sc.case.fp_rtol)
    assert rs.rowCount() == oracle.row_count(q, want)
    fetched = rs.fetch()
    compare_rows(q, oracle.fetch_rows(q, want), fetched, sc.case.fp_rtol)
    if sc.empty:
        assert rs.rowCount() == 0
    if sc.sql:
        rows_agree_with_sqlite(sc, q, fetched)
    name = rs.report.kernel_name.decode()
    if star_runs:
        assert name == "k_star_groupby_lds", name
    else:
        assert name and name != "k_star_groupby_lds", name
