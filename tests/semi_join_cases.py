"""SEMI and ANTI join levels (capi.JOIN_SEMI / JOIN_ANTI: WHERE EXISTS / NOT EXISTS), shared by the host-simulation tests
(tests/test_semi_join.py) and the device tests (tests/test_zz_gpu_semi_join.py):

    SELECT f.q, COUNT(*), SUM(f.amount) FROM fact f WHERE EXISTS (SELECT 1 FROM dim d WHERE d.id = f.did) GROUP BY f.q

The oracle cannot state these kinds.  The references are (1) the oracle on the JOINLESS plan plus a mask column that `mask_of()`
computes here with numpy alone — np.isin of the fact keys in the dimension keys, FALSE for a NULL key (any NULL component of a
composite key), inverted for ANTI — plus the qual `mask = 1`, which keeps a Projection entry's key (the row's offset in its
fragment) intact; and (2) SQLite on the query text itself (tables f(c0 ..) and d(k0 ..)).  Nothing here calls the library's own
rewrite.

The geometry is the star cases': 50 000 fact rows in fragments [1, 16384, 16385, 5, rest] (a one-row fragment, whole tiles, a
tile boundary one row into a fragment, a partial quad, several tiles with a ragged end); a 1 000-row dimension whose keys leave
holes inside [100, 1399]; fact keys that fall below and above that range; 3 % NULLs in the nullable INT64 key, a NOT NULL INT32
key as well; a one-to-many twin of the dimension (some keys two and three times); a keyed build of both; one composite
(INT64, INT64) one-to-one table."""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import AVG, COUNT, DOUBLE, INT8, INT32, INT64, MIN, PROJECT, PROJECT_KEY, SUM
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests.cases import NULLS, Case, col_range

N_ROWS = 50_000
FRAG_SIZES = [1, 16384, 16385, 5, N_ROWS - 32775]
N_DIM = 1000
KEY_MIN, KEY_MAX = 100, 1399
KINDS = [("semi", capi.JOIN_SEMI), ("anti", capi.JOIN_ANTI)]
NOTE = {capi.JOIN_SEMI: "semi join", capi.JOIN_ANTI: "anti join"}
KERNEL = "k_join_exists_mask"
# outer columns
DID, DID32, AMT, V32, FD, Q, BK, DIDF, CA, CB = range(10)


@dataclass
class Dim:
    """a dimension as mi355q_join_build sees it"""
    name: str
    keys: object                     # the key column, or a list of two for the composite table
    key_type: object = INT64
    key_range: Optional[ExpressionRange] = None
    keyed: bool = False
    many: bool = False


@dataclass
class SemiCase:
    name: str
    ra: RelAlgExecutionUnit          # the stated plan; join_kind is set per run
    dim: Dim
    sql: Optional[str] = None        # the query text for SQLite with {EXISTS} for EXISTS / NOT EXISTS, where one is compared
    unaligned: bool = False          # the fact chunks sit 4 bytes off a 16-byte boundary
    general: bool = False            # the key column is not the fast member's (the route text says which member is planned)
    small_buffer: bool = False       # a Projection into a buffer that is too small: the negative matched-row count


def _split(cols, sizes):
    out, at = [], 0
    for s in sizes:
        out.append([c[at:at + s] for c in cols])
        at += s
    assert at == len(cols[0])
    return out


def _build():
    rng = np.random.default_rng(4242)
    D, R = InputColDescriptor, ExpressionRange
    n, m = N_ROWS, N_DIM
    # ---- the dimension: 1 000 of the 1 300 keys of [100, 1399], shuffled; the range's ends are present
    keys = np.sort(rng.choice(np.arange(KEY_MIN + 1, KEY_MAX), m - 2, replace=False))
    keys = np.concatenate([[KEY_MIN], keys, [KEY_MAX]]).astype(np.int64)
    rng.shuffle(keys)
    # its one-to-many twin: the keys of the first 400 rows twice, every other one of them three times
    dup = np.arange(400)
    many_keys = keys[np.concatenate([np.arange(m), dup, dup[::2]])].copy()
    rng.shuffle(many_keys)
    join_rng = R(True, KEY_MIN, KEY_MAX)
    # the composite table: 1 000 of the 2 000 pairs of [0, 99] x [0, 19]
    pairs = rng.choice(2000, m, replace=False)
    ka, kb = (pairs // 20).astype(np.int64), (pairs % 20).astype(np.int64)
    dims = {
        "one": Dim("one", keys, INT64, join_rng),
        "many": Dim("many", many_keys, INT64, join_rng, many=True),
        "keyed_one": Dim("keyed_one", keys, INT64, join_rng, keyed=True),
        "keyed_many": Dim("keyed_many", many_keys, INT64, join_rng, keyed=True, many=True),
        "composite": Dim("composite", [ka, kb], [INT64, INT64], R(), keyed=True),
        "far": Dim("far", (keys + 5000).astype(np.int64), INT64, R(True, KEY_MIN + 5000, KEY_MAX + 5000)),   # nothing matches
        "empty": Dim("empty", np.zeros(0, np.int64), INT64, join_rng),
    }
    # ---- the fact table
    did = rng.integers(KEY_MIN - 40, KEY_MAX + 41, n).astype(np.int64)
    did[rng.random(n) < 0.03] = NULLS[INT64]
    did32 = rng.integers(KEY_MIN - 40, KEY_MAX + 41, n).astype(np.int32)
    didf = rng.integers(KEY_MIN - 40, KEY_MAX + 41, n).astype(np.int32)     # FIXED(32) storage of a BIGINT key
    didf[rng.random(n) < 0.03] = NULLS[INT32]
    amt = rng.integers(-10**6, 10**6, n).astype(np.int64)
    v32 = rng.integers(-1000, 1000, n).astype(np.int32)
    fd = rng.random(n) * 100 - 50
    q = rng.integers(0, 100, n).astype(np.int32)
    bk = (rng.integers(0, 3000, n) * 1000003 - 10**9).astype(np.int64)      # a BIGINT key without a usable range: baseline hash
    ca = rng.integers(-5, 105, n).astype(np.int64)
    ca[rng.random(n) < 0.03] = NULLS[INT64]
    cb = rng.integers(0, 20, n).astype(np.int64)
    cols = [did, did32, amt, v32, fd, q, bk, didf, ca, cb]
    descs = [D(INT64, True, col_range([did], INT64, True)), D(INT32, False, col_range([did32], INT32, False)),
             D(INT64, False, col_range([amt], INT64, False)), D(INT32, False, col_range([v32], INT32, False)),
             D(DOUBLE, False, col_range([fd], DOUBLE, False)), D(INT32, False, R(True, 0, 99)), D(INT64, False, R(False)),
             D(INT32, True, R(True, KEY_MIN - 40, KEY_MAX + 40, True), capi.ENC_FIXED, INT64),
             D(INT64, True, col_range([ca], INT64, True)), D(INT64, False, R(True, 0, 19))]
    frags = _split(cols, FRAG_SIZES)

    KEY = TargetExpr(PROJECT_KEY)
    out: List[SemiCase] = []

    def add(name, group, targets, quals=(), key=DID, dim="one", sql=None, guess=16384, limit=0, columnar=0, **kw):
        ra = RelAlgExecutionUnit(list(descs), list(targets), list(quals), list(group), join_outer_col=key, join_kind=capi.JOIN_SEMI,
                                 max_groups_buffer_entry_guess=guess, scan_limit=limit, output_columnar_hint=columnar, num_tuples=n)
        out.append(SemiCase(name, ra, dims[dim], sql, **kw))

    NG = [TargetExpr(COUNT), TargetExpr(SUM, AMT)]
    FEW = [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT), TargetExpr(AVG, FD), TargetExpr(MIN, V32)]
    TWO_QUALS = [Qual(V32, capi.LT, 500), Qual(AMT, capi.GT, -900_000)]
    ex = "{EXISTS} (SELECT 1 FROM d WHERE d.k0 = f.c0)"
    ng_sql = "SELECT COUNT(*), SUM(f.c2) FROM f WHERE " + ex
    few_sql = "SELECT f.c5, COUNT(*), SUM(f.c2), AVG(f.c4), MIN(f.c3) FROM f WHERE " + ex + " GROUP BY f.c5"
    add("non_grouped_count_sum", [], NG, sql=ng_sql)
    add("few_groups", [Q], FEW, sql=few_sql)
    add("baseline_bigint_key", [BK], [KEY, TargetExpr(COUNT), TargetExpr(SUM, AMT)], guess=8192,
        sql="SELECT f.c6, COUNT(*), SUM(f.c2) FROM f WHERE " + ex + " GROUP BY f.c6")
    add("few_groups_two_outer_quals", [Q], FEW, TWO_QUALS,
        sql="SELECT f.c5, COUNT(*), SUM(f.c2), AVG(f.c4), MIN(f.c3) FROM f WHERE f.c3 < 500 AND f.c2 > -900000 AND " + ex + " GROUP BY f.c5")
    PROJ = [TargetExpr(PROJECT, AMT), TargetExpr(PROJECT, FD), TargetExpr(PROJECT, V32)]
    add("projection_three_columns", [], PROJ, guess=N_ROWS)
    add("projection_limit_100", [], PROJ, guess=N_ROWS, limit=100)
    add("projection_buffer_too_small", [], PROJ, guess=1000, small_buffer=True)
    add("few_groups_columnar_hint", [Q], FEW, columnar=capi.OUTPUT_COLUMNAR)
    # ---- over the perfect one-to-one table
    add("int32_key", [Q], FEW, key=DID32,
        sql="SELECT f.c5, COUNT(*), SUM(f.c2), AVG(f.c4), MIN(f.c3) FROM f WHERE {EXISTS} (SELECT 1 FROM d WHERE d.k0 = f.c1) GROUP BY f.c5")
    add("fixed_encoded_key", [Q], FEW, key=DIDF, general=True)
    add("unaligned_fragments", [Q], FEW, unaligned=True)
    add("dimension_nothing_matches", [], NG, dim="far")
    add("empty_dimension", [Q], FEW, dim="empty")
    # ---- the other tables
    for dim in ("many", "keyed_one", "keyed_many"):
        add(f"{dim}_non_grouped", [], NG, dim=dim, sql=ng_sql, general=dim != "many")
        add(f"{dim}_few_groups", [Q], FEW, dim=dim, sql=few_sql if dim == "many" else None, general=dim != "many")
    cex = "{EXISTS} (SELECT 1 FROM d WHERE d.k0 = f.c8 AND d.k1 = f.c9)"
    add("composite_non_grouped", [], NG, key=[CA, CB], dim="composite", general=True, sql="SELECT COUNT(*), SUM(f.c2) FROM f WHERE " + cex)
    add("composite_few_groups", [Q], FEW, key=[CA, CB], dim="composite", general=True)
    return out, frags, dims


CASES, FRAGS, DIMS = _build()


def key_cols(sc: SemiCase):
    k = sc.ra.join_outer_col
    return list(k) if isinstance(k, (list, tuple)) else [k]


def mask_of(sc: SemiCase, cols, kind) -> np.ndarray:
    """the join level of one fragment in numpy: 1 = the row passes"""
    kc = key_cols(sc)
    null = np.zeros(len(cols[0]), bool)
    for c in kc:
        d = sc.ra.input_col_descs[c]
        if d.nullable:
            null |= cols[c] == NULLS[d.type]
    dk = sc.dim.keys if isinstance(sc.dim.keys, list) else [sc.dim.keys]
    if len(kc) == 1:
        hit = np.isin(cols[kc[0]].astype(np.int64), np.asarray(dk[0], np.int64))
    else:   # every component: the pair as one number (both components of both sides lie far inside +-10^6, NULLs aside)
        code = lambda a, b: np.where((a > -10**6) & (a < 10**6), a, 10**6) * 10**7 + b   # noqa: E731
        assert all(np.abs(np.asarray(x)).max() < 10**6 for x in dk)
        hit = np.isin(code(cols[kc[0]].astype(np.int64), cols[kc[1]].astype(np.int64)), code(dk[0], dk[1]))
    hit &= ~null
    return (hit if kind == capi.JOIN_SEMI else ~hit).astype(np.int8)


def stated(sc: SemiCase, kind) -> Case:
    """the stated plan of one run as a tests.cases.Case (what the join-table and SQLite helpers take)"""
    ra = copy.copy(sc.ra)
    ra.join_kind = kind
    multi = isinstance(sc.dim.keys, list)
    return Case(f"{sc.name}_{dict((v, k) for k, v in KINDS)[kind]}", ra, FRAGS, [], sc.dim.keys, sc.dim.key_type, sc.dim.key_range,
                sc.dim.keyed and not multi, join_one_to_many=2 if sc.dim.many else 0)


def joinless(sc: SemiCase) -> RelAlgExecutionUnit:
    ra = copy.copy(sc.ra)
    ra.join_outer_col = -1
    ra.join_kind = capi.JOIN_INNER
    ra.join_table = None
    return ra


def reference_case(sc: SemiCase, kind) -> Case:
    """the joinless plan + the mask column + `mask = 1`, and its fragments"""
    ra = joinless(sc)
    nc = len(ra.input_col_descs)
    ra.input_col_descs = list(ra.input_col_descs) + [InputColDescriptor(INT8, False, ExpressionRange(True, 0, 1))]
    ra.simple_quals = list(ra.simple_quals) + [Qual(nc, capi.EQ, 1)]
    frags = [list(cols) + [mask_of(sc, cols, kind)] for cols in FRAGS]
    return Case(sc.name + "_masked", ra, frags)


_REFS = {}


def oracle_reference(oracle, sc: SemiCase, kind):
    """(descriptor, buffer, code) of the oracle on the masked joinless plan; computed once per case and kind"""
    if (sc.name, kind) not in _REFS:
        ref = reference_case(sc, kind)
        _REFS[(sc.name, kind)] = oracle.execute(ref.ra.to_plan(), ref.frags, [], None, n_threads=2)
    return _REFS[(sc.name, kind)]


def passing_rows(sc: SemiCase, kind) -> int:
    """rows that pass the join level and the plain quals (numpy)"""
    total = 0
    for cols in FRAGS:
        ok = mask_of(sc, cols, kind) == 1
        for ql in sc.ra.simple_quals:
            v = cols[ql.col]
            ok &= {capi.LT: v < ql.literal, capi.GT: v > ql.literal}[ql.op]
        total += int(ok.sum())
    return total


_DBS = {}


def sql_rows(sc: SemiCase, kind):
    """SQLite's answer to the query text: rows as tuples (None = NULL)"""
    from tests.test_sqlite_semantics import _load
    if sc.dim.name not in _DBS:
        db = _load(stated(sc, kind))
        db.execute("CREATE INDEX d_keys ON d (" + ", ".join(f"k{i}" for i in range(len(key_cols(sc)))) + ")")
        _DBS[sc.dim.name] = db
    return _DBS[sc.dim.name].execute(sc.sql.replace("{EXISTS}", "EXISTS" if kind == capi.JOIN_SEMI else "NOT EXISTS")).fetchall()


def rows_agree_with_sqlite(sc: SemiCase, kind, q, fetched, rtol=1e-9):
    import math
    from tests.star_join_cases import result_rows
    from tests.test_sqlite_semantics import _key
    fp = [bool(q.target_is_fp[t]) for t in range(q.n_targets)]
    want = sorted((tuple(float(v) if f and v is not None else v for v, f in zip(r, fp)) for r in sql_rows(sc, kind)), key=_key)
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


def check_result(oracle, sc: SemiCase, kind, rs):
    """the parity bar against the oracle on the masked joinless plan, SQLite where the case has a query text"""
    from tests.helpers import compare_buffers, compare_rows, qmd_equal
    q, want, code = oracle_reference(oracle, sc, kind)
    assert code == 0
    qmd_equal(q, rs.getQueryMemDesc())
    got = rs.getStorage()
    if q.output_columnar:
        from tests.helpers import columnar_to_rows, rowwise_qmd
        assert got.nbytes == want.nbytes == oracle.buffer_bytes(q)
        compare_buffers(rowwise_qmd(q), columnar_to_rows(q, want), columnar_to_rows(q, got), 1e-9)
    else:
        compare_buffers(q, want, got, 0.0 if q.desc_type == capi.PROJECTION else 1e-9)
    assert rs.rowCount() == oracle.row_count(q, want)
    fetched = rs.fetch()
    compare_rows(q, oracle.fetch_rows(q, want), fetched, 1e-9)
    if sc.sql:
        rows_agree_with_sqlite(sc, kind, q, fetched)


def variants():
    return [("default", {}), ("variant2", {"kernel_variant": 2})]


# ---- no case can pass by keeping everything or nothing: for each table the SEMI set and the ANTI set hold more than 500 rows,
# and some row falls below the key range, above it and into a hole
def _self_check():
    every = [np.concatenate([cols[c] for cols in FRAGS]) for c in range(len(FRAGS[0]))]
    seen = set()
    for sc in CASES:
        tag = (sc.dim.name, tuple(key_cols(sc)))
        if sc.dim.name in ("far", "empty") or tag in seen:
            continue
        seen.add(tag)
        semi = mask_of(sc, every, capi.JOIN_SEMI)
        anti = mask_of(sc, every, capi.JOIN_ANTI)
        assert (semi + anti == 1).all() and semi.sum() > 500 and anti.sum() > 500, (tag, semi.sum(), anti.sum())
        k = every[key_cols(sc)[0]].astype(np.int64)
        d = sc.ra.input_col_descs[key_cols(sc)[0]]
        live = ~(k == NULLS[d.type]) if d.nullable else np.ones(len(k), bool)
        dk = np.asarray(sc.dim.keys[0] if isinstance(sc.dim.keys, list) else sc.dim.keys, np.int64)
        assert (live & (k < dk.min())).any() and (live & (k > dk.max())).any(), tag
        assert (live & (k > dk.min()) & (k < dk.max()) & (semi == 0)).any(), tag
        if d.nullable:
            assert (~live).sum() > 500 and (semi[~live] == 0).all() and (anti[~live] == 1).all(), tag
    far = next(sc for sc in CASES if sc.dim.name == "far")
    assert mask_of(far, every, capi.JOIN_SEMI).sum() == 0


_self_check()
