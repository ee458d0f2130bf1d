"""The NDV estimate (mi355q_estimate_ndv, k_ndv_hll) and the join tables sized by it: the cases and the reference, shared
by tests/test_ndv.py (both host simulations) and tests/test_zz_gpu_ndv.py (the device).

The reference is a numpy restatement of the specification in include/mi355q.h (the reference's
approximate_distinct_tuples_impl and HyperLogLog.h): vectorised uint64 arithmetic for the hash, the registers and the
estimate.  It is never the library, and it is a restatement, not vectors the reference executed."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from heavydb_amd import capi
from heavydb_amd.capi import COUNT, INT8, INT16, INT32, INT64, SUM
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit, TargetExpr
from tests.cases import NP, NULLS, Case, col_range, split
from tests.proj_cases import ProjCase

U = np.uint64
MUL = 0xc6a4a7935bd1e995
ROT = 47
MASK = (1 << 64) - 1
SPLIT = [1, 16384, 16385, 5]   # the project's usual fragment split (a full tile of the kernel is 2048 rows), then the rest


# ---------------------------------------------------------------------------------------------------- the restatement
def key_words(cols: List[np.ndarray]):
    """(width, [n, n_keys] uint64 of the sign-extended components cut to `width` bytes)"""
    width = 8 if any(c.dtype.itemsize > 4 for c in cols) else 4
    comp = [c.astype(np.int64).view(U) & U(MASK if width == 8 else 0xFFFFFFFF) for c in cols]
    return width, np.stack(comp, axis=1) if len(cols[0]) else np.zeros((0, len(cols)), U)


def murmur64a(cols: List[np.ndarray]) -> np.ndarray:
    """MurmurHash64A, seed 0, of every row's key bytes"""
    width, w = key_words(cols)
    n, nk = w.shape
    m, r = U(MUL), U(ROT)
    h = np.full(n, (nk * width * MUL) & MASK, U)
    blocks = [w[:, i] for i in range(nk)] if width == 8 else [w[:, 2 * i] | (w[:, 2 * i + 1] << U(32)) for i in range(nk // 2)]
    for k in blocks:
        k = k * m
        k = k ^ (k >> r)
        k = k * m
        h = (h ^ k) * m
    if width == 4 and nk % 2:
        h = (h ^ w[:, nk - 1]) * m
    h = h ^ (h >> r)
    h = h * m
    return h ^ (h >> r)


def clz64(x: np.ndarray) -> np.ndarray:
    zero = x == 0
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> U(64 - s)) == 0
        n += np.where(top_clear, s, 0)
        x = np.where(top_clear, x << U(s), x)
    return np.where(zero, 64, n)


def live_rows(cols: List[np.ndarray], types, nullables) -> np.ndarray:
    ok = np.ones(len(cols[0]), bool)
    for c, t, nl in zip(cols, types, nullables):
        if nl:
            ok &= c != NP[t](NULLS[t])
    return ok


def registers(frags: List[List[np.ndarray]], types, nullables, bits: int) -> np.ndarray:
    b = bits or 11
    regs = np.zeros(1 << b, np.uint32)
    for cols in frags:
        ok = live_rows(cols, types, nullables)
        h = murmur64a([c[ok] for c in cols])
        idx = (h >> U(64 - b)).astype(np.int64)
        rank = np.minimum(64 - b, clz64(h << U(b))) + 1
        np.maximum.at(regs, idx, rank.astype(np.uint32))
    return regs


def estimate(regs: np.ndarray) -> int:
    m = len(regs)
    alpha = {16: 0.673, 32: 0.697, 64: 0.709}.get(m, 0.7213 / (1 + 1.079 / m))
    e = alpha * m * m / float(np.sum(np.ldexp(1.0, -regs.astype(np.int64))))
    z = int(np.count_nonzero(regs == 0))
    if e <= 2.5 * m and z > 0:
        e = m * math.log(m / z)
    return int(e)


def exact_distinct(frags, types, nullables) -> int:
    rows = []
    for cols in frags:
        ok = live_rows(cols, types, nullables)
        rows.append(np.stack([c[ok].astype(np.int64) for c in cols], axis=1))
    return len(np.unique(np.concatenate(rows), axis=0))


def unmix_block(hash_: int) -> int:
    """the ONE 8-byte key whose MurmurHash64A is hash_: for a single block every step is an xor-shift by 47 (its own
    inverse, 2 x 47 > 64) or a multiplication by an odd constant"""
    inv = pow(MUL, -1, 1 << 64)
    h = hash_
    h ^= h >> ROT
    h = (h * inv) & MASK
    h ^= h >> ROT
    h = (h * inv) & MASK            # = h0 ^ k'
    k = h ^ ((8 * MUL) & MASK)
    k = (k * inv) & MASK
    k ^= k >> ROT
    return (k * inv) & MASK


def colliding_keys(n: int, bits: int = 11) -> np.ndarray:
    """n distinct INT64 keys whose hashes all have their top `bits` bits zero: one register, an estimate of 1"""
    hashes = [((i + 1) * 0x9E3779B97F4A7C15) & ((1 << (64 - bits)) - 1) for i in range(n)]
    assert len(set(hashes)) == n
    keys = np.array([unmix_block(h) for h in hashes], U).view(np.int64)
    assert (murmur64a([keys]) == np.array(hashes, U)).all()
    assert len(np.unique(keys)) == n and (keys != 2**63 - 1).all()
    return keys


# ------------------------------------------------------------------------------------------------------------ the cases
@dataclass
class NdvCase:
    name: str
    frags: List[List[np.ndarray]]       # [frag][key]
    types: List[int]
    nullables: List[bool]
    bits: int = 0                       # 0 = the default, 11
    offset: int = 0                     # bytes every chunk is moved off its 16-byte boundary (the row-by-row loads)
    want_ndv: Optional[int] = None      # where the case pins the number itself


def _frag(cols, sizes):
    per = [split(c, sizes) for c in cols]
    return [[per[k][f] for k in range(len(cols))] for f in range(len(sizes))]


def _edges(rng, t, n):
    """values over the whole type, the type's min + 1 and max among them"""
    info = np.iinfo(NP[t])
    a = rng.integers(info.min + 1, info.max, n, dtype=np.int64, endpoint=True).astype(NP[t])
    a[n // 3] = info.min + 1
    a[n // 2] = info.max
    return a


BIG_N = 200_003
BIG_SEEDS = {"few": 11, "all": 12}      # (the first seeds tried: both fall inside the accuracy bound, see test_ndv.py)


def big_case(which: str, bits: int) -> NdvCase:
    rng = np.random.default_rng(BIG_SEEDS[which])
    if which == "few":
        pool = rng.integers(-2**62, 2**62, 1000, dtype=np.int64)
        a = pool[rng.integers(0, 1000, BIG_N)]
        a[:1000] = pool
    else:
        a = rng.permutation(BIG_N).astype(np.int64) * 7919 - 10**8
    sizes = [60_001, 0, 70_000, BIG_N - 130_001]
    return NdvCase(f"{BIG_N}_rows_{'1000_distinct' if which == 'few' else 'all_distinct'}_b{bits or 11}", _frag([a], sizes),
                   [INT64], [False], bits)


def build_cases() -> List[NdvCase]:
    rng = np.random.default_rng(2024)
    cases: List[NdvCase] = []
    e64 = np.zeros(0, np.int64)
    cases.append(NdvCase("empty", [[e64]], [INT64], [False], want_ndv=0))
    cases.append(NdvCase("three_empty_fragments", [[e64], [e64], [e64]], [INT64], [False], want_ndv=0))
    cases.append(NdvCase("no_fragments", [], [INT64], [False], want_ndv=0))
    for n in (1, 3, 4, 5):
        cases.append(NdvCase(f"{n}_rows", [[rng.integers(-10**12, 10**12, n, dtype=np.int64)]], [INT64], [False]))
    a = rng.integers(0, 20_000, 50_000).astype(np.int64) * 10**9
    sizes = SPLIT + [50_000 - sum(SPLIT)]
    cases.append(NdvCase("fragment_split_int64", _frag([a], sizes), [INT64], [False]))
    cases.append(NdvCase("fragment_split_int64_unaligned", _frag([a], sizes), [INT64], [False], offset=8))
    for t, name in ((INT8, "int8"), (INT16, "int16"), (INT32, "int32"), (INT64, "int64")):
        cases.append(NdvCase(f"single_{name}_type_edges", _frag([_edges(rng, t, 3001)], [2049, 952]), [t], [False]))
    n = 5003
    i32 = lambda lo, hi: rng.integers(lo, hi, n).astype(np.int32)   # noqa: E731
    cases.append(NdvCase("int32_int16_one_block", _frag([i32(-50, 50), rng.integers(-40, 40, n).astype(np.int16)], [4100, 903]),
                         [INT32, INT16], [False, False]))
    cases.append(NdvCase("three_int32_block_and_tail", _frag([i32(-20, 20), i32(0, 15), _edges(rng, INT32, n) // 2**28], [4100, 903]),
                         [INT32, INT32, INT32], [False] * 3))
    cases.append(NdvCase("three_int32_unaligned", _frag([i32(-20, 20), i32(0, 15), i32(-3, 3)], [4100, 903]),
                         [INT32, INT32, INT32], [False] * 3, offset=4))
    cases.append(NdvCase("int64_int8_widened", _frag([rng.integers(-30, 30, n).astype(np.int64) * 2**40, rng.integers(-128, 128, n).astype(np.int8)],
                                                     [4100, 903]), [INT64, INT8], [False, False]))
    cases.append(NdvCase("four_int64", _frag([rng.integers(-9, 9, n).astype(np.int64) * 3**k for k in (30, 20, 10, 0)], [4100, 903]),
                         [INT64] * 4, [False] * 4))
    # NULLs: rows with a NULL in a nullable component are skipped
    k32 = i32(0, 3000)
    k32[rng.random(n) < 0.3] = NULLS[INT32]
    cases.append(NdvCase("nullable_int32_30pct_null", _frag([k32], [4100, 903]), [INT32], [True]))
    k64 = rng.integers(0, 3000, n).astype(np.int64)
    k64[rng.random(n) < 0.3] = NULLS[INT64]
    cases.append(NdvCase("nullable_int64_int16_30pct_null", _frag([k64, rng.integers(0, 3, n).astype(np.int16)], [4100, 903]),
                         [INT64, INT16], [True, False]))
    cases.append(NdvCase("the_sentinel_in_a_not_null_column_counts", _frag([k32], [4100, 903]), [INT32], [False]))
    cases.append(NdvCase("column_all_null", _frag([np.full(n, NULLS[INT32], np.int32)], [4100, 903]), [INT32], [True], want_ndv=0))
    second = i32(0, 50)
    second[::3] = NULLS[INT32]
    cases.append(NdvCase("null_only_in_the_second_component", _frag([i32(0, 40), second], [4100, 903]), [INT32, INT32], [True, True]))
    second_all = np.full(n, NULLS[INT16], np.int16)
    cases.append(NdvCase("second_component_all_null", _frag([i32(0, 40), second_all], [4100, 903]), [INT32, INT16], [False, True],
                         want_ndv=0))
    for bits in (0, 4, 13):
        cases.append(big_case("few", bits))
        cases.append(big_case("all", bits))
    return cases


# -------------------------------------------------------------------------------- memory: the simulations' and the device's
def aligned(a: np.ndarray, offset: int = 0) -> np.ndarray:
    """a copy of the array `offset` bytes behind a 64-byte boundary"""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 128, np.uint8)
    off = (-raw.ctypes.data) % 64 + offset
    out = raw[off:off + a.nbytes].view(a.dtype)
    out[...] = a
    return out


class HostMem:
    """the host simulations: "device" memory is host memory"""

    def put(self, a: np.ndarray, offset: int = 0):
        b = aligned(a, offset)
        return b, b.ctypes.data

    def zeros_u32(self, n: int):
        b = np.zeros(n, np.uint32)
        return b, b.ctypes.data

    def get_u32(self, handle) -> np.ndarray:
        return handle.copy()

    def read(self, ptr: int, nbytes: int) -> bytes:
        return C.string_at(ptr, nbytes)


def run_estimate(mem, case: NdvCase, regs_addr=None, frags=None) -> int:
    from heavydb_amd.executor import estimate_ndv
    keep, table = [], []
    for cols in (case.frags if frags is None else frags):
        ups = [mem.put(c, case.offset) for c in cols]
        keep.append(ups)
        table.append(([addr for _, addr in ups], len(cols[0])))
    return estimate_ndv(table, case.types, case.nullables, case.bits, regs_addr)


def check_case(mem, case: NdvCase):
    """the registers bit for bit, the estimate within 1 (the summation order of the estimate is free)"""
    want_regs = registers(case.frags, case.types, case.nullables, case.bits)
    handle, addr = mem.zeros_u32(len(want_regs))
    ndv = run_estimate(mem, case, addr)
    got = mem.get_u32(handle)
    bad = np.nonzero(got != want_regs)[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want_regs[bad[:5]])
    assert abs(ndv - estimate(want_regs)) <= 1, (ndv, estimate(want_regs))
    if case.want_ndv is not None:
        assert ndv == case.want_ndv
    # without a register buffer of the caller's: the same estimate from registers of the call's own
    assert run_estimate(mem, case) == ndv


def check_accumulation(mem, case: NdvCase):
    """two calls over halves A and B into one register buffer == one call over A || B == the element-wise max of A's and
    B's own registers (the reference's hll_unify)"""
    half = len(case.frags) // 2
    fa, fb = case.frags[:half], case.frags[half:]
    m = 1 << (case.bits or 11)
    h_ab, a_ab = mem.zeros_u32(m)
    run_estimate(mem, case, a_ab, fa)
    ndv_two_calls = run_estimate(mem, case, a_ab, fb)
    h_one, a_one = mem.zeros_u32(m)
    ndv_one_call = run_estimate(mem, case, a_one)
    h_a, a_a = mem.zeros_u32(m)
    h_b, a_b = mem.zeros_u32(m)
    run_estimate(mem, case, a_a, fa)
    run_estimate(mem, case, a_b, fb)
    two, one, ra, rb = (mem.get_u32(h) for h in (h_ab, h_one, h_a, h_b))
    assert (two == one).all() and (np.maximum(ra, rb) == one).all()
    assert (one == registers(case.frags, case.types, case.nullables, case.bits)).all()
    assert ndv_two_calls == ndv_one_call
    assert ra.any() and rb.any() and (ra != rb).any()


# ------------------------------------------------------------------------------------------------ join tables sized by it
SENTINEL = capi.KEYED_ENTRIES_FROM_NDV


@dataclass
class JoinSizingCase:
    agg: Case                                   # non-grouped COUNT(*), SUM(dim.w) through the table
    proj: Optional[ProjCase] = None             # a Projection through the table (the one-to-many table)
    rows: int = 0


def _outer(rng, inner_keys: List[np.ndarray], types, n, sizes):
    """outer key columns: rows of the inner table picked at random, one in ten made a miss; and a value column"""
    pick = rng.integers(0, len(inner_keys[0]), n)
    cols = [k[pick].copy() for k in inner_keys]
    miss = rng.random(n) < 0.1
    cols[0][miss] = cols[0][miss] + NP[types[0]](3)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    return cols + [v]


def _agg_case(name, outer_cols, outer_types, sizes, inner, inner_types, join_keys, key_types, one_to_many) -> Case:
    nk = len(join_keys)
    fdescs = [InputColDescriptor(t, False, col_range([c], t, False)) for c, t in zip(outer_cols, outer_types)]
    idescs = [InputColDescriptor(t, False, col_range([c], t, False)) for c, t in zip(inner, inner_types)]
    ra = RelAlgExecutionUnit(fdescs, [TargetExpr(COUNT), TargetExpr(SUM, nk, 1), TargetExpr(SUM, nk)], inner_col_descs=idescs,
                             join_outer_col=0 if nk == 1 else list(range(nk)))
    multi = nk > 1
    return Case(name, ra, _frag(outer_cols, sizes), list(inner), list(join_keys) if multi else join_keys[0],
                list(key_types) if multi else key_types[0],
                col_range([join_keys[0]], key_types[0], False) if not multi else ExpressionRange(), True, one_to_many)


def one_to_many_case() -> JoinSizingCase:
    """keyed one-to-many INT64: 40 000 rows over 5 000 keys"""
    rng = np.random.default_rng(31)
    base = rng.choice(10**12, 5000, replace=False).astype(np.int64)
    dk = np.concatenate([base, base[rng.integers(0, 5000, 35_000)]])
    rng.shuffle(dk)
    dw = rng.integers(-1000, 1000, len(dk)).astype(np.int64)
    n, sizes = 6000, [3007, 2993]
    outer = _outer(rng, [dk], [INT64], n, sizes)
    agg = _agg_case("ndv_sized_1n_int64", outer, [INT64, INT64], sizes, [dk, dw], [INT64, INT64], [dk], [INT64], 1)
    uniq, cnt = np.unique(dk, return_counts=True)
    pos = np.minimum(np.searchsorted(uniq, outer[0]), len(uniq) - 1)
    joined = int(cnt[pos][uniq[pos] == outer[0]].sum()) + 64    # room for every joined row
    pra = RelAlgExecutionUnit(list(agg.ra.input_col_descs), [TargetExpr(capi.PROJECT, 1, 0), TargetExpr(capi.PROJECT, 1, 1)],
                              inner_col_descs=list(agg.ra.inner_col_descs), join_outer_col=0, max_groups_buffer_entry_guess=joined)
    proj = ProjCase("ndv_sized_1n_int64_projection", pra, agg.frags, None, 0, list(agg.inner), dk, INT64, agg.join_range, True, 1, False)
    return JoinSizingCase(agg, proj, len(dk))


def composite_case() -> JoinSizingCase:
    """keyed one-to-one (INT32, INT32): 40 000 distinct pairs"""
    rng = np.random.default_rng(32)
    idx = rng.choice(400 * 400, 40_000, replace=False)
    ka, kb = (idx // 400 - 50).astype(np.int32), (idx % 400 * 7).astype(np.int32)
    dw = rng.integers(-1000, 1000, len(ka)).astype(np.int64)
    n, sizes = 6000, [3007, 2993]
    outer = _outer(rng, [ka, kb], [INT32, INT32], n, sizes)
    agg = _agg_case("ndv_sized_1to1_int32_int32", outer, [INT32, INT32, INT64], sizes, [ka, kb, dw], [INT32, INT32, INT64], [ka, kb],
                    [INT32, INT32], 0)
    return JoinSizingCase(agg, None, len(ka))


def fallback_case() -> JoinSizingCase:
    """5 000 distinct INT64 keys whose estimate is 1: the first table has 2 entries, the fill finds it full, the build goes on at
    the default size"""
    rng = np.random.default_rng(33)
    dk = colliding_keys(5000)
    dw = rng.integers(-1000, 1000, len(dk)).astype(np.int64)
    n, sizes = 6000, [3007, 2993]
    outer = _outer(rng, [dk], [INT64], n, sizes)
    agg = _agg_case("ndv_fallback_int64", outer, [INT64, INT64], sizes, [dk, dw], [INT64, INT64], [dk], [INT64], 0)
    return JoinSizingCase(agg, None, len(dk))


def restated_join_ndv(case) -> int:
    keys = case.join_keys if isinstance(case.join_keys, (list, tuple)) else [case.join_keys]
    types = case.join_key_type if isinstance(case.join_key_type, (list, tuple)) else [case.join_key_type]
    return estimate(registers([list(keys)], types, [False] * len(keys), 11))


def build_join(mem, case, keyed_entry_count: int):
    """the case's join table with the given keyed_entry_count -> (HashJoin, what keeps the key columns alive)"""
    from heavydb_amd.executor import HashJoin
    multi = isinstance(case.join_keys, (list, tuple))
    ups = [mem.put(k) for k in (case.join_keys if multi else [case.join_keys])]
    addrs = [addr for _, addr in ups]
    hj = HashJoin.getInstance(addrs if multi else addrs[0], len(ups[0][0]), case.join_key_type, case.join_range,
                              key_nullable=case.join_key_nullable, prefer_baseline=case.join_prefer_baseline,
                              one_to_many=case.join_one_to_many, keyed_entry_count=keyed_entry_count)
    return hj, ups


def oracle_join_sized(oracle, case, entry_count: int):
    r = case.join_range
    return oracle.OracleJoin(case.join_keys, case.join_key_type, r.min, r.max, nullable=case.join_key_nullable,
                             prefer_baseline=case.join_prefer_baseline, one_to_many=case.join_one_to_many,
                             keyed_entry_count=entry_count)


def fetch_result(mem, case):
    from heavydb_amd.executor import FetchResult
    frags = [[mem.put(a) for a in cols] for cols in case.frags]
    inner = [mem.put(a) for a in case.inner]
    return FetchResult([[addr for _, addr in cols] for cols in frags], [len(cols[0]) for cols in case.frags],
                       [addr for _, addr in inner], len(case.inner[0]) if case.inner else 0, 0, [frags, inner])


def check_agg_step(oracle, mem, case: Case, hj):
    """the step through `hj` against the oracle on a table of hj's entry count"""
    from heavydb_amd.executor import Executor
    from tests.helpers import compare_buffers, qmd_equal
    oj = oracle_join_sized(oracle, case, hj.info()["entry_count"])
    q, want, code = oracle.execute(case.ra.to_plan(), case.frags, case.inner, oj, n_threads=2)
    assert code == 0
    case.ra.join_table = hj
    try:
        rs = Executor(0).executeWorkUnit(case.ra, fetch_result(mem, case), allow_retry=False)
        qmd_equal(q, rs.getQueryMemDesc())
        compare_buffers(q, want, rs.getStorage(), case.fp_rtol)
        assert int(want.reshape(-1)[0]) > 1000   # (COUNT(*): the join matched)
    finally:
        case.ra.join_table = None


def check_projection_step(oracle, mem, case: ProjCase, hj):
    """a Projection through the one-to-many table `hj` against the oracle on a table of hj's entry count: the key
    sequence entry by entry, the rows of every run of equal keys as a multiset (the order of the row ids inside one key's
    payload run depends on the build order, as tests/test_projection.py check_projection says)"""
    from heavydb_amd.executor import Executor
    from tests.helpers import qmd_equal
    oj = oracle_join_sized(oracle, case, hj.info()["entry_count"])
    q, want, code = oracle.execute(case.ra.to_plan(), case.frags, case.inner, oj)
    assert code == 0 and q.desc_type == capi.PROJECTION and not q.output_columnar
    case.ra.join_table = hj
    try:
        rs = Executor(0).executeWorkUnit(case.ra, fetch_result(mem, case), allow_retry=False)
    finally:
        case.ra.join_table = None
    qmd_equal(q, rs.getQueryMemDesc())
    n_live = oracle.row_count(q, want)
    assert rs.rowCount() == n_live and n_live > 10_000
    n = q.entry_count
    kw = want.view(np.int64).reshape(n, -1)[:, 0]
    kg = rs.getStorage().view(np.int64).reshape(n, -1)[:, 0]
    assert (kw == kg).all()
    run = np.concatenate([[0], np.cumsum(kw[1:n_live] != kw[:n_live - 1])])

    def canon(rows):
        iv, dv, nu = (np.asarray(x)[:n_live] for x in rows)
        cols = [run] + [c for t in range(iv.shape[1]) for c in (nu[:, t].astype(np.int64), iv[:, t], dv[:, t])]
        order = np.lexsort(cols[::-1])
        return [c[order] for c in cols]
    for a_, b_ in zip(canon(oracle.fetch_rows(q, want)), canon(rs.fetch())):
        assert (a_ == b_).all()


def check_ndv_sized_table(oracle, mem, jc: JoinSizingCase, smaller_than_rows: bool):
    hj, keep = build_join(mem, jc.agg, SENTINEL)
    info = hj.info()
    ndv = restated_join_ndv(jc.agg)
    assert abs(info["entry_count"] - 2 * max(ndv, 1)) <= 2, (info["entry_count"], ndv)
    assert info["hash_type"] == (3 if jc.agg.join_one_to_many else 1)
    if smaller_than_rows:
        assert info["entry_count"] < 2 * jc.rows
    check_agg_step(oracle, mem, jc.agg, hj)
    if jc.proj is not None:
        check_projection_step(oracle, mem, jc.proj, hj)


def check_fallback(oracle, mem):
    jc = fallback_case()
    assert restated_join_ndv(jc.agg) == 1
    hj, keep = build_join(mem, jc.agg, SENTINEL)
    info = hj.info()
    assert info["hash_type"] == 1 and info["entry_count"] == 2 * jc.rows
    check_agg_step(oracle, mem, jc.agg, hj)


def check_other_counts_are_as_before(mem):
    """0 and a positive count size the table as they always have; any other negative value is 0; a perfect table ignores
    the field"""
    jc = one_to_many_case()
    for count, want in ((0, 2 * jc.rows), (12345, 12345), (-2, 2 * jc.rows), (-(2**40), 2 * jc.rows)):
        hj, keep = build_join(mem, jc.agg, count)
        assert hj.info()["entry_count"] == want, (count, hj.info()["entry_count"])
    from heavydb_amd.executor import HashJoin
    keys = np.random.default_rng(34).permutation(3000).astype(np.int64) + 17
    tabs = []
    for count in (SENTINEL, 0):
        k, addr = mem.put(keys)
        hj = HashJoin.getInstance(addr, len(keys), INT64, ExpressionRange(True, 17, 3016), keyed_entry_count=count)
        info = hj.info()
        assert info["hash_type"] == 0 and info["entry_count"] == 3000 and info["bytes"] == 12000
        tabs.append(mem.read(info["device_ptr"], info["bytes"]))
    assert tabs[0] == tabs[1]


# ------------------------------------------------------------------------------------------------------- hostile specs
def hostile_specs():
    """(name, (spec, what it points to), pass an out pointer, the code) — none of them may reach a launch"""
    buf = np.zeros(64, np.int64)
    ptrs = (C.c_void_p * 4)(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    rows = (C.c_int64 * 2)(8, 8)

    def spec(n_keys=1, types=(INT64,), bits=0, n_frags=1, key_buffers=ptrs, frag_rows=rows):
        s = capi.NdvSpec(0, n_keys)
        for k, t in enumerate(types):
            s.key_types[k] = t
        s.precision_bits = bits
        s.n_frags = n_frags
        s.key_buffers = C.cast(key_buffers, C.POINTER(C.c_void_p)) if key_buffers is not None else None
        s.frag_rows = C.cast(frag_rows, C.POINTER(C.c_int64)) if frag_rows is not None else None
        return s, (key_buffers, frag_rows, buf)
    inv, uns = capi.ERR_INVALID_PLAN, capi.ERR_UNSUPPORTED
    out = [("null_spec", None, True, inv), ("null_out_pointer", spec(), False, inv),
           ("no_keys", spec(n_keys=0), True, inv), ("five_keys", spec(n_keys=5), True, inv), ("negative_keys", spec(n_keys=-1), True, inv),
           ("negative_rows", spec(frag_rows=(C.c_int64 * 2)(8, -1), n_frags=2), True, inv),
           ("negative_fragment_count", spec(n_frags=-1), True, inv),
           ("null_row_counts", spec(frag_rows=None), True, inv),
           ("null_buffer_table", spec(key_buffers=None), True, inv),
           ("null_buffer_of_a_fragment_with_rows", spec(key_buffers=(C.c_void_p * 2)(buf.ctypes.data, None), n_frags=2), True, inv),
           ("null_second_key_buffer", spec(n_keys=2, types=(INT64, INT64), key_buffers=(C.c_void_p * 2)(buf.ctypes.data, None)), True, inv),
           ("precision_3", spec(bits=3), True, inv), ("precision_14", spec(bits=14), True, inv), ("precision_negative", spec(bits=-11), True, inv),
           ("double_key", spec(types=(capi.DOUBLE,)), True, uns), ("float_key", spec(types=(capi.FLOAT,)), True, uns),
           ("type_0", spec(types=(0,)), True, uns), ("second_key_double", spec(n_keys=2, types=(INT32, capi.DOUBLE)), True, uns)]
    return out


def check_hostile(lib, live_allocations=None):
    """every hostile spec answers its code and leaves *ndv alone; live_allocations (the simulations' count of device
    allocations): nothing was even allocated, so nothing was launched"""
    for name, sp, with_out, code in hostile_specs():
        before = live_allocations() if live_allocations else 0
        ndv = C.c_int64(-7)
        s = C.byref(sp[0]) if sp is not None else None
        assert lib.mi355q_estimate_ndv(s, None, None, C.byref(ndv) if with_out else None) == code, name
        assert ndv.value == -7, name
        assert (live_allocations() if live_allocations else 0) == before, name
