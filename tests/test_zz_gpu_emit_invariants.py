"""The emission kernels that merge with PLAIN read-modify-writes — k_cast_key_emit (DOUBLE casts of keys inside
[-2^53, 2^53]), k_perfect_twin_emit, k_affine_twin_emit, k_zip_targets, idx_emit<NK, false> — against the oracle ON THE
DEVICE.  They all rest on "exactly one lane touches one output row per launch"; the host simulation runs the lanes of a
block one after the other and cannot see that rule broken, and the reference-benchmark shapes of test_zz_gpu_refbench.py
reach these kernels only with small keys, injective casts, one chunk and mostly empty tables.  Here: casts that are NOT
injective (INT64 keys beyond 2^53, INT32 keys beyond 2^24 cast to FLOAT: neighbouring lanes merge into one row, which
needs atomics), baseline tables filled close to capacity (long probe chains, lanes claiming neighbouring rows), several
chunks (a later chunk merges into rows an earlier one wrote), spilled records next to phase 2, one zip per value column.

Every value column is an integer column: keys, COUNT, SUM, MIN, MAX are compared bit for bit, only the AVG quotient of the
fetched rows has the 1e-9 tolerance — a lost update cannot hide.  Every case asserts the route it is about (report.kernel_name /
variant / n_launches), compares every slot of every group, and runs twice (a race that lands right once rarely does twice).

Fragments are uploaded one by one (an allocation each: 16-byte aligned whatever the cut), cut at odd rows."""
import os

import numpy as np
import pytest

from heavydb_amd import capi
from tests.helpers import check_probe_invariant, compare_buffers, compare_rows, qmd_equal

pytestmark = pytest.mark.gpu

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
NPT = {capi.INT32: np.int32, capi.INT64: np.int64}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    capi.load_library()
    return torch


def _values(rng, n, t, lo, hi, null_frac=0.1):
    """a nullable integer value column: uniform in [lo, hi], about 10 % NULLs"""
    v = rng.integers(lo, hi + 1, n).astype(NPT[t])
    v[rng.random(n) < null_frac] = np.iinfo(NPT[t]).min
    return v


def _seven(n_keys=1, v=None):
    """PROJECT_KEY ..., COUNT(*), SUM(v), MIN(v), MAX(v), AVG(v), COUNT(v) — a plan holds MAX_TARGETS = 8: with three keys
    COUNT(v) stays out (AVG(v) keeps the same count in its second slot)"""
    from heavydb_amd.executor import TargetExpr
    return ([TargetExpr(capi.PROJECT_KEY, g) for g in range(n_keys)] +
            [TargetExpr(capi.COUNT), TargetExpr(capi.SUM, v), TargetExpr(capi.MIN, v), TargetExpr(capi.MAX, v),
             TargetExpr(capi.AVG, v), TargetExpr(capi.COUNT, v)])[:capi.MAX_TARGETS]


def _frags(cols, cuts):
    cuts = [0] + list(cuts) + [len(cols[0])]
    return [[c[a:b] for c in cols] for a, b in zip(cuts[:-1], cuts[1:])]


def _check(torch, oracle, ra, frags, **opts):
    """the step through the library (kernel_variant 2 = the large-input members on a small input, no retry with a larger
    table) against the oracle's walk over the stated plan, twice"""
    from heavydb_amd.executor import Executor, FetchResult
    q, want, code = oracle.execute(ra.to_plan(), frags, n_threads=min(os.cpu_count() or 1, 16))
    assert code == 0, code
    dev = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols] for cols in frags]
    fr = FetchResult([[int(t.data_ptr()) for t in cols] for cols in dev], [len(cols[0]) for cols in frags], keepalive=dev)
    ex = Executor(0)
    rs = ex.executeWorkUnit(ra, fr, kernel_variant=2, allow_retry=False, **opts)
    qmd_equal(q, rs.getQueryMemDesc())
    first = rs.getStorage()
    compare_buffers(q, want, first, 1e-9)
    check_probe_invariant(q, first)
    assert rs.rowCount() == oracle.row_count(q, want)
    compare_rows(q, oracle.fetch_rows(q, want), rs.fetch(), 1e-9)
    again = ex.executeWorkUnit(ra, fr, kernel_variant=2, allow_retry=False, **opts)
    compare_buffers(q, first, again.getStorage())
    rs.n_groups = oracle.row_count(q, want)
    rs.q = q
    return rs


# ---- a / b / c: GROUP BY CAST(<integer column> AS DOUBLE | FLOAT) -> the step on the integer column + k_cast_key_emit ----------
def _cast_key_case(rng, n, to, key_type, base, span, key_null_frac, val_type, guess, cut=15_001):
    from heavydb_amd.executor import Expr, ExpressionRange, InputColDescriptor, RelAlgExecutionUnit
    key = (base + rng.integers(0, span, n)).astype(NPT[key_type])
    nullable = key_null_frac > 0
    if nullable:
        key[rng.random(n) < key_null_frac] = np.iinfo(NPT[key_type]).min
    val = _values(rng, n, val_type, -1000, 999)
    descs = [InputColDescriptor(key_type, nullable, ExpressionRange(True, base, base + span - 1, nullable)),
             InputColDescriptor(val_type, True, ExpressionRange(True, -1000, 999, True))]
    e = Expr.col(0).cast(to).with_range(ExpressionRange(True, 0, 0, nullable, float(base), float(base + span - 1)))
    ra = RelAlgExecutionUnit(descs, _seven(1, 1), [], [2], max_groups_buffer_entry_guess=guess, exprs=[e], num_tuples=n)
    # the groups the cast leaves, counted without the library or the oracle: distinct casts of the non-NULL keys (+ the NULL group)
    live = key[key != np.iinfo(NPT[key_type]).min] if nullable else key
    cast = live.astype(np.float32 if to == capi.FLOAT else np.float64)
    groups = len(np.unique(cast)) + (1 if nullable and live.size < n else 0)
    return ra, _frags([key, val], [cut]), groups, len(np.unique(live))


@pytest.mark.parametrize("base,key_null_frac,want_groups", [(2**60, 0.0, 9), (-2**60, 0.05, 18), (2**53 - 1000, 0.05, 1502)],
                         ids=["2p60", "minus_2p60_null_keys", "straddling_2p53_null_keys"])
def test_cast_key_double_beyond_2p53_merges_entries(torch_cuda, oracle, base, key_null_frac, want_groups):
    """INT64 keys beyond 2^53: neighbouring doubles are 2 (just above 2^53) to 256 (at 2^60) apart, so up to 256 NEIGHBOURING
    entries of the integer-keyed table — neighbouring lanes of one wave — cast to ONE double and merge into one row of the
    stated table: atomics, as for FLOAT (CastKeyArgs::injective = 0).  With plain read-modify-writes the device loses
    COUNT / SUM / MIN / MAX / AVG updates here; the host simulation (one lane after the other) cannot."""
    ra, frags, groups, distinct = _cast_key_case(np.random.default_rng(53), 40_000, capi.DOUBLE, capi.INT64, base, 2000,
                                                 key_null_frac, capi.INT64, 8192)
    assert distinct == 2000 and groups == want_groups, (distinct, groups)     # (the test's own arithmetic)
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.report.n_launches >= 2, rs.report.n_launches      # the step on the integer column + the emit
    assert rs.n_groups == want_groups, rs.n_groups


def test_cast_key_float_with_32_integers_per_group(torch_cuda, oracle):
    """INT32 keys 2^28 + [0, 3000): 32 integers per FLOAT (round to nearest: 95 FLOATs) + the NULL group; every row of the
    stated table is merged into by up to 32 neighbouring lanes (the atomic branch)"""
    ra, frags, groups, distinct = _cast_key_case(np.random.default_rng(28), 40_000, capi.FLOAT, capi.INT32, 2**28, 3000, 0.05,
                                                 capi.INT64, 8192)
    assert distinct == 3000 and groups == 96, (distinct, groups)
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.report.n_launches >= 2, rs.report.n_launches
    assert rs.n_groups == 96, rs.n_groups


def test_cast_key_double_injective_into_a_full_table(torch_cuda, oracle):
    """the plain read-modify-write path that stays (keys inside [-2^53, 2^53]): ~97 K entries, each its own group, into a
    baseline table with 1 / 64 of its rows to spare — long probe chains, every wave's lanes claim rows next to one another"""
    rng = np.random.default_rng(120)
    ra, frags, groups, distinct = _cast_key_case(rng, 200_003, capi.DOUBLE, capi.INT32, 0, 120_000, 0.01, capi.INT32, 0,
                                                 cut=75_001)
    assert groups == distinct + 1 and groups > 90_000
    ra.max_groups_buffer_entry_guess = groups + groups // 64
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.report.n_launches >= 2, rs.report.n_launches
    assert rs.n_groups == groups


# ---- d: baseline steps over ranged INT keys -> perfect-hash twin (index-partitioned family) + k_perfect_twin_emit -------------
# scratch_bytes = 1 MB is below what the family's staging lines alone need (make_idx_plan: a line per partition and
# workgroup), so a chunk shrinks to its floor, ONE FRAGMENT: four fragments = four chunks on any device
TINY_SCRATCH = 1 << 20
FOUR_CUTS = [15_001, 30_003, 45_006]


@pytest.mark.parametrize("packed", [False, True], ids=["plain_records", "packed_records"])
@pytest.mark.parametrize("n_keys", [2, 3])
def test_perfect_twin_in_four_chunks_into_a_full_table(torch_cuda, oracle, n_keys, packed):
    """1401 x 901 / 102 x 121 x 111 key combinations (beyond the perfect-hash threshold: a baseline layout), ~58 K of them
    live, NULL keys in every column; the twin's table is built by four chunks (phase 2 merges chunks 2 - 4 into rows chunk 1
    wrote: idx_emit<NK, false> / k_idx_aggregate_pk) and re-keyed into a baseline table with 1 / 32 of its rows to spare"""
    from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit
    rng = np.random.default_rng(8 + n_keys)
    n = 60_000
    bounds = [(-700, 699), (0, 899)] if n_keys == 2 else [(-50, 50), (0, 119), (0, 109)]
    keys, descs = [], []
    for lo, hi in bounds:
        k = rng.integers(lo, hi + 1, n).astype(np.int32)
        k[rng.random(n) < 0.03] = I32.min
        keys.append(k)
        descs.append(InputColDescriptor(capi.INT32, True, ExpressionRange(True, lo, hi, True)))
    val = _values(rng, n, capi.INT32, -1000, 999)
    descs.append(InputColDescriptor(capi.INT32, True, ExpressionRange(True, -1000, 999, True)))
    groups = len(np.unique(np.stack(keys, axis=1), axis=0))
    assert groups > 55_000
    ra = RelAlgExecutionUnit(descs, _seven(n_keys, n_keys), [], list(range(n_keys)),
                             max_groups_buffer_entry_guess=groups + groups // 32, num_tuples=n)
    rs = _check(torch_cuda, oracle, ra, _frags(keys + [val], FOUR_CUTS), scratch_bytes=TINY_SCRATCH,
                flags=0 if packed else capi.OPT_NO_IDX_PACK)
    assert rs.q.desc_type == capi.GROUP_BY_BASELINE_HASH
    assert rs.report.kernel_name.decode() == "k_idx_scatter", rs.report.kernel_name
    assert (rs.report.variant in (7, 8)) == packed and (packed or rs.report.variant == 6), rs.report.variant
    assert rs.report.n_launches > 2, rs.report.n_launches          # the twin's chunks + the emit
    assert rs.n_groups == groups


# ---- e: the index-partitioned family itself, four chunks, spilled records next to phase 2 ----------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["plain_records", "packed_records"])
@pytest.mark.parametrize("n_vals", [1, 3])
def test_idx_partitioned_in_four_chunks_with_spilled_records(torch_cuda, oracle, n_vals, packed):
    """one INT32 key, 150 K entries, value columns that carry ranges and a few values outside them (NULLs in a column declared
    without, the NOT NULL column's INT32_MIN): those rows leave as full records through the spill list (idx_emit<NK, true>,
    atomic) and land in rows phase 2 (plain) writes in the same step; chunks 2 - 4 merge into rows chunk 1 wrote"""
    from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit, TargetExpr
    rng = np.random.default_rng(150 + n_vals)
    n, card = 200_003, 150_000
    key = rng.integers(1, card + 1, n).astype(np.int32)
    key[rng.random(n) < 0.02] = I32.min
    v0 = rng.integers(1, 11, n).astype(np.int32)             # declared [1, 10], nullable, "no NULLs"
    v0[rng.random(n) < 0.01] = I32.min
    v0[rng.random(n) < 0.002] = 11
    v0[rng.random(n) < 0.002] = -7
    v0[rng.random(n) < 0.001] = I32.max
    v1 = rng.integers(-3, 4, n).astype(np.int32)             # declared [-3, 3], NOT NULL
    v1[rng.random(n) < 0.002] = I32.min
    v1[rng.random(n) < 0.002] = 1 << 20
    v2 = rng.integers(0, 100, n).astype(np.int32)            # declared [0, 99], nullable, ~10 % NULLs
    v2[rng.random(n) < 0.1] = I32.min
    descs = [InputColDescriptor(capi.INT32, True, ExpressionRange(True, 1, card, True)),
             InputColDescriptor(capi.INT32, True, ExpressionRange(True, 1, 10, False)),
             InputColDescriptor(capi.INT32, False, ExpressionRange(True, -3, 3, False)),
             InputColDescriptor(capi.INT32, True, ExpressionRange(True, 0, 99, True))]
    if n_vals == 1:
        targets = _seven(1, 1)
    else:
        targets = [TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.SUM, 1), TargetExpr(capi.MIN, 1),
                   TargetExpr(capi.MAX, 2), TargetExpr(capi.SUM, 2), TargetExpr(capi.AVG, 3), TargetExpr(capi.COUNT, 3)]
    ra = RelAlgExecutionUnit(descs, targets, [], [0], num_tuples=n)
    rs = _check(torch_cuda, oracle, ra, _frags([key, v0, v1, v2], [50_001, 100_003, 150_006]), scratch_bytes=TINY_SCRATCH,
                flags=0 if packed else capi.OPT_NO_IDX_PACK)
    assert rs.q.desc_type == capi.GROUP_BY_PERFECT_HASH
    assert rs.report.kernel_name.decode() == "k_idx_scatter", rs.report.kernel_name
    assert (rs.report.variant in (7, 8)) if packed else rs.report.variant == 6, rs.report.variant
    assert rs.report.n_launches >= 3, rs.report.n_launches
    assert not packed or rs.report.spilled_rows > 0, rs.report.spilled_rows   # (plain records hold any INT32: nothing to spill)


# ---- f: BIGINT keys on a lattice -> INT32 lattice indices + perfect-hash twin + k_affine_twin_emit -------------------------
def _affine_case(rng, n_keys, off_lattice):
    from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit
    n, cut = 100_003, 35_001
    # (the twin's step is the index-partitioned family's from 65 537 entries on, and nobody's between the LDS members' 32 K
    # and that: 70 000 lattice points)
    points = [70_000] if n_keys == 1 else [280, 250]
    mins = [-123_456_789_012, 7][:n_keys]
    keys, descs = [], []
    for pts, lo in zip(points, mins):
        k = (lo + 10_000 * rng.integers(0, pts, n)).astype(np.int64)
        k[rng.random(n) < 0.03] = I64.min
        keys.append(k)
        descs.append(InputColDescriptor(capi.INT64, True, ExpressionRange(True, lo, lo + 10_000 * (pts - 1), True)))
    if off_lattice:
        keys[0][cut + 4_321] = mins[0] + 10_000 * 7 + 1      # one key between two lattice points, in the SECOND fragment
    val = _values(rng, n, capi.INT32, -1000, 999)
    descs.append(InputColDescriptor(capi.INT32, True, ExpressionRange(True, -1000, 999, True)))
    groups = len(np.unique(np.stack(keys, axis=1), axis=0))
    ra = RelAlgExecutionUnit(descs, _seven(n_keys, n_keys), [], list(range(n_keys)),
                             max_groups_buffer_entry_guess=groups + groups // 32, num_tuples=n)
    return ra, _frags(keys + [val], [cut]), groups


@pytest.mark.parametrize("n_keys", [1, 2])
def test_affine_twin_into_a_full_table(torch_cuda, oracle, n_keys):
    """keys = min + 10 000 i with NULL keys, 70 K lattice points (one key: 70 000; two: 280 x 250), ~3 / 4 of them live,
    re-keyed into a baseline table with 1 / 32 of its rows to spare"""
    ra, frags, groups = _affine_case(np.random.default_rng(10_000 + n_keys), n_keys, False)
    assert groups > 40_000
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.q.desc_type == capi.GROUP_BY_BASELINE_HASH
    assert rs.report.n_launches >= 2, rs.report.n_launches
    # the inner step ran on a perfect-hash twin: no baseline step of 40 K+ groups is either family's
    assert rs.report.kernel_name.decode() in ("k_idx_scatter", "k_groupby_lds"), rs.report.kernel_name
    assert rs.n_groups == groups


def test_affine_twin_is_given_up_for_a_key_off_the_lattice(torch_cuda, oracle):
    """one key of the second fragment lies between two lattice points: k_affine_keys raises its flag, the step runs as
    stated (a baseline family) and the odd key is a group of its own"""
    on = _affine_case(np.random.default_rng(10_002), 2, False)
    ra, frags, groups = _affine_case(np.random.default_rng(10_002), 2, True)
    assert groups == on[2] + 1
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.n_groups == groups
    # (the index-partitioned family takes perfect-hash layouts only: its name in the report is the twin's)
    assert rs.report.kernel_name.decode() != "k_idx_scatter", rs.report.kernel_name
    twin = _check(torch_cuda, oracle, on[0], on[1])
    assert twin.report.kernel_name.decode() == "k_idx_scatter", twin.report.kernel_name


# ---- g: several value columns -> one run per value column + k_zip_targets -----------------------------------------------------
def _zip_case(rng, n_vals, n_keys=1):
    """value columns v0 INT32, v1 INT64, v2 INT32, v3 INT64 (nullable, ~10 % NULLs), one or two aggregates each (a plan holds
    MAX_TARGETS = 8: SUM AVG | MIN COUNT | MAX AVG | SUM MIN, the second of a column as far as there is room), AVG among them.  An
    INT64 value column keeps the lattice route away; keys too wide to be packed (one BIGINT key beyond INT32; two whose
    ranges need 70 bits) keep the packed-key route away: execute_multi_value zips into the stated table itself"""
    from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit, TargetExpr
    n, cut = 200_003, 75_001
    if n_keys == 1:
        card = 100_000
        keys = [(rng.integers(0, card, n) * 1000003 + 7).astype(np.int64)]
        descs = [InputColDescriptor(capi.INT64, False, ExpressionRange(True, 7, (card - 1) * 1000003 + 7))]
    else:
        keys = [(rng.integers(0, 400, n) * 1000003 + 7).astype(np.int64), (rng.integers(0, 250, n) << 33).astype(np.int64)]
        keys[1][rng.random(n) < 0.03] = I64.min
        descs = [InputColDescriptor(capi.INT64, False, ExpressionRange(True, 7, 399 * 1000003 + 7)),
                 InputColDescriptor(capi.INT64, True, ExpressionRange(True, 0, 249 << 33, True))]
    vtypes = [capi.INT32, capi.INT64, capi.INT32, capi.INT64][:n_vals]
    vals = [_values(rng, n, t, -1000 * (j + 1), 999 * (j + 1)) for j, t in enumerate(vtypes)]
    descs += [InputColDescriptor(t, True, ExpressionRange(True, -1000 * (j + 1), 999 * (j + 1), True)) for j, t in enumerate(vtypes)]
    pairs = [(capi.SUM, capi.AVG), (capi.MIN, capi.COUNT), (capi.MAX, capi.AVG), (capi.SUM, capi.MIN)]
    room = capi.MAX_TARGETS - n_keys - 1 - n_vals
    two = [j for j in (0, 2, 1, 3) if j < n_vals][:room]
    targets = [TargetExpr(capi.PROJECT_KEY, g) for g in range(n_keys)] + [TargetExpr(capi.COUNT)]
    for j in range(n_vals):
        targets += [TargetExpr(a, n_keys + j) for a in pairs[j][:2 if j in two else 1]]
    groups = len(np.unique(np.stack(keys, axis=1), axis=0))
    ra = RelAlgExecutionUnit(descs, targets, [], list(range(n_keys)), max_groups_buffer_entry_guess=groups + groups // 32,
                             num_tuples=n)
    return ra, _frags(keys + vals, [cut]), groups


def test_zip_of_two_to_four_value_columns_into_a_full_table(torch_cuda, oracle):
    """one BIGINT key, ~86 K groups in a baseline table with 1 / 32 of its rows to spare: run 0's zip claims the rows, the
    zips of runs 1 ... n find them again (baseline_find_or_insert at a high fill) and store their own slots"""
    launches = []
    for n_vals in (2, 3, 4):
        ra, frags, groups = _zip_case(np.random.default_rng(100 + n_vals), n_vals)
        assert groups > 80_000
        rs = _check(torch_cuda, oracle, ra, frags)
        assert rs.q.desc_type == capi.GROUP_BY_BASELINE_HASH and rs.n_groups == groups
        launches.append(rs.report.n_launches)
    assert launches[0] >= 2 and launches[0] < launches[1] < launches[2], launches       # one run more per value column


def test_zip_with_two_key_columns(torch_cuda, oracle):
    """two BIGINT keys (400 x 251 combinations, NULLs in the second): the rows are found through baseline_find_or_insert_multi"""
    ra, frags, groups = _zip_case(np.random.default_rng(202), 3, n_keys=2)
    assert groups > 80_000
    one_run = _zip_case(np.random.default_rng(202), 2, n_keys=2)
    rs = _check(torch_cuda, oracle, ra, frags)
    assert rs.q.desc_type == capi.GROUP_BY_BASELINE_HASH and rs.q.group_col_count == 2 and rs.n_groups == groups
    fewer = _check(torch_cuda, oracle, one_run[0], one_run[1])
    assert 2 <= fewer.report.n_launches < rs.report.n_launches, (fewer.report.n_launches, rs.report.n_launches)


def test_zip_into_a_perfect_hash_table_that_keeps_its_keys(torch_cuda, oracle):
    """a perfect-hash layout no aggregate of which can tell an empty entry (nullable arguments with NULLs, no COUNT(*), no
    MIN): the rows keep their key, run 0's zip finds it empty and writes it with plain stores"""
    from heavydb_amd.executor import ExpressionRange, InputColDescriptor, RelAlgExecutionUnit, TargetExpr
    rng = np.random.default_rng(800)
    n, card = 40_003, 800
    key = rng.integers(0, card, n).astype(np.int32)
    key[key % 7 == 3] = 5                                     # (some entries stay empty)
    vals = [_values(rng, n, t, -1000, 999, 0.3) for t in (capi.INT32, capi.INT64, capi.INT32)]
    descs = [InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, card - 1))] + \
        [InputColDescriptor(t, True, ExpressionRange(True, -1000, 999, True)) for t in (capi.INT32, capi.INT64, capi.INT32)]
    targets = [TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.SUM, 1), TargetExpr(capi.MAX, 1), TargetExpr(capi.AVG, 2),
               TargetExpr(capi.COUNT, 2), TargetExpr(capi.MAX, 3)]

    def run(tg):
        ra = RelAlgExecutionUnit(descs, tg, [], [0], num_tuples=n)
        return _check(torch_cuda, oracle, ra, _frags([key] + vals, [15_001]))
    rs = run(targets)
    assert rs.q.desc_type == capi.GROUP_BY_PERFECT_HASH and not rs.q.keyless
    assert rs.n_groups == len(np.unique(key)) < card
    fewer = run(targets[:5])                                  # two value columns: a run less
    assert 2 <= fewer.report.n_launches < rs.report.n_launches, (fewer.report.n_launches, rs.report.n_launches)
