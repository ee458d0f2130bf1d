"""Inputs of the partitioned GROUP BY's lattice member (kernels_part.hip: k_part_scatter MODE 3 + k_part_aggregate_idx +
k_lattice_emit), shared by the host simulation (tests/test_part_lattice.py) and the device (tests/test_zz_gpu_part_lattice.py).

Every case is `key, COUNT(*), AVG(f64)`-like over `n_rows` rows in four fragments with kernel_variant 2 (the large-input
members on a small input), each the smallest input that reaches one way of going wrong.  The device runs them at 1 M rows
(a few seconds each, the oracle included).  The host simulation runs a workgroup as 1024 fibers and needs 30 - 60 s per
case at that size (measured: 532 s for the fifteen), so it runs the same cases at 250 K rows, the size of the other
simulated k_part_* tests — the group counts, strides, bounds and fragment shapes are the same.  `member` says what the TRACE line of the step
must show: "idx" (the lattice member ran), "gave_up" (it ran, met a key off the lattice, and the plain member ran after
it), "plain" (it was never started) or None (not looked at).

The number of partitions depends on the device (P = 16 on the host simulation's 8 "CUs", 256 on 256 CUs), so the two cases
that are about P take it as an argument.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from heavydb_amd import capi
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests.cases import Case

DEVICE_ROWS = 1_000_000
SIM_ROWS = 250_000
NULL_DOUBLE = np.finfo(np.float64).tiny   # NULL_DOUBLE = DBL_MIN
TRACE_IDX = "phase 2 member: k_part_aggregate_idx"
TRACE_GAVE_UP = "lattice member gave up"
TRACE_PLAIN = "phase 2 member: k_part_aggregate"


@dataclass
class LatticeCase:
    name: str
    case: Case
    member: Optional[str]
    opts: dict = field(default_factory=dict)
    min_launches: int = 1
    max_groups: Optional[int] = None     # the result has fewer groups than this (filtered-out groups)


def _cuts(n, uneven=False):
    if uneven:                              # no fragment a multiple of 4, one empty
        return [0, 0, n // 4 + 1, n // 4 + 1 + n // 3 + 2, n]
    return [0] + [(n * k // 4) & ~3 for k in range(1, 4)] + [n]


def _build(name, idx, stride, kmin, card, member, *, rng, key_type=capi.INT64, fil=None, val=None, val_nullable=False,
           uneven=False, opts=None, min_launches=1, max_groups=None, n_entries=None, targets=None, key_override=None, pass_row=None):
    """idx: lattice index of every row; the key column's range is [kmin, kmin + (card - 1) * stride]"""
    n = len(idx)
    key = kmin + idx.astype(np.int64) * stride
    if key_override is not None:
        key = key_override(key)
    key = key.astype(np.int32 if key_type == capi.INT32 else np.int64)
    if val is None:
        val = rng.random(n) * 1000.0
    if fil is None:
        fil = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    if pass_row is not None:
        fil[pass_row] = 0                   # this row passes the filter
    descs = [InputColDescriptor(key_type, False, ExpressionRange(True, int(kmin), int(kmin + (card - 1) * stride))),
             InputColDescriptor(capi.DOUBLE, val_nullable, ExpressionRange(True, 0, 0, val_nullable, 0.0, 1000.0)),
             InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 2**31 - 1))]
    if targets is None:
        targets = [TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.AVG, 1)]
    quals = [Qual(2, capi.LT, 2**30)]       # the cfg3f filter
    groups = len(np.unique(idx))
    ra = RelAlgExecutionUnit(descs, targets, quals, [0], max_groups_buffer_entry_guess=n_entries or 2 * groups)
    cuts = _cuts(n, uneven)
    frags = [[key[a:b], val[a:b], fil[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]
    return LatticeCase(name, Case(name, ra, frags), member, dict(kernel_variant=2, **(opts or {})), min_launches, max_groups)


def build_cases(n_partitions: int, n_rows: int):
    """n_partitions: P of a 40 K - 400 K-entry table on the device the cases run on"""
    n = n_rows
    cases = []
    rng = np.random.default_rng(20261)

    # plain lattice: the headline's keys, 7 + 1 000 003 x i
    cases.append(_build("plain", rng.integers(0, 100_000, n), 1_000_003, 7, 100_000, "idx", rng=rng))

    # other strides and bounds: a power of two and a prime with a negative minimum, both ends of the range present
    # (ranges beyond INT32: a BIGINT column whose keys all fit 4 bytes gets 4-byte key components and takes the packed route)
    idx = rng.integers(0, 120_000, n)
    idx[:2] = [0, 119_999]
    cases.append(_build("stride_4096_negative_min", idx, 4096, -(2**40) - 3, 120_000, "idx", rng=rng))
    idx = rng.integers(0, 60_001, n)
    idx[n - 2:] = [60_000, 0]
    cases.append(_build("stride_prime_key_at_max", idx, 999_983, -(10**12) - 11, 60_001, "idx", rng=rng))
    # stride 1: a baseline layout needs a range of tens of millions of points, more than the units' LDS tables hold
    pts = rng.choice(50_000_000, 100_000, replace=False)
    pts[:2] = [0, 49_999_999]
    cases.append(_build("stride_1", pts[rng.integers(0, len(pts), n)], 1, -(2**35), 50_000_000, "plain", rng=rng))
    # an INT32 key column (not a key of the partitioned family: whatever runs, with and without the flag)
    idx = rng.integers(0, 100_000, n)
    idx[:2] = [0, 99_999]
    cases.append(_build("int32_key", idx, 1000, -50_000_000, 100_000, None, rng=rng, key_type=capi.INT32))

    # uneven fragments: sizes that are no multiple of 4, an empty first fragment (the stride is sampled from the second)
    cases.append(_build("uneven_fragments", rng.integers(0, 50_000, n), 1_000_003, 7, 50_000, "idx", rng=rng, uneven=True))

    # two chunks: the accumulator is added into across chunks
    cases.append(_build("two_chunks", rng.integers(0, 20_000, n), 1_000_003, 7, 20_000, "idx", rng=rng,
                        opts=dict(scratch_bytes=12 << 20), min_launches=2))

    # filtered-out groups: every row of the groups 0 (mod 3) fails the filter
    idx = rng.integers(0, 90_000, n)
    fil = rng.integers(0, 2**30, n).astype(np.int32)
    fil[idx % 3 == 0] += 2**30
    cases.append(_build("filtered_out_groups", idx, 1_000_003, 7, 90_000, "idx", rng=rng, fil=fil, max_groups=60_001))

    # NULL values: the groups 0 (mod 5) only hold NULLs (AVG -> NULL, COUNT(*) counted), 10 % NULLs elsewhere
    idx = rng.integers(0, 40_000, n)
    val = rng.random(n) * 1000.0
    val[(idx % 5 == 0) | (rng.random(n) < 0.1)] = NULL_DOUBLE
    cases.append(_build("null_values", idx, 1_000_003, 7, 40_000, "idx", rng=rng, val=val, val_nullable=True,
                        targets=[TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.AVG, 1),
                                 TargetExpr(capi.COUNT, 1)]))

    # lost increment: card no multiple of P and below 4 P — units of two entries, of one, and (points 7 (mod 8) unused) of none
    card = n_partitions + 5
    pts = np.array([i for i in range(card) if i % 8 != 7])
    cases.append(_build("few_points_per_unit", pts[rng.integers(0, len(pts), n)], 10_000_019, 7 + 2**33, card, "idx", rng=rng,
                        n_entries=40_000))

    # heavy hitter: one key owns half the rows — the hot table and the spill merge write its row, emission merges into it
    idx = rng.integers(0, 30_000, n)
    idx[rng.random(n) < 0.5] = 4242
    cases.append(_build("heavy_hitter", idx, 1_000_003, 7, 30_000, "idx", rng=rng))

    # clustered keys: only the lowest tenth of the lattice is used; the interleaved partitions still fill evenly
    # (the table is sized for the declared lattice)
    cases.append(_build("clustered_keys", rng.integers(0, 30_000, n), 1_000_003, 7, 300_000, "idx", rng=rng, n_entries=600_000))

    # off-lattice key: one, in the last fragment only (a row that passes the filter) — nothing is guessed, the plain member
    # computes the step
    def one_off(key):
        key = key.copy()
        key[n - 5] += 1
        return key
    cases.append(_build("off_lattice_key", rng.integers(0, 50_000, n), 1_000_003, 7, 50_000, "gave_up", rng=rng,
                        key_override=one_off, pass_row=n - 5))

    # coarse sample: the first fragment holds even multiples only, so its stride is twice the column's
    idx = rng.integers(0, 50_000, n)
    idx[:n // 4] &= ~1
    idx[n // 4 + 1] = 1
    cases.append(_build("coarse_sample", idx, 1_000_003, 7, 50_000, "gave_up", rng=rng))

    # over the LDS bound: 5 M lattice points, 100 K of them used — more than P units of 12-byte entries hold
    pts = rng.choice(5_000_000, 100_000, replace=False)
    cases.append(_build("over_the_lds_bound", pts[rng.integers(0, len(pts), n)], 1_000_003, 7, 5_000_000, "plain", rng=rng))

    # a range that spans the type: keys anywhere in [-2^63, 2^63 - 2], stride 1, 2^64 - 1 lattice points — the count of
    # points per unit must not wrap into "fits"
    idx = rng.integers(0, 40_000, n)
    wide = rng.integers(-2**63, 2**63 - 2, 40_000, dtype=np.int64)
    wide[:4] = [-2**63, 2**63 - 2, 0, -1]
    cases.append(_build("range_spans_int64", idx, 1, -2**63, 2**64 - 1, "plain", rng=rng, key_override=lambda key: wide[idx]))
    return cases
