"""Inputs of the lattice member's packed records (kernels_part.hip: k_part_scatter MODE 4 + the PACK member of
k_part_aggregate_idx: twelve {8-byte value, 16-bit entry} per 128-byte segment), shared by the host simulation
(tests/test_part_lattice_pack.py) and the device (tests/test_zz_gpu_part_lattice_pack.py).

Built with tests/part_lattice_cases.py's `_build` (four fragments, the cfg3f filter, kernel_variant 2) and run at the same
sizes: 1 M rows on the device, 250 K in the simulation.  Every case is the smallest input that reaches one way the packed
line can go wrong; each runs packed (the default), with MI355Q_OPT_NO_LATTICE_PACK (the 16-byte records) and in the oracle.

A staged line holds 12 x 1024 / P records (P = 256 on the device: 48; P = 16 in the simulation: 768), so the cases about
run lengths and entries take P as an argument.
"""
from __future__ import annotations

import numpy as np

from heavydb_amd import capi
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, TargetExpr
from tests.part_lattice_cases import NULL_DOUBLE, _build

TRACE_PACKED = "lattice records: 12 per 128-byte segment"
TRACE_UNPACKED = "lattice records: 8 per 128-byte segment"
SUPER_TILE = 12 * 64 * 4   # rows one scatter workgroup takes in one step (12 producer waves x 64 lanes x 4 rows)


def build_cases(n_partitions: int, n_rows: int):
    """n_partitions: P of a 40 K - 400 K-entry table on the device the cases run on"""
    n, P = n_rows, n_partitions
    cases = []
    rng = np.random.default_rng(20262)

    # run lengths around the segment and the line: every row fails the filter but a few hundred of ONE super-tile (one
    # workgroup) in the last fragment; partition j of that workgroup receives exactly lens[j] records — a single record, one
    # short of a segment, a full segment, one over, an odd tail pair, and the same around the line (and two lines + 1)
    line = 12 * 1024 // P
    lens = [1, 11, 12, 13, 25, line - 1, line, line + 1]
    if sum(lens) + 2 * line + 1 <= SUPER_TILE:
        lens.append(2 * line + 1)
    assert sum(lens) <= SUPER_TILE and len(lens) <= P
    start = (n * 3 // 4) & ~3                  # the last fragment's first row (part_lattice_cases._cuts)
    rows = start + rng.permutation(SUPER_TILE)[:sum(lens)]
    idx = rng.integers(0, 3 * P, n)
    idx[rows] = np.repeat(np.arange(len(lens)), lens) + P * rng.integers(0, 3, len(rows))   # three groups per partition
    fil = rng.integers(2**30, 2**31 - 1, n).astype(np.int32)
    fil[rows] = 0
    cases.append(_build("run_lengths_around_the_line", idx, 10_000_019, 7 + 2**33, 3 * P, "idx", rng=rng, fil=fil,
                        n_entries=40_000, max_groups=3 * len(lens) + 1))

    # high entry, unsigned: key, COUNT(*) only — 4-byte entries, 36 000 of them per unit; both ends of the lattice are
    # present, so entries 0 and 35 999 (> 32 767: a signed 16-bit read would lose it) occur
    card = P * 36_000
    pts = rng.choice(card, 100_000, replace=False)
    pts[:2] = [0, card - 1]
    idx = pts[rng.integers(0, len(pts), n)]
    idx[:2] = pts[:2]
    lc = _build("high_entry_count_only", idx, 1_000_003, 7, card, "idx", rng=rng, fil=np.zeros(n, np.int32),
                targets=[TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT)])
    cases.append(lc)

    # one partition overflows: every index a multiple of P, thousands of keys — all records land in partition 0, its runs
    # fill to the last packed record (cap / 8 x 12) and the rest takes the spill list
    cases.append(_build("one_partition_overflows", P * rng.integers(0, 5_000, n), 1_000_003, 7, P * 5_000, "idx", rng=rng,
                        fil=np.zeros(n, np.int32)))

    # value bits: SUM(BIGINT) over [-2^62, 2^62] (the upper bits of the 8-byte value must survive the line) ...
    val = rng.integers(-2**62, 2**62, n, dtype=np.int64, endpoint=True)
    lc = _build("bigint_values", rng.integers(0, 40_000, n), 1_000_003, 7, 40_000, "idx", rng=rng, val=val,
                targets=[TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.SUM, 1)])
    lc.case.ra.input_col_descs[1] = InputColDescriptor(capi.INT64, False, ExpressionRange(True, -2**62, 2**62))
    cases.append(lc)
    # ... and AVG(f64) over negative doubles with NULL_DOUBLE: the groups 0 (mod 5) only hold NULLs, 10 % NULLs elsewhere
    idx = rng.integers(0, 40_000, n)
    val = -1.0 - rng.random(n) * 1000.0
    val[(idx % 5 == 0) | (rng.random(n) < 0.1)] = NULL_DOUBLE
    lc = _build("negative_doubles_and_nulls", idx, 1_000_003, 7, 40_000, "idx", rng=rng, val=val, val_nullable=True,
                targets=[TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.AVG, 1),
                         TargetExpr(capi.COUNT, 1)])
    lc.case.ra.input_col_descs[1] = InputColDescriptor(capi.DOUBLE, True, ExpressionRange(True, 0, 0, True, -1001.0, -1.0))
    cases.append(lc)

    # two chunks: run lengths and staged lines of the first chunk must not leak into the second
    cases.append(_build("two_chunks", rng.integers(0, 20_000, n), 1_000_003, 7, 20_000, "idx", rng=rng,
                        opts=dict(scratch_bytes=12 << 20), min_launches=2))

    # uneven fragments: sizes that are no multiple of 4, one empty
    cases.append(_build("uneven_fragments", rng.integers(0, 50_000, n), 1_000_003, 7, 50_000, "idx", rng=rng, uneven=True))

    # off-lattice key in uneven fragments: the packed member gives up, the plain member restarts and computes the step
    def one_off(key):
        key = key.copy()
        key[n - 5] += 1
        return key
    cases.append(_build("off_lattice_key", rng.integers(0, 50_000, n), 1_000_003, 7, 50_000, "gave_up", rng=rng, uneven=True,
                        key_override=one_off, pass_row=n - 5))
    return cases
