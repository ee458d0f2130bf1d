"""Inputs for the tail of the lattice member (kernels_part.hip): k_lattice_emit's claim-and-store emission and the packed
walk of k_part_aggregate_idx over its runs.  Shared by the host simulation (tests/test_part_lattice_tail.py) and the
device (tests/test_zz_gpu_part_lattice_tail.py); built on tests/part_lattice_cases.py, with the same sizes (1 M rows on the
device, 250 K in the simulation) and the same four fragments.

Emission (`emission_cases`): a row whose key the emitting lane inserted itself is written with plain stores, a row an
earlier spill merge created is merged into with atomics.
  crowded_table      30 000 groups in a table of 30 300 entries: long probe chains, many lanes claiming neighbouring slots
                     at once; no spill, so every row takes the store path
  both_paths         one key owns half the rows and a NULL-only key another 15 % (their rows come from the hot table
                     through the spill merge: the merge path), two chunks, a nullable value column, targets key, COUNT(*),
                     AVG(v), COUNT(v); the groups 0 (mod 5) hold only NULLs and keep their NULL on both paths
  every_op_double    key, COUNT(*), MIN(v), MAX(v), SUM(v) over a nullable DOUBLE column (the member's generic instantiation)
  every_op_bigint    the same over a nullable BIGINT column

Run edges (`run_edge_case`, host simulation only): the simulation has 8 "CUs", so a unit has B = 8 runs and P = 16 units.
Workgroup b of the scatter owns the super-tiles (12 wave-tiles of 64 quads = 3 072 rows, numbered through the fragments)
that are b (mod 8), and its rows of partition p = index mod 16 make run (b, p).  The case sets the number of rows that
pass the filter per run: 0, 1, one stage minus one record, exactly one stage, one stage plus one, two stages and an odd
bit, exactly two stages; an empty run between two full ones, an empty last run, and a unit whose runs are all empty.  A
stage is what a wave loads ahead: 64 lanes x three pairs of records.
"""
from __future__ import annotations

import numpy as np

from heavydb_amd import capi
from heavydb_amd.executor import ExpressionRange, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
from tests import part_lattice_cases as plc
from tests.cases import Case

NULL_BIGINT = -2**63
SUPER_TILE_ROWS = 12 * 64 * 4   # kProdWaves wave-tiles of 64 quads
SIM_WORKGROUPS = 8              # B on the host simulation's 8 "CUs"
SIM_PARTITIONS = 16             # P of its tables


def pack_stage_records() -> int:
    """records a wave of k_part_aggregate_idx takes per stage of a packed run: 64 lanes x three pairs (its loop steps by 192 pairs)"""
    return 64 * 3 * 2


def _every_op(name, n, rng, bigint):
    idx = rng.integers(0, 40_000, n)
    nulls = (idx % 5 == 0) | (rng.random(n) < 0.1)      # the groups 0 (mod 5) hold only NULLs
    if bigint:
        val = rng.integers(-10**6, 10**6, n).astype(np.int64)
        val[nulls] = NULL_BIGINT
        vdesc = InputColDescriptor(capi.INT64, True, ExpressionRange(True, -10**6, 10**6, True))
    else:
        val = rng.random(n) * 2000.0 - 1000.0
        val[nulls] = plc.NULL_DOUBLE
        vdesc = InputColDescriptor(capi.DOUBLE, True, ExpressionRange(True, 0, 0, True, -1000.0, 1000.0))
    stride, kmin, card = 1_000_003, 7, 40_000
    key = kmin + idx.astype(np.int64) * stride
    fil = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    descs = [InputColDescriptor(capi.INT64, False, ExpressionRange(True, kmin, kmin + (card - 1) * stride)), vdesc,
             InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 2**31 - 1))]
    targets = [TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.MIN, 1), TargetExpr(capi.MAX, 1),
               TargetExpr(capi.SUM, 1)]
    ra = RelAlgExecutionUnit(descs, targets, [Qual(2, capi.LT, 2**30)], [0], max_groups_buffer_entry_guess=2 * card)
    cuts = plc._cuts(n)
    frags = [[key[a:b], val[a:b], fil[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]
    return plc.LatticeCase(name, Case(name, ra, frags), "idx", dict(kernel_variant=2))


def emission_cases(n_rows: int):
    n = n_rows
    rng = np.random.default_rng(20262)
    cases = []

    idx = rng.integers(0, 30_000, n)
    idx[:30_000] = np.arange(30_000)                     # every group is there
    cases.append(plc._build("crowded_table", idx, 1_000_003, 7, 30_000, "idx", rng=rng, n_entries=30_300))

    idx = rng.integers(0, 30_000, n)
    r = rng.random(n)
    idx[r < 0.5] = 4242
    idx[(r >= 0.5) & (r < 0.65)] = 4245                  # 0 (mod 5): NULLs only
    val = rng.random(n) * 1000.0
    val[(idx % 5 == 0) | (rng.random(n) < 0.1)] = plc.NULL_DOUBLE
    cases.append(plc._build("both_paths", idx, 1_000_003, 7, 30_000, "idx", rng=rng, val=val, val_nullable=True,
                            targets=[TargetExpr(capi.PROJECT_KEY), TargetExpr(capi.COUNT), TargetExpr(capi.AVG, 1),
                                     TargetExpr(capi.COUNT, 1)],
                            opts=dict(scratch_bytes=12 << 20), min_launches=2))

    cases.append(_every_op("every_op_double", n, rng, bigint=False))
    cases.append(_every_op("every_op_bigint", n, rng, bigint=True))
    return cases


def run_edge_counts(stage: int) -> np.ndarray:
    """[b][p]: the rows of run (b, p) that pass the filter"""
    rng = np.random.default_rng(20263)
    t = rng.integers(0, 50, (SIM_WORKGROUPS, SIM_PARTITIONS))
    t[:, 0] = [stage, 0, stage, stage, 1, stage - 1, stage + 1, 0]        # an empty run between two full ones, an empty last run
    t[:, 1] = [0, 1, stage - 1, stage, stage + 1, 2 * stage + 21, 2 * stage, 0]
    t[:, 2] = 2 * stage + 21                                              # two stages and an odd bit, every run of the unit
    t[:, 3] = 0                                                           # a unit without a record
    return t


def run_edge_case(n_rows: int = plc.SIM_ROWS):
    stage = pack_stage_records()
    want = run_edge_counts(stage)
    rng = np.random.default_rng(20264)
    n = n_rows
    cuts = plc._cuts(n)
    # the scatter workgroup of every row: super-tiles are numbered through the fragments, each fragment rounded up
    owner = np.empty(n, np.int64)
    first = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        tiles = np.arange(b - a) // SUPER_TILE_ROWS
        owner[a:b] = (first + tiles) % SIM_WORKGROUPS
        first += (b - a + SUPER_TILE_ROWS - 1) // SUPER_TILE_ROWS
    per_unit = 2000                                      # lattice points per partition: far too many for a heavy hitter
    card = SIM_PARTITIONS * per_unit
    idx = rng.integers(0, card, n)
    fil = rng.integers(2**30, 2**31 - 1, n).astype(np.int32)   # fails the filter unless chosen below
    for b in range(SIM_WORKGROUPS):
        rows = rng.permutation(np.flatnonzero(owner == b))
        assert want[b].sum() <= len(rows)
        at = 0
        for p in range(SIM_PARTITIONS):
            mine = rows[at:at + want[b, p]]
            at += want[b, p]
            idx[mine] = p + SIM_PARTITIONS * rng.integers(0, per_unit, len(mine))
            fil[mine] = rng.integers(0, 2**30, len(mine))
    lc = plc._build("run_edges", idx, 1_000_003, 7, card, "idx", rng=rng, fil=fil)
    return lc, want
