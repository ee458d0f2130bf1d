#!/usr/bin/env python
"""SEMI / ANTI join levels at benchmark size — one JSON line per run:

    SELECT SUM(f.amount), COUNT(*)          FROM f WHERE [NOT] EXISTS (SELECT 1 FROM d WHERE d.id = f.did)     (step "sum")
    SELECT f.code, COUNT(*), SUM(f.amount)  FROM f WHERE ... GROUP BY f.code      -- 1 000 groups              (step "few")
    SELECT f.gk, COUNT(*), SUM(f.amount)    FROM f WHERE ... GROUP BY f.gk        -- 10 M BIGINT groups        (step "many")

f: --rows fact rows in resident device-generated fragments (did BIGINT over a span that makes 80 % of the rows match; amount
BIGINT; code INT32; gk BIGINT).  d: ids 0 .. S - 1 without every --holes-th one, behind a perfect table of S slots: one-to-one,
and ("many") one-to-many with every id twice.

Every (S, table, step) is run --repeats times ALTERNATING the routes:
  semi / anti   the mask route (k_join_exists_mask, then the joinless step on `mask = 1`);
  inner         the same plan stated as INNER over the one-to-one table — identical rows, the existing routes;
  floor         the joinless step on a mask column computed beforehand (torch): what the step costs with the probe for free.
A run is the best and the median of --steps steps after --warmup; times are HIP-event times of the whole step on the launch
stream (report.total_ms).  Every measured table is held against the floor's (the semi floor for semi / inner, the anti floor for
anti: compare_buffers, integer slots exact) before its time is printed — the first run of every route and shape, every run
with --verify-every-run.

    python tools/semi_join_bench.py --rows 1e9 --slots 1e6,1e8 --holes 16 > profiles/semi_join_bench_1b.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/semi_join_bench.py --rows 1e9 --modes semi --steps-list sum   # the kernel alone"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slots", default="1e6,1e8")
    ap.add_argument("--holes", type=int, default=16, help="every holes-th id of the dimension is missing (0: none)")
    ap.add_argument("--tables", default="one,many")
    ap.add_argument("--steps-list", default="sum,few,many")
    ap.add_argument("--modes", default="semi,anti,inner,floor")
    ap.add_argument("--many-groups", type=float, default=1e7)
    ap.add_argument("--flags", type=int, default=0, help="exec flags of the mask route's runs (64: the general member)")
    ap.add_argument("--mask-variant", type=int, default=0, help="kernel_variant of the semi / anti runs (2 keeps the mask route where the default restates the step as the INNER plan)")
    ap.add_argument("--verify-every-run", action="store_true", help="compare every run's table with the floor's, not the first one's of each route")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    args = ap.parse_args()
    import torch
    from heavydb_amd import capi
    from heavydb_amd.capi import COUNT, GEN_I32_MOD, GEN_I64_MOD, INT8, INT32, INT64, PROJECT_KEY, SUM
    from heavydb_amd.executor import Executor, ExpressionRange as R, FetchResult, HashJoin, InputColDescriptor, Qual, RelAlgExecutionUnit, TargetExpr
    from heavydb_amd.synth import ColSpec, generate_table, my_fragments
    from tests.helpers import compare_buffers
    capi.load_library()
    n = int(args.rows)
    frags = my_fragments(n, 0, 1)
    ex = Executor(0)
    modes = args.modes.split(",")
    many_groups = int(args.many_groups)

    def timed(ra, fr, flags=0, variant=0):
        ev, wall, rs = [], [], None
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            rs = ex.executeWorkUnit(ra, fr, allow_retry=False, flags=flags, kernel_variant=variant)
            t1 = time.perf_counter()
            if i >= args.warmup:
                ev.append(rs.report.total_ms)
                wall.append((t1 - t0) * 1e3)
        return rs, ev, wall

    def line_of(rs, ev, wall, **kw):
        out = dict(kw)
        out.update({"rows": n, "label": args.label, "kernel": rs.report.kernel_name.decode(), "variant": rs.report.variant,
                    "n_launches": rs.report.n_launches, "ms": round(min(ev), 3), "ms_median": round(statistics.median(ev), 3),
                    "ms_all": [round(x, 3) for x in ev], "wall_ms": round(min(wall), 3), "result_rows": rs.rowCount()})
        return out

    for slots in [int(float(s)) for s in args.slots.split(",")]:
        ids = torch.arange(slots, device="cuda", dtype=torch.int64)
        if args.holes > 0:
            ids = ids[ids % args.holes != 0]
        live = int(ids.numel())
        span = int(live / 0.8)                   # 80 % of the fact keys have a row
        specs = [ColSpec(INT64, GEN_I64_MOD, a=span, range=R(True, 0, span - 1)),
                 ColSpec(INT64, GEN_I64_MOD, a=1000, range=R(True, 0, 999)),
                 ColSpec(INT32, GEN_I32_MOD, a=1000, range=R(True, 0, 999)),
                 ColSpec(INT64, GEN_I64_MOD, a=many_groups, range=R(False))]
        cols, bufs, rows = generate_table(torch, specs, frags, 0)
        # the floor's mask columns, one byte per row: 1 = the dimension has the key (semi) / has it not (anti)
        hit = cols[0] < slots
        if args.holes > 0:
            hit &= cols[0] % args.holes != 0
        mask_t = {"semi": hit.to(torch.int8), "anti": (~hit).to(torch.int8)}
        del hit
        starts = [sum(rows[:f]) for f in range(len(rows))]
        assert all(lo % 16 == 0 for lo in starts)   # (the typed families want 16-byte aligned chunks)
        masks = {k: [int(m.data_ptr()) + lo for lo in starts] for k, m in mask_t.items()}
        descs = [InputColDescriptor(s.type, False, s.range) for s in specs]
        fr = FetchResult(bufs, rows, keepalive=cols)
        step_plans = {"sum": ([], [TargetExpr(SUM, 1), TargetExpr(COUNT)], 16384),
                      "few": ([2], [TargetExpr(PROJECT_KEY), TargetExpr(COUNT), TargetExpr(SUM, 1)], 16384),
                      "many": ([3], [TargetExpr(PROJECT_KEY), TargetExpr(COUNT), TargetExpr(SUM, 1)], 2 * many_groups)}
        for table in args.tables.split(","):
            keys = torch.cat([ids, ids]) if table == "many" else ids
            hj = HashJoin.getInstance(int(keys.data_ptr()), int(keys.numel()), INT64, R(True, 0, slots - 1), one_to_many=2 if table == "many" else 0)
            for step in args.steps_list.split(","):
                group, targets, guess = step_plans[step]
                floors = {}
                for kind in ("semi", "anti"):
                    if kind not in modes and not (kind == "semi" and "inner" in modes):
                        continue
                    ra = RelAlgExecutionUnit(descs + [InputColDescriptor(INT8, False, R(True, 0, 1))], targets, [Qual(len(descs), capi.EQ, 1)], group,
                                             max_groups_buffer_entry_guess=guess, num_tuples=n)
                    frm = FetchResult([b + [m] for b, m in zip(bufs, masks[kind])], rows, keepalive=cols + [mask_t[kind]])
                    rs, ev, wall = timed(ra, frm)
                    floors[kind] = rs
                    if "floor" in modes and table == args.tables.split(",")[0]:
                        print(json.dumps(line_of(rs, ev, wall, mode="floor_" + kind, slots=slots, table="-", step=step, route=ex.explain(ra, rows))), flush=True)
                runs = [m for m in ("semi", "anti", "inner") if m in modes and not (m == "inner" and table == "many")]
                for run in range(args.repeats):
                    for mode in runs:
                        jk = {"semi": capi.JOIN_SEMI, "anti": capi.JOIN_ANTI, "inner": capi.JOIN_INNER}[mode]
                        ra = RelAlgExecutionUnit(descs, targets, [], group, join_outer_col=0, join_table=hj, join_kind=jk,
                                                 max_groups_buffer_entry_guess=guess, num_tuples=n)
                        rs, ev, wall = timed(ra, fr, 0 if mode == "inner" else args.flags, 0 if mode == "inner" else args.mask_variant)
                        if run == 0 or args.verify_every_run:   # before the time is kept (a route is deterministic in its integer slots)
                            ref = floors["anti" if mode == "anti" else "semi"]
                            compare_buffers(rs.getQueryMemDesc(), ref.getStorage(), rs.getStorage(), 1e-9)
                        print(json.dumps(line_of(rs, ev, wall, mode=mode, slots=slots, live_keys=live, table=table, step=step, run=run, flags=args.flags,
                                                 verified_against_floor=bool(run == 0 or args.verify_every_run), kernel_variant=0 if mode == "inner" else args.mask_variant,
                                                 route=ex.explain(ra, rows, inner_rows=int(keys.numel()), kernel_variant=0 if mode == "inner" else args.mask_variant))), flush=True)
                del floors
            hj.free()
            del keys
        del cols, fr, masks, mask_t


if __name__ == "__main__":
    main()
