#!/usr/bin/env python
"""Star joins at benchmark size — one JSON line per run:

    SELECT d.region, COUNT(*), SUM(f.amount) FROM f [LEFT] JOIN d ON f.did = d.id WHERE d.segment BETWEEN 2 AND 8 GROUP BY d.region

f: --rows fact rows (did BIGINT over 1.25 x S values, so 80 % of the rows match; amount BIGINT; code INT32 with G distinct values)
in resident device-generated fragments; d: S rows, id = 0 .. S - 1 behind a one-to-one perfect table of S slots, region INT32 with
G distinct values (a multiplicative scramble of the id, so neighbouring slots differ), segment = id % 10.

Every shape (S, G, join kind) is run `--repeats` times ALTERNATING the two routes: the star member (k_join_group_code +
k_star_groupby_lds; with kernel_variant 2 for maps above --variant2-above bytes, which reaches the member whatever the planner's default) and the flattened route
(MI355Q_OPT_NO_STAR_GROUPBY: k_join_gather + the joinless step).  As a floor, the plain few-groups step over the same fact
columns with the group code handed in as a column (`SELECT f.code, COUNT(*), SUM(f.amount) FROM f GROUP BY f.code`: no join, no
map) is timed once per (S, G).  A run is the best and the median of --steps steps after --warmup; times are HIP-event times of
the whole step on the launch stream (report.total_ms).  The first star run of a shape is held against the flattened route's table
(compare_buffers: integer slots exact).

    python tools/star_join_bench.py --rows 1e9 > profiles/star_join_bench_1b.jsonl"""
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
    ap.add_argument("--groups", default="100,1000")
    ap.add_argument("--slots", default="100000,1000000,16000000")
    ap.add_argument("--kinds", default="inner,left")
    ap.add_argument("--variant2-above", type=int, default=4 << 20, help="star runs over a larger map pass kernel_variant 2")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    args = ap.parse_args()
    import torch
    from heavydb_amd import capi
    from heavydb_amd.capi import COUNT, GEN_I32_MOD, GEN_I64_MOD, INT32, INT64, PROJECT_KEY, SUM
    from heavydb_amd.executor import (Executor, ExpressionRange as R, FetchResult, HashJoin, InputColDescriptor, Qual, RelAlgExecutionUnit,
                                      TargetExpr, inner)
    from heavydb_amd.synth import ColSpec, generate_table, my_fragments
    capi.load_library()
    n = int(args.rows)
    frags = my_fragments(n, 0, 1)
    ex = Executor(0)

    def timed(ra, fr, flags, variant):
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
        did = torch.arange(slots, device="cuda", dtype=torch.int64)
        seg = (did % 10).to(torch.int32)
        hj = HashJoin.getInstance(int(did.data_ptr()), slots, INT64, R(True, 0, slots - 1))
        span = slots + slots // 4
        for groups in [int(float(g)) for g in args.groups.split(",")]:
            region = ((did * 2654435761) % groups).to(torch.int32)
            specs = [ColSpec(INT64, GEN_I64_MOD, a=span, range=R(True, 0, span - 1)),
                     ColSpec(INT64, GEN_I64_MOD, a=1000, range=R(True, 0, 999)),
                     ColSpec(INT32, GEN_I32_MOD, a=groups, range=R(True, 0, groups - 1))]
            cols, bufs, rows = generate_table(torch, specs, frags, 0)
            fr = FetchResult(bufs, rows, keepalive=cols + [did, region, seg])
            fr.inner_col_buffers = [int(region.data_ptr()), int(seg.data_ptr())]
            fr.inner_num_rows = slots
            descs = [InputColDescriptor(s.type, False, s.range) for s in specs]
            inner_descs = [InputColDescriptor(INT32, False, R(True, 0, groups - 1)), InputColDescriptor(INT32, False, R(True, 0, 9))]
            targets = [TargetExpr(PROJECT_KEY), TargetExpr(COUNT), TargetExpr(SUM, 1)]
            # the floor: the group code as a fact column, no join
            floor = RelAlgExecutionUnit(descs, targets, groupby_exprs=[2], num_tuples=n)
            rs, ev, wall = timed(floor, fr, 0, 0)
            print(json.dumps(line_of(rs, ev, wall, mode="floor_plain_groupby", slots=slots, groups=groups, route=ex.explain(floor, rows))), flush=True)
            code_bytes = slots * (2 if groups + 1 <= 32767 else 4)
            for ktag in args.kinds.split(","):
                ra = RelAlgExecutionUnit(descs, targets, [Qual(inner(1), capi.GE, 2), Qual(inner(1), capi.LE, 8)], [inner(0)],
                                         inner_col_descs=inner_descs, join_outer_col=0, join_table=hj,
                                         join_kind=capi.JOIN_LEFT if ktag == "left" else capi.JOIN_INNER, num_tuples=n)
                first = {}
                for run in range(args.repeats):
                    for mode, flags in [("star", 0), ("flattened", capi.OPT_NO_STAR_GROUPBY)]:
                        variant = 2 if mode == "star" and code_bytes > args.variant2_above else 0
                        rs, ev, wall = timed(ra, fr, flags, variant)
                        line = line_of(rs, ev, wall, mode=mode, slots=slots, groups=groups, kind=ktag, run=run, flags=flags, kernel_variant=variant,
                                       map_bytes=code_bytes, route=ex.explain(ra, rows, flags=flags, kernel_variant=variant, inner_rows=slots))
                        if mode not in first and not args.no_verify:
                            first[mode] = rs
                            if len(first) == 2:
                                from tests.helpers import compare_buffers
                                compare_buffers(rs.getQueryMemDesc(), first["flattened"].getStorage(), first["star"].getStorage(), 1e-9)
                                line["verified_against_flattened"] = True
                                first = {"star": None, "flattened": None}
                        print(json.dumps(line), flush=True)
            del cols, fr
        hj.free()


if __name__ == "__main__":
    main()
