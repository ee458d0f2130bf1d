#!/usr/bin/env python
"""Grouped steps over a ONE-TO-MANY join at benchmark size — one JSON line per run:

    SELECT f.g, COUNT(*), SUM(f.v), SUM(d.w) FROM f [LEFT] JOIN d ON f.k = d.k GROUP BY f.g

f: --rows outer rows (k BIGINT over 12.5 M values, g INT32 with G distinct values, v BIGINT) in resident device-generated
fragments; d: tools/feature_bench.py f2's dimension — 20 M inner rows, every key 0 .. 9 999 999 twice, so 80 % of the outer rows
match, each of them twice — behind a perfect and a keyed one-to-many table.  Two shape classes: G = 10 000 (the group table in
LDS reach) and G = 10 M (beyond it).

Every shape (table, join kind, G) is run `--repeats` times ALTERNATING the two routes: the expansion (k_join_expand_count / _scan /
_write, then the step without the join) and the same step with MI355Q_OPT_NO_JOIN_EXPAND (the row kernel: probe and group update
per joined row).  A run is the best and the median of --steps steps after --warmup; times are HIP-event times of the whole step on
the launch stream (report.total_ms) and the host's wall clock around the call.  `--lib PATH` loads another build of the library (an
older one ignores the flag: it only has the row kernel); `--only-row-kernel` runs the flagged route alone (what such a build is
measured with).  The first expansion run of a shape is held against the row kernel's table of the same shape (compare_buffers:
integer slots exact).

    python tools/join_expand_bench.py --rows 1e9 > profiles/join_expand_bench_1b.jsonl"""
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
    ap.add_argument("--groups", default="10000,10000000")
    ap.add_argument("--tables", default="perfect,keyed")
    ap.add_argument("--kinds", default="inner,left")
    ap.add_argument("--kernel-variant", type=int, default=0, help="mi355q_exec_options.kernel_variant of the expansion runs (2: the route below its thresholds)")
    ap.add_argument("--only-row-kernel", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--lib", default="", help="path of the libmi355q.so to load (default: this tree's build)")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    args = ap.parse_args()
    import torch
    from heavydb_amd import capi
    from heavydb_amd.capi import COUNT, GEN_I32_MOD, GEN_I64_MOD, INT32, INT64, PROJECT_KEY, SUM
    from heavydb_amd.executor import Executor, ExpressionRange as R, FetchResult, HashJoin, InputColDescriptor, RelAlgExecutionUnit, TargetExpr
    from heavydb_amd.synth import ColSpec, generate_table, my_fragments
    lib = capi.load_library(args.lib or None)
    capi._lib = lib   # (a library loaded by path becomes the process's)
    no_expand = getattr(capi, "OPT_NO_JOIN_EXPAND", 32768)
    n = int(args.rows)
    frags = my_fragments(n, 0, 1)
    ex = Executor(0)
    m = 20_000_000
    dk = torch.arange(m, device="cuda", dtype=torch.int64) // 2
    dw = torch.arange(m, device="cuda", dtype=torch.int64) % 1000
    inner = [InputColDescriptor(INT64, False, R(True, 0, m // 2 - 1)), InputColDescriptor(INT64, False, R(True, 0, 999))]

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

    for groups in [int(float(g)) for g in args.groups.split(",")]:
        specs = [ColSpec(INT64, GEN_I64_MOD, a=12_500_000, range=R(True, 0, 12_499_999)),
                 ColSpec(INT32, GEN_I32_MOD, a=groups, range=R(True, 0, groups - 1)),
                 ColSpec(INT64, GEN_I64_MOD, a=1000, range=R(True, 0, 999))]
        cols, bufs, rows = generate_table(torch, specs, frags, 0)
        fr = FetchResult(bufs, rows, keepalive=cols + [dk, dw])
        fr.inner_col_buffers = [int(dk.data_ptr()), int(dw.data_ptr())]
        fr.inner_num_rows = m
        descs = [InputColDescriptor(s.type, False, s.range) for s in specs]
        for tag in args.tables.split(","):
            hj = HashJoin.getInstance(int(dk.data_ptr()), m, INT64, R(True, 0, m // 2 - 1), prefer_baseline=tag == "keyed", one_to_many=1)
            for ktag in args.kinds.split(","):
                ra = RelAlgExecutionUnit(descs, [TargetExpr(PROJECT_KEY), TargetExpr(COUNT), TargetExpr(SUM, 2), TargetExpr(SUM, 1, 1)],
                                         groupby_exprs=[1], inner_col_descs=inner, join_outer_col=0, join_table=hj,
                                         join_kind=capi.JOIN_LEFT if ktag == "left" else capi.JOIN_INNER,
                                         max_groups_buffer_entry_guess=2 * groups, num_tuples=n)
                first = {}
                for run in range(args.repeats):
                    for mode, flags in [("expand", 0), ("row_kernel", no_expand)]:
                        if mode == "expand" and args.only_row_kernel:
                            continue
                        variant = args.kernel_variant if mode == "expand" else 0
                        rs, ev, wall = timed(ra, fr, flags, variant)
                        line = {"table": tag, "table_type": hj.info()["hash_type"], "kind": ktag, "groups": groups, "rows": n, "mode": mode, "run": run,
                                "label": args.label, "flags": flags, "kernel_variant": variant,
                                "route": ex.explain(ra, rows, flags=flags, kernel_variant=variant), "kernel": rs.report.kernel_name.decode(),
                                "n_launches": rs.report.n_launches, "ms": round(min(ev), 3), "ms_median": round(statistics.median(ev), 3),
                                "ms_all": [round(x, 3) for x in ev], "wall_ms": round(min(wall), 3), "result_rows": rs.rowCount()}
                        if mode not in first and not args.no_verify:
                            first[mode] = rs
                            if len(first) == 2:
                                from tests.helpers import compare_buffers
                                compare_buffers(rs.getQueryMemDesc(), first["row_kernel"].getStorage(), first["expand"].getStorage(), 1e-9)
                                line["verified_against_row_kernel"] = True
                                first = {"expand": None, "row_kernel": None}
                        print(json.dumps(line), flush=True)
            hj.free()
        del cols, fr


if __name__ == "__main__":
    main()
