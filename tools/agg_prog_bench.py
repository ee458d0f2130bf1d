#!/usr/bin/env python
"""Aggregates of EXPRESSIONS at benchmark size — one JSON line per shape:

    i32_product     SELECT SUM(a * b)                            FROM t WHERE c < K      a, b, c INT32 (TPC-H Q6's shape)
    cast_bigint     SELECT SUM(CAST(a AS BIGINT) * CAST(b AS BIGINT))   ... WHERE c < K
    double_arith    SELECT SUM(p * 2.5 - q), MIN(..), AVG(..)    ... WHERE c < K         p, q DOUBLE

K passes 50 % of the rows.  Each shape is timed next to its YARDSTICK, the plain-column step that reads the same columns under
the same qual (SUM(a), SUM(b) / SUM(p), SUM(q): k_scan_agg), over resident device-generated columns in 32 M-row fragments.
`--flags 4096` (MI355Q_OPT_NO_AGG_PROGRAMS) runs the two-pass route (k_project, then the plain-column step); `--lib PATH` loads
another build of the library (an older one ignores the flag: it only has the two-pass route).  Times are HIP-event times of
the whole step on the launch stream (report.total_ms), best and median of --steps runs after --warmup runs, and the host's
wall clock around the call.  Every line is verified against the oracle on the first --verify-rows rows, through the same
route.

`--group G` runs the GROUPED variants of the three shapes — SELECT g, SUM(a * b) ... WHERE c < K GROUP BY g, key g INT32 with G
distinct values — next to the plain-column grouped step over the same columns.  The one-pass route (k_groupby_lds_prog) is not a
default (it lost this measurement): `--kernel-variant 2` asks for it; without it, or with `--flags 8192`
(MI355Q_OPT_NO_GROUPED_AGG_PROGRAMS), the step takes the two passes.

    python tools/agg_prog_bench.py --rows 1e9 > profiles/agg_prog_bench_1b.jsonl
    python tools/agg_prog_bench.py --rows 1e9 --group 100 --kernel-variant 2 >> profiles/agg_prog_grouped_bench_1b.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(capi, Expr, TargetExpr, nc=5):
    """(name, expressions, targets over expression column NC.., yardstick targets, columns read)"""
    I32, I64, F64 = capi.INT32, capi.INT64, capi.DOUBLE
    C = Expr.col
    arith = C(3).mul(Expr.lit(F64, 2.5), F64).sub(C(4), F64)
    two_sums = lambda x, y: [TargetExpr(capi.SUM, x), TargetExpr(capi.SUM, y)]   # noqa: E731
    return [
        ("i32_product", [C(0).mul(C(1), I32)], [TargetExpr(capi.SUM, nc)], two_sums(0, 1), [0, 1, 2]),
        ("cast_bigint", [C(0).cast(I64).mul(C(1).cast(I64), I64)], [TargetExpr(capi.SUM, nc)], two_sums(0, 1), [0, 1, 2]),
        ("double_arith", [arith], [TargetExpr(capi.SUM, nc), TargetExpr(capi.MIN, nc), TargetExpr(capi.AVG, nc)], two_sums(3, 4), [2, 3, 4]),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flags", type=int, default=0, help="MI355Q_OPT_* of the expression step (4096 / 8192: the two-pass route, non-grouped / grouped)")
    ap.add_argument("--kernel-variant", type=int, default=0, help="mi355q_exec_options.kernel_variant of the expression step (2: the grouped one-pass route)")
    ap.add_argument("--group", type=int, default=0, help="G > 0: GROUP BY g, an INT32 key column with G distinct values")
    ap.add_argument("--lib", default="", help="path of the libmi355q.so to load (default: this tree's build)")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    ap.add_argument("--verify-rows", type=float, default=1_000_003)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--tune-blocks-per-cu", type=int, default=0)
    args = ap.parse_args()
    import torch
    from heavydb_amd import capi
    from heavydb_amd.executor import (Executor, Expr, ExpressionRange, FetchResult, InputColDescriptor, Qual, RelAlgExecutionUnit,
                                      TargetExpr, generate_column)
    lib = capi.load_library(args.lib or None)
    capi._lib = lib   # (a library loaded by path becomes the process's)
    n, frag = int(args.rows), 32_000_000
    # 0 a, 1 b: INT32 in [0, 30 000) (a * b fits INT32); 2 c: INT32 in [0, 1 M); 3 p: DOUBLE in [0, 1000); 4 q: DOUBLE in [0, 100)
    gens = [(torch.int32, capi.GEN_I32_MOD, 31, 30_000, 0.0), (torch.int32, capi.GEN_I32_MOD, 32, 30_000, 0.0),
            (torch.int32, capi.GEN_I32_MOD, 33, 1_000_000, 0.0), (torch.float64, capi.GEN_F64_UNIT, 34, 0, 1000.0),
            (torch.float64, capi.GEN_F64_UNIT, 35, 0, 100.0)]
    if args.group > 0:   # 5 g: INT32 in [0, G)
        gens.append((torch.int32, capi.GEN_I32_MOD, 36, args.group, 0.0))
    cols = [torch.empty(n, dtype=dt, device="cuda:0") for dt, *_ in gens]
    bufs, rows, off = [], [], 0
    while off < n:
        k = min(frag, n - off)
        for t, (_, kind, seed, mod, scale) in zip(cols, gens):
            generate_column(int(t.data_ptr()) + off * t.element_size(), k, kind, seed, mod, 0, 0, scale, 0, off, 0)
        bufs.append([int(t.data_ptr()) + off * t.element_size() for t in cols])
        rows.append(k)
        off += k
    torch.cuda.synchronize()
    descs = [InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 29_999)), InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 29_999)),
             InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, 999_999)),
             InputColDescriptor(capi.DOUBLE, False, ExpressionRange(True, 0, 0, False, 0.0, 1000.0)),
             InputColDescriptor(capi.DOUBLE, False, ExpressionRange(True, 0, 0, False, 0.0, 100.0))]
    width = [4, 4, 4, 8, 8]
    group, keys = [], []
    if args.group > 0:
        descs.append(InputColDescriptor(capi.INT32, False, ExpressionRange(True, 0, args.group - 1)))
        width.append(4)
        group, keys = [5], [TargetExpr(capi.PROJECT_KEY, 0)]
    quals = [Qual(2, capi.LT, 500_000)]
    fr = FetchResult(bufs, rows, keepalive=cols)
    ex = Executor(0)

    def timed(ra, flags, variant=0):
        ev, wall, rs = [], [], None
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            rs = ex.executeWorkUnit(ra, fr, allow_retry=False, flags=flags, tune_blocks_per_cu=args.tune_blocks_per_cu, kernel_variant=variant)
            t1 = time.perf_counter()
            if i >= args.warmup:
                ev.append(rs.report.total_ms)
                wall.append((t1 - t0) * 1e3)
        return rs, ev, wall

    for name, exprs, targets, yard_targets, reads in shapes(capi, Expr, TargetExpr, len(descs)):
        if args.only and name not in args.only.split(','):
            continue
        rng = ExpressionRange(True, 0, 900_000_000) if name != "double_arith" else ExpressionRange(True, 0, 0, False, -100.0, 2500.0)
        xs = [e.with_range(rng) for e in exprs]
        ra = RelAlgExecutionUnit(descs, keys + targets, quals, group, exprs=xs, num_tuples=n)
        yard = RelAlgExecutionUnit(descs, keys + yard_targets, quals, group, num_tuples=n)
        reads = reads + group
        rs, ev, wall = timed(ra, args.flags, args.kernel_variant)
        yrs, yev, _ = timed(yard, 0)
        per_row = sum(width[c] for c in reads)
        best, ybest = min(ev), min(yev)
        line = {"shape": name, "rows": n, "groups": args.group, "label": args.label, "flags": args.flags, "kernel_variant": args.kernel_variant,
                "route": ex.explain(ra, rows, flags=args.flags, kernel_variant=args.kernel_variant),
                "kernel": rs.report.kernel_name.decode(), "ms": round(best, 3), "ms_median": round(statistics.median(ev), 3),
                "ms_all": [round(x, 3) for x in ev], "wall_ms": round(min(wall), 3), "yardstick_kernel": yrs.report.kernel_name.decode(),
                "yardstick_ms": round(ybest, 3), "yardstick_ms_all": [round(x, 3) for x in yev], "ratio_to_yardstick": round(best / ybest, 3),
                "bytes_per_row": per_row, "frac_of_8TBs": round(per_row * n / (best * 1e-3) / 8e12, 4)}
        if args.verify_rows:
            from oracle import oracle as orc
            from tests.helpers import compare_buffers
            m = min(int(args.verify_rows), rows[0])
            host = [t[:m].cpu().numpy() for t in cols]
            small = FetchResult([[int(t.data_ptr()) for t in cols]], [m], keepalive=cols)
            got = ex.executeWorkUnit(ra, small, allow_retry=False, flags=args.flags, kernel_variant=args.kernel_variant)
            q, want, code = orc.execute(ra.to_plan(), [host], n_threads=8)
            assert code == 0
            compare_buffers(q, want, got.getStorage(), 1e-9)
            line["verified_rows"] = m
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
