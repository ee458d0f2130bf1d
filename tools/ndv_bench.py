"""The NDV estimate (mi355q_estimate_ndv, k_ndv_hll) against a scan of the same bytes on one MI355X: ms per 1 B resident
rows for one INT64 key and for an (INT32, INT32) key, next to a non-grouped MIN(col) step over the same column(s) through
the library, and the ratio of the two.  One JSON line per key shape.  Both calls end in a device synchronise and are
timed with the host clock, alternating, after a warm-up of each; the estimate's time includes its own small copies
(the fragment table to the device, the registers back).  Data is generated on the device with the library's generator.

  python tools/ndv_bench.py [--rows 1e9] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from heavydb_amd import capi
    from heavydb_amd.capi import GEN_I32_MOD, GEN_I64_MOD_MUL, INT32, INT64, MIN
    from heavydb_amd.executor import (Executor, ExpressionRange, FetchResult, InputColDescriptor, RelAlgExecutionUnit,
                                      TargetExpr, estimate_ndv)
    from heavydb_amd.synth import ColSpec, generate_table, my_fragments
    capi.load_library()
    assert torch.cuda.is_available(), "this benchmark measures the device: it has no other path"
    n = int(args.rows)
    frags = my_fragments(n, 0, 1)
    ex = Executor(0)
    R = ExpressionRange
    shapes = [
        ("one INT64 key", 8, [ColSpec(INT64, GEN_I64_MOD_MUL, a=10_000_000, b=1_000_003, c=7, range=R(True, 7, 9_999_999 * 1_000_003 + 7))]),
        ("(INT32, INT32) key", 8, [ColSpec(INT32, GEN_I32_MOD, a=100_000, range=R(True, 0, 99_999)),
                                   ColSpec(INT32, GEN_I32_MOD, a=1000, range=R(True, 0, 999))]),
    ]
    for name, bytes_per_row, specs in shapes:
        cols, bufs, rows = generate_table(torch, specs, frags, 0)
        fr = FetchResult(bufs, rows, keepalive=cols)
        types = [s.type for s in specs]
        table = list(zip(bufs, rows))
        ra = RelAlgExecutionUnit([InputColDescriptor(s.type, False, s.range) for s in specs],
                                 [TargetExpr(MIN, c) for c in range(len(specs))])

        def ndv():
            return estimate_ndv(table, types, [False] * len(types))

        def scan():
            rs = ex.executeWorkUnit(ra, fr, allow_retry=False)
            torch.cuda.synchronize()
            return rs
        est, rs = ndv(), scan()   # warm-up of both
        t_ndv = t_scan = 0.0
        for _ in range(args.steps):
            t0 = time.perf_counter()
            ndv()
            t1 = time.perf_counter()
            scan()
            t2 = time.perf_counter()
            t_ndv += t1 - t0
            t_scan += t2 - t1
        per_b = 1e9 / n * 1e3 / args.steps
        print(json.dumps({"shape": name, "rows": n, "ndv_estimate": est,
                          "ndv_ms_per_1B_rows": t_ndv * per_b, "min_scan_ms_per_1B_rows": t_scan * per_b,
                          "ndv_over_scan": t_ndv / t_scan, "ndv_gbs": n * bytes_per_row * args.steps / t_ndv / 1e9,
                          "scan_gbs": n * bytes_per_row * args.steps / t_scan / 1e9, "scan_kernel": rs.report.kernel_name.decode()}),
              flush=True)
        del cols, fr


if __name__ == "__main__":
    main()
