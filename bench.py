#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X-native query-step executor.

Metric (BASELINE.json): rows/sec + achieved HBM GB/s of a filtered GROUP BY on 10 B rows at
1/2/4/8 GPUs.  A "step" is one execution of the query step over the synthetic table already
resident in HBM (SURVEY.md section 8(d), cfg3-filtered by default):

    SELECT key, COUNT(*), AVG(f64) FROM t WHERE i32 < 2^30 GROUP BY key
    10 B rows, 10 M int64 keys (baseline hash layout, 20 M entries x 32 B), 20 B/row

  python bench.py                       # N=1, cfg3f at the largest row count that fits
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

Multi-GPU: fragments are dealt round-robin to the ranks (total rows fixed -> "strong"
scaling), each rank runs the step on its shard and the partial tables are merged over RCCL
(heavydb_amd/multi_gpu.py) inside the timed region.

One JSON line on rank 0: metric/value/unit/... plus
  "roofline":     dominant kernel's algorithmic bytes per launch / its HIP-event duration,
                  against the 8 TB/s HBM3E peak (guide: ~6.3 TB/s is the copy ceiling)

A plain run only sets up, warms up, times the --steps steps and prints that line.  --full adds
what takes runs of its own:
  "roofline.measured_ceiling" / "scheme_ceiling": this GPU's HBM read and copy rates, measured
                  here (a 1 B-row COUNT(*) scan and a 4 GB device copy)
  "cpu_baseline": the oracle (CPU restatement of HeavyDB's CPU executor; kind "port") timed on
                  this box's host cores on a bounded sample of the same workload
  "per_rank":     N > 1: one more, untimed step taken apart on every rank (step, then merge)

--dump-outputs DIR writes the rows the last timed step returned as DIR/*.npy (dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cfg3f", choices=["cfg1", "cfg2", "cfg3", "cfg3f", "cfg4"])
    ap.add_argument("--rows", type=float, default=0, help="total rows (default: the config's size)")
    ap.add_argument("--variant", type=int, default=0, help="kernel variant (0 = plan-time choice)")
    ap.add_argument("--force-generic", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="(kept for compatibility; unused)")
    ap.add_argument("--cpu-rows", type=float, default=0, help="CPU-baseline sample rows (default: SURVEY 8(d): cfg1/cfg2 "
                    "full size, cfg3*/cfg4 1 B rows)")
    ap.add_argument("--scratch-gb", type=float, default=0, help="partition scratch cap of the step (0 = library default)")
    ap.add_argument("--overlap-cus", type=int, default=0, help="partitioned GROUP BY: CUs of phase 1 while phase 2 of the previous "
                    "chunk runs on the rest (tune_overlap_cus; 0 = the library's choice, -1 = phases one after the other)")
    ap.add_argument("--blocks-per-cu", type=int, default=0, help="tune_blocks_per_cu (experiments)")
    ap.add_argument("--opt-flags", type=int, default=0, help="mi355q_exec_options.flags (MI355Q_OPT_*, experiments: 4 = payload probe without pacing)")
    ap.add_argument("--probe-passes", type=int, default=0, help="cfg4 --sparse: passes per partition of the keyed payload probe "
                    "(probe_keyed_passes; 0 = the library's choice)")
    ap.add_argument("--sparse", action="store_true", help="cfg4: sparse dim keys -> keyed {key, row id} join table (3.2 GB)")
    ap.add_argument("--sum-dim", action="store_true", help="cfg4: Query B, also SUM(dim.w) (reads an inner column)")
    ap.add_argument("--holes", type=int, default=0, help="cfg4: the dimension without the keys = 5 (mod HOLES): a perfect table with empty slots "
                                                          "(the general probe; the dense dimension's join is planned away as a range filter)")
    ap.add_argument("--verify", action="store_true", help="size-independent property checks")
    ap.add_argument("--prepartitioned", action="store_true",
                    help="cfg3/cfg3f, N > 1: the table arrives hash-partitioned by key (every key on one "
                         "rank), so the final merge is skipped (SURVEY 8e's second mode)")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "traffic.json"),
                    help="per-kernel HBM bytes/launch from a rocprofv3 --pmc pass (optional)")
    ap.add_argument("--hostsim", action="store_true",
                    help="TEST ONLY (tests/test_bench_multi_rank.py): every rank runs the host simulation of the library "
                         "(tests/hostsim) on CPU tensors and gloo carries the collectives — exercises the N-rank control flow "
                         "of this script without a GPU; its numbers are not measurements")
    ap.add_argument("--full", action="store_true",
                    help="also measure the HBM ceiling, the CPU baseline and (N > 1) the per-rank breakdown")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the rows the last timed step returned as DIR/*.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs needs --steps >= 1")
    return args


def _free_port() -> int:
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _bind_host_simulation(torch):
    """--hostsim: this process's `device` is the host simulation of the library (the real device sources compiled for the
    CPU, tests/hostsim); tensors are CPU tensors."""
    from heavydb_amd import capi
    from tests.helpers import hostsim_lib
    capi._lib = capi.load_library(hostsim_lib(real_fast=True))
    real = {n: getattr(torch, n) for n in ("zeros", "empty", "full", "arange", "tensor")}
    strip = lambda f: (lambda *a, **k: f(*a, **{x: y for x, y in k.items() if x != "device" or not str(y).startswith("cuda")}))  # noqa: E731
    for n, f in real.items():
        setattr(torch, n, strip(f))

    class _Stream:
        def synchronize(self):
            pass
    torch.cuda.current_stream = lambda *a, **k: _Stream()
    torch.cuda.synchronize = lambda *a, **k: None
    torch.cuda.set_device = lambda *a, **k: None
    torch.cuda.empty_cache = lambda *a, **k: None


def fit_rows(cfg: str, want_rows: int, world: int, free_bytes: int, bytes_per_row: int) -> int:
    """Largest row count (multiple of the fragment size) whose shard fits this GPU with
    headroom for the output table and the partition scratch."""
    from heavydb_amd.synth import FRAGMENT_ROWS
    budget = int(free_bytes * 0.90) - (24 << 30)  # table, scratch, allocator slack
    per_rank = max(budget // bytes_per_row, FRAGMENT_ROWS)
    total = min(want_rows, per_rank * world)
    if total < want_rows:
        total = max(total // (FRAGMENT_ROWS * world), 1) * FRAGMENT_ROWS * world
    return int(total)


def cpu_baseline(cfg: str, info: dict, target_s: float, sample_rows: int = 0) -> dict:
    """The oracle (kind "port": CPU restatement of HeavyDB's CPU executor) timed on this
    box's host cores: one kernel per 32 M-row fragment on its own host thread with a private output
    buffer (Execute.cpp:3121-3153), then ResultSetStorage::reduce of the buffers in order, itself
    multi-threaded for big baseline tables like the reference's (ResultSetReduction.cpp:236-272).
    Sample: cfg1 and cfg2 at their full size, cfg3 / cfg3f / cfg4 at N = 1 B rows; the
    fragments are generated inside the kernel threads (no 20 GB host arrays), and the time spent in the
    generator is reported so it can be taken out of the kernel phase."""
    import numpy as np
    from heavydb_amd import capi
    from heavydb_amd import synth as synth_mod
    from oracle import oracle as orc
    plan = info["ra"].to_plan()
    full = {"cfg1": 100_000_000, "cfg2": 1_000_000_000}.get(cfg, 1_000_000_000)
    rows = int(sample_rows) if sample_rows else full
    q = orc.qmd_init(plan)
    table_bytes = max(int(orc.buffer_bytes(q)), 1)
    # threads = kernels in flight = private output buffers: nproc, bounded by half of the free host
    # memory (a 640 MB table per kernel for cfg3) and by 64 (the reference's default would be
    # 2 x hardware_concurrency, thread_count.h:25-28; more tables than that only adds reduce time)
    host = os.cpu_count() or 1
    threads = orc.host_threads_for_tables(table_bytes, want=min(host, 64))
    n_frags = (rows + 31_999_999) // 32_000_000
    frag_rows = 32_000_000
    if n_frags < threads:  # fewer fragments than cores: smaller fragments keep every thread busy
        frag_rows = max((rows + threads - 1) // threads, 1 << 20)
    join = None
    inner = []
    build_s = None
    if cfg == "cfg4":
        m = info["dim_rows"]
        mul = info.get("dim_mul", 1)
        span = info.get("key_span", m)
        dim_k = synth_mod.dim_keys_with_holes(np, span, mul, info.get("dim_holes", 0))
        assert len(dim_k) == m
        g = info["dim_w_gen"]
        dim_w = orc.generate_column(m, g[0], g[1], g[2], g[3], g[4], g[5])
        t0 = time.perf_counter()
        join = orc.OracleJoin(dim_k, capi.INT64, 0, (span - 1) * mul)
        build_s = time.perf_counter() - t0
        inner = [dim_k, dim_w]
        plan.join_table = None
    t0 = time.perf_counter()
    _, _, code, tm = orc.execute_streamed(plan, info["gens"], rows, frag_rows=frag_rows, inner_cols=inner, join=join,
                                          n_threads=threads, reduce_threads=min(host, 64))
    dt = time.perf_counter() - t0
    assert code == 0, code
    scan_s = max(tm["kernels_s"] - tm["generate_s"], 1e-9)
    out = {"value": rows / dt, "unit": "rows/s", "cores": threads, "kind": "port", "host_cores": host,
           "sample": f"{rows} rows of {cfg} ({(rows + frag_rows - 1) // frag_rows} fragments x {frag_rows} rows, one kernel "
                     f"per fragment on {threads} host threads with a private {table_bytes / 1e6:.0f} MB output buffer each, "
                     f"then reduce in order), {dt:.2f} s",
           "phases_s": {"buffer_init": tm["init_s"], "kernels_incl_generation": tm["kernels_s"],
                        "generation": tm["generate_s"], "reduce": tm["reduce_s"]},
           "kernel_phase_rows_per_s": rows / scan_s,
           "init_plus_reduce_s": tm["init_s"] + tm["reduce_s"]}
    if build_s is not None:
        out["join_build_s"] = build_s
    return out


def measure_ceiling(torch, device_id: int) -> dict:
    """What this GPU's HBM delivers to the two simplest streams, measured here and now (SURVEY 8(d):
    "a measured ceiling alongside the 8 TB/s spec"): a read-only scan (the library's own COUNT(*) WHERE
    kernel over 4 GB: 16-byte non-temporal loads, nothing written) and a device-to-device copy of 4 GB
    (read + write, torch's copy kernel)."""
    from heavydb_amd import synth
    from heavydb_amd.executor import Executor
    out = {}
    try:
        n = 1 << 30
        ra, fr, _ = synth.cfg1(torch, n, 0, 1, device_id)
        ex = Executor(device_id)
        ex.executeWorkUnit(ra, fr)
        best = 1e9
        for _ in range(5):
            rs = ex.executeWorkUnit(ra, fr)
            best = min(best, rs.report.kernel_ms)
        out["read_gbs"] = round(4.0 * n / (best * 1e-3) / 1e9, 1)
        a = fr.keepalive[0].view(torch.int64)
        b = torch.empty_like(a)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.copy_(a)
        best = 1e9
        for _ in range(5):
            ev0.record()
            b.copy_(a)
            ev1.record()
            ev1.synchronize()
            best = min(best, ev0.elapsed_time(ev1))
        out["copy_gbs"] = round(2.0 * a.numel() * 8 / (best * 1e-3) / 1e9, 1)
        del a, b, fr, ra
        torch.cuda.empty_cache()
    except Exception as e:  # a report, never a reason to lose the bench line
        out["error"] = repr(e)
    return out


def _keyed_merge_path():
    from heavydb_amd import multi_gpu
    return multi_gpu.LAST_KEYED_PATH or None


DUMP_BUDGET_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 0


def dump_outputs(shard, out_dir: str, prefix: str = "", budget_bytes: int = DUMP_BUDGET_BYTES) -> None:
    """The rows a caller of the step receives (ResultSet.fetch), as float64 .npy files that two builds can be compared by:
      target<t>.npy    one column per target, SQL NULL as NaN (integers are exact up to 2^53)
      row_index.npy    which rows these are: the rows are sorted by their target values (target 0 first), so that builds
                       that lay the table out differently agree row for row; past the budget, a fixed seeded sample
      row_count.npy    the number of rows, target_sums.npy: per target, the sum over every row (NULLs left out)
    Floating-point aggregates are summed in no fixed order on the device: from run to run they agree to a few ulps, not
    bit for bit, so compare them with a tolerance."""
    import numpy as np
    rs = shard.result_set()
    q = rs.getQueryMemDesc()
    ival, dval, nul = rs.fetch()
    n, nt = ival.shape
    raw = [dval[:, t] if q.target_is_fp[t] else ival[:, t] for t in range(nt)]
    order = np.lexsort(raw[::-1]) if n else np.zeros(0, dtype=np.int64)
    cols = []
    for t in range(nt):
        c = raw[t][order].astype(np.float64)
        c[nul[order, t] != 0] = np.nan
        cols.append(c)
    keep = max((budget_bytes - (1 << 20)) // (8 * (nt + 1)), 1)
    idx = np.arange(n)
    if n > keep:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, keep, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    for t, c in enumerate(cols):
        np.save(os.path.join(out_dir, f"{prefix}target{t}.npy"), c[idx])
    np.save(os.path.join(out_dir, f"{prefix}row_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, f"{prefix}row_count.npy"), np.array([n], dtype=np.float64))
    np.save(os.path.join(out_dir, f"{prefix}target_sums.npy"), np.array([np.nansum(c) for c in cols], dtype=np.float64))


def main():
    args = parse_args()
    import torch
    from heavydb_amd import capi, synth
    from heavydb_amd.executor import Executor
    from heavydb_amd.multi_gpu import HipShard, merge

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves, one process per GPU, the way the
        # driver does (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...)
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)", file=sys.stderr)
        sys.exit(2)
    if args.hostsim:
        _bind_host_simulation(torch)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.hostsim:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device(f"cuda:{local_rank}"))
    torch.cuda.set_device(local_rank)
    if args.hostsim:
        local_rank = 0  # (one simulated device per process)
    lib = capi.load_library()  # fails loudly if the HIP extension is missing
    import ctypes as C
    name = C.create_string_buffer(256)
    cus, tot, free, clk, bus = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
    capi.check(lib.mi355q_device_info(local_rank, name, C.byref(cus), C.byref(tot), C.byref(free),
                                      C.byref(clk), C.byref(bus)))

    cfg = args.config
    want = int(args.rows) if args.rows else synth.DEFAULT_ROWS[cfg]
    bpr = {"cfg1": 4, "cfg2": 12, "cfg3": 16, "cfg3f": 20, "cfg4": 16}[cfg]
    total_rows = want if args.hostsim else fit_rows(cfg, want, world, free.value, bpr)
    if world > 1:  # all ranks must agree
        t = torch.tensor([total_rows], dtype=torch.int64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        total_rows = int(t.item())

    ceiling = measure_ceiling(torch, local_rank) if args.full and rank == 0 and not args.hostsim else None

    prepart = bool(args.prepartitioned and cfg in ("cfg3", "cfg3f") and world > 1)
    extra = {"prepartitioned": True} if prepart else {}
    if cfg == "cfg4":
        extra = {"sparse": bool(args.sparse), "sum_dim": bool(args.sum_dim), "holes": int(args.holes)}
    ra, fr, info = synth.CONFIGS[cfg](torch, total_rows, rank, world, local_rank, **extra)
    info["ra"] = ra
    if cfg == "cfg4":
        info["dim_rows"] = fr.inner_num_rows
    ex = Executor(local_rank)
    local_rows = sum(fr.num_rows)

    # the plan / input structs of the C-ABI are built once (as the reference compiles a step once); a step = one
    # mi355q_execute on them + the result storage it writes
    prep = HipShard.prepare(ex, ra, fr, kernel_variant=args.variant, force_generic=args.force_generic,
                            scratch_bytes=int(args.scratch_gb * 2**30), tune_overlap_cus=args.overlap_cus,
                            probe_keyed_passes=args.probe_passes, tune_blocks_per_cu=args.blocks_per_cu, flags=args.opt_flags)

    def step():
        sh = HipShard.execute_prepared(torch, prep)
        rep = sh.report
        if world > 1:
            sh = merge(sh, dist, torch, prepartitioned=prepart)
        return sh, rep

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the very first call allocates the partition scratch, the event pool and sets the LDS limits of the
    # kernels: timed once and reported (cold_first_call_ms), never part of `value`
    last = None
    cold_ms = None
    if args.warmup > 0:
        sync()
        t_cold = time.perf_counter()
        last = step()
        sync()
        cold_ms = (time.perf_counter() - t_cold) * 1e3
    for _ in range(max(args.warmup - 1, 0)):
        last = step()
    sync()
    reports = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
        reports.append(last[1])
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed * 1e3 / max(args.steps, 1)
    rows_per_s = total_rows * args.steps / elapsed

    if args.dump_outputs:
        dump_outputs(last[0], args.dump_outputs, prefix=f"rank{rank}_" if world > 1 else "",
                     budget_bytes=DUMP_BUDGET_BYTES // world)

    # N > 1: one more, UNTIMED step taken apart on every rank — the rank's own step, then the merge — so that the line
    # shows where a rank's time goes (the timed loop above has no sync between the two)
    per_rank = None
    if world > 1 and args.full:
        from heavydb_amd import multi_gpu
        sync()
        t1 = time.perf_counter()
        sh1 = HipShard.execute(torch, ex, ra, fr, kernel_variant=args.variant, force_generic=args.force_generic,
                               scratch_bytes=int(args.scratch_gb * 2**30), tune_overlap_cus=args.overlap_cus)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        merge(sh1, dist, torch, prepartitioned=prepart)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        r1 = sh1.report
        mine = {"rank": rank, "rows": local_rows, "step_ms": round((t2 - t1) * 1e3, 3), "merge_ms": round((t3 - t2) * 1e3, 3),
                "kernel": r1.kernel_name.decode(), "kernel_ms_per_launch": round(float(r1.kernel_ms) / max(int(r1.n_launches), 1), 3),
                "launches": int(r1.n_launches),
                "roofline_frac": round(float(r1.algorithmic_bytes) / max(float(r1.kernel_ms), 1e-9) / 1e6 / HBM_PEAK_GBS, 4),
                "merge_bytes_sent": int(multi_gpu.LAST_MERGE_BYTES_SENT), "keyed_merge": multi_gpu.LAST_KEYED_PATH or None}
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        per_rank = gathered

    # dominant kernel roofline (rank 0's launches; HIP events on the launch stream)
    k_ms = sum(r.kernel_ms for r in reports)
    k_n = sum(max(r.n_launches, 1) for r in reports)
    avg_ms = k_ms / max(k_n, 1)
    alg_bytes_launch = sum(r.algorithmic_bytes for r in reports) / max(k_n, 1)
    achieved = alg_bytes_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    kname = reports[-1].kernel_name.decode() if reports else ""
    # HBM bytes per launch from the committed rocprofv3 --pmc passes (profiles/traffic.json:
    # FETCH_SIZE x 2 per the gfx950 correction + WRITE_SIZE, per input row of that kernel)
    traffic = None
    traffic_source = None
    try:
        import hashlib
        with open(args.traffic_json) as f:
            tall = json.load(f)
        tj = tall.get(kname)
        # the counters belong to ONE build of the kernel: the file records the hash of the kernel source it was
        # measured on (tools/make_traffic_json.py), and a build whose source differs reports no traffic rather than
        # a number that can no longer notice a regression.  The PMC passes are taken on the default workload only.
        src = os.path.join(ROOT, "heavydb_amd", "csrc", "kernels_part.hip")
        sha = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
        if tj and k_n and cfg == "cfg3f":
            if tall.get("kernel_source_sha16") == sha:
                rows_per_launch = sum(r.rows_scanned for r in reports) / k_n
                traffic = tj["hbm_bytes_per_row"] * rows_per_launch
                traffic_source = "rocprofv3 --pmc passes of this build (kernels_part.hip " + sha + "): " + tj.get("from", "")[:160]
            else:
                traffic_source = "none: profiles/traffic.json was measured on another build of kernels_part.hip"
    except Exception:
        pass

    # what the partition-then-aggregate scheme can reach at best on THIS box: per input row 20 B read,
    # s x 16 B of records written, R x s x 16 B of records read back, each at the rate the box measures for that
    # kind of traffic (reads: the scan kernel; writes: derived from the copy rate, a copy being one read + one write)
    scheme_ceiling = None
    if cfg == "cfg3f" and ceiling and ceiling.get("read_gbs") and ceiling.get("copy_gbs"):
        rd = ceiling["read_gbs"]
        wr = 1.0 / max(2.0 / ceiling["copy_gbs"] - 1.0 / rd, 1e-9)
        sel, R = 0.5, 2
        ns_per_row = 20.0 / rd + sel * 16.0 / wr + R * sel * 16.0 / (0.93 * rd)
        scheme_ceiling = {"frac": 20.0 / ns_per_row / HBM_PEAK_GBS, "read_gbs": rd, "write_gbs": round(wr, 1),
                          "selectivity": sel, "sub_ranges": R,
                          "formula": "20 B / (20/read + s*16/write + R*s*16/(0.93*read)) / 8 TB/s"}

    verify = None
    if args.verify and rank == 0:
        rs = last[0].result_set()
        ival, dval, nul = rs.fetch()
        # timed_steps / launches: counted by the timed loop itself (its reports), not echoed from --steps
        verify = {"groups": int(ival.shape[0]), "timed_steps": len(reports), "launches": int(sum(r.n_launches for r in reports))}
        if cfg in ("cfg3", "cfg3f"):
            verify["sum_count"] = int(ival[:, 1].sum())
        if cfg == "cfg4":
            verify["slots"] = [int(x) for x in ival[0]]

    out = {
        # BASELINE.json's headline metric for the default workload; the other configs name their own query
        "metric": {"cfg3f": "rows/sec, filtered GROUP BY (key, COUNT(*), AVG(f64)) on 10 B int64-key rows",
                   "cfg1": "rows/sec, COUNT(*) WHERE i32 < k",
                   "cfg2": "rows/sec, GROUP BY (key, SUM(i64)) over 1 K int32 keys",
                   "cfg3": "rows/sec, unfiltered GROUP BY (key, COUNT(*), AVG(f64)) on int64 keys",
                   "cfg4": "rows/sec, fact JOIN dim + SUM"}.get(cfg, cfg),
        "value": rows_per_s,
        "unit": "rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "int64" if cfg != "cfg1" else "int32",
        "data": "synthetic (device-generated splitmix64 columns, 32 M-row fragments)",
        "config": {"workload": f"{cfg}: {total_rows} rows" + ("" if total_rows == want else f" (largest that fits; asked {want})"),
                   "bytes_per_row": bpr, "fragments_per_rank": len(fr.num_rows), "rows_per_rank": local_rows,
                   "prepartitioned_by_key": prepart, "keyed_merge": _keyed_merge_path() if world > 1 else None,
                   "kernel": kname, "variant": int(reports[-1].variant) if reports else 0,
                   "device": name.value.decode(), "cus": cus.value,
                   "hbm_reported_gbs": round(2 * clk.value * 1e3 * bus.value / 8 / 1e9, 1)},
        "achieved_gbs_whole_step": total_rows * bpr * args.steps / elapsed / 1e9,
        "cold_first_call_ms": cold_ms,
        # roofline: `achieved` credits the step's algorithmic bytes to the DOMINANT kernel's launches
        # only (the contract's definition); `whole_step_frac` divides the same bytes by the whole
        # step's wall time (every kernel + merge) and is the number to hold against the 0.70 target
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                     "kernel": kname, "avg_launch_ms": avg_ms, "algorithmic_bytes_per_launch": alg_bytes_launch,
                     "whole_step_achieved": total_rows * bpr * args.steps / elapsed / 1e9,
                     "whole_step_frac": total_rows * bpr * args.steps / elapsed / 1e9 / HBM_PEAK_GBS,
                     "scheme_ceiling_frac": scheme_ceiling["frac"] if scheme_ceiling else None,
                     "scheme_ceiling": scheme_ceiling,
                     "measured_ceiling": ceiling},
    }
    if per_rank:
        out["per_rank"] = per_rank
    out["ranks_reported_by_rccl"] = 1 if dist is None else dist.get_world_size()
    if args.hostsim:
        out["data"] = "HOST SIMULATION (tests/hostsim + gloo): control flow only, not a measurement"
    if verify:
        out["verify"] = verify
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.hostsim:
        try:
            out["cpu_baseline"] = cpu_baseline(cfg, info, args.cpu_seconds, int(args.cpu_rows))
        except Exception as e:  # the baseline is a report, never a reason to lose the bench line
            out["cpu_baseline"] = {"value": None, "unit": "rows/s", "cores": os.cpu_count(), "kind": "port",
                                   "sample": f"failed: {e!r}"}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
