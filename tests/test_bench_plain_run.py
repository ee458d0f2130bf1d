"""A plain `python bench.py --gpus 1 --steps N --warmup W` times exactly N steps; `--dump-outputs DIR` writes the rows of
the last timed step, the same from run to run.  Run here with --hostsim (the library's real device sources compiled for the
CPU): control flow only, not a measurement.  (What a plain run leaves to --full: tests/test_bench_multi_rank.py.)"""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _run_bench(dump_dir, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--rows", "500000", "--hostsim", "--verify", "--dump-outputs", str(dump_dir), *extra], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _arrays(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    from tests.helpers import hostsim_lib
    hostsim_lib(real_fast=True)
    d = _run_bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["verify"]["timed_steps"] == 3                              # counted by the timed loop
    assert d["verify"]["launches"] > 0 and d["verify"]["launches"] % 3 == 0
    assert d["value"] > 0 and d["unit"] == "rows/s" and d["higher_is_better"] is True and d["dtype"] == "int64"
    a = _arrays(tmp_path / "a")
    assert set(a) == {"target0.npy", "target1.npy", "target2.npy", "row_index.npy", "row_count.npy", "target_sums.npy"}
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 << 20
    n = int(a["row_count.npy"][0])
    assert n == d["verify"]["groups"] == len(a["target0.npy"])
    assert np.all(np.diff(a["target0.npy"]) > 0)                       # rows sorted by key
    assert a["target1.npy"].sum() == a["target_sums.npy"][1] == d["verify"]["sum_count"]
    _run_bench(tmp_path / "b")                                          # same arguments, same inputs: same outputs
    again = _arrays(tmp_path / "b")
    assert set(again) == set(a) and all(np.array_equal(a[f], again[f], equal_nan=True) for f in a)


class _FakeResult:
    def __init__(self, ival, dval, nul, fp):
        self._rows, self._q = (ival, dval, nul), SimpleNamespace(target_is_fp=fp)

    def getQueryMemDesc(self):
        return self._q

    def fetch(self):
        return self._rows


def test_dump_outputs_samples_a_large_result_with_a_fixed_seed(tmp_path):
    rng = np.random.default_rng(7)
    n = 50_000
    keys = rng.permutation(n).astype(np.int64) * 3 + 1
    ival = np.stack([keys, rng.integers(1, 100, n), np.zeros(n, np.int64)], axis=1)
    dval = np.stack([np.zeros(n), np.zeros(n), rng.random(n)], axis=1)
    nul = np.zeros((n, 3), np.int8)
    nul[5, 2] = 1
    shard = SimpleNamespace(result_set=lambda: _FakeResult(ival, dval, nul, [0, 0, 1]))
    budget = (1 << 20) + 32 * 10_000                                     # room for 10 000 rows of 3 targets + their index
    for sub in ("a", "b"):
        bench.dump_outputs(shard, str(tmp_path / sub), budget_bytes=budget)
    a, b = _arrays(tmp_path / "a"), _arrays(tmp_path / "b")
    assert all(np.array_equal(a[f], b[f], equal_nan=True) for f in a)
    idx = a["row_index.npy"].astype(np.int64)
    assert len(idx) == 10_000 and np.all(np.diff(idx) > 0) and idx[-1] < n
    order = np.argsort(keys)
    np.testing.assert_array_equal(a["target0.npy"], keys[order][idx].astype(np.float64))
    np.testing.assert_array_equal(a["target1.npy"], ival[order, 1][idx].astype(np.float64))
    want_avg = dval[order, 2].copy()
    want_avg[np.argsort(order)[5]] = np.nan
    np.testing.assert_array_equal(a["target2.npy"], want_avg[idx])
    assert a["row_count.npy"][0] == n and a["target_sums.npy"][1] == ival[:, 1].sum()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= budget
