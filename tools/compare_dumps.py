#!/usr/bin/env python
"""Compare the `bench.py --dump-outputs DIR` files of two builds (same workload, same seeds):

    python tools/compare_dumps.py DIR_A DIR_B [out.json]

Row count and target_sums must be equal, every column identical or (floating-point aggregates, summed in no fixed order on
the device) within 1e-9 relative.  Prints one JSON line, writes it to out.json, exits non-zero when they differ."""
import json
import os
import sys

import numpy as np


def main():
    a, b = sys.argv[1], sys.argv[2]
    ld = lambda d, f: np.load(os.path.join(d, f))
    out = {"row_count": [float(ld(a, "row_count.npy")[0]), float(ld(b, "row_count.npy")[0])]}
    sa, sb = ld(a, "target_sums.npy"), ld(b, "target_sums.npy")
    out["target_sums_a"] = [repr(float(x)) for x in sa]
    out["target_sums_b"] = [repr(float(x)) for x in sb]
    out["target_sums_rel"] = [float(abs(x - y) / max(abs(x), abs(y), 1e-300)) for x, y in zip(sa, sb)]
    ok = out["row_count"][0] == out["row_count"][1] and np.array_equal(ld(a, "row_index.npy"), ld(b, "row_index.npy"))
    ok = ok and all(r <= 1e-9 for r in out["target_sums_rel"])
    for t in range(len(sa)):
        ca, cb = ld(a, f"target{t}.npy"), ld(b, f"target{t}.npy")
        same_shape = ca.shape == cb.shape
        ident = bool(same_shape and np.array_equal(ca, cb, equal_nan=True))
        close = bool(same_shape and np.array_equal(np.isnan(ca), np.isnan(cb)) and
                     np.all(np.abs(ca - cb)[~np.isnan(ca)] <= 1e-9 * np.maximum(np.abs(ca), np.abs(cb))[~np.isnan(ca)]))
        out[f"target{t}"] = {"rows": int(ca.shape[0]), "identical": ident, "within_1e-9": close}
        ok = ok and close
    out["ok"] = bool(ok)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
