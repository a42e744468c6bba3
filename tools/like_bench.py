#!/usr/bin/env python3
"""LIKE on the GPU, measured (profiles/r07_like.txt):
  (a) the matcher alone (vnm_strdict_like over every id of a dictionary) for the exact / prefix / suffix / contains / mixed
      shapes at 1e3, 1e5, 5e6 distinct ~11-byte values and 1e5 ~200-byte values;
  (b) WHERE s LIKE p over 5e8 rows of int32 codes: the mask kernel (vnm_project with the lookup) and the compaction
      (vnm_filter_mask), next to WHERE s = 'x' (a code comparison) on the same batch;
  (c) end to end from an Arrow table through vinum_amd.planner, next to the reference's algorithm (np.vectorize over
      re.match, vinum/core/functions.py:322-338) on a 1e6-row slice on the host.
Times: median of --reps runs, each bracketed by device synchronisation (warm-up runs first)."""
import argparse
import os
import re
import statistics
import sys
import time

import numpy as np
import pyarrow as pa
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def values(n, length, seed):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    raw = alpha[rng.integers(0, 26, (n, length))]
    raw[:, :3] = np.frombuffer(b"abc", np.uint8)          # a shared prefix: every value is a candidate for 'abc%'
    buf = raw.tobytes()
    offs = np.arange(n + 1, dtype=np.int32) * length
    return pa.Array.from_buffers(pa.string(), n, [None, pa.py_buffer(offs), pa.py_buffer(buf)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=float, default=5e8)
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops, planner
    from vinum_amd.core.base import DeviceRecordBatch
    from vinum_amd.device import DeviceBuffer, DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    lib = L.lib()
    print(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}")

    print("\n(a) matcher alone: vnm_strdict_like over every id")
    for n, length in ((1000, 11), (100_000, 11), (5_000_000, 11), (100_000, 200)):
        arr = values(n, length, 1)
        kd = KeyDictionary(pa.string())
        for s in range(0, n, 1 << 20):
            kd.encode(arr.slice(s, 1 << 20))
        top = int(lib.vnm_strdict_ids(kd.handle()))
        out = DeviceBuffer(top)
        one = arr[n // 2].as_py()
        shapes = {"exact": one, "prefix": "abc%", "suffix": "%" + one[-3:], "contains": "%" + one[4:7] + "%",
                  "mixed": "a_c%" + one[5] + "_" + one[7] + "%"}
        for name, p in shapes.items():
            raw = p.encode()
            t = timed(lambda: L.check(lib.vnm_strdict_like(kd.handle(), raw, len(raw), 1, 0, out.ptr, None)), args.reps)
            m = int(out.to_host(np.uint8, top).sum())
            print(f"  {n:>9d} values x {length:3d} B  {name:9s} {t * 1e3:9.3f} ms  {n / t / 1e9:7.2f} G values/s  ({m} match)")

    print(f"\n(b) WHERE over {args.rows:.0e} rows of int32 codes (dictionary of 64 values)")
    n = int(args.rows)
    words = [f"w{i:02d}{'J' if i % 3 == 0 else 'x'}" for i in range(64)]
    kd = KeyDictionary(pa.string())
    codes = np.unique(kd.encode(pa.array(words)).to_numpy(zero_copy_only=False)).astype(np.int32)
    rows = torch.from_numpy(codes).cuda()[torch.randint(0, len(codes), (n,), device="cuda")].contiguous()
    col = DeviceColumn.from_torch(rows)
    tab = kd.like_table("%J")
    eq_code = int(kd.code_of(words[3]))
    like_cols = {"s": col, "__t": tab}
    for name, expr, cols in (("LIKE '%J'", ("lookup", "s", "__t"), like_cols), ("= 'w03J'", ("eq", "s", eq_code), {"s": col})):
        t_mask = timed(lambda: ops.predicate_mask(expr, cols, n), args.reps)
        mask = ops.predicate_mask(expr, cols, n)
        t_comp = timed(lambda: ops.filter_mask(mask, None, n, [col]), args.reps)
        k = ops.filter_mask(mask, None, n, [col])[1]
        print(f"  {name:10s} mask {t_mask * 1e3:8.2f} ms ({n * 5 / t_mask / 1e12:5.2f} TB/s of codes + mask)  "
              f"compaction {t_comp * 1e3:8.2f} ms  total {(t_mask + t_comp) * 1e3:8.2f} ms  ({k} rows)")
    del rows, col, mask

    print("\n(c) end to end from an Arrow table")
    rng = np.random.default_rng(2)
    names = np.array(["Joseph", "Jonas", "Joe", "José", "Berlin", "Munich", "Riva", "Naples"] + [f"v{i}" for i in range(992)])
    for m in (1_000_000, 100_000_000):
        t = pa.table({"s": pa.array(names[rng.integers(0, len(names), m)])})
        q = {"select": ["s"], "where": ["like", "s", ["lit", "Jos%"]]}
        dt = timed(lambda: planner.execute(q, t), max(3, args.reps // 3), warm=1)
        print(f"  GPU planner   {m:>11d} rows  {dt * 1e3:9.1f} ms  {m / dt / 1e6:9.1f} M rows/s")
    sl = t.slice(0, 1_000_000)["s"].to_numpy(zero_copy_only=False).astype("U")
    pat = re.compile("^" + "Jos%".replace("_", ".").replace("%", ".*") + "$")
    f = np.vectorize(lambda v: bool(pat.match(v)) != False)   # noqa: E712  (the reference's re_lambda)
    t0 = time.perf_counter()
    f(sl)
    dt = time.perf_counter() - t0
    print(f"  host np.vectorize(re.match)  1000000 rows  {dt * 1e3:9.1f} ms  {1e6 / dt / 1e6:9.1f} M rows/s  (the reference's per-row match)")


if __name__ == "__main__":
    main()
