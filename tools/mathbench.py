#!/usr/bin/env python3
"""Time the built-in scalar functions in the projection kernel against the `v*2+1` reference point (same process, same
columns), and sum(sqrt(v)) against sum(v*2) in the aggregate.  Prints one line per case.

    python tools/mathbench.py [--rows 1e9] [--groups 1e6] [--reps 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402

from vinum_amd import ops  # noqa: E402
from vinum_amd import _lib as L  # noqa: E402
from vinum_amd.device import DeviceColumn  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--groups", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = int(args.rows)
    g = torch.Generator(device="cuda").manual_seed(0)
    v = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1000 + 1e-3
    k = torch.randint(0, int(args.groups), (n,), dtype=torch.int64, device="cuda", generator=g)
    cols = {"v": DeviceColumn.from_torch(v), "k": DeviceColumn.from_torch(k)}
    # the reference point is timed first AND last: the first call of a size also grows the library's memory pool
    cases = [("v*2+1", ("add", ("mul", "v", 2), 1)), ("abs(v)", ("abs", "v")), ("sqrt(v)", ("sqrt", "v")),
             ("to_int(v)", ("to_int", "v")), ("to_float(k)", ("to_float", "k")), ("sin(v)", ("sin", "v")),
             ("log(v)", ("log", "v")), ("power(v, 2.5)", ("power", "v", 2.5)), ("v*2+1 (again)", ("add", ("mul", "v", 2), 1))]
    times = {}
    print(f"# projection over {n:.3g} rows (float64 / int64 in, 8-byte result out), median of {args.reps}")
    for name, e in cases:
        c = {x: cols[x] for x in ops.columns_of(e)}
        times[name] = timed(lambda: ops.project(e, c, length=n), args.reps)
    base = min(times["v*2+1"], times["v*2+1 (again)"])
    for name, ms in times.items():
        print(f"{name:16s} {ms:8.3f} ms  {16 * n / ms / 1e9:6.2f} TB/s  x{ms / base:5.3f} of v*2+1 (the faster of its two runs)", flush=True)
    # sum(v*2) is evaluated in registers by the hot kernels; sum(sqrt(v)) is projected into a column first (one more
    # 16 GB pass), then aggregated
    print(f"# aggregate: SELECT k, sum(<expr>) GROUP BY k, G = {args.groups:.3g}")
    ref = None
    for name, e in [("sum(v*2)", ("mul", "v", 2)), ("sum(sqrt(v))", ("sqrt", "v"))]:
        def run():
            agg = ops.DeviceAggregate(L.SINGLE_NUMERICAL, [pa.int64()], [(L.SUM, 10_000, pa.float64())],
                                      expected_groups=int(args.groups))
            agg.set_input_expr(0, e, ["v"])
            agg.next([cols["k"]], [None], nrows=n, expr_cols=[cols["v"]])
            agg.finish()
            agg.close()
        ms = timed(run, args.reps)
        ref = ref or ms
        print(f"{name:16s} {ms:8.3f} ms  x{ms / ref:5.3f} of sum(v*2)", flush=True)


if __name__ == "__main__":
    main()
