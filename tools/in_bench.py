#!/usr/bin/env python3
"""IN lists on the GPU, measured (profiles/r09_in_set.txt): the mask of `x IN (v1 .. vm)` over --rows resident int64 rows at
selectivity 0.5,
  (a) as the projection interpreter's OR chain of `==` (m = 2, 4, 8, 16: what compiles) -- run this file with --tree <checkout of
      the parent commit> --chain-only for the baseline the threshold is judged against;
  (b) as a set probe plus the `mask != 0` program (VNM_IN_SET_MIN=2) for the same m, and for m = 17, 100, 4096, 4097, 1e5, 1e6,
      members scattered (sorted table: LDS up to 4096 members, then global memory) and dense (bitmap: LDS up to 32 KB);
  (c) the probe kernel alone (vnm_in_set_probe), so the share of the extra mask pass (1 B/row written, 1 B/row read next to
      8 B/row of column) is the difference;
  (d) a float64 column against a float list;
  (e) next to the mask of a numeric `=` over two int32 columns of the same length, the yardstick of tools/strcmp_bench.py;
  (f) np.isin on the host for the same lists over the first --cpu-rows rows.
The column holds multiples of the members' spacing drawn from twice the members' count, so every second row is a member.
Times: median (min .. max) of --reps runs, each bracketed by device synchronisation, after warm-up runs."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def show(label, t, rows, extra=""):
    med, lo, hi = t
    print(f"{label:58s} {med:9.3f} ms  ({lo:8.3f} .. {hi:8.3f}; spread {100 * (hi - lo) / med:5.1f} %)  {rows / med / 1e6:8.1f} Grows/s {extra}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=float, default=5e8)
    ap.add_argument("--cpu-rows", type=float, default=2e7)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="import vinum_amd from this checkout (the parent commit's, for the chain baseline)")
    ap.add_argument("--chain-only", action="store_true", help="only what a tree without set probes can run: (a) and (e)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.device import DeviceColumn
    n = int(args.rows)
    os.environ.pop("VNM_IN_SET_MIN", None)
    print(f"# tree {os.path.abspath(args.tree)}  rows {n}  reps {args.reps}  device {torch.cuda.get_device_name(0)}", flush=True)

    def route():
        buf = (ctypes.c_char * 512)()
        L.lib().vnm_route_last(buf, 512)
        return buf.value.decode().split(":")[1] if buf.value.startswith(b"in_set") else "?"

    # (e) the yardstick
    p = torch.randint(0, 2, (n,), dtype=torch.int32, device="cuda")
    q = torch.randint(0, 2, (n,), dtype=torch.int32, device="cuda")
    cols = {"p": DeviceColumn.from_torch(p), "q": DeviceColumn.from_torch(q)}
    show("numeric = over two int32 columns (8 B/row read)", timed(lambda: ops.project(("eq", "p", "q"), cols), args.reps), n)
    del p, q, cols

    def column(m, spacing, dtype=torch.int64):
        x = torch.randint(0, 2 * m, (n,), dtype=torch.int64, device="cuda") * spacing
        return x if dtype == torch.int64 else x.to(dtype) / 2

    def members(m, spacing):
        return tuple(int(v) for v in (np.arange(m, dtype=np.int64) * 2 * spacing))

    cpu_n = int(min(args.cpu_rows, n))

    def cpu(x, vals, label):
        host = x[:cpu_n].cpu().numpy()
        arr = np.array(vals)
        t0 = time.perf_counter()
        got = np.isin(host, arr)
        dt = (time.perf_counter() - t0) * 1e3
        print(f"{label:58s} {dt:9.1f} ms for {cpu_n} rows = {dt * n / cpu_n:10.1f} ms per {n} rows (scaled)  selectivity {got.mean():.3f}", flush=True)

    for m in (2, 4, 8, 16):
        x = column(m, 1000)
        c = {"x": DeviceColumn.from_torch(x)}
        vals = members(m, 1000)
        os.environ["VNM_IN_SET_MIN"] = "17"                   # (whatever the default: the chain)
        show(f"chain   m={m:<8d} scattered", timed(lambda: ops.project(("in", "x", vals), c), args.reps), n)
        if not args.chain_only:
            os.environ["VNM_IN_SET_MIN"] = "2"
            t = timed(lambda: ops.project(("in", "x", vals), c), args.reps)
            show(f"set     m={m:<8d} scattered  probe + mask program", t, n, route())
            show(f"set     m={m:<8d} scattered  probe kernel alone", timed(lambda: ops.in_set_probe(c["x"], vals), args.reps), n, route())
            dense = members(m, 1)
            xd = {"x": DeviceColumn.from_torch(column(m, 1))}
            show(f"set     m={m:<8d} dense      probe + mask program", timed(lambda: ops.project(("in", "x", dense), xd), args.reps), n, route())
            os.environ.pop("VNM_IN_SET_MIN", None)
            if m == 16:
                cpu(x, vals, f"np.isin m={m} scattered")
        del x, c
    if args.chain_only:
        return
    for m in (17, 100, 4096, 4097, 100_000, 1_000_000):
        for kind, spacing in (("scattered", 1000), ("dense", 1)):
            x = column(m, spacing)
            c = {"x": DeviceColumn.from_torch(x)}
            vals = members(m, spacing)
            ops.in_set(vals)                                  # (the upload is once per list, outside the timed window)
            show(f"set     m={m:<8d} {kind:9s}  probe + mask program", timed(lambda: ops.project(("in", "x", vals), c), args.reps), n, route())
            show(f"set     m={m:<8d} {kind:9s}  probe kernel alone", timed(lambda: ops.in_set_probe(c["x"], vals), args.reps), n, route())
            if kind == "scattered" or m == 100_000:
                cpu(x, vals, f"np.isin m={m} {kind}")
            del x, c
    for m in (100, 4096, 100_000):
        x = column(m, 1000, torch.float64)
        c = {"x": DeviceColumn.from_torch(x)}
        vals = tuple(v / 2 for v in members(m, 1000))
        show(f"set     m={m:<8d} float64    probe + mask program", timed(lambda: ops.project(("in", "x", vals), c), args.reps), n, route())
        if m == 4096:
            cpu(x, vals, f"np.isin m={m} float64")
        del x, c


if __name__ == "__main__":
    main()
