#!/usr/bin/env python3
"""Arithmetic on temporal values and is_busday() on the device, measured (profiles/r16_temporal_arith.txt), over --rows resident rows:
  (a) vnm_temporal_affine over two non-null int64 columns (8 + 8 bytes in, 8 bytes + 1 validity bit out: 24.1 bytes per row) against
      the projection interpreter's program computing the same integers, ("sub", ("mul", "a", ka), "b") over the same columns typed
      int64 (8 + 8 in, 8 out: 24 bytes per row) -- what `dropoff - pickup` ran as before it was typed; the expectation is a ratio near
      1, and the run-to-run spread (max - min of the repetitions over the median) stands next to it;
  (b) the same kernel over ONE column (16.1 bytes per row) against vnm_temporal_rescale over that column (16): near 1; two columns
      against one: near 24.1 / 16.1 = 1.5;
  (c) vnm_temporal_busday (4 bytes in, 1 out) with 0 and 8192 holidays against the IN probe's mask (vnm_in_set_probe, sorted route
      in LDS) over the same int32 rows and the same 8192 days;
  (d) NumPy on one host thread for each of (a) to (c) over --host-rows rows, scaled to --rows; and WHERE dropoff - pickup >
      timedelta(30, 'm') next to a plain WHERE a > b over the same two columns.
Times: median of --reps runs, each bracketed by device synchronisation, after warm-up runs.  Two asymmetries to read the report with:
in (a) the interpreter's side (ops.project) takes its output from the caching pool inside every repetition while the kernel writes
into a preallocated buffer, which favours the kernel; the host baselines of (d) are single runs without a spread."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import pyarrow as pa
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_all(fn, reps, warmup=2):
    """the repetitions' times in seconds, each bracketed by device synchronisation"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--host-rows", type=float, default=1e7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.core.base import DeviceRecordBatch
    from vinum_amd.core.lowering import lower_dictionary, used_columns
    from vinum_amd.device import DeviceBuffer, DeviceColumn
    lib = L.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def med(ts):
        return float(np.median(ts))

    def spread(ts):
        return (max(ts) - min(ts)) / med(ts)

    def line(what, ts, nbytes):
        return f"{what} {med(ts) * 1e3:7.3f} ms ({nbytes / med(ts) / 1e12:5.2f} TB/s, spread {spread(ts) * 100:4.1f} %)"

    n, nh = int(args.rows), int(args.host_rows)
    say(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}  rows={n:.0e}  host rows={nh:.0e}")
    gen = torch.Generator(device="cuda").manual_seed(16)
    pickup_t = torch.randint(1_600_000_000, 1_603_000_000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    dropoff_t = pickup_t * 1000 + torch.randint(0, 3 * 3600 * 1000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    pickup, dropoff = DeviceColumn.from_torch(pickup_t, pa.timestamp("s")), DeviceColumn.from_torch(dropoff_t, pa.timestamp("ms"))
    a_i64, b_i64 = DeviceColumn.from_torch(pickup_t), DeviceColumn.from_torch(dropoff_t)
    out64, bitmap = DeviceBuffer(n * 8), DeviceBuffer((n + 7) >> 3)
    da, db = pickup.dcol(), dropoff.dcol()

    say("\n(a) dropoff[ms] - pickup[s]: vnm_temporal_affine (24.1 B / row) against the interpreter's untyped program (24 B / row)")

    def affine2():
        L.check(lib.vnm_temporal_affine(ctypes.byref(db), 1, ctypes.byref(da), -1000, 0, n, 8, out64.ptr, bitmap.ptr, None, None))

    def interpreter():
        return ops.project(("sub", "b", ("mul", "a", 1000)), {"a": a_i64, "b": b_i64}, n)
    t2, ti = timed_all(affine2, args.reps), timed_all(interpreter, args.reps)
    affine2()
    same = bool((torch.from_numpy(out64.to_host(np.int64, 1 << 20)).cuda() == (dropoff_t - pickup_t * 1000)[:1 << 20]).all())
    assert same and (interpreter().to_numpy()[:1 << 20] == out64.to_host(np.int64, 1 << 20)).all()
    say("  " + line("vnm_temporal_affine, two columns", t2, n * 24.125))
    say("  " + line("interpreter, sub(b, mul(a, 1000))", ti, n * 24) + f"   ratio {med(t2) / med(ti):5.2f} (bytes: 1.01)")

    say("\n(b) one column: vnm_temporal_affine (16.1 B / row) against vnm_temporal_rescale (16 B / row), s -> ms")

    def affine1():
        L.check(lib.vnm_temporal_affine(ctypes.byref(da), 1000, None, 0, 0, n, 8, out64.ptr, bitmap.ptr, None, None))

    def rescale():
        L.check(lib.vnm_temporal_rescale(ctypes.byref(da), 1000, 1, n, 8, out64.ptr, None))
    t1, tr = timed_all(affine1, args.reps), timed_all(rescale, args.reps)
    say("  " + line("vnm_temporal_affine, one column ", t1, n * 16.125))
    say("  " + line("vnm_temporal_rescale            ", tr, n * 16) + f"   ratio {med(t1) / med(tr):5.2f} (bytes: 1.01)")
    say(f"  two columns against one: {med(t2) / med(t1):5.2f} (bytes: {24.125 / 16.125:4.2f})")

    say("\n(c) is_busday over int32 days: vnm_temporal_busday (5 B / row) against the IN probe's mask over the same rows and days")
    days_t = (pickup_t // 86400).to(torch.int32) - torch.randint(0, 30_000, (n,), device="cuda", dtype=torch.int32, generator=gen)
    days = DeviceColumn.from_torch(days_t, pa.date32())
    dd = days.dcol()
    mask = DeviceBuffer(n)
    every = np.busdaycalendar("1111100", np.arange(-12_000, 19_000).astype("datetime64[D]")).holidays[:8192]
    hol = every.astype(np.int64).astype(np.int32)
    hol_dev = DeviceBuffer.from_host(hol)
    members = tuple(int(x) for x in hol[::3]) + tuple(int(x) + 100_000 for x in hol[1::3]) + tuple(int(x) - 100_000 for x in hol[2::3])

    def busday(count):
        return lambda: L.check(lib.vnm_temporal_busday(ctypes.byref(dd), n, 31, hol_dev.ptr, count, mask.ptr, None))

    def probe():
        return ops.in_set_probe(days, members, length=n)
    tb0, tb1, tp = timed_all(busday(0), args.reps), timed_all(busday(8192), args.reps), timed_all(probe, args.reps)
    busday(8192)()
    got = mask.to_host(np.uint8, 1 << 20).astype(bool)
    assert (got == np.is_busday(days_t[:1 << 20].cpu().numpy().astype(np.int64).view("datetime64[D]"), holidays=every)).all()
    say("  " + line("vnm_temporal_busday,    0 holidays", tb0, n * 5))
    say("  " + line("vnm_temporal_busday, 8192 holidays", tb1, n * 5) + f"   {med(tb1) / med(tb0):5.2f} x the empty list")
    say("  " + line("vnm_in_set_probe, 8192 members    ", tp, n * 5) + f"   busday / probe {med(tb1) / med(tp):5.2f}")

    say(f"\n(d) NumPy on one host thread over {nh:.0e} rows, scaled to {n:.0e}; and the WHERE query")
    hp = pickup_t[:nh].cpu().numpy().view("datetime64[s]")
    hd = dropoff_t[:nh].cpu().numpy().view("datetime64[ms]")
    hdays = days_t[:nh].cpu().numpy().astype(np.int64).view("datetime64[D]")
    scale = n / nh

    def host(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * scale
    h2, h1 = host(lambda: hd - hp), host(lambda: hp.astype("datetime64[ms]"))
    hb0, hb1 = host(lambda: np.is_busday(hdays)), host(lambda: np.is_busday(hdays, holidays=every))
    say(f"  dropoff - pickup       {h2 * 1e3:9.1f} ms = {h2 / med(t2):6.0f} x vnm_temporal_affine")
    say(f"  pickup.astype(ms)      {h1 * 1e3:9.1f} ms = {h1 / med(t1):6.0f} x vnm_temporal_affine over one column")
    say(f"  np.is_busday, 0 / 8192 holidays {hb0 * 1e3:9.1f} / {hb1 * 1e3:9.1f} ms = {hb0 / med(tb0):6.0f} x / {hb1 / med(tb1):6.0f} x vnm_temporal_busday")
    batch = DeviceRecordBatch({"pickup": pickup, "dropoff": dropoff, "a": a_i64, "b": b_i64}, n)

    def where(pred):
        low, extra = lower_dictionary(pred, batch.columns)
        return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)
    p0, p1 = ("gt", "b", "a"), ("gt", ("sub", "dropoff", "pickup"), ("timedelta", 30, ("lit", "m")))
    w0, w1 = timed_all(lambda: where(p0), args.reps), timed_all(lambda: where(p1), args.reps)
    k1 = int(where(p1).to_host(np.uint8, n).sum(dtype=np.int64))
    assert k1 == int((dropoff_t - pickup_t * 1000 > 1_800_000).sum())
    say(f"  WHERE b > a                                   {med(w0) * 1e3:8.2f} ms (spread {spread(w0) * 100:4.1f} %)")
    say(f"  WHERE dropoff - pickup > timedelta(30, 'm')   {med(w1) * 1e3:8.2f} ms (spread {spread(w1) * 100:4.1f} %)   {med(w1) / med(w0):5.2f} x   ({k1} rows)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
