#!/usr/bin/env python3
"""date() / datetime() through the device dictionary, measured (profiles/r15_datetime.txt):
  (a) the row pass vnm_strdict_gather_temporal (4 code bytes in, 8 value bytes + 1 validity bit out: 12.1 bytes per row) against
      vnm_strdict_gather_codes (4 in, 4 out: 8 bytes per row) over the SAME codes in the same run, at 4096 and 1e7 distinct 19-byte
      values over --rows resident rows; the expectation is a ratio near 12.1 / 8 = 1.5, and the run-to-run spread (max - min of the
      repetitions over the median) stands next to it;
  (b) parsing 1e7 distinct values -- vnm_strdict_parse_datetime over the whole dictionary, the first time (the tables are allocated)
      and again -- against np.array(values, dtype='datetime64[s]') on one host thread over the same values;
  (c) WHERE date(d) >= date('...') and GROUP BY date(d) over --rows rows of 4096 values next to WHERE c = 'x' and GROUP BY c.
Times: median of --reps runs, each bracketed by device synchronisation, after warm-up runs."""
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
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.core import AggregateFunction, AggregateOperator, ProjectOperator
    from vinum_amd.core.base import DeviceRecordBatch, Operator
    from vinum_amd.core.lowering import lower_dictionary, used_columns
    from vinum_amd.device import DeviceBuffer, DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    lib = L.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def med(ts):
        return float(np.median(ts))

    def spread(ts):
        return (max(ts) - min(ts)) / med(ts)

    n = int(args.rows)
    say(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}  rows={n:.0e}")

    def texts(count):
        secs = 1_000_000_000 + np.arange(count, dtype=np.int64) * 61
        return [str(s).replace("T", " ") for s in np.array(secs, dtype="datetime64[s]").astype("str")]

    def code_column(kd, values):
        c = kd.encode(pa.array(values, pa.string())).to_numpy(zero_copy_only=False).astype(np.int32)
        pool = torch.from_numpy(c).cuda()
        col = DeviceColumn.from_torch(pool[torch.randint(0, len(pool), (n,), device="cuda")].contiguous())
        col.dictionary = kd
        return col

    say("\n(a) the row pass: vnm_strdict_gather_temporal (12.1 B / row) against vnm_strdict_gather_codes (8 B / row), the same codes")
    big = None
    for distinct in (4096, 10_000_000):
        values = texts(distinct)
        kd = KeyDictionary(pa.string())
        col = code_column(kd, values)
        t_first = None
        if distinct == 10_000_000:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kd.parsed("s")
            torch.cuda.synchronize()
            t_first = time.perf_counter() - t0
            big = (kd, values, t_first)
        value_of, status_of = kd.parsed("s")
        ids = value_of.length
        table32 = DeviceBuffer(max(ids, 1) * 4)
        L.check(lib.vnm_memset(table32.ptr, 0, table32.nbytes))
        out64, out32, bitmap = DeviceBuffer(n * 8), DeviceBuffer(n * 4), DeviceBuffer((n + 7) >> 3)

        def temporal():
            L.check(lib.vnm_strdict_gather_temporal(col.values_ptr, None, 0, value_of.values_ptr, status_of.values_ptr, ids, n, 8, out64.ptr, bitmap.ptr,
                                                    None, None, None))

        def codes():
            L.check(lib.vnm_strdict_gather_codes(col.values_ptr, None, 0, table32.ptr, ids, n, -1, out32.ptr, None))
        tt, tc = timed_all(temporal, args.reps), timed_all(codes, args.reps)
        say(f"  {distinct:>9d} distinct values: gather_temporal {med(tt) * 1e3:7.3f} ms ({n * 12.125 / med(tt) / 1e12:5.2f} TB/s, spread {spread(tt) * 100:4.1f} %)   "
            f"gather_codes {med(tc) * 1e3:7.3f} ms ({n * 8 / med(tc) / 1e12:5.2f} TB/s, spread {spread(tc) * 100:4.1f} %)   ratio {med(tt) / med(tc):5.2f} (bytes: 1.52)")
        del out64, out32, bitmap, table32
        if distinct != 10_000_000:
            del kd, col

    say("\n(b) parsing 1e7 distinct 19-byte values into the per-id tables (unit s)")
    kd, values, t_first = big
    ids = kd._id_count()
    tv, ts = DeviceBuffer(ids * 8), DeviceBuffer(ids)
    refused = ctypes.c_int64(0)

    def parse():
        L.check(lib.vnm_strdict_parse_datetime(kd.handle(), 1, 0, tv.ptr, ts.ptr, ctypes.byref(refused), None))
    tp = timed_all(parse, args.reps)
    assert refused.value == -1
    t0 = time.perf_counter()
    host = np.array(values, dtype="datetime64[s]")
    t_host = time.perf_counter() - t0
    got = tv.to_host(np.int64, ids)
    assert (np.sort(got[ts.to_host(np.uint8, ids) == 0]) == np.sort(host.astype(np.int64))).all()
    say(f"  KeyDictionary.parsed('s') the first time (tables allocated, {ids} ids): {t_first * 1e3:8.2f} ms;  vnm_strdict_parse_datetime again: "
        f"{med(tp) * 1e3:7.3f} ms (spread {spread(tp) * 100:4.1f} %, {len(values) / med(tp) / 1e9:5.2f} G values/s)")
    say(f"  np.array(values, dtype='datetime64[s]'), one host thread: {t_host * 1e3:9.1f} ms = {t_host / med(tp):7.0f} x the repeat call")
    del tv, ts, kd, values, big, col

    say(f"\n(c) whole predicates and group-bys over {n:.0e} rows: d 4096 date-time strings, c a plain string column of 4096 values")
    kd = KeyDictionary(pa.string())
    d = code_column(kd, texts(4096))
    kc = KeyDictionary(pa.string())
    c = code_column(kc, [f"c{i:07d}" for i in range(4095)] + ["x"])
    batch = DeviceRecordBatch({"d": d, "c": c}, n)

    def mask(pred):
        low, extra = lower_dictionary(pred, batch.columns)
        return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)
    p0, p1 = ("eq", "c", ("lit", "x")), ("ge", ("date", "d"), ("date", ("lit", "2001-09-11")))
    w0, w1 = timed_all(lambda: mask(p0), args.reps), timed_all(lambda: mask(p1), args.reps)
    k0, k1 = (int(mask(p).to_host(np.uint8, n).sum(dtype=np.int64)) for p in (p0, p1))
    assert k0 > 0 and 0 < k1 < n
    say(f"  WHERE c = 'x'                        {med(w0) * 1e3:8.2f} ms   ({k0} rows)")
    say(f"  WHERE date(d) >= date('2001-09-11')  {med(w1) * 1e3:8.2f} ms   {med(w1) / med(w0):5.2f} x   ({k1} rows)")

    class Once(Operator):
        def next(self):
            yield batch

    def group(by_date):
        op, key = Once(), "c"
        if by_date:
            op, key = ProjectOperator([("date", "d")], op, col_names=["u"], keep_input_table=True), "u"
        return next(AggregateOperator(op, [key], [AggregateFunction("count_star", None, "n")], [key]).next()).num_rows
    g0, g1 = timed_all(lambda: group(False), max(3, args.reps // 2)), timed_all(lambda: group(True), max(3, args.reps // 2))
    say(f"  GROUP BY c                           {med(g0) * 1e3:8.2f} ms   ({group(False)} groups)")
    say(f"  GROUP BY date(d)                     {med(g1) * 1e3:8.2f} ms   {med(g1) / med(g0):5.2f} x   ({group(True)} groups)")
    say(f"  the dictionary of d: {kd.parse_launches} parse launch(es) over {kd.parse_ids_parsed} ids")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
