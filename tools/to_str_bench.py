#!/usr/bin/env python3
"""to_str() through the device value table, measured (profiles/r14_to_str.txt):
  (1) vnm_strval_to_str alone over --rows resident int64 rows at 100, 4096, 1e5 and 1e7 distinct values: the FIRST call (every value is
      new: claimed, formatted, inserted; the table grows from its initial size) and a call AGAIN (every value is known), each split
      into its find, format and gather passes by the library's own event spans.  Yardsticks in the same run: vnm_strpair_concat over
      two code columns at the same number of distinct pairs -- the same passes over the same number of row bytes (2 x 4 against 8) --
      and np.array(column, dtype='U') on one host thread over --host-rows of the same rows;
  (2) the same call over date32 at 4096 distinct days and timestamp[us] at 1e7 distinct instants;
  (3) WHERE to_str(v) = '7', GROUP BY to_str(v) and concat(a, '-', to_str(v)) over --rows rows (v: 4096 values, a: 64 values) next to
      WHERE c = 'x' and GROUP BY c over a plain string column of 4096 values.
Times: median of --reps runs, each bracketed by device synchronisation (warm-up runs first, except where the first call is the
subject)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import pyarrow as pa
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.strcase_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--host-rows", type=float, default=2e6)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.core import AggregateFunction, AggregateOperator, ProjectOperator
    from vinum_amd.core.base import DeviceRecordBatch, Operator
    from vinum_amd.core.lowering import lower_dictionary, project_lowered, used_columns
    from vinum_amd.device import DeviceColumn
    from vinum_amd.keydict import ValueTable
    from vinum_amd.vinum_lib import KeyDictionary
    lib = L.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spans(names):
        out = {}
        for name in names:
            ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
            lib.vnm_profile_query(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
            out[name] = ms.value
        return out

    n = int(args.rows)
    say(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}  rows={n:.0e}")
    parts = ("strpair_find", "strpair_rehash", "strval_to_str", "strpair_concat", "strdict_encode", "strdict_compact", "strpair_gather")

    def first_and_again(call, stats, label, image):
        """one table's first call and its repeat, each with the library's spans"""
        lib.vnm_set_profiling(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        first = spans(parts)
        lib.vnm_set_profiling(0)
        st = stats()
        t_again = timed(call, args.reps)
        lib.vnm_set_profiling(1)
        call()
        torch.cuda.synchronize()
        again = spans(parts)
        lib.vnm_set_profiling(0)
        assert stats()["half_written"] == 0
        say(f"  {label} ({st['slots']} slots after {st['rehashes']} rehashes)")
        say(f"      first call {t_first * 1e3:9.2f} ms: find {first['strpair_find']:8.2f}  rehash {first['strpair_rehash']:7.2f}  images (lengths + bytes) "
            f"{first[image]:7.2f}  insert into dst {first['strdict_encode'] + first['strdict_compact']:8.2f}  gather {first['strpair_gather']:7.2f}")
        say(f"      again      {t_again * 1e3:9.2f} ms: find {again['strpair_find']:8.2f}  gather {again['strpair_gather']:7.2f}   ({n / t_again / 1e9:6.2f} G rows/s)")
        del out
        return t_first, t_again

    def value_column(values, arrow_type):
        """n rows drawn from `values` (a NumPy array of the storage type), resident"""
        pool = torch.from_numpy(values).cuda()
        return DeviceColumn.from_torch(pool[torch.randint(0, len(pool), (n,), device="cuda")].contiguous(), arrow_type=arrow_type)

    def host_text(col, view=None):
        m = int(min(args.host_rows, n))
        host = col.slice(0, m).to_numpy()
        host = host if view is None else host.astype(np.int64).view(view)
        t0 = time.perf_counter()
        text = np.array(host, dtype="U")
        t = time.perf_counter() - t0
        assert len(text) == m
        return t / m * n

    say("\n(1) vnm_strval_to_str over int64 alone; per call in ms: total = find + format + gather (+ host).  Yardstick: vnm_strpair_concat(a, '-', b)")
    rng = np.random.default_rng(14)
    for distinct, side in ((100, 10), (4096, 64), (100_000, 316), (10_000_000, 3163)):
        values = np.unique(rng.integers(-2**62, 2**62, int(distinct * 1.01)))[:distinct].astype(np.int64)
        rng.shuffle(values)
        col = value_column(values, pa.int64())
        table = ValueTable.of(col)
        t_first, t_again = first_and_again(lambda: table.column(col), table.stats, f"to_str(int64): {distinct:>9d} distinct values", "strval_to_str")
        assert table.stats()["values_formatted"] <= distinct
        t_host = host_text(col)
        del table, col
        da, db = KeyDictionary(pa.string()), KeyDictionary(pa.string())
        codes = []
        for kd, tag in ((da, "a"), (db, "b")):
            c = kd.encode(pa.array([f"{tag}{i:07d}" for i in range(side)], pa.string())).to_numpy(zero_copy_only=False).astype(np.int32)
            pool = torch.from_numpy(c).cuda()
            cc = DeviceColumn.from_torch(pool[torch.randint(0, len(pool), (n,), device="cuda")].contiguous())
            cc.dictionary = kd
            codes.append(cc)
        pairs = da.paired(db, b"", b"-", b"")
        p_first, p_again = first_and_again(lambda: pairs.column(da, db, codes[0], codes[1]), pairs.stats, f"yardstick concat: {side * side:>9d} distinct pairs", "strpair_concat")
        say(f"      to_str / concat: first {t_first / p_first:5.2f} x  again {t_again / p_again:5.2f} x      np.array(column, dtype='U'), one host thread: "
            f"{t_host * 1e3:10.1f} ms per {n:.0e} rows = {t_host / t_again:7.0f} x the repeat call")
        del pairs, codes, da, db

    say("\n(2) the temporal kinds")
    days = np.arange(-2048, 2048, dtype=np.int32) * 7
    col = value_column(days, pa.date32())
    table = ValueTable.of(col)
    first_and_again(lambda: table.column(col), table.stats, "to_str(date32): 4096 distinct days", "strval_to_str")
    say(f"      np.array(column, dtype='U'), one host thread: {host_text(col, 'datetime64[D]') * 1e3:10.1f} ms per {n:.0e} rows")
    del table, col
    instants = np.unique(rng.integers(-2**60, 2**60, 10_100_000))[:10_000_000].astype(np.int64)
    col = value_column(instants, pa.timestamp("us"))
    table = ValueTable.of(col)
    first_and_again(lambda: table.column(col), table.stats, "to_str(timestamp[us]): 1e7 distinct instants", "strval_to_str")
    say(f"      np.array(column, dtype='U'), one host thread: {host_text(col, 'datetime64[us]') * 1e3:10.1f} ms per {n:.0e} rows")
    del table, col, instants

    say(f"\n(3) whole queries over {n:.0e} rows: v int64 of 4096 values, a 64 string values, c a plain string column of 4096 values")

    def string_column(count, tag, also):
        kd = KeyDictionary(pa.string())
        c = kd.encode(pa.array([f"{tag}{i:07d}" for i in range(count - 1)] + [also], pa.string())).to_numpy(zero_copy_only=False).astype(np.int32)
        pool = torch.from_numpy(c).cuda()
        out = DeviceColumn.from_torch(pool[torch.randint(0, len(pool), (n,), device="cuda")].contiguous())
        out.dictionary = kd
        return out
    v = value_column(np.arange(4096, dtype=np.int64), pa.int64())
    v.value_tables = {}                                     # (what a scan's registry gives the column: one table for every call below)
    batch = DeviceRecordBatch({"v": v, "a": string_column(64, "a", "x"), "c": string_column(4096, "c", "x")}, n)

    def mask(pred):
        low, extra = lower_dictionary(pred, batch.columns)
        return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)
    w0 = timed(lambda: mask(("eq", "c", ("lit", "x"))), args.reps)
    w1 = timed(lambda: mask(("eq", ("to_str", "v"), ("lit", "7"))), args.reps)
    k0 = int(mask(("eq", "c", ("lit", "x"))).to_host(np.uint8, n).sum(dtype=np.int64))
    k1 = int(mask(("eq", ("to_str", "v"), ("lit", "7"))).to_host(np.uint8, n).sum(dtype=np.int64))
    assert k0 > 0 and k1 > 0
    say(f"  WHERE c = 'x'                        {w0 * 1e3:8.2f} ms   ({k0} rows)")
    say(f"  WHERE to_str(v) = '7'                {w1 * 1e3:8.2f} ms   {w1 / w0:5.2f} x   ({k1} rows)")

    class Once(Operator):
        def next(self):
            yield batch

    def group(by_text):
        op, key = Once(), "c"
        if by_text:
            op, key = ProjectOperator([("to_str", "v")], op, col_names=["u"], keep_input_table=True), "u"
        return next(AggregateOperator(op, [key], [AggregateFunction("count_star", None, "n")], [key]).next()).num_rows
    g0 = timed(lambda: group(False), max(3, args.reps // 2))
    g1 = timed(lambda: group(True), max(3, args.reps // 2))
    say(f"  GROUP BY c                           {g0 * 1e3:8.2f} ms   ({group(False)} groups)")
    say(f"  GROUP BY to_str(v)                   {g1 * 1e3:8.2f} ms   {g1 / g0:5.2f} x   ({group(True)} groups)")
    c1 = timed(lambda: project_lowered([("concat", "a", ("lit", "-"), ("to_str", "v"))], batch.columns, n), args.reps)
    c0 = timed(lambda: project_lowered([("concat", "a", ("lit", "-"), "c")], batch.columns, n), args.reps)
    say(f"  concat(a, '-', c)                    {c0 * 1e3:8.2f} ms   (64 x 4096 pairs)")
    say(f"  concat(a, '-', to_str(v))            {c1 * 1e3:8.2f} ms   {c1 / c0:5.2f} x")
    (table,) = v.value_tables.values()
    st = table.stats()
    say(f"  the value table of v: {st['launches']} launches, {st['values_formatted']} values formatted, {st['rehashes']} rehashes")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
