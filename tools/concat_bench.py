#!/usr/bin/env python3
"""concat() through the device dictionary, measured (profiles/r13_concat.txt):
  (1) vnm_strpair_concat alone over --rows rows of resident codes at 4096, 1e5 and 1e7 distinct pairs: the FIRST call (every pair is
      new: claimed, concatenated, inserted; the table grows from its initial size) and a call AGAIN (every pair is known), each split
      into its find, concat and gather passes by the library's own event spans.  Yardstick in the same run: the `a = b` comparison of
      two dictionary-coded columns, a pass that reads the same two code columns;
  (2) vnm_strdict_concat_affix over dictionaries of 1e5 and 5e6 distinct 11-byte values, first call and again, next to
      vnm_strdict_map_codepoints (upper) over the same values;
  (3) GROUP BY concat(a, '-', b) and WHERE concat(a, b) = 'xy' over --rows rows next to GROUP BY c and WHERE c = 'x' over a plain
      string column;
  (4) the host alternative: pc.binary_join_element_wise on ONE host thread over --host-rows of the same rows.
Times: median of --reps runs, each bracketed by device synchronisation (warm-up runs first, except where the first call is the
subject)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.strcase_bench import timed, values  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--host-rows", type=float, default=2e7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops, strcase
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

    def spans(names):
        out = {}
        for name in names:
            ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
            lib.vnm_profile_query(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
            out[name] = ms.value
        return out

    n = int(args.rows)
    say(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}  rows={n:.0e}")

    def dictionary(count, tag, also=()):
        kd = KeyDictionary(pa.string())
        codes = kd.encode(pa.array([f"{tag}{i:07d}" for i in range(count - len(also))] + list(also), pa.string())).to_numpy(zero_copy_only=False).astype(np.int32)
        return kd, torch.from_numpy(codes).cuda()

    def column(kd, codes):
        col = DeviceColumn.from_torch(codes[torch.randint(0, len(codes), (n,), device="cuda")].contiguous())
        col.dictionary = kd
        return col

    say("\n(1) vnm_strpair_concat(a, '-', b) alone; 8-byte values on both sides; per call in ms: total = find + concat + gather (+ host)")
    parts = ("strpair_find", "strpair_rehash", "strpair_concat", "strdict_encode", "strdict_compact", "strpair_gather")
    for side in (64, 316, 3163):
        da, codes_a = dictionary(side, "a")
        db, codes_b = dictionary(side, "b")
        ca, cb = column(da, codes_a), column(db, codes_b)
        batch = DeviceRecordBatch({"a": ca, "b": cb}, n)

        def mask():
            low, extra = lower_dictionary(("eq", "a", "b"), batch.columns)
            return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)
        t_eq = timed(mask, args.reps)
        table = da.paired(db, b"", b"-", b"")
        lib.vnm_set_profiling(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = table.column(da, db, ca, cb)
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        first = spans(parts)
        lib.vnm_set_profiling(0)
        st = table.stats()
        t_again = timed(lambda: table.column(da, db, ca, cb), args.reps)
        lib.vnm_set_profiling(1)
        table.column(da, db, ca, cb)
        torch.cuda.synchronize()
        again = spans(parts)
        lib.vnm_set_profiling(0)
        st2 = table.stats()
        assert st2["pairs_concatenated"] == st["pairs_concatenated"] and st2["half_written"] == 0
        say(f"  {st['pairs_concatenated']:>9d} distinct pairs ({side} x {side} values; {st['slots']} slots after {st['rehashes']} rehashes)")
        say(f"      first call {t_first * 1e3:9.2f} ms: find {first['strpair_find']:8.2f}  rehash {first['strpair_rehash']:7.2f}  concat (lengths + bytes) "
            f"{first['strpair_concat']:7.2f}  insert into dst {first['strdict_encode'] + first['strdict_compact']:8.2f}  gather {first['strpair_gather']:7.2f}")
        say(f"      again      {t_again * 1e3:9.2f} ms: find {again['strpair_find']:8.2f}  concat {again['strpair_concat']:7.2f}  gather {again['strpair_gather']:7.2f}"
            f"   ({n / t_again / 1e9:6.2f} G rows/s)      yardstick  a = b  {t_eq * 1e3:8.2f} ms")
        del out, table, batch, ca, cb, da, db

    say("\n(2) vnm_strdict_concat_affix('<', value, '>') over a dictionary of n distinct 11-byte values, next to vnm_strdict_map_codepoints (upper)")
    map_from, map_to = strcase.case_table("upper")
    pa.set_cpu_count(1)
    for count in (100_000, 5_000_000):
        src = KeyDictionary(pa.string())
        vals = values(count, False)
        for s in range(0, count, 1 << 20):
            src.encode(vals.slice(s, 1 << 20))
        top = int(lib.vnm_strdict_ids(src.handle()))
        out = DeviceBuffer(top * 4)
        null_code = ctypes.c_int32(0)
        keep = []

        def first_affix():
            h = lib.vnm_strdict_create()
            keep.append(h)
            L.check(lib.vnm_strdict_concat_affix(src.handle(), h, b"<", 1, b">", 1, 0, out.ptr, ctypes.byref(null_code), None))

        def first_map():
            h = lib.vnm_strdict_create()
            keep.append(h)
            L.check(lib.vnm_strdict_map_codepoints(src.handle(), h, map_from.ctypes.data, map_to.ctypes.data, len(map_from), 0, out.ptr, None, None))
        t_first = timed(first_affix, 3, warm=1)
        dst = keep[-1]
        t_again = timed(lambda: L.check(lib.vnm_strdict_concat_affix(src.handle(), dst, b"<", 1, b">", 1, 0, out.ptr, ctypes.byref(null_code), None)), args.reps)
        assert int((out.to_host(np.int32, top) >= 0).sum()) == count
        t_map_first = timed(first_map, 3, warm=1)
        mdst = keep[-1]
        t_map_again = timed(lambda: L.check(lib.vnm_strdict_map_codepoints(src.handle(), mdst, map_from.ctypes.data, map_to.ctypes.data, len(map_from), 0, out.ptr, None, None)), args.reps)
        t0 = time.perf_counter()
        host = pc.binary_join_element_wise(pa.scalar("<"), vals, pa.scalar(">"), "")
        t_host = time.perf_counter() - t0
        assert len(host) == count
        for h in keep:
            lib.vnm_strdict_destroy(h)
        say(f"  {count:>9d} values: affix first {t_first * 1e3:8.3f} ms ({count / t_first / 1e6:6.1f} M values/s)  again {t_again * 1e3:8.3f} ms   |   map_codepoints first "
            f"{t_map_first * 1e3:8.3f} ms  again {t_map_again * 1e3:8.3f} ms   |   pc.binary_join_element_wise, one host thread {t_host * 1e3:8.3f} ms   first / host = {t_first / t_host:5.2f}")
        del src, out

    say(f"\n(3) whole queries over {n:.0e} rows: a, b 64 values each (4096 pairs), c a plain column of 4096 values")
    da, codes_a = dictionary(64, "a", ["x"])
    db, codes_b = dictionary(64, "b", ["y"])
    dc, codes_c = dictionary(4096, "c", ["x"])
    batch = DeviceRecordBatch({"a": column(da, codes_a), "b": column(db, codes_b), "c": column(dc, codes_c)}, n)

    def mask(pred):
        low, extra = lower_dictionary(pred, batch.columns)
        return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)
    w0 = timed(lambda: mask(("eq", "c", ("lit", "x"))), args.reps)
    w1 = timed(lambda: mask(("eq", ("concat", "a", "b"), ("lit", "xy"))), args.reps)
    k0 = int(mask(("eq", "c", ("lit", "x"))).to_host(np.uint8, n).sum(dtype=np.int64))
    k1 = int(mask(("eq", ("concat", "a", "b"), ("lit", "xy"))).to_host(np.uint8, n).sum(dtype=np.int64))
    assert k0 > 0 and k1 > 0
    say(f"  WHERE c = 'x'                 {w0 * 1e3:8.2f} ms   ({k0} rows)")
    say(f"  WHERE concat(a, b) = 'xy'     {w1 * 1e3:8.2f} ms   {w1 / w0:5.2f} x   ({k1} rows)")

    class Once(Operator):
        def next(self):
            yield batch

    def group(by_concat):
        op, key = Once(), "c"
        if by_concat:
            op, key = ProjectOperator([("concat", "a", ("lit", "-"), "b")], op, col_names=["u"], keep_input_table=True), "u"
        return next(AggregateOperator(op, [key], [AggregateFunction("count_star", None, "n")], [key]).next()).num_rows
    g0 = timed(lambda: group(False), max(3, args.reps // 2))
    g1 = timed(lambda: group(True), max(3, args.reps // 2))
    say(f"  GROUP BY c                    {g0 * 1e3:8.2f} ms   ({group(False)} groups)")
    say(f"  GROUP BY concat(a, '-', b)    {g1 * 1e3:8.2f} ms   {g1 / g0:5.2f} x   ({group(True)} groups)")
    tables = da.pair_tables
    say(f"  pair tables: {[(t.stats()['pair_launches'], t.stats()['pairs_concatenated'], t.stats()['rehashes']) for t in tables]} (launches, pairs concatenated, rehashes)")

    m = int(min(args.host_rows, n))
    say(f"\n(4) the host alternative over {m:.0e} of these rows (one thread): the strings materialised per row")
    ia = batch.columns["a"].to_numpy()[:m]
    ib = batch.columns["b"].to_numpy()[:m]
    ha = da.values_by_code().take(pa.array(ia))
    hb = db.values_by_code().take(pa.array(ib))
    t0 = time.perf_counter()
    joined = pc.binary_join_element_wise(ha, hb, "-")
    t_host = time.perf_counter() - t0
    assert len(joined) == m
    say(f"  pc.binary_join_element_wise(a, b, '-')   {t_host * 1e3:9.2f} ms for {m:.0e} rows = {t_host / m * n * 1e3:9.2f} ms per {n:.0e} rows ({m / t_host / 1e6:6.1f} M rows/s)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
