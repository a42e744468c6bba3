#!/usr/bin/env python3
"""upper() / lower() through the device dictionary, measured (profiles/r11_strcase.txt):
  (a) vnm_strdict_map_codepoints alone over dictionaries of 1e5 and 5e6 distinct 11-byte values, all ASCII and with one non-ASCII
      code point per value: the FIRST call into an empty derived dictionary (every image is hashed and inserted, the table grows
      from its initial size) and a call AGAIN over the same ids (every image is found).  Yardsticks: vnm_strdict_translate of the
      source into the derived dictionary (a probe per value, no decode, no insert) and pc.utf8_upper over the same values on ONE
      host thread;
  (b) WHERE upper(c) = 'X' and GROUP BY upper(c) over --rows rows of resident codes against WHERE c = 'x' and GROUP BY c over the
      same column: the row pass adds one int32 gather per function (the table of the batch's dictionary is built once, before the
      timed runs: launches only on dictionary growth).
Times: median of --reps runs, each bracketed by device synchronisation (warm-up runs first)."""
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


def values(n, non_ascii):
    """n distinct 11-byte values: lower-case letters with the value's number in the last 8 bytes; non_ascii: bytes 0-1 are 'ß'"""
    rng = np.random.default_rng(1)
    raw = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)[rng.integers(0, 26, (n, 11))]
    num = np.arange(n)
    for k in range(8):
        raw[:, 10 - k] = 97 + (num // 16 ** k) % 16
    if non_ascii:
        raw[:, 0], raw[:, 1] = 0xC3, 0x9F
    offs = np.arange(n + 1, dtype=np.int32) * 11
    return pa.Array.from_buffers(pa.string(), n, [None, pa.py_buffer(offs), pa.py_buffer(raw.tobytes())])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=float, default=1e8)
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

    map_from, map_to = strcase.case_table("upper")
    strcase.case_table("lower")
    say(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}")
    say(f"code point tables from pyarrow {pa.__version__}: upper {len(map_from)} pairs in {strcase.build_seconds['upper']:.2f} s, "
        f"lower {len(strcase.case_table('lower')[0])} pairs in {strcase.build_seconds['lower']:.2f} s (host, once per process)")

    say("\n(a) vnm_strdict_map_codepoints (upper) over a dictionary of n distinct 11-byte values")
    pa.set_cpu_count(1)
    for n in (100_000, 5_000_000):
        for non_ascii in (False, True):
            src = KeyDictionary(pa.string())
            vals = values(n, non_ascii)
            for s in range(0, n, 1 << 20):
                src.encode(vals.slice(s, 1 << 20))
            top = int(lib.vnm_strdict_ids(src.handle()))
            out = DeviceBuffer(top * 4)
            keep = []

            def first():
                h = lib.vnm_strdict_create()
                keep.append(h)
                L.check(lib.vnm_strdict_map_codepoints(src.handle(), h, map_from.ctypes.data, map_to.ctypes.data, len(map_from), 0, out.ptr, None, None))
            t_first = timed(first, max(3, args.reps // 2), warm=1)
            dst = keep[-1]
            t_again = timed(lambda: L.check(lib.vnm_strdict_map_codepoints(src.handle(), dst, map_from.ctypes.data, map_to.ctypes.data, len(map_from), 0, out.ptr, None, None)), args.reps)
            mapped = int((out.to_host(np.int32, top) >= 0).sum())
            assert mapped == n, f"{mapped} of {n} values mapped"
            t_tr = timed(lambda: L.check(lib.vnm_strdict_translate(src.handle(), dst, 0, out.ptr, None)), args.reps)
            t0 = time.perf_counter()
            host = pc.utf8_upper(vals)
            t_host = time.perf_counter() - t0
            assert len(host) == n
            for h in keep:
                lib.vnm_strdict_destroy(h)
            kind = "one 'ß' per value" if non_ascii else "ASCII"
            say(f"  {n:>9d} values, {kind:<18s} first call {t_first * 1e3:8.3f} ms ({n / t_first / 1e6:7.1f} M values/s)   again {t_again * 1e3:8.3f} ms   "
                f"translate {t_tr * 1e3:7.3f} ms   pc.utf8_upper, one host thread {t_host * 1e3:8.3f} ms   first / host = {t_first / t_host:5.2f}")
            del src, out

    n = int(args.rows)
    say(f"\n(b) {n:.0e} rows of resident int32 codes over a dictionary of 4096 mixed-case values")
    kd = KeyDictionary(pa.string())
    words = pa.array([("City%04d" % i if i % 2 else "city%04d" % i) for i in range(4096)] + ["x", "X"], pa.string())
    codes = np.unique(kd.encode(words).to_numpy(zero_copy_only=False).astype(np.int32))
    rows = torch.from_numpy(codes).cuda()[torch.randint(0, len(codes), (n,), device="cuda")].contiguous()
    col = DeviceColumn.from_torch(rows)
    col.dictionary = kd
    batch = DeviceRecordBatch({"c": col}, n)

    def mask(pred):
        low, extra = lower_dictionary(pred, batch.columns)
        return ops.predicate_mask(low, used_columns([low], batch.columns, extra), n)

    base = timed(lambda: mask(("eq", "c", ("lit", "x"))), args.reps)
    up = timed(lambda: mask(("eq", ("upper", "c"), ("lit", "X"))), args.reps)
    k0 = int(mask(("eq", "c", ("lit", "x"))).to_host(np.uint8, n).sum(dtype=np.int64))
    k1 = int(mask(("eq", ("upper", "c"), ("lit", "X"))).to_host(np.uint8, n).sum(dtype=np.int64))
    say(f"  WHERE c = 'x'            {base * 1e3:8.2f} ms   ({k0} rows)")
    say(f"  WHERE upper(c) = 'X'     {up * 1e3:8.2f} ms   {up / base:5.2f} x   ({k1} rows: 'x' and 'X')")
    assert k1 > k0 > 0

    class Once(Operator):
        def next(self):
            yield batch

    def group(by_upper):
        op = Once()
        key = "c"
        if by_upper:
            op, key = ProjectOperator([("upper", "c")], op, col_names=["u"], keep_input_table=True), "u"
        res = next(AggregateOperator(op, [key], [AggregateFunction("count_star", None, "n")], [key]).next())
        return res.num_rows
    def route():
        buf = ctypes.create_string_buffer(1024)
        lib.vnm_route_last(buf, len(buf))
        return buf.value.decode(errors="replace")

    g0 = timed(lambda: group(False), max(3, args.reps // 2))
    r0 = route()
    g1 = timed(lambda: group(True), max(3, args.reps // 2))
    r1 = route()
    gather = DeviceBuffer(n * 4)
    _, table = kd.mapped("upper")
    t_g = timed(lambda: L.check(lib.vnm_strdict_codes_to_ranks(col.values_ptr, table.values_ptr, n, gather.ptr, None)), args.reps)
    say(f"  GROUP BY c               {g0 * 1e3:8.2f} ms   ({group(False)} groups; key codes below {kd._id_count()})   route: {r0}")
    say(f"  GROUP BY upper(c)        {g1 * 1e3:8.2f} ms   {g1 / g0:5.2f} x   ({group(True)} groups; key codes below {kd.mapped('upper')[0]._id_count()})   route: {r1}")
    say(f"  the gather alone (table[code] per row)        {t_g * 1e3:8.2f} ms")
    proj = ProjectOperator([("upper", "c")], None, col_names=["u"], keep_input_table=True)
    t_p = timed(lambda: proj._kernel(batch), args.reps)
    projected = proj._kernel(batch)

    class OnceProjected(Operator):
        def next(self):
            yield projected
    t_a = timed(lambda: next(AggregateOperator(OnceProjected(), ["u"], [AggregateFunction("count_star", None, "n")], ["u"]).next()), max(3, args.reps // 2))
    say(f"  its two steps: the projection (lowering + gather) {t_p * 1e3:8.2f} ms, the aggregate over the projected column {t_a * 1e3:8.2f} ms")
    say(f"  map launches over all timed runs: {kd.map_launches} (ids mapped: {kd.map_ids_mapped} of {kd._id_count()})")
    assert kd.map_launches == 1
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
