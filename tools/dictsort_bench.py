"""ORDER BY over a dictionary-typed string column (dictionary<int32, utf8>) from HOST record batches to a HOST record batch, PCIe
included, through vinum_lib.Sort (vnm_sort_op_*): `ORDER BY c` carrying an int64, 100 / 1e5 / 5e6 distinct 11-byte values, two ways --
  (a) the dictionary-typed column (the batch dictionary's values through vnm_strdict_encode, the indices through
      vnm_strdict_remap_indices, the result through vnm_dict_take_compact);
  (b) the same data as plain utf8 through the existing string-key route (every row's bytes staged and hashed on the device, the
      result's bytes gathered) --
each with and without LIMIT 100; `GROUP BY c` with COUNT(*) through vinum_lib.GenericHashAggregate (vnm_agg_op_*) the same two ways;
then vnm_dict_take_compact alone over device buffers (wall time of the whole call, its two
synchronisations included), identity rows and a random permutation, both table forms where the ids fit LDS.
usage: dictsort_bench.py [rows]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import pyarrow as pa

from vinum_amd import _lib as L
from vinum_amd import vinum_lib as V
from vinum_amd.device import DeviceBuffer

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
rng = np.random.default_rng(0)
lib = L.lib()


def timed_sort(table, limit, reps=3):
    best = None
    for _ in range(reps):                  # (the first run also grows the pool; the best is reported)
        t0 = time.perf_counter()
        op = V.Sort(["c"], [V.SortOrder(0)])
        for b in table.to_batches():
            op.next(b)
        out = op.sorted(limit) if limit else op.sorted()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def timed_group_by(table, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        op = V.GenericHashAggregate(["c"], ["c"], [V.AggFuncDef(V.COUNT_STAR, "", "n")])
        for b in table.to_batches():
            op.next(b)
        out = op.result()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


print(f"rows {n}", flush=True)
for G in (100, 100_000, 5_000_000):
    values = pa.array([f"cty_{i:07d}" for i in range(G)])
    idx = pa.array(rng.integers(0, G, n).astype(np.int32))
    payload = pa.array(np.arange(n, dtype=np.int64))
    as_dict = pa.table({"c": pa.DictionaryArray.from_arrays(idx, values), "p": payload})
    as_utf8 = pa.table({"c": values.take(idx), "p": payload})
    for limit in (0, 100):
        ta, out_a = timed_sort(as_dict, limit)
        tb, out_b = timed_sort(as_utf8, limit)
        same = out_a.column("p").equals(out_b.column("p")) and out_a.column("c").cast(pa.string()).equals(out_b.column("c"))
        print(f"G={G:>8d} ORDER BY c{' LIMIT 100' if limit else '':10s} (a) dictionary {ta * 1e3:8.1f} ms {n / ta / 1e6:7.1f} Mrows/s   "
              f"(b) utf8 {tb * 1e3:8.1f} ms {n / tb / 1e6:7.1f} Mrows/s   same rows: {same}   "
              f"[(a) {idx.nbytes / 1e6:.0f} MB of indices + {values.nbytes / 1e6:.1f} MB of values, (b) {as_utf8['c'].nbytes / 1e6:.0f} MB of offsets + bytes; "
              f"result dictionary {len(out_a.column('c').dictionary)} values]", flush=True)
    ta, out_a = timed_group_by(as_dict)
    tb, out_b = timed_group_by(as_utf8)
    counts = lambda out: dict(zip(out.column("c").cast(pa.string()).to_pylist(), out.column("n").to_pylist())) if G <= 100_000 else out.num_rows  # noqa: E731
    print(f"G={G:>8d} GROUP BY c          (a) dictionary {ta * 1e3:8.1f} ms {n / ta / 1e6:7.1f} Mrows/s   "
          f"(b) utf8 {tb * 1e3:8.1f} ms {n / tb / 1e6:7.1f} Mrows/s   same groups: {counts(out_a) == counts(out_b)}   [{out_a.num_rows} groups]", flush=True)
    del as_dict, as_utf8

print("vnm_dict_take_compact alone (device buffers; wall time per call, best of 2 rounds of 20 calls):", flush=True)
nk = max(n, 100_000_000)            # (codes + indices well beyond the 256 MiB last-level cache)
perm = DeviceBuffer.from_host(rng.permutation(nk).astype(np.int64))
for G, index_type in ((100, np.int8), (100, np.int32), (8192, np.int32), (100_000, np.int32), (5_000_000, np.int32)):
    codes = DeviceBuffer.from_host(rng.integers(0, G, nk).astype(np.int32))
    w = np.dtype(index_type).itemsize
    out, bits, used = DeviceBuffer(nk * w), DeviceBuffer((nk + 7) >> 3), DeviceBuffer(G * 4)
    vt = L.I8 if index_type is np.int8 else L.I32
    nulls, n_used = ctypes.c_int64(0), ctypes.c_int64(0)
    for rows, rows_name in ((None, "identity"), (perm.ptr, "permutation")):
        moved = 2 * nk * 4 + (2 * nk * 8 if rows else 0) + nk * w + ((nk + 7) >> 3)     # codes twice (mark, gather), rows twice, indices, bitmap
        for form in (("global", "lds") if G <= 8192 else ("global",)):
            os.environ["VNM_DICT_COMPACT_LDS"] = "1" if form == "lds" else "0"
            best = None
            for rnd in range(2):
                L.check(lib.vnm_dict_take_compact(codes.ptr, rows, nk, G, vt, out.ptr, bits.ptr, ctypes.byref(nulls), used.ptr, ctypes.byref(n_used), None))
                t0 = time.perf_counter()
                for _ in range(20):
                    L.check(lib.vnm_dict_take_compact(codes.ptr, rows, nk, G, vt, out.ptr, bits.ptr, ctypes.byref(nulls), used.ptr, ctypes.byref(n_used), None))
                per = (time.perf_counter() - t0) / 20
                best = per if best is None else min(best, per)
            print(f"G={G:>8d} {np.dtype(index_type).name:5s} rows={rows_name:11s} {form:6s} table: {best * 1e3:7.3f} ms  {nk / best / 1e9:6.2f} Grows/s  "
                  f"{moved / best / 1e9:7.1f} GB/s ({moved / 1e6:.0f} MB moved, {nk} rows, {n_used.value} ids used)", flush=True)
    os.environ.pop("VNM_DICT_COMPACT_LDS", None)
    del codes, out, bits, used
