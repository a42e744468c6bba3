"""A dictionary-typed string key column (dictionary<intN, utf8>) from HOST record batches, PCIe included: `GROUP BY c` and
`WHERE c = 'x'` through the planner, three ways --
  (a) the dictionary-typed column on the device route (the batch dictionary's values through vnm_strdict_encode, the indices through
      vnm_strdict_remap_indices);
  (b) the same data as plain utf8, the existing device route (every row hashed by vnm_strdict_encode);
  (c) the dictionary-typed column on the HOST route, what such a column took before it had a device route (Arrow dictionary_encode +
      index_in + NumPy merges; switched on here by taking the device route away from dictionary types; on a tenth of the rows) --
for 100 / 1e5 / 5e6 distinct 11-byte values with int8 (100 only) and int32 indices; then the remap kernel alone in rows/s and
bytes/s over at least 1e8 rows, the table read from global memory (VNM_REMAP_LDS=0) and -- up to 8192 values, VNM_REMAP_LDS=1 -- from LDS.
usage: dictcol_bench.py [rows]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import pyarrow as pa

from vinum_amd import _lib as L
from vinum_amd import keydict, planner, vinum_lib
from vinum_amd.device import DeviceBuffer, physical_type

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
rng = np.random.default_rng(0)
lib = L.lib()


def timed(query, table, reps=3):
    best = None
    for _ in range(reps):                  # (the first run also grows the pool; the best is reported)
        t0 = time.perf_counter()
        out = planner.execute(query, table)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out.num_rows


class host_route:
    """dictionary types lose the device route inside: KeyDictionary takes Arrow dictionary_encode + index_in for them"""

    def __enter__(self):        # (in both modules that look the function up: KeyDictionary's own and the aggregates')
        self._was = keydict.device_value_type
        keydict.device_value_type = vinum_lib.device_value_type = lambda t: None if pa.types.is_dictionary(t) else self._was(t)

    def __exit__(self, *exc):
        keydict.device_value_type = vinum_lib.device_value_type = self._was


print(f"rows {n}", flush=True)
for G in (100, 100_000, 5_000_000):
    values = pa.array([f"cty_{i:07d}" for i in range(G)])
    raw = rng.integers(0, G, n)
    for index_type in ((np.int8, np.int32) if G <= 127 else (np.int32,)):
        idx = pa.array(raw.astype(index_type))
        as_dict = pa.table({"c": pa.DictionaryArray.from_arrays(idx, values)})
        as_utf8 = pa.table({"c": values.take(idx)})
        x = values[G // 2].as_py()
        queries = {"GROUP BY c": {"select": ["c", ["fn", "count_star"]], "group_by": ["c"]},
                   "WHERE c = 'x'": {"select": [["fn", "count_star"]], "where": ["eq", "c", ["lit", x]]}}
        for what, q in queries.items():
            line = f"G={G:>8d} {np.dtype(index_type).name:5s} {what:14s}"
            ta, rows_a = timed(q, as_dict)
            tb, rows_b = timed(q, as_utf8)
            line += f" (a) dictionary {n / ta / 1e6:8.1f} Mrows/s  (b) utf8 {n / tb / 1e6:8.1f} Mrows/s"
            sub = as_dict.slice(0, n // 10)
            try:
                with host_route():
                    tc, _ = timed(q, sub, reps=1)
                line += f"  (c) host route {len(sub) / tc / 1e6:8.1f} Mrows/s"
            except Exception as e:             # (the host route has no way from a string literal to a code of a dictionary-typed column)
                line += f"  (c) host route: {type(e).__name__}: {str(e)[:90]}"
            print(line + f"   [(a) {idx.nbytes / 1e6:.0f} MB of indices, (b) {as_utf8.nbytes / 1e6:.0f} MB of offsets + bytes; {rows_a} / {rows_b} result rows]",
                  flush=True)

print("the remap kernel alone (device buffers; 2 alternating rounds of 50 launches per form):", flush=True)
nk = max(n, 100_000_000)            # (indices + codes well beyond the 256 MiB last-level cache: the rate is HBM's, not the cache's)
for G, index_type in ((100, np.int8), (100, np.int32), (8192, np.int32), (100_000, np.int32), (5_000_000, np.int32)):
    idx = rng.integers(0, G, nk).astype(index_type)
    d = L.DCol()
    dvals = DeviceBuffer.from_host(idx)
    d.values, d.validity, d.offset, d.length, d.type, d.flags = dvals.ptr, None, 0, nk, physical_type(pa.from_numpy_dtype(idx.dtype))[0], 0
    table = DeviceBuffer.from_host(rng.permutation(G).astype(np.int32))
    out, bits = DeviceBuffer(nk * 4), DeviceBuffer((nk + 7) >> 3)
    moved = idx.nbytes + nk * 4 + ((nk + 7) >> 3)
    forms = ("global", "lds") if G <= 8192 else ("global",)
    for rnd in range(2):
        for form in forms:
            os.environ["VNM_REMAP_LDS"] = "1" if form == "lds" else "0"
            L.check(lib.vnm_strdict_remap_indices(ctypes.byref(d), table.ptr, G, out.ptr, bits.ptr, None, None))      # warm-up
            L.check(lib.vnm_device_synchronize())
            lib.vnm_set_profiling(1)
            for _ in range(50):
                L.check(lib.vnm_strdict_remap_indices(ctypes.byref(d), table.ptr, G, out.ptr, bits.ptr, None, None))
            ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
            lib.vnm_profile_query(b"strdict_remap_indices", ctypes.byref(ms), ctypes.byref(cnt))
            lib.vnm_set_profiling(0)
            per = ms.value / max(cnt.value, 1) / 1e3
            print(f"G={G:>8d} {idx.dtype.name:5s} {form:6s} table, round {rnd}: {per * 1e3:7.3f} ms  {nk / per / 1e9:7.2f} Grows/s  "
                  f"{moved / per / 1e9:7.1f} GB/s ({moved / 1e6:.0f} MB moved, {nk} rows)", flush=True)
    os.environ.pop("VNM_REMAP_LDS", None)
    del dvals, out, bits, table
