#!/usr/bin/env python3
"""Two dictionary-coded string columns compared on the GPU, measured (profiles/r08_strcmp.txt):
  (a) the two table builds (vnm_strdict_translate, vnm_strdict_ranks_joint) over two dictionaries of 1e3, 1e5, 5e6 distinct
      11-byte values and 1e5 200-byte values, half of the values shared;
  (b) the mask of `a = b` (one fused int32 lookup) and `a < b` (two) over 5e8 rows of codes, next to the mask of a numeric `eq`
      over two int32 columns of the same length -- the floor: the lookup adds one dependent 4-byte gather per row; that program
      runs the project_kernel<0, 0> instantiation, whose code this feature leaves as it was -- and next to materialising the
      translated column with vnm_strdict_codes_to_ranks and comparing two plain columns.
Times: median of --reps runs, each bracketed by device synchronisation (warm-up runs first)."""
import argparse
import os
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
    """n distinct values: a random body and the value's number in its last 8 bytes"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    raw = alpha[rng.integers(0, 26, (n, length))]
    num = np.arange(n)
    for k in range(8):
        raw[:, length - 1 - k] = 97 + (num // 16 ** k) % 16
    offs = np.arange(n + 1, dtype=np.int32) * length
    return pa.Array.from_buffers(pa.string(), n, [None, pa.py_buffer(offs), pa.py_buffer(raw.tobytes())])


def pair(n, length, seed):
    """two lists of n values with n / 2 in common: rows [0, n) and [n / 2, 3 n / 2) of one list of 3 n / 2 distinct values"""
    v = values(n + n // 2, length, seed)
    return v.slice(0, n), v.slice(n // 2, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=float, default=5e8)
    args = ap.parse_args()
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.device import DeviceBuffer, DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    lib = L.lib()
    print(f"device: {torch.cuda.get_device_name(0)}  reps={args.reps}")

    print("\n(a) table builds over two dictionaries of n values each, n / 2 shared")
    for n, length in ((1000, 11), (100_000, 11), (5_000_000, 11), (100_000, 200)):
        ka, kb = KeyDictionary(pa.string()), KeyDictionary(pa.string())
        va, vb = pair(n, length, 1)
        for s in range(0, n, 1 << 20):
            ka.encode(va.slice(s, 1 << 20))
            kb.encode(vb.slice(s, 1 << 20))
        ta, tb = int(lib.vnm_strdict_ids(ka.handle())), int(lib.vnm_strdict_ids(kb.handle()))
        out_a, out_b = DeviceBuffer(ta * 4), DeviceBuffer(tb * 4)
        t = timed(lambda: L.check(lib.vnm_strdict_translate(kb.handle(), ka.handle(), 0, out_b.ptr, None)), args.reps)
        found = int((out_b.to_host(np.int32, tb) >= 0).sum())
        assert found == n - n // 2, f"{found} of b's values found in a, expected {n - n // 2}"
        print(f"  {n:>9d} values x {length:3d} B  translate   {t * 1e3:9.3f} ms  {n / t / 1e9:7.3f} G values/s  ({found} present)")
        t = timed(lambda: L.check(lib.vnm_strdict_ranks_joint(ka.handle(), kb.handle(), out_a.ptr, out_b.ptr, None)), max(3, args.reps // 2))
        top = int(max(out_a.to_host(np.int32, ta).max(), out_b.to_host(np.int32, tb).max()))
        assert top == n + n // 2 - 1, f"top rank {top}, expected {n + n // 2 - 1} (the union has {n + n // 2} values)"
        print(f"  {n:>9d} values x {length:3d} B  joint ranks {t * 1e3:9.3f} ms  {2 * n / t / 1e9:7.3f} G values/s  (top rank {top})")
        del ka, kb, out_a, out_b

    n = int(args.rows)
    print(f"\n(b) masks over {n:.0e} rows of int32 codes (two dictionaries of 4096 values, 2048 shared)")
    ka, kb = KeyDictionary(pa.string()), KeyDictionary(pa.string())
    va, vb = pair(4096, 11, 3)
    ea = ka.encode(va).to_numpy(zero_copy_only=False).astype(np.int32)
    eb = kb.encode(vb).to_numpy(zero_copy_only=False).astype(np.int32)
    ca, cb = np.unique(ea), np.unique(eb)
    rows_a = torch.from_numpy(ca).cuda()[torch.randint(0, len(ca), (n,), device="cuda")].contiguous()
    rows_b = torch.from_numpy(cb).cuda()[torch.randint(0, len(cb), (n,), device="cuda")].contiguous()
    a, b = DeviceColumn.from_torch(rows_a), DeviceColumn.from_torch(rows_b)
    xl = kb.translate_table(ka)
    ra, rb = ka.joint_rank_tables(kb)
    floor = timed(lambda: ops.predicate_mask(("eq", "a", "b"), {"a": a, "b": b}, n), args.reps)
    print(f"  numeric eq over two int32 columns (the floor) {floor * 1e3:8.2f} ms  {n * 9 / floor / 1e12:5.2f} TB/s of codes + mask")
    eq = timed(lambda: ops.predicate_mask(("eq", "a", ("lookup_i32", "b", "t")), {"a": a, "b": b, "t": xl}, n), args.reps)
    print(f"  a = b, fused lookup                          {eq * 1e3:8.2f} ms  {eq / floor:5.2f} x the floor")
    lt = timed(lambda: ops.predicate_mask(("lt", ("lookup_i32", "a", "ra"), ("lookup_i32", "b", "rb")), {"a": a, "b": b, "ra": ra, "rb": rb}, n), args.reps)
    print(f"  a < b, two fused lookups                     {lt * 1e3:8.2f} ms  {lt / floor:5.2f} x the floor")
    tmp = DeviceBuffer(n * 4)
    tcol = DeviceColumn(tmp, None, 0, n, pa.int32())

    def materialised():
        L.check(lib.vnm_strdict_codes_to_ranks(b.values_ptr, xl.values_ptr, n, tmp.ptr, None))
        return ops.predicate_mask(("eq", "a", "x"), {"a": a, "x": tcol}, n)
    mt = timed(materialised, args.reps)
    print(f"  a = b, translated column materialised first  {mt * 1e3:8.2f} ms  {mt / floor:5.2f} x the floor  (fused / materialised = {eq / mt:4.2f})")
    # what the masks must count, from the host's view of the values: ranks in the sorted union, equal bytes sharing one
    order = {v: r for r, v in enumerate(sorted(set(va.to_pylist()) | set(vb.to_pylist()), key=str.encode))}
    ha, hb = np.zeros(ea.max() + 1, np.int64), np.zeros(eb.max() + 1, np.int64)
    ha[ea], hb[eb] = [order[v] for v in va.to_pylist()], [order[v] for v in vb.to_pylist()]
    wa, wb = torch.from_numpy(ha).cuda()[rows_a.long()], torch.from_numpy(hb).cuda()[rows_b.long()]
    want_eq, want_lt = int((wa == wb).sum()), int((wa < wb).sum())
    del wa, wb
    k = int(ops.predicate_mask(("eq", "a", ("lookup_i32", "b", "t")), {"a": a, "b": b, "t": xl}, n).to_host(np.uint8, n).sum(dtype=np.int64))
    m = int(ops.predicate_mask(("lt", ("lookup_i32", "a", "ra"), ("lookup_i32", "b", "rb")), {"a": a, "b": b, "ra": ra, "rb": rb}, n).to_host(np.uint8, n).sum(dtype=np.int64))
    print(f"  ({k} rows equal, {m} rows less; the host's ranks give {want_eq} and {want_lt})")
    assert (k, m) == (want_eq, want_lt) and k > 0


if __name__ == "__main__":
    main()
