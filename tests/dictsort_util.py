"""Shared by tests/test_dictsort_cpu.py and tests/test_gpu_dictsort.py: the NumPy model of vnm_dict_take_compact (checked against
pyarrow by the CPU tests, compared bit for bit with the kernels by the GPU tests) and the tables both Sort legs run over."""
import numpy as np
import pyarrow as pa

INDEX_TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]
VALUE_TYPES = [pa.string(), pa.large_string(), pa.binary(), pa.large_binary()]
OVERFLOW = "These dictionaries cannot be combined.  The unified dictionary requires a larger index type."


def take_compact_model(codes, rows, n_ids, index_dtype):
    """c_i = codes[rows[i]] (rows None: identity).  Returns a dict: used_ids (ascending ids some c_i equals), indices (the position of
    c_i in used_ids in index_dtype, 0 where c_i < 0), valid, bitmap (little-endian bits, zero padded), null_count, bad (rows with a
    code >= n_ids; such rows take no part in the rest) and overflow (more used ids than the index type's largest value)."""
    codes = np.asarray(codes, dtype=np.int32)
    c = codes if rows is None else codes[np.asarray(rows, dtype=np.int64)]
    dt = np.dtype(index_dtype)
    valid = c >= 0
    inside = valid & (c < n_ids)
    used = np.unique(c[inside]).astype(np.int32)
    dense = np.where(inside, np.searchsorted(used, np.where(inside, c, 0)), 0)
    overflow = len(used) > np.iinfo(dt).max
    return {"used_ids": used, "indices": dense.astype(dt) if not overflow else None, "valid": valid,
            "bitmap": np.packbits(valid, bitorder="little"), "null_count": int((~valid).sum()), "bad": int((valid & ~inside).sum()),
            "overflow": overflow}


def dict_array(indices, values, index_type=pa.int8(), value_type=pa.string(), mask=None, ordered=False):
    values = values if isinstance(values, pa.Array) else pa.array(values, value_type)
    return pa.DictionaryArray.from_arrays(pa.array(np.asarray(indices), index_type, mask=mask), values, ordered=ordered)


def is_bin(t):
    return pa.types.is_binary(t) or pa.types.is_large_binary(t)


POOL = ["", "a", "ab", "añb", "aß", "abc", "b", "bär", "m", "mm", "ma", "x", "zürich", "東京", "東", "Ωmega", "l", "lz"] + [f"v{i:02d}é" for i in range(42)]


def sort_table(value_type, index_type, n=2003, seed=31, ordered=False, pool=POOL):
    """Batches over columns k (row id), g (int64, 5 values: ties), v (float64), c (dictionary-typed) and s (plain utf8): three
    dictionaries in different orders, each with a NULL value and a value no row uses; ~10 % NULL rows; the first batch a slice at
    Arrow offset 13 and the third at offset 1; lengths that are no multiples of 8; the last batch repeats the third's dictionary
    buffers.  Returns (batches, the table with c decoded to its value type)."""
    rng = np.random.default_rng(seed)
    mk = (lambda xs: pa.array([None if x is None else x.encode() for x in xs], value_type)) if is_bin(value_type) else (lambda xs: pa.array(xs, value_type))
    if n >= 40:
        lens = [n // 3 + 1, n // 4 + 3, n // 5 + 2]
        lens.append(n - sum(lens))
    else:                                                          # (tiny tables: random cuts, empty batches among them)
        cuts = [0] + sorted(rng.integers(0, n + 1, 3).tolist()) + [n]
        lens = [b - a for a, b in zip(cuts, cuts[1:])]
    per_dict = min(len(pool), 40)
    batches, row0, values = [], 0, None
    for b, m in enumerate(lens):
        if b < 3:                                                  # (batch 3 shares batch 2's dictionary)
            words = [pool[i] for i in rng.permutation(len(pool))[:per_dict]]
            words.insert(int(rng.integers(0, len(words))), None)     # a NULL value some rows point at
            values = mk(words)
            unused = int(rng.integers(0, len(words)))
            if words[unused] is None:
                unused = (unused + 1) % len(words)
        off = {0: 13, 2: 1}.get(b, 0)
        ci = rng.integers(0, len(words), m + off)
        ci[ci == unused] = (unused + 1) % len(words)
        c = dict_array(ci, values, index_type, value_type, mask=rng.random(m + off) < 0.1, ordered=ordered).slice(off, m)
        s = pa.array([pool[j] for j in rng.integers(0, len(pool), m)], pa.string(), mask=rng.random(m) < 0.05)
        batches.append(pa.RecordBatch.from_arrays(
            [pa.array(np.arange(row0, row0 + m, dtype=np.int64)), pa.array(rng.integers(0, 5, m).astype(np.int64)),
             pa.array(rng.integers(0, 100, m).astype(np.float64)), c, s], names=["k", "g", "v", "c", "s"]))
        row0 += m
    t = pa.Table.from_batches(batches)
    decoded = t.set_column(3, "c", pa.chunked_array([b.column(3).cast(value_type) for b in batches], value_type))
    return batches, decoded.combine_chunks()
