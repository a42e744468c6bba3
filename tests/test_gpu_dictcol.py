"""Dictionary-typed string columns (dictionary<intN, utf8 | large_utf8 | binary | large_binary>) through the device dictionary:
vnm_strdict_remap_indices through raw ctypes against a NumPy model (every index type, row count, Arrow offset and table size at
which the kernel takes another path; NULL rows and NULL values; indices out of bounds; one leg under the pool's guard mode);
KeyDictionary over a stream of batches whose dictionaries differ, repeat, hold duplicates and unused values, and grow; the
queries of the string features end to end through the planner and the adapter against pyarrow over the decoded column; the
Parquet sources and vinum_lib's operators."""
import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

pytestmark = pytest.mark.gpu

T = 2048            # the kernel's rows per workgroup (VNM_STRDICT_REMAP_TILE)
INDEX_TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]


# ---- 1. the kernel through raw ctypes -----------------------------------------------------------------------------------------------
def _remap(idx: pa.Array, table: np.ndarray, with_validity=True, with_bad=True, shift_out=0):
    """idx: an Arrow integer array (sliced or not, with or without NULLs), staged with its buffers as they are so the Arrow
    offset reaches the kernel; table: int32 code per dictionary value.  Returns ((rc, error text), bad, codes, validity bytes, guard bytes)."""
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer, physical_type
    lib = L.lib()
    n, off = len(idx), idx.offset
    dt = np.dtype(idx.type.to_pandas_dtype())
    vbuf, dbuf = idx.buffers()
    vals = np.frombuffer(dbuf, dtype=dt)[:off + n] if (dbuf is not None and n) else np.zeros(0, dt)
    dvals = DeviceBuffer.from_host(vals)
    dvalid = None
    if idx.null_count and vbuf is not None:
        dvalid = DeviceBuffer.from_host(np.frombuffer(vbuf, dtype=np.uint8)[:(off + n + 7) >> 3])
    d = L.DCol()
    d.values, d.validity, d.offset, d.length = dvals.ptr, dvalid.ptr if dvalid is not None else None, off, n
    d.type, d.flags = physical_type(idx.type)[0], 0
    dtable = DeviceBuffer.from_host(np.ascontiguousarray(table, dtype=np.int32))
    nb = (n + 7) >> 3
    out = DeviceBuffer(n * 4 + 4 * shift_out + 16)
    bits = DeviceBuffer(nb + 16)
    L.check(lib.vnm_memset(out.ptr, 0x5A, out.nbytes))          # (a row the kernel skipped shows as 0x5A5A5A5A)
    L.check(lib.vnm_memset(bits.ptr, 0xA5, bits.nbytes))
    bad = ctypes.c_int64(-7)
    rc = lib.vnm_strdict_remap_indices(ctypes.byref(d), dtable.ptr, len(table), out.ptr + 4 * shift_out,
                                       bits.ptr if with_validity else None, ctypes.byref(bad) if with_bad else None, None)
    err = L.last_error() if rc else ""
    L.check(lib.vnm_device_synchronize())
    raw = out.to_host(np.int32, n + shift_out + 4)
    assert (raw[:shift_out] == 0x5A5A5A5A).all() and (raw[shift_out + n:] == 0x5A5A5A5A).all()      # nothing outside the n codes
    b = bits.to_host(np.uint8, nb + 16)
    return (rc, err), bad.value, raw[shift_out:shift_out + n], b[:nb], b[nb:]


def _model(idx: pa.Array, table: np.ndarray):
    """np.where(row_valid & (table[idx] >= 0), table[idx], -1), an index outside the table counted and -1"""
    n = len(idx)
    valid = idx.is_valid().to_numpy(zero_copy_only=False) if n else np.zeros(0, bool)
    raw = idx.fill_null(0).to_numpy(zero_copy_only=False) if n else np.zeros(0, np.int64)
    if raw.dtype.kind == "u":
        inside = raw.astype(np.uint64) < np.uint64(len(table))
    else:
        inside = (raw >= 0) & (raw.astype(np.int64) < len(table))
    at = np.where(valid & inside, raw, 0).astype(np.int64)
    looked = table[at] if len(table) else np.full(n, -1, np.int32)
    codes = np.where(valid & inside & (looked >= 0), looked, -1).astype(np.int32)
    return codes, int((valid & ~inside).sum())


def _check(idx, table, **kw):
    want, want_bad = _model(idx, table)
    (rc, err), bad, codes, bits, guard = _remap(idx, table, **kw)
    assert want_bad == 0 and rc == 0 and bad == 0, err
    assert np.array_equal(codes, want), np.flatnonzero(codes != want)[:10]
    if kw.get("with_validity", True):
        # bit for bit: the last partial byte included (packbits pads it with zeros: no bit is set past n), nothing behind it touched
        assert np.array_equal(bits, np.packbits(want >= 0, bitorder="little"))
        assert (guard == 0xA5).all()
    else:
        assert (bits == 0xA5).all() and (guard == 0xA5).all()
    return codes


def _table(n_values, rng, null_values=0.0):
    t = rng.permutation(np.arange(3, 3 + 2 * n_values, 2)).astype(np.int32)[:n_values]     # distinct, not the identity
    if null_values:
        t[rng.random(n_values) < null_values] = -1
    return t


def _indices(n, n_values, dtype, rng, null_rows=0.0, reach_top=True):
    raw = rng.integers(0, max(n_values, 1), n).astype(dtype)
    mask = (rng.random(n) < null_rows) if null_rows else None
    if reach_top and n and n_values:                       # one valid row holds the last index of the table
        at = rng.integers(0, n)
        raw[at] = n_values - 1
        if mask is not None:
            mask[at] = False
    if n_values == 0:
        mask = np.ones(n, bool)
    return pa.array(raw, mask=mask)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    table = _table(128, rng, null_values=0.2)
    _check(_indices(n, 128, np.int32, rng, null_rows=0.1), table)
    _check(_indices(n, 128, np.int8, rng), table)                       # no bitmap in
    _check(_indices(n, 128, np.int64, rng), table, with_validity=False)  # no bitmap out


@pytest.mark.parametrize("dtype", INDEX_TYPES)
def test_index_types(dtype):
    rng = np.random.default_rng(3)
    table = _table(100, rng, null_values=0.1)
    for n in (5, 3 * T + 5):
        _check(_indices(n, 100, np.dtype(dtype), rng, null_rows=0.15), table)
        _check(_indices(n, 100, np.dtype(dtype), rng), table)


@pytest.mark.parametrize("with_nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("offset", [0, 1, 7, 8, 13])
def test_arrow_offsets_on_a_sliced_array(offset, with_nulls):
    """the wide loads need values + offset aligned: 0 and 8 take them for every width, 1 / 7 / 13 take the element loads (13: a
    bitmap byte straddled as well); the last partial group takes the element loads either way"""
    rng = np.random.default_rng(offset)
    table = _table(90, rng, null_values=0.1)
    for dtype in (np.int8, np.uint16, np.int32, np.int64):
        for n in (T + 5, 64, 3):
            whole = _indices(offset + n + 9, 90, dtype, rng, null_rows=0.2 if with_nulls else 0.0)
            _check(whole.slice(offset, n), table)


@pytest.mark.parametrize("n_values, dtype", [(1, "int8"), (2, "int8"), (128, "int8"), (256, "uint8"), (70_000, "int32"), (70_000, "uint64")])
def test_table_sizes(n_values, dtype):
    rng = np.random.default_rng(n_values)
    table = _table(n_values, rng, null_values=0.05 if n_values > 2 else 0.0)
    idx = _indices(T + 77, n_values, np.dtype(dtype), rng, null_rows=0.1)
    top = idx.fill_null(0).to_numpy(zero_copy_only=False).max()
    assert int(top) == n_values - 1                                  # int8 reaches 127, uint8 255
    _check(idx, table)


@pytest.mark.parametrize("content", ["null_values", "null_rows", "both", "all_null_over_an_empty_dictionary"])
def test_null_rows_and_null_values(content):
    rng = np.random.default_rng(5)
    n = T + 100
    if content == "all_null_over_an_empty_dictionary":
        codes = _check(_indices(n, 0, np.int32, rng), np.zeros(0, np.int32))
        assert (codes == -1).all()
        return
    table = _table(50, rng, null_values=0.3 if content != "null_rows" else 0.0)
    idx = _indices(n, 50, np.int16, rng, null_rows=0.25 if content != "null_values" else 0.0)
    codes = _check(idx, table)
    assert (codes == -1).any() and (codes >= 0).any()
    if content == "null_values":
        assert idx.null_count == 0


@pytest.mark.parametrize("form", ["0", "1"], ids=["table_through_l2", "table_in_lds"])
def test_both_table_forms(form, monkeypatch):
    """VNM_REMAP_LDS pins the form the launch would otherwise choose by the sizes: 8192 values is the largest table the LDS form
    takes, 8193 goes through L2 whatever the switch says; several tiles per workgroup of the persistent grid"""
    monkeypatch.setenv("VNM_REMAP_LDS", form)
    rng = np.random.default_rng(13)
    for n_values, dtype, n in ((1, np.int8, 70), (100, np.uint8, 5 * T + 3), (8192, np.int16, 3 * T + 5), (8193, np.int32, T + 1)):
        table = _table(n_values, rng, null_values=0.1 if n_values > 1 else 0.0)
        _check(_indices(n, n_values, dtype, rng, null_rows=0.1), table)
    table = _table(300, rng)
    _check(_indices(2500 * T + 11, 300, np.int32, rng), table)          # more tiles than the persistent grid holds workgroups


def test_unaligned_output_takes_the_element_stores():
    rng = np.random.default_rng(9)
    table = _table(40, rng)
    _check(_indices(T + 9, 40, np.int32, rng, null_rows=0.1), table, shift_out=1)


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "uint8", "uint64"])
def test_an_index_out_of_bounds_is_counted_and_never_loaded(dtype):
    """-1 and n_values on valid rows: non-zero, *out_bad counts exactly those rows, every other row is right.  (The bounds test
    precedes the table load; the table here is the whole allocation, so a load behind it would be a guard-mode violation too.)"""
    rng = np.random.default_rng(11)
    dt = np.dtype(dtype)
    n_values = 100
    table = _table(n_values, rng, null_values=0.1)
    n = 2 * T + 31
    raw = rng.integers(0, n_values, n).astype(dt)
    mask = rng.random(n) < 0.1
    outside = [n_values] + ([-1, -100] if dt.kind == "i" else [np.iinfo(dt).max])
    where = rng.choice(n, 40, replace=False)
    raw[where] = [outside[i % len(outside)] for i in range(40)]
    mask[where[:30]] = False                                  # 30 of them on valid rows, the rest on whatever the mask says
    idx = pa.array(raw, mask=mask)
    want, want_bad = _model(idx, table)
    assert want_bad >= 30
    (rc, err), bad, codes, bits, guard = _remap(idx, table)
    assert rc != 0 and "dictionary index out of bounds" in err
    assert bad == want_bad
    assert np.array_equal(codes, want) and (codes[where] == -1).all()
    assert np.array_equal(bits, np.packbits(want >= 0, bitorder="little")) and (guard == 0xA5).all()
    # without out_bad the launch is asynchronous and such rows are -1
    (rc, _), bad, codes, bits, _ = _remap(idx, table, with_bad=False)
    assert rc == 0 and bad == -7 and np.array_equal(codes, want)


def test_refusals():
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib = L.lib()
    buf = DeviceBuffer(64)
    d = L.DCol()
    d.values, d.validity, d.offset, d.length, d.type, d.flags = buf.ptr, None, 0, 4, L.F32, 0
    assert lib.vnm_strdict_remap_indices(ctypes.byref(d), buf.ptr, 4, buf.ptr, None, None, None) != 0
    assert "integer type" in L.last_error()
    d.type = L.I32
    assert lib.vnm_strdict_remap_indices(ctypes.byref(d), None, 4, buf.ptr, None, None, None) != 0
    assert lib.vnm_strdict_remap_indices(ctypes.byref(d), buf.ptr, -1, buf.ptr, None, None, None) != 0
    assert lib.vnm_strdict_remap_indices(None, buf.ptr, 4, buf.ptr, None, None, None) != 0


def test_under_the_pool_guard():
    """the same selection with every allocation red-zoned and poisoned (as tests/test_gpu_in_set.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        test_row_counts(1)
        test_row_counts(65)
        test_row_counts(T - 1)
        test_row_counts(3 * T + 5)
        test_index_types("int8")
        test_index_types("uint64")
        test_arrow_offsets_on_a_sliced_array(13, True)
        test_arrow_offsets_on_a_sliced_array(8, False)
        test_table_sizes(256, "uint8")
        test_table_sizes(70_000, "int32")
        test_null_rows_and_null_values("all_null_over_an_empty_dictionary")
        test_an_index_out_of_bounds_is_counted_and_never_loaded("int8")
        test_an_index_out_of_bounds_is_counted_and_never_loaded("uint64")
        test_a_stream_of_batches()
        lib.vnm_device_synchronize()
        v, c = ctypes.c_int64(0), ctypes.c_int64(0)
        need = lib.vnm_pool_guard_report(None, 0, ctypes.byref(v), ctypes.byref(c))
        buf = ctypes.create_string_buffer(int(need) + 65536)
        lib.vnm_pool_guard_report(buf, len(buf), ctypes.byref(v), ctypes.byref(c))
        assert v.value == 0, buf.value.decode()
        assert c.value > 0
    finally:
        lib.vnm_pool_set_guard(0)
        lib.vnm_pool_guard_reset()


# ---- 2. KeyDictionary over a stream ---------------------------------------------------------------------------------------------------
def _dict_array(indices, values, index_type=pa.int8(), value_type=pa.string(), mask=None, ordered=False):
    values = values if isinstance(values, pa.Array) else pa.array(values, value_type)
    return pa.DictionaryArray.from_arrays(pa.array(np.asarray(indices), index_type, mask=mask), values, ordered=ordered)


def test_a_stream_of_batches():
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    rng = np.random.default_rng(21)
    t = pa.dictionary(pa.int8(), pa.string())
    kd = KeyDictionary(t)
    d0 = pa.array(["b", "añ", "c", "東京"])
    d2 = pa.array(["c", "x", "c", "añ", "unused", "x"])                    # duplicates and a value no row uses
    d3 = pa.array(["b", "añ", "c", "東京"] + [f"w{i:03d}" for i in range(100)])   # d0 grown
    d4 = pa.array(d0.to_pylist())                                           # d0's content in other buffers

    def draw(d, n=500, avoid=()):
        ok = [i for i in range(len(d)) if i not in avoid]
        return np.array([ok[i] for i in rng.integers(0, len(ok), n)])
    batches = [(draw(d0), d0, 1), (draw(d0), d0, 1), (draw(d2, avoid=(4,)), d2, 2), (draw(d3, 3000), d3, 3), (draw(d4), d4, 4),
               (draw(d4), d4, 4), (draw(d0), d0, 5)]
    code_of, value_of = {}, {}
    for indices, d, encodes in batches:
        mask = rng.random(len(indices)) < 0.1
        arr = _dict_array(indices, d, mask=mask)
        col = DeviceColumn.from_arrow(arr, dictionary=kd)
        assert kd.values_encodes == encodes                                  # skipped exactly when the dictionary's buffers repeat
        assert col.arrow_type == pa.int32() and col.dictionary is kd and len(col) == len(arr)
        codes = col.to_numpy()
        vals = arr.cast(pa.string()).to_pylist()
        for c, v in zip(codes.tolist(), vals):
            assert (c < 0) == (v is None)
            if v is not None:                                               # equal bytes <=> equal code, across batches
                assert code_of.setdefault(v, c) == c and value_of.setdefault(c, v) == v
        back = col.to_arrow()
        assert back.type == t and back.cast(pa.string()).equals(arr.cast(pa.string()))
        assert kd.encode(arr).to_pylist() == [None if c < 0 else c for c in codes.tolist()]
    assert kd.remap_launches == 2 * len(batches)
    assert kd.code_of("unused") is not None and kd.code_of("unused") not in value_of      # entered the dictionary, used by no row
    assert kd.code_of("nowhere") is None
    assert len(code_of) == 4 + 1 + 100


@pytest.mark.parametrize("index_type", [pa.int8(), pa.uint16(), pa.int64()], ids=str)
@pytest.mark.parametrize("value_type", [pa.string(), pa.large_string(), pa.binary(), pa.large_binary()], ids=str)
def test_slices_chunks_and_types(value_type, index_type):
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    rng = np.random.default_rng(4)
    words = ["", "a", "ab", "zürich", "a\0", "東京都", "m" * 40] + [f"k{i}" for i in range(60)]
    values = pa.array([w.encode() for w in words], pa.binary()).cast(value_type)
    t = pa.dictionary(index_type, value_type, True)
    kd = KeyDictionary(t)
    whole = _dict_array(rng.integers(0, len(words), 5000), values, index_type, value_type, mask=rng.random(5000) < 0.1, ordered=True)
    encodes, before = 0, None
    for piece in (whole.slice(13, 4000), whole.slice(0, 0), pa.chunked_array([whole.slice(0, 100), whole.slice(100, 50)]), whole):
        col = DeviceColumn.from_arrow(piece, dictionary=kd)
        back = col.to_arrow()
        want = piece.combine_chunks() if isinstance(piece, pa.ChunkedArray) else piece
        assert back.type == t and back.type.ordered
        assert back.cast(value_type).equals(want.cast(value_type))
        if len(want):                        # (slices share the dictionary's buffers; whether combined chunks do is Arrow's business)
            now = [(b.address, b.size) if b is not None else None for b in want.dictionary.buffers()]
            encodes, before = encodes + (now != before), now
        assert kd.values_encodes == encodes
    assert 1 <= encodes <= 3


def test_a_bad_index_raises_what_validate_full_says():
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    arr = pa.DictionaryArray.from_arrays(pa.array([0, 1, 2, None], pa.int8()), pa.array(["a", "b"]), safe=False)
    with pytest.raises(pa.ArrowInvalid, match="out of bounds"):
        arr.validate(full=True)
    kd = KeyDictionary(arr.type)
    with pytest.raises(L.VinumHipError, match="dictionary index out of bounds"):
        DeviceColumn.from_arrow(arr, dictionary=kd)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------
N_BATCH, BATCHES = 2000, 3
POOL = ["a", "ab", "añb", "aß", "abc", "b", "bär", "m", "mm", "ma", "x", "zürich", "東京", "東", "Ωmega", "l", "lz"] + [f"v{i:02d}é" for i in range(43)]
IN3 = ["ab", "東京", "nowhere"]
IN20 = POOL[3:21] + ["nowhere", "else"]
_TABLES = {}


def _is_bin(t):
    return pa.types.is_binary(t) or pa.types.is_large_binary(t)


def _table_of(value_type, index_type):
    """k: row id, g: 5 groups, v: small integers as float64, c / d: dictionary-typed (three batches, three dictionaries, ~10 % NULL
    rows, multi-byte values), s: plain utf8.  Returns (table, the same with c and d decoded to their value type)"""
    key = (str(value_type), str(index_type))
    if key in _TABLES:
        return _TABLES[key]
    rng = np.random.default_rng(31)
    mk = (lambda xs: pa.array([x.encode() for x in xs], value_type)) if _is_bin(value_type) else (lambda xs: pa.array(xs, value_type))
    other_index = pa.int32() if index_type == pa.int8() else pa.int16()
    batches = []
    for b in range(BATCHES):
        words = [POOL[i] for i in rng.permutation(len(POOL))[:40]]         # another dictionary, in another order, per batch
        dwords = [POOL[i] for i in rng.permutation(len(POOL))[:35]]
        ci = rng.integers(0, len(words), N_BATCH)
        c = _dict_array(ci, mk(words), index_type, value_type, mask=rng.random(N_BATCH) < 0.1)
        # d agrees with c on about a third of the rows, s on another third
        di = np.array([dwords.index(words[i]) if (words[i] in dwords and r < 0.5) else j
                       for i, j, r in zip(ci, rng.integers(0, len(dwords), N_BATCH), rng.random(N_BATCH))])
        d = _dict_array(di, mk(dwords), other_index, value_type, mask=rng.random(N_BATCH) < 0.1)
        s = pa.array([words[i] if r < 0.3 else POOL[j] for i, j, r in zip(ci, rng.integers(0, len(POOL), N_BATCH), rng.random(N_BATCH))],
                     pa.string(), mask=rng.random(N_BATCH) < 0.05)
        batches.append(pa.RecordBatch.from_arrays(
            [pa.array(np.arange(b * N_BATCH, (b + 1) * N_BATCH, dtype=np.int64)), pa.array(rng.integers(0, 5, N_BATCH).astype(np.int64)),
             pa.array(rng.integers(0, 100, N_BATCH).astype(np.float64)), c, d, s], names=["k", "g", "v", "c", "d", "s"]))
    t = pa.Table.from_batches(batches)
    o = t.set_column(3, "c", t["c"].cast(value_type)).set_column(4, "d", t["d"].cast(value_type))
    _TABLES[key] = (t, o)
    return t, o


def _b(col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return col.cast(pa.large_binary())


def _lit(x, value_type):
    return x.encode() if _is_bin(value_type) else x


def _where_cases(o, value_type):
    """name -> (the WHERE tree, pyarrow's mask over the decoded table with NULL by the project's rule: compares False, != and NOT
    LIKE True)"""
    c, s, d = _b(o["c"]), _b(o["s"]), _b(o["d"])
    sc = lambda x: pa.scalar(x.encode(), pa.large_binary())     # noqa: E731
    lit = lambda x: ("lit", _lit(x, value_type))                # noqa: E731
    cases = {
        "eq_lit": (("eq", "c", lit("añb")), pc.equal(c, sc("añb")).fill_null(False)),
        "eq_absent": (("eq", "c", lit("nowhere")), pc.equal(c, sc("nowhere")).fill_null(False)),
        "ne_lit": (("ne", "c", lit("añb")), pc.not_equal(c, sc("añb")).fill_null(True)),
        "lt_lit": (("lt", "c", lit("m")), pc.less(c, sc("m")).fill_null(False)),
        "ge_lit_flipped": (("le", lit("m"), "c"), pc.greater_equal(c, sc("m")).fill_null(False)),
        "in_3": (("in", "c", tuple(_lit(x, value_type) for x in IN3)),
                 pc.is_in(c, value_set=pa.array([x.encode() for x in IN3], pa.large_binary())).fill_null(False)),
        "in_20": (("in", "c", tuple(_lit(x, value_type) for x in IN20)),
                  pc.is_in(c, value_set=pa.array([x.encode() for x in IN20], pa.large_binary())).fill_null(False)),
        "not_in_20": (("not_in", "c", tuple(_lit(x, value_type) for x in IN20)),
                      pc.invert(pc.is_in(c, value_set=pa.array([x.encode() for x in IN20], pa.large_binary()))).fill_null(True)),
        "eq_utf8_column": (("eq", "c", "s"), pc.equal(c, s).fill_null(False)),
        "lt_utf8_column": (("lt", "c", "s"), pc.less(c, s).fill_null(False)),
        "gt_utf8_column_flipped": (("gt", "s", "c"), pc.greater(s, c).fill_null(False)),
        "eq_dictionary_column": (("eq", "c", "d"), pc.equal(c, d).fill_null(False)),
        "ne_dictionary_column": (("ne", "d", "c"), pc.not_equal(d, c).fill_null(True)),
        "lt_dictionary_column": (("lt", "c", "d"), pc.less(c, d).fill_null(False)),
        "mixed": (("and", ("ge", "c", "d"), ("gt", "v", 40)), pc.and_(pc.greater_equal(c, d).fill_null(False), pc.greater(o["v"].combine_chunks(), 40))),
    }
    if not _is_bin(value_type):
        text = o["c"].combine_chunks().cast(pa.large_string())
        cases["like"] = (("like", "c", ("lit", "a%")), pc.match_like(text, "a%").fill_null(False))
        cases["not_like"] = (("not_like", "c", ("lit", "a%")), pc.invert(pc.match_like(text, "a%")).fill_null(True))
        cases["like_multibyte"] = (("like", "c", ("lit", "_ä%")), pc.match_like(text, "_ä%").fill_null(False))
    return cases


COMBOS = [(pa.string(), pa.int8()), (pa.string(), pa.int32()), (pa.large_string(), pa.int8()), (pa.large_string(), pa.int32()),
          (pa.binary(), pa.int8()), (pa.binary(), pa.int32())]
_ids = lambda x: str(x) if isinstance(x, pa.DataType) else None     # noqa: E731


def _assert_carries(got_col, want_col, dict_type):
    """a result column that carries c: the dictionary type, equal to the oracle after the cast"""
    got_col = got_col.combine_chunks() if isinstance(got_col, pa.ChunkedArray) else got_col
    want_col = want_col.combine_chunks() if isinstance(want_col, pa.ChunkedArray) else want_col
    assert got_col.type == dict_type, got_col.type
    assert got_col.cast(dict_type.value_type).to_pylist() == want_col.to_pylist()


@pytest.mark.parametrize("value_type, index_type", COMBOS, ids=_ids)
def test_where_through_the_planner(value_type, index_type):
    from vinum_amd import planner, set_batch_size
    t, o = _table_of(value_type, index_type)
    set_batch_size(N_BATCH)
    try:
        for name, (where, mask) in _where_cases(o, value_type).items():
            got = planner.execute({"select": ["k", "c"], "where": where}, t)
            want = o.filter(mask)
            assert want.num_rows > 0 or name == "eq_absent", name
            assert got.column("k").to_pylist() == want.column("k").to_pylist(), name
            _assert_carries(got.column("c"), want.column("c"), t.schema.field("c").type)
    finally:
        set_batch_size(1 << 24)


def test_like_over_a_dictionary_of_binary_raises():
    from vinum_amd import planner
    t, _ = _table_of(pa.binary(), pa.int8())
    with pytest.raises(TypeError, match="LIKE needs a string column"):
        planner.execute({"select": ["k"], "where": ["like", "c", ["lit", "a%"]]}, t)


@pytest.mark.parametrize("value_type, index_type", COMBOS, ids=_ids)
def test_group_by_order_by_and_select_through_the_planner(value_type, index_type):
    from vinum_amd import planner, set_batch_size
    t, o = _table_of(value_type, index_type)
    dict_type = t.schema.field("c").type
    set_batch_size(N_BATCH)
    try:
        got = planner.execute({"select": ["c", ["fn", "count_star"], ["fn", "sum", "v"], ["fn", "count", "c"]], "group_by": ["c"],
                               "aliases": [None, "n", "total", "nc"]}, t)
        sel = planner.execute({"select": ["c"]}, t)
        srt = planner.execute({"select": ["c", "k"], "order_by": ["c", "k"], "sort_order": ["DESC", "ASC"]}, t)
        top = planner.execute({"select": ["k", "c"], "order_by": ["c", "k"], "sort_order": ["ASC", "DESC"], "limit": 50}, t)
    finally:
        set_batch_size(1 << 24)
    # GROUP BY c: NULL is one group
    want = o.group_by("c").aggregate([([], "count_all"), ("v", "sum"), ("c", "count")])
    assert got.column("c").type == dict_type
    keys = got.column("c").combine_chunks().cast(value_type).to_pylist()
    assert len(keys) == len(set(keys)) == want.num_rows and None in keys
    assert dict(zip(keys, zip(got["n"].to_pylist(), got["total"].to_pylist(), got["nc"].to_pylist()))) == \
        dict(zip(want["c"].to_pylist(), zip(want["count_all"].to_pylist(), want["v_sum"].to_pylist(), want["c_count"].to_pylist())))
    # SELECT c
    _assert_carries(sel.column("c"), o["c"], dict_type)
    # ORDER BY c DESC, k: byte order, NULLs last
    ob = pa.table({"c": _b(o["c"]), "k": o["k"]})
    idx = pc.sort_indices(ob, sort_keys=[("c", "descending"), ("k", "ascending")])
    assert srt.column("k").to_pylist() == o["k"].take(idx).to_pylist()
    _assert_carries(srt.column("c"), o["c"].take(idx), dict_type)
    idx = pc.sort_indices(ob, sort_keys=[("c", "ascending"), ("k", "descending")]).slice(0, 50)
    assert top.column("k").to_pylist() == o["k"].take(idx).to_pylist()
    _assert_carries(top.column("c"), o["c"].take(idx), dict_type)


@pytest.mark.parametrize("value_type, index_type", [(pa.string(), pa.int8()), (pa.large_string(), pa.int32()), (pa.binary(), pa.int32())], ids=_ids)
def test_through_the_adapter(value_type, index_type):
    """binding.GpuFilterOperator / GpuProjectOperator over binding.vectorize trees (binding.lower and the lowering behind it), as
    tests/test_gpu_strcmp.py drives the adapter"""
    from vinum_amd import binding as B
    from vinum_amd import set_batch_size
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    t, o = _table_of(value_type, index_type)
    cases = _where_cases(o, value_type)
    set_batch_size(N_BATCH)
    try:
        for name, (where, mask) in cases.items():
            op = B.GpuFilterOperator(B.vectorize(where), TableReaderOperator(t))
            op = B.GpuProjectOperator([B.vectorize("k"), B.vectorize("c")], op, col_names=["k", "c"])
            got = next(MaterializeTableOperator(op).next())
            want = o.filter(mask)
            assert got.column("k").to_pylist() == want.column("k").to_pylist(), name
            _assert_carries(got.column("c"), want.column("c"), t.schema.field("c").type)
        # predicates in the SELECT list: uint8 masks
        names = [n for n in cases if n != "mixed"]
        op = B.GpuProjectOperator([B.vectorize("k")] + [B.vectorize(cases[n][0]) for n in names], TableReaderOperator(t), col_names=["k"] + names)
        got = next(MaterializeTableOperator(op).next())
        for n in names:
            assert got.schema.field(n).type == pa.uint8()
            assert np.array_equal(got[n].to_numpy().astype(bool), cases[n][1].to_numpy(zero_copy_only=False)), n
    finally:
        set_batch_size(1 << 24)


def _min_max_oracle(o, key):
    want = {}
    for g, c in zip(o[key].to_pylist(), _b(o["c"]).to_pylist()):
        lo, hi = want.get(g, (None, None))
        if c is not None:
            lo, hi = (c if lo is None or c < lo else lo), (c if hi is None or c > hi else hi)
        want[g] = (lo, hi)
    return want


@pytest.mark.parametrize("value_type, index_type", COMBOS, ids=_ids)
def test_string_min_max(value_type, index_type):
    """min(c), max(c) per group through vinum_lib's operators (_StringMinMax: ranks on the device), batch by batch"""
    from vinum_amd import vinum_lib as V
    t, o = _table_of(value_type, index_type)
    dict_type = t.schema.field("c").type
    op = V.SingleNumericalHashAggregate(["g"], ["g"], [V.AggFuncDef(V.MIN, "c", "lo"), V.AggFuncDef(V.MAX, "c", "hi"), V.AggFuncDef(V.COUNT, "c", "n")])
    for b in t.to_batches():
        op.next(b)
    got = op.result()
    assert got.schema.field("lo").type == dict_type and got.schema.field("hi").type == dict_type
    lo, hi = _b(got.column("lo").cast(value_type)).to_pylist(), _b(got.column("hi").cast(value_type)).to_pylist()
    assert dict(zip(got.column("g").to_pylist(), zip(lo, hi))) == _min_max_oracle(o, "g")
    counts = o.group_by("g").aggregate([("c", "count")])
    assert dict(zip(got.column("g").to_pylist(), got.column("n").to_pylist())) == dict(zip(counts["g"].to_pylist(), counts["c_count"].to_pylist()))
    one = V.OneGroupAggregate([V.AggFuncDef(V.MIN, "c", "lo"), V.AggFuncDef(V.MAX, "c", "hi"), V.AggFuncDef(V.COUNT_STAR, "", "n")])
    for b in t.to_batches():
        one.next(b)
    res = one.result()
    assert res.column("n").to_pylist() == [o.num_rows]
    everything = [x for x in _b(o["c"]).to_pylist() if x is not None]
    assert _b(res.column("lo").cast(value_type)).to_pylist() == [min(everything)] and _b(res.column("hi").cast(value_type)).to_pylist() == [max(everything)]


def test_a_row_pointing_at_a_null_value_is_a_null_row():
    """pyarrow's own group_by over the undecoded column keeps `NULL row` and `row -> NULL value` apart; here, as after a cast to the
    value type, both are NULL: one group, compares False, != True"""
    from vinum_amd import planner
    n = 3000
    rng = np.random.default_rng(8)
    idx = rng.integers(0, 4, n)
    c = _dict_array(idx, pa.array(["a", None, "b", "añ"]), pa.int8(), pa.string(), mask=rng.random(n) < 0.1)
    assert c.null_count < c.cast(pa.string()).null_count
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(np.ones(n)), "c": c})
    o = t.set_column(2, "c", c.cast(pa.string()))
    got = planner.execute({"select": ["c", ["fn", "count_star"]], "group_by": ["c"], "aliases": [None, "n"]}, t)
    want = o.group_by("c").aggregate([([], "count_all")])
    assert got.num_rows == 4 and got.column("c").type == c.type
    assert dict(zip(got.column("c").combine_chunks().cast(pa.string()).to_pylist(), got["n"].to_pylist())) == \
        dict(zip(want["c"].to_pylist(), want["count_all"].to_pylist()))
    ne = planner.execute({"select": ["k"], "where": ["ne", "c", ["lit", "a"]]}, t)
    assert ne.column("k").to_pylist() == o.filter(pc.not_equal(o["c"], "a").fill_null(True)).column("k").to_pylist()
    sel = planner.execute({"select": ["c"]}, t)
    assert sel.column("c").combine_chunks().cast(pa.string()).equals(o["c"].combine_chunks())


# ---- 4. entry points --------------------------------------------------------------------------------------------------------------------
def _parquet(tmp_path):
    import pyarrow.parquet as pq
    t, o = _table_of(pa.string(), pa.int32())
    path = str(tmp_path / "dictcol.parquet")
    pq.write_table(o, path, row_group_size=1500)
    return path, o


def test_stream_parquet_with_read_dictionary(tmp_path):
    from vinum_amd import io
    path, o = _parquet(tmp_path)
    src = io.stream_parquet(path, batch_rows=2500, read_dictionary=["c", "d"])
    rows, kd = 0, None
    for batch in src:
        col = batch.column("c")
        kd = kd or col.dictionary
        assert col.dictionary is kd and kd.on_device and pa.types.is_dictionary(kd.type)
        back = batch.to_arrow()
        assert back.schema.field("c").type == pa.dictionary(pa.int32(), pa.string())
        assert back.column("c").cast(pa.string()).equals(o["c"].combine_chunks().slice(rows, batch.num_rows))
        assert back.column("k").to_pylist() == o["k"].slice(rows, batch.num_rows).to_pylist()
        rows += batch.num_rows
    assert rows == o.num_rows and kd.remap_launches >= 3 and kd.values_encodes >= 1


def test_read_parquet_with_read_dictionary_feeds_the_operators(tmp_path):
    from vinum_amd import io
    from vinum_amd.core import FilterOperator
    path, o = _parquet(tmp_path)
    batch = io.read_parquet(path, read_dictionary=["c"])
    assert batch.num_rows == o.num_rows and batch.column("c").dictionary.on_device
    assert pa.types.is_dictionary(batch.column("c").dictionary.type) and batch.column("d").dictionary.type == pa.string()
    got = FilterOperator(("and", ("like", "c", ("lit", "a%")), ("eq", "c", "d")), None)._kernel(batch).to_arrow()
    mask = pc.and_(pc.match_like(o["c"], "a%").fill_null(False), pc.equal(o["c"], o["d"]).fill_null(False))
    want = o.filter(mask)
    assert want.num_rows > 0 and got.column("k").to_pylist() == want.column("k").to_pylist()
    assert got.column("c").type == pa.dictionary(pa.int32(), pa.string())


@pytest.mark.parametrize("value_type, index_type", [(pa.string(), pa.int8()), (pa.large_binary(), pa.int32())], ids=_ids)
def test_generic_hash_aggregate_with_a_dictionary_typed_key(value_type, index_type):
    from vinum_amd import vinum_lib as V
    t, o = _table_of(value_type, index_type)
    dict_type = t.schema.field("c").type
    op = V.GenericHashAggregate(["c", "g"], ["c", "g"], [V.AggFuncDef(V.COUNT_STAR, "", "n"), V.AggFuncDef(V.SUM, "v", "total"),
                                                       V.AggFuncDef(V.MIN, "c", "lo"), V.AggFuncDef(V.COUNT, "c", "nc")])
    for b in t.to_batches():
        op.next(b)
    got = op.result()
    assert got.schema.field("c").type == dict_type and got.schema.field("lo").type == dict_type
    want = o.group_by(["c", "g"]).aggregate([([], "count_all"), ("v", "sum"), ("c", "count")])
    keys = list(zip(got.column("c").cast(value_type).to_pylist(), got.column("g").to_pylist()))
    assert len(keys) == len(set(keys)) == want.num_rows
    assert dict(zip(keys, zip(got.column("n").to_pylist(), got.column("total").to_pylist(), got.column("nc").to_pylist()))) == \
        dict(zip(zip(want["c"].to_pylist(), want["g"].to_pylist()),
                 zip(want["count_all"].to_pylist(), want["v_sum"].to_pylist(), want["c_count"].to_pylist())))
    assert got.column("lo").cast(value_type).to_pylist() == got.column("c").cast(value_type).to_pylist()      # min(c) per (c, g) is c
