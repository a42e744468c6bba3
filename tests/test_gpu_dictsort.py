"""Dictionary-typed string columns (dictionary<intN, utf8 | large_utf8 | binary | large_binary>) below the C ABI of Sort and the aggregates:
vnm_dict_take_compact through raw ctypes against the NumPy model of tests/dictsort_util.py (exact: every row count, id count, index
type and alignment at which the kernels take another path); vnm_sort_op_* through raw ctypes and vinum_lib.Sort against pyarrow
over the decoded column; vnm_agg_op_* through raw ctypes and vinum_lib.GenericHashAggregate against pyarrow group_by over the decoded
column; one leg under the pool's guard mode."""
import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests.dictsort_util import INDEX_TYPES, OVERFLOW, dict_array, sort_table, take_compact_model

pytestmark = pytest.mark.gpu

T = 2048            # rows per workgroup of the gather, ids per workgroup of the scan (VNM_DICT_COMPACT_TILE)
LDS_IDS = 8192      # the largest table the LDS form takes (VNM_DICT_COMPACT_LDS_IDS)


# ---- 1. the entry point through raw ctypes --------------------------------------------------------------------------------------------
def _compact(codes, rows, n_ids, dtype, shift_out=0):
    """Returns ((rc, error text), model, got) with got = dict(indices, bitmap, null_count, used_ids, n_used); the bytes around every
    output are checked to be untouched here."""
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib = L.lib()
    dt = np.dtype(dtype)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    n = len(codes) if rows is None else len(rows)
    dcodes = DeviceBuffer.from_host(codes)
    drows = DeviceBuffer.from_host(np.ascontiguousarray(rows, dtype=np.int64)) if rows is not None else None
    w, nb, room = dt.itemsize, (n + 7) >> 3, max(min(n, n_ids), 1)
    out = DeviceBuffer((n + shift_out + 4) * w)
    bits = DeviceBuffer(nb + 16)
    used = DeviceBuffer((room + 4) * 4)
    L.check(lib.vnm_memset(out.ptr, 0x5A, out.nbytes))
    L.check(lib.vnm_memset(bits.ptr, 0xA5, bits.nbytes))
    L.check(lib.vnm_memset(used.ptr, 0x5A, used.nbytes))
    nulls, n_used = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = lib.vnm_dict_take_compact(dcodes.ptr, drows.ptr if drows is not None else None, n, n_ids, INDEX_TYPES.index(dt.name),
                                   out.ptr + w * shift_out, bits.ptr, ctypes.byref(nulls), used.ptr, ctypes.byref(n_used), None)
    err = L.last_error() if rc else ""
    L.check(lib.vnm_device_synchronize())
    raw = out.to_host(np.uint8, out.nbytes)
    assert (raw[:shift_out * w] == 0x5A).all() and (raw[(shift_out + n) * w:] == 0x5A).all()        # nothing outside the n indices
    b = bits.to_host(np.uint8, nb + 16)
    assert (b[nb:] == 0xA5).all()                                                                    # nothing behind (n + 7) / 8 bytes
    u = used.to_host(np.int32, room + 4)
    assert (u[room:] == 0x5A5A5A5A).all()
    got = {"indices": raw[shift_out * w:(shift_out + n) * w].view(dt), "bitmap": b[:nb], "null_count": nulls.value,
           "used_ids": u[:max(n_used.value, 0)], "n_used": n_used.value}
    return (rc, err), take_compact_model(codes, rows, n_ids, dt), got


def _check(codes, rows, n_ids, dtype, **kw):
    (rc, err), m, got = _compact(codes, rows, n_ids, dtype, **kw)
    assert rc == 0 and m["bad"] == 0 and not m["overflow"], err
    assert got["n_used"] == len(m["used_ids"]) and np.array_equal(got["used_ids"], m["used_ids"])
    assert np.array_equal(got["indices"], m["indices"]), np.flatnonzero(got["indices"] != m["indices"])[:10]
    assert np.array_equal(got["bitmap"], m["bitmap"])            # bit for bit: packbits pads the last byte with zeros
    assert got["null_count"] == m["null_count"]
    return got


def _codes(n, n_ids, rng, nulls=0.1):
    c = rng.integers(0, n_ids, n).astype(np.int32)
    if n:
        c[rng.integers(0, n)] = n_ids - 1                         # the last id is used
    c[rng.random(n) < nulls] = -1
    return c


def _rows(kind, n_codes, rng):
    if kind == "identity":
        return None
    p = rng.permutation(n_codes)
    return p if kind == "permutation" else p[:n_codes // 3]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    _check(_codes(n, 100, rng), None, 100, np.int8)
    _check(_codes(n, 100, rng, nulls=0.0), None, 100, np.int32)
    _check(_codes(n + 11, 100, rng), rng.permutation(n + 11)[:n], 100, np.uint16)


@pytest.mark.parametrize("form", ["0", "1"], ids=["table_through_l2", "table_in_lds"])
@pytest.mark.parametrize("n_ids", [1, 2, 255, 256, 257, LDS_IDS - 1, LDS_IDS, LDS_IDS + 1, 70_000])
def test_id_counts_and_both_table_forms(n_ids, form, monkeypatch):
    """VNM_DICT_COMPACT_LDS pins the form the launch would otherwise choose by the sizes; past 8192 ids the table goes through L2
    whatever the switch says.  5 * T + 3 rows: several tiles per workgroup of the persistent grid when there are few of them."""
    monkeypatch.setenv("VNM_DICT_COMPACT_LDS", form)
    rng = np.random.default_rng(n_ids)
    dtype = np.uint8 if n_ids <= 255 else np.int32
    for n in (70, 5 * T + 3):
        _check(_codes(n, n_ids, rng), None, n_ids, dtype)
    _check(_codes(T + 77, n_ids, rng), rng.permutation(T + 77), n_ids, np.int64)


def test_the_launch_chooses_a_form_by_the_sizes(monkeypatch):
    monkeypatch.delenv("VNM_DICT_COMPACT_LDS", raising=False)
    rng = np.random.default_rng(17)
    _check(_codes(40 * T + 1, 300, rng), None, 300, np.int16)       # rows per workgroup >= 4 x ids: LDS
    _check(_codes(T, 8000, rng), None, 8000, np.int16)              # not: L2


@pytest.mark.parametrize("rows_kind", ["identity", "permutation", "prefix"])
@pytest.mark.parametrize("dtype", INDEX_TYPES)
def test_index_types(dtype, rows_kind):
    rng = np.random.default_rng(len(dtype) + len(rows_kind))
    for n in (5, 3 * T + 5):
        _check(_codes(n, 100, rng), _rows(rows_kind, n, rng), 100, np.dtype(dtype))


def test_nulls_only_and_no_ids_at_all():
    got = _check(np.full(T + 9, -1, np.int32), None, 50, np.int8)
    assert got["n_used"] == 0 and got["null_count"] == T + 9 and not got["indices"].any()
    _check(np.full(13, -1, np.int32), None, 0, np.uint32)


def test_unused_ids_in_runs_that_cross_a_scan_tile():
    rng = np.random.default_rng(23)
    n_ids = 3 * T + 100
    pick = np.concatenate([np.arange(0, 10), np.arange(T - 100 - 7, T - 100), np.arange(T + 100, T + 103),     # [T - 100, T + 100) unused
                           np.array([2 * T - 1, 2 * T]), np.array([n_ids - 1])]).astype(np.int32)            # [2T + 1, n_ids - 1) unused
    codes = pick[rng.integers(0, len(pick), 4 * T + 3)]
    codes[:len(pick)] = pick
    codes[rng.random(len(codes)) < 0.05] = -1
    got = _check(codes, None, n_ids, np.int16)
    assert got["n_used"] <= len(pick)
    _check(codes, rng.permutation(len(codes))[:T + 1], n_ids, np.uint64)


@pytest.mark.parametrize("dtype", ["int8", "uint16", "int32", "int64"])
def test_unaligned_output_takes_the_element_stores(dtype):
    rng = np.random.default_rng(9)
    _check(_codes(T + 9, 90, rng), None, 90, np.dtype(dtype), shift_out=1)


@pytest.mark.parametrize("dtype, k, overflows", [("int8", 127, False), ("int8", 128, True), ("uint8", 255, False), ("uint8", 256, True)])
def test_more_used_ids_than_the_index_type_holds(dtype, k, overflows):
    rng = np.random.default_rng(k)
    ids = rng.permutation(3 * k)[:k].astype(np.int32)
    codes = np.concatenate([ids, ids[rng.integers(0, k, T)]])
    if not overflows:
        assert _check(codes, None, 3 * k, np.dtype(dtype))["n_used"] == k
        return
    (rc, err), m, got = _compact(codes, None, 3 * k, np.dtype(dtype))
    assert m["overflow"] and rc != 0 and OVERFLOW in err
    assert got["n_used"] == k


@pytest.mark.parametrize("rows_kind", ["identity", "permutation"])
def test_a_code_past_the_ids_is_counted_and_never_an_address(rows_kind):
    """(the bounds test precedes every table access; the tables are n_ids entries rounded up to a tile, so under the guard leg a load
    or a store behind them would be a violation too)"""
    rng = np.random.default_rng(11)
    n, n_ids = 2 * T + 31, 100
    codes = _codes(n, n_ids, rng)
    where = rng.choice(n, 40, replace=False)
    codes[where] = [(n_ids, n_ids + 1, 2**31 - 1, 5 * T)[i % 4] for i in range(40)]
    (rc, err), m, _ = _compact(codes, _rows(rows_kind, n, rng), n_ids, np.int32)
    assert m["bad"] == 40 and rc != 0 and "code out of bounds (40 row(s)" in err


def test_refusals():
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib = L.lib()
    buf = DeviceBuffer(256)
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    ok = (buf.ptr, None, 4, 4, L.I32, buf.ptr, buf.ptr, ctypes.byref(a), buf.ptr, ctypes.byref(b), None)
    for at in (0, 5, 8, 9):                       # codes, out_indices, out_used_ids, out_n_used
        args = list(ok)
        args[at] = None
        assert lib.vnm_dict_take_compact(*args) != 0 and "null argument" in L.last_error()
    for at, bad in ((2, -1), (3, -1), (4, L.F32), (4, -1)):
        args = list(ok)
        args[at] = bad
        assert lib.vnm_dict_take_compact(*args) != 0


# ---- 2. Sort through raw ctypes -------------------------------------------------------------------------------------------------------
def _raw_sort(table_batches, cols, orders, limit=0) -> pa.RecordBatch:
    """vnm_sort_op_create / _next / _sorted through ctypes and the Arrow C Data Interface only"""
    from vinum_amd import _lib as L
    lib = L.lib()
    names = (ctypes.c_char_p * len(cols))(*[c.encode() for c in cols])
    ords = (ctypes.c_int * len(cols))(*[int(o) for o in orders])
    h = lib.vnm_sort_op_create(len(cols), names, ords)
    assert h, L.last_error()
    try:
        for b in table_batches:
            arr, sch = ctypes.create_string_buffer(80), ctypes.create_string_buffer(72)
            b._export_to_c(ctypes.addressof(arr), ctypes.addressof(sch))
            L.check(lib.vnm_sort_op_next(h, ctypes.addressof(arr), ctypes.addressof(sch)))
        arr, sch = ctypes.create_string_buffer(80), ctypes.create_string_buffer(72)
        L.check(lib.vnm_sort_op_sorted(h, int(limit), ctypes.addressof(arr), ctypes.addressof(sch)))
        return pa.RecordBatch._import_from_c(ctypes.addressof(arr), ctypes.addressof(sch))
    finally:
        lib.vnm_sort_op_destroy(h)


def _route_last():
    from vinum_amd import _lib as L
    buf = ctypes.create_string_buffer(600)
    L.lib().vnm_route_last(buf, len(buf))
    return buf.value.decode()


def _expected(decoded, keys, limit):
    """pc.sort_indices over the table with c decoded (bytes compared as bytes; NULLs last in both directions; stable), then take"""
    by = decoded.set_column(decoded.schema.get_field_index("c"), "c", decoded["c"].cast(pa.large_binary()))
    idx = pc.sort_indices(by, sort_keys=[(c, "descending" if o else "ascending") for c, o in keys])
    want = decoded.take(idx)
    return want.slice(0, limit) if limit else want


def _assert_sorted(got, want, dict_type, what):
    assert got.schema.names == want.schema.names, what
    assert got.num_rows == want.num_rows, what
    for name in want.schema.names:
        g, w = got.column(name), want.column(name).combine_chunks()
        if name != "c":
            assert g.type == w.type and g.equals(w), f"{what}: column {name}"
            continue
        assert g.type == dict_type and g.type.ordered == dict_type.ordered, f"{what}: {g.type} for {dict_type}"
        g.validate(full=True)
        assert g.cast(dict_type.value_type).equals(w), f"{what}: column c"
        values = g.dictionary.to_pylist()
        assert g.dictionary.null_count == 0 and len(set(values)) == len(values), f"{what}: the dictionary of c"
        assert set(g.indices.drop_null().to_pylist()) == set(range(len(values))), f"{what}: an unused value in the dictionary of c"


SORT_TYPES = [(pa.string(), pa.int8()), (pa.large_binary(), pa.int32()), (pa.binary(), pa.uint16())]
SHAPES = {"only_key": ["c"], "after_an_int_key_with_ties": ["g", "c"], "payload_only": ["g", "k"]}
_ids = lambda x: str(x) if isinstance(x, pa.DataType) else None     # noqa: E731
_TABLES = {}


def _table(value_type, index_type, ordered=False):
    key = (str(value_type), str(index_type), ordered)
    if key not in _TABLES:
        _TABLES[key] = sort_table(value_type, index_type, ordered=ordered)
    return _TABLES[key]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("value_type, index_type", SORT_TYPES, ids=_ids)
def test_sort_through_the_raw_c_abi(value_type, index_type, shape):
    """On the code before this file the library took c for its indices: an intN column came back, ordered by index."""
    ordered = shape == "after_an_int_key_with_ties"
    batches, decoded = _table(value_type, index_type, ordered)
    dict_type = pa.dictionary(index_type, value_type, ordered)
    assert batches[0].schema.field("c").type == dict_type
    n = decoded.num_rows
    for desc in (0, 1):
        keys = [(c, desc if c == "c" else 0) for c in SHAPES[shape]]
        for limit in (0, 5, n // 3):
            what = f"{shape} desc={desc} limit={limit}"
            got = _raw_sort(batches, [c for c, _ in keys], [o for _, o in keys], limit)
            note = _route_last()
            _assert_sorted(got, _expected(decoded, keys, limit), dict_type, what)
            assert note.startswith("sort:dictionary_key_ranks") and f"rows={n} " in note, note
            assert "dictionaries_skipped=1" in note, note              # the last batch repeats its neighbour's dictionary buffers
            if limit == 5:
                assert len(got.column("c").dictionary) <= 5


@pytest.mark.parametrize("n", [1, 7, 1000, 40_000])
def test_sort_fuzz(n):
    types = [(v, i) for v in (pa.string(), pa.large_string(), pa.binary(), pa.large_binary()) for i in INDEX_TYPES]
    for seed in range(16):
        rng = np.random.default_rng(1000 * n + seed)
        value_type, index_name = types[int(rng.integers(0, len(types)))]
        index_type = pa.from_numpy_dtype(np.dtype(index_name))
        ordered = bool(rng.integers(0, 2))
        batches, decoded = sort_table(value_type, index_type, n=n, seed=seed + n, ordered=ordered)
        keys = [[("c", int(rng.integers(0, 2)))], [("g", int(rng.integers(0, 2))), ("c", int(rng.integers(0, 2)))], [("g", 0), ("k", 1)]][seed % 3]
        limit = [0, 0, 1, n // 2][seed % 4]
        got = _raw_sort(batches, [c for c, _ in keys], [o for _, o in keys], limit)
        _assert_sorted(got, _expected(decoded, keys, limit), pa.dictionary(index_type, value_type, ordered), f"n={n} seed={seed} {keys} limit={limit}")


def test_batches_that_together_hold_more_values_than_int8_names():
    from vinum_amd import _lib as L
    words = [f"w{i:03d}" for i in range(200)]
    batches = [pa.RecordBatch.from_arrays([pa.array(np.arange(100, dtype=np.int64) + 100 * b),
                                           dict_array(np.arange(100), words[100 * b:100 * (b + 1)], pa.int8())], names=["k", "c"]) for b in range(2)]
    with pytest.raises(pa.ArrowInvalid) as e:
        pa.concat_arrays([b.column("c") for b in batches])
    assert OVERFLOW in str(e.value)
    for cols in (["c"], ["k"]):
        with pytest.raises(L.VinumHipError) as e:
            _raw_sort(batches, cols, [0])
        assert OVERFLOW in str(e.value)
    # the first 100 rows alone fit
    got = _raw_sort(batches, ["k"], [0], limit=100)
    assert got.column("c").type == pa.dictionary(pa.int8(), pa.string()) and got.column("c").to_pylist() == words[:100]


def test_a_dictionary_over_other_values_is_refused_not_sorted_as_integers():
    from vinum_amd import _lib as L
    d = pa.DictionaryArray.from_arrays(pa.array([2, 0, 1, 0], pa.int32()), pa.array([30, 10, 20], pa.int64()))
    b = pa.RecordBatch.from_arrays([pa.array([3, 1, 2, 0], pa.int64()), d], names=["k", "d"])
    for cols in (["k"], ["d"]):
        with pytest.raises(L.VinumHipError, match="has a type the GPU path does not handle"):
            _raw_sort([b], cols, [0])


def test_batches_whose_dictionary_types_differ_are_no_table():
    from vinum_amd import _lib as L
    k = pa.array([1, 0], pa.int64())
    a = pa.RecordBatch.from_arrays([k, dict_array([0, 1], ["x", "y"], pa.int8(), pa.string())], names=["k", "c"])
    b = pa.RecordBatch.from_arrays([k, dict_array([0, 1], [b"x", b"y"], pa.int8(), pa.binary())], names=["k", "c"])
    with pytest.raises(L.VinumHipError, match="Failed to create table from record batches"):
        _raw_sort([a, b], ["k"], [0])


# ---- 3. vinum_lib.Sort ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_type, index_type", SORT_TYPES, ids=_ids)
def test_vinum_lib_sort(value_type, index_type):
    from vinum_amd import vinum_lib as V
    batches, decoded = _table(value_type, index_type)
    dict_type = pa.dictionary(index_type, value_type)
    for cols, orders, limit in ((["c"], [1], 0), (["g", "c"], [0, 0], 0), (["c", "k"], [0, 1], 50)):
        op = V.Sort(cols, [V.SortOrder(o) for o in orders])
        for b in batches:
            op.next(b)                                  # (raised "ORDER BY a column of type dictionary<...>" before)
        assert op._carried == []                        # no __vnm_row_id detour: the column crosses the ABI as it is
        got = op.sorted(limit) if limit else op.sorted()
        raw = _raw_sort(batches, cols, orders, limit)
        _assert_sorted(got, _expected(decoded, list(zip(cols, orders)), limit), dict_type, f"{cols} {orders} {limit}")
        assert got.equals(raw)


def test_vinum_lib_sort_hands_a_payload_dictionary_back_as_it_came():
    """a dictionary-typed column that is only payload stays with the wrapper (Arrow `take`: the input's dictionary, not a compacted
    one -- what tests/test_gpu_batch_layout.py holds Sort to); as a key of the same table it goes below the ABI"""
    from vinum_amd import vinum_lib as V
    rng = np.random.default_rng(2)
    c = dict_array(rng.integers(0, 5, 3000), ["p", "q", "r", "s", "t"], pa.int32(), mask=rng.random(3000) < 0.2)
    t = pa.table({"k": pa.array(rng.permutation(3000).astype(np.int64)), "c": c})
    op = V.Sort(["k"], [V.SortOrder(0)])
    for b in t.to_batches(max_chunksize=1000):
        op.next(b)
    assert op._carried == ["c"]
    got = op.sorted(7)
    assert got.column("c").equals(c.take(pc.sort_indices(t["k"])).slice(0, 7))
    op = V.Sort(["c", "k"], [V.SortOrder(1), V.SortOrder(0)])
    for b in t.to_batches(max_chunksize=1000):
        op.next(b)
    assert op._carried == []
    got = op.sorted(7)
    assert got.column("c").type == c.type and got.column("c").to_pylist() == ["t"] * 7 and got.column("c").dictionary.to_pylist() == ["t"]


# ---- 4. aggregates --------------------------------------------------------------------------------------------------------------------
def _raw_aggregate(kind, groupby, agg_cols, funcs, batches) -> pa.RecordBatch:
    """vnm_agg_op_create / _next / _result through ctypes and the Arrow C Data Interface only"""
    from vinum_amd import _lib as L
    lib = L.lib()
    cs = lambda xs: (ctypes.c_char_p * max(len(xs), 1))(*[x.encode() for x in xs])      # noqa: E731
    ft = (ctypes.c_int * len(funcs))(*[int(f[0]) for f in funcs])
    h = lib.vnm_agg_op_create(int(kind), len(groupby), cs(groupby), len(agg_cols), cs(agg_cols), len(funcs), ft, cs([f[1] for f in funcs]), cs([f[2] for f in funcs]))
    assert h, L.last_error()
    try:
        for b in batches:
            arr, sch = ctypes.create_string_buffer(80), ctypes.create_string_buffer(72)
            b._export_to_c(ctypes.addressof(arr), ctypes.addressof(sch))
            L.check(lib.vnm_agg_op_next(h, ctypes.addressof(arr), ctypes.addressof(sch)))
        arr, sch = ctypes.create_string_buffer(80), ctypes.create_string_buffer(72)
        L.check(lib.vnm_agg_op_result(h, ctypes.addressof(arr), ctypes.addressof(sch)))
        return pa.RecordBatch._import_from_c(ctypes.addressof(arr), ctypes.addressof(sch))
    finally:
        lib.vnm_agg_op_destroy(h)


def _route_counts():
    from vinum_amd import _lib as L
    lib = L.lib()
    buf = ctypes.create_string_buffer(int(lib.vnm_route_counts(None, 0)) + 16)
    lib.vnm_route_counts(buf, len(buf))
    return {k: int(v) for k, _, v in (line.rpartition("=") for line in buf.value.decode().splitlines())}


def _compact_dictionary(col, what):
    col.validate(full=True)
    values = col.dictionary.to_pylist()
    assert col.dictionary.null_count == 0 and len(set(values)) == len(values), what
    assert set(col.indices.drop_null().to_pylist()) == set(range(len(values))), f"{what}: an unused value in the dictionary"


def _assert_aggregated(got, decoded, dict_type, what):
    """pyarrow group_by over the decoded column: COUNT(*), SUM(v), COUNT(c) per (c, g); MIN(c) = MAX(c) = c inside a group of c"""
    value_type = dict_type.value_type
    want = decoded.group_by(["c", "g"]).aggregate([([], "count_all"), ("v", "sum"), ("c", "count")])
    for name in ("c", "lo", "hi"):
        assert got.schema.field(name).type == dict_type, f"{what}: {name} is {got.schema.field(name).type}"
        _compact_dictionary(got.column(name), f"{what}: {name}")
    keys = list(zip(got.column("c").cast(value_type).to_pylist(), got.column("g").to_pylist()))
    assert len(keys) == len(set(keys)) == want.num_rows, what
    assert dict(zip(keys, zip(got.column("n").to_pylist(), got.column("total").to_pylist(), got.column("nc").to_pylist()))) == \
        dict(zip(zip(want["c"].to_pylist(), want["g"].to_pylist()), zip(want["count_all"].to_pylist(), want["v_sum"].to_pylist(), want["c_count"].to_pylist()))), what
    assert got.column("lo").cast(value_type).to_pylist() == got.column("c").cast(value_type).to_pylist(), what
    assert got.column("hi").cast(value_type).to_pylist() == got.column("c").cast(value_type).to_pylist(), what
    # the NULL groups hold the rows that are NULL by index AND those NULL only by value, and COUNT(c) counts none of them
    null_rows = sum(n for (c, _), n in zip(keys, got.column("n").to_pylist()) if c is None)
    assert null_rows == decoded["c"].null_count > 0, what
    assert all(nc == 0 for (c, _), nc in zip(keys, got.column("nc").to_pylist()) if c is None), what


def _agg_funcs():
    from vinum_amd import _lib as L
    return [(L.COUNT_STAR, "", "n"), (L.SUM, "v", "total"), (L.COUNT, "c", "nc"), (L.MIN, "c", "lo"), (L.MAX, "c", "hi")]


@pytest.mark.parametrize("value_type, index_type", SORT_TYPES, ids=_ids)
def test_aggregate_through_the_raw_c_abi(value_type, index_type):
    """On the code before this file the library grouped by the batch-local indices and handed an intN key back."""
    from vinum_amd import _lib as L
    batches, decoded = _table(value_type, index_type)
    dict_type = pa.dictionary(index_type, value_type)
    assert sum(b.column("c").null_count for b in batches) < decoded["c"].null_count      # rows NULL only by value exist
    before = _route_counts().get("keys:dictionary_child", 0)
    got = _raw_aggregate(L.MULTI_NUMERICAL, ["c", "g"], ["c", "g"], _agg_funcs(), batches)
    assert _route_counts().get("keys:dictionary_child", 0) > before
    _assert_aggregated(got, decoded, dict_type, f"{dict_type}")
    # one group: COUNT, MIN and MAX over the column without any key
    one = _raw_aggregate(L.ONE_GROUP, [], [], _agg_funcs(), batches)
    everything = [x for x in decoded["c"].cast(pa.large_binary()).to_pylist() if x is not None]
    assert one.column("n").to_pylist() == [decoded.num_rows] and one.column("nc").to_pylist() == [len(everything)]
    assert one.column("lo").type == dict_type and one.column("lo").cast(value_type).cast(pa.large_binary()).to_pylist() == [min(everything)]
    assert one.column("hi").cast(value_type).cast(pa.large_binary()).to_pylist() == [max(everything)]
    assert len(one.column("lo").dictionary) == 1


def test_aggregate_keeps_the_ordered_flag():
    from vinum_amd import _lib as L
    batches, decoded = _table(pa.large_string(), pa.int16(), True)
    got = _raw_aggregate(L.MULTI_NUMERICAL, ["c", "g"], ["c", "g"], _agg_funcs(), batches)
    _assert_aggregated(got, decoded, pa.dictionary(pa.int16(), pa.large_string(), True), "ordered")


def test_aggregate_refuses_what_it_cannot_mean():
    from vinum_amd import _lib as L
    batches, _ = _table(pa.string(), pa.int8())
    with pytest.raises(L.VinumHipError, match="not supported by sum"):
        _raw_aggregate(L.SINGLE_NUMERICAL, ["g"], ["g"], [(L.SUM, "c", "s")], batches)        # (summed the indices before)
    d = pa.DictionaryArray.from_arrays(pa.array([2, 0, 1, 0], pa.int32()), pa.array([30, 10, 20], pa.int64()))
    b = pa.RecordBatch.from_arrays([pa.array([3, 1, 2, 0], pa.int64()), d], names=["k", "d"])
    with pytest.raises(L.VinumHipError, match="Unsupported data type for aggregation column"):
        _raw_aggregate(L.SINGLE_NUMERICAL, ["d"], ["d"], [(L.COUNT_STAR, "", "n")], [b])
    with pytest.raises(L.VinumHipError, match="not supported by min"):
        _raw_aggregate(L.SINGLE_NUMERICAL, ["k"], ["k"], [(L.MIN, "d", "lo")], [b])


def test_aggregate_with_more_groups_than_int8_names():
    from vinum_amd import _lib as L
    words = [f"w{i:03d}" for i in range(200)]
    batches = [pa.RecordBatch.from_arrays([dict_array(np.arange(100), words[100 * b:100 * (b + 1)], pa.int8())], names=["c"]) for b in range(2)]
    with pytest.raises(L.VinumHipError) as e:
        _raw_aggregate(L.SINGLE_NUMERICAL, ["c"], ["c"], [(L.COUNT_STAR, "", "n")], batches)
    assert OVERFLOW in str(e.value)


@pytest.mark.parametrize("value_type, index_type", SORT_TYPES, ids=_ids)
def test_vinum_lib_generic_hash_aggregate(value_type, index_type):
    from vinum_amd import vinum_lib as V
    batches, decoded = _table(value_type, index_type)
    op = V.GenericHashAggregate(["c", "g"], ["c", "g"], [V.AggFuncDef(V.COUNT_STAR, "", "n"), V.AggFuncDef(V.SUM, "v", "total"),
                                                       V.AggFuncDef(V.COUNT, "c", "nc"), V.AggFuncDef(V.MIN, "c", "lo"), V.AggFuncDef(V.MAX, "c", "hi")])
    before = _route_counts().get("keys:dictionary_child", 0)
    for b in batches:
        op.next(b)
    got = op.result()
    assert op._dicts == {}                         # no KeyDictionary: the column crosses the ABI as it is
    assert _route_counts().get("keys:dictionary_child", 0) > before
    _assert_aggregated(got, decoded, pa.dictionary(index_type, value_type), "GenericHashAggregate")


def test_vinum_lib_aggregates_with_a_stand_in_beside_the_dictionary_typed_column():
    """COUNT over the plain string column s makes the numeric classes build an int8 stand-in per batch; the waiting batches, whose
    dictionaries differ and hold a NULL (pyarrow cannot join those), must still reach the library"""
    from vinum_amd import vinum_lib as V
    batches, decoded = _table(pa.string(), pa.int8())
    dict_type = pa.dictionary(pa.int8(), pa.string())
    want = decoded.group_by("c").aggregate([([], "count_all"), ("s", "count")])
    op = V.GenericHashAggregate(["c"], ["c"], [V.AggFuncDef(V.COUNT_STAR, "", "n"), V.AggFuncDef(V.COUNT, "s", "ns")])
    for b in batches:
        op.next(b)
    got = op.result()
    assert op._dicts == {} and got.column("c").type == dict_type
    assert dict(zip(got.column("c").cast(pa.string()).to_pylist(), zip(got.column("n").to_pylist(), got.column("ns").to_pylist()))) == \
        dict(zip(want["c"].to_pylist(), zip(want["count_all"].to_pylist(), want["s_count"].to_pylist())))
    # the dictionary-typed column under COUNT, MIN and MAX of a numeric class keyed by an int column, s counted beside it
    op = V.SingleNumericalHashAggregate(["g"], ["g"], [V.AggFuncDef(V.COUNT, "c", "nc"), V.AggFuncDef(V.COUNT, "s", "ns"), V.AggFuncDef(V.MAX, "c", "hi")])
    for b in batches:
        op.next(b)
    got = op.result()
    want = decoded.group_by("g").aggregate([("c", "count"), ("s", "count"), ("c", "max")])
    assert got.column("hi").type == dict_type
    assert dict(zip(got.column("g").to_pylist(), zip(got.column("nc").to_pylist(), got.column("ns").to_pylist(), got.column("hi").cast(pa.string()).to_pylist()))) == \
        dict(zip(want["g"].to_pylist(), zip(want["c_count"].to_pylist(), want["s_count"].to_pylist(), want["c_max"].to_pylist())))


# ---- 5. guard mode ------------------------------------------------------------------------------------------------------------------
def test_under_the_pool_guard(monkeypatch):
    """a selection of the above with every allocation red-zoned and poisoned (as tests/test_gpu_dictcol.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        for n in (1, 9, T - 1, 3 * T + 5):
            test_row_counts(n)
        test_id_counts_and_both_table_forms(257, "0", monkeypatch)
        test_id_counts_and_both_table_forms(LDS_IDS, "1", monkeypatch)
        test_id_counts_and_both_table_forms(70_000, "1", monkeypatch)
        monkeypatch.delenv("VNM_DICT_COMPACT_LDS", raising=False)
        test_index_types("int8", "prefix")
        test_index_types("uint64", "permutation")
        test_nulls_only_and_no_ids_at_all()
        test_unused_ids_in_runs_that_cross_a_scan_tile()
        test_unaligned_output_takes_the_element_stores("int64")
        test_a_code_past_the_ids_is_counted_and_never_an_address("permutation")
        test_sort_through_the_raw_c_abi(pa.string(), pa.int8(), "only_key")
        test_sort_through_the_raw_c_abi(pa.binary(), pa.uint16(), "payload_only")
        test_sort_fuzz(7)
        test_aggregate_through_the_raw_c_abi(pa.string(), pa.int8())
        test_aggregate_with_more_groups_than_int8_names()
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


# ---- 6. one reader of dictionary-typed columns under both operators; one batch routine under both batch paths ---------------------
_BOTH_OPERATORS = """
import json
import pyarrow as pa
from vinum_amd import _lib as L
from tests.dictsort_util import sort_table
from tests.test_gpu_dictsort import _raw_aggregate, _raw_sort
batches, _ = sort_table(pa.string(), pa.int8())
s = _raw_sort(batches, ["c"], [0])
a = _raw_aggregate(L.SINGLE_NUMERICAL, ["c"], ["c"], [(L.COUNT_STAR, "", "n")], batches)
print(json.dumps({"rows": sum(b.num_rows for b in batches), "sorted": s.column("c").cast(pa.string()).to_pylist(),
                  "keys": a.column("c").cast(pa.string()).to_pylist(), "n": a.column("n").to_pylist()}))
"""


def test_both_operators_read_a_dictionary_column_the_same_way():
    """The four batches of sort_table (misaligned lengths, a sliced first batch, a NULL value in every dictionary, the last batch
    repeating its neighbour's dictionary buffers) once through vnm_sort_op_* and once through vnm_agg_op_* as the key of COUNT(*).
    The aggregate's note is followed by the device operator's, so both notes are read from the trace of a fresh process
    (VNM_AGG_TRACE is read once per process)."""
    import json
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _BOTH_OPERATORS], cwd=root, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "VNM_AGG_TRACE": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    fields = lambda name: [dict(kv.split("=") for kv in line.split(": ", 1)[1].split())      # noqa: E731
                           for line in p.stderr.splitlines() if re.match(r"\[route\] " + re.escape(name) + ":", line)]
    sort_notes, agg_notes = fields("sort:dictionary_key_ranks"), fields("keys:dictionary_child")
    assert len(sort_notes) == 1, p.stderr[-2000:]
    assert len(agg_notes) == 1, p.stderr[-2000:]                      # four batches below the coalescing threshold: one flush
    for f in ("rows", "values_encoded", "dictionaries_skipped"):
        assert sort_notes[0][f] == agg_notes[0][f], (f, sort_notes, agg_notes)
    assert agg_notes[0]["dictionaries_skipped"] == "1" and int(agg_notes[0]["rows"]) == out["rows"]
    assert int(agg_notes[0]["values_encoded"]) > 0
    assert len(out["keys"]) == len(set(out["keys"])) and None in out["keys"]
    assert set(out["keys"]) == set(out["sorted"])
    assert sum(out["n"]) == out["rows"] == len(out["sorted"])


def test_a_large_batch_and_the_same_rows_in_small_batches_agree():
    """2^20 + 3 rows, just over the coalescing threshold's default: as one batch they are staged straight from their own buffers
    (vnm_agg_op_next's direct path), cut into 7 uneven batches they wait and go as one flush.  Same groups, bit for bit."""
    from vinum_amd import _lib as L
    n, off = (1 << 20) + 3, 5
    rng = np.random.default_rng(77)
    m = n + off
    k = pa.array(rng.integers(-40, 40, m).astype(np.int64), mask=rng.random(m) < 0.03)
    words = np.array([f"w{i:02d}é" for i in range(23)] + [""], dtype=object)
    s = pa.array(words[rng.integers(0, len(words), m)], pa.string(), mask=rng.random(m) < 0.04)
    v = pa.array(rng.standard_normal(m) * 1e3, mask=rng.random(m) < 0.05)
    whole = pa.RecordBatch.from_arrays([k, s, v], names=["k", "s", "v"]).slice(off, n)
    assert whole.num_rows == n and whole.column("v").offset == off
    cuts = [0, 1, 100_003, 100_003, 377_777, 900_001, n - 7, n]         # (7 batches, one of them empty, all below 2^20 rows)
    small = [whole.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
    funcs = [(L.SUM, "v", "sum"), (L.COUNT, "v", "count"), (L.MIN, "v", "min"), (L.MAX, "v", "max")]
    got = [_raw_aggregate(L.MULTI_NUMERICAL, ["k", "s"], ["k", "s"], funcs, bs) for bs in ([whole], small)]
    assert got[0].schema == got[1].schema

    def rows(r):
        keys = list(zip(r.column("k").to_pylist(), r.column("s").to_pylist()))
        cols = [np.asarray(r.column(c).to_numpy(zero_copy_only=False)).view(np.uint64 if c != "count" else np.int64).tolist() for c in ("sum", "min", "max", "count")]
        assert all(r.column(c).null_count == 0 for c in ("sum", "min", "max", "count"))
        return sorted(zip(keys, *cols), key=lambda x: (x[0][0] is None, x[0][0] or 0, x[0][1] is None, x[0][1] or ""))

    a, b = rows(got[0]), rows(got[1])
    assert len(a) == len({x[0] for x in a}) > 81 * 20 and any(x[0][0] is None for x in a) and any(x[0][1] is None for x in a)
    assert a == b
