"""to_str() on integer, date32 and timestamp columns through the device value table: vnm_strval_to_str through raw ctypes against
NumPy's own text (np.array(values, dtype='str'), what StringCastFunction computes, vinum/core/functions.py:189-193) for every
integer type, date32 and the four timestamp units, over the row counts round the 1024-row tile and the Arrow offsets that take the
vector and the scalar load path; the side slots (the all-ones value, NULL), growth, colliding values, a second batch, a dst that
already holds some of the texts, the refusals; a selection under the pool's guard mode; ValueTable over a stream of batches through
the planner; every golden case (tests/golden/to_str_cases.py) through the planner and through the adapter; and the queries with
NULLs restated against NumPy / pyarrow (a NULL row is "None": DESIGN.md 4.9g).

On the parent commit the ctypes tests find no symbol and every end-to-end case raises: the planner knows no function "to_str"."""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

TILE = 1024            # rows per workgroup and step of the find pass (SP_TILE, csrc/vnm_strconcat.inc), 4 rows per lane
INT, UINT, DATE32, TS_S, TS_MS, TS_US, TS_NS = range(7)                   # enum vnm_tostr_kind
I64_MIN, I64_MAX = -2**63, 2**63 - 1

# name -> (kind, NumPy storage dtype, how NumPy sees the storage)
TYPES = {
    "int8": (INT, np.int8, None), "int16": (INT, np.int16, None), "int32": (INT, np.int32, None), "int64": (INT, np.int64, None),
    "uint8": (UINT, np.uint8, None), "uint16": (UINT, np.uint16, None), "uint32": (UINT, np.uint32, None), "uint64": (UINT, np.uint64, None),
    "date32": (DATE32, np.int32, "datetime64[D]"),
    "timestamp[s]": (TS_S, np.int64, "datetime64[s]"), "timestamp[ms]": (TS_MS, np.int64, "datetime64[ms]"),
    "timestamp[us]": (TS_US, np.int64, "datetime64[us]"), "timestamp[ns]": (TS_NS, np.int64, "datetime64[ns]"),
}


def numpy_text(values: np.ndarray, view):
    """NumPy's text of the stored values, as bytes"""
    a = values if view is None else values.astype(np.int64).view(view)
    return [str(s).encode() for s in np.array(a, dtype="str")]


def _vnm_type(dtype):
    from vinum_amd import _lib as L
    return {np.int8: L.I8, np.int16: L.I16, np.int32: L.I32, np.int64: L.I64, np.uint8: L.U8, np.uint16: L.U16, np.uint32: L.U32, np.uint64: L.U64,
            np.float64: L.F64}[dtype]


def _fetch_new(h):
    """(ids, values) the last call added to the dictionary `h`"""
    from vinum_amd import _lib as L
    lib = L.lib()
    n, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(lib.vnm_strdict_last_new(h, ctypes.byref(n), ctypes.byref(nbytes)))
    ids, lens, data = np.empty(max(n.value, 1), np.int32), np.empty(max(n.value, 1), np.int32), np.empty(max(nbytes.value, 1), np.uint8)
    L.check(lib.vnm_strdict_fetch_new(h, ids.ctypes.data, lens.ctypes.data, data.ctypes.data))
    offs = np.concatenate([[0], np.cumsum(lens[:n.value])])
    raw = data.tobytes()
    return ids[:n.value], [raw[offs[i]:offs[i + 1]] for i in range(n.value)]


class _Values:
    """a value table and its derived dictionary through raw ctypes, with the host copy of what the calls added"""

    def __init__(self, type_name, kind=None):
        from vinum_amd import _lib as L
        self.lib = L.lib()
        self.kind, self.dtype, self.view = TYPES[type_name]
        self.h = self.lib.vnm_strval_create(self.kind if kind is None else kind)
        assert self.h, L.last_error()
        self.dst = self.lib.vnm_strdict_create()
        self.derived, self.code_of_value, self.calls = {}, {}, 0

    def close(self):
        self.lib.vnm_strval_destroy(self.h)
        self.lib.vnm_strdict_destroy(self.dst)

    def stats(self):
        from vinum_amd import _lib as L
        out = (ctypes.c_int64 * 6)()
        L.check(self.lib.vnm_strval_stats(self.h, out, None))
        return dict(zip(("launches", "values_formatted", "rehashes", "slots", "occupied", "half_written"), [int(v) for v in out]))

    def run(self, values, valid=None, offset=0, dtype=None, check=True):
        """stored values and optional validity (False = NULL) behind `offset` rows -> the rows' dst codes, held against NumPy's text"""
        from vinum_amd import _lib as L
        from vinum_amd.device import DeviceBuffer
        lib, dtype = self.lib, dtype or self.dtype
        values = np.asarray(values, dtype)
        n = len(values)
        d = L.DCol()
        vals = DeviceBuffer.from_host(np.concatenate([np.full(offset, 77, dtype), values]))
        bits = DeviceBuffer.from_host(np.packbits(np.concatenate([np.ones(offset, bool), valid]), bitorder="little")) if valid is not None else None
        d.values, d.validity, d.offset, d.length, d.type, d.flags = vals.ptr, bits.ptr if bits is not None else None, offset, n, _vnm_type(dtype), 0
        out = DeviceBuffer((n + 16) * 4)
        L.check(lib.vnm_memset(out.ptr, 0x5A, out.nbytes))
        rc = lib.vnm_strval_to_str(self.h, self.dst, ctypes.byref(d), n, out.ptr + 32, None)
        err = L.last_error() if rc else ""
        L.check(lib.vnm_device_synchronize())
        if not check:
            return rc, err
        assert rc == 0, err
        self.calls += 1 if n else 0
        raw = out.to_host(np.int32, n + 16)
        assert (raw[:8] == 0x5A5A5A5A).all() and (raw[8 + n:] == 0x5A5A5A5A).all()
        got = raw[8:8 + n]
        if n:
            ids, self.last_new = _fetch_new(self.dst)                                      # (a fetch hands the values over once)
            assert not (set(ids.tolist()) & set(self.derived))
            self.derived.update(zip(ids.tolist(), self.last_new))
        want = numpy_text(values, self.view)
        for i in range(n):
            null = valid is not None and not valid[i]
            assert self.derived[int(got[i])] == (b"None" if null else want[i]), (i, values[i], null)
            key = None if null else int(values[i])
            assert self.code_of_value.setdefault(key, int(got[i])) == int(got[i])          # a value keeps its code for good
        st = self.stats()
        assert st["values_formatted"] == len(self.code_of_value) == st["occupied"]         # one image per distinct value, never per row
        assert st["half_written"] == 0 and st["launches"] == self.calls                    # no slot is left without a code
        assert len(set(self.derived.values())) == len(self.derived)
        return got


def _edge_values(type_name, n, rng):
    """n stored values of the type: its minimum, its maximum and the all-ones bit pattern first, then small and random ones"""
    _, dtype, _ = TYPES[type_name]
    info = np.iinfo(dtype)
    ones = np.array([-1 if info.min < 0 else info.max]).astype(dtype)[0]
    head = np.array([info.min, info.max, ones, 0, 1, 9, 10, 99, 100], dtype=dtype)
    if type_name == "date32":
        head = np.concatenate([head, np.array([-719528, -719529, 2932896, 2932897, 11016, 11017], dtype)])
    if type_name.startswith("timestamp"):
        head = np.concatenate([head, np.array([I64_MIN + 1, I64_MAX - 1, -1, 951782399, -86400000000001, 1700000000123456789], dtype)])
    small = rng.integers(-50 if info.min < 0 else 0, 50, n).astype(dtype)                   # repeats: most rows are known values
    wide = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    body = np.where(rng.random(n) < 0.7, small, wide).astype(dtype)
    return np.concatenate([head, body])[:n] if n else body[:0]


# ---- 1. the entry point through raw ctypes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", list(TYPES))
def test_every_type_row_count_and_offset_against_numpy(type_name):
    """one table per type over every (row count, Arrow offset): offsets 0 and 8 keep row 0 aligned for one access per lane, 1, 7 and
    13 do not (the scalar path) and move the validity bit offset; every nullable call holds NULL rows"""
    v = _Values(type_name)
    try:
        rng = np.random.default_rng(len(type_name))
        for n in (0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 4 * TILE + 3):
            for offset in (0, 1, 7, 8, 13):
                values = _edge_values(type_name, n, rng)
                rng.shuffle(values)
                valid = None if (offset == 8 and n) else rng.random(n) > 0.15
                if valid is not None and n:
                    valid[rng.integers(0, n)] = False
                got = v.run(values, valid, offset)
                assert got.dtype == np.int32 and (got >= 0).all()                          # codes, no validity: never NULL
        if type_name in ("int64", "uint64") or type_name.startswith("timestamp"):
            assert None in v.code_of_value and (-1 if v.kind != UINT else 2**64 - 1) in v.code_of_value     # both side slots were used
    finally:
        v.close()


@pytest.mark.parametrize("type_name,value", [("int64", 12345), ("int64", -1), ("uint64", 2**64 - 1), ("int8", -1), ("timestamp[ns]", -1), ("date32", 7)])
def test_every_row_the_same_value_is_formatted_once(type_name, value):
    v = _Values(type_name)
    try:
        got = v.run(np.full(2 * TILE + 1, value, dtype=v.dtype))
        assert len(set(got.tolist())) == 1 and v.stats()["values_formatted"] == 1
        got = v.run(np.full(5, value, dtype=v.dtype), offset=3)
        assert v.stats()["values_formatted"] == 1 and v.stats()["launches"] == 2
    finally:
        v.close()


def test_every_row_null_is_one_none():
    v = _Values("int32")
    try:
        got = v.run(np.arange(TILE + 7, dtype=np.int32), np.zeros(TILE + 7, bool), offset=1)
        assert len(set(got.tolist())) == 1 and v.derived[int(got[0])] == b"None" and v.stats()["values_formatted"] == 1
    finally:
        v.close()


def test_growth_keeps_the_codes_and_both_side_slots(monkeypatch):
    monkeypatch.setenv("VNM_STRPAIR_SLOTS", "16")
    v = _Values("int64")
    try:
        first_values = np.array([5, -1, 0, I64_MIN, 6], np.int64)
        first = v.run(first_values, np.array([True, True, False, True, True]))         # 3 values in 16 slots, -1 and NULL beside them
        assert v.stats()["rehashes"] == 0 and v.stats()["slots"] == 16 and v.stats()["values_formatted"] == 5
        values = np.concatenate([np.array([-1, 5, I64_MIN, 6], np.int64), np.arange(1000, 1296, dtype=np.int64) * 1_000_003])      # 300 distinct with NULL
        values = np.concatenate([values, [0]])
        valid = np.ones(len(values), bool)
        valid[-1] = False
        order = np.random.default_rng(4).permutation(len(values))
        allc = v.run(values[order], valid[order])
        st = v.stats()
        assert st["rehashes"] > 0 and st["slots"] >= 512 and st["values_formatted"] == 301 and st["half_written"] == 0
        back = np.empty(len(values), np.int32)
        back[order] = allc
        assert back[0] == first[1] and back[1] == first[0] and back[2] == first[3] and back[3] == first[4] and back[-1] == first[2]
        rehashes = st["rehashes"]
        again = v.run(values, valid, offset=1)                                        # known values only: no growth, nothing formatted
        assert np.array_equal(again, back) and v.stats()["rehashes"] == rehashes and v.stats()["values_formatted"] == 301
    finally:
        v.close()


def _home(key, mask):
    """sp_home of csrc/vnm_strconcat.inc"""
    m = 2**64 - 1
    h = (key * 0x9E3779B97F4A7C15) & m
    h ^= h >> 32
    h = (h * 0xff51afd7ed558ccd) & m
    h ^= h >> 29
    return h & mask


def test_two_values_with_one_home_slot_take_two_slots_and_two_codes(monkeypatch):
    monkeypatch.setenv("VNM_STRPAIR_SLOTS", "1024")
    seen = {}
    for x in range(1, 100000):
        h = _home(x, 1023)
        if h in seen:
            a, b = seen[h], x
            break
        seen[h] = x
    v = _Values("int64")
    try:
        got = v.run(np.array([a, b, a, b, b], np.int64))
        assert got[0] != got[1] and got[0] == got[2] and got[1] == got[3] == got[4]
        st = v.stats()
        assert st["occupied"] == 2 and st["values_formatted"] == 2 and st["slots"] == 1024 and st["rehashes"] == 0
    finally:
        v.close()


def test_a_second_batch_formats_only_the_new_values():
    v = _Values("timestamp[us]")
    try:
        rng = np.random.default_rng(8)
        old = np.unique(rng.integers(-10**15, 10**15, 200))
        valid = np.concatenate([np.ones(len(old), bool), rng.random(2800) > 0.1])
        v.run(np.concatenate([old, old[rng.integers(0, len(old), 2800)]]), valid, offset=7)
        before = v.stats()["values_formatted"]
        assert before == len(old) + 1                                                 # every old value, and None
        new = np.unique(rng.integers(10**16, 10**17, 50))
        both = np.concatenate([old, new, [-1]])
        v.run(both[rng.permutation(len(both))])                                       # (run() holds every old value to its first code)
        assert v.stats()["values_formatted"] - before == len(new) + 1
        assert sorted(v.last_new) == sorted(                                          # the call's new texts: the new values' and -1's
            numpy_text(np.concatenate([new, [-1]]), v.view))
    finally:
        v.close()


def test_a_dst_that_already_holds_some_of_the_texts():
    from vinum_amd import _lib as L
    v = _Values("int64")
    try:
        have = pa.array([b"7", b"None", b"-1", b"unrelated"], pa.binary())
        _, obuf, dbuf = have.buffers()
        codes = np.empty(4, np.int32)
        L.check(v.lib.vnm_strdict_encode(v.dst, obuf.address, 0, dbuf.address, None, 0, 4, codes.ctypes.data, None, None, None))
        v.derived.update(zip(codes.tolist(), [b"7", b"None", b"-1", b"unrelated"]))
        got = v.run(np.array([7, -1, 0, 8, 7], np.int64), np.array([True, True, False, True, True]))
        assert got[0] == codes[0] == got[4] and got[1] == codes[2] and got[2] == codes[1] and got[3] not in codes.tolist()
        assert v.last_new == [b"8"]                                                      # the only text the call added
    finally:
        v.close()


def test_refusals():
    from vinum_amd import _lib as L
    lib = L.lib()
    assert not lib.vnm_strval_create(7) and "vnm_tostr_kind" in L.last_error()
    assert not lib.vnm_strval_create(-1)
    for type_name, dtype, what in (("date32", np.int64, "a date kind over an int64 column"), ("int64", np.float64, "a float column"),
                                   ("int64", np.uint64, "an unsigned column under the signed kind"), ("uint8", np.int8, "a signed column under the unsigned kind"),
                                   ("timestamp[s]", np.int32, "a timestamp kind over an int32 column")):
        v = _Values(type_name)
        try:
            rc, err = v.run(np.zeros(4), dtype=dtype, check=False)
            assert rc != 0 and "does not fit kind" in err, what
            assert v.stats()["launches"] == 0
        finally:
            v.close()
    v = _Values("int64")
    try:
        v.run(np.arange(5))
        rc, err = v.run(np.arange(5), dtype=np.int32, check=False)                    # the keys are the first call's type
        assert rc != 0 and "was built over" in err
        d = L.DCol()
        assert lib.vnm_strval_to_str(None, v.dst, ctypes.byref(d), 0, None, None) != 0 and "null argument" in L.last_error()
        assert lib.vnm_strval_to_str(v.h, None, ctypes.byref(d), 0, None, None) != 0
        assert lib.vnm_strval_to_str(v.h, v.dst, None, 0, None, None) != 0
        assert lib.vnm_strval_stats(None, None, None) != 0
        v.run(np.arange(7))                                                          # the table is none the worse for it
    finally:
        v.close()


def _route_count(name):
    from vinum_amd import _lib as L
    buf = ctypes.create_string_buffer(int(L.lib().vnm_route_counts(None, 0)) + 16)
    L.lib().vnm_route_counts(buf, len(buf))
    return {k: int(n) for k, _, n in (line.rpartition("=") for line in buf.value.decode().splitlines())}.get(name, 0)


def test_every_call_leaves_its_route_note():
    from vinum_amd import _lib as L
    before = _route_count("to_str:value_table")
    v = _Values("uint16")
    try:
        v.run(np.arange(10))
        v.run(np.arange(10), offset=1)
    finally:
        v.close()
    assert _route_count("to_str:value_table") == before + 2
    buf = ctypes.create_string_buffer(600)
    L.lib().vnm_route_last(buf, len(buf))
    assert buf.value.decode().startswith("to_str:value_table: 10 rows") and "scalar loads" in buf.value.decode()


# ---- 2. under the pool's guard mode -----------------------------------------------------------------------------------------------------
def test_under_the_pool_guard(monkeypatch):
    """a selection with every allocation red-zoned and poisoned (as tests/test_gpu_concat.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        for type_name in ("int8", "uint16", "int64", "date32", "timestamp[ns]"):
            test_every_type_row_count_and_offset_against_numpy(type_name)
        test_every_row_the_same_value_is_formatted_once("uint64", 2**64 - 1)
        test_every_row_null_is_one_none()
        test_growth_keeps_the_codes_and_both_side_slots(monkeypatch)
        test_a_second_batch_formats_only_the_new_values()
        test_a_dst_that_already_holds_some_of_the_texts()
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


# ---- 3. ValueTable over a stream of batches through the planner ---------------------------------------------------------------------------
_main = {}


def _main_table():
    from tests import util
    if "t" not in _main:
        _main["t"] = util.read_ipc("to_str_in_main.arrow")
    return _main["t"]


def _execute(query, t, batch=300):
    from vinum_amd import planner, set_batch_size
    set_batch_size(batch)
    try:
        return planner.execute(query, t)
    finally:
        set_batch_size(1 << 24)


def _query(select, where=None, group_by=(), aliases=None, order_by=(), sort_order=None, distinct=False):
    from tests.golden import to_str_cases as C
    return C._case("q", select, where, group_by, aliases, order_by, sort_order, distinct)


def _s(x):
    return ["fn", "to_str", x]


def test_a_stream_of_batches_formats_each_value_once():
    """the scan's per-name registry holds ONE table for the column: four batches, every distinct value formatted once over all of them"""
    from vinum_amd import planner, set_batch_size
    from vinum_amd.keydict import ValueTable
    t = _main_table()
    set_batch_size(300)
    try:
        plan = planner.plan_query(_query(["k", _s("v"), ["concat", "city", ["lit", "/"], _s("day")]], aliases=[None, "s", "c"]), t)
        got = plan.execute()
    finally:
        set_batch_size(1 << 24)
    from tests.golden import to_str_cases as C
    assert got["s"].to_pylist() == C.text_of(t["v"])
    op = plan.root
    while getattr(op, "_dicts", None) is None:
        op = op._parent_operator
    tables = {name: list(op._dicts[("to_str", name)].values()) for name in ("v", "day")}
    assert all(len(x) == 1 and isinstance(x[0], ValueTable) for x in tables.values())
    for name, (table,) in tables.items():
        st = table.stats()
        assert st["launches"] == 4 and st["values_formatted"] == len(set(t[name].to_pylist())) and st["half_written"] == 0
    assert ("to_str", "k") in op._dicts and not op._dicts[("to_str", "k")]          # a column nobody prints has no table


def test_a_column_built_by_hand_gets_a_table_for_the_call():
    from tests.golden import to_str_cases as C
    from vinum_amd.core.lowering import lower_dictionary
    from vinum_amd.device import DeviceColumn
    arr = pa.array([3, None, -1, 3], pa.int16())
    cols = {"v": DeviceColumn.from_arrow(arr)}
    e, extra = lower_dictionary(("to_str", "v"), cols)
    assert e == "__to_str_v" and extra[e].validity_ptr is None and extra[e].dictionary.type == pa.string()
    assert extra[e].to_arrow().to_pylist() == C.text_of(arr) == ["3", "None", "-1", "3"]


# ---- 4. the golden fixtures through the planner and through the adapter -----------------------------------------------------------------
def _adapter(t, select, names, where=None, batch=300):
    """binding.vectorize trees through GpuFilterOperator / GpuProjectOperator (so binding.lower and the mirror classes run)"""
    from vinum_amd import binding as B
    from vinum_amd import set_batch_size
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    from vinum_amd.planner import _t
    op = TableReaderOperator(t)
    if where is not None:
        op = B.GpuFilterOperator(B.vectorize(_t(where)), op)
    op = B.GpuProjectOperator([B.vectorize(_t(e)) for e in select], op, col_names=names)
    set_batch_size(batch)
    try:
        return next(MaterializeTableOperator(op).next())
    finally:
        set_batch_size(1 << 24)


def _cases():
    from tests.golden import to_str_cases as C
    return C.CASES


def _meta():
    import json
    import os
    from tests import util
    if "meta" not in _main:
        with open(os.path.join(util.GOLDEN, "to_str_cases.json")) as f:
            _main["meta"] = json.load(f)
    return _main["meta"]


def _compare_fixture(got, case):
    """the fixture is the reference's own result; a case it raised on in the build container (to_str_cases.json says which, and
    with what) is held against the restatement over NumPy's text instead"""
    from tests import util
    from tests.golden import to_str_cases as C
    meta = _meta()
    assert (case["name"] in meta["cases"]) != (case["name"] in meta["raised"])
    if case["name"] in meta["raised"]:
        want = C.restate_query(_main_table(), case)
        key = want.column_names[0]
        got, want = got.sort_by(key), want.sort_by(key)
    else:
        want = util.read_ipc(f"to_str_{case['name']}.arrow")
        if not case["order_by"]:
            got, want = got.sort_by("k"), want.sort_by("k")
    assert got.column_names == want.column_names and got.num_rows == want.num_rows
    for name in want.column_names:
        assert got.schema.field(name).type == want.schema.field(name).type, (case["name"], name)
        assert got[name].null_count == 0 and got[name].to_pylist() == want[name].to_pylist(), (case["name"], name)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    _compare_fixture(_execute(case, _main_table()), case)


@pytest.mark.parametrize("case", [c for c in _cases() if not (c["order_by"] or c["group_by"] or c["distinct"])], ids=lambda c: c["name"])
def test_reference_fixtures_through_the_adapter(case):
    """(the adapter has no sort or aggregate operator of its own: those fixtures go through the planner alone)"""
    from vinum_amd.planner import _raw, output_names
    names = output_names([_raw(e) for e in case["select"]], case["aliases"])
    _compare_fixture(_adapter(_main_table(), case["select"], names, where=case["where"]), case)


# ---- 5. restated against NumPy / pyarrow with NULLs present ------------------------------------------------------------------------------
def _null_table(n=1500, seed=21):
    """v: few distinct int64 values, -1 among them; day, ts: temporal; a, c: strings; every one with NULL rows"""
    if "nulls" not in _main:
        rng = np.random.default_rng(seed)
        mask = lambda rate=0.1: rng.random(n) < rate
        words = ["7", "10", "9", "None", "x", "-1", ""]
        _main["nulls"] = pa.table({
            "k": pa.array(np.arange(n, dtype=np.int64)),
            "v": pa.array(rng.integers(-2, 25, n).astype(np.int64), mask=mask()),
            "y": pa.array(rng.integers(0, 100, n).astype(np.int64)),
            "day": pa.array(rng.integers(-3, 4, n).astype(np.int32), pa.int32(), mask=mask()).cast(pa.date32()),
            "ts": pa.array(rng.integers(-3, 3, n).astype(np.int64) * 86_400_000_001, pa.int64(), mask=mask()).cast(pa.timestamp("us")),
            "a": pa.array([words[i] for i in rng.integers(0, len(words), n)], pa.string(), mask=mask()),
            "c": pa.array([words[i] for i in rng.integers(0, len(words), n)], pa.string(), mask=mask(0.05)),
        })
    return _main["nulls"]


def test_restated_select_list():
    from tests.golden import to_str_cases as C
    t = _null_table()
    got = _execute(_query(["k", _s("v"), _s("day"), _s("ts"), _s("a"), ["fn", "upper", _s("a")]], aliases=[None, "v", "day", "ts", "a", "ua"]), t)
    assert got["k"].to_pylist() == t["k"].to_pylist()
    for name in ("v", "day", "ts", "a"):
        assert got.schema.field(name).type == pa.string() and got[name].null_count == 0
        assert got[name].to_pylist() == C.text_of(t[name]), name
    assert "None" in got["v"].to_pylist() and "-1" in got["v"].to_pylist() and "1969-12-29" in got["day"].to_pylist()
    assert got["ua"].to_pylist() == [s.upper() for s in C.text_of(t["a"])]


@pytest.mark.parametrize("shape", ["eq", "ne", "lt", "in", "like", "column", "eq_none"])
def test_where_follows_the_string_rules(shape):
    """to_str(v) is an ordinary string column to WHERE: =, !=, < (bytes: '10' < '9'), IN, LIKE, and against a string column (whose
    own NULL rows compare False, `!=` True); a NULL v is the string "None", so it is found by = 'None'"""
    from tests.golden import to_str_cases as C
    t = _null_table()
    text, a = C.text_of(t["v"]), t["a"].to_pylist()
    where, keep = {
        "eq": (["eq", _s("v"), ["lit", "7"]], [s == "7" for s in text]),
        "ne": (["ne", _s("v"), ["lit", "7"]], [s != "7" for s in text]),
        "lt": (["lt", _s("v"), ["lit", "2"]], [s.encode() < b"2" for s in text]),
        "in": (["in", _s("v"), ["7", "-1", "None", "nothing"]], [s in ("7", "-1", "None") for s in text]),
        "like": (["like", _s("v"), ["lit", "1%"]], [s.startswith("1") for s in text]),
        "column": (["eq", _s("v"), "a"], [x is not None and s == x for s, x in zip(text, a)]),
        "eq_none": (["eq", _s("v"), ["lit", "None"]], [s == "None" for s in text]),
    }[shape]
    got = _execute(_query(["k"], where=where), t)
    want = [k for k, m in zip(t["k"].to_pylist(), keep) if m]
    assert 0 < len(want) < t.num_rows and got["k"].to_pylist() == want


def test_restated_group_by_with_sum():
    from tests.golden import to_str_cases as C
    t = _null_table()
    got = _execute(_query([_s("v"), ["fn", "count_star"], ["fn", "sum", "y"]], aliases=["s", "n", "y"], group_by=[_s("v")]), t).sort_by("s")
    w = pa.table({"s": pa.array(C.text_of(t["v"])), "y": t["y"]}).group_by("s").aggregate([([], "count_all"), ("y", "sum")]).sort_by("s")
    assert got["s"].null_count == 0 and "None" in got["s"].to_pylist()
    assert got["s"].to_pylist() == w["s"].to_pylist() and got["n"].to_pylist() == w["count_all"].to_pylist() and got["y"].to_pylist() == w["y_sum"].to_pylist()


def test_restated_order_by_is_byte_order_with_none_among_the_values():
    from tests.golden import to_str_cases as C
    t = _null_table()
    got = _execute(_query(["k"], order_by=[_s("v"), "k"], sort_order=["DESC", "ASC"]), t)
    text = C.text_of(t["v"])
    want = sorted(range(t.num_rows), key=lambda i: ([-b for b in text[i].encode()] + [1], i))       # bytes descending, a prefix after its extensions
    assert got["k"].to_pylist() == want
    firsts = [text[i] for i in want]
    assert firsts[0] == "None" and firsts.index("9") < firsts.index("10")                            # 'N' > '9' > '1'


def test_restated_distinct():
    from tests.golden import to_str_cases as C
    t = _null_table()
    got = _execute(_query([_s("day")], aliases=["d"], distinct=True), t)
    assert sorted(got["d"].to_pylist()) == sorted(set(C.text_of(t["day"]))) and "None" in got["d"].to_pylist()


def test_restated_concat_of_two_to_str():
    from tests.golden import to_str_cases as C
    t = _null_table()
    got = _execute(_query(["k", ["concat", "a", ["lit", "-"], _s("v"), ["lit", "/"], _s("day")]], aliases=[None, "c"]), t)
    a, v, d = C.text_of(t["a"]), C.text_of(t["v"]), C.text_of(t["day"])
    assert got["c"].null_count == 0 and got["c"].to_pylist() == [f"{x}-{y}/{z}" for x, y, z in zip(a, v, d)]


def test_min_of_the_result_goes_the_way_min_of_upper_goes():
    """min / max over a function result is out of scope and to_str() adds nothing to it: whatever the operator
    path does with min(upper(a)) today -- it answers with an int32 column of the derived column's codes, it does not refuse -- it
    does with min(to_str(a)): the same outcome, error type or result type"""
    t = _null_table()
    outcome = []
    for fn in ("upper", "to_str"):
        try:
            got = _execute(_query([["fn", "min", ["fn", fn, "a"]]], aliases=["m"]), t)
            outcome.append(("result", got.schema.field("m").type, got.num_rows))
        except (TypeError, NotImplementedError, ValueError) as e:
            outcome.append(("refused", type(e), 0))
    assert outcome[0] == outcome[1]


def test_zero_rows_and_errors():
    from tests.golden import to_str_cases as C
    t = _main_table()
    got = _execute(_query(["k", _s("v")], where=["lt", "k", 0], aliases=[None, "s"]), t)
    assert got.num_rows == 0 and got.schema.field("s").type == pa.string()
    with pytest.raises(TypeError, match="'x' is double"):             # the planner knows a table's schema: refused at plan time
        _execute(_query([_s("x")]), t)
    with pytest.raises(TypeError, match="'x' is double"):             # the lowering, when the batch arrives
        _adapter(t, [_s("x")], ["s"])
    with pytest.raises(NotImplementedError, match="no GPU lowering for to_str\\(\\) over"):
        _execute(_query([_s(["mul", "v", 2])]), t)
    with pytest.raises(TypeError, match="'v' is int64"):              # a bare numeric column inside concat stays refused
        _execute(_query([["concat", "city", "v"]]), t)
