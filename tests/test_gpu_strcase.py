"""upper() / lower() on string columns through the device dictionary: vnm_strdict_map_codepoints through raw ctypes against
pc.utf8_upper / pc.utf8_lower of the same values (every length around the 8-byte step, every mapped code point, growing and
shrinking images, 4-byte sequences, NULs, sequences straddling an 8-byte boundary, colliding images, incremental calls, refused
maps); the structurally malformed values Arrow refuses; both under the pool's guard mode; KeyDictionary.mapped over a stream of
batches; the queries end to end through the planner and through the adapter against pyarrow.compute over the mapped column."""
import ctypes
import random

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

pytestmark = pytest.mark.gpu

KERNEL = {"upper": pc.utf8_upper, "lower": pc.utf8_lower}
# what Arrow raises "Invalid UTF8 sequence in input" for: a stray continuation byte, a lead byte without all its continuation bytes,
# the bytes 0xF8 .. 0xFF
MALFORMED = [b"\x80", b"a\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc3(", b"\xe2(\xa1", b"\xf8", b"\xf9", b"\xfa", b"\xfb", b"\xfc",
             b"\xfd", b"\xfe", b"\xff"]


# ---- 1. the entry point through raw ctypes ------------------------------------------------------------------------------------------
def _encode(h, values):
    """a list of bytes values into the dictionary `h` (vnm_strdict_encode over a binary array's buffers): their codes"""
    from vinum_amd import _lib as L
    arr = pa.array(values, pa.binary())
    _, obuf, dbuf = arr.buffers()
    codes = np.empty(max(len(arr), 1), np.int32)
    L.check(L.lib().vnm_strdict_encode(h, obuf.address, 0, dbuf.address if dbuf is not None and dbuf.size else None, None, 0, len(arr),
                                       codes.ctypes.data, None, None, None))
    return codes[:len(arr)]


def _fetch_new(h):
    """(ids, values) the last call added to `h`"""
    from vinum_amd import _lib as L
    lib = L.lib()
    n, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(lib.vnm_strdict_last_new(h, ctypes.byref(n), ctypes.byref(nbytes)))
    ids, lens, data = np.empty(max(n.value, 1), np.int32), np.empty(max(n.value, 1), np.int32), np.empty(max(nbytes.value, 1), np.uint8)
    L.check(lib.vnm_strdict_fetch_new(h, ids.ctypes.data, lens.ctypes.data, data.ctypes.data))
    offs = np.concatenate([[0], np.cumsum(lens[:n.value])])
    raw = data.tobytes()
    return ids[:n.value], [raw[offs[i]:offs[i + 1]] for i in range(n.value)]


class _Pair:
    """a source and a derived dictionary handle, the table between them and the host copy of the derived values"""

    def __init__(self, fn):
        from vinum_amd import _lib as L
        from vinum_amd import strcase
        self.fn, self.lib = fn, L.lib()
        self.src, self.dst = self.lib.vnm_strdict_create(), self.lib.vnm_strdict_create()
        self.map_from, self.map_to = strcase.case_table(fn)
        self.value_of_code = {}       # src code -> bytes
        self.derived = {}             # dst code -> bytes
        self.table = np.zeros(0, np.int32)

    def close(self):
        self.lib.vnm_strdict_destroy(self.src)
        self.lib.vnm_strdict_destroy(self.dst)

    def add(self, values):
        codes = _encode(self.src, values)
        for c, v in zip(codes.tolist(), values):
            assert self.value_of_code.setdefault(c, v) == v
        return codes

    def map(self, id_begin=0, with_invalid=True, map_from=None, map_to=None):
        """-> (rc, error text, invalid count); self.table holds the whole table afterwards (entries below id_begin as they were)"""
        from vinum_amd import _lib as L
        from vinum_amd.device import DeviceBuffer
        lib = self.lib
        top = int(lib.vnm_strdict_ids(self.src))
        buf = DeviceBuffer((top + 8) * 4)
        L.check(lib.vnm_memset(buf.ptr, 0x5A, buf.nbytes))
        if id_begin:
            L.check(lib.vnm_memcpy_h2d(buf.ptr, self.table.ctypes.data, id_begin * 4))
        mf = self.map_from if map_from is None else np.ascontiguousarray(map_from, np.int32)
        mt = self.map_to if map_to is None else np.ascontiguousarray(map_to, np.int32)
        invalid = ctypes.c_int64(-7)
        rc = lib.vnm_strdict_map_codepoints(self.src, self.dst, mf.ctypes.data, mt.ctypes.data, len(mf), id_begin, buf.ptr,
                                            ctypes.byref(invalid) if with_invalid else None, None)
        err = L.last_error() if rc else ""
        L.check(lib.vnm_device_synchronize())
        raw = buf.to_host(np.int32, top + 8)
        assert (raw[top:] == 0x5A5A5A5A).all()                    # nothing past the ids
        if id_begin:
            assert np.array_equal(raw[:id_begin], self.table[:id_begin])      # the part it covered before is untouched
        self.table = raw[:top].copy()
        ids, vals = _fetch_new(self.dst)
        assert len(set(ids.tolist())) == len(ids) and not (set(ids.tolist()) & set(self.derived))
        self.derived.update(zip(ids.tolist(), vals))
        return rc, err, invalid.value

    def check(self, malformed=()):
        """the table, the derived values and the id count against pc.utf8_upper / utf8_lower of the source values"""
        top = len(self.table)
        codes = np.array(sorted(self.value_of_code), np.int64)
        good = [c for c in codes.tolist() if self.value_of_code[c] not in malformed]
        want = KERNEL[self.fn](pa.array([self.value_of_code[c] for c in good], pa.binary()).cast(pa.string())).cast(pa.binary()).to_pylist()
        got = [self.derived.get(int(self.table[c])) for c in good]
        assert got == want
        never = np.ones(top, bool)
        never[codes] = False
        assert (self.table[never] == -2).all()                   # an id never handed out
        assert all(self.table[c] == -2 for c in codes.tolist() if self.value_of_code[c] in malformed)
        # one code per distinct image, and the derived dictionary holds exactly the images
        assert len({int(self.table[c]) for c in good}) == len(set(want))
        assert sorted(self.derived.values()) == sorted(set(want))
        n_ids = int(self.lib.vnm_strdict_ids(self.dst))
        assert all(0 <= c < n_ids for c in self.derived) and n_ids >= len(self.derived)   # (ids come in chunks: holes, never fewer)


def _corpus(fn, seed=0):
    from vinum_amd import strcase
    map_from, _ = strcase.case_table(fn)
    rng = random.Random(seed)
    mapped = [chr(c) for c in map_from.tolist()]
    vals = [""] + ["aBcDeFgHiJkLmNoPq"[:k] for k in range(1, 18)] + ["Zz" * 8 + "q"]
    vals += mapped                                                               # every mapped code point on its own
    pool = mapped + list("abcXYZ 019_") * 40 + ["中", "文", "\U0001F600", "\U0001E922", "\U0001E900"]
    vals += ["".join(rng.choice(pool) for _ in range(rng.randint(1, 20))) for _ in range(3000)]
    vals += ["ȿ" * k for k in range(1, 10)] + ["ß" * k for k in (1, 4, 5, 9)] + ["İ" * k for k in (1, 3, 8)] + ["ı", "ſ", "K", "ıſK" * 3, "Ⱥ", "Ⱦ" * 5]
    vals += ["\U0001E922", "\U0001E900\U0001E943", "\U0001F600", "中文字", "a\U0001F600b"]
    vals += ["a\x00", "\x00", "a\x00b", "AbC\x00\x00"]
    for pad in range(0, 12):                                                     # a sequence across an 8-byte boundary, at every byte
        vals += ["a" * pad + ch + "b" * 9 for ch in ("ß", "中", "\U0001E922", "\U0001F600", "ȿ")]
    return list(dict.fromkeys(v.encode() for v in vals))


@pytest.mark.parametrize("fn", ["upper", "lower"])
def test_every_mapped_code_point_and_the_edge_values(fn):
    p = _Pair(fn)
    try:
        p.add(_corpus(fn))
        assert p.map() == (0, "", 0)
        p.check()
    finally:
        p.close()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2049, 70_000])
def test_value_counts(count):
    fn = "upper" if count % 2 else "lower"
    rng = random.Random(count)
    base = _corpus(fn, seed=count)
    vals = list(dict.fromkeys(base[:count] + [("%s%dÿ" % (rng.choice(["k", "Ǆ", "ß", ""]), i)).encode() for i in range(max(0, count - len(base)))]))[:count]
    assert len(vals) == count
    p = _Pair(fn)
    try:
        p.add(vals)
        assert p.map() == (0, "", 0)
        p.check()
    finally:
        p.close()


def test_colliding_images_share_a_code():
    for fn, groups in (("upper", [["a", "A"], ["ǆ", "ǅ", "Ǆ"], ["ß", "ẞ"]]), ("lower", [["a", "A"], ["ǆ", "ǅ", "Ǆ"], ["K", "k", "K"]])):
        p = _Pair(fn)
        try:
            codes = p.add([v.encode() for g in groups for v in g])
            assert p.map() == (0, "", 0)
            p.check()
            at = 0
            for g in groups:
                assert len({int(p.table[c]) for c in codes[at:at + len(g)]}) == 1, (fn, g)
                at += len(g)
        finally:
            p.close()


def test_a_second_call_extends_the_table():
    p = _Pair("upper")
    try:
        first = [("v%dß" % i).encode() for i in range(3000)]
        p.add(first)
        assert p.map() == (0, "", 0)
        p.check()
        before, covered = dict(p.derived), len(p.table)
        p.add(first[:100] + [("w%dȿ" % i).encode() for i in range(5000)] + ["V7ẞ".encode()])  # old values, new ones, an image dst holds
        assert p.map(id_begin=covered) == (0, "", 0)              # (map() itself asserts the first `covered` entries are untouched)
        p.check()
        assert all(p.derived[c] == v for c, v in before.items()) and len(p.derived) == len(before) + 5000
        # nothing new: no id in range, nothing added, the table as it is
        assert p.map(id_begin=len(p.table)) == (0, "", 0)
        p.check()
    finally:
        p.close()


def test_refused_maps():
    p = _Pair("upper")
    try:
        p.add([b"abc"])
        rc, err, _ = p.map(map_from=[0x62, 0x61], map_to=[0x42, 0x41])
        assert rc != 0 and "strictly ascending" in err
        rc, err, _ = p.map(map_from=[0x61, 0x61], map_to=[0x42, 0x41])
        assert rc != 0 and "strictly ascending" in err
        rc, err, _ = p.map(map_from=[0x61], map_to=[0x4E2D])      # 1 byte -> 3 bytes: outgrows the room of 2 x length
        assert rc != 0 and "twice" in err
        rc, err, _ = p.map(map_from=[0xE9], map_to=[0x110000])
        assert rc != 0 and "code point" in err
        assert int(p.lib.vnm_strdict_ids(p.dst)) == 0             # none of them touched dst
        # a map that leaves ASCII (1 -> 2 bytes: inside the room) takes the code point path for ASCII too
        assert p.map(map_from=[0x61, 0x62], map_to=[0xE9, 0x42]) == (0, "", 0)
        assert p.derived[int(p.table[0])] == "éBc".encode()
        rc, err, _ = p.map()                                      # ... and dst stays with the map it was derived with
        assert rc != 0 and "another map" in err
    finally:
        p.close()


# ---- 2. malformed values ----------------------------------------------------------------------------------------------------------------
def _malformed_case(fn, with_invalid=True):
    for v in MALFORMED:                                           # the list is what Arrow refuses, here and now
        with pytest.raises(pa.ArrowInvalid, match="Invalid UTF8 sequence in input"):
            KERNEL[fn](pa.Array.from_buffers(pa.string(), 1, pa.array([v], pa.binary()).buffers()))     # (a cast would validate first)
    vals = []
    for i, v in enumerate(MALFORMED):                             # each between well-formed neighbours ...
        vals += [("left%dß" % i).encode(), v, ("İright%d" % i).encode(), b"abcdefg" + v, b"12345678" + v + b"z"]
    vals = list(dict.fromkeys(vals))
    bad = {v for v in vals if not _well_formed(v)}                 # (only the classes above occur: Python's strict decoder agrees on them)
    assert len(bad) == 3 * len(MALFORMED)
    p = _Pair(fn)
    try:
        p.add(vals)
        # ... and as the LAST value of the heap: one encode per value, so each in turn ends the heap while the next is mapped
        for v in MALFORMED:
            p.add([b"tail" + v])
            bad.add(b"tail" + v)
        p.add([b"end\xf0\x9f\x98"])                                 # the heap's last bytes: a lead byte that asks for one more than there is
        bad.add(b"end\xf0\x9f\x98")
        rc, err, invalid = p.map(with_invalid=with_invalid)
        if with_invalid:
            assert rc != 0 and "Invalid UTF8 sequence in input" in err and invalid == len(bad)
        else:
            assert rc == 0 and invalid == -7
        p.check(malformed=bad)
        assert not (set(p.derived.values()) & bad)
    finally:
        p.close()


def _well_formed(v):
    try:
        v.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.parametrize("fn", ["upper", "lower"])
def test_malformed_values_are_counted_and_not_inserted(fn):
    _malformed_case(fn)


def test_malformed_values_without_a_count():
    _malformed_case("upper", with_invalid=False)


# ---- 3. under the pool's guard mode -----------------------------------------------------------------------------------------------------
def test_under_the_pool_guard():
    """one leg of the entry point and all of the malformed values with every allocation red-zoned and poisoned (as
    tests/test_gpu_dictcol.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        test_every_mapped_code_point_and_the_edge_values("upper")
        test_value_counts(257)
        test_a_second_call_extends_the_table()
        _malformed_case("upper")
        _malformed_case("lower")
        _malformed_case("upper", with_invalid=False)
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


# ---- 4. KeyDictionary.mapped over a stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source_type", [pa.string(), pa.large_string(), pa.dictionary(pa.int8(), pa.string())])
def test_a_stream_of_batches_maps_each_value_once(source_type):
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    kd = KeyDictionary(source_type)
    batches = [["Berlin", "berlin", None, "Köln"], ["Köln", "Berlin", None], ["straße", "İzmir", "Berlin"], ["berlin"], ["ȿx", "KÖLN", None, "大阪"]]
    brought_new = [True, False, True, False, True]
    derived0, launches, seen = None, 0, []
    for vals, new in zip(batches, brought_new):
        arr = pa.array(vals, pa.string()).cast(source_type)
        col = DeviceColumn.from_arrow(arr, dictionary=kd)
        out = kd.mapped_column("upper", col)
        launches += new
        assert kd.map_launches == launches
        derived0 = derived0 or out.dictionary
        assert out.dictionary is derived0 and out.dictionary.type == pa.string()
        got = out.to_arrow()
        assert got.type == pa.string() and got.to_pylist() == pc.utf8_upper(pa.array(vals, pa.string())).to_pylist()
        seen += vals
    assert kd.map_ids_mapped == kd._id_count()                    # (the last batch brought new values)
    want = set(pc.utf8_upper(pa.array([v for v in seen if v is not None])).to_pylist())
    assert set(derived0.values_by_code().drop_null().to_pylist()) == want
    # the derived dictionary is a full one: a literal's code, ranks, LIKE, another map
    assert derived0.code_of("BERLIN") is not None and derived0.code_of("berlin") is None
    assert derived0.like_table("K_LN").to_numpy().sum() == 1
    lower_again, _ = derived0.mapped("lower")
    assert set(lower_again.values_by_code().drop_null().to_pylist()) == set(pc.utf8_lower(pa.array(sorted(want))).to_pylist())
    assert kd.mapped("upper")[0] is derived0 and kd.map_launches == launches


def test_sources_that_do_not_map():
    from vinum_amd.vinum_lib import KeyDictionary
    for t in (pa.binary(), pa.large_binary(), pa.dictionary(pa.int32(), pa.binary())):
        with pytest.raises(TypeError, match="needs a string column"):
            KeyDictionary(t).mapped("upper")
    for t in (pa.bool_(), pa.decimal128(10, 2)):
        with pytest.raises(NotImplementedError, match="no GPU lowering"):
            KeyDictionary(t).mapped("lower")


# ---- 5. queries through the planner and the adapter ------------------------------------------------------------------------------------
N = 4000
POOL = ["Berlin", "BERLIN", "berlin", "Köln", "KÖLN", "straße", "STRASSE", "İzmir", "izmir", "ȿal", "大阪", "Oslo", "oslo", "", "a", "A", "Zürich", "x\x00y"]
SOURCE_TYPES = {"utf8": pa.string(), "large_utf8": pa.large_string(), "dict8": pa.dictionary(pa.int8(), pa.string()),
                "dict32_large": pa.dictionary(pa.int32(), pa.large_string())}
_tables = {}


def _table(kind, n=N):
    if (kind, n) not in _tables:
        rng = np.random.default_rng(11)
        def col(seed_shift):
            idx = rng.integers(0, len(POOL), n)
            mask = rng.random(n) < 0.05
            return pa.array([POOL[i] for i in idx], pa.string(), mask=mask).cast(SOURCE_TYPES[kind]) if n else pa.array([], SOURCE_TYPES[kind])
        _tables[(kind, n)] = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "c": col(0), "d": col(1),
                                       "v": pa.array(rng.integers(0, 100, n).astype(np.int64)), "g": pa.array(rng.integers(0, 7, n).astype(np.int32))})
    return _tables[(kind, n)]


def _s(t, name):
    """the column as plain string values (what the reference's cast to string gives the function)"""
    c = t[name].combine_chunks()
    return c.cast(pa.string()) if not pa.types.is_dictionary(c.type) else c.dictionary_decode().cast(pa.string())


def _up(t, name):
    return pc.utf8_upper(_s(t, name))


def _lo(t, name):
    return pc.utf8_lower(_s(t, name))


def _np(mask, null=False):
    return mask.fill_null(null).to_numpy(zero_copy_only=False)


def _execute(query, t, batch=1300):
    from vinum_amd import planner, set_batch_size
    set_batch_size(batch)
    try:
        return planner.execute(query, t)
    finally:
        set_batch_size(1 << 24)


def _adapter(t, select, names, where=None, batch=1300):
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


@pytest.mark.parametrize("kind", list(SOURCE_TYPES))
def test_select_list(kind):
    t = _table(kind)
    select = ["k", ["fn", "upper", "c"], ["fn", "LOWER", "c"], ["fn", "upper", ["fn", "lower", "c"]], ["fn", "lower", ["fn", "upper", "d"]]]
    names = ["k", "u", "l", "ul", "lu"]
    want = {"u": _up(t, "c"), "l": _lo(t, "c"), "ul": pc.utf8_upper(_lo(t, "c")), "lu": pc.utf8_lower(_up(t, "d"))}
    for got in (_execute({"select": select, "aliases": names}, t), _adapter(t, select, names)):
        assert got["k"].to_pylist() == list(range(N))
        for name, exp in want.items():
            assert got.schema.field(name).type == pa.string()
            assert got[name].combine_chunks().equals(exp), (kind, name)


def test_zero_rows():
    from vinum_amd.core import ProjectOperator
    from vinum_amd.core.base import DeviceRecordBatch
    for t in (pa.string(), pa.dictionary(pa.int8(), pa.string())):
        b = DeviceRecordBatch.from_arrow(pa.RecordBatch.from_arrays([pa.array([], t)], names=["c"]), {})
        out = ProjectOperator([("upper", ("lower", "c"))], None, col_names=["u"])._kernel(b).to_arrow()
        assert out.num_rows == 0 and out.schema.field("u").type == pa.string()
    assert _execute({"select": ["k", ["fn", "upper", "c"]], "aliases": ["k", "u"]}, _table("utf8", 0)).num_rows == 0


def _bin(a):
    return a.cast(pa.binary())


WHERE = {
    "eq": (["eq", ["fn", "upper", "c"], ["lit", "BERLIN"]], lambda t: _np(pc.equal(_up(t, "c"), "BERLIN"))),
    "eq_flipped": (["eq", ["lit", "straße"], ["fn", "lower", "c"]], lambda t: _np(pc.equal(_lo(t, "c"), "straße"))),
    "eq_absent": (["eq", ["fn", "upper", "c"], ["lit", "berlin"]], lambda t: np.zeros(N, bool)),
    "ne": (["ne", ["fn", "upper", "c"], ["lit", "KÖLN"]], lambda t: _np(pc.not_equal(_up(t, "c"), "KÖLN"), True)),
    "lt": (["lt", ["fn", "lower", "c"], ["lit", "k"]], lambda t: _np(pc.less(_bin(_lo(t, "c")), pa.scalar(b"k")))),
    "between": (["between", ["fn", "upper", "c"], ["lit", "B"], ["lit", "P"]],
                lambda t: _np(pc.and_(pc.greater_equal(_bin(_up(t, "c")), pa.scalar(b"B")), pc.less_equal(_bin(_up(t, "c")), pa.scalar(b"P"))))),
    "in_3": (["in", ["fn", "lower", "c"], ["berlin", "köln", "nowhere"]], lambda t: _np(pc.is_in(_lo(t, "c"), value_set=pa.array(["berlin", "köln", "nowhere"])))),
    "in_20": (["in", ["fn", "upper", "c"], ["BERLIN", "OSLO", "A"] + ["N%d" % i for i in range(17)]],
              lambda t: _np(pc.is_in(_up(t, "c"), value_set=pa.array(["BERLIN", "OSLO", "A"])))),
    "like": (["like", ["fn", "lower", "c"], ["lit", "b%"]], lambda t: _np(pc.match_like(_lo(t, "c"), "b%"))),
    "not_like": (["not_like", ["fn", "upper", "c"], ["lit", "%L_"]], lambda t: ~_np(pc.match_like(_up(t, "c"), "%L_"))),
    "both_upper": (["eq", ["fn", "upper", "c"], ["fn", "upper", "d"]], lambda t: _np(pc.equal(_up(t, "c"), _up(t, "d")))),
    "col_eq_lower": (["eq", "c", ["fn", "lower", "d"]], lambda t: _np(pc.equal(_s(t, "c"), _lo(t, "d")))),
    "lower_lt_lower": (["lt", ["fn", "lower", "c"], ["fn", "lower", "d"]], lambda t: _np(pc.less(_bin(_lo(t, "c")), _bin(_lo(t, "d"))))),
}


@pytest.mark.parametrize("kind", ["utf8", "dict32_large"])
@pytest.mark.parametrize("shape", list(WHERE))
def test_where(shape, kind):
    """the project's string-column rules over the function result: bytes compared exactly, NULL compares False, `!=` True, LIKE False /
    NOT LIKE True on NULL -- computed with pyarrow.compute over pc.utf8_upper / utf8_lower of the decoded column"""
    t = _table(kind)
    where, model = WHERE[shape]
    keep = model(t)
    assert 0 < keep.sum() < N or shape == "eq_absent"
    want = t.filter(pa.array(keep))["k"].to_pylist()
    assert _execute({"select": ["k"], "where": where}, t)["k"].to_pylist() == want
    if kind == "utf8":
        assert _adapter(t, ["k"], ["k"], where=where)["k"].to_pylist() == want


@pytest.mark.parametrize("kind", list(SOURCE_TYPES))
def test_group_by_upper(kind):
    t = _table(kind)
    q = {"select": [["fn", "upper", "c"], ["fn", "count_star"], ["fn", "sum", "v"]], "aliases": ["u", "n", "s"], "group_by": [["fn", "upper", "c"]]}
    got = _execute(q, t)
    assert got.schema.field("u").type == pa.string()
    want = pa.table({"u": _up(t, "c"), "v": t["v"]}).group_by("u").aggregate([([], "count_all"), ("v", "sum")])      # pa.TableGroupBy
    exp = {u: (n, s) for u, n, s in zip(want["u"].to_pylist(), want["count_all"].to_pylist(), want["v_sum"].to_pylist())}
    assert {u: (n, s) for u, n, s in zip(got["u"].to_pylist(), got["n"].to_pylist(), got["s"].to_pylist())} == exp
    assert got.num_rows == len(exp)


def test_order_by_lower():
    t = _table("utf8")
    got = _execute({"select": ["k", "c"], "order_by": [["fn", "lower", "c"], "k"], "sort_order": ["ASC", "DESC"]}, t)
    keyed = pa.table({"k": t["k"], "c": t["c"], "l": _bin(_lo(t, "c"))})
    want = keyed.take(pc.sort_indices(keyed, sort_keys=[("l", "ascending"), ("k", "descending")]))     # (NULL last, Arrow's default and the sort operator's rule)
    assert got["k"].to_pylist() == want["k"].to_pylist()
    assert got.column_names == ["k", "c"]


@pytest.mark.parametrize("kind", ["utf8", "dict8"])
def test_sum_to_int_of_a_comparison(kind):
    t = _table(kind)
    q = {"select": ["g", ["fn", "sum", ["fn", "to_int", ["eq", ["fn", "upper", "c"], ["lit", "BERLIN"]]]],
                    ["fn", "sum", ["fn", "to_int", ["in", ["fn", "lower", "c"], ["oslo", "a"]]]]], "aliases": ["g", "b", "o"], "group_by": ["g"]}
    got = _execute(q, t)
    g = t["g"].to_numpy()
    b, o = _np(pc.equal(_up(t, "c"), "BERLIN")), _np(pc.is_in(_lo(t, "c"), value_set=pa.array(["oslo", "a"])))
    exp = {int(k): (int(b[g == k].sum()), int(o[g == k].sum())) for k in np.unique(g)}
    assert {k: (x, y) for k, x, y in zip(got["g"].to_pylist(), got["b"].to_pylist(), got["o"].to_pylist())} == exp


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from vinum_amd import binding as B
    t = _table("utf8")
    with pytest.raises(TypeError, match="needs a string column, 'v' is int64"):     # the lowering, when the batch arrives
        _adapter(t, [["upper", "v"]], ["u"])
    with pytest.raises(ValueError, match="unknown aggregate function 'upper'"):    # the planner knows a table's schema: refused at plan time
        _execute({"select": [["fn", "upper", "v"]]}, t)
    tb = pa.table({"k": t["k"], "c": _s(t, "c").cast(pa.binary())})
    with pytest.raises(TypeError, match="needs a string column"):
        _execute({"select": [["fn", "lower", "c"]]}, tb)
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        _execute({"select": ["k"], "where": ["eq", ["fn", "upper", ["lit", "x"]], ["lit", "X"]]}, t)
    with pytest.raises((ValueError, NotImplementedError)):         # concat stays outside: the planner knows no such function
        _execute({"select": [["fn", "concat", "c", "c"]]}, t)
    # ConcatFunction carries np.char.add (functions.py:263-268), which newer NumPy makes the `add` ufunc itself: either the node has
    # no lowering, or it lowers to an addition that the dictionary lowering refuses for string columns
    from vinum_amd.core.base import DeviceRecordBatch
    concat = B.VectorizedExpression([B.Column("c"), B.Column("d")], function=np.char.add, is_numpy_func=True, is_binary_func=True)
    with pytest.raises((NotImplementedError, TypeError), match="no GPU lowering|not a numeric operand"):
        B.GpuProjectOperator([concat], None, col_names=["x"])._kernel(DeviceRecordBatch.from_arrow(t.slice(0, 50).to_batches()[0], {}))


def test_a_malformed_value_raises_even_when_filtered_out():
    """the documented deviation: the batch that brings the value into the dictionary raises, whether or not a row holding it remains"""
    raw = pa.array([b"ok", b"a\xc3", b"fine"], pa.binary())
    bad = pa.Array.from_buffers(pa.string(), 3, raw.buffers())     # (no validation: what a file read without it delivers)
    t = pa.table({"k": pa.array([1, 2, 3], pa.int64()), "c": bad})
    with pytest.raises(ValueError, match="Invalid UTF8 sequence in input"):
        _execute({"select": ["k", ["fn", "upper", "c"]]}, t)
    with pytest.raises(ValueError, match="Invalid UTF8 sequence in input"):
        _execute({"select": [["fn", "upper", "c"]], "where": ["ne", "k", 2]}, t)


# ---- 6. fixtures of the reference's own planner (tests/golden/gen_golden_strcase.py) ------------------------------------------------
def _fixture_cases():
    from tests.golden import strcase_cases as C
    return C.CASES


def _compare_fixture(got, case):
    from tests import util
    want = util.read_ipc(f"strcase_{case['name']}.arrow")
    assert got.column_names == want.column_names and got.num_rows == want.num_rows
    if not case["order_by"]:                                      # no ORDER BY: rows in key order on both sides
        got, want = got.sort_by("k"), want.sort_by("k")
    for name in want.column_names:
        assert got.schema.field(name).type == want.schema.field(name).type, (case["name"], name)
        assert got[name].combine_chunks().equals(want[name].combine_chunks()), (case["name"], name)


@pytest.mark.parametrize("case", _fixture_cases(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    from tests import util
    _compare_fixture(_execute(case, util.read_ipc("strcase_in_main.arrow"), batch=400), case)


@pytest.mark.parametrize("case", [c for c in _fixture_cases() if not c["order_by"]], ids=lambda c: c["name"])
def test_reference_fixtures_through_the_adapter(case):
    """binding.vectorize trees through GpuFilterOperator / GpuProjectOperator (the adapter has no sort operator of its own: the
    ORDER BY fixture goes through the planner alone)"""
    from tests import util
    from vinum_amd.planner import _raw, output_names
    names = output_names([_raw(e) for e in case["select"]], case["aliases"])
    _compare_fixture(_adapter(util.read_ipc("strcase_in_main.arrow"), case["select"], names, where=case["where"], batch=400), case)
