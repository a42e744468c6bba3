"""concat() / || on string columns through the device dictionary: vnm_strdict_concat_affix, vnm_strdict_gather_codes and
vnm_strpair_concat through raw ctypes against a Python restatement of ConcatFunction on bytes (an operand without its trailing
NULs, "None" for NULL); the same under the pool's guard mode; KeyDictionary.affixed / paired over a stream of batches with their
counters; every golden case (tests/golden/concat_cases.py) through the planner and through the adapter.

Queries spell concat as the operator node ("concat", x, ...) or ("||", a, b); the "fn" spelling of that name stays the unknown
function tests/test_strcase_cpu.py and tests/test_gpu_strcase.py hold it to.  On the parent commit the ctypes tests find no symbol
and every end-to-end case raises: the projection compiler knows no operator "concat", the adapter answers "no GPU lowering"."""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

TILE = 1024            # rows per workgroup and step of the pair find pass (SP_TILE, csrc/vnm_strconcat.inc)


def _strip(v):
    return b"None" if v is None else v.rstrip(b"\x00")


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


# ---- 1. the affix entry through raw ctypes ----------------------------------------------------------------------------------------------
class _Affix:
    """a source and a derived dictionary handle, the table between them and the host copy of the derived values"""

    def __init__(self, prefix=b"", suffix=b""):
        from vinum_amd import _lib as L
        self.lib, self.prefix, self.suffix = L.lib(), prefix, suffix
        self.src, self.dst = self.lib.vnm_strdict_create(), self.lib.vnm_strdict_create()
        self.value_of_code, self.derived, self.table, self.null_code = {}, {}, np.zeros(0, np.int32), None

    def close(self):
        self.lib.vnm_strdict_destroy(self.src)
        self.lib.vnm_strdict_destroy(self.dst)

    def add(self, values):
        codes = _encode(self.src, values)
        for c, v in zip(codes.tolist(), values):
            assert self.value_of_code.setdefault(c, v) == v
        return codes

    def run(self, id_begin=0, prefix=None, suffix=None):
        """-> (rc, error text); self.table holds the whole table afterwards (entries below id_begin as they were)"""
        from vinum_amd import _lib as L
        from vinum_amd.device import DeviceBuffer
        lib = self.lib
        prefix, suffix = self.prefix if prefix is None else prefix, self.suffix if suffix is None else suffix
        top = int(lib.vnm_strdict_ids(self.src))
        buf = DeviceBuffer((top + 8) * 4)
        L.check(lib.vnm_memset(buf.ptr, 0x5A, buf.nbytes))
        if id_begin:
            L.check(lib.vnm_memcpy_h2d(buf.ptr, self.table.ctypes.data, id_begin * 4))
        null_code = ctypes.c_int32(-7)
        rc = lib.vnm_strdict_concat_affix(self.src, self.dst, prefix, len(prefix), suffix, len(suffix), id_begin, buf.ptr, ctypes.byref(null_code), None)
        err = L.last_error() if rc else ""
        L.check(lib.vnm_device_synchronize())
        raw = buf.to_host(np.int32, top + 8)
        assert (raw[top:] == 0x5A5A5A5A).all()                    # nothing past the ids
        if id_begin:
            assert np.array_equal(raw[:id_begin], self.table[:id_begin])      # the part it covered before is untouched
        if rc == 0:
            self.table, self.null_code = raw[:top].copy(), null_code.value
            ids, vals = _fetch_new(self.dst)
            assert len(set(ids.tolist())) == len(ids) and not (set(ids.tolist()) & set(self.derived))
            self.derived.update(zip(ids.tolist(), vals))
        return rc, err

    def image(self, v):
        return self.prefix + _strip(v) + self.suffix

    def check(self):
        top = len(self.table)
        codes = sorted(self.value_of_code)
        want = [self.image(self.value_of_code[c]) for c in codes]
        assert [self.derived.get(int(self.table[c])) for c in codes] == want
        never = np.ones(top, bool)
        never[np.array(codes, np.int64)] = False
        assert (self.table[never] == -2).all()                   # an id never handed out
        assert self.derived[self.null_code] == self.image(None)   # the NULL image, inserted by the same call
        images = set(want) | {self.image(None)}
        assert len({int(self.table[c]) for c in codes} | {self.null_code}) == len(images)     # one code per distinct image
        assert sorted(self.derived.values()) == sorted(images)    # the derived dictionary holds exactly the images
        n_ids = int(self.lib.vnm_strdict_ids(self.dst))
        assert all(0 <= c < n_ids for c in self.derived)


def _edge_values():
    vals = [b"abcdefghijklmnopq"[:k] for k in range(0, 18)]                         # lengths 0 .. 17
    vals += [b"\x00" * k for k in (1, 2, 8, 9)]                                      # only NULs: every one is the empty image
    vals += [b"y\x00", b"\x00z", b"q\x00\x00", b"x\x00y", b"\x00a\x00", b"abcdefg\x00", b"abcdefgh\x00\x00", "Köln".encode(), "大阪\x00".encode(),
             b"None", b"\xc3", b"\xff\x00"]                                          # (malformed UTF-8 is concatenated as it stands)
    return list(dict.fromkeys(vals))


@pytest.mark.parametrize("prefix,suffix", [(b"", b""), (b"#", b""), (b"", b"!"), ("«ö".encode(), b"-\x00-0123456789abcdef")])
def test_affix_edge_values(prefix, suffix):
    p = _Affix(prefix, suffix)
    try:
        codes = p.add(_edge_values())
        assert p.run() == (0, "")
        p.check()
        by_value = dict(zip(_edge_values(), codes.tolist()))
        for group in ([b"", b"\x00", b"\x00\x00", b"\x00" * 8, b"\x00" * 9], [b"abcdefg", b"abcdefg\x00"], [b"abcdefgh", b"abcdefgh\x00\x00"]):
            assert len({int(p.table[by_value[v]]) for v in group}) == 1, group        # colliding images get one code
        assert int(p.table[by_value[b"None"]]) == p.null_code                        # the value "None" and NULL are one image
        assert p.table[by_value[b"\x00z"]] != p.table[by_value[b"abcdefghijklmnopq"[:1]]] and p.derived[int(p.table[by_value[b"\x00a\x00"]])] == prefix + b"\x00a" + suffix
    finally:
        p.close()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 5000])
def test_affix_value_counts(count):
    p = _Affix(b"<", b">")
    try:
        p.add([("v%d\x00" % i).encode() if i % 3 == 0 else ("v%d" % i).encode() for i in range(count)])
        assert p.run() == (0, "")
        p.check()
    finally:
        p.close()


def test_affix_incremental_calls_and_an_empty_source():
    p = _Affix(b"", b"/x")
    try:
        assert p.run() == (0, "")                                  # no value yet: the NULL image alone
        assert p.derived == {p.null_code: b"None/x"}
        p.add([("a%d" % i).encode() for i in range(3000)])
        assert p.run() == (0, "")
        p.check()
        before, covered, null_code = dict(p.derived), len(p.table), p.null_code
        p.add([b"a7", b"a8"] + [("b%d\x00" % i).encode() for i in range(4000)] + [b"a9\x00"])     # old values, new ones, an image dst holds
        assert p.run(id_begin=covered) == (0, "")                  # (run() itself asserts the first `covered` entries are untouched)
        p.check()
        assert p.null_code == null_code and all(p.derived[c] == v for c, v in before.items()) and len(p.derived) == len(before) + 4000
        assert p.run(id_begin=len(p.table)) == (0, "")             # nothing new: nothing added, the table as it is
        p.check()
        rc, err = p.run(prefix=b"other")
        assert rc != 0 and "another prefix / suffix" in err
        rc, err = p.run(prefix=b"/", suffix=b"x")                  # the same bytes split elsewhere
        assert rc != 0 and "another prefix / suffix" in err
    finally:
        p.close()


def _gather(codes, valid, table, null_code, offset):
    """vnm_strdict_gather_codes over codes staged behind `offset` int32s (so the pointers are unaligned for offset % 4 != 0)"""
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib, n = L.lib(), len(codes)
    cbuf = DeviceBuffer.from_host(np.concatenate([np.full(offset, 12345, np.int32), codes.astype(np.int32)]))
    tbuf = DeviceBuffer.from_host(np.ascontiguousarray(table, np.int32))
    vbuf = None
    if valid is not None:
        bits = np.concatenate([np.ones(offset, bool), valid])
        vbuf = DeviceBuffer.from_host(np.packbits(bits, bitorder="little"))
    out = DeviceBuffer((offset + n + 8) * 4)
    L.check(lib.vnm_memset(out.ptr, 0x5A, out.nbytes))
    L.check(lib.vnm_strdict_gather_codes(cbuf.ptr + offset * 4, vbuf.ptr if vbuf is not None else None, offset, tbuf.ptr, len(table), n, null_code,
                                         out.ptr + offset * 4, None))
    L.check(lib.vnm_device_synchronize())
    raw = out.to_host(np.int32, offset + n + 8)
    assert (raw[:offset] == 0x5A5A5A5A).all() and (raw[offset + n:] == 0x5A5A5A5A).all()
    return raw[offset:offset + n]


@pytest.mark.parametrize("n", [1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
@pytest.mark.parametrize("offset", [0, 1, 4])
def test_gather_writes_the_null_code_and_no_validity(n, offset):
    rng = np.random.default_rng(n * 7 + offset)
    table = rng.integers(100, 200, 50).astype(np.int32)
    codes = rng.integers(-1, 50, n).astype(np.int32)
    valid = rng.random(n) > 0.2
    want = np.where((codes < 0) | ~valid, 77, table[np.maximum(codes, 0)])
    assert np.array_equal(_gather(codes, valid, table, 77, offset), want)
    assert np.array_equal(_gather(codes, None, table, 77, offset), np.where(codes < 0, 77, table[np.maximum(codes, 0)]))
    if n > 2:                                                      # a code past the table is never an address
        codes[1] = 50
        assert _gather(codes, None, table, 77, offset)[1] == -2


# ---- 2. the pair entry through raw ctypes -----------------------------------------------------------------------------------------------
class _Pairs:
    """two source dictionaries (or one, twice), the derived one, a vnm_strpair and the model: every (code_a, code_b) seen -> its
    code in dst, which must never change"""

    def __init__(self, prefix=b"", sep=b"", suffix=b"", same=False):
        from vinum_amd import _lib as L
        self.lib, self.prefix, self.sep, self.suffix = L.lib(), prefix, sep, suffix
        self.a = self.lib.vnm_strdict_create()
        self.b = self.a if same else self.lib.vnm_strdict_create()
        self.dst = self.lib.vnm_strdict_create()
        self.h = self.lib.vnm_strpair_create(prefix, len(prefix), suffix, len(suffix))
        assert self.h
        self.values = {id(self.a): {}, id(self.b): {}}             # per dictionary: code -> bytes
        self.derived, self.code_of_pair, self.calls = {}, {}, 0

    def close(self):
        self.lib.vnm_strpair_destroy(self.h)
        for h in {self.a, self.b, self.dst}:
            self.lib.vnm_strdict_destroy(h)

    def add(self, which, values):
        h = self.a if which == "a" else self.b
        codes = _encode(h, values)
        self.values[id(h)].update(zip(codes.tolist(), values))
        return codes

    def stats(self):
        from vinum_amd import _lib as L
        out = (ctypes.c_int64 * 6)()
        L.check(self.lib.vnm_strpair_stats(self.h, out, None))
        return dict(zip(("pair_launches", "pairs_concatenated", "rehashes", "slots", "occupied", "half_written"), [int(v) for v in out]))

    def run(self, ca, cb, valid_a=None, valid_b=None, offset=0, sep=None, check=True):
        """codes (-1 = NULL) and optional validity (False = NULL) behind `offset` rows -> the rows' dst codes (and checks them)"""
        from vinum_amd import _lib as L
        from vinum_amd.device import DeviceBuffer
        lib, n = self.lib, len(ca)
        sep = self.sep if sep is None else sep

        def stage(codes, valid):
            d = L.DCol()
            vals = DeviceBuffer.from_host(np.concatenate([np.full(offset, 2**30, np.int32), np.asarray(codes, np.int32)]))
            bits = DeviceBuffer.from_host(np.packbits(np.concatenate([np.ones(offset, bool), valid]), bitorder="little")) if valid is not None else None
            d.values, d.validity, d.offset, d.length, d.type, d.flags = vals.ptr, bits.ptr if bits is not None else None, offset, n, L.I32, 0
            return d, (vals, bits)
        da, keep_a = stage(ca, valid_a)
        db, keep_b = stage(cb, valid_b)
        out = DeviceBuffer((offset + n + 8) * 4)
        L.check(lib.vnm_memset(out.ptr, 0x5A, out.nbytes))
        rc = lib.vnm_strpair_concat(self.h, self.a, self.b, self.dst, sep, len(sep), ctypes.byref(da), ctypes.byref(db), n, out.ptr + offset * 4, None)
        err = L.last_error() if rc else ""
        L.check(lib.vnm_device_synchronize())
        if not check:
            return rc, err
        assert rc == 0, err
        self.calls += 1 if n else 0
        raw = out.to_host(np.int32, offset + n + 8)
        assert (raw[:offset] == 0x5A5A5A5A).all() and (raw[offset + n:] == 0x5A5A5A5A).all()
        got = raw[offset:offset + n]
        ids, vals = _fetch_new(self.dst)
        assert not (set(ids.tolist()) & set(self.derived))
        self.derived.update(zip(ids.tolist(), vals))
        va, vb = self.values[id(self.a)], self.values[id(self.b)]
        for i in range(n):
            x = None if (ca[i] < 0 or (valid_a is not None and not valid_a[i])) else int(ca[i])
            y = None if (cb[i] < 0 or (valid_b is not None and not valid_b[i])) else int(cb[i])
            want = self.prefix + _strip(None if x is None else va[x]) + self.sep + _strip(None if y is None else vb[y]) + self.suffix
            assert self.derived[int(got[i])] == want, (i, x, y)
            assert self.code_of_pair.setdefault((x, y), int(got[i])) == int(got[i])       # a pair keeps its code for good
        st = self.stats()
        assert st["pairs_concatenated"] == len(self.code_of_pair) == st["occupied"]     # string bytes once per distinct pair
        assert st["half_written"] == 0 and st["pair_launches"] == self.calls            # no slot is left without a code
        assert len(set(self.derived.values())) == len(self.derived)
        return got


_A = [b"ab", b"a", b"", b"y\x00", b"\x00z", b"q\x00\x00", b"x\x00y", "Köln".encode(), b"abcdefghijklmnopq", b"None"]
_B = [b"c", b"bc", b"", b"\x00", b"tail\x00", b"\x00lead", "大阪".encode(), b"0123456789abcdef0"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_pair_row_counts(n):
    p = _Pairs(b"<", b"-", b">")
    try:
        ca_all, cb_all = p.add("a", _A), p.add("b", _B)
        rng = np.random.default_rng(n)
        ca = np.where(rng.random(n) < 0.1, -1, ca_all[rng.integers(0, len(_A), n)]).astype(np.int32)
        cb = cb_all[rng.integers(0, len(_B), n)].astype(np.int32)
        valid_b = rng.random(n) > 0.1                               # NULL by code -1 on one side, by validity bit on the other
        p.run(ca, cb, None, valid_b)
        if n == 0:
            assert p.stats()["pair_launches"] == 0
    finally:
        p.close()


def test_pair_nulls_on_either_and_both_sides():
    p = _Pairs(b"", b" ", b"")
    try:
        ca, cb = p.add("a", [b"Ada", b"y\x00"]), p.add("b", [b"Lovelace", b"\x00"])
        a = np.array([ca[0], -1, ca[0], -1, ca[1], ca[1], ca[0]], np.int32)
        b = np.array([cb[0], cb[0], -1, -1, cb[1], cb[0], cb[0]], np.int32)
        valid_a = np.array([1, 1, 1, 1, 1, 1, 0], bool)            # the last row: NULL by the bit, whatever the code says
        got = p.run(a, b, valid_a, np.ones(7, bool))
        assert [p.derived[int(c)] for c in got] == [b"Ada Lovelace", b"None Lovelace", b"Ada None", b"None None", b"y ", b"y Lovelace", b"None Lovelace"]
        assert got[1] == got[6] and p.stats()["pairs_concatenated"] == 6
    finally:
        p.close()


def test_pair_every_row_the_same_pair():
    p = _Pairs()
    try:
        ca, cb = p.add("a", _A), p.add("b", _B)
        n = 5 * TILE + 3                                            # all lanes on one slot
        got = p.run(np.full(n, ca[0], np.int32), np.full(n, cb[0], np.int32))
        assert len(set(got.tolist())) == 1 and p.stats()["pairs_concatenated"] == 1
        before = p.stats()
        p.run(np.full(n, ca[0], np.int32), np.full(n, cb[0], np.int32))         # only known pairs: nothing concatenated
        after = p.stats()
        assert after["pairs_concatenated"] == before["pairs_concatenated"] == 1 and after["pair_launches"] == 2
        assert int(p.lib.vnm_strdict_ids(p.dst)) >= 1 and len(p.derived) == 1
    finally:
        p.close()


def test_pair_growth_keeps_the_codes(monkeypatch):
    monkeypatch.setenv("VNM_STRPAIR_SLOTS", "64")
    p = _Pairs(b"", b"|", b"")
    try:
        ca = p.add("a", [("a%d\x00" % i).encode() for i in range(40)])
        cb = p.add("b", [("b%d" % i).encode() for i in range(30)])
        ia, ib = np.divmod(np.arange(1200), 30)
        first = p.run(ca[ia[:30]], cb[ib[:30]])                     # 30 pairs: inside the 64 slots
        assert p.stats()["rehashes"] == 0 and p.stats()["slots"] == 64
        order = np.random.default_rng(3).permutation(1200)
        allc = p.run(ca[ia[order]], cb[ib[order]])                   # every row a distinct pair: 1200 pairs
        st = p.stats()
        assert st["rehashes"] >= 2 and st["slots"] >= 2048 and st["pairs_concatenated"] == 1200
        back = np.empty(1200, np.int32)
        back[order] = allc
        assert np.array_equal(back[:30], first)                    # (run() also holds every pair to its first code)
        rehashes = st["rehashes"]
        again = p.run(ca[ia], cb[ib])                               # known pairs only: no growth, nothing concatenated
        assert np.array_equal(again, back) and p.stats()["rehashes"] == rehashes and p.stats()["pairs_concatenated"] == 1200
    finally:
        p.close()


def test_pair_a_second_batch_after_a_dictionary_grew():
    p = _Pairs(b"", b"-", b"!")
    try:
        ca, cb = p.add("a", _A), p.add("b", _B)
        rng = np.random.default_rng(5)
        p.run(ca[rng.integers(0, len(_A), 500)], cb[rng.integers(0, len(_B), 500)])
        more = p.add("a", [("new%d" % i).encode() for i in range(3000)])          # ids past what the first call saw
        p.run(np.concatenate([more, ca]), np.concatenate([cb[rng.integers(0, len(_B), 3000)], cb[rng.integers(0, len(_B), len(ca))]]))
    finally:
        p.close()


def test_pair_colliding_pairs_take_two_slots_and_one_code():
    p = _Pairs()
    try:
        ca, cb = p.add("a", [b"ab", b"a", b"abc\x00"]), p.add("b", [b"c", b"bc", b"\x00"])
        got = p.run(np.array([ca[0], ca[1], ca[2], ca[0]], np.int32), np.array([cb[0], cb[1], cb[2], cb[0]], np.int32))
        assert len(set(got.tolist())) == 1 and p.derived[int(got[0])] == b"abc"
        st = p.stats()
        assert st["occupied"] == 3 and st["pairs_concatenated"] == 3 and len(p.derived) == 1
    finally:
        p.close()


@pytest.mark.parametrize("offset", [1, 2, 3, 5])
def test_pair_unaligned_code_pointers(offset):
    p = _Pairs(b"", b"+", b"")
    try:
        ca, cb = p.add("a", _A), p.add("b", _B)
        rng = np.random.default_rng(offset)
        n = 2 * TILE + 5
        p.run(ca[rng.integers(0, len(_A), n)], cb[rng.integers(0, len(_B), n)], rng.random(n) > 0.1, rng.random(n) > 0.1, offset=offset)
    finally:
        p.close()


def test_pair_one_dictionary_on_both_sides_and_the_refusals():
    p = _Pairs(b"", b"=", b"", same=True)
    try:
        c = p.add("a", _A)
        rng = np.random.default_rng(9)
        p.run(c[rng.integers(0, len(_A), 700)], c[rng.integers(0, len(_A), 700)])
        p.run(c[:4], c[:4])                                         # (the pairs of the refused calls below are known ones)
        rc, err = p.run(c[:4], c[:4], sep=b"/", check=False)
        assert rc != 0 and "another separator" in err
        top = int(p.lib.vnm_strdict_ids(p.a))
        rc, err = p.run(np.array([c[0], top], np.int32), np.array([c[0], c[0]], np.int32), check=False)     # a code that is no id
        assert rc != 0 and "outside their dictionary" in err
        rc, err = p.run(np.array([-2], np.int32), np.array([c[0]], np.int32), check=False)
        assert rc != 0 and "outside their dictionary" in err
    finally:
        p.close()


# ---- 3. under the pool's guard mode -----------------------------------------------------------------------------------------------------
def test_under_the_pool_guard(monkeypatch):
    """the same selection with every allocation red-zoned and poisoned (as tests/test_gpu_strcase.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        test_affix_edge_values("«ö".encode(), b"-\x00-0123456789abcdef")
        test_affix_value_counts(257)
        test_affix_incremental_calls_and_an_empty_source()
        test_gather_writes_the_null_code_and_no_validity(TILE + 1, 1)
        for n in (1, 65, TILE + 1):
            test_pair_row_counts(n)
        test_pair_nulls_on_either_and_both_sides()
        test_pair_growth_keeps_the_codes(monkeypatch)
        test_pair_a_second_batch_after_a_dictionary_grew()
        test_pair_unaligned_code_pointers(3)
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


# ---- 4. KeyDictionary over a stream of batches: string work per distinct value or pair, not per row ------------------------------------
_main = {}


def _main_table():
    from tests import util
    if "t" not in _main:
        _main["t"] = util.read_ipc("concat_in_main.arrow")
    return _main["t"]


def test_a_stream_of_batches_concatenates_each_pair_once():
    from tests.golden import concat_cases as C
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    t = _main_table()
    da, db, dd = KeyDictionary(t.schema.field("a").type), KeyDictionary(t.schema.field("b").type), KeyDictionary(t.schema.field("d").type)
    pairs, dvals, tables, launches = set(), set(), set(), 0
    for start in range(0, t.num_rows, 400):                        # five batches
        part = t.slice(start, 400)
        ca, cb, cd = (DeviceColumn.from_arrow(part[n], dictionary=kd) for n, kd in (("a", da), ("b", db), ("d", dd)))
        out = da.pair_column(db, b"<", b"-", b">", ca, cb)
        assert out.validity_ptr is None and out.dictionary.type == pa.string()
        assert out.to_arrow().to_pylist() == C.restate(part, ["concat", ["lit", "<"], "a", ["lit", "-"], "b", ["lit", ">"]])
        pairs |= set(zip(part["a"].to_pylist(), part["b"].to_pylist()))
        table = da.paired(db, b"<", b"-", b">")
        tables.add(id(table))
        st = table.stats()
        assert st["pairs_concatenated"] == len(pairs) and st["pair_launches"] == start // 400 + 1 and st["half_written"] == 0
        # one column: the dictionary-typed one, each distinct value written once
        before = set(dvals)
        dvals |= set(part["d"].to_pylist()) - {None}
        one = dd.affixed_column(b"", b":", cd)
        launches += (dvals != before) or start == 0
        assert dd.affix_launches == launches
        assert one.validity_ptr is None and one.to_arrow().to_pylist() == C.restate(part, ["concat", "d", ["lit", ":"]])
    assert len(tables) == 1 and len(pairs) < 400                   # one table for the stream; far fewer pairs than rows
    assert table.stats()["pairs_concatenated"] == len(pairs)
    assert dd.affix_ids_mapped <= dd._id_count()
    derived = table.derived                                         # a full dictionary: a literal's code, LIKE, another function
    assert derived.code_of("<Ada-Lovelace>") is not None and derived.like_table("<Ada-%").to_numpy().sum() >= 1
    assert derived.mapped("upper")[0].code_of("<ADA-LOVELACE>") is not None


# ---- 5. queries through the planner and the adapter ------------------------------------------------------------------------------------
def _execute(query, t, batch=400):
    from vinum_amd import planner, set_batch_size
    set_batch_size(batch)
    try:
        return planner.execute(query, t)
    finally:
        set_batch_size(1 << 24)


def _adapter(t, select, names, where=None, batch=400):
    """binding.vectorize trees through GpuFilterOperator / GpuProjectOperator (so binding.lower and the mirror classes run)"""
    from vinum_amd import binding as B
    from vinum_amd import set_batch_size
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    from vinum_amd.planner import _t
    op = TableReaderOperator(t)
    if where is not None:
        op = B.GpuFilterOperator(B.vectorize(_t(where)), op)
    op = B.GpuProjectOperator([B.vectorize(_t(e) if not (isinstance(e, list) and e[0] == "||") else _tuple(e)) for e in select], op, col_names=names)
    set_batch_size(batch)
    try:
        return next(MaterializeTableOperator(op).next())
    finally:
        set_batch_size(1 << 24)


def _tuple(e):
    return tuple(_tuple(x) for x in e) if isinstance(e, list) else e


def _cases():
    from tests.golden import concat_cases as C
    return C.CASES


def _restated():
    from tests.golden import concat_cases as C
    return C.RESTATED


def _compare_fixture(got, case):
    """the fixture is the reference's own result.  A string column of it went through pa.array(ndarray 'U'), which cuts a value at
    its first NUL (tests/golden/concat_cases.py): the result must equal the restatement of ConcatFunction, the fixture the result
    cut that way -- for a value without a NUL, which is nearly all of them, the two are one comparison."""
    from tests import util
    from tests.golden import concat_cases as C
    want, t = util.read_ipc(f"concat_{case['name']}.arrow"), _main_table()
    assert got.column_names == want.column_names and got.num_rows == want.num_rows
    if not case["order_by"]:                                      # no ORDER BY: rows in key order on both sides
        got, want = got.sort_by("k"), want.sort_by("k")
    for name, e in zip(want.column_names, case["select"]):
        assert got.schema.field(name).type == want.schema.field(name).type, (case["name"], name)
        if isinstance(e, list) and not case["where"] and not case["order_by"]:
            assert got[name].null_count == 0 and got[name].to_pylist() == C.restate(t, e), (case["name"], name)
            assert C.cut_at_nul(got[name].to_pylist()) == want[name].to_pylist(), (case["name"], name)
        else:
            assert got[name].combine_chunks().equals(want[name].combine_chunks()), (case["name"], name)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    _compare_fixture(_execute(case, _main_table()), case)


@pytest.mark.parametrize("case", [c for c in _cases() if not c["order_by"]], ids=lambda c: c["name"])
def test_reference_fixtures_through_the_adapter(case):
    """(the adapter has no sort operator of its own: the ORDER BY fixture goes through the planner alone)"""
    from vinum_amd.planner import _raw, output_names
    names = output_names([_raw(e) for e in case["select"]], case["aliases"])
    _compare_fixture(_adapter(_main_table(), case["select"], names, where=case["where"]), case)


def test_pipe_operator_through_the_adapter():
    """`a || b` (SQLExpression.CONCAT): the adapter case list, against the restatement and the two-column fixture"""
    from tests import util
    from tests.golden import concat_cases as C
    t = _main_table()
    for _name, select, names in C.ADAPTER_PIPE:
        got = _adapter(t, select, names).sort_by("k")
        for e, name in zip(select[1:], names[1:]):
            assert got.schema.field(name).type == pa.string() and got[name].to_pylist() == C.restate(t, e), name
    assert C.cut_at_nul(got["ab"].to_pylist()) == util.read_ipc("concat_two_columns.arrow").sort_by("k")["ab"].to_pylist()
    assert _execute({"select": ["k", ["||", "a", "b"]], "aliases": ["k", "ab"]}, t).sort_by("k")["ab"].to_pylist() == got["ab"].to_pylist()


def test_restated_select_list():
    """two concat() calls that begin with one column: the reference's planner loses the shared node (concat_cases.json)"""
    from tests.golden import concat_cases as C
    from vinum_amd.planner import _raw, output_names
    case, t = next(c for c in _restated() if c["name"] == "shared_first_column"), _main_table()
    names = output_names([_raw(e) for e in case["select"]], case["aliases"])
    for got in (_execute(case, t).sort_by("k"), _adapter(t, case["select"], names).sort_by("k")):
        assert got.column_names == names
        for e, name in zip(case["select"][1:], names[1:]):
            assert got.schema.field(name).type == pa.string() and got[name].null_count == 0
            assert got[name].to_pylist() == C.restate(t, e), name


def test_restated_group_by_key_with_count_and_sum():
    from tests.golden import concat_cases as C
    case, t = next(c for c in _restated() if c["name"] == "group_by"), _main_table()
    got = _execute(case, t)
    assert got.column_names == ["c", "n", "s", "m"] and got.schema.field("c").type == pa.string()
    keys, v = C.restate(t, case["group_by"][0]), t["v"].to_pylist()
    exp = {}
    for key, x in zip(keys, v):
        n, s = exp.get(key, (0, 0))
        exp[key] = (n + 1, s + x)
    assert {c: (n, s) for c, n, s in zip(got["c"].to_pylist(), got["n"].to_pylist(), got["s"].to_pylist())} == exp
    assert got.num_rows == len(exp) and got["m"].to_pylist() == got["n"].to_pylist()      # count(concat(..)): never NULL, every row counts


def test_restated_order_by_over_values_with_nuls():
    """byte-wise order of the whole values, as every string sort key of this project (the reference sorts the column it cut)"""
    from tests.golden import concat_cases as C
    case, t = next(c for c in _restated() if c["name"] == "order_by_with_nuls"), _main_table()
    got = _execute(case, t)
    keys, ks = C.restate(t, case["order_by"][0]), t["k"].to_pylist()
    order = sorted(range(t.num_rows), key=lambda i: ks[i])
    order.sort(key=lambda i: keys[i].encode(), reverse=True)       # (stable: k ascending inside equal keys)
    assert got.column_names == ["k", "a"] and got["k"].to_pylist() == [ks[i] for i in order]


def test_restated_distinct():
    from tests.golden import concat_cases as C
    case, t = next(c for c in _restated() if c["name"] == "distinct"), _main_table()
    got = _execute(case, t)
    want = set(C.restate(t, case["select"][0]))
    assert got.num_rows == len(want) and set(got["c"].to_pylist()) == want


WHERE = {
    "lt": (["lt", ["concat", "a", "b"], ["lit", "M"]], lambda s: s.encode() < b"M"),
    "ne": (["ne", ["concat", "p", "q"], ["lit", "abc"]], lambda s: s != "abc"),
    "in": (["in", ["concat", "p", ["lit", "-"], "q"], ["ab-c", "a-bc", "None-None", "nowhere"]], lambda s: s in ("ab-c", "a-bc", "None-None")),
    "like": (["like", ["concat", "a", ["lit", " "], "b"], ["lit", "Ada %"]], lambda s: s.startswith("Ada ")),
    "between": (["between", ["concat", "a", "b"], ["lit", "B"], ["lit", "P"]], lambda s: b"B" <= s.encode() <= b"P"),
    "pair_eq_pair": (["eq", ["concat", "p", "q"], ["concat", "q", "p"]], None),
}


@pytest.mark.parametrize("shape", list(WHERE))
def test_where_follows_the_string_rules(shape):
    """the result is an ordinary string column: bytes compared exactly, byte-wise order, IN, LIKE, BETWEEN, column against column"""
    from tests.golden import concat_cases as C
    t = _main_table()
    where, model = WHERE[shape]
    node = where[1]
    if model is None:
        x, y = C.restate(t, where[1]), C.restate(t, where[2])
        keep = [a == b for a, b in zip(x, y)]
    else:
        keep = [bool(model(s)) for s in C.restate(t, node)]
    assert 0 < sum(keep) < t.num_rows
    want = [k for k, ok in zip(t["k"].to_pylist(), keep) if ok]
    assert sorted(_execute({"select": ["k"], "where": where}, t)["k"].to_pylist()) == want
    assert sorted(_adapter(t, ["k"], ["k"], where=where)["k"].to_pylist()) == want


def test_zero_rows_and_errors():
    t = _main_table()
    assert _execute({"select": ["k", ["concat", "a", "b"]], "aliases": ["k", "c"]}, t.slice(0, 0)).num_rows == 0
    with pytest.raises(TypeError, match="'v' is int64"):           # the planner knows a table's schema: refused at plan time
        _execute({"select": [["concat", "a", "v"]]}, t)
    with pytest.raises(TypeError, match="needs a string column, 'v' is int64"):     # the lowering, when the batch arrives
        _adapter(t, [["concat", "a", "v"]], ["c"])
    tb = pa.table({"k": t["k"], "a": t["a"], "r": t["a"].cast(pa.binary())})
    with pytest.raises(TypeError, match="needs a string column"):
        _execute({"select": [["concat", "a", "r"]]}, tb)
    with pytest.raises(NotImplementedError, match="literals alone"):
        _execute({"select": ["k"], "where": ["eq", ["concat", ["lit", "x"], 7], ["lit", "x7"]]}, t)
