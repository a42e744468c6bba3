"""date() / datetime() / from_timestamp() on the device: vnm_strdict_parse_datetime, vnm_strdict_gather_temporal and
vnm_temporal_rescale through raw ctypes against NumPy's own parser and casts (what DatetimeFunction computes,
vinum/core/functions.py:112-119) -- dictionaries of 0, 1, 5 and 70 000 values, the last built in two encodes so that id_begin extends
a table; the row pass over the lengths round the 64-row wavefront and the 2048-row workgroup, without validity and with it at Arrow
offsets 1 and 7, with codes of -1 and codes past the table, both output widths, the bitmap's bits past n left alone --; the same
under the pool's guard mode; whole queries through the planner over every batch split against NumPy / pyarrow on the host; and the
golden cases of the reference's own planner (tests/golden/datetime_cases.py).

On the parent commit the ctypes tests find no symbol and every query raises: the planner knows no function "date"."""
import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests.test_dtparse_host_cpu import NULL, REFUSED, UNITS, VALUE, expected

pytestmark = pytest.mark.gpu

TILE = 2048            # rows per workgroup and step of the row pass (DT_TILE, csrc/vnm_datetime.inc), 8 rows per lane
LENGTHS = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 7)
I64_MIN, I64_MAX = -2**63, 2**63 - 1
FILL = 0x5A


# ---- 1. the kernels through raw ctypes -----------------------------------------------------------------------------------------------------
def _mixed_values(n, seed):
    """n DISTINCT strings: accepted in every depth of the grammar, NULL ('' once, NaT in several cases), refused"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    special = ["", "NaT", "nat", "NAT", "2021-02-29", "2020-13-01", "2020-10-08t03", " 2020-10-08", "2020-10-08T03:26:54Z", "now", "2020-1-6", "x",
               "0000-01-01", "9999-12-31T23:59:59.999999999", "1969-12-31T23:59:59.9", "1960-01-01T00:00:00.0005", "2020", "2020-10", "2020-10-08 03"]
    for s in special[:n]:
        out.append(s)
        seen.add(s)
    while len(out) < n:
        y, mo, d = int(rng.integers(0, 10000)), int(rng.integers(1, 13)), int(rng.integers(1, 32))
        h, mi, s = int(rng.integers(0, 25)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
        kind = int(rng.integers(0, 10))
        text = f"{y:04d}-{mo:02d}-{d:02d}" if kind == 0 else f"{y:04d}-{mo:02d}-{d:02d} {h:02d}:{mi:02d}:{s:02d}" if kind < 7 else \
            f"{y:04d}-{mo:02d}-{d:02d}T{h:02d}:{mi:02d}:{s:02d}.{int(rng.integers(0, 10**9)):09d}"[:int(rng.integers(20, 30))] if kind < 9 else f"bad{len(out)}"
        if text not in seen:
            seen.add(text)
            out.append(text)
    return out


class _Dict:
    """a device dictionary built by encodes, the host copy of value -> id, and its parsed tables through raw ctypes"""

    def __init__(self):
        from vinum_amd.keydict import KeyDictionary
        self.kd = KeyDictionary(pa.string())
        self.id_of = {}

    def encode(self, values):
        codes = self.kd._encode_values(pa.array(values, pa.string()))
        self.id_of.update(zip(values, (int(c) for c in codes)))
        return codes

    @property
    def ids(self):
        return self.kd._id_count()

    def parse(self, unit, id_begin, value_buf, status_buf):
        from vinum_amd import _lib as L
        refused = ctypes.c_int64(-7)
        L.check(L.lib().vnm_strdict_parse_datetime(self.kd.handle(), UNITS.index(unit), id_begin, value_buf.ptr, status_buf.ptr, ctypes.byref(refused), None))
        return refused.value

    def check_tables(self, unit, values_host, status_host, id_begin, first_refused):
        """ids [id_begin, ids) against NumPy; an id never handed out has status 2; the lowest refused id handed out is returned"""
        want_refused = []
        handed = np.zeros(self.ids, bool)
        for text, i in self.id_of.items():
            handed[i] = True
            if i < id_begin:
                continue
            st, v = expected(text.encode(), unit)
            assert (int(status_host[i]), int(values_host[i])) == (st, v), (text, unit, i)
            if st == REFUSED:
                want_refused.append(i)
        holes = np.nonzero(~handed[id_begin:])[0] + id_begin
        assert (status_host[holes] == REFUSED).all() and (values_host[holes] == 0).all()
        assert first_refused == (min(want_refused) if want_refused else -1)


def _tables(d, unit, pad=8):
    """fresh device tables of d.ids entries behind and in front of `pad` entries of fill"""
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    values, status = DeviceBuffer((d.ids + 2 * pad) * 8), DeviceBuffer(d.ids + 2 * pad)
    for b in (values, status):
        L.check(L.lib().vnm_memset(b.ptr, FILL, b.nbytes))
    return values, status


class _At:
    """a DeviceBuffer seen from `skip` bytes in"""

    def __init__(self, buf, skip):
        self.ptr = buf.ptr + skip


@pytest.mark.parametrize("n_values", [0, 1, 5])
@pytest.mark.parametrize("unit", UNITS)
def test_small_dictionaries_in_every_unit_against_numpy(n_values, unit):
    from vinum_amd import _lib as L
    d = _Dict()
    if n_values:
        d.encode(["2020-10-08 03:26:54.123456789", "", "2021-02-29", "NaT", "1969-12-31T23:59:59.9"][:n_values][::-1] if n_values == 5 else ["2020-10-08"])
    pad = 8
    values, status = _tables(d, unit, pad)
    refused = d.parse(unit, 0, _At(values, pad * 8), _At(status, pad))
    L.check(L.lib().vnm_device_synchronize())
    v, s = values.to_host(np.int64, d.ids + 2 * pad), status.to_host(np.uint8, d.ids + 2 * pad)
    fill64 = int.from_bytes(bytes([FILL]) * 8, "little")
    assert (v[:pad] == fill64).all() and (v[pad + d.ids:] == fill64).all() and (s[:pad] == FILL).all() and (s[pad + d.ids:] == FILL).all()
    d.check_tables(unit, v[pad:pad + d.ids], s[pad:pad + d.ids], 0, refused)
    if n_values == 5:
        assert sorted(int(s[pad + i]) for i in d.id_of.values()) == [VALUE, VALUE, NULL, NULL, REFUSED]


_big = {}


def _big_dictionary():
    """70 000 values in two encodes; the table of unit s parsed in two calls, the second with id_begin = the first's id count"""
    if _big:
        return _big
    from vinum_amd import _lib as L
    values = _mixed_values(70_000, 31)
    values[-1] = "2262-04-11T23:47:16.854775807"               # the LAST value of the heap: 29 bytes read up to its end
    assert len(set(values)) == len(values)
    d = _Dict()
    d.encode(values[:40_000])
    first_ids = d.ids
    tv, ts = _tables(d, "s", 0)
    first_refused = d.parse("s", 0, tv, ts)
    L.check(L.lib().vnm_device_synchronize())
    v1, s1 = tv.to_host(np.int64, first_ids), ts.to_host(np.uint8, first_ids)
    d.check_tables("s", v1, s1, 0, first_refused)
    d.encode(values[40_000:])
    assert d.ids > first_ids
    gv, gs = _tables(d, "s", 0)                                  # the grown tables: the covered part copied, the rest fill
    L.check(L.lib().vnm_memcpy_d2d(gv.ptr, tv.ptr, first_ids * 8, None))
    L.check(L.lib().vnm_memcpy_d2d(gs.ptr, ts.ptr, first_ids, None))
    second_refused = d.parse("s", first_ids, gv, gs)
    L.check(L.lib().vnm_device_synchronize())
    v2, s2 = gv.to_host(np.int64, d.ids), gs.to_host(np.uint8, d.ids)
    assert (v2[:first_ids] == v1).all() and (s2[:first_ids] == s1).all()          # only [id_begin, ids) is written
    d.check_tables("s", v2, s2, first_ids, second_refused)
    _big.update(d=d, values=values, dev=(gv, gs), host=(v2, s2))
    return _big


def test_a_dictionary_of_70000_values_extended_with_id_begin():
    big = _big_dictionary()
    v, s = big["host"]
    counts = np.bincount(s[[big["d"].id_of[t] for t in big["values"]]], minlength=3)
    assert counts[VALUE] > 50_000 and counts[NULL] == 4 and counts[REFUSED] > 5_000
    from vinum_amd import _lib as L
    assert L.lib().vnm_strdict_parse_datetime(big["d"].kd.handle(), 9, 0, big["dev"][0].ptr, big["dev"][1].ptr, None, None) != 0
    assert "unknown unit" in L.last_error()
    assert L.lib().vnm_strdict_parse_datetime(big["d"].kd.handle(), 1, big["d"].ids + 5, big["dev"][0].ptr, big["dev"][1].ptr, None, None) == 0


def _gather(codes, valid, offset, values_dev, status_dev, values_host, status_host, n_ids, width, count_nulls=True):
    """one row pass held against the host copies of the tables: values, validity bits, the fill around both outputs, the NULL count"""
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib = L.lib()
    n = len(codes)
    codes_dev = DeviceBuffer.from_host(np.concatenate([np.full(offset, 3, np.int32), codes.astype(np.int32)]))
    bits = DeviceBuffer.from_host(np.packbits(np.concatenate([np.zeros(offset, bool), valid]), bitorder="little")) if valid is not None else None
    dtype = np.int32 if width == 4 else np.int64
    lead = 16 + (offset % 2) * width                   # (an odd offset also moves row 0 of the output off the 16-byte boundary)
    out = DeviceBuffer(lead + (n + 16) * width)
    nbytes = (n + 7) >> 3
    bitmap = DeviceBuffer(nbytes + 8)
    for b in (out, bitmap):
        L.check(lib.vnm_memset(b.ptr, FILL, b.nbytes))
    nulls, refused = ctypes.c_int64(-1), ctypes.c_int64(-7)
    L.check(lib.vnm_strdict_gather_temporal(codes_dev.ptr + offset * 4, bits.ptr if bits is not None else None, offset, values_dev.ptr, status_dev.ptr,
                                            n_ids, n, width, out.ptr + lead, bitmap.ptr, ctypes.byref(nulls) if count_nulls else None,
                                            ctypes.byref(refused) if count_nulls else None, None))
    L.check(lib.vnm_device_synchronize())
    raw = out.to_host(np.uint8, out.nbytes)
    got = raw[lead:lead + n * width].view(dtype)
    assert (raw[:lead] == FILL).all() and (raw[lead + n * width:] == FILL).all()
    got_bits = bitmap.to_host(np.uint8, nbytes + 8)
    assert (got_bits[nbytes:] == FILL).all()                                  # the bytes past (n + 7) / 8 ...
    unpacked = np.unpackbits(got_bits[:nbytes], bitorder="little").astype(bool)
    assert (unpacked[n:] == np.unpackbits(np.full(nbytes, FILL, np.uint8), bitorder="little").astype(bool)[n:]).all()    # ... and the bits past n
    inside = (codes >= 0) & (codes < n_ids)
    safe = np.where(inside, codes, 0)
    st = status_host[safe] if n_ids else np.zeros(n, np.uint8)
    want_valid = inside & (st != NULL) & (valid if valid is not None else True)
    want = np.where(want_valid, values_host[safe] if n_ids else 0, 0).astype(np.int64).astype(dtype)
    assert (unpacked[:n] == want_valid).all()
    assert (got == want).all()
    assert nulls.value == (int((~want_valid).sum()) if count_nulls else -1)
    held = codes[want_valid & (st == REFUSED)]                                # the refused ids non-NULL rows hold: the lowest is reported
    assert refused.value == ((int(held.min()) if len(held) else -1) if count_nulls else -7)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("offset", [None, 1, 7])
def test_the_row_pass_at_every_length(width, offset):
    big = _big_dictionary()
    n_ids = big["d"].ids
    rng = np.random.default_rng(5 + width + (offset or 0))
    (vd, sd), (vh, sh) = big["dev"], big["host"]
    for n in LENGTHS:
        codes = rng.integers(0, n_ids, n).astype(np.int64)
        codes[rng.random(n) < 0.05] = -1
        codes[rng.random(n) < 0.05] = n_ids
        codes[rng.random(n) < 0.02] = 2**31 - 1
        codes[rng.random(n) < 0.02] = -2**31
        valid = None if offset is None else rng.random(n) < 0.8
        _gather(codes, valid, offset or 0, vd, sd, vh, sh, n_ids, width, count_nulls=(n % 2 == 1))
    # a table of no ids: every row is NULL, nothing is an address
    from vinum_amd.device import DeviceBuffer
    none = DeviceBuffer(8)
    _gather(np.array([0, -1, 5]), None, 0, none, none, np.zeros(0, np.int64), np.zeros(0, np.uint8), 0, width)


def test_the_row_pass_refuses_what_it_cannot_take():
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    b = DeviceBuffer(64)
    assert L.lib().vnm_strdict_gather_temporal(b.ptr, None, 0, b.ptr, b.ptr, 1, 1, 2, b.ptr, b.ptr, None, None, None) != 0 and "out_width" in L.last_error()
    assert L.lib().vnm_strdict_gather_temporal(b.ptr, None, 0, b.ptr, b.ptr, 1, 1, 8, b.ptr, None, None, None, None) != 0 and "null argument" in L.last_error()


_RESCALE_I64 = np.array([-1, 0, 86399, 86400, -86400, -86401, I64_MIN + 1, I64_MAX], np.int64)
_RESCALE_I32 = np.array([-1, 0, 86399, 86400, -86400, -86401, -2**31 + 1, 2**31 - 1], np.int32)
_PER_DAY = {"D": 1, "s": 86_400, "ms": 86_400_000, "ns": 86_400 * 10**9}


@pytest.mark.parametrize("have, want", [("D", "s"), ("s", "D"), ("s", "ns"), ("ns", "s"), ("ms", "D")])
def test_rescale_against_numpys_cast(have, want):
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    lib = L.lib()
    base = _RESCALE_I32 if have == "D" else _RESCALE_I64
    width = 4 if want == "D" else 8
    a, b = _PER_DAY[have], _PER_DAY[want]
    mul, div = (b // a, 1) if b >= a else (1, a // b)
    for n in LENGTHS:
        for offset in (0, 3):
            values = np.resize(base, n) if n else base[:0]
            cast = values.astype(np.int64).view(f"datetime64[{have}]").astype(f"datetime64[{want}]").view(np.int64)
            col = DeviceBuffer.from_host(np.concatenate([np.full(offset, 77, base.dtype), values]))
            d = L.DCol()
            d.values, d.validity, d.offset, d.length, d.type, d.flags = col.ptr, None, offset, n, L.I32 if have == "D" else L.I64, 0
            out = DeviceBuffer((n + 8) * width)
            L.check(lib.vnm_memset(out.ptr, FILL, out.nbytes))
            L.check(lib.vnm_temporal_rescale(ctypes.byref(d), mul, div, n, width, out.ptr + 4 * width, None))
            L.check(lib.vnm_device_synchronize())
            raw = out.to_host(np.uint8, out.nbytes)
            got = raw[4 * width:(4 + n) * width].view(np.int32 if width == 4 else np.int64)
            assert (raw[:4 * width] == FILL).all() and (raw[(4 + n) * width:] == FILL).all()
            assert (got == cast.astype(got.dtype)).all(), (have, want, n, offset)


def test_rescale_takes_the_six_values_of_the_issue_and_refuses_other_shapes():
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    from vinum_amd.keydict import rescaled_column, timestamp_column
    from vinum_amd.device import DeviceColumn
    secs = pa.array([-1, 0, 86399, 86400, -86400, -86401, None], pa.timestamp("s"))
    got = rescaled_column(DeviceColumn.from_arrow(secs), "D").to_arrow()
    assert got.type == pa.date32() and got.cast(pa.int32()).to_pylist() == [-1, 0, 0, 1, -1, -2, None]
    narrow = timestamp_column(DeviceColumn.from_arrow(pa.array([-5, None, 2**31 - 1], pa.int32())), "ms").to_arrow()
    assert narrow.type == pa.timestamp("ms") and narrow.cast(pa.int64()).to_pylist() == [-5, None, 2**31 - 1]
    b = DeviceBuffer(64)
    d = L.DCol()
    d.values, d.validity, d.offset, d.length, d.type, d.flags = b.ptr, None, 0, 4, L.F64, 0
    assert L.lib().vnm_temporal_rescale(ctypes.byref(d), 1, 86400, 4, 4, b.ptr, None) != 0 and "narrower than VNM_U64" in L.last_error()
    d.type = L.U64
    assert L.lib().vnm_temporal_rescale(ctypes.byref(d), 1, 1, 4, 8, b.ptr, None) != 0
    d.type = L.I64
    assert L.lib().vnm_temporal_rescale(ctypes.byref(d), 1000, 1000, 4, 8, b.ptr, None) != 0 and "mul / div" in L.last_error()
    assert L.lib().vnm_temporal_rescale(ctypes.byref(d), 1, 1000, 5, 8, b.ptr, None) != 0 and "length" in L.last_error()


# ---- 2. under the pool's guard mode -----------------------------------------------------------------------------------------------------
def test_under_the_pool_guard():
    """the parity cases once more with every allocation red-zoned and poisoned (as tests/test_gpu_to_str.py runs its guard leg)"""
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    saved = dict(_big)
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        _big.clear()                                     # (the big dictionary and its tables are built again, inside guarded blocks)
        for unit in UNITS:
            test_small_dictionaries_in_every_unit_against_numpy(5, unit)
        test_small_dictionaries_in_every_unit_against_numpy(0, "s")
        test_a_dictionary_of_70000_values_extended_with_id_begin()
        for width, offset in ((4, None), (8, 1), (4, 7), (8, None)):
            test_the_row_pass_at_every_length(width, offset)
        for have, want in (("D", "s"), ("s", "D"), ("s", "ns"), ("ms", "D")):
            test_rescale_against_numpys_cast(have, want)
        _big.clear()
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
        _big.clear()
        _big.update(saved)


# ---- 3. whole queries through the planner, every batch split ----------------------------------------------------------------------------
SPLITS = (1, 700, 2500)
_main = {}


def _main_table():
    from tests.golden import datetime_cases as C
    if "t" not in _main:
        _main["t"] = C.datetime_null_table()
    return _main["t"]


def _execute(query, t, batch):
    from vinum_amd import planner, set_batch_size
    set_batch_size(batch)
    try:
        return planner.execute(query, t)
    finally:
        set_batch_size(1 << 24)


def _every_split(query, t=None):
    """the query's result, identical (as a table: schema, order, NULLs) under every batch split"""
    t = _main_table() if t is None else t
    results = [_execute(query, t, b) for b in SPLITS]
    for b, r in zip(SPLITS[1:], results[1:]):
        assert r.schema == results[0].schema and r.equals(results[0]), f"batches of {b} rows differ from batches of {SPLITS[0]}"
    return results[0]


def _q(select, **kw):
    from tests.golden import datetime_cases as C
    return C._case("q", select, **kw)


def _fn(name, *x):
    return ["fn", name] + list(x)


def _lit(s):
    return ["lit", s]


def _host(unit, strings):
    """np.array(strings, dtype='datetime64[unit]') as the Arrow array the planner returns: NaT ('' / NaT / None) is NULL"""
    from tests.golden import datetime_cases as C
    return C.parsed_on_host(strings, unit)


def test_select_list_over_a_string_and_a_dictionary_typed_column():
    t = _main_table()
    got = _every_split(_q(["k", _fn("date", "d"), _fn("datetime", "d"), _fn("datetime", "d", _lit("ms")), _fn("date", "dd"), _fn("from_timestamp", "d", _lit("us"))],
                          aliases=[None, "a", "b", "c", "e", "f"]))
    d, dd = t["d"].to_pylist(), t["dd"].to_pylist()
    assert got.schema.types == [pa.int64(), pa.date32(), pa.timestamp("s"), pa.timestamp("ms"), pa.date32(), pa.timestamp("us")]
    assert got["k"].equals(t["k"])
    for name, unit, src in (("a", "D", d), ("b", "s", d), ("c", "ms", d), ("e", "D", dd), ("f", "us", d)):
        assert got[name].combine_chunks().equals(_host(unit, src)), name
    assert got["a"].null_count == sum(1 for s in d if s in (None, "", "NaT")) > 100


def test_where_against_a_constant_and_between():
    t = _main_table()
    day = np.array([np.datetime64("NaT") if s in (None, "", "NaT") else np.datetime64(s[:10], "D") for s in t["d"].to_pylist()])
    k = np.arange(t.num_rows)
    got = _every_split(_q(["k"], where=[">=", _fn("date", "d"), _fn("date", _lit("2020-10-09"))]))
    assert got["k"].to_pylist() == k[day >= np.datetime64("2020-10-09")].tolist()              # (NaT >= x is False: NULL rows go)
    got = _every_split(_q(["k"], where=["between", _fn("date", "d"), _fn("date", _lit("2020-10-06")), _fn("date", _lit("2020-10-09"))]))
    assert got["k"].to_pylist() == k[(day >= np.datetime64("2020-10-06")) & (day <= np.datetime64("2020-10-09"))].tolist()
    # a timestamp[s] node against a D constant and a date32 node against an s constant: aligned to seconds, as NumPy does
    sec = _host("s", t["d"].to_pylist()).to_numpy(zero_copy_only=False)
    got = _every_split(_q(["k"], where=["<", _fn("datetime", "d"), _fn("date", _lit("2020-10-09"))]))
    assert got["k"].to_pylist() == k[sec < np.datetime64("2020-10-09", "D")].tolist()
    got = _every_split(_q(["k"], where=[">", _fn("date", "d"), _fn("datetime", _lit("2020-10-08 12:00:00"), _lit("s"))]))
    assert got["k"].to_pylist() == k[day > np.datetime64("2020-10-08T12:00:00", "s")].tolist()


def test_is_null_and_is_not_null():
    t = _main_table()
    null = np.array([s in (None, "", "NaT") for s in t["d"].to_pylist()])
    got = _every_split(_q(["k"], where=["is_null", _fn("date", "d")]))
    assert got["k"].to_pylist() == np.nonzero(null)[0].tolist()
    got = _every_split(_q(["k"], where=["is_not_null", _fn("datetime", "d")]))
    assert got["k"].to_pylist() == np.nonzero(~null)[0].tolist()


def _groups(table, key, value):
    return dict(zip(table[key].to_pylist(), table[value].to_pylist()))


def test_group_by_distinct_and_aggregates():
    t = _main_table()
    day = _host("D", t["d"].to_pylist())
    want = pa.table({"day": day}).group_by("day").aggregate([([], "count_all")])
    got = _every_split(_q([_fn("date", "d"), _fn("count_star")], group_by=[_fn("date", "d")], aliases=["day", "n"], order_by=[_fn("date", "d")]))
    assert got.schema.field("day").type == pa.date32()
    assert _groups(got, "day", "n") == _groups(want, "day", "count_all") and got.num_rows == want.num_rows
    got = _every_split(_q([_fn("date", "d")], distinct=True, aliases=["day"], order_by=[_fn("date", "d")]))
    assert sorted(got["day"].to_pylist(), key=str) == sorted(set(day.to_pylist()), key=str)
    got = _every_split(_q([_fn("min", _fn("date", "d")), _fn("max", _fn("datetime", "d")), _fn("count", _fn("date", "d"))], aliases=["lo", "hi", "n"]))
    sec = _host("s", t["d"].to_pylist())
    assert got["lo"].to_pylist() == [pc.min(day).as_py()] and got["hi"].to_pylist() == [pc.max(sec).as_py()]
    assert got["n"].to_pylist() == [len(day) - day.null_count]
    assert got.schema.field("lo").type == pa.date32() and got.schema.field("hi").type == pa.timestamp("s")


def test_order_by_datetime():
    t = _main_table()
    sec = _host("s", t["d"].to_pylist())
    valid = sec.is_valid().to_numpy(zero_copy_only=False)
    got = _every_split(_q(["k"], where=["is_not_null", _fn("datetime", "d")], order_by=[_fn("datetime", "d"), "k"]))
    v = sec.cast(pa.int64()).to_numpy(zero_copy_only=False)
    order = [int(i) for i in np.lexsort((np.arange(len(v)), np.where(valid, v, 0))) if valid[i]]
    assert got["k"].to_pylist() == order
    got = _every_split(_q(["k"], where=["is_not_null", _fn("datetime", "d")], order_by=[_fn("datetime", "d"), "k"], sort_order=["DESC", "ASC"]))
    assert got["k"].to_pylist() == [int(i) for i in np.lexsort((np.arange(len(v)), -np.where(valid, v, 0))) if valid[i]]


def test_to_str_of_date_and_date_of_concat():
    t = _main_table()
    d = t["d"].to_pylist()
    got = _every_split(_q(["k", _fn("to_str", _fn("date", "d"))], aliases=[None, "s"]))
    assert got["s"].to_pylist() == ["None" if s in (None, "", "NaT") else s[:10] for s in d]       # (to_str()'s rule: a NULL row is "None")
    got = _every_split(_q(["k", _fn("date", ["concat", "ym", _lit("-01")])], aliases=[None, "first"]))
    assert got["first"].combine_chunks().equals(_host("D", [s + "-01" for s in t["ym"].to_pylist()]))
    got = _every_split(_q(["k", _fn("datetime", _fn("upper", "d"), _lit("ns"))], aliases=[None, "x"]))           # ('nat' -> 'NAT', ' ' / 'T' stay)
    assert got["x"].combine_chunks().equals(_host("ns", d))


def test_from_timestamp_over_integers_with_nulls_and_date_of_a_timestamp():
    t = _main_table()
    got = _every_split(_q(["k", _fn("from_timestamp", "i32"), _fn("from_timestamp", "i64", _lit("ms")), _fn("date", "ts"), _fn("datetime", "ts", _lit("s")),
                          _fn("datetime", "day", _lit("us")), _fn("datetime", "ts", _lit("ms"))], aliases=[None, "a", "b", "c", "e", "f", "g"]))
    assert got["a"].combine_chunks().equals(t["i32"].combine_chunks().cast(pa.int64()).view(pa.timestamp("s")))
    assert got["b"].combine_chunks().equals(t["i64"].combine_chunks().view(pa.timestamp("ms")))
    ms = t["ts"].combine_chunks().cast(pa.int64())
    null = ~ms.is_valid().to_numpy(zero_copy_only=False)
    raw = ms.fill_null(0).to_numpy(zero_copy_only=False)
    assert got["c"].combine_chunks().equals(pa.array((raw // 86_400_000).astype(np.int32), pa.date32(), mask=null))         # (the floor, before 1970 too)
    assert got["e"].combine_chunks().equals(pa.array(raw // 1000, pa.timestamp("s"), mask=null)) and (raw < 0).any()
    assert got["f"].combine_chunks().equals(t["day"].combine_chunks().cast(pa.timestamp("us")))
    assert got["g"].combine_chunks().equals(t["ts"].combine_chunks())                                               # (already the target: the column itself)
    got = _every_split(_q(["k"], where=["<", "ts", _fn("date", _lit("1970-01-01"))]))
    assert got["k"].to_pylist() == np.nonzero(~null & (raw < 0))[0].tolist()


def test_a_refused_value_raises_naming_it():
    t = _main_table()
    bad = t.set_column(t.schema.get_field_index("d"), "d", pa.array(["2020-10-08 03:26:54"] * 2000 + ["2020-10-08 25:00:00"] + ["2020-10-08 03:26:55"] * 499))
    for batch in SPLITS:
        with pytest.raises(ValueError, match='Error parsing datetime string "2020-10-08 25:00:00"'):
            _execute(_q(["k", _fn("date", "d")], aliases=[None, "a"]), bad, batch)
        with pytest.raises(ValueError, match='Error parsing datetime string "2020-10-08 25:00:00"'):
            # (the predicate over the node sees every row of the batch, the one it would reject included)
            _execute(_q(["k"], where=["<", _fn("datetime", "d"), _fn("date", _lit("2000-01-01"))]), bad, batch)
        # a row an EARLIER filter removed never reaches the function, as in the reference (its filter runs before its projection too):
        # the value sits in the dictionary, marked refused, and is nobody's error
        got = _execute(_q(["k", _fn("date", "d")], where=["<", "k", 10], aliases=[None, "a"]), bad, batch)
        assert got["a"].to_pylist() == [np.datetime64("2020-10-08").item()] * 10
    with pytest.raises(NotImplementedError, match="temporal constant"):
        _execute(_q(["k", _fn("date", _lit("2020-10-06"))], aliases=[None, "a"]), t, 2500)
    # concat() is never NULL: a NULL operand is "None", and a ROW that holds that image is refused as NumPy refuses the text -- while
    # the image every concat() dictionary holds, with no row behind it, is nobody's error (test_to_str_of_date_and_date_of_concat)
    ym = pa.table({"k": pa.array([0, 1, 2]), "ym": pa.array(["2020-10", None, "2020-11"], pa.large_string())})
    with pytest.raises(ValueError, match='Error parsing datetime string "None-01"'):
        _execute(_q(["k", _fn("date", ["concat", "ym", _lit("-01")])], aliases=[None, "a"]), ym, 2500)
    got = _execute(_q(["k", _fn("date", ["concat", "ym", _lit("-01")])], where=["is_not_null", "ym"], aliases=[None, "a"]), ym, 2500)
    assert got["a"].to_pylist() == [np.datetime64("2020-10-01").item(), np.datetime64("2020-11-01").item()]


def test_each_distinct_value_is_parsed_once_over_a_stream_of_batches():
    from vinum_amd import planner, set_batch_size
    t = _main_table()
    set_batch_size(700)
    try:
        plan = planner.plan_query(_q(["k", _fn("date", "d"), _fn("datetime", "d")], aliases=[None, "a", "b"]), t)
        plan.execute()
    finally:
        set_batch_size(1 << 24)
    op = plan.root
    while getattr(op, "_dicts", None) is None:
        op = op._parent_operator
    kd = op._dicts["d"]
    assert sorted(kd._parsed) == ["D", "s"] and kd.parse_launches <= 2 * 4
    assert kd._parsed["D"].values.covered == kd._id_count() and kd.parse_ids_parsed == 2 * kd._id_count()


# ---- 4. the golden cases of the reference's own planner -------------------------------------------------------------------------------------
def _cases():
    from tests.golden import datetime_cases as C
    return C.CASES


def _meta():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datetime_cases.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    from tests import util
    from tests.golden import datetime_cases as C
    meta = _meta()
    assert not meta["raised"] and sorted(meta["cases"]) == sorted(c["name"] for c in C.CASES)
    t = C.TABLES[case["table"]]()
    if case["table"] == "main":
        assert t.equals(util.read_ipc("datetime_in_main.arrow"))
    want = util.read_ipc(f"datetime_{case['name']}.arrow")
    assert meta["cases"][case["name"]]["rows"] == want.num_rows and meta["cases"][case["name"]]["types"] == [str(x) for x in want.schema.types]
    got = _every_split(case, t)
    assert got.schema.names == want.schema.names and got.num_rows == want.num_rows
    for name in want.schema.names:
        g, w = got[name].combine_chunks(), want[name].combine_chunks()
        assert g.type == w.type and g.equals(w), name
