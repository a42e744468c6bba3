"""KeyDictionary: the running dictionary of one non-numeric column (value -> int32 code) and the device tables derived from it,
one entry per dictionary id: LIKE matches, translations into and joint ranks with another dictionary, upper() / lower() maps,
concat() with literals, the parsed values of date() / datetime(); the pair tables of concat() over two columns; and the value tables
of to_str() over a numeric or temporal column (ValueTable: no KeyDictionary of its own, the column's VALUE is the key).
Importable without the shared library, like vinum_lib (which re-exports KeyDictionary and device_value_type)."""
import collections
import ctypes
from dataclasses import dataclass

import numpy as np
import pyarrow as pa

from . import _lib as L


def _is_string_like(t) -> bool:
    return pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t)


def device_value_type(t):
    """The type of the values the DEVICE dictionary holds for a column of type `t`: `t` itself for utf8 / large_utf8 / binary /
    large_binary, the value type of a dictionary<intN, one of those four>; None for every other type (the host route)."""
    if _is_string_like(t):
        return t
    if pa.types.is_dictionary(t) and _is_string_like(t.value_type):
        return t.value_type
    return None


class _IdTable:
    """A device table with one entry of `itemsize` bytes per dictionary id.  Entries [0, covered) are filled; the table grows by
    doubling and keeps them.  Its owner fills [covered, top) and advances `covered` -- when, is the owner's rule."""

    def __init__(self, top: int, itemsize: int):
        from .device import DeviceBuffer
        self.cap, self.covered, self.itemsize = max(top, 1), 0, itemsize
        self.buf = DeviceBuffer(self.cap * itemsize)

    def reserve(self, top: int) -> None:
        from .device import DeviceBuffer
        if top <= self.cap:
            return
        self.cap = max(top, 2 * self.cap)
        grown = DeviceBuffer(self.cap * self.itemsize)
        if self.covered:
            L.check(L.lib().vnm_memcpy_d2d(grown.ptr, self.buf.ptr, self.covered * self.itemsize, None))
        self.buf = grown

    def column(self, arrow_type):
        from .device import DeviceColumn
        return DeviceColumn(self.buf, None, 0, self.covered, arrow_type)


@dataclass
class _Translation:               # KeyDictionary._translate[id(other)]
    ref: object                   # weak reference to `other`
    table: _IdTable               # int32: code here -> code in `other`, -2 where it holds none
    mine: int = -1                # own / other's value count at the last call
    theirs: int = -1


@dataclass
class _JointRanks:                # KeyDictionary._joint[id(other)]
    ref: object                   # weak reference to `other`
    stamp: tuple                  # (own, other's value count) the tables were built at
    mine: object                  # DeviceBuffers of int32 ranks: own / other's table ...
    theirs: object
    ids: tuple                    # ... and their lengths, (own, other's id count)


@dataclass
class _CaseMap:                   # KeyDictionary._mapped["upper" | "lower"]
    derived: "KeyDictionary"
    table: _IdTable               # int32: code here -> code in `derived`, -2 for an id never handed out
    mine: int = -1                # own value count when the table last advanced


@dataclass
class _Affix:                     # KeyDictionary._affixed[(prefix, suffix)]
    derived: "KeyDictionary"
    table: _IdTable               # int32: code here -> code in `derived`, -2 for an id never handed out
    null_code: int = -2           # `derived`'s code of prefix + "None" + suffix, what a NULL row gets
    mine: int = -1                # own value count when the table last advanced


@dataclass
class _Parsed:                    # KeyDictionary._parsed[unit]
    values: _IdTable              # int64: code here -> days / unit counts since 1970-01-01
    status: _IdTable              # uint8: 0 a value, 1 NULL ('' / NaT), 2 refused or an id never handed out
    mine: int = -1                # own value count when the tables last advanced
    any_refused: bool = False     # a value handed out was refused: the row pass looks for rows that hold one (and reads that back)
    value_tables: dict = None     # where to_str(date(c))'s table lives from batch to batch (DeviceColumn.value_tables)


TEMPORAL_UNITS = ("D", "s", "ms", "us", "ns")             # enum vnm_temporal_unit, in its order
UNITS_PER_DAY = {"D": 1, "s": 86_400, "ms": 86_400_000, "us": 86_400_000_000, "ns": 86_400_000_000_000}


def temporal_type(unit: str):
    """the Arrow type of a date() / datetime() / from_timestamp() result in `unit`: date32 for D, timestamp[unit] otherwise"""
    return pa.date32() if unit == "D" else pa.timestamp(unit)


def temporal_unit(t):
    """the unit of a date32 / timestamp type (a zone-aware one too: the stored value is the UTC instant); None for any other type"""
    if pa.types.is_date32(t):
        return "D"
    return t.unit if pa.types.is_timestamp(t) else None


def rescaled_column(col, unit: str):
    """date(ts) / datetime(temporal column, unit): `col` -- date32 or timestamp -- in `unit` (vnm_temporal_rescale: to a coarser
    unit the FLOOR of the division, to a finer one the wrapping product NumPy's cast gives), with `col`'s validity; `col` itself
    when the unit is its own"""
    from .device import DeviceBuffer, DeviceColumn
    have = temporal_unit(col.arrow_type)
    if have is None:
        raise TypeError(f"not a date32 / timestamp column: {col.arrow_type}")
    if have == unit and not (pa.types.is_timestamp(col.arrow_type) and col.arrow_type.tz):
        return col
    a, b = UNITS_PER_DAY[have], UNITS_PER_DAY[unit]
    mul, div = (b // a, 1) if b >= a else (1, a // b)
    n, width = col.length, 4 if unit == "D" else 8
    off = col.offset if col._validity is not None else 0          # (one Arrow offset serves values and bitmap)
    out = DeviceBuffer(max(off + n, 1) * width)
    if n:
        d = col.dcol()
        L.check(L.lib().vnm_temporal_rescale(ctypes.byref(d), mul, div, n, width, out.ptr + off * width, None))
    return DeviceColumn(out, col._validity, off, n, temporal_type(unit), keep=(col,))


def timestamp_column(col, unit: str):
    """from_timestamp(integer column[, unit]) (TimestampFunction, functions.py:131-137): the same values as timestamp[unit], exact,
    with `col`'s validity -- an int64 column retyped over its own buffers, a narrower one widened (vnm_temporal_rescale, 1 / 1)"""
    from .device import DeviceBuffer, DeviceColumn
    t = pa.timestamp(unit)
    if pa.types.is_int64(col.arrow_type):
        return DeviceColumn(col._values, col._validity, col.offset, col.length, t, keep=(col,))
    n = col.length
    off = col.offset if col._validity is not None else 0
    out = DeviceBuffer(max(off + n, 1) * 8)
    if n:
        d = col.dcol()
        L.check(L.lib().vnm_temporal_rescale(ctypes.byref(d), 1, 1, n, 8, out.ptr + off * 8, None))
    return DeviceColumn(out, col._validity, off, n, t, keep=(col,))


def duration_unit(t):
    """the unit of a duration type; None for any other type"""
    return t.unit if pa.types.is_duration(t) else None


def affine_column(a, ka: int, b, kb: int, c: int, arrow_type):
    """Arithmetic on temporal values (vnm_temporal_affine): a * ka + b * kb + c per row, exact and wrapping in int64, as a column of
    `arrow_type` -- date32 (4 bytes), timestamp[u] or duration[u] (8) -- WITH the kernel's validity: NULL where an operand is NULL
    or NaT, or the result is NaT.  `a` (and `b`, which may be None) are date32 / timestamp / duration columns."""
    from .device import DeviceBuffer, DeviceColumn
    n = a.length
    if b is not None and b.length != n:
        raise ValueError(f"temporal arithmetic over operands of {n} and {b.length} rows")
    for k in (ka, kb, c):
        if not -2**63 <= k < 2**63:
            raise OverflowError(f"the factor or constant {k} of a temporal expression does not fit int64")
    width = 4 if pa.types.is_date32(arrow_type) else 8
    out, bitmap = DeviceBuffer(max(n, 1) * width), DeviceBuffer((n + 7) // 8 or 1)
    if n:
        da, db = a.dcol(), b.dcol() if b is not None else None
        L.check(L.lib().vnm_temporal_affine(ctypes.byref(da), ka, ctypes.byref(db) if db is not None else None, kb, c, n, width, out.ptr,
                                            bitmap.ptr, None, None))
    return DeviceColumn(out, bitmap, 0, n, arrow_type, keep=(a, b))


MAX_HOLIDAYS = 8192                      # what fits 32 KB of LDS (vnm_temporal_busday)
_DEFAULT_WEEKMASK = "1111100"
_CALENDAR_CACHE_SIZE = 32
_calendars = collections.OrderedDict()   # the NORMALISED calendar (bits, the days' bytes) -> (bits, days, device buffer or None), least recently used first
_spellings = {}                          # (weekmask, holidays) as written -> the normalised key: no np.busdaycalendar per batch


def busday_calendar(weekmask=None, holidays=()):
    """is_busday()'s weekmask (either of NumPy's spellings) and holidays (date strings) normalised by np.busdaycalendar itself: (the 7
    bits as an int, bit 0 Monday; the holidays as a sorted, distinct int32 array of days without NaT and non-business days).  More
    than MAX_HOLIDAYS of them raise ValueError."""
    cal = np.busdaycalendar(_DEFAULT_WEEKMASK if weekmask is None else weekmask, list(holidays))
    bits = sum(1 << k for k, on in enumerate(cal.weekmask) if on)
    days = cal.holidays.astype("datetime64[D]").astype(np.int64).astype(np.int32)
    if len(days) > MAX_HOLIDAYS:
        raise ValueError(f"is_busday() takes at most {MAX_HOLIDAYS} holidays (32 KB of LDS), not {len(days)}")
    return bits, days


def busday_key(weekmask=None, holidays=()):
    """the normalised calendar as a hashable key, (bits, the sorted days' bytes): two spellings of one calendar share it, two
    calendars never do"""
    spelt = (weekmask, tuple(holidays))
    if spelt not in _spellings:
        bits, days = busday_calendar(weekmask, holidays)
        if len(_spellings) >= 8 * _CALENDAR_CACHE_SIZE:
            _spellings.clear()
        _spellings[spelt] = (bits, days.tobytes())
    return _spellings[spelt]


def busday_mask(col, weekmask=None, holidays=()):
    """np.is_busday(col, weekmask, holidays) over a date32 column as a uint8 mask column (vnm_temporal_busday): 0 for a NULL row.  The
    holiday list is uploaded once per normalised calendar and kept in a small LRU (an evicted list goes back to the pool once the
    masks that hold it are gone)."""
    from .device import DeviceBuffer, DeviceColumn
    if not pa.types.is_date32(col.arrow_type):
        raise TypeError(f"is_busday() takes a date32 column, not {col.arrow_type}: write is_busday(date(x))")
    key = busday_key(weekmask, holidays)
    if key in _calendars:
        _calendars.move_to_end(key)
    else:
        days = np.frombuffer(key[1], np.int32)
        _calendars[key] = (key[0], days, DeviceBuffer.from_host(days) if len(days) else None)
        while len(_calendars) > _CALENDAR_CACHE_SIZE:
            _calendars.popitem(last=False)
    bits, days, dev = _calendars[key]
    n = col.length
    out = DeviceBuffer(max(n, 1))
    if n:
        d = col.dcol()
        L.check(L.lib().vnm_temporal_busday(ctypes.byref(d), n, bits, dev.ptr if dev is not None else None, len(days), out.ptr, None))
    return DeviceColumn(out, None, 0, n, pa.uint8(), keep=(col, dev))


def floordiv_column(a, ka: int, b, kb: int):
    """duration // duration (vnm_temporal_floordiv): floor((a * ka) / (b * kb)) per row as an int64 column WITH validity -- NULL where
    an operand is NULL or NaT; a zero divisor gives 0 as in NumPy.  a or b may be None: that side is the constant ka / kb itself."""
    from .device import DeviceBuffer, DeviceColumn
    n = (a if a is not None else b).length
    if a is not None and b is not None and b.length != n:
        raise ValueError(f"temporal arithmetic over operands of {n} and {b.length} rows")
    for k in (ka, kb):
        if not -2**63 <= k < 2**63:
            raise OverflowError(f"the factor or constant {k} of a temporal expression does not fit int64")
    out, bitmap = DeviceBuffer(max(n, 1) * 8), DeviceBuffer((n + 7) // 8 or 1)
    if n:
        da, db = a.dcol() if a is not None else None, b.dcol() if b is not None else None
        L.check(L.lib().vnm_temporal_floordiv(ctypes.byref(da) if da is not None else None, ka, ctypes.byref(db) if db is not None else None, kb, n,
                                              out.ptr, bitmap.ptr, None, None))
    return DeviceColumn(out, bitmap, 0, n, pa.int64(), keep=(a, b))


def temporal_operand_kind(fn: str, t, name) -> str:
    """How date() / datetime() / from_timestamp() (`fn`) takes a column `name` of Arrow type `t`: "parse" (a string column, through
    its dictionary), "rescale" (date32 / timestamp: a change of unit) or "retype" (an integer column under from_timestamp).  A
    binary, float, uint64, decimal ... column raises TypeError naming it, a column whose dictionary stays on the host (bool,
    date64, a dictionary type over numbers) NotImplementedError -- the texts upper() / to_str() use."""
    takes = "a string, date32, timestamp or integer column" if fn == "from_timestamp" else "a string, date32 or timestamp column"
    dt = device_value_type(t)
    if dt is not None:
        if pa.types.is_binary(dt) or pa.types.is_large_binary(dt):
            raise TypeError(f"{fn}() takes {takes}, {name!r} is {t}")
        return "parse"
    if temporal_unit(t) is not None:
        return "rescale"
    if fn == "from_timestamp" and pa.types.is_integer(t) and not pa.types.is_uint64(t):
        return "retype"
    if pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_decimal(t) or pa.types.is_temporal(t):
        raise TypeError(f"{fn}() takes {takes}, {name!r} is {t}")
    raise NotImplementedError(f"no GPU lowering for {fn}() over the {t} column {name!r}: only string columns keep their dictionaries on the device")


class PairTable:
    """The device pair table (vnm_strpair) of concat(a, sep, b) over two dictionaries and the dictionary derived from them:
    (code_a, code_b) -> code in `derived`, alive across batches so a pair keeps its code.  `pair_launches`, `pairs_concatenated`
    (= the distinct pairs seen: string bytes are touched once per pair, never per row), `rehashes`, `slots`, `occupied` and
    `half_written` (occupied slots without a code: 0 after every call) are read from the device object (stats())."""

    def __init__(self, prefix: bytes, sep: bytes, suffix: bytes):
        self.prefix, self.sep, self.suffix = prefix, sep, suffix
        self.derived = KeyDictionary(pa.string())
        self.ref = None           # weak reference to the right operand's dictionary (KeyDictionary._paired)
        self._h = L.lib().vnm_strpair_create(prefix, len(prefix), suffix, len(suffix))
        if not self._h:
            raise RuntimeError(L.last_error())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().vnm_strpair_destroy(h)
            except Exception:
                pass

    def stats(self) -> dict:
        out = (ctypes.c_int64 * 6)()
        L.check(L.lib().vnm_strpair_stats(self._h, out, None))
        return dict(zip(("pair_launches", "pairs_concatenated", "rehashes", "slots", "occupied", "half_written"), (int(v) for v in out)))

    pair_launches = property(lambda self: self.stats()["pair_launches"])
    pairs_concatenated = property(lambda self: self.stats()["pairs_concatenated"])
    rehashes = property(lambda self: self.stats()["rehashes"])

    def column(self, da, db, col_a, col_b):
        """the codes of prefix + a + sep + b + suffix per row: an int32 DeviceColumn WITHOUT validity (concat() is never NULL), its
        `.dictionary` the derived dictionary"""
        from .device import DeviceBuffer, DeviceColumn
        n = col_a.length
        if col_b.length != n:
            raise ValueError(f"concat(): operands of {n} and {col_b.length} rows")
        out = DeviceBuffer(max(n, 1) * 4)
        a, b = col_a.dcol(), col_b.dcol()
        rc = L.lib().vnm_strpair_concat(self._h, da.handle(), db.handle(), self.derived.handle(), self.sep, len(self.sep), ctypes.byref(a),
                                        ctypes.byref(b), n, out.ptr, None)
        message = L.last_error() if rc != 0 else None
        if self.derived._h is not None and n:
            self.derived.absorb_new()
        if rc != 0:
            raise L.VinumHipError(message)
        return DeviceColumn(out, None, 0, n, pa.int32(), keep=(self,), dictionary=self.derived)


TOSTR_INT, TOSTR_UINT, TOSTR_DATE32, TOSTR_TIMESTAMP_S, TOSTR_TIMESTAMP_MS, TOSTR_TIMESTAMP_US, TOSTR_TIMESTAMP_NS = range(7)     # enum vnm_tostr_kind


def to_str_kind(t, name=None):
    """The vnm_tostr_kind of a column of Arrow type `t` under to_str() (StringCastFunction, functions.py:189-193): the integers,
    date32 and the four timestamp units (a zone-aware one prints its UTC instant, the stored value, as the reference does).
    Everything else raises TypeError naming the column and its type: floats (shortest round-trip digits are a piece of work of
    their own), decimal, date64, time32 / time64, duration, boolean and binary."""
    T = pa.types
    if T.is_signed_integer(t):
        return TOSTR_INT
    if T.is_unsigned_integer(t):
        return TOSTR_UINT
    if T.is_date32(t):
        return TOSTR_DATE32
    if T.is_timestamp(t):
        return {"s": TOSTR_TIMESTAMP_S, "ms": TOSTR_TIMESTAMP_MS, "us": TOSTR_TIMESTAMP_US, "ns": TOSTR_TIMESTAMP_NS}[t.unit]
    raise TypeError(f"to_str() takes an integer, date32, timestamp or string column, {name!r} is {t}" if name is not None else
                    f"to_str() takes an integer, date32, timestamp or string column, not {t}")


class ValueTable:
    """The device value table (vnm_strval) of to_str(v) over an integer, date32 or timestamp column and the dictionary derived from
    it: value -> code in `derived`, alive across batches so a value keeps its code and is formatted once.  `launches`,
    `values_formatted` (= the distinct values seen, NULL and the all-ones value included: string bytes are written once per value,
    never per row), `rehashes`, `slots`, `occupied` and `half_written` (occupied slots without a code: 0 after every call) are read
    from the device object (stats())."""

    def __init__(self, kind: int):
        self.kind = kind
        self.derived = KeyDictionary(pa.string())
        self._h = L.lib().vnm_strval_create(kind)
        if not self._h:
            raise RuntimeError(L.last_error())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().vnm_strval_destroy(h)
            except Exception:
                pass

    @staticmethod
    def of(col, name=None) -> "ValueTable":
        """the table of column `col`: the one hanging in its scan's per-name registry (DeviceColumn.value_tables), made on first
        use; a column built by hand gets a table for this call only"""
        kind = to_str_kind(col.arrow_type, name)
        tables = col.value_tables if col.value_tables is not None else {}
        key = (kind, col.vnm_type)
        if key not in tables:
            tables[key] = ValueTable(kind)
        return tables[key]

    def stats(self) -> dict:
        out = (ctypes.c_int64 * 6)()
        L.check(L.lib().vnm_strval_stats(self._h, out, None))
        return dict(zip(("launches", "values_formatted", "rehashes", "slots", "occupied", "half_written"), (int(v) for v in out)))

    launches = property(lambda self: self.stats()["launches"])
    values_formatted = property(lambda self: self.stats()["values_formatted"])
    rehashes = property(lambda self: self.stats()["rehashes"])

    def column(self, col):
        """the codes of to_str(col) per row: an int32 DeviceColumn WITHOUT validity (a NULL row is "None"), its `.dictionary` the
        derived dictionary"""
        from .device import DeviceBuffer, DeviceColumn
        n = col.length
        out = DeviceBuffer(max(n, 1) * 4)
        v = col.dcol()
        rc = L.lib().vnm_strval_to_str(self._h, self.derived.handle(), ctypes.byref(v), n, out.ptr, None)
        message = L.last_error() if rc != 0 else None
        if self.derived._h is not None and n:
            self.derived.absorb_new()
        if rc != 0:
            raise L.VinumHipError(message)
        return DeviceColumn(out, None, 0, n, pa.int32(), keep=(self, col), dictionary=self.derived)


class KeyDictionary:
    """Running dictionary of one non-numeric group-by column: value -> int32 code.

    The reference keys its generic map on arrow::Scalar vectors (generic_hash_aggregate.h:10-45): hash + Equals per row.
    Here every batch is encoded once on ingest and the GPU groups by 4-byte codes with the numeric machinery (NULL stays
    NULL: its own group, as in the reference where a NULL scalar equals a NULL scalar).

    utf8 / large_utf8 / binary / large_binary columns are encoded ON THE DEVICE (`vnm_strdict_encode`, csrc/vnm_strdict.hip:
    offsets and bytes cross PCIe once, one kernel hashes every row and finds or inserts it in the dictionary table; only the
    values a batch ADDS come back, and this object keeps them to decode the result's key column).  Other types (bool, decimal,
    date64 ...: a handful of values or fixed width) keep the host route: Arrow's `dictionary_encode` + a NumPy merge.

    A DICTIONARY-TYPED column -- dictionary<intN, utf8 | large_utf8 | binary | large_binary> -- takes the device route too
    (DESIGN.md 4.9c): the batch dictionary's VALUES go through vnm_strdict_encode, the indices through vnm_strdict_remap_indices
    (encode_to_device).  `type` stays the column's type and is what decode() returns (decoded to the value type, then cast);
    everything that reasons about the VALUES -- LIKE's utf8 rule, literals, the offsets' width -- uses `value_type`.  A
    dictionary type over any other value type (numbers, decimals, nested) keeps the host route.

    The derived device tables (like_table, translate_table, joint_rank_tables, mapped) are cached here.  The ID count
    (`_id_count()`) sizes a table and moves by whole chunks on every encode; the VALUE count (`_n_values`) moves only when a
    value is new, and only that is work.  Each method states its rule; DESIGN.md 4.9 has all four side by side."""

    def __init__(self, arrow_type: pa.DataType):
        self.type = arrow_type
        self.values = pa.array([], type=arrow_type)     # host route: the dictionary in order of first appearance
        dev_type = device_value_type(arrow_type)
        self._device = dev_type is not None
        self.value_type = dev_type if dev_type is not None else arrow_type    # what the device dictionary's values are
        self._dict_typed = self._device and pa.types.is_dictionary(arrow_type)
        self._batch_dict = None    # dictionary-typed input: the previous batch's dictionary (kept alive: its addresses are compared) ...
        self._batch_table, self._batch_table_nulls = None, False   # ... its codes in HBM (DeviceBuffer of int32, -1 = a NULL value); is any NULL
        self.values_encodes = self.remap_launches = 0    # batch dictionaries encoded (a repeated one is not), vnm_strdict_remap_indices calls
        self._h = None
        self._chunks = []          # device route: the values each batch added ...
        self._pos = None           # ... and id -> position in their concatenation (-1: an id never handed out)
        self._n_values = 0
        self._by_code_cache = None  # ((id count, chunk count), values_by_code() at that stamp)
        self._like = {}            # LIKE pattern -> _IdTable of uint8 (like_table)
        self.like_launches = self.like_ids_matched = 0       # vnm_strdict_like calls and the ids they matched, over every pattern
        self._translate = {}       # id(other dictionary) -> _Translation
        self._joint = {}           # id(other dictionary) -> _JointRanks
        self._mapped = {}          # "upper" | "lower" -> _CaseMap
        self.map_launches = self.map_ids_mapped = 0          # vnm_strdict_map_codepoints calls and the ids they mapped, over both functions
        self.translate_builds = self.joint_rank_builds = 0   # vnm_strdict_translate / vnm_strdict_ranks_joint calls this dictionary made
        self._affixed = {}         # (prefix, suffix) -> _Affix
        self.affix_launches = self.affix_ids_mapped = 0      # vnm_strdict_concat_affix calls and the ids they covered, over every (prefix, suffix)
        self._paired = {}          # (id(other dictionary), prefix, sep, suffix) -> PairTable
        self._parsed = {}          # unit -> _Parsed
        self.parse_launches = self.parse_ids_parsed = 0      # vnm_strdict_parse_datetime calls and the ids they covered, over every unit

    @property
    def on_device(self) -> bool:
        """True for the four string / binary types and the dictionary types over them, whose dictionary lives in HBM
        (vnm_strdict); the host-route dictionaries (bool, decimal, date64 ...) have no device tables"""
        return self._device

    @property
    def _wide(self) -> bool:
        return pa.types.is_large_string(self.value_type) or pa.types.is_large_binary(self.value_type)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().vnm_strdict_destroy(h)
            except Exception:
                pass

    def handle(self):
        """the device dictionary (vnm_strdict*) behind a utf8 / binary column, created on first use"""
        if self._h is None:
            self._h = L.lib().vnm_strdict_create()
            if not self._h:
                raise RuntimeError(L.last_error())
        return self._h

    def _id_count(self) -> int:
        return int(L.lib().vnm_strdict_ids(self._h)) if self._h is not None else 0

    def _values_in_order(self) -> pa.Array:
        """the device route's values in order of first appearance: what `_pos` indexes"""
        return pa.concat_arrays(self._chunks) if self._chunks else pa.array([], type=self.value_type)

    def absorb_new(self):
        """after an encode through this dictionary's handle (vnm_strdict_encode here, vnm_csv_parse_block_ex in io.py): fetch the values
        it added -- the host copy of the dictionary is the concatenation of these"""
        lib = L.lib()
        n_new, new_bytes = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(lib.vnm_strdict_last_new(self._h, ctypes.byref(n_new), ctypes.byref(new_bytes)))
        n = n_new.value
        if not n:
            return
        ids, lens, data = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(max(new_bytes.value, 1), np.uint8)
        L.check(lib.vnm_strdict_fetch_new(self._h, ids.ctypes.data, lens.ctypes.data, data.ctypes.data))
        offs = np.zeros(n + 1, np.int64 if self._wide else np.int32)
        np.cumsum(lens, out=offs[1:])
        self._chunks.append(pa.Array.from_buffers(self.value_type, n, [None, pa.py_buffer(offs), pa.py_buffer(data[:new_bytes.value])]))
        top, old = self._id_count(), self._pos if self._pos is not None else np.zeros(0, np.int64)
        if len(old) < top:
            self._pos = np.full(max(top, 2 * len(old)), -1, np.int64)
            self._pos[:len(old)] = old
        self._pos[ids] = self._n_values + np.arange(n, dtype=np.int64)
        self._n_values += n

    def _encode_values(self, column: pa.Array):
        """a utf8 / binary array of the value type through vnm_strdict_encode: its codes as a NumPy int32 array, -1 for NULL"""
        n = len(column)
        vbuf, obuf, dbuf = column.buffers()
        codes = np.empty(max(n, 1), np.int32)
        L.check(L.lib().vnm_strdict_encode(self.handle(), obuf.address if obuf is not None else None, 1 if self._wide else 0,
                                           dbuf.address if dbuf is not None and dbuf.size else None,
                                           vbuf.address if (vbuf is not None and column.null_count) else None,
                                           column.offset, n, codes.ctypes.data, None, None, None))
        self.absorb_new()
        return codes[:n]

    @staticmethod
    def _same_buffers(a: pa.Array, b: pa.Array) -> bool:
        """two arrays over the very same memory (type, offset, length, every buffer's address and size)"""
        if a is b:
            return True
        if a.type != b.type or len(a) != len(b) or a.offset != b.offset:
            return False
        ba, bb = a.buffers(), b.buffers()
        return len(ba) == len(bb) and all((x is None) == (y is None) and (x is None or (x.address == y.address and x.size == y.size))
                                          for x, y in zip(ba, bb))

    def encode_to_device(self, column, stage=None):
        """A DICTIONARY-TYPED column -> the DeviceColumn of its running codes, without a host copy of the codes (None for any
        other input: the caller encodes on the host route of encode()).  (1) The batch dictionary's values through the device
        encode, skipped when they are the previous batch's buffers: int32 codes, -1 for a NULL value -- the table; (2) the index
        buffer staged at its native width (`stage`: array -> DeviceColumn, default DeviceColumn.from_arrow; io sources pass the
        pinned ring); (3) vnm_strdict_remap_indices: codes = table[index], -1 and a cleared validity bit for a NULL row or a NULL
        value; an index outside the batch dictionary raises "dictionary index out of bounds"."""
        from .device import DeviceBuffer, DeviceColumn
        if not self._dict_typed:
            return None
        if isinstance(column, pa.ChunkedArray):
            column = column.combine_chunks() if column.num_chunks != 1 else column.chunk(0)
        if not isinstance(column, pa.DictionaryArray):
            return None
        n = len(column)
        if n == 0:
            return DeviceColumn(DeviceBuffer(0), None, 0, 0, pa.int32(), dictionary=self)
        values = column.dictionary
        if values.type != self.value_type:
            values = values.cast(self.value_type)
        if self._batch_dict is None or not self._same_buffers(values, self._batch_dict):
            table = self._encode_values(values) if len(values) else np.zeros(0, np.int32)
            self.values_encodes += 1
            self._batch_dict, self._batch_table = values, DeviceBuffer.from_host(table)
            self._batch_table_nulls = bool((table < 0).any())
        idx = column.indices                           # (the column's validity, offset and length with the integer type)
        icol = stage(idx) if stage is not None else DeviceColumn.from_arrow(idx)
        d = icol.dcol()
        codes = DeviceBuffer(n * 4)
        validity = DeviceBuffer((n + 7) >> 3) if (idx.null_count or self._batch_table_nulls) else None
        bad = ctypes.c_int64(0)
        L.check(L.lib().vnm_strdict_remap_indices(ctypes.byref(d), self._batch_table.ptr, len(values), codes.ptr,
                                                 validity.ptr if validity is not None else None, ctypes.byref(bad), None))
        self.remap_launches += 1
        return DeviceColumn(codes, validity, 0, n, pa.int32(), dictionary=self)

    def encode(self, column) -> pa.Array:
        import pyarrow.compute as pc
        if isinstance(column, pa.ChunkedArray):
            column = column.combine_chunks()
        if self._dict_typed and not len(column):
            return pa.array([], type=pa.int32())
        if self._dict_typed:
            dev = self.encode_to_device(column)
            if dev is None:
                raise TypeError(f"KeyDictionary({self.type}).encode: a {column.type} column")
            codes = dev.to_numpy()
            return pa.array(codes, type=pa.int32(), mask=(codes < 0) if dev.validity_ptr else None)
        if self._device and len(column):
            codes = self._encode_values(column)
            return pa.array(codes, type=pa.int32(), mask=(codes < 0) if column.null_count else None)
        enc = column.dictionary_encode()
        local = enc.dictionary
        pos = pc.index_in(local, value_set=self.values) if len(self.values) else pa.nulls(len(local), pa.int32())
        known = pos.is_valid().to_numpy(zero_copy_only=False)
        mapping = pos.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int32)
        n_new = int((~known).sum())
        if n_new:
            mapping[~known] = len(self.values) + np.arange(n_new, dtype=np.int32)
            fresh = local.filter(pa.array(~known))
            self.values = pa.concat_arrays([self.values, fresh]) if len(self.values) else fresh
        idx = enc.indices
        codes = mapping[idx.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int64)] if len(local) else np.zeros(len(idx), np.int32)
        mask = ~idx.is_valid().to_numpy(zero_copy_only=False) if idx.null_count else None
        return pa.array(codes, type=pa.int32(), mask=mask)

    def code_of(self, value):
        """The code of `value` in this dictionary, or None (predicates on a dictionary-coded column: `city = 'Berlin'` is a
        comparison of int32 codes in HBM)."""
        import pyarrow.compute as pc
        vals = self.values_by_code()
        if not len(vals):
            return None
        i = pc.index(vals, pa.scalar(value, type=self.value_type)).as_py()
        return None if i < 0 else int(i)

    def rank_bounds(self, value):
        """(number of dictionary values < value, 1 if value is in the dictionary else 0): with r = rank_column's rank of a row,
        v < value <=> r < less, v <= value <=> r < less + present, v > value <=> r >= less + present, v >= value <=> r >= less
        (byte-wise order, as Arrow compares utf8 / binary)."""
        import pyarrow.compute as pc
        vals = self.values_by_code()
        if not len(vals):
            return 0, 0
        lit = pa.scalar(value, type=self.value_type)
        less = int(pc.sum(pc.less(vals, lit)).as_py() or 0)
        return less, 0 if self.code_of(value) is None else 1

    @staticmethod
    def _gather(codes_col, table_ptr, keep, dictionary=None):
        """table[code] per row (vnm_strdict_codes_to_ranks): a fresh int32 DeviceColumn with the codes' validity; `keep` owns the table"""
        from .device import DeviceBuffer, DeviceColumn
        n = codes_col.length
        off = codes_col.offset if codes_col._validity is not None else 0      # (one Arrow offset serves values and bitmap)
        out = DeviceBuffer(max(off + n, 1) * 4)
        if n:
            L.check(L.lib().vnm_strdict_codes_to_ranks(codes_col.values_ptr + codes_col.offset * 4, table_ptr, n, out.ptr + off * 4, None))
        return DeviceColumn(out, codes_col._validity, off, n, pa.int32(), keep=(keep, codes_col), dictionary=dictionary)

    def _device_ranks(self):
        """DeviceBuffer of int32: id -> rank of its value in byte-wise order, as Arrow's SortIndices compares (an id never handed out: unspecified)"""
        from .device import DeviceBuffer
        rank_of = DeviceBuffer(max(self._id_count(), 1) * 4)
        L.check(L.lib().vnm_strdict_ranks_device(self._h, rank_of.ptr, None))
        return rank_of

    def ranked_values(self):
        """A device-route dictionary's (rank of id: host int32, one entry per id, unspecified for an id never handed out; the
        values in rank order).  A dictionary without values launches nothing and ranks its ids 0."""
        values, top = self._values_in_order(), self._id_count()
        if not len(values):
            return np.zeros(max(top, 1), np.int32), values
        rank_of_id = self._device_ranks().to_host(np.int32, top)
        live = np.nonzero(self._pos[:top] >= 0)[0]
        by_rank = np.empty(len(values), np.int64)
        by_rank[rank_of_id[live]] = self._pos[live]             # rank -> position in `values`
        return rank_of_id, values.take(pa.array(by_rank))

    def rank_column(self, codes_col):
        """ORDER BY a dictionary-coded column: the rows' order-preserving RANKS as an int32 DeviceColumn (NULL stays NULL).  utf8 /
        binary dictionaries are ranked on the device (_device_ranks), the small host-route ones (decimals, date64 ...) by Arrow."""
        from .device import DeviceBuffer
        if self._device and self._h is not None:
            rank_of = self._device_ranks()
        else:
            import pyarrow.compute as pc
            order = pc.sort_indices(self.values).to_numpy(zero_copy_only=False) if len(self.values) else np.zeros(0, np.int64)
            r = np.zeros(max(len(self.values), 1), np.int32)
            r[order] = np.arange(len(order), dtype=np.int32)
            rank_of = DeviceBuffer.from_host(r)
        return self._gather(codes_col, rank_of.ptr, rank_of)

    def like_table(self, pattern: str):
        """`column LIKE pattern` for every value of this dictionary: a device uint8 DeviceColumn, entry = 1 when the value with
        that code matches (vnm_strdict_like: the reference's regex restated, functions.py:301-344; trailing NULs dropped for utf8,
        whose values reach the reference as a NumPy 'U' array).  Its length is the number of ids handed out so far.  Cached per
        pattern: a call matches only the ids handed out since the last one, so a stream matches each distinct value once per pattern."""
        from . import ops
        t = self.value_type                                              # (a dictionary-typed column: what its values are)
        if not (pa.types.is_string(t) or pa.types.is_large_string(t)):
            raise TypeError(f"LIKE needs a string column, not {self.type}")    # (the reference's re.match raises on bytes / numbers)
        ops.like_tokens(pattern)                                         # (NotImplementedError for a regex metacharacter)
        top = self._id_count()
        table = self._like.get(pattern)
        if table is None:
            table = self._like[pattern] = _IdTable(top, 1)
        if top > table.covered:
            table.reserve(top)
            raw = pattern.encode("utf-8")
            L.check(L.lib().vnm_strdict_like(self._h, raw, len(raw), L.LIKE_STRIP_NUL if pa.types.is_string(t) else 0, table.covered,
                                             table.buf.ptr, None))
            self.like_launches += 1
            self.like_ids_matched += top - table.covered
            table.covered = top
        return table.column(pa.uint8())

    def _pair_check(self, other, what):
        if not (self._device and getattr(other, "on_device", False)):
            raise NotImplementedError(f"no GPU lowering for {what} of a {self.value_type} and a {getattr(other, 'value_type', other.type)} dictionary: the device "
                                      "dictionaries are the string and binary types")

    @staticmethod
    def _pair_ref(cache, other, key=None):
        """A weak reference to `other` that drops `other`'s entry (and its device tables) from `cache` when `other` dies."""
        import weakref
        key = id(other) if key is None else key

        def drop(ref):
            entry = cache.get(key)
            if entry is not None and entry.ref is ref:
                del cache[key]
        return weakref.ref(other, drop)

    def translate_table(self, other):
        """This dictionary's codes in terms of `other`'s: an int32 DeviceColumn with one entry per id handed out here, the code
        `other` holds for the same BYTES, or -2 where it holds none (vnm_strdict_translate; bytes compared exactly, whatever mix
        of utf8 / large_utf8 / binary / large_binary the two are).  `a = b` over two dictionary-coded columns then is
        code_a == table[code_b].  Cached per pair; work only when a dictionary GREW by values: while `other` has not, only the ids
        handed out here since are looked up; once it has, an absent value may be present now and the whole table is built again."""
        self._pair_check(other, "a translation")
        top = self._id_count()
        entry = self._translate.get(id(other))
        if entry is None or entry.ref() is not other:
            entry = self._translate[id(other)] = _Translation(self._pair_ref(self._translate, other), _IdTable(top, 4))
        table = entry.table
        if entry.theirs != other._n_values:
            table.covered = 0
        if (table.covered == 0 or entry.mine != self._n_values) and top > table.covered:
            table.reserve(top)
            L.check(L.lib().vnm_strdict_translate(self.handle(), other.handle(), table.covered, table.buf.ptr, None))
            self.translate_builds += 1
            table.covered = top
        entry.mine, entry.theirs = self._n_values, other._n_values
        return table.column(pa.int32())

    def joint_rank_tables(self, other):
        """(own table, other's table): int32 DeviceColumns, one entry per id, the dense rank of the value in the ascending byte
        order of the UNION of both dictionaries (vnm_strdict_ranks_joint: the order of rank_column; equal bytes share a rank), so
        `a < b` over two dictionary-coded columns is table_a[code_a] < table_b[code_b].  Cached per pair and rebuilt in full when
        either grows (by values, as translate_table)."""
        from .device import DeviceBuffer, DeviceColumn
        self._pair_check(other, "joint ranks")
        lib = L.lib()
        stamp = (self._n_values, other._n_values)
        entry = self._joint.get(id(other))
        if entry is None or entry.ref() is not other or entry.stamp != stamp:
            ids = (self._id_count(), other._id_count())
            mine, theirs = (DeviceBuffer(max(n, 1) * 4) for n in ids)
            for buf in (mine, theirs):
                L.check(lib.vnm_memset(buf.ptr, 0xFF, buf.nbytes))           # (ids never handed out: -1, no row holds them)
            L.check(lib.vnm_strdict_ranks_joint(self.handle(), other.handle(), mine.ptr, theirs.ptr, None))
            self.joint_rank_builds += 1
            entry = self._joint[id(other)] = _JointRanks(self._pair_ref(self._joint, other), stamp, mine, theirs, ids)
        return (DeviceColumn(entry.mine, None, 0, entry.ids[0], pa.int32()), DeviceColumn(entry.theirs, None, 0, entry.ids[1], pa.int32()))

    def mapped(self, fn: str):
        """upper() / lower() of this dictionary (`fn`: "upper" | "lower"; pc.utf8_upper / pc.utf8_lower, functions.py:279-298):
        (the DERIVED dictionary, an int32 DeviceColumn `code here -> code there`, one entry per id handed out here; -2 for an id
        never handed out).  The function depends on the value alone, so each distinct value is mapped ONCE, on the device
        (vnm_strdict_map_codepoints with the code point table of vinum_amd.strcase), and found or inserted in the derived
        dictionary; a row then costs one lookup of its code (mapped_column).  One derived dictionary per (dictionary, function),
        the same object for the life of this one, extended with the ids handed out since the last call; a batch that brought no
        new value launches nothing (`map_launches`, `map_ids_mapped`).  It is a full KeyDictionary of type string, whatever this
        one's is (the reference casts first, functions.py:219-221), and absorbs its new values: it decodes, ranks, matches LIKE,
        pairs and maps again.  A binary dictionary raises TypeError (Arrow has no such kernel), a host-route one
        NotImplementedError, a structurally malformed UTF-8 value ValueError("Invalid UTF8 sequence in input") from every call
        that has to map it -- whether or not a row holding it survives the query's filter."""
        from . import strcase
        if fn not in strcase.CASE_FNS:
            raise ValueError(f"no case map {fn!r}: one of {strcase.CASE_FNS}")
        if not self._device:
            raise NotImplementedError(f"no GPU lowering for {fn}() over a {self.type} column: only string columns keep their dictionaries on the device")
        t = self.value_type
        if not (pa.types.is_string(t) or pa.types.is_large_string(t)):
            raise TypeError(f"{fn}() needs a string column, not {self.type}")      # (pc.utf8_upper has no kernel for binary)
        top = self._id_count()
        entry = self._mapped.get(fn)
        if entry is None:
            entry = self._mapped[fn] = _CaseMap(KeyDictionary(pa.string()), _IdTable(top, 4))
        derived, table = entry.derived, entry.table
        if top > table.covered and entry.mine != self._n_values:       # (by values, as translate_table: only a new value is work)
            table.reserve(top)
            map_from, map_to = strcase.case_table(fn)
            invalid = ctypes.c_int64(0)
            rc = L.lib().vnm_strdict_map_codepoints(self.handle(), derived.handle(), map_from.ctypes.data, map_to.ctypes.data, len(map_from),
                                                    table.covered, table.buf.ptr, ctypes.byref(invalid), None)
            self.map_launches += 1
            self.map_ids_mapped += top - table.covered
            message = L.last_error() if rc != 0 else None
            if derived._h is not None:
                derived.absorb_new()        # (also after a malformed value: the well-formed ones are in the derived dictionary)
            if rc != 0:                     # (nothing is recorded as covered: the next call maps these ids, and raises, again)
                raise ValueError("Invalid UTF8 sequence in input") if invalid.value else L.VinumHipError(message)
            table.covered, entry.mine = top, self._n_values
        return derived, table.column(pa.int32())

    def mapped_column(self, fn: str, codes_col):
        """upper(column) / lower(column) over a column of THIS dictionary's codes: the derived dictionary's codes, table[code] per
        row (NULL stays NULL), with `.dictionary` the derived dictionary, so every operator takes it as the string column it is."""
        derived, table = self.mapped(fn)
        return self._gather(codes_col, table.values_ptr, table, dictionary=derived)

    def _concat_check(self):
        if not self._device:
            raise NotImplementedError(f"no GPU lowering for concat() over a {self.type} column: only string columns keep their dictionaries on the device")
        t = self.value_type
        if not (pa.types.is_string(t) or pa.types.is_large_string(t)):
            raise TypeError(f"concat() needs a string column, not {self.type}")

    def affixed(self, prefix: bytes, suffix: bytes):
        """concat(prefix, c, suffix) of this dictionary (ConcatFunction, functions.py:250-276; either literal may be empty): (the
        DERIVED dictionary, an int32 DeviceColumn `code here -> code there`, the derived code a NULL row gets).  A function of the
        value alone, so each distinct value is written ONCE on the device -- prefix + the value without trailing NULs + suffix,
        vnm_strdict_concat_affix -- and found or inserted in the derived dictionary; NULL is the value "None".  One derived
        dictionary per (dictionary, prefix, suffix), the same object for the life of this one, extended only when this one gained
        a value (`affix_launches`, `affix_ids_mapped`).  Refusals as mapped(): binary TypeError, host route NotImplementedError."""
        self._concat_check()
        top = self._id_count()
        entry = self._affixed.get((prefix, suffix))
        if entry is None:
            entry = self._affixed[(prefix, suffix)] = _Affix(KeyDictionary(pa.string()), _IdTable(top, 4))
        derived, table = entry.derived, entry.table
        if entry.null_code < 0 or (top > table.covered and entry.mine != self._n_values):
            table.reserve(top)
            null_code = ctypes.c_int32(-2)
            rc = L.lib().vnm_strdict_concat_affix(self.handle(), derived.handle(), prefix, len(prefix), suffix, len(suffix), table.covered,
                                                  table.buf.ptr, ctypes.byref(null_code), None)
            self.affix_launches += 1
            self.affix_ids_mapped += top - table.covered
            message = L.last_error() if rc != 0 else None
            if derived._h is not None:
                derived.absorb_new()
            if rc != 0:
                raise L.VinumHipError(message)
            table.covered, entry.mine, entry.null_code = top, self._n_values, int(null_code.value)
        return derived, table.column(pa.int32()), entry.null_code

    def affixed_column(self, prefix: bytes, suffix: bytes, codes_col):
        """concat(prefix, column, suffix) over a column of THIS dictionary's codes: table[code] per row, the NULL image's code where
        the row is NULL (by validity bit or code -1); no validity -- concat() is never NULL -- and `.dictionary` the derived one."""
        from .device import DeviceBuffer, DeviceColumn
        derived, table, null_code = self.affixed(prefix, suffix)
        n = codes_col.length
        out = DeviceBuffer(max(n, 1) * 4)
        if n:
            L.check(L.lib().vnm_strdict_gather_codes(codes_col.values_ptr + codes_col.offset * 4, codes_col.validity_ptr, codes_col.offset,
                                                     table.values_ptr, table.length, n, null_code, out.ptr, None))
        return DeviceColumn(out, None, 0, n, pa.int32(), keep=(table, codes_col), dictionary=derived)

    def parsed(self, unit: str):
        """date() / datetime() of this dictionary in `unit` (DateFunction / DatetimeFunction, functions.py:25-128: np.array(x,
        dtype='datetime64[unit]')): (an int64 DeviceColumn `code here -> days / unit counts since 1970-01-01`, a uint8 DeviceColumn
        `code here -> 0 a value | 1 NULL | 2 refused or never handed out`), one entry per id covered.  A function of the value
        alone, so each distinct value is parsed ONCE on the device (vnm_strdict_parse_datetime, the grammar in csrc/vnm_dtparse.hpp);
        a row then costs one lookup of its code (parsed_column).  Cached per unit and extended only when this dictionary gained a
        value (`parse_launches`, `parse_ids_parsed`).  A value the parser refuses is DATA here -- status 2 --: whether a row holds it
        is parsed_column's to say (a dictionary derived by concat() always holds the image of NULL, "None...", and a batch
        dictionary may hold values no row uses).  Refusals as mapped(): binary TypeError, host route NotImplementedError."""
        if unit not in TEMPORAL_UNITS:
            raise ValueError(f"no temporal unit {unit!r}: one of {TEMPORAL_UNITS}")
        if not self._device:
            raise NotImplementedError(f"no GPU lowering for date() / datetime() over a {self.type} column: only string columns keep their dictionaries on the device")
        t = self.value_type
        if not (pa.types.is_string(t) or pa.types.is_large_string(t)):
            raise TypeError(f"date() / datetime() need a string column, not {self.type}")
        top = self._id_count()
        entry = self._parsed.get(unit)
        if entry is None:
            entry = self._parsed[unit] = _Parsed(_IdTable(top, 8), _IdTable(top, 1))
        values, status = entry.values, entry.status
        if top > values.covered and entry.mine != self._n_values:       # (by values, as mapped(): only a new value is work)
            values.reserve(top)
            status.reserve(top)
            refused = ctypes.c_int64(-1)
            L.check(L.lib().vnm_strdict_parse_datetime(self.handle(), TEMPORAL_UNITS.index(unit), values.covered, values.buf.ptr, status.buf.ptr,
                                                       ctypes.byref(refused), None))
            self.parse_launches += 1
            self.parse_ids_parsed += top - values.covered
            entry.any_refused = entry.any_refused or refused.value >= 0
            values.covered = status.covered = top
            entry.mine = self._n_values
        return values.column(pa.int64()), status.column(pa.uint8())

    def parsed_column(self, unit: str, codes_col):
        """date(column) / datetime(column, unit) over a column of THIS dictionary's codes: a date32 / timestamp[unit] DeviceColumn
        WITH validity and without a dictionary -- table[code] per row (vnm_strdict_gather_temporal), NULL where the row is NULL or
        its value is '' / NaT.  A non-NULL row that holds a value the parser refuses raises ValueError('Error parsing datetime string
        "<value>"') -- NumPy's words -- naming the value of the lowest such id, when its batch comes through here: a predicate over
        the node sees every row, the ones it would reject included; a row an EARLIER filter removed never gets here, as in the
        reference.  Only a dictionary that holds a refused value pays the read-back for it."""
        from .device import DeviceBuffer, DeviceColumn
        values, status = self.parsed(unit)
        refused = ctypes.c_int64(-1) if self._parsed[unit].any_refused else None
        n, width = codes_col.length, 4 if unit == "D" else 8
        out, bitmap = DeviceBuffer(max(n, 1) * width), DeviceBuffer(max((n + 7) >> 3, 1))
        if n:
            L.check(L.lib().vnm_strdict_gather_temporal(codes_col.values_ptr + codes_col.offset * 4, codes_col.validity_ptr, codes_col.offset,
                                                        values.values_ptr, status.values_ptr, values.length, n, width, out.ptr, bitmap.ptr, None,
                                                        ctypes.byref(refused) if refused is not None else None, None))
        if refused is not None and refused.value >= 0:
            raise ValueError(f'Error parsing datetime string "{self.values_by_code()[refused.value].as_py()}"')
        col = DeviceColumn(out, bitmap, 0, n, temporal_type(unit), keep=(values, status, codes_col))
        entry = self._parsed[unit]
        if entry.value_tables is None:
            entry.value_tables = {}
        col.value_tables = entry.value_tables
        return col

    def paired(self, other, prefix: bytes, sep: bytes, suffix: bytes) -> PairTable:
        """The pair table of concat(prefix, a, sep, b, suffix) with this dictionary on the left and `other` on the right (which may
        be this one): one per (pair of dictionaries, literals), kept here as long as both live."""
        self._concat_check()
        if not isinstance(other, KeyDictionary):
            raise NotImplementedError(f"no GPU lowering for concat() with a {type(other).__name__} dictionary")
        other._concat_check()
        key = (id(other), prefix, sep, suffix)
        entry = self._paired.get(key)
        if entry is None or entry.ref() is not other:
            entry = self._paired[key] = PairTable(prefix, sep, suffix)
            entry.ref = self._pair_ref(self._paired, other, key)
        return entry

    def pair_column(self, other, prefix: bytes, sep: bytes, suffix: bytes, col_a, col_b):
        """concat(prefix, a, sep, b, suffix) per row over columns of this dictionary's and `other`'s codes (PairTable.column)"""
        return self.paired(other, prefix, sep, suffix).column(self, other, col_a, col_b)

    @property
    def pair_tables(self):
        """the PairTables with this dictionary on the left (their counters: pair_launches, pairs_concatenated, rehashes)"""
        return list(self._paired.values())

    def values_by_code(self) -> pa.Array:
        """The dictionary as an array indexed by CODE (a code the device never handed out: NULL) -- what the ranks exchange to build
        one dictionary before partial groups keyed by these codes can travel (distributed.union_dictionary)."""
        if self._device and self._h is not None:
            # (cached until the dictionary grows: a predicate asks once per batch and literal, the concat + take is O(distinct values))
            stamp = (self._id_count(), len(self._chunks))
            if self._by_code_cache is None or self._by_code_cache[0] != stamp:
                pos = self._pos[:stamp[0]] if self._pos is not None else np.zeros(0, np.int64)
                out = self._values_in_order().take(pa.array(np.where(pos < 0, 0, pos), type=pa.int64(), mask=(pos < 0) if (pos < 0).any() else None))
                self._by_code_cache = (stamp, out)
            return self._by_code_cache[1]
        return self.values

    def decode(self, codes: pa.Array) -> pa.Array:
        """codes -> values of the column's type.  A dictionary-typed column comes back with ITS type (value type, index type,
        `ordered`): decoded to the value type, then cast; more distinct values than the index type numbers surface Arrow's cast error."""
        if self._device and (self._h is not None or self._pos is not None):
            c = codes.fill_null(0).to_numpy(zero_copy_only=False).astype(np.int64)
            pos = self._pos[c] if self._pos is not None and len(c) else np.zeros(len(c), np.int64)
            null = ~codes.is_valid().to_numpy(zero_copy_only=False) if codes.null_count else np.zeros(len(c), bool)
            if ((pos < 0) & ~null).any():
                raise RuntimeError("KeyDictionary.decode: a code that was never handed out (internal error)")
            values = self._values_in_order().take(pa.array(np.where(null, 0, pos), type=pa.int64(), mask=null if null.any() else None))
        else:
            values = self.values.take(codes)
        return values.cast(self.type) if self._dict_typed else values
