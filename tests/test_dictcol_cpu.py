"""Dictionary-typed columns (dictionary<intN, utf8 | large_utf8 | binary | large_binary>) without a GPU: which types take the
device route, that the VALUE type reaches the rules about "the type", that decode() returns the declared type, and that the
lowerings give the trees a plain utf8 column gives."""
import numpy as np
import pyarrow as pa
import pytest

from vinum_amd.core.base import DeviceRecordBatch
from vinum_amd.core.lowering import lower_dictionary
from vinum_amd.vinum_lib import KeyDictionary, device_value_type

STRINGS = (pa.string(), pa.large_string(), pa.binary(), pa.large_binary())
INDICES = (pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64())


# ---- 1. the type rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_type", STRINGS, ids=str)
@pytest.mark.parametrize("index_type", INDICES, ids=str)
def test_dictionary_types_over_strings_take_the_device_route(index_type, value_type):
    for ordered in (False, True):
        t = pa.dictionary(index_type, value_type, ordered)
        kd = KeyDictionary(t)
        assert kd.on_device
        assert kd.type == t and kd.value_type == value_type and device_value_type(t) == value_type


@pytest.mark.parametrize("value_type", STRINGS, ids=str)
def test_plain_string_types_are_their_own_value_type(value_type):
    kd = KeyDictionary(value_type)
    assert kd.on_device and kd.value_type == value_type and kd.type == value_type
    assert kd.encode_to_device(pa.array([], value_type)) is None          # (only dictionary-typed input is remapped on the device)


@pytest.mark.parametrize("value_type", [pa.int64(), pa.float64(), pa.decimal128(10, 2), pa.bool_(), pa.date64(), pa.list_(pa.string())], ids=str)
def test_dictionary_types_over_other_values_keep_the_host_route(value_type):
    t = pa.dictionary(pa.int32(), value_type)
    assert device_value_type(t) is None and device_value_type(value_type) is None
    if pa.types.is_primitive(value_type) and not pa.types.is_temporal(value_type):    # (the types Arrow builds an empty dictionary array of)
        kd = KeyDictionary(t)
        assert not kd.on_device and kd.value_type == t and kd.encode_to_device(pa.array([], t)) is None


def test_a_dictionary_of_int64_still_encodes_and_decodes_on_the_host_as_before():
    t = pa.dictionary(pa.int32(), pa.int64())
    kd = KeyDictionary(t)
    a = pa.array([7, 9, None, 7, 11], pa.int64()).dictionary_encode()
    b = pa.array([11, 5, 7], pa.int64()).dictionary_encode()
    assert a.type == t
    ca, cb = kd.encode(a), kd.encode(b)
    assert ca.to_pylist() == [0, 1, None, 0, 2] and cb.to_pylist() == [2, 3, 0]      # running codes in order of first appearance
    assert kd.values_encodes == 0 and kd.remap_launches == 0
    out = kd.decode(ca)
    assert out.type == pa.int64() and out.to_pylist() == [7, 9, None, 7, 11]      # (the host route hands back the values' type)
    assert kd.decode(cb).to_pylist() == [11, 5, 7]


# ---- 2. the value type reaches the rules ----------------------------------------------------------------------------------------
def test_like_over_a_dictionary_of_binary_raises_the_utf8_type_error():
    kd = KeyDictionary(pa.dictionary(pa.int8(), pa.binary()))
    with pytest.raises(TypeError, match="LIKE needs a string column"):
        kd.like_table("a%")
    with pytest.raises(TypeError, match="LIKE needs a string column"):
        KeyDictionary(pa.dictionary(pa.int32(), pa.large_binary())).like_table("a%")


def test_like_over_a_dictionary_of_strings_gets_past_the_type_check(monkeypatch):
    """... and then needs the device: the library is the next thing it asks for"""
    from vinum_amd import _lib as L

    class NeedsTheDevice(Exception):
        pass

    def no_device():
        raise NeedsTheDevice()
    monkeypatch.setattr(L, "lib", no_device)
    for vt in (pa.string(), pa.large_string()):
        with pytest.raises(NeedsTheDevice):
            KeyDictionary(pa.dictionary(pa.int8(), vt)).like_table("a%")
    with pytest.raises(NotImplementedError):                      # (the pattern check sits between the two)
        KeyDictionary(pa.dictionary(pa.int8(), pa.string())).like_table("a[bc]%")


def _hand_filled(t):
    """a device-route dictionary as two encodes would have left it on the host: ids 0, 1, 3 handed out (2 never was)"""
    kd = KeyDictionary(t)
    vt = kd.value_type
    mk = (lambda xs: pa.array(xs, vt)) if pa.types.is_string(vt) or pa.types.is_large_string(vt) else (lambda xs: pa.array([x.encode() for x in xs], vt))
    kd._chunks = [mk(["bär", "apple"]), mk(["zebra"])]
    kd._pos = np.array([1, 0, -1, 2], np.int64)          # id -> position in the concatenation
    kd._n_values = 3
    return kd


@pytest.mark.parametrize("t", [pa.dictionary(pa.int8(), pa.string()), pa.dictionary(pa.int32(), pa.large_string(), True),
                               pa.dictionary(pa.uint16(), pa.binary()), pa.dictionary(pa.int64(), pa.large_binary())], ids=str)
def test_decode_returns_the_declared_dictionary_type(t):
    kd = _hand_filled(t)
    codes = pa.array([3, 0, None, 1, 0], pa.int32())
    out = kd.decode(codes)
    assert out.type == t and out.type.ordered == t.ordered
    want = ["zebra", "apple", None, "bär", "apple"]
    if pa.types.is_binary(t.value_type) or pa.types.is_large_binary(t.value_type):
        want = [None if w is None else w.encode() for w in want]
    assert out.cast(t.value_type).to_pylist() == want
    assert kd.decode(pa.array([], pa.int32())).type == t
    with pytest.raises(RuntimeError, match="never handed out"):
        kd.decode(pa.array([2], pa.int32()))


def test_decode_of_a_plain_string_dictionary_stays_plain():
    kd = _hand_filled(pa.string())
    assert kd.decode(pa.array([1, 3], pa.int32())).type == pa.string()


def test_more_distinct_values_than_the_index_type_numbers_surface_arrows_cast_error():
    kd = KeyDictionary(pa.dictionary(pa.int8(), pa.string()))
    kd._chunks = [pa.array([f"v{i}" for i in range(200)])]
    kd._pos = np.arange(200, dtype=np.int64)
    kd._n_values = 200
    assert len(kd.decode(pa.array(np.arange(100, dtype=np.int32)))) == 100
    with pytest.raises(pa.ArrowInvalid):
        kd.decode(pa.array(np.arange(200, dtype=np.int32)))


def test_literals_are_scalars_of_the_value_type():
    kd = _hand_filled(pa.dictionary(pa.int8(), pa.string()))
    kd.values_by_code = lambda: pa.array(["apple", "bär", None, "zebra"], pa.string())      # (what the device route builds by code)
    assert kd.code_of("zebra") == 3 and kd.code_of("nope") is None
    assert kd.rank_bounds("b") == (1, 0) and kd.rank_bounds("bär") == (1, 1)


# ---- 3. the lowerings: the same trees as over a utf8 column -----------------------------------------------------------------------
class FakeDict:
    """what the lowerings ask of a KeyDictionary (as tests/test_expr_cpu.py's)"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.on_device = name, arrow_type, on_device
        vt = device_value_type(arrow_type)
        if vt is not None:
            self.value_type = vt

    def translate_table(self, other):
        return f"<codes of {self.name} in {other.name}>"

    def joint_rank_tables(self, other):
        return f"<joint ranks of {self.name}>", f"<joint ranks of {other.name}>"

    def rank_column(self, col):
        return f"<ranks of {col.name}>"

    def like_table(self, pattern):
        return f"<like {pattern!r} in {self.name}>"

    def code_of(self, value):
        return {"m": 4, "Berlin": 3}.get(value)

    def rank_bounds(self, value):
        return 2, 1


class FakeColumn:
    vnm_type = 2          # L.I32
    length = 10

    def __init__(self, name, dictionary=None, arrow_type=pa.int32()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


def _batch(c_type, s_type):
    return DeviceRecordBatch({"c": FakeColumn("c", FakeDict("C", c_type)), "s": FakeColumn("s", FakeDict("S", s_type)),
                              "v": FakeColumn("v", None, pa.int64())}, 0)


TREES = [("like", "c", ("lit", "a%")), ("not_like", "c", ("lit", "_b%")), ("eq", "c", "s"), ("ne", "s", "c"), ("lt", "c", "s"),
         ("lt", "c", ("lit", "m")), ("ge", ("lit", "m"), "c"), ("eq", "c", ("lit", "Berlin")), ("in", "c", ("m", "Berlin", "x")),
         ("between", "c", "s", ("lit", "m")), ("and", ("like", "c", ("lit", "a%")), ("gt", "v", 3))]


@pytest.mark.parametrize("tree", TREES, ids=lambda t: f"{t[0]}_{t[1] if isinstance(t[1], str) else 'lit'}")
@pytest.mark.parametrize("c_type, s_type", [(pa.dictionary(pa.int8(), pa.string()), pa.string()),
                                            (pa.dictionary(pa.int32(), pa.large_string(), True), pa.dictionary(pa.int8(), pa.string())),
                                            (pa.dictionary(pa.uint8(), pa.string()), pa.large_string())], ids=["d8-utf8", "d32l-d8", "du8-lutf8"])
def test_lowering_over_dictionary_typed_columns_gives_the_utf8_trees(c_type, s_type, tree):
    want = lower_dictionary(tree, _batch(pa.string(), pa.string()).columns)
    got = lower_dictionary(tree, _batch(c_type, s_type).columns)
    assert got == want
    assert got[0] != tree                                  # (it did lower)


def test_refusals_name_the_value_type():
    cols = _batch(pa.dictionary(pa.int8(), pa.string()), pa.string()).columns
    with pytest.raises(TypeError, match="cannot compare the string column 'c' with 'v'"):
        lower_dictionary(("eq", "c", "v"), cols)
    with pytest.raises(TypeError, match=r"add\(\) over the string column 'c'"):
        lower_dictionary(("add", "c", 1), cols)
    host = DeviceRecordBatch({"c": FakeColumn("c", FakeDict("C", pa.dictionary(pa.int8(), pa.string()))),
                              "h": FakeColumn("h", FakeDict("H", pa.dictionary(pa.int32(), pa.int64()), on_device=False))}, 0).columns
    with pytest.raises(NotImplementedError, match="only string and binary columns keep their dictionaries on the device"):
        lower_dictionary(("eq", "c", "h"), host)


def test_the_adapter_lowers_a_string_literal_to_a_literal():
    """`c = 'x'` from the reference's planner: Literal('x') is not the column x"""
    from vinum_amd import binding as B
    assert B.lower(B.vectorize(("eq", "c", ("lit", "x")))) == ("eq", "c", ("lit", "x"))
    assert B.lower(B.vectorize(("lt", ("lit", b"m"), "c"))) == ("lt", ("lit", b"m"), "c")
    assert B.lower(B.vectorize(("in", "c", ("a", "b")))) == ("in", "c", ("a", "b"))
    assert B.lower(B.vectorize(("gt", "v", 3))) == ("gt", "v", 3)
