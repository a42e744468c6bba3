"""to_str() without a GPU: core.lowering.lower_case_functions over stub columns (the node becomes a derived column, nests with upper /
concat, is materialised once, is the empty affix over a string column), every refusal with its error type and the column's name,
planner._t / _case_by_type / output_names, the adapter's round trip with the mirror class and with a reference-shaped class built
by name, the exported symbols against the header's signatures, and the restatement the GPU tests compare with against NumPy itself.

On the parent commit P._t(["fn", "to_str", "v"]) stays the unknown function ("fn", "to_str", "v") and the lowering knows no such node."""
import ctypes
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import binding as B
from vinum_amd import planner as P
from vinum_amd.core import lowering
from vinum_amd.core.lowering import lower_case_functions, lower_dictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the lowering over stub columns -----------------------------------------------------------------------------------------------------
class StubDict:
    """what lower_case_functions asks of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.on_device = name, arrow_type, on_device
        self.value_type = arrow_type.value_type if pa.types.is_dictionary(arrow_type) else arrow_type       # (as KeyDictionary.value_type)
        self.calls = []

    def mapped_column(self, fn, col):
        self.calls.append((fn, col.name))
        return StubColumn(f"{fn}({col.name})", StubDict(f"{fn}({self.name})"))

    def affixed_column(self, prefix, suffix, col):
        self.calls.append(("affix", prefix, col.name, suffix))
        return StubColumn(f"[{prefix.decode()}{col.name}{suffix.decode()}]", StubDict(f"affix({self.name})"))

    def pair_column(self, other, prefix, sep, suffix, a, b):
        self.calls.append(("pair", prefix, a.name, sep, b.name, suffix))
        return StubColumn(f"[{prefix.decode()}{a.name}{sep.decode()}{b.name}{suffix.decode()}]", StubDict(f"pair({self.name},{other.name})"))

    def code_of(self, value):
        return {"7": 3}.get(value)


class StubColumn:
    length, value_tables, vnm_type = 10, None, 3

    def __init__(self, name, dictionary=None, arrow_type=pa.int32()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


class StubValueTable:
    """stands where keydict.ValueTable stands in the lowering: of() is asked once per materialised node"""
    calls = []

    @classmethod
    def of(cls, col, name=None):
        cls.calls.append((name, str(col.arrow_type)))
        return cls()

    def column(self, col):
        return StubColumn(f"str({col.name})", StubDict(f"values({col.name})"))


@pytest.fixture
def tables(monkeypatch):
    StubValueTable.calls = []
    monkeypatch.setattr(lowering, "ValueTable", StubValueTable)
    return StubValueTable


def _columns():
    num = lambda n, t: StubColumn(n, None, t)
    return {"a": StubColumn("a", StubDict("A")), "d": StubColumn("d", StubDict("D", pa.dictionary(pa.int8(), pa.string()))),
            "raw": StubColumn("raw", StubDict("R", pa.binary())), "flag": StubColumn("flag", StubDict("F", pa.bool_(), on_device=False)),
            "dec": StubColumn("dec", StubDict("M", pa.decimal128(10, 2), on_device=False)), "d64": StubColumn("d64", StubDict("E", pa.date64(), on_device=False)),
            "v": num("v", pa.int64()), "u": num("u", pa.uint8()), "day": num("day", pa.date32()), "ts": num("ts", pa.timestamp("us", tz="UTC")),
            "f": num("f", pa.float64()), "h": num("h", pa.float32()), "t32": num("t32", pa.time32("s")), "t64": num("t64", pa.time64("us")),
            "dur": num("dur", pa.duration("s"))}


def test_the_node_becomes_a_derived_column(tables):
    cols = _columns()
    e, extra = lower_case_functions(("to_str", "v"), cols)
    assert e == "__to_str_v" and list(extra) == [e] and extra[e].name == "str(v)" and extra[e].dictionary is not None
    assert tables.calls == [("v", "int64")]
    for name in ("u", "day", "ts"):
        e, extra = lower_case_functions(("to_str", name), cols)
        assert e == f"__to_str_{name}" and extra[e].name == f"str({name})"
    # to the later lowerings it is an ordinary string column: a literal becomes its code in the derived dictionary
    e, extra = lower_dictionary(("eq", ("to_str", "v"), ("lit", "7")), cols)
    assert e == ("eq", "__to_str_v", 3)
    e, extra = lower_dictionary(("eq", ("to_str", "v"), ("lit", "8")), cols)
    assert e == ("eq", "__to_str_v", -2)


def test_it_nests_with_upper_and_concat_in_any_order(tables):
    cols = _columns()
    e, extra = lower_case_functions(("upper", ("to_str", "v")), cols)
    assert e == "__upper___to_str_v" and extra["__to_str_v"].dictionary.calls == [("upper", "str(v)")]
    e, extra = lower_case_functions(("concat", "a", ("lit", "-"), ("to_str", "v")), cols)
    assert cols["a"].dictionary.calls == [("pair", b"", "a", b"-", "str(v)", b"")] and extra[e].name == "[a-str(v)]"
    e, extra = lower_case_functions(("to_str", ("concat", ("to_str", "day"), ("lit", "T"))), cols)
    inner = next(n for n in extra if n.startswith("__concat("))
    assert e == f"__to_str_{inner}" and extra[e].name == "[[str(day)T]]"               # to_str of a string node: the empty affix of it
    e, extra = lower_case_functions(("to_str", ("to_str", "u")), cols)
    assert e == "__to_str___to_str_u" and extra[e].name == "[str(u)]"


def test_a_repeated_node_is_materialised_once(tables):
    cols = _columns()
    extra = {}
    node = ("to_str", "v")
    e1, _ = lower_dictionary(("or", ("eq", node, ("lit", "7")), ("eq", node, ("lit", "nobody"))), cols, extra)
    e2, _ = lower_dictionary(("upper", node), cols, extra)
    e3, _ = lower_dictionary(("concat", node, ("lit", "!")), cols, extra)
    assert tables.calls == [("v", "int64")]
    assert e1 == ("or", ("eq", "__to_str_v", 3), ("eq", "__to_str_v", -2)) and e2 == "__upper___to_str_v"
    assert extra["__to_str_v"].dictionary.calls == [("upper", "str(v)"), ("affix", b"", "str(v)", b"!")] and extra[e3].name == "[str(v)!]"


def test_to_str_of_a_string_column_is_the_empty_affix(tables):
    cols = _columns()
    for name in ("a", "d"):                                                             # utf8 and dictionary-typed
        e, extra = lower_case_functions(("to_str", name), cols)
        assert e == f"__to_str_{name}" and cols[name].dictionary.calls == [("affix", b"", name, b"")] and extra[e].name == f"[{name}]"
    assert tables.calls == []


def test_every_refusal_raises_its_error_type_and_names_the_column(tables):
    cols = _columns()
    for name, t in (("f", "double"), ("h", "float"), ("t32", "time32\\[s\\]"), ("t64", "time64\\[us\\]"), ("dur", "duration\\[s\\]"),
                    ("raw", "binary"), ("flag", "bool"), ("dec", "decimal128\\(10, 2\\)"), ("d64", "date64")):
        with pytest.raises(TypeError, match=f"to_str\\(\\) takes an integer, date32, timestamp or string column, '{name}' is {t}"):
            lower_dictionary(("to_str", name), cols)
    assert tables.calls == []
    with pytest.raises(NotImplementedError, match="no GPU lowering for to_str\\(\\) over \\('mul', 'v', 2\\)"):
        lower_dictionary(("to_str", ("mul", "v", 2)), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for to_str\\(\\) over 7"):
        lower_dictionary(("to_str", 7), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for to_str\\(\\) over \\('lit', 'x'\\)"):
        lower_dictionary(("to_str", ("lit", "x")), cols)
    with pytest.raises(NotImplementedError, match="over 'nowhere'"):
        lower_dictionary(("to_str", "nowhere"), cols)
    with pytest.raises(NotImplementedError, match="with 2 operand"):
        lower_dictionary(("to_str", "v", "u"), cols)
    # unchanged: a BARE numeric column inside concat / upper stays refused, the explicit to_str() is the capability
    with pytest.raises(TypeError, match="concat\\(\\) needs a string column, 'v' is int64"):
        lower_dictionary(("concat", "a", "v"), cols)
    with pytest.raises(TypeError, match="upper\\(\\) needs a string column, 'v' is int64"):
        lower_dictionary(("upper", "v"), cols)


def test_the_kind_of_every_type():
    from vinum_amd import keydict as K
    kinds = {pa.int8(): K.TOSTR_INT, pa.int64(): K.TOSTR_INT, pa.uint8(): K.TOSTR_UINT, pa.uint64(): K.TOSTR_UINT, pa.date32(): K.TOSTR_DATE32,
             pa.timestamp("s"): K.TOSTR_TIMESTAMP_S, pa.timestamp("ms"): K.TOSTR_TIMESTAMP_MS, pa.timestamp("us", tz="Europe/Berlin"): K.TOSTR_TIMESTAMP_US,
             pa.timestamp("ns"): K.TOSTR_TIMESTAMP_NS}
    for t, kind in kinds.items():
        assert K.to_str_kind(t) == kind, t
    assert list(range(7)) == [K.TOSTR_INT, K.TOSTR_UINT, K.TOSTR_DATE32, K.TOSTR_TIMESTAMP_S, K.TOSTR_TIMESTAMP_MS, K.TOSTR_TIMESTAMP_US, K.TOSTR_TIMESTAMP_NS]
    text = open(os.path.join(ROOT, "include", "vinum_hip.h")).read()
    order = re.search(r"enum vnm_tostr_kind \{([^}]*)\}", text).group(1)
    assert [s.strip().split(" ")[0] for s in order.split(",")] == ["VNM_TOSTR_INT", "VNM_TOSTR_UINT", "VNM_TOSTR_DATE32", "VNM_TOSTR_TIMESTAMP_S",
                                                                  "VNM_TOSTR_TIMESTAMP_MS", "VNM_TOSTR_TIMESTAMP_US", "VNM_TOSTR_TIMESTAMP_NS"]
    for t in (pa.float16(), pa.float64(), pa.bool_(), pa.decimal128(5, 1), pa.date64(), pa.time32("ms"), pa.duration("ns"), pa.binary(), pa.string()):
        with pytest.raises(TypeError, match="to_str\\(\\) takes"):
            K.to_str_kind(t)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def test_the_planner_knows_the_function_and_names_the_column():
    assert P._t(["fn", "to_str", "v"]) == ("to_str", "v") and P._t(["fn", "TO_STR", "v"]) == ("to_str", "v")
    assert P._t(["concat", "a", ["lit", "-"], ["fn", "to_str", "v"]]) == ("concat", "a", ("lit", "-"), ("to_str", "v"))
    assert P.SCALAR_FN_NAMES["to_str"] == "to_str"
    assert P.output_names([("fn", "to_str", "v"), "k", ("fn", "to_str", "v")], [None, None, None]) == ["to_str", "k", "to_str_1"]
    t = pa.table({"v": pa.array([1]), "k": pa.array([1])})
    plan = P.plan_query({"select": [["fn", "to_str", "v"], ["fn", "count_star"]], "group_by": [["fn", "to_str", "v"]]}, t)
    assert ("project_inner", ((("to_str", "v"), "__inner_0"),)) in plan.steps
    assert any(s[0] == "aggregate" and s[1] == ("__inner_0",) for s in plan.steps)
    plan = P.plan_query({"select": ["k"], "order_by": [["fn", "to_str", "v"]]}, t)
    assert ("sort", ("__sort_0",), (0,)) in plan.steps


def test_the_plan_time_refusals():
    t = pa.table({"a": pa.array(["x"]), "v": pa.array([1]), "f": pa.array([1.5]), "h": pa.array([1.5], pa.float32()), "flag": pa.array([True]),
                  "dec": pa.array([1], pa.decimal128(5, 1)), "d64": pa.array([0], pa.date64()), "t": pa.array([0], pa.time32("s")),
                  "dur": pa.array([0], pa.duration("s")), "raw": pa.array([b"x"]), "day": pa.array([0], pa.date32()), "ts": pa.array([0], pa.timestamp("ns")),
                  "d": pa.array(["x"]).dictionary_encode()})
    for col in ("f", "h", "flag", "dec", "d64", "t", "dur", "raw"):
        with pytest.raises(TypeError, match=f"to_str\\(\\) takes an integer, date32, timestamp or string column, '{col}' is "):
            P.plan_query({"select": [["fn", "to_str", col]]}, t)
        with pytest.raises(TypeError, match=f"'{col}' is "):
            P.plan_query({"select": ["a"], "where": ["eq", ["fn", "upper", ["concat", "a", ["fn", "to_str", col]]], ["lit", "X"]]}, t)
    for col in ("a", "v", "day", "ts", "d"):
        assert P._case_by_type(("to_str", col), t.schema) is None
    with pytest.raises(TypeError, match="'v' is int64"):                                # unchanged: the bare column inside concat
        P.plan_query({"select": [["concat", "a", "v"]]}, t)
    assert P.plan_query({"select": [["concat", "a", ["fn", "to_str", "v"]]]}, t) is not None


# ---- the adapter ------------------------------------------------------------------------------------------------------------------------
def _reference_shaped(class_name, arguments, cast_type):
    """a node with only the reference class's name, `type` and attributes (AbstractCastFunction, functions.py:148-162)"""
    node = type(class_name, (), {"type": cast_type})()
    node.arguments, node._function, node._is_numpy_function, node._is_binary_func = tuple(arguments), None, False, False
    return node


def test_vectorize_and_lower_round_trip():
    want = ("to_str", "v")
    assert issubclass(B.StringCastFunction, B.AbstractCastFunction) and B.StringCastFunction.type == "str"
    assert B.FUNCTIONS_REGISTRY["to_str"] == (B.StringCastFunction, B.FunctionType.CLASS)
    for spelling in (want, ("fn", "to_str", "v"), ("fn", "TO_STR", "v")):
        node = B.vectorize(spelling)
        assert type(node) is B.StringCastFunction and B.lower(node) == want
    assert B.lower(B.StringCastFunction([B.Column("v")])) == want
    assert B.lower(_reference_shaped("StringCastFunction", [B.Column("v")], "str")) == want
    nested = B.vectorize(("concat", "a", ("lit", "-"), ("to_str", "v")))
    assert B.lower(nested) == ("concat", "a", ("lit", "-"), ("to_str", "v"))
    assert B.lower(B.vectorize(("like", ("to_str", "v"), ("lit", "1%")))) == ("like", ("to_str", "v"), ("lit", "1%"))
    assert B.lower(B.vectorize(("to_int", "v"))) == ("to_int", "v")                     # the other three casts as before
    # not the reference's class, or not its cast: no lowering
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(_reference_shaped("StringCastFunction", [B.Column("v")], "bytes"))
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(_reference_shaped("TextCastFunction", [B.Column("v")], "str"))
    text = ""
    try:
        B.lower(_reference_shaped("SomeUdf", [B.Column("v")], None))
    except NotImplementedError as e:
        text = str(e)
    assert "to_str" in text.split(";")[0] and "to_str" not in text.split(";")[1]         # the refusal names to_str among what runs


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
_C = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void": None}


def test_the_new_symbols_are_exported_with_the_headers_signatures():
    from vinum_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vinum_hip.h")).read(), flags=re.S)
    for name in ("vnm_strval_create", "vnm_strval_destroy", "vnm_strval_to_str", "vnm_strval_stats"):
        m = re.search(r"([\w\*]+(?:\s*\*)?)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        ret, params = m.group(1).strip(), [p.strip() for p in m.group(2).split(",")]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == len(params), (name, params)
        assert restype == (ctypes.c_void_p if "*" in ret else _C[ret]), (name, ret)
        for p, at in zip(params, argtypes):
            base = p.replace("const ", "").rsplit(" ", 1)[0].strip()
            assert at == (ctypes.c_void_p if "*" in p else _C[base]), (name, p)


# ---- the restatement is the reference's function ----------------------------------------------------------------------------------------
def test_the_restatement_equals_numpy_and_the_fixtures():
    """text_of() is np.array(column, dtype='str') for a column without NULLs (StringCastFunction's kernel, functions.py:148-162,189-193) --
    the reference's own results say so, the zone-aware column included (its UTC instant) -- and "None" for a NULL row"""
    from tests import util
    from tests.golden import to_str_cases as C
    t = util.read_ipc("to_str_in_main.arrow")
    assert t.equals(C.to_str_main_table())
    for case, col, out in (("select_int64", "v", "sv"), ("select_int64", "w", "sw"), ("select_uint8", "u8", "s"), ("select_int32_negative", "i32", "s"),
                           ("select_date32", "day", "s"), ("select_timestamps", "ts_s", "s"), ("select_timestamps", "ts_ms", "ms"),
                           ("select_timestamps", "ts_us", "us"), ("select_timestamps", "ts_ns", "ns"), ("select_timestamp_with_zone", "ts_tz", "s"),
                           ("select_string", "city", "s"), ("select_dictionary_typed", "dcity", "s")):
        assert C.text_of(t[col]) == util.read_ipc(f"to_str_{case}.arrow")[out].to_pylist(), (case, col)
    assert C.text_of(t["w"]) == [str(s) for s in np.array(t["w"].to_numpy(), dtype="str")]
    assert C.text_of(pa.array([1, None, -1], pa.int8())) == ["1", "None", "-1"]
    assert C.text_of(pa.array([0, None], pa.date32())) == ["1970-01-01", "None"] and C.text_of(pa.array(["a\x00", None])) == ["a", "None"]
