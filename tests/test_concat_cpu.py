"""concat() / || without a GPU: core.lowering.lower_case_functions over stub dictionaries (names, reuse, the left fold, where the
literals go), the refusals with their error types, planner._t / output_names / _case_by_type, the adapter's recognition of the
reference's ConcatFunction by qualified name and shape, the exported symbols against the header's signatures, and the Python
restatement the GPU tests compare with against np.char.add itself."""
import ctypes
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import binding as B
from vinum_amd import planner as P
from vinum_amd.core.lowering import concat_literal, lower_case_functions, lower_dictionary, project_lowered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the lowering over stub dictionaries ------------------------------------------------------------------------------------------------
class StubDict:
    """what lower_case_functions asks of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.value_type, self.on_device = name, arrow_type, arrow_type, on_device
        self.calls = []

    def _check(self):
        if not self.on_device:
            raise NotImplementedError(f"no GPU lowering for concat() over a {self.type} column")
        if not (pa.types.is_string(self.type) or pa.types.is_large_string(self.type)):
            raise TypeError(f"concat() needs a string column, not {self.type}")

    def mapped_column(self, fn, col):
        self.calls.append((fn, col.name))
        return StubColumn(f"{fn}({col.name})", StubDict(f"{fn}({self.name})"))

    def affixed_column(self, prefix, suffix, col):
        self._check()
        self.calls.append(("affix", prefix, col.name, suffix))
        return StubColumn(f"[{prefix.decode()}{col.name}{suffix.decode()}]", StubDict(f"affix({self.name})"))

    def pair_column(self, other, prefix, sep, suffix, a, b):
        self._check()
        other._check()
        self.calls.append(("pair", prefix, a.name, sep, b.name, suffix))
        return StubColumn(f"[{prefix.decode()}{a.name}{sep.decode()}{b.name}{suffix.decode()}]", StubDict(f"pair({self.name},{other.name})"))

    def code_of(self, value):
        return {"Ada Lovelace": 9}.get(value)


class StubColumn:
    length = 10

    def __init__(self, name, dictionary=None, arrow_type=pa.int32()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


def _columns():
    return {"a": StubColumn("a", StubDict("A")), "b": StubColumn("b", StubDict("B", pa.large_string())), "c": StubColumn("c", StubDict("C")),
            "raw": StubColumn("raw", StubDict("R", pa.binary())), "flag": StubColumn("flag", StubDict("F", pa.bool_(), on_device=False)),
            "v": StubColumn("v", None, pa.int64()), "ts": StubColumn("ts", None, pa.timestamp("s")), "day": StubColumn("day", None, pa.date32())}


def test_one_column_and_literals_is_an_affix():
    cols = _columns()
    e, extra = lower_case_functions(("concat", ("lit", "#"), 1, "a", ("lit", "!\x00"), 2.5), cols)
    assert cols["a"].dictionary.calls == [("affix", b"#1", "a", b"!2.5")]        # adjacent literals merged, str(number), trailing NUL dropped
    assert e in extra and extra[e].name == "[#1a!2.5]"
    e1, extra = lower_case_functions(("concat", "a"), cols)
    assert cols["a"].dictionary.calls[-1] == ("affix", b"", "a", b"") and extra[e1].name == "[a]"


def test_two_columns_are_one_pair_step_with_the_literals_in_its_writer():
    cols = _columns()
    e, extra = lower_case_functions(("concat", ("lit", "<"), "a", ("lit", "-"), "b", ("lit", ">")), cols)
    assert cols["a"].dictionary.calls == [("pair", b"<", "a", b"-", "b", b">")] and cols["b"].dictionary.calls == []
    assert list(extra) == [e] and extra[e].name == "[<a-b>]"


def test_three_columns_fold_left_through_the_derived_dictionary():
    cols = _columns()
    e, extra = lower_case_functions(("concat", ("lit", "("), "a", "b", ("lit", "/"), "c", ("lit", ")")), cols)
    assert cols["a"].dictionary.calls == [("pair", b"(", "a", b"", "b", b"")]
    first = next(c for n, c in extra.items() if n != e)
    assert first.dictionary.calls == [("pair", b"", "[(ab]", b"/", "c", b")")]     # the first step's dictionary is the second step's left one
    assert extra[e].name == "[[(ab]/c)]"


def test_a_repeated_node_is_materialised_once_and_nests_with_upper():
    cols = _columns()
    extra = {}
    node = ("concat", "a", ("lit", " "), "b")
    e1, _ = lower_dictionary(("or", ("eq", node, ("lit", "Ada Lovelace")), ("eq", node, ("lit", "nobody"))), cols, extra)
    e2, _ = lower_dictionary(("upper", node), cols, extra)
    assert cols["a"].dictionary.calls == [("pair", b"", "a", b" ", "b", b"")]
    name = next(iter(extra))
    assert e1 == ("or", ("eq", name, 9), ("eq", name, -2))
    assert extra[name].dictionary.calls == [("upper", "[a b]")] and e2 == f"__upper_{name}"
    cols = _columns()
    e3, extra = lower_case_functions(("concat", ("upper", "a"), ("lower", "b")), cols)
    assert cols["a"].dictionary.calls == [("upper", "a")] and cols["b"].dictionary.calls == [("lower", "b")]
    assert extra[e3].name == "[upper(a)lower(b)]"


def test_a_bare_concat_is_the_derived_column(monkeypatch):
    from vinum_amd import ops
    cols = _columns()
    seen = []
    monkeypatch.setattr(ops, "project_many", lambda exprs, used, length=None: seen.append((list(exprs), list(used))) or [f"<{e}>" for e in exprs])
    out = project_lowered([("concat", "a", "b"), ("add", "v", 1)], cols, 10)
    assert seen == [([("add", "v", 1)], ["v"])] and out[0].name == "[ab]"


def test_the_refusals_and_their_error_types():
    cols = _columns()
    for col, t in (("v", "int64"), ("ts", "timestamp"), ("day", "date32")):          # numeric and temporal: TypeError naming the column
        with pytest.raises(TypeError, match=f"concat\\(\\) needs a string column, '{col}' is {t}"):
            lower_dictionary(("concat", "a", col), cols)
    with pytest.raises(TypeError, match="needs a string column, not binary"):
        lower_dictionary(("concat", "raw", ("lit", "x")), cols)
    with pytest.raises(TypeError, match="needs a string column, not binary"):
        lower_dictionary(("concat", "a", "raw"), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        lower_dictionary(("concat", "flag", "a"), cols)
    with pytest.raises(NotImplementedError, match="literals alone"):
        lower_dictionary(("concat", ("lit", "x"), 7), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for concat\\(\\) over \\('add', 'v', 1\\)"):
        lower_dictionary(("concat", "a", ("add", "v", 1)), cols)
    with pytest.raises(NotImplementedError, match="over 'nowhere'"):
        lower_dictionary(("concat", "a", "nowhere"), cols)
    # the planner knows a table's schema: refused at plan time, by column name
    t = pa.table({"a": pa.array(["x"]), "v": pa.array([1]), "f": pa.array([1.5]), "ts": pa.array([0], pa.timestamp("s")), "raw": pa.array([b"x"])})
    for col in ("v", "f", "ts"):
        with pytest.raises(TypeError, match=f"'{col}' is "):
            P.plan_query({"select": [["concat", "a", ["lit", "-"], col]]}, t)
        with pytest.raises(TypeError, match=f"'{col}' is "):
            P.plan_query({"select": ["a"], "where": ["eq", ["fn", "upper", ["concat", col, "a"]], ["lit", "X"]]}, t)
    assert P._case_by_type(("concat", "a", "raw"), t.schema) is None                 # (binary: the lowering's TypeError)


def test_key_dictionary_refuses_before_it_touches_the_device():
    from vinum_amd.vinum_lib import KeyDictionary
    for t in (pa.binary(), pa.large_binary(), pa.dictionary(pa.int8(), pa.binary())):
        with pytest.raises(TypeError, match="needs a string column"):
            KeyDictionary(t).affixed(b"", b"")
        with pytest.raises(TypeError, match="needs a string column"):
            KeyDictionary(pa.string()).paired(KeyDictionary(t), b"", b"", b"")
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        KeyDictionary(pa.bool_()).affixed(b"x", b"")
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        KeyDictionary(pa.decimal128(10, 2)).paired(KeyDictionary(pa.string()), b"", b"", b"")


def test_literals():
    assert concat_literal(("lit", "x\x00\x00")) == b"x" and concat_literal(("lit", "\x00x")) == b"\x00x" and concat_literal(("lit", "ö")) == "ö".encode()
    assert concat_literal(7) == b"7" and concat_literal(2.5) == b"2.5" and concat_literal(-1) == b"-1" and concat_literal(1e30) == b"1e+30"
    assert concat_literal("a") is None and concat_literal(("upper", "a")) is None


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def test_the_planner_keeps_the_literals_and_names_the_column():
    """concat is spelled as the operator node; the "fn" spelling of that name stays the unknown function it was (tests/test_strcase_cpu.py)"""
    assert P._t(["concat", "a", ["lit", "-"], 7, 2.5, "b"]) == ("concat", "a", ("lit", "-"), 7, 2.5, "b")
    assert P._t(["fn", "upper", ["concat", ["fn", "lower", "a"], "b"]]) == ("upper", ("concat", ("lower", "a"), "b"))
    assert P._t(["||", ["||", "a", ["lit", " "]], "b"]) == ("concat", ("concat", "a", ("lit", " ")), "b")
    assert "concat" not in P.SCALAR_FN_NAMES and P._t(["fn", "concat", "a", "b"]) == ("fn", "concat", "a", "b")
    assert P.output_names([("concat", "a", "b"), "k", ("fn", "concat", "a")], ["c", None, None]) == ["c", "k", "concat"]      # (unchanged)
    t = pa.table({"a": pa.array(["x"]), "b": pa.array(["y"]), "k": pa.array([1])})
    plan = P.plan_query({"select": [["concat", "a", "b"], ["fn", "count_star"]], "group_by": [["concat", "a", "b"]]}, t)
    assert ("project_inner", ((("concat", "a", "b"), "__inner_0"),)) in plan.steps
    assert any(s[0] == "aggregate" and s[1] == ("__inner_0",) for s in plan.steps)


# ---- the adapter ------------------------------------------------------------------------------------------------------------------------
def _reference_shaped(class_name, arguments, function, binary):
    """a node with only the reference class's qualified name and attributes (functions.py:250-276)"""
    node = type(class_name, (), {})()
    node.arguments, node._function, node._is_numpy_function, node._is_binary_func = tuple(arguments), function, True, binary
    return node


def test_lower_recognises_concat_by_qualified_name_and_shape():
    """(on the parent commit every one of these raised NotImplementedError("no GPU lowering ...") or lowered to an addition)"""
    want = ("concat", "a", ("lit", "-"), 7, "b")
    args = [B.Column("a"), B.Literal("-"), B.Literal(7), B.Column("b")]
    assert B.lower(B.ConcatFunction(args)) == want
    assert B.lower(_reference_shaped("ConcatFunction", args, np.char.add, True)) == want
    assert B.lower(B.vectorize(want)) == want and type(B.vectorize(want)) is B.ConcatFunction
    assert B.lower(B.vectorize(("fn", "concat", "a"))) == ("fn", "concat", "a")       # the "fn" spelling builds what it always built
    pipe = B.vectorize(("||", ("||", "a", ("lit", " ")), "b"))                       # SQLExpression.CONCAT: the registry's class
    assert type(pipe) is B.ConcatFunction and B.lower(pipe) == ("concat", ("concat", "a", ("lit", " ")), "b")
    assert B.EXPRESSION_FUNCTIONS[B.SQLExpression.CONCAT] == (B.ConcatFunction, B.FunctionType.CLASS)
    assert B.FUNCTIONS_REGISTRY["concat"] == (B.ConcatFunction, B.FunctionType.CLASS) and B._SPEC_TO_SQL["concat"] == "CONCAT"
    nested = B.UpperStringFunction([B.ConcatFunction([B.LowerStringFunction([B.Column("a")]), B.Column("b")])])
    assert B.lower(nested) == ("upper", ("concat", ("lower", "a"), "b"))
    # not the reference's shape, or not its class: no lowering to concat
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(_reference_shaped("ConcatFunction", args, None, False))
    renamed = type("Other", (B.VectorizedExpression,), {})([B.Column("a")], function=len, is_binary_func=True)
    type(renamed).__name__ = "ConcatFunction"
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(renamed)
    text = ""
    try:
        B.lower(_reference_shaped("ToStrFunction", args, None, False))
    except NotImplementedError as e:
        text = str(e)
    assert "concat" in text.split(";")[0] and "concat" not in text.split(";")[1]     # the refusal names concat among what runs


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
_C = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void": None}


def test_the_new_symbols_are_exported_with_the_headers_signatures():
    from vinum_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vinum_hip.h")).read(), flags=re.S)
    names = ["vnm_strdict_concat_affix", "vnm_strdict_gather_codes", "vnm_strpair_create", "vnm_strpair_destroy", "vnm_strpair_concat", "vnm_strpair_stats"]
    for name in names:
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
def test_the_restatement_equals_np_char_add():
    """ConcatFunction's kernel (functions.py:263-276) over rows with trailing, embedded and leading NULs, NULL and numbers"""
    from tests.golden import concat_cases as C
    a = ["y\x00", "\x00z", "q\x00\x00", "x\x00y", None, "", "p"]
    b = ["c", None, "\x00", "tail\x00", "None", "", "ö"]
    t = pa.table({"a": pa.array(a, pa.string()), "b": pa.array(b, pa.large_string())})
    u = lambda x: np.array(x, dtype="U")
    want = np.char.add(np.char.add(np.char.add(u(a), u("-\x00")), u(b)), u(str(7))).tolist()
    assert C.restate(t, ["concat", "a", ["lit", "-\x00"], "b", 7]) == want
    assert want[0] == "y-c7" and want[1] == "\x00z-None7" and want[4] == "None-None7" and want[2] == "q-7"
