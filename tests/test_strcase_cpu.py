"""upper() / lower() without a GPU: the code point tables built from the installed pyarrow, the bindings (binding.lower over
reference-shaped nodes, vectorize, planner._t) and core.lowering.lower_case_functions over stub dictionaries."""
import random

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from vinum_amd import binding as B
from vinum_amd import planner as P
from vinum_amd import strcase
from vinum_amd.core.lowering import lower_case_functions, lower_dictionary, project_lowered

KERNEL = {"upper": pc.utf8_upper, "lower": pc.utf8_lower}


# ---- the table builder ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["upper", "lower"])
def test_tables_hold_what_the_device_code_relies_on(fn):
    map_from, map_to = strcase.case_table(fn)
    assert map_from.dtype == np.int32 and map_to.dtype == np.int32 and len(map_from) == len(map_to)
    assert 1000 < len(map_from) <= 2048                           # what a workgroup holds in LDS (MC_MAX_MAP)
    assert (np.diff(map_from) > 0).all()                          # strictly ascending
    for a in (map_from, map_to):
        assert not ((a >= 0xD800) & (a < 0xE000)).any() and (a >= 0).all() and (a <= 0x10FFFF).all()     # no surrogate
    assert (map_from != map_to).all()
    ascii_part = map_from < 0x80
    assert ascii_part.sum() == 26 and (map_to[ascii_part] < 0x80).all()                       # ASCII maps within ASCII
    assert (strcase.utf8_width(map_to) <= 2 * strcase.utf8_width(map_from)).all()               # the 2x bound
    assert strcase.case_table(fn)[0] is map_from                  # built once per process
    assert 0 < strcase.build_seconds[fn] < 30


def test_the_counts_the_design_quotes():
    up, lo = strcase.case_table("upper"), strcase.case_table("lower")
    grows = lambda t: int((strcase.utf8_width(t[1]) > strcase.utf8_width(t[0])).sum())
    shrinks = lambda t: int((strcase.utf8_width(t[1]) < strcase.utf8_width(t[0])).sum())
    # (the numbers of DESIGN.md section 4.9d, from the utf8proc the installed pyarrow carries: printed, not pinned, but the shape is)
    print("upper", len(up[0]), grows(up), shrinks(up), hex(int(up[0].max())), "lower", len(lo[0]), grows(lo), shrinks(lo), hex(int(lo[0].max())))
    assert grows(up) > 0 and shrinks(up) > 0 and grows(lo) > 0 and shrinks(lo) > 0
    assert dict(zip(up[0].tolist(), up[1].tolist()))[ord("ß")] == ord("ẞ")
    assert dict(zip(lo[0].tolist(), lo[1].tolist()))[ord("İ")] == ord("i")
    assert int(up[0].max()) >= 0x10000 and int(lo[0].max()) >= 0x10000       # 4-byte sequences are mapped too


@pytest.mark.parametrize("fn", ["upper", "lower"])
def test_substitution_equals_the_arrow_kernel(fn):
    map_from, _ = strcase.case_table(fn)
    rng = random.Random(5)
    pool = [chr(c) for c in map_from.tolist()] + list("abcxyzABCXYZ 0189_-") * 20 + ["中", "文", "大", "阪", "\U0001F600"]
    texts = ["".join(rng.choice(pool) for _ in range(rng.randint(0, 16))) for _ in range(20_000)]
    texts += [chr(c) for c in map_from.tolist()] + ["", "a\x00", "\x00"]
    want = KERNEL[fn](pa.array(texts, pa.string())).to_pylist()
    assert [strcase.substitute(fn, s) for s in texts] == want


def test_a_multi_code_point_image_raises():
    data, offs = np.frombuffer("SS".encode(), np.uint8), np.array([0, 2], np.int32)
    with pytest.raises(RuntimeError, match="not a single code point"):
        strcase._decode_single(data, offs)
    with pytest.raises(ValueError, match="no case map"):
        strcase.case_table("title")


# ---- the bindings -----------------------------------------------------------------------------------------------------------------------
def _stand_in(class_name, arguments):
    """a node that has only the reference class's name and attributes (functions.py:279-298: Cls(arguments), no callable)"""
    cls = type(class_name, (), {})
    node = cls()
    node.arguments, node._function, node._is_numpy_function, node._is_binary_func = tuple(arguments), None, False, False
    return node


def test_lower_recognises_the_reference_shaped_nodes():
    """(on the parent commit this raised NotImplementedError("no GPU lowering ..."))"""
    assert B.lower(B.UpperStringFunction([B.Column("city")])) == ("upper", "city")
    assert B.lower(B.LowerStringFunction([B.Column("city")])) == ("lower", "city")
    assert B.lower(_stand_in("UpperStringFunction", [B.Column("city")])) == ("upper", "city")
    assert B.lower(_stand_in("LowerStringFunction", [B.Column("name")])) == ("lower", "name")
    nested = _stand_in("UpperStringFunction", [B.LowerStringFunction([B.Column("city")])])
    assert B.lower(nested) == ("upper", ("lower", "city"))
    like = B.LikeFunction((B.LowerStringFunction([B.Column("name")]), B.Literal("b%")), False)
    assert B.lower(like) == ("like", ("lower", "name"), ("lit", "b%"))
    eq = B.vectorize(("eq", ("upper", "city"), ("lit", "BERLIN")))
    assert B.lower(eq) == ("eq", ("upper", "city"), ("lit", "BERLIN"))
    with pytest.raises(NotImplementedError, match="no GPU lowering"):            # two arguments: not the reference's shape
        B.lower(_stand_in("UpperStringFunction", [B.Column("a"), B.Column("b")]))
    renamed = type("Other", (B.VectorizedExpression,), {})([B.Column("s")])       # some other class that merely carries the name
    type(renamed).__name__ = "UpperStringFunction"
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(renamed)
    assert B.FUNCTIONS_REGISTRY["upper"] == (B.UpperStringFunction, B.FunctionType.CLASS)
    assert B.FUNCTIONS_REGISTRY["lower"] == (B.LowerStringFunction, B.FunctionType.CLASS)


@pytest.mark.parametrize("expr", [("upper", "city"), ("lower", ("upper", "city")), ("in", ("lower", "city"), ("a", "b")),
                                  ("and", ("like", ("upper", "n"), ("lit", "A%")), ("lt", ("lower", "a"), ("lower", "b")))])
def test_vectorize_round_trips(expr):
    assert B.lower(B.vectorize(expr)) == expr
    node = B.vectorize(("upper", "city"))
    assert type(node) is B.UpperStringFunction and node._function is None and B.lower(node) == ("upper", "city")
    # the "fn" spelling builds the function node it always built; planner._t maps its lowering
    assert P._t(B.lower(B.vectorize(("fn", "UPPER", "city")))) == ("upper", "city")


def test_the_planner_maps_the_function_names():
    assert P._t(["fn", "UPPER", "city"]) == ("upper", "city")
    assert P._t(["fn", "lower", ["fn", "Upper", "city"]]) == ("lower", ("upper", "city"))
    assert P._t(["eq", ["fn", "upper", "c"], ["lit", "X"]]) == ("eq", ("upper", "c"), ("lit", "X"))
    assert P._t(["fn", "concat", "a", "b"]) == ("fn", "concat", "a", "b")           # not a built-in: stays a function node
    # over a numeric column of a table (the schema is known at plan time) the query is refused as one with an unknown function is
    with pytest.raises(ValueError, match="unknown aggregate function 'lower'"):
        P.plan_query({"select": ["k"], "where": ["eq", ["fn", "lower", "k"], ["lit", "x"]], "group_by": [["fn", "lower", "k"]]}, pa.table({"k": pa.array([1])}))
    assert P._case_by_type(("upper", ("lower", "k")), pa.schema([("k", pa.binary())])) is None        # (binary: the lowering's TypeError)
    t = pa.table({"c": pa.array(["x"]), "k": pa.array([1])})
    plan = P.plan_query({"select": ["k"], "group_by": [["fn", "upper", "c"]], "order_by": [["fn", "lower", "c"]]}, t)
    assert ("project_inner", ((("upper", "c"), "__inner_0"),)) in plan.steps        # the GROUP BY expression is projected, then grouped by
    assert any(s[0] == "aggregate" and s[1] == ("__inner_0",) for s in plan.steps)


# ---- the lowering over stub dictionaries ------------------------------------------------------------------------------------------------
class StubDict:
    """what lower_case_functions and the later steps ask of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.value_type, self.on_device = name, arrow_type, arrow_type, on_device
        self.calls, self.derived = [], {}

    def mapped_column(self, fn, col):
        if not self.on_device:
            raise NotImplementedError(f"no GPU lowering for {fn}() over a {self.type} column")
        if not (pa.types.is_string(self.type) or pa.types.is_large_string(self.type)):
            raise TypeError(f"{fn}() needs a string column, not {self.type}")
        self.calls.append((fn, col.name))
        d = self.derived.setdefault(fn, StubDict(f"{fn}({self.name})"))
        return StubColumn(f"{fn}({col.name})", d)

    def like_table(self, pattern):
        return f"<like {pattern!r} in {self.name}>"

    def code_of(self, value):
        return {"BERLIN": 4}.get(value)

    def translate_table(self, other):
        return f"<codes of {self.name} in {other.name}>"


class StubColumn:
    length = 10

    def __init__(self, name, dictionary=None, arrow_type=pa.int32()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


def _columns():
    return {"city": StubColumn("city", StubDict("C")), "name": StubColumn("name", StubDict("N", pa.large_string())),
            "raw": StubColumn("raw", StubDict("R", pa.binary())), "flag": StubColumn("flag", StubDict("F", pa.bool_(), on_device=False)),
            "v": StubColumn("v", None, pa.int64())}


def test_a_repeated_node_is_materialised_once():
    cols = _columns()
    extra = {}
    e1, _ = lower_dictionary(("or", ("eq", ("upper", "city"), ("lit", "BERLIN")), ("like", ("upper", "city"), ("lit", "B%"))), cols, extra)
    e2, _ = lower_dictionary(("eq", ("upper", "city"), ("lit", "nowhere")), cols, extra)
    assert cols["city"].dictionary.calls == [("upper", "city")]
    assert e1 == ("or", ("eq", "__upper_city", 4), ("lookup", "__upper_city", "__like_1___upper_city"))
    assert e2 == ("eq", "__upper_city", -2)
    assert extra["__upper_city"].dictionary is cols["city"].dictionary.derived["upper"]
    assert extra["__like_1___upper_city"] == "<like 'B%' in upper(C)>"            # LIKE asked the DERIVED dictionary


def test_a_nested_node_chains_two_derived_dictionaries():
    cols = _columns()
    e, extra = lower_case_functions(("upper", ("lower", "city")), cols)
    assert e == "__upper___lower_city" and list(extra) == ["__lower_city", "__upper___lower_city"]
    first = cols["city"].dictionary.derived["lower"]
    assert extra["__lower_city"].dictionary is first and first.calls == [("upper", "lower(city)")]
    assert extra["__upper___lower_city"].dictionary is first.derived["upper"]
    # two columns, two dictionaries: the pair lowering sees two ordinary string columns
    e, extra = lower_dictionary(("eq", ("upper", "city"), ("upper", "name")), cols)
    assert e == ("eq", "__upper_city", ("lookup_i32", "__upper_name", "__codes_of___upper_name_in___upper_city"))
    assert extra["__codes_of___upper_name_in___upper_city"] == "<codes of upper(N) in upper(C)>"


def test_operands_that_do_not_lower():
    cols = _columns()
    with pytest.raises(TypeError, match="upper\\(\\) needs a string column, 'v' is int64"):
        lower_dictionary(("upper", "v"), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for lower\\(\\) over \\('lit', 'x'\\)"):
        lower_dictionary(("eq", ("lower", ("lit", "x")), ("lit", "x")), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for upper\\(\\) over \\('add', 'v', 1\\)"):
        lower_dictionary(("upper", ("add", "v", 1)), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering for upper\\(\\) over 'nowhere'"):
        lower_dictionary(("upper", "nowhere"), cols)
    with pytest.raises(NotImplementedError, match="2 operand"):
        lower_dictionary(("upper", "city", "name"), cols)
    with pytest.raises(TypeError, match="needs a string column, not binary"):
        lower_dictionary(("lower", "raw"), cols)
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        lower_dictionary(("lower", "flag"), cols)


def test_key_dictionary_refuses_before_it_touches_the_device():
    from vinum_amd.vinum_lib import KeyDictionary
    with pytest.raises(TypeError, match="needs a string column, not binary"):
        KeyDictionary(pa.binary()).mapped("upper")
    with pytest.raises(TypeError, match="needs a string column"):
        KeyDictionary(pa.dictionary(pa.int8(), pa.large_binary())).mapped("lower")
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        KeyDictionary(pa.bool_()).mapped("upper")
    with pytest.raises(ValueError, match="no case map"):
        KeyDictionary(pa.string()).mapped("title")


def test_a_bare_function_is_the_derived_column(monkeypatch):
    """SELECT upper(city): no program runs for it, the derived column itself is the output"""
    from vinum_amd import ops
    cols = _columns()
    seen = []
    monkeypatch.setattr(ops, "project_many", lambda exprs, used, length=None: seen.append((list(exprs), list(used))) or [f"<{e}>" for e in exprs])
    out = project_lowered([("upper", "city"), ("add", "v", 1), ("lower", "city")], cols, 10)
    assert seen == [([("add", "v", 1)], ["v"])]
    assert out[0].name == "upper(city)" and out[1] == "<('add', 'v', 1)>" and out[2].name == "lower(city)"


def test_concat_still_has_no_lowering():
    # ConcatFunction carries np.char.add (functions.py:263-268), which newer NumPy makes the `add` ufunc itself: either the node has
    # no lowering, or it lowers to an addition that the dictionary lowering refuses for string columns
    concat = B.VectorizedExpression([B.Column("city"), B.Column("name")], function=np.char.add, is_numpy_func=True, is_binary_func=True)
    with pytest.raises((NotImplementedError, TypeError), match="no GPU lowering|not a numeric operand"):
        lower_dictionary(B.lower(concat), _columns())
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(_stand_in("ConcatFunction", [B.Column("a"), B.Column("b")]))
    with pytest.raises(ValueError, match="unknown aggregate function"):
        P.plan_query({"select": [["fn", "concat", "a", "b"]]}, pa.table({"a": pa.array(["x"]), "b": pa.array(["y"])}))
