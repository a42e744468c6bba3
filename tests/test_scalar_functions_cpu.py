"""Built-in scalar functions (abs, sqrt, sin, ..., power, pi, e, to_int / to_float / to_bool) on the host side: the
planner plans them as projections, the B2 adapter lowers the reference's trees for them, literal subtrees fold with
NumPy's own values and types, and what stays off the GPU path still says so.  No GPU needed."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import binding as B
from vinum_amd import expr as E
from vinum_amd import ops
from vinum_amd import planner as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

CASES = [
    (("fn", "sqrt", "total"), ("sqrt", "total")),
    (("fn", "np.sin", "lat"), ("sin", "lat")),
    (("fn", "to_int", ("mul", ("fn", "np.sin", "lat"), 100000)), ("to_int", ("mul", ("sin", "lat"), 100000))),
    (("add", "fare", ("fn", "pi")), ("add", "fare", ("pi",))),
    (("fn", "abs", ("sub", "total", "tip")), ("abs", ("sub", "total", "tip"))),
    (("fn", "power", "fare", 2), ("power", "fare", 2)),
    (("fn", "log10", "fare"), ("log10", "fare")),
    (("fn", "to_float", "n"), ("to_float", "n")),
    (("fn", "to_bool", "n"), ("to_bool", "n")),
    (("mul", ("fn", "e"), ("fn", "np.cos", "lat")), ("mul", ("e",), ("cos", "lat"))),
]


@pytest.mark.parametrize("spelled,prefix", CASES)
def test_planner_turns_builtins_into_expression_nodes(spelled, prefix):
    assert P._t(spelled) == prefix
    assert not P._has_fn(P._t(spelled))


@pytest.mark.parametrize("spelled,prefix", CASES)
def test_mirror_trees_lower_to_the_planner_programs(spelled, prefix):
    assert B.lower(B.vectorize(spelled)) == prefix


def test_scalar_functions_plan_as_projections_not_aggregates():
    t = pa.table({"fare": pa.array([1.0, 4.0]), "lat": pa.array([0.5, 1.5])})
    q = {"select": [("fn", "sqrt", "fare"), ("fn", "np.sin", "lat")], "aliases": [None, "s"],
         "where": ("gt", ("fn", "log10", "fare"), 0.0)}
    plan = P.plan_query(q, t)
    kinds = [s[0] for s in plan.steps]
    assert "aggregate" not in kinds
    assert kinds == ["read", "filter", "project"]
    assert plan.steps[-1][1] == (("sqrt", "fare"), ("sin", "lat"))
    assert plan.steps[-1][2] == ("sqrt", "s")            # the reference names a function column after the function


def test_scalar_functions_inside_aggregates_and_having():
    t = pa.table({"k": pa.array([1, 2]), "v": pa.array([1.0, 4.0])})
    q = {"select": ["k", ("fn", "sum", ("fn", "sqrt", "v")), ("fn", "avg", ("fn", "power", "v", 2))],
         "aliases": [None, "s", "p"], "group_by": ["k"],
         "having": ("gt", ("fn", "to_float", ("fn", "count_star")), 0.5),
         "order_by": [("fn", "abs", ("sub", "k", 5))], "sort_order": ["ASC"], "limit": 1}
    plan = P.plan_query(q, t)
    agg = next(s for s in plan.steps if s[0] == "aggregate")
    assert {f for (f, _), _ in agg[2]} == {"sum", "avg", "count_star"}
    assert (("sum", ("sqrt", "v"))) in [k for k, _ in agg[2]]
    having = next(s for s in plan.steps if s[0] == "having")[1]
    assert having[0] == "gt" and having[1][0] == "to_float"


def test_unknown_functions_keep_todays_error():
    t = pa.table({"v": pa.array([1.0])})
    with pytest.raises(ValueError, match="unknown aggregate function"):
        P.plan_query({"select": [("fn", "upper", "v")]}, t)


def test_literal_folding_keeps_numpy_value_and_type():
    assert E.fold(("sqrt", 4)) == ("strong", 2.0)                 # np.sqrt(4) -> np.float64: strong
    assert E.fold(("abs", -5)) == ("strong", 5)                   # np.absolute(-5) -> np.int64: strong
    assert E.fold(("pi",)) == np.pi and type(E.fold(("pi",))) is float    # lambda: np.pi -> weak Python float
    assert E.fold(("e",)) == np.e and type(E.fold(("e",))) is float
    assert E.fold(("sin", 1.0)) == ("strong", float(np.sin(1.0)))
    assert E.fold(("power", 2, 10)) == ("strong", 1024)
    assert E.fold(("to_int", ("log10", 1000.0))) == ("strong", 3)
    assert E.fold(("add", "x", ("sqrt", 2))) == ("add", "x", ("strong", float(np.sqrt(2))))
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed"):
        E.fold(("power", 2, -1))


def test_negative_literal_exponent_on_an_integer_column_raises_at_compile_time():
    """vnm_project's host typing (no device, a zero-length call) raises NumPy's ValueError before any row is touched"""
    types = {"i": (pa.int32(), False), "f": (pa.float64(), False), "n": (pa.int64(), True), "u8": (pa.uint8(), False)}
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.result_type(("power", "i", -2), types)
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.result_type(("add", 1, ("power", ("abs", "i"), ("to_int", -3.5))), types)     # a folded strong exponent
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.result_type(("power", "i", ("neg", 2)), types)                                # np.negative(2): strong int64
    assert ops.result_type(("power", "f", -2), types) == pa.float64()      # float base: fine
    assert ops.result_type(("power", "n", -2), types) == pa.float64()      # an int column with NULLs is float64
    assert ops.result_type(("power", "i", 2), types) == pa.int32()


@pytest.mark.parametrize("expr,want", [
    (("sqrt", "u8"), pa.float16()), (("sin", "i16"), pa.float32()), (("log", "i32"), pa.float64()),
    (("cos", "f32"), pa.float32()), (("abs", "i8"), pa.int8()), (("abs", "u64"), pa.uint64()),
    (("to_int", "f32"), pa.int64()), (("to_float", "u8"), pa.float64()), (("to_bool", "f64"), pa.uint8()),
    (("add", ("sqrt", "u8"), 1.5), pa.float16()), (("mul", ("sqrt", "u8"), "i16"), pa.float32()),
    (("power", "i16", "u8"), pa.int16()), (("power", "f32", 2), pa.float32()), (("sqrt", "n"), pa.float64()),
])
def test_result_types_follow_numpy(expr, want):
    types = {"u8": (pa.uint8(), False), "i8": (pa.int8(), False), "i16": (pa.int16(), False), "i32": (pa.int32(), False),
             "u64": (pa.uint64(), False), "f32": (pa.float32(), False), "f64": (pa.float64(), False), "n": (pa.int64(), True)}
    assert ops.result_type(expr, types) == want
    npt = {"u8": np.uint8, "i8": np.int8, "i16": np.int16, "i32": np.int32, "u64": np.uint64, "f32": np.float32,
           "f64": np.float64, "n": np.float64}
    fn = {"sqrt": np.sqrt, "sin": np.sin, "log": np.log, "cos": np.cos, "abs": np.absolute, "power": np.power,
          "add": np.add, "mul": np.multiply, "to_int": lambda x: np.array(x, dtype="int"),
          "to_float": lambda x: np.array(x, dtype="float"), "to_bool": lambda x: np.array(x, dtype="bool")}

    def ev(e):
        if isinstance(e, str):
            return np.ones(2, npt[e])
        if not isinstance(e, tuple):
            return e
        return fn[e[0]](*[ev(x) for x in e[1:]])
    got = np.asarray(ev(expr)).dtype
    assert (pa.uint8() if got == np.bool_ else pa.from_numpy_dtype(got)) == want


def test_float16_is_a_result_type_only():
    from vinum_amd.device import DeviceColumn, is_supported, physical_type
    assert not is_supported(pa.float16())
    with pytest.raises(RuntimeError, match="Unsupported data type"):
        physical_type(pa.float16())                      # an Arrow float16 input column is refused at staging, as before
    col = DeviceColumn(None, None, 0, 0, pa.float16())   # a projection result
    with pytest.raises(RuntimeError, match="float16 columns are not GPU operator inputs"):
        col.dcol()


def test_vectorize_keeps_unknown_functions_as_aggregate_nodes():
    node = B.vectorize(("fn", "upper", "v"))
    assert isinstance(node, B.AggregateFunction)                    # what it built before built-ins existed
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(B.vectorize(("fn", "np.exp", "v")))                  # a ufunc outside the built-ins: no lowering


def test_compiled_programs_use_the_new_opcodes():
    from vinum_amd import _lib as L
    prog = ops.compile_expr(("add", ("sqrt", "a"), ("power", "b", 2.5)), {"a": 0, "b": 1})
    assert [p.op for p in prog] == [L.EX_COL, L.EX_SQRT, L.EX_COL, L.EX_CONST_F, L.EX_POW, L.EX_ADD]
    prog = ops.compile_expr(("to_int", ("mul", ("pi",), "a")), {"a": 0})
    assert [p.op for p in prog] == [L.EX_CONST_F, L.EX_COL, L.EX_MUL, L.EX_TO_I64]
    assert prog[0].arg == 0 and prog[0].imm_f == np.pi            # weak literal
    prog = ops.compile_expr(("mul", ("sqrt", 4), "a"), {"a": 0})
    assert prog[0].op == L.EX_CONST_F and prog[0].arg == 1 and prog[0].imm_f == 2.0   # strong np.float64
    assert ops.columns_of(("add", ("pi",), ("e",))) == []
    assert L.OUT_F16 == 101 and L.EX_STORE == 24 and L.EX_TO_BOOL == 36


@pytest.mark.parametrize("fn", [np.exp, "upper", "date", "like"])
def test_other_functions_still_raise_not_implemented(fn):
    if fn == "upper" or fn == "date" or fn == "like":
        class Other(B.VectorizedExpression):      # a CLASS built-in: _function is None
            pass
        node = Other([B.Column("s")])
        node.__class__.__name__ = {"upper": "UpperStringFunction", "date": "DateFunction", "like": "LikeFunction"}[fn]
    else:
        node = B.VectorizedExpression([B.Column("v")], function=fn, is_numpy_func=True)
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(node)


def _reference():
    if not os.path.isdir(os.path.join(REF, "vinum")) or not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")):
        # oracle/_ref is what build() compiles from the reference; the lowering itself is checked on the mirror above
        pytest.skip("the reference is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pglast_stub"))
    if REF not in sys.path:
        sys.path.append(REF)
    from oracle import ref_vinum_lib
    sys.modules.setdefault("vinum_lib", ref_vinum_lib)
    import vinum
    return vinum


REF_CASES = [
    ("fn", "sqrt", "total"), ("fn", "np.sin", "lat"), ("fn", "to_int", ("mul", ("fn", "np.sin", "lat"), 100000)),
    ("add", "fare", ("fn", "pi")), ("fn", "to_float", "n"), ("fn", "to_bool", "n"), ("fn", "abs", ("sub", "total", "tip")),
    ("fn", "power", "fare", 2), ("fn", "log2", "fare"), ("fn", "np.abs", "tip"),
]


@pytest.mark.parametrize("spelled", REF_CASES)
def test_reference_planner_trees_lower_under_install(spelled):
    vinum = _reference()
    from vinum.core import base as rbase
    from vinum.core import functions as rfn
    from vinum.core.expressions import EXPRESSION_FUNCTIONS
    from vinum.parser.query import Column, Expression, Literal, Query, SQLExpression
    from vinum.planner.planner import QueryPlanner
    from vinum.arrow.arrow_table import ArrowTable
    B.install(vinum)
    import vinum.planner.planner as pm
    index = pm._vinum_amd_index

    def to_ast(e):
        if isinstance(e, str):
            return Column(e)
        if isinstance(e, (int, float)):
            return Literal(e)
        if e[0] == "fn":
            return Expression(SQLExpression.FUNCTION, tuple(to_ast(a) for a in e[2:]), function_name=e[1])
        name = {"add": "ADDITION", "sub": "SUBTRACTION", "mul": "MULTIPLICATION"}[e[0]]
        return Expression(SQLExpression[name], tuple(to_ast(a) for a in e[1:]))

    table = pa.table({c: pa.array([1.0, 2.0]) for c in ("total", "lat", "fare", "tip", "n")})
    planner = QueryPlanner(Query(table.schema, (to_ast(spelled),), False, False, None, (), None, (), (), None, 0),
                           table=ArrowTable(table))
    tree = planner._process_expressions_tree(to_ast(spelled), set())
    assert B.lower(tree, index) == P._t(spelled)
