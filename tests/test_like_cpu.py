"""LIKE / NOT LIKE without a GPU: the host pattern compiler, the adapter's lowering of LikeFunction (mirror classes and, where the
reference is on the machine, the reference planner's own tree), vectorize() round trips and the shapes that keep raising."""
import os
import sys

import pyarrow as pa
import pytest

from vinum_amd import _lib as L
from vinum_amd import binding as B
from vinum_amd import ops
from vinum_amd import planner as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
LIT, ANY, STAR = L.LIKE_TOK_LIT, L.LIKE_TOK_ANY, L.LIKE_TOK_STAR


@pytest.mark.parametrize("pattern,tokens", [
    ("Jos%", [(LIT, b"Jos"), (STAR, b"%")]),
    ("%iv%", [(STAR, b"%"), (LIT, b"iv"), (STAR, b"%")]),
    ("a_c", [(LIT, b"a"), (ANY, b"_"), (LIT, b"c")]),
    ("a.c", [(LIT, b"a"), (ANY, b"."), (LIT, b"c")]),
    ("", []),
    ("%%_%%", [(STAR, b"%"), (ANY, b"_"), (STAR, b"%")]),
    ("ü€\n%", [(LIT, "ü€\n".encode()), (STAR, b"%")]),
    ("x" * 1500 + "%", [(LIT, b"x" * 1500), (STAR, b"%")]),
])
def test_pattern_tokens(pattern, tokens):
    assert ops.like_tokens(pattern) == tokens


@pytest.mark.parametrize("meta", list("\\^$*+?{}[]|()"))
def test_regex_metacharacters_are_refused(meta):
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        ops.like_tokens("a" + meta + "%")


def test_mirror_like_lowers():
    node = B.LikeFunction((B.Column("name"), B.Literal("Jos%")), False)
    assert B.lower(node) == ("like", "name", ("lit", "Jos%"))
    node = B.LikeFunction((B.Column("name"), B.Literal("Jos%")), True)
    assert B.lower(node) == ("not_like", "name", ("lit", "Jos%"))
    tree = B.vectorize(("or", ("eq", "id", 4), ("not_like", "city", ("lit", "%iv%"))))
    assert B.lower(tree) == ("or", ("eq", "id", 4), ("not_like", "city", ("lit", "%iv%")))


@pytest.mark.parametrize("spelled", [
    ["like", "name", ["lit", "Jos%"]], ["not_like", "s", ["lit", ""]],
    ["and", ["like", "s", ["lit", "a_c"]], ["gt", "v", 3]], ["not", ["like", "u", ["lit", "ü%"]]],
    ["fn", "to_int", ["like", "s", ["lit", "%b%"]]],
])
def test_vectorize_round_trip(spelled):
    e = P._t(spelled)
    tree = B.vectorize(e)
    assert B.lower(tree) == e


@pytest.mark.parametrize("make", [
    lambda: B.LikeFunction((B.Column("s"),), False),                                        # one operand
    lambda: B.LikeFunction((B.Column("s"), B.Literal("a%"), B.Literal("b")), False),        # three operands
    lambda: B.LikeFunction((B.Column("s"), B.Literal("a%")), None),                         # no boolean invert
    lambda: B.LikeFunction((B.Column("s"), B.Literal(5)), False),                           # not a string pattern
    lambda: B.LikeFunction((B.Column("s"), B.Column("t")), False),                          # a column pattern
])
def test_malformed_like_nodes_raise(make):
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(make())


def test_like_node_without_invert_attribute_raises():
    node = B.LikeFunction((B.Column("s"), B.Literal("a%")), False)
    del node.invert
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(node)


def test_like_outside_the_operators_is_not_compiled():
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        ops.compile_expr(("like", "s", ("lit", "a%")), {"s": 0})


def test_lookup_opcode_and_columns():
    assert L.EX_LOOKUP_U8 == 37 and L.EX_TO_BOOL == 36 and L.EX_STORE == 24 and L.OUT_F16 == 101
    prog = ops.compile_expr(("not", ("lookup", "s", "__t")), {"s": 0, "__t": 1})
    assert [(p.op, p.arg, p.imm_i) for p in prog] == [(L.EX_LOOKUP_U8, 0, 1), (L.EX_NOT, 0, 0)]
    assert ops.columns_of(("like", "s", ("lit", "a%"))) == ["s"]
    assert ops.columns_of(("lookup", "s", "__t")) == ["s", "__t"]


def test_lookup_typing_without_a_device():
    """a zero-length call type-checks: the lookup is a predicate, its table is exempt from the row-length check, a table
    cannot be read as a row column, the codes must be int32"""
    import ctypes
    dummy = ctypes.create_string_buffer(8)

    def typed(prog_ins, types, lengths):
        prog = ops._program(prog_ins)
        cols = (L.DCol * len(types))()
        for i, (t, n) in enumerate(zip(types, lengths)):
            cols[i].type, cols[i].length, cols[i].values = t, n, ctypes.addressof(dummy)
        ot = ctypes.c_int(0)
        rc = L.load().vnm_project(len(prog), prog, len(types), cols, 0, ctypes.addressof(dummy), ctypes.byref(ot), None)
        return rc, ot.value

    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 1)], [L.I32, L.U8], [0, 1000]) == (0, L.MASK_U8)
    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 1), (L.EX_NOT, 0, 0.0, 0)], [L.I32, L.U8], [0, 7]) == (0, L.MASK_U8)
    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 1)], [L.I64, L.U8], [0, 7])[0] != 0          # codes are int32
    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 1)], [L.I32, L.I32], [0, 7])[0] != 0         # the table is uint8
    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 1), (L.EX_COL, 1, 0.0, 0), (L.EX_CONST_I, 0, 0.0, 1), (L.EX_EQ, 0, 0.0, 0),
                  (L.EX_AND, 0, 0.0, 0)], [L.I32, L.U8], [0, 7])[0] != 0                  # a table is no row column
    assert typed([(L.EX_LOOKUP_U8, 0, 0.0, 2)], [L.I32, L.U8], [0, 7])[0] != 0          # table index out of range
    assert typed([(L.EX_COL, 0, 0.0, 0)], [L.I32, L.U8], [0, 7])[0] != 0                # no lookup: every column is a row column


def _reference():
    if not os.path.isdir(os.path.join(REF, "vinum")) or not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")):
        pytest.skip("the reference is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pglast_stub"))
    if REF not in sys.path:
        sys.path.append(REF)
    from oracle import ref_vinum_lib
    sys.modules.setdefault("vinum_lib", ref_vinum_lib)
    import vinum
    return vinum


@pytest.mark.parametrize("invert", [False, True])
def test_reference_planner_like_tree_lowers_under_install(invert):
    vinum = _reference()
    from vinum.arrow.arrow_table import ArrowTable
    from vinum.parser.query import Column, Expression, Literal, Query, SQLExpression
    from vinum.planner.planner import QueryPlanner
    B.install(vinum)
    import vinum.planner.planner as pm
    index = pm._vinum_amd_index
    e = Expression(SQLExpression.NOT_LIKE if invert else SQLExpression.LIKE, (Column("name"), Literal("Jos%")))
    table = pa.table({"name": pa.array(["Joe", "Joseph"])})
    planner = QueryPlanner(Query(table.schema, (e,), False, False, None, (), None, (), (), None, 0), table=ArrowTable(table))
    tree = planner._process_expressions_tree(e, set())
    assert type(tree).__name__ == "LikeFunction"
    assert B.lower(tree, index) == ("not_like" if invert else "like", "name", ("lit", "Jos%"))
    from vinum.core.functions import LikeFunction
    from vinum.core import base as rbase
    from vinum.core.expressions import BINARY_EXPRESSIONS, EXPRESSION_FUNCTIONS
    from vinum.core.functions import FunctionType
    from vinum.parser.query import Column as RC, Literal as RL
    from vinum.core.aggregate import AggregateFunction as RAF
    built = B.vectorize(("like", "name", ("lit", "Jos%")), registry=EXPRESSION_FUNCTIONS,
                        classes=(RC, RL, rbase.VectorizedExpression, RAF, SQLExpression, FunctionType, BINARY_EXPRESSIONS),
                        like_cls=LikeFunction)
    assert isinstance(built, LikeFunction) and B.lower(built, index) == ("like", "name", ("lit", "Jos%"))
