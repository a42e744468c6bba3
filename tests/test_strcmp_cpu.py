"""Two dictionary-coded columns compared with each other, without a GPU: the lowering over a mirror batch with fake
dictionaries (shapes of the rewrites, the pairs left alone, the three error cases), the opcode values and what
ops.compile_expr emits, and the host-side typing of VNM_EX_LOOKUP_I32 (a zero-length vnm_project call)."""
import ctypes

import pyarrow as pa
import pytest

from vinum_amd import _lib as L
from vinum_amd import ops
from vinum_amd.core.algebra import FilterOperator, lower_column_compares
from vinum_amd.core.base import DeviceRecordBatch


class FakeDict:
    """what the lowering asks of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.on_device = name, arrow_type, on_device
        self.calls = []

    def translate_table(self, other):
        self.calls.append(("translate", other.name))
        return f"<codes of {self.name} in {other.name}>"

    def joint_rank_tables(self, other):
        self.calls.append(("joint", other.name))
        return f"<joint ranks of {self.name}>", f"<joint ranks of {other.name}>"

    def rank_column(self, col):
        self.calls.append(("rank", col.name))
        return f"<ranks of {col.name}>"

    def code_of(self, value):
        return {"Berlin": 3}.get(value)

    def rank_bounds(self, value):
        return 2, 1


class FakeColumn:
    def __init__(self, name, dictionary=None, arrow_type=pa.int64()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


def _batch():
    da, db, shared = FakeDict("A"), FakeDict("B", pa.large_string()), FakeDict("S")
    host = FakeDict("H", pa.decimal128(10, 2), on_device=False)
    cols = {"a": FakeColumn("a", da), "b": FakeColumn("b", db), "s1": FakeColumn("s1", shared), "s2": FakeColumn("s2", shared),
            "h": FakeColumn("h", host), "v": FakeColumn("v"), "w": FakeColumn("w")}
    return DeviceRecordBatch(cols, 0), da, db, shared


@pytest.mark.parametrize("op", ["eq", "ne"])
def test_equality_translates_the_right_operand(op):
    batch, da, db, _ = _batch()
    pred, extra = FilterOperator.lower_dictionary_predicates((op, "a", "b"), batch)
    assert pred == (op, "a", ("lookup_i32", "b", "__codes_of_b_in_a"))
    assert extra == {"__codes_of_b_in_a": "<codes of B in A>"}
    assert db.calls == [("translate", "A")] and da.calls == []


@pytest.mark.parametrize("op", ["lt", "le", "gt", "ge"])
def test_ordered_operators_compare_joint_ranks(op):
    batch, da, db, _ = _batch()
    pred, extra = FilterOperator.lower_dictionary_predicates((op, "a", "b"), batch)
    assert pred == (op, ("lookup_i32", "a", "__joint_rank_a_with_b"), ("lookup_i32", "b", "__joint_rank_b_with_a"))
    assert extra == {"__joint_rank_a_with_b": "<joint ranks of A>", "__joint_rank_b_with_a": "<joint ranks of B>"}
    assert da.calls == [("joint", "B")] and db.calls == []


@pytest.mark.parametrize("op", ["eq", "ne"])
def test_one_shared_dictionary_compares_codes(op):
    batch, _, _, shared = _batch()
    pred, extra = FilterOperator.lower_dictionary_predicates((op, "s1", "s2"), batch)
    assert pred == (op, "s1", "s2") and extra == {} and shared.calls == []


@pytest.mark.parametrize("op", ["lt", "le", "gt", "ge"])
def test_one_shared_dictionary_orders_by_rank_columns(op):
    batch, _, _, shared = _batch()
    pred, extra = FilterOperator.lower_dictionary_predicates((op, "s1", "s2"), batch)
    assert pred == (op, "__rank_s1", "__rank_s2")
    assert extra == {"__rank_s1": "<ranks of s1>", "__rank_s2": "<ranks of s2>"}
    assert shared.calls == [("rank", "s1"), ("rank", "s2")]


def test_between_with_column_bounds_follows_from_the_primitives():
    batch, da, db, _ = _batch()
    pred, extra = FilterOperator.lower_dictionary_predicates(("between", "a", "b", "s1"), batch)
    assert pred == ("and", ("ge", ("lookup_i32", "a", "__joint_rank_a_with_b"), ("lookup_i32", "b", "__joint_rank_b_with_a")),
                    ("le", ("lookup_i32", "a", "__joint_rank_a_with_s1"), ("lookup_i32", "s1", "__joint_rank_s1_with_a")))
    assert sorted(extra) == ["__joint_rank_a_with_b", "__joint_rank_a_with_s1", "__joint_rank_b_with_a", "__joint_rank_s1_with_a"]
    pred, _ = FilterOperator.lower_dictionary_predicates(("not_between", "a", "b", "b"), batch)
    assert pred == ("or", ("lt", ("lookup_i32", "a", "__joint_rank_a_with_b"), ("lookup_i32", "b", "__joint_rank_b_with_a")),
                    ("gt", ("lookup_i32", "a", "__joint_rank_a_with_b"), ("lookup_i32", "b", "__joint_rank_b_with_a")))
    assert da.calls.count(("joint", "B")) == 2          # one per lowering: one pair of tables serves both halves of NOT BETWEEN


def test_rewrites_nest_and_leave_the_rest_alone():
    batch, _, _, _ = _batch()
    tree = ("or", ("and", ("eq", "a", "b"), ("gt", "v", 3)), ("not", ("lt", "b", "a")), ("eq", "a", ("lit", "Berlin")),
            ("to_int", ("ne", "a", "b")))
    pred, extra = FilterOperator.lower_dictionary_predicates(tree, batch)
    assert pred == ("or", ("and", ("eq", "a", ("lookup_i32", "b", "__codes_of_b_in_a")), ("gt", "v", 3)),
                    ("not", ("lt", ("lookup_i32", "b", "__joint_rank_b_with_a"), ("lookup_i32", "a", "__joint_rank_a_with_b"))),
                    ("eq", "a", 3), ("to_int", ("ne", "a", ("lookup_i32", "b", "__codes_of_b_in_a"))))
    assert ("eq", "v", "w") == lower_column_compares(("eq", "v", "w"), batch.columns)[0]      # numeric columns: untouched


@pytest.mark.parametrize("tree", [
    ("eq", "a", "v"), ("lt", "v", "a"), ("ne", "a", 5), ("ge", 2.5, "a"), ("eq", "a", ("add", "v", 1)), ("between", "a", "v", "b"),
    ("between", "v", "a", "b"),
])
def test_a_numeric_operand_raises(tree):
    batch, _, _, _ = _batch()
    with pytest.raises(TypeError, match="cannot compare"):
        FilterOperator.lower_dictionary_predicates(tree, batch)


@pytest.mark.parametrize("tree", [("add", "a", 1), ("gt", ("mul", "v", "a"), 3), ("neg", "b"), ("to_int", "a"), ("sqrt", "a"),
                                  ("eq", ("mod", "a", "b"), 0)])
def test_arithmetic_on_a_dictionary_column_raises(tree):
    batch, _, _, _ = _batch()
    with pytest.raises(TypeError, match="not a numeric operand"):
        FilterOperator.lower_dictionary_predicates(tree, batch)


def test_symbolic_operator_names_are_lowered_and_refused_alike():
    batch, _, _, _ = _batch()
    assert lower_column_compares(("==", "a", "b"), batch.columns)[0] == ("eq", "a", ("lookup_i32", "b", "__codes_of_b_in_a"))
    assert lower_column_compares(("<", "a", "b"), batch.columns)[0] == \
        ("lt", ("lookup_i32", "a", "__joint_rank_a_with_b"), ("lookup_i32", "b", "__joint_rank_b_with_a"))
    assert lower_column_compares((">", "v", "w"), batch.columns)[0] == (">", "v", "w")
    with pytest.raises(TypeError, match="cannot compare"):
        lower_column_compares(("<>", "a", "v"), batch.columns)
    with pytest.raises(TypeError, match="not a numeric operand"):
        lower_column_compares(("*", "a", 2), batch.columns)


def test_an_operator_that_is_not_arithmetic_passes_through():
    """the TypeError is for the arithmetic / math / cast names only: any other operator over a dictionary-coded column (a string
    function, say) is left to whoever compiles it, and a comparison inside it is still lowered"""
    batch, _, _, _ = _batch()
    assert lower_column_compares(("upper", "a"), batch.columns)[0] == ("upper", "a")
    assert lower_column_compares(("some_function", "h", ("eq", "a", "b")), batch.columns)[0] == \
        ("some_function", "h", ("eq", "a", ("lookup_i32", "b", "__codes_of_b_in_a")))


@pytest.mark.parametrize("tree", [("eq", "a", "h"), ("lt", "h", "b"), ("between", "a", "h", "b")])
def test_a_host_route_dictionary_raises(tree):
    batch, _, _, _ = _batch()
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        FilterOperator.lower_dictionary_predicates(tree, batch)


def test_simple_predicate_on_codes_raises():
    batch, _, _, _ = _batch()
    with pytest.raises(TypeError, match="cannot compare"):
        FilterOperator(("a", "==", 5), None)._kernel(batch)


def test_opcode_values():
    assert L.EX_LOOKUP_I32 == 38
    assert (L.EX_LOOKUP_U8, L.EX_TO_BOOL, L.EX_TO_I64, L.EX_POW, L.EX_ABS, L.EX_STORE, L.EX_NOT, L.EX_EQ, L.EX_COL) == (37, 36, 35, 33, 25, 24, 21, 13, 0)
    assert L.MASK_U8 == 100 and L.OUT_F16 == 101


def test_compile_expr_emits_the_lookup():
    index = {"a": 0, "b": 1, "__t": 2, "__u": 3}
    prog = ops.compile_expr(("eq", "a", ("lookup_i32", "b", "__t")), index)
    assert [(p.op, p.arg, p.imm_i) for p in prog] == [(L.EX_COL, 0, 0), (L.EX_LOOKUP_I32, 1, 2), (L.EX_EQ, 0, 0)]
    prog = ops.compile_expr(("not", ("lt", ("lookup_i32", "a", "__t"), ("lookup_i32", "b", "__u"))), index)
    assert [(p.op, p.arg, p.imm_i) for p in prog] == [(L.EX_LOOKUP_I32, 0, 2), (L.EX_LOOKUP_I32, 1, 3), (L.EX_LT, 0, 0), (L.EX_NOT, 0, 0)]
    assert ops.columns_of(("eq", "a", ("lookup_i32", "b", "__t"))) == ["a", "b", "__t"]


def test_lookup_i32_typing_without_a_device():
    """a zero-length call type-checks: the lookup is a VALUE (compared: a mask; alone: float64, the type of an int32 column with
    NULLs), its table is exempt from the row-length check, is no row column, must be int32 without NULLs; the codes are int32"""
    dummy = ctypes.create_string_buffer(8)

    def typed(prog_ins, types, lengths, nullable=()):
        prog = ops._program(prog_ins)
        cols = (L.DCol * len(types))()
        for i, (t, n) in enumerate(zip(types, lengths)):
            cols[i].type, cols[i].length, cols[i].values = t, n, ctypes.addressof(dummy)
            if i in nullable:
                cols[i].validity = ctypes.addressof(dummy)
        ot = ctypes.c_int(0)
        rc = L.load().vnm_project(len(prog), prog, len(types), cols, 0, ctypes.addressof(dummy), ctypes.byref(ot), None)
        return rc, ot.value

    look = (L.EX_LOOKUP_I32, 1, 0.0, 2)
    eq = [(L.EX_COL, 0, 0.0, 0), look, (L.EX_EQ, 0, 0.0, 0)]
    assert typed(eq, [L.I32, L.I32, L.I32], [0, 0, 1000]) == (0, L.MASK_U8)
    assert typed(eq, [L.I32, L.I32, L.I32], [0, 0, 1000], nullable=(0, 1)) == (0, L.MASK_U8)
    assert typed([look], [L.I32, L.I32, L.I32], [0, 0, 7]) == (0, L.F64)
    both = [(L.EX_LOOKUP_I32, 0, 0.0, 2), (L.EX_LOOKUP_I32, 1, 0.0, 3), (L.EX_LT, 0, 0.0, 0), (L.EX_LOOKUP_U8, 0, 0.0, 4), (L.EX_AND, 0, 0.0, 0)]
    assert typed(both, [L.I32, L.I32, L.I32, L.I32, L.U8], [0, 0, 5, 9, 5]) == (0, L.MASK_U8)
    assert typed(eq, [L.I32, L.I32, L.U8], [0, 0, 7])[0] != 0                       # the table is int32
    assert typed(eq, [L.I32, L.I32, L.I64], [0, 0, 7])[0] != 0
    assert typed(eq, [L.I32, L.I32, L.I32], [0, 0, 7], nullable=(2,))[0] != 0       # ... without NULLs
    assert typed(eq, [L.I32, L.I64, L.I32], [0, 0, 7])[0] != 0                      # codes are int32
    assert typed([(L.EX_COL, 2, 0.0, 0), look, (L.EX_EQ, 0, 0.0, 0)], [L.I32, L.I32, L.I32], [0, 0, 7])[0] != 0    # a table is no row column
    assert typed([(L.EX_LOOKUP_I32, 1, 0.0, 3)], [L.I32, L.I32, L.I32], [0, 0, 7])[0] != 0                          # table index out of range
    assert typed([(L.EX_LOOKUP_I32, 2, 0.0, 2)], [L.I32, L.I32, L.I32], [0, 0, 7])[0] != 0                          # codes from its own table
    assert typed([(L.EX_LOOKUP_I32, 0, 0.0, 2), (L.EX_LOOKUP_U8, 1, 0.0, 2), (L.EX_AND, 0, 0.0, 0)], [L.I32, L.I32, L.I32], [0, 0, 7])[0] != 0
    assert typed([(L.EX_COL, 0, 0.0, 0)], [L.I32, L.I32, L.I32], [0, 0, 7])[0] != 0     # no lookup: every column is a row column
