"""IN / NOT IN lists as sets, the host side (no device): compare domains, canonical tables and routes through
vnm_in_set_plan_host, and which lists vinum_amd.ops.lower_in_sets turns into mask columns."""
import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import _lib as L
from vinum_amd import expr as E
from vinum_amd import ops

I64_MIN, I64_MAX = -2**63, 2**63 - 1
INT_TYPES = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32()]


# ---- domains: every row of the table in DESIGN.md section 4.9b ------------------------------------------------------------
@pytest.mark.parametrize("t", INT_TYPES, ids=str)
def test_domain_integer_column_int_list_is_exact_int64(t):
    assert ops.in_set_plan([1, 2, 300], t)["domain"] == L.IN_DOM_I64


def test_domain_uint64_column_int_list_is_exact_uint64():
    assert ops.in_set_plan([1, 2], pa.uint64())["domain"] == L.IN_DOM_U64


@pytest.mark.parametrize("t", [pa.float32(), pa.float64()], ids=str)
@pytest.mark.parametrize("vals", [[1, 2], [1.0, 2]], ids=["int_list", "float_list"])
def test_domain_float_column_is_float64(t, vals):
    assert ops.in_set_plan(vals, t)["domain"] == L.IN_DOM_F64


@pytest.mark.parametrize("t", INT_TYPES + [pa.uint64(), pa.float32(), pa.float64()], ids=str)
@pytest.mark.parametrize("vals", [[1, 2], [1.5, 2]], ids=["int_list", "float_list"])
def test_domain_column_with_validity_is_float64(t, vals):
    assert ops.in_set_plan(vals, t, has_validity=True)["domain"] == L.IN_DOM_F64


@pytest.mark.parametrize("t", INT_TYPES + [pa.uint64()], ids=str)
def test_domain_integer_column_float_list_is_float64(t):
    assert ops.in_set_plan([1, 2.5], t)["domain"] == L.IN_DOM_F64


# ---- canonical tables ----------------------------------------------------------------------------------------------------------
def test_table_sorted_and_distinct():
    p = ops.in_set_plan([5, -3, 5, 900, -3, 0], pa.int32())
    assert p["table"].tolist() == [-3, 0, 5, 900] and p["range"] == 904


def test_table_keeps_members_outside_the_column_type():
    # the column is widened, never the member narrowed: int8 against 300 matches nothing, and 300 must not wrap to 44
    assert ops.in_set_plan([300, 44], pa.int8())["table"].tolist() == [44, 300]


def test_table_float_drops_nan_and_folds_negative_zero():
    p = ops.in_set_plan([float("nan"), -0.0, 0.0, 2.5, float("inf"), float("nan"), 2.5], pa.float64())
    assert p["table"].tolist() == [0.0, 2.5, float("inf")]
    assert not np.signbit(p["table"][0])
    assert p["range"] == 0


def test_table_all_nan_is_empty():
    p = ops.in_set_plan([float("nan")], pa.float64())
    assert len(p["table"]) == 0 and p["route"] == "in_set:sorted_lds"


def test_table_uint64_drops_negative_members():
    p = ops.in_set_plan([-1, 7, I64_MIN, I64_MAX, 7], pa.uint64())
    assert p["table"].dtype == np.uint64 and p["table"].tolist() == [7, I64_MAX]
    assert len(ops.in_set_plan([-1, -2], pa.uint64())["table"]) == 0


def test_table_ints_that_collapse_to_one_double():
    # 2^53 and 2^53 + 1 are one float64: a column with NULLs compares in float64, where they are one member
    p = ops.in_set_plan([2**53, 2**53 + 1, 2**53 + 2], pa.int64(), has_validity=True)
    assert p["table"].tolist() == [float(2**53), float(2**53 + 2)]
    assert ops.in_set_plan([2**53, 2**53 + 1, 2**53 + 2], pa.int64())["table"].tolist() == [2**53, 2**53 + 1, 2**53 + 2]


# ---- routes at their boundaries -----------------------------------------------------------------------------------------------
def test_route_bitmap_up_to_64_bits_per_member():
    assert ops.in_set_plan([0, 5, 191], pa.int64()) | {"table": None} == {"domain": L.IN_DOM_I64, "route": "in_set:bitmap_lds",
                                                                          "table": None, "range": 192}
    p = ops.in_set_plan([0, 5, 192], pa.int64())
    assert p["route"] == "in_set:sorted_lds" and p["range"] == 193
    assert ops.in_set_plan([7], pa.int64())["route"] == "in_set:bitmap_lds"


def test_route_bitmap_of_32_kb_and_one_bit_more():
    p = ops.in_set_plan(list(range(4095)) + [262143], pa.int64())
    assert p["range"] == 262144 and p["route"] == "in_set:bitmap_lds"
    p = ops.in_set_plan(list(range(4096)) + [262144], pa.int64())
    assert p["range"] == 262145 and p["route"] == "in_set:bitmap_global"
    p = ops.in_set_plan(list(range(4096)) + [262144], pa.uint64())
    assert p["domain"] == L.IN_DOM_U64 and p["route"] == "in_set:bitmap_global"


def test_route_sorted_table_of_4096_and_4097_members():
    assert ops.in_set_plan([i * 1000 for i in range(4096)], pa.int64())["route"] == "in_set:sorted_lds"
    assert ops.in_set_plan([i * 1000 for i in range(4097)], pa.int64())["route"] == "in_set:sorted_global"
    # the float64 domain has no bitmap, however dense
    assert ops.in_set_plan(list(range(4096)), pa.float64())["route"] == "in_set:sorted_lds"
    assert ops.in_set_plan(list(range(4097)), pa.float64())["route"] == "in_set:sorted_global"
    # members are counted after canonicalisation
    assert ops.in_set_plan([i * 1000 for i in range(4096)] * 2, pa.int64())["route"] == "in_set:sorted_lds"


def test_route_int64_extremes_do_not_overflow():
    p = ops.in_set_plan([I64_MAX, 0, I64_MIN], pa.int64())
    assert p["table"].tolist() == [I64_MIN, 0, I64_MAX] and p["route"] == "in_set:sorted_lds"
    p = ops.in_set_plan([I64_MAX, I64_MAX - 1], pa.int64())
    assert p["route"] == "in_set:bitmap_lds" and p["range"] == 2
    p = ops.in_set_plan([I64_MIN, I64_MIN + 100], pa.int64())
    assert p["route"] == "in_set:bitmap_lds" and p["range"] == 101


def test_empty_list_is_an_error():
    with pytest.raises(ValueError, match="IN with an empty list"):
        ops.in_set_plan([], pa.int64())
    with pytest.raises(ValueError, match="IN with an empty list"):
        ops.InSet([])
    import ctypes
    h = ctypes.c_void_p(0)
    assert L.load().vnm_in_set_create(0, None, 0, ctypes.byref(h)) != 0
    assert "ValueError: IN with an empty list" in L.last_error()
    assert L.load().vnm_in_set_plan_host(0, None, 0, L.I64, 0, None, None, None, None, None) != 0


# ---- which lists become sets ---------------------------------------------------------------------------------------------------
def _ins(prog):
    return [(i.op, i.arg, i.imm_f, i.imm_i) for i in prog]


def _chain(col, vals, op="in"):
    """the parent commit's program for a bare list: column, strong constant, == per member, OR between them"""
    out = []
    for k, v in enumerate(vals):
        out += [(L.EX_COL, 0, 0.0, 0), (L.EX_CONST_I, 1, 0.0, v), (L.EX_EQ if op == "in" else L.EX_NE, 0, 0.0, 0)]
        if k:
            out.append((L.EX_OR if op == "in" else L.EX_AND, 0, 0.0, 0))
    return out


class _FakeColumn:
    vnm_type = L.I64
    length = 10


@pytest.fixture
def fake_probe(monkeypatch):
    calls = []

    def probe(col, values, invert=False, length=None, stream=None):
        calls.append((col, tuple(values), length))
        return ("mask", len(calls) - 1)
    monkeypatch.setattr(ops, "in_set_probe", probe)
    monkeypatch.setenv("VNM_IN_SET_MIN", "17")       # the first length whose bare chain no longer compiles
    return calls


def test_default_threshold(fake_probe, monkeypatch):
    """profiles/r09_in_set.txt: from 4 members on the set route beats the chain beyond the spread; 2 and 3 members keep the chain"""
    monkeypatch.delenv("VNM_IN_SET_MIN", raising=False)
    assert ops.in_set_min() == 4
    expr = ("in", "k", (1, 2, 3))
    assert ops.lower_in_sets(expr, {"k": _FakeColumn()}, 10) == (expr, {}) and not fake_probe
    assert ops.lower_in_sets(("in", "k", (1, 2, 3, 4)), {"k": _FakeColumn()}, 10)[0] == ("ne", "__in_0", 0)


@pytest.mark.parametrize("op", ["in", "not_in"])
def test_sixteen_members_keep_the_chain(fake_probe, op):
    vals = tuple(range(100, 116))
    expr = (op, "k", vals)
    assert ops.lower_in_sets(expr, {"k": _FakeColumn()}, 10) == (expr, {})
    assert not fake_probe
    prog = ops.compile_expr(expr, {"k": 0})
    assert len(prog) == 63 and _ins(prog) == _chain("k", vals, op)


def test_seventeen_members_become_a_mask_column(fake_probe):
    vals = tuple(range(17))
    k = _FakeColumn()
    got, extra = ops.lower_in_sets(("and", ("in", "k", vals), ("gt", "k", 3)), {"k": k}, 10)
    assert got == ("and", ("ne", "__in_0", 0), ("gt", "k", 3))
    assert extra == {"__in_0": ("mask", 0)} and fake_probe == [(k, vals, 10)]
    got, extra = ops.lower_in_sets(("not_in", "k", vals), {"k": k}, 10)
    assert got == ("eq", "__in_0", 0)


def test_two_ten_member_lists_rewrite_the_longer_first(fake_probe):
    a, b = tuple(range(10)), tuple(range(11))
    expr = ("and", ("in", "x", a), ("in", "y", b))
    with pytest.raises(L.VinumHipError, match="1..63 instructions"):       # what the parent commit does with it
        ops.result_type(("and",) + tuple(E.desugar(e) for e in expr[1:]), {"x": (pa.int64(), False), "y": (pa.int64(), False)})
    x, y = _FakeColumn(), _FakeColumn()
    got, extra = ops.lower_in_sets(expr, {"x": x, "y": y}, 10)
    assert got == ("and", ("in", "x", a), ("ne", "__in_0", 0)) and fake_probe == [(y, b, 10)]
    assert len(ops.compile_expr(got, {"x": 0, "__in_0": 1})) + 1 <= ops.PJ_MAX_INS
    # three of them: the two longest go, the shortest stays a chain
    c = tuple(range(12))
    got, extra = ops.lower_in_sets(("and", ("in", "x", a), ("in", "y", b), ("in", "x", c)), {"x": x, "y": y}, 10)
    assert got == ("and", ("in", "x", a), ("ne", "__in_0", 0), ("ne", "__in_1", 0))      # (masks are numbered in tree order)
    assert [v for _, v, _ in fake_probe[1:]] == [b, c]
    # the type check sees the same program
    assert ops.result_type(expr, {"x": (pa.int64(), False), "y": (pa.int32(), True)}) == pa.uint8()


def test_in_set_min_two_rewrites_everything(fake_probe, monkeypatch):
    monkeypatch.setenv("VNM_IN_SET_MIN", "2")
    assert ops.in_set_min() == 2
    got, extra = ops.lower_in_sets(("or", ("in", "k", (1, 2)), ("not_in", "k", (3, 4, 5)), ("in", "k", (6,))), {"k": _FakeColumn()}, 10)
    assert got == ("or", ("ne", "__in_0", 0), ("eq", "__in_1", 0), ("in", "k", (6,)))
    monkeypatch.setenv("VNM_IN_SET_MIN", "1")
    got, extra = ops.lower_in_sets(("in", "k", (6,)), {"k": _FakeColumn()}, 10)
    assert got == ("ne", "__in_0", 0)


def test_result_type_of_long_lists(monkeypatch):
    monkeypatch.setenv("VNM_IN_SET_MIN", "17")
    types = {"k": (pa.int64(), False), "h": (pa.int8(), False)}
    assert ops.result_type(("in", "k", tuple(range(1000))), types) == pa.uint8()
    assert ops.result_type(("to_int", ("not_in", ("add", "k", 1), tuple(range(1000)))), types) == pa.int64()
    with pytest.raises(TypeError, match="float16"):
        ops.result_type(("in", ("sqrt", "h"), tuple(range(17))), types)
    with pytest.raises(TypeError, match="predicate"):
        ops.result_type(("in", ("gt", "k", 1), tuple(range(17))), types)


def test_aggregate_projects_an_input_holding_a_long_list(monkeypatch):
    from vinum_amd.core.aggregate import _has_cast
    monkeypatch.setenv("VNM_IN_SET_MIN", "17")
    assert _has_cast(("mul", "v", ("to_float", ("in", "k", tuple(range(17))))))
    assert _has_cast(("in", "k", tuple(range(17))))
    assert not _has_cast(("in", "k", tuple(range(16))))
    assert not _has_cast(("mul", "v", ("add", "k", 1)))
    assert _has_cast(("and", ("in", "x", tuple(range(10))), ("in", "y", tuple(range(11)))))     # does not fit: one list goes
    assert _has_cast(("like", "s", ("lit", "a%")))


def test_binding_round_trips_a_thousand_members():
    from vinum_amd import binding as B
    from vinum_amd.planner import _t
    vals = tuple(range(0, 3000, 3))
    for expr in (("in", "k", vals), ("and", ("not_in", ("add", "k", 1), vals), ("gt", "k", 5)),
                 ("in", "s", tuple(f"city{i}" for i in range(1000)))):
        assert B.lower(B.vectorize(expr)) == expr
    assert _t(["in", "k", list(vals)]) == ("in", "k", vals)
    assert ops.columns_of(("in", ("add", "a", "b"), vals)) == ["a", "b"]


def test_handle_cache_is_a_small_lru(monkeypatch):
    closed = []
    real = ops.InSet.close

    def close(self):
        if self.ptr:
            closed.append(id(self))
        real(self)
    monkeypatch.setattr(ops.InSet, "close", close)
    ops.in_set_cache_clear()
    first = ops.in_set((1, 2, 3))
    assert ops.in_set([1, 2, 3]) is first and not first.is_float
    assert ops.in_set((1.0, 2, 3)) is not first and ops.in_set((1.0, 2, 3)).is_float
    for k in range(ops._IN_SET_CACHE_SIZE):
        ops.in_set((k, k + 1))
    assert id(first) in closed and first.ptr is None
    assert len(ops._in_sets) == ops._IN_SET_CACHE_SIZE
    ops.in_set_cache_clear()
