"""date() / datetime() / from_timestamp() without a GPU: the node forms of vinum_amd.expr, core.lowering.lower_case_functions over
stub columns (a string column is parsed through its dictionary, a temporal column rescaled, an integer column retyped, a literal
folded by NumPy), units and their errors, the plan-time refusals, the alignment of comparisons to the finer unit, and the adapter
by qualified class name.

On the parent commit P._t(["fn", "date", "d"]) stays the unknown function ("fn", "date", "d"), expr has no fold_temporal and the
lowering knows no such node."""
import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import binding as B
from vinum_amd import expr as E
from vinum_amd import keydict as K
from vinum_amd import planner as P
from vinum_amd.core import lowering
from vinum_amd.core.lowering import lower_case_functions, lower_dictionary


class StubDict:
    """what the lowering asks of a KeyDictionary"""

    def __init__(self, name, arrow_type=pa.string(), on_device=True):
        self.name, self.type, self.on_device = name, arrow_type, on_device
        self.value_type = arrow_type.value_type if pa.types.is_dictionary(arrow_type) else arrow_type
        self.calls = []

    def parsed_column(self, unit, col):
        self.calls.append((unit, col.name))
        return StubColumn(f"{unit}({col.name})", None, K.temporal_type(unit))

    def affixed_column(self, prefix, suffix, col):
        return StubColumn(f"[{prefix.decode()}{col.name}{suffix.decode()}]", StubDict(f"affix({self.name})"))

    def mapped_column(self, fn, col):
        return StubColumn(f"{fn}({col.name})", StubDict(f"{fn}({self.name})"))

    def pair_column(self, other, prefix, sep, suffix, a, b):
        return StubColumn(f"[{a.name}{sep.decode()}{b.name}]", StubDict("pair"))


class StubColumn:
    length, value_tables, vnm_type = 10, None, 3

    def __init__(self, name, dictionary=None, arrow_type=pa.int32()):
        self.name, self.dictionary, self.arrow_type = name, dictionary, arrow_type


@pytest.fixture
def columns(monkeypatch):
    calls = []

    def rescaled(col, unit):
        if K.temporal_unit(col.arrow_type) == unit:
            return col
        calls.append(("rescale", col.name, unit))
        return StubColumn(f"{unit}({col.name})", None, K.temporal_type(unit))

    def retyped(col, unit):
        calls.append(("retype", col.name, unit))
        return StubColumn(f"ts_{unit}({col.name})", None, pa.timestamp(unit))
    monkeypatch.setattr(K, "rescaled_column", rescaled)
    monkeypatch.setattr(K, "timestamp_column", retyped)
    num = lambda n, t: StubColumn(n, None, t)
    cols = {"d": StubColumn("d", StubDict("D")), "dd": StubColumn("dd", StubDict("DD", pa.dictionary(pa.int8(), pa.string()))),
            "ym": StubColumn("ym", StubDict("YM", pa.large_string())), "day": num("day", pa.date32()), "ts": num("ts", pa.timestamp("s")),
            "ms": num("ms", pa.timestamp("ms")), "i": num("i", pa.int64()), "i32": num("i32", pa.int32()), "u64": num("u64", pa.uint64()),
            "f": num("f", pa.float64())}
    cols["__calls__"] = calls
    return cols


# ---- the node forms ---------------------------------------------------------------------------------------------------------------------
def test_the_unit_is_no_operand():
    node = ("datetime", "d", ("lit", "ms"))
    assert E.operands(node) == ("d",) and E.columns_of(("ge", node, ("date", ("lit", "2020-10-09")))) == ["d"]
    assert E.operands(("temporal", 5, "D")) == () and E.with_operands(node, ["x"]) == ("datetime", "x", ("lit", "ms"))
    assert P._t(["fn", "date", "d"]) == ("date", "d") and P._t(["fn", "DATETIME", "d", ["lit", "us"]]) == ("datetime", "d", ("lit", "us"))
    assert P._t(["fn", "from_timestamp", "i"]) == ("from_timestamp", "i")
    for name in ("date", "datetime", "from_timestamp"):
        assert P.SCALAR_FN_NAMES[name] == name
    assert P.output_names([P._raw(["fn", "date", "d"])], [None]) == ["date"]


def test_units_and_their_errors():
    assert E.temporal_unit_arg(("date", "d")) == "D" and E.temporal_unit_arg(("datetime", "d")) is None
    assert E.temporal_unit_arg(("from_timestamp", "i")) == "s" and E.temporal_unit_arg(("from_timestamp", "i", ("lit", "ns"))) == "ns"
    for unit in ("D", "s", "ms", "us", "ns"):
        assert E.temporal_unit_arg(("datetime", "d", ("lit", unit))) == unit
    with pytest.raises(ValueError, match=r"Unsupported DatetimeFunction unit: 'h'. Supported units are: \[D, s, ms, us, ns\]"):
        E.temporal_unit_arg(("datetime", "d", ("lit", "h")))
    with pytest.raises(ValueError, match=r"Unsupported DateFunction unit: 's'. Supported units are: \[D\]"):
        E.temporal_unit_arg(("date", "d", ("lit", "s")))
    with pytest.raises(ValueError, match=r"Unsupported TimestampFunction unit: 'D'. Supported units are: \[s, ms, us, ns\]"):
        E.temporal_unit_arg(("from_timestamp", "i", ("lit", "D")))
    with pytest.raises(ValueError, match="Unsupported DatetimeFunction unit"):
        E.temporal_unit_arg(("datetime", "d", "ms"))             # (a bare str is a column name, no unit)
    with pytest.raises(NotImplementedError, match="3 operand"):
        E.temporal_unit_arg(("datetime", "d", ("lit", "s"), 1))


# ---- literal folding: NumPy itself, with the reference's unit rules (the literal cases of test_query_results.py:1002-1105) ---------------
@pytest.mark.parametrize("node, want", [
    (("date", ("lit", "2020-10-06")), np.datetime64("2020-10-06", "D")),
    (("date", ("lit", "2020-10-06 12:30:00")), np.datetime64("2020-10-06", "D")),
    (("datetime", ("lit", "2020-10-07")), np.datetime64("2020-10-07", "D")),
    (("datetime", ("lit", "2020-10")), np.datetime64("2020-10-01", "D")),                # (M is not listed: the next finer unit, D)
    (("datetime", ("lit", "2020-10-07 19:30")), np.datetime64("2020-10-07T19:30", "s")),  # (m -> s)
    (("datetime", ("lit", "2020-10-07T19")), np.datetime64("2020-10-07T19", "s")),        # (h -> s)
    (("datetime", ("lit", "2020-10-07 19:30:15.5")), np.datetime64("2020-10-07T19:30:15.500", "ms")),
    (("datetime", ("lit", "2020-10-07 19:30"), ("lit", "s")), np.datetime64("2020-10-07T19:30", "s")),
    (("datetime", ("lit", "2020-10-07 19:30:15.123456"), ("lit", "ms")), np.datetime64("2020-10-07T19:30:15.123", "ms")),
    (("datetime", ("lit", "2020-10-07"), ("lit", "ns")), np.datetime64("2020-10-07", "ns")),
    (("from_timestamp", 1602841523), np.datetime64(1602841523, "s")),
    (("from_timestamp", 1602841523123, ("lit", "ms")), np.datetime64(1602841523123, "ms")),
    (("from_timestamp", ("lit", "2020-10-16 09:45:23")), np.datetime64("2020-10-16T09:45:23", "s")),
])
def test_literal_calls_fold_with_numpy(node, want):
    got = E.fold_temporal(node)
    unit = np.datetime_data(want.dtype)[0]
    assert got == ("temporal", int(want.astype(np.int64)), unit)
    assert np.datetime64(got[1], got[2]) == want


def test_literal_folding_leaves_columns_alone_and_raises_numpys_errors():
    assert E.fold_temporal(("date", "d")) is None and E.fold_temporal(("datetime", ("upper", "d"))) is None
    with pytest.raises(ValueError, match="out of range in datetime string"):
        E.fold_temporal(("date", ("lit", "2020-13-45")))
    with pytest.raises(ValueError, match="Error parsing datetime string"):
        E.fold_temporal(("date", ("lit", "2020-1-6")))
    with pytest.raises(NotImplementedError, match="NaT"):
        E.fold_temporal(("datetime", ("lit", "NaT"), ("lit", "s")))


# ---- the lowering -----------------------------------------------------------------------------------------------------------------------
def test_a_string_column_is_parsed_through_its_dictionary(columns):
    e, extra = lower_case_functions(("date", "d"), columns)
    assert e == "__temporal_date_D_d" and extra[e].arrow_type == pa.date32() and extra[e].dictionary is None
    assert columns["d"].dictionary.calls == [("D", "d")]
    e, extra = lower_case_functions(("datetime", "dd"), columns)                  # no unit over a column: timestamp[s]
    assert e == "__temporal_datetime_s_dd" and extra[e].arrow_type == pa.timestamp("s")
    e, extra = lower_case_functions(("datetime", "ym", ("lit", "us")), columns)
    assert extra[e].arrow_type == pa.timestamp("us") and columns["ym"].dictionary.calls == [("us", "ym")]
    e, extra = lower_case_functions(("from_timestamp", "d", ("lit", "ms")), columns)
    assert extra[e].arrow_type == pa.timestamp("ms")


def test_it_nests_with_the_string_functions_both_ways(columns, monkeypatch):
    e, extra = lower_case_functions(("date", ("concat", "ym", ("lit", "-01"))), columns)
    inner = next(n for n in extra if n.startswith("__concat("))
    assert e == f"__temporal_date_D_{inner}" and extra[e].name == "D([ym-01])"
    seen = []

    class Table:                      # stands where keydict.ValueTable stands: to_str() of the derived date32 column is a value table
        @classmethod
        def of(cls, col, name=None):
            seen.append((name, str(col.arrow_type)))
            return cls()

        def column(self, col):
            return StubColumn(f"str({col.name})", StubDict("values"))
    monkeypatch.setattr(lowering, "ValueTable", Table)
    e, extra = lower_case_functions(("to_str", ("date", "d")), columns)
    assert e == "__to_str___temporal_date_D_d" and extra[e].name == "str(D(d))" and seen == [("__temporal_date_D_d", "date32[day]")]


def test_a_repeated_node_is_materialised_once(columns):
    extra = {}
    node = ("date", "d")
    lower_dictionary(("ge", node, ("date", ("lit", "2020-10-09"))), columns, extra)
    lower_dictionary(("is_null", node), columns, extra)
    lower_dictionary(node, columns, extra)
    assert columns["d"].dictionary.calls == [("D", "d")]


def test_temporal_and_integer_columns(columns):
    calls = columns["__calls__"]
    assert lower_case_functions(("date", "day"), columns) == ("day", {})                   # already the target: the column itself
    assert lower_case_functions(("datetime", "ts"), columns) == ("ts", {})
    e, extra = lower_case_functions(("date", "ts"), columns)
    assert extra[e].arrow_type == pa.date32() and calls == [("rescale", "ts", "D")]
    e, extra = lower_case_functions(("datetime", "day", ("lit", "ms")), columns)
    assert extra[e].arrow_type == pa.timestamp("ms") and calls[-1] == ("rescale", "day", "ms")
    e, extra = lower_case_functions(("from_timestamp", "i"), columns)
    assert extra[e].arrow_type == pa.timestamp("s") and calls[-1] == ("retype", "i", "s")
    e, extra = lower_case_functions(("from_timestamp", "i32", ("lit", "ns")), columns)
    assert extra[e].arrow_type == pa.timestamp("ns") and calls[-1] == ("retype", "i32", "ns")


def test_refusals_of_the_lowering(columns):
    with pytest.raises(TypeError, match="from_timestamp.*'f' is double"):
        lower_case_functions(("from_timestamp", "f"), columns)
    with pytest.raises(TypeError, match="from_timestamp.*'u64' is uint64"):
        lower_case_functions(("from_timestamp", "u64"), columns)
    with pytest.raises(TypeError, match="date.*'i' is int64"):
        lower_case_functions(("date", "i"), columns)
    with pytest.raises(ValueError, match="Unsupported DatetimeFunction unit: 'h'"):
        lower_case_functions(("datetime", "d", ("lit", "h")), columns)
    with pytest.raises(NotImplementedError, match="no GPU lowering for date\\(\\) over"):
        lower_case_functions(("date", ("add", "i", 1)), columns)
    for alone in (("date", ("lit", "2020-10-06")), ("add", ("from_timestamp", 5), 1)):
        with pytest.raises(NotImplementedError, match="temporal constant"):
            lower_case_functions(alone, columns)


def test_the_real_dictionary_refuses_binary_and_host_route_columns():
    with pytest.raises(TypeError, match="need a string column, not binary"):
        K.KeyDictionary(pa.binary()).parsed("D")
    with pytest.raises(NotImplementedError, match="only string columns keep their dictionaries on the device"):
        K.KeyDictionary(pa.dictionary(pa.int8(), pa.bool_())).parsed("s")
    with pytest.raises(ValueError, match="no temporal unit 'h'"):
        K.KeyDictionary(pa.string()).parsed("h")


# ---- comparisons are aligned to the finer unit --------------------------------------------------------------------------------------------
def test_comparisons_with_a_constant_are_aligned_to_the_finer_unit(columns):
    day = int(np.datetime64("2020-10-09", "D").astype(np.int64))
    sec = int(np.datetime64("2020-10-07T19:30", "s").astype(np.int64))
    # same unit: the constant's count
    e, _ = lower_case_functions((">=", ("date", "d"), ("date", ("lit", "2020-10-09"))), columns)
    assert e == (">=", "__temporal_date_D_d", ("strong", day))
    # a date32 column against an `s` constant: the COLUMN is scaled
    e, _ = lower_case_functions(("lt", "day", ("datetime", ("lit", "2020-10-07 19:30"), ("lit", "s"))), columns)
    assert e == ("lt", ("mul", "day", ("strong", 86400)), ("strong", sec))
    # an `s` column against a `D` constant: the CONSTANT is scaled
    e, _ = lower_case_functions(("eq", "ts", ("date", ("lit", "2020-10-09"))), columns)
    assert e == ("eq", "ts", ("strong", day * 86400))
    # the constant on the left; ms column against an s constant
    e, _ = lower_case_functions(("le", ("from_timestamp", 1602841523), "ms"), columns)
    assert e == ("le", ("strong", 1602841523000), "ms")
    # two columns of different units: the coarser is scaled; equal units stay as they are
    e, _ = lower_case_functions(("gt", "ts", "ms"), columns)
    assert e == ("gt", ("mul", "ts", ("strong", 1000)), "ms")
    node = ("gt", "ts", "ts")
    assert lower_case_functions(node, columns)[0] is node
    # what NumPy says of the same comparison
    assert (np.datetime64("2020-10-09", "D") == np.datetime64(day * 86400, "s")) and (np.datetime64("2020-10-09", "D") > np.datetime64(sec, "s"))


def test_between_follows_through_the_same_alignment(columns):
    lo, hi = (int(np.datetime64(s, "D").astype(np.int64)) for s in ("2020-10-06", "2020-10-09"))
    e, _ = lower_case_functions(("between", ("date", "d"), ("date", ("lit", "2020-10-06")), ("date", ("lit", "2020-10-09"))), columns)
    assert e == ("and", ("ge", "__temporal_date_D_d", ("strong", lo)), ("le", "__temporal_date_D_d", ("strong", hi)))
    e, _ = lower_case_functions(("not_between", "ts", ("date", ("lit", "2020-10-06")), ("date", ("lit", "2020-10-09"))), columns)
    assert e == ("or", ("lt", "ts", ("strong", lo * 86400)), ("gt", "ts", ("strong", hi * 86400)))
    node = ("between", "i", 1, 5)
    assert lower_case_functions(node, columns)[0] is node


def test_a_constant_against_a_number_or_another_constant_is_refused(columns):
    with pytest.raises(TypeError, match="cannot compare the temporal constant"):
        lower_case_functions(("eq", "i", ("date", ("lit", "2020-10-09"))), columns)
    with pytest.raises(TypeError, match="cannot compare the temporal constant"):
        lower_case_functions(("eq", ("date", ("lit", "2020-10-09")), 18544), columns)
    with pytest.raises(NotImplementedError, match="two temporal constants"):
        lower_case_functions(("eq", ("date", ("lit", "2020-10-09")), ("date", ("lit", "2020-10-09"))), columns)
    with pytest.raises(OverflowError):
        lower_case_functions(("eq", ("datetime", "d", ("lit", "ns")), ("date", ("lit", "9999-01-01"))), columns)


# ---- plan time ----------------------------------------------------------------------------------------------------------------------------
def _table():
    return pa.table({"d": pa.array(["2020-10-08 03:26:54"]), "raw": pa.array([b"x"]), "flag": pa.array([True]).dictionary_encode(),
                     "f": pa.array([1.5]), "u64": pa.array([1], pa.uint64()), "i": pa.array([1]), "ts": pa.array([1], pa.timestamp("s"))})


@pytest.mark.parametrize("select, exc, text", [
    (["fn", "from_timestamp", "f"], TypeError, "from_timestamp.*'f' is double"),
    (["fn", "from_timestamp", "u64"], TypeError, "'u64' is uint64"),
    (["fn", "date", "raw"], TypeError, "date.*'raw' is binary"),
    (["fn", "datetime", "flag"], NotImplementedError, "only string columns keep their dictionaries on the device"),
    (["fn", "datetime", "d", ["lit", "h"]], ValueError, "Unsupported DatetimeFunction unit: 'h'"),
    (["fn", "date", "i"], TypeError, "'i' is int64"),
    (["fn", "date", ["lit", "2020-02-30"]], ValueError, "out of range in datetime string"),
])
def test_plan_time_refusals(select, exc, text):
    with pytest.raises(exc, match=text):
        P.plan_query({"select": [select]}, _table())


def test_plan_time_accepts_what_runs():
    for select in (["fn", "date", "d"], ["fn", "datetime", "d", ["lit", "ms"]], ["fn", "from_timestamp", "i"], ["fn", "date", "ts"],
                   ["fn", "from_timestamp", "d"]):
        plan = P.plan_query({"select": [select], "where": [">=", ["fn", "date", "d"], ["fn", "date", ["lit", "2020-10-09"]]]}, _table())
        assert plan.steps[0][0] == "read" and "d" in plan.steps[0][1]


# ---- the adapter --------------------------------------------------------------------------------------------------------------------------
def test_the_binding_lowers_the_classes_by_qualified_name():
    assert B.lower(B.DateFunction([B.Column("d")])) == ("date", "d")
    assert B.lower(B.DatetimeFunction([B.Column("d"), B.Literal("ms")])) == ("datetime", "d", ("lit", "ms"))
    assert B.lower(B.TimestampFunction([B.Literal(1602841523)])) == ("from_timestamp", 1602841523)
    assert B.lower(B.DateFunction([B.Literal("2020-10-06")])) == ("date", ("lit", "2020-10-06"))
    for name, cls in (("date", B.DateFunction), ("datetime", B.DatetimeFunction), ("from_timestamp", B.TimestampFunction)):
        built = B.vectorize((name, "d"))
        assert type(built) is cls and B.lower(built) == (name, "d")
    # a reference-shaped class of that name, defined at module level elsewhere
    ref = type("DateFunction", (B.VectorizedExpression,), {"__init__": lambda self, arguments: B.VectorizedExpression.__init__(self, arguments)})
    assert ref.__qualname__ == "DateFunction" and B.lower(ref([B.Column("d")])) == ("date", "d")


def test_an_impostor_named_like_the_class_still_raises():
    class Other(B.VectorizedExpression):
        pass
    node = Other([B.Column("s")])
    node.__class__.__name__ = "DateFunction"
    with pytest.raises(NotImplementedError, match="no GPU lowering.*now, timedelta, is_busday"):
        B.lower(node)
