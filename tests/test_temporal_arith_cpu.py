"""Arithmetic on temporal values, timedelta(), is_busday(), now() and IN lists of temporal constants without a GPU: the type rules of
core.lowering.TemporalArithmetic held against NumPy's own datetime64 / timedelta64 arithmetic on one-element arrays, the lowered forms
(factors and constant of vnm_temporal_affine), the constant folds, the unit rules of timedelta(), now() folded once per query, the
calendar of is_busday() against np.busdaycalendar, the adapter round trips and the plan-time refusals.

On the parent commit expr has no fold_timedelta / fold_now, the lowering raises "arithmetic on temporal values is not built" for every
constant outside a comparison and lowers column arithmetic onto the untyped interpreter, and the adapter refuses the three names."""
import itertools
import time

import numpy as np
import pyarrow as pa
import pytest

from vinum_amd import binding as B
from vinum_amd import expr as E
from vinum_amd import keydict as K
from vinum_amd import planner as P
from vinum_amd.core import lowering
from vinum_amd.core.lowering import lower_case_functions


class StubDict:
    on_device = True

    def __init__(self, arrow_type=pa.string()):
        self.type = self.value_type = arrow_type


class StubColumn:
    length, value_tables, vnm_type = 10, None, 3

    def __init__(self, name, arrow_type, dictionary=None):
        self.name, self.arrow_type, self.dictionary = name, arrow_type, dictionary


T_UNITS = ("D", "s", "ms", "us", "ns")
D_UNITS = ("s", "ms", "us", "ns")


@pytest.fixture
def columns(monkeypatch):
    """t<unit>: date32 / timestamp columns, d<unit>: duration columns, i / f / txt: an int64, a float64 and a string column; the
    kernels' host wrappers record their calls and return a column of the type they were asked for"""
    calls = []

    def affine(a, ka, b, kb, c, t):
        calls.append((a.name, ka, b.name if b is not None else None, kb, c, t))
        return StubColumn(f"affine{len(calls)}", t)

    def busday(col, weekmask, holidays):
        calls.append(("busday", col.name, weekmask, holidays))
        return StubColumn(f"busday{len(calls)}", pa.uint8())

    def rescaled(col, unit):
        if K.temporal_unit(col.arrow_type) == unit:
            return col
        calls.append(("rescale", col.name, unit))
        return StubColumn(f"{unit}({col.name})", K.temporal_type(unit))
    def floordiv(a, ka, b, kb):
        calls.append(("floordiv", a.name if a is not None else None, ka, b.name if b is not None else None, kb))
        return StubColumn(f"floordiv{len(calls)}", pa.int64())
    monkeypatch.setattr(K, "affine_column", affine)
    monkeypatch.setattr(K, "floordiv_column", floordiv)
    monkeypatch.setattr(K, "busday_mask", busday)
    monkeypatch.setattr(K, "rescaled_column", rescaled)
    cols = {f"t{u}": StubColumn(f"t{u}", K.temporal_type(u)) for u in T_UNITS}
    cols.update({f"d{u}": StubColumn(f"d{u}", pa.duration(u)) for u in D_UNITS})
    cols.update({"i": StubColumn("i", pa.int64()), "f": StubColumn("f", pa.float64()), "txt": StubColumn("txt", pa.int32(), StubDict())})
    cols["__calls__"] = calls
    return cols


# ---- NumPy parity of the rules ------------------------------------------------------------------------------------------------------------
# an operand: (the node, the one-element NumPy array it stands for)
def _operands():
    out = []
    for u in T_UNITS:
        out.append((f"t{u}", np.array([100], dtype=f"datetime64[{u}]")))
    for u in D_UNITS:
        out.append((f"d{u}", np.array([7], dtype=f"timedelta64[{u}]")))
    for u in ("W", "D", "h", "m", "s", "ms", "us", "ns"):
        out.append((("timedelta", 3, ("lit", u)), np.array([3], dtype=f"timedelta64[{u}]")))
    out.append((("datetime", ("lit", "2020-10-09"), ("lit", "D")), np.array(["2020-10-09"], dtype="datetime64[D]")))
    out.append((("datetime", ("lit", "2020-10-09 01:02:03"), ("lit", "ms")), np.array(["2020-10-09 01:02:03"], dtype="datetime64[ms]")))
    out.append(("i", np.array([5], dtype=np.int64)))
    out.append(("f", np.array([1.5])))
    out.append(("txt", np.array(["x"])))
    out.append((4, 4))
    out.append((2.5, 2.5))
    return out


_NP_OP = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "floordiv": np.floor_divide}
# what this project refuses (or does not build) though NumPy computes it: DESIGN.md section 4.9i
_UNIT_OUT = {"W": "D", "h": "s", "m": "s"}


def _numpy_kind(r):
    """(kind, unit) of a NumPy result as the rules state it: h / m -> s, W -> D, a duration in days -> s"""
    name = r.dtype.name
    unit = name[name.index("[") + 1:name.index("]")] if "[" in name else None
    unit = _UNIT_OUT.get(unit, unit)
    if r.dtype.kind == "m" and unit == "D":
        unit = "s"
    return {"M": "temporal", "m": "duration"}.get(r.dtype.kind, r.dtype.kind), unit


def _lowered_kind(e, columns, extra):
    if isinstance(e, str):
        t = (extra[e] if e in extra else columns[e]).arrow_type
        return ("temporal", K.temporal_unit(t)) if K.temporal_unit(t) else ("duration", K.duration_unit(t))
    assert isinstance(e, tuple)
    if e[0] in ("temporal", "duration"):
        unit = e[2]
        return e[0], "s" if e[0] == "duration" and unit == "D" else unit
    return e[0], None


def _is_temporal(v):
    return isinstance(v, np.ndarray) and v.dtype.kind in "Mm"


@pytest.mark.parametrize("op", ["add", "sub", "mul", "div", "floordiv"])
def test_every_pair_of_operands_types_as_numpy_does(columns, op):
    checked = raised = 0
    for (a, na), (b, nb) in itertools.product(_operands(), repeat=2):
        if not (_is_temporal(na) or _is_temporal(nb)):
            continue
        node = (op, a, b)
        try:
            with np.errstate(all="ignore"):
                want = _NP_OP[op](na, nb)
        except TypeError:                                  # UFuncTypeError and its "no loop" kin
            raised += 1
            with pytest.raises(TypeError):
                lower_case_functions(node, columns)
            continue
        both_const = not isinstance(a, str) and not isinstance(b, str)
        try:
            e, extra = lower_case_functions(node, columns)
        except (TypeError, NotImplementedError) as exc:
            # stricter than NumPy, by the issue's table: an integer COLUMN is a generic timedelta under + and - only, duration * float
            # and duration / number (// number) are out of scope, and a constant alone has no per-row work
            strict = ("i" in (a, b) or isinstance(a, float) or isinstance(b, float) or "f" in (a, b) or (op in ("div", "floordiv") and (a == 4 or b == 4))
                      or both_const)
            assert strict, (node, exc)
            continue
        checked += 1
        if op == "floordiv":                                # int64: a constant folded by NumPy itself, else the kernel's column
            assert want.dtype == np.int64 and (e == ("strong", int(want[0])) if both_const else extra[e].arrow_type == pa.int64()), node
            continue
        if op == "div" and both_const:                      # folded by NumPy itself: a float64 number
            assert e == ("strong", float(want[0])), node
            continue
        if op == "div":
            assert want.dtype == np.float64 and e[0] == "div", node
            for side in e[1:]:                              # both sides in ONE unit: the finer one
                assert (isinstance(side, tuple) and side[0] == "strong") or _lowered_kind(side, columns, extra)[0] == "duration"
            units = {_lowered_kind(s, columns, extra)[1] for s in e[1:] if isinstance(s, str)}
            assert len(units) == 1, node
            continue
        assert _lowered_kind(e, columns, extra) == _numpy_kind(want), (node, e, want.dtype)
    assert checked >= (60 if op in ("add", "sub") else 8) and raised >= 20, (checked, raised)


def test_constants_among_themselves_fold_with_numpy(columns):
    for op in ("add", "sub"):
        for (a, na), (b, nb) in itertools.product([o for o in _operands() if isinstance(o[0], tuple)], repeat=2):
            try:
                want = _NP_OP[op](na, nb)
            except TypeError:
                with pytest.raises(TypeError):
                    lower_case_functions((op, a, b), columns)
                continue
            # a constant alone is refused (no per-row work), so fold it inside a comparison with a column of its kind
            col = "tns" if want.dtype.kind == "M" else "dns"
            e, _ = lower_case_functions(("eq", col, (op, a, b)), columns)
            assert e == ("eq", col, ("strong", int(want.astype(f"{want.dtype.kind}8[ns]").astype(np.int64)[0]))), (op, a, b)
    week_ago = int((np.datetime64("2020-10-09", "D") - np.timedelta64(7, "D")).astype(np.int64))
    e, _ = lower_case_functions((">=", "tD", ("sub", ("date", ("lit", "2020-10-09")), ("timedelta", 7, ("lit", "D")))), columns)
    assert e == (">=", "tD", ("strong", week_ago))
    e, _ = lower_case_functions(("lt", "ds", ("mul", ("timedelta", 2, ("lit", "h")), 3)), columns)
    assert e == ("lt", "ds", ("strong", 6 * 3600))
    e, _ = lower_case_functions(("lt", "ds", ("neg", ("timedelta", 2, ("lit", "m")))), columns)
    assert e == ("lt", "ds", ("strong", -120))
    assert not columns["__calls__"]


def test_negation(columns):
    e, extra = lower_case_functions(("neg", "dms"), columns)
    assert extra[e].arrow_type == pa.duration("ms") and columns["__calls__"] == [("dms", -1, None, 0, 0, pa.duration("ms"))]
    assert (-np.array([7], dtype="timedelta64[ms]")).dtype == np.dtype("timedelta64[ms]")
    with pytest.raises(TypeError):
        np.negative(np.array([7], dtype="datetime64[s]"))
    with pytest.raises(TypeError, match="neg.*datetime64\\[s\\]"):
        lower_case_functions(("neg", "ts"), columns)


# ---- the lowered forms --------------------------------------------------------------------------------------------------------------------
def test_lowered_forms(columns):
    calls = columns["__calls__"]
    day = lambda s: int(np.datetime64(s, "D").astype(np.int64))

    def form(node):
        del calls[:]
        e, extra = lower_case_functions(node, columns)
        return e, extra, list(calls)
    # two columns of different units: the coarser side carries the factor, subtraction is kb = -k
    e, extra, got = form(("sub", "ts", "tms"))
    assert got == [("ts", 1000, "tms", -1, 0, pa.duration("ms"))] and e.startswith("__temporal_affine") and extra[e].arrow_type == pa.duration("ms")
    e, extra, got = form(("-", "tD", "tns"))
    assert got == [("tD", 86_400 * 10**9, "tns", -1, 0, pa.duration("ns"))]
    # D - D is a duration in seconds
    assert form(("sub", "tD", "tD"))[2] == [("tD", 86400, "tD", -86400, 0, pa.duration("s"))]
    # a date and whole days stays a date; hours make it a timestamp[s]
    assert form(("sub", "tD", ("timedelta", 7, ("lit", "D"))))[2] == [("tD", 1, None, 0, -7, pa.date32())]
    assert form(("add", "tD", ("timedelta", 2, ("lit", "W"))))[2] == [("tD", 1, None, 0, 14, pa.date32())]
    assert form(("add", "tD", ("timedelta", 1, ("lit", "h"))))[2] == [("tD", 86400, None, 0, 3600, pa.timestamp("s"))]
    assert form(("add", ("timedelta", 1, ("lit", "ms")), "ts"))[2] == [("ts", 1000, None, 0, 1, pa.timestamp("ms"))]
    # const - column: ka = -1 (times the unit factor), c = the constant
    assert form(("sub", ("date", ("lit", "2021-01-01")), "tD"))[2] == [("tD", -86400, None, 0, day("2021-01-01") * 86400, pa.duration("s"))]
    assert form(("sub", ("date", ("lit", "2021-01-01")), "tms"))[2] == [("tms", -1, None, 0, day("2021-01-01") * 86_400_000, pa.duration("ms"))]
    # an integer literal is in the column's own unit; so is timedelta(n) without one
    assert form(("add", "tms", 5))[2] == [("tms", 1, None, 0, 5, pa.timestamp("ms"))]
    assert form(("sub", "tD", ("timedelta", 5)))[2] == [("tD", 1, None, 0, -5, pa.date32())]
    assert form(("add", 5, "tus"))[2] == [("tus", 1, None, 0, 5, pa.timestamp("us"))]
    # duration * integer literal, either order
    assert form(("mul", "dms", 3))[2] == [("dms", 3, None, 0, 0, pa.duration("ms"))]
    assert form(("*", -2, "ds"))[2] == [("ds", -2, None, 0, 0, pa.duration("s"))]
    # durations among themselves
    assert form(("add", "ds", "dus"))[2] == [("ds", 10**6, "dus", 1, 0, pa.duration("us"))]
    # a chain folds left: (ts - tms) + 1 s
    e, extra, got = form(("add", ("sub", "ts", "tms"), ("timedelta", 1, ("lit", "s"))))
    assert got[0] == ("ts", 1000, "tms", -1, 0, pa.duration("ms")) and got[1][1:] == (1, None, 0, 1000, pa.duration("ms"))
    # a node that occurs twice under one `extra` is computed once
    del calls[:]
    extra = {}
    a, _ = lower_case_functions(("sub", "ts", "tms"), columns, extra)
    b, _ = lower_case_functions(("gt", ("sub", "ts", "tms"), ("timedelta", 30, ("lit", "m"))), columns, extra)
    assert len(calls) == 1 and b == ("gt", a, ("strong", 1_800_000))


def test_comparisons_and_between_of_durations_align_to_the_finer_unit(columns):
    e, _ = lower_case_functions(("gt", ("sub", "ts", "ts"), ("timedelta", 30, ("lit", "m"))), columns)
    assert e[0] == "gt" and e[1].startswith("__temporal_affine") and e[2] == ("strong", 1800)
    assert lower_case_functions(("le", "ds", ("timedelta", 5, ("lit", "ms"))), columns)[0] == ("le", ("mul", "ds", ("strong", 1000)), ("strong", 5))
    assert lower_case_functions(("le", "dms", ("timedelta", 1, ("lit", "D"))), columns)[0] == ("le", "dms", ("strong", 86_400_000))
    assert lower_case_functions(("lt", "ds", "dms"), columns)[0] == ("lt", ("mul", "ds", ("strong", 1000)), "dms")
    assert lower_case_functions(("eq", "dus", ("timedelta", 5)), columns)[0] == ("eq", "dus", ("strong", 5))
    e, _ = lower_case_functions(("between", "ds", ("timedelta", 1, ("lit", "m")), ("timedelta", 1, ("lit", "h"))), columns)
    assert e == ("and", ("ge", "ds", ("strong", 60)), ("le", "ds", ("strong", 3600)))
    with pytest.raises(TypeError, match="a date / timestamp and a duration"):
        lower_case_functions(("gt", "ts", ("timedelta", 30, ("lit", "m"))), columns)
    with pytest.raises(TypeError, match="a date / timestamp and a duration"):
        lower_case_functions(("gt", "ds", "ts"), columns)


def test_division_of_durations(columns):
    e, extra = lower_case_functions(("div", ("sub", "ts", "ts"), ("timedelta", 1, ("lit", "h"))), columns)
    assert e[0] == "div" and extra[e[1]].arrow_type == pa.duration("s") and e[2] == ("strong", 3600)
    del columns["__calls__"][:]
    e, extra = lower_case_functions(("/", "ds", "dms"), columns)
    assert columns["__calls__"] == [("ds", 1000, None, 0, 0, pa.duration("ms"))] and e == ("div", e[1], "dms") and extra[e[1]].arrow_type == pa.duration("ms")
    assert float(np.timedelta64(90, "m") / np.timedelta64(1, "h")) == 1.5


def test_floor_division_of_durations(columns):
    calls = columns["__calls__"]
    e, extra = lower_case_functions(("floordiv", ("sub", "ts", "tms"), ("timedelta", 1, ("lit", "h"))), columns)
    assert extra[e].arrow_type == pa.int64() and calls[-1] == ("floordiv", "affine1", 1, None, 3_600_000)
    lower_case_functions(("//", "ds", "dms"), columns)
    assert calls[-1] == ("floordiv", "ds", 1000, "dms", 1)
    lower_case_functions(("//", ("timedelta", 1, ("lit", "D")), "dus"), columns)
    assert calls[-1] == ("floordiv", None, 86_400 * 10**6, "dus", 1)
    e, _ = lower_case_functions(("gt", ("floordiv", "ds", ("timedelta", 1, ("lit", "m"))), 5), columns)
    assert e[0] == "gt" and e[1].startswith("__temporal_floordiv") and e[2] == 5
    assert (np.array([-7], "m8[s]") // np.timedelta64(2, "s")).tolist() == [-4]
    for node in (("floordiv", "ts", "ds"), ("floordiv", "ds", 2), ("floordiv", "ds", "ts"), ("floordiv", "ts", "ts")):
        with pytest.raises(TypeError, match="cannot use operands with types"):
            lower_case_functions(node, columns)


def test_an_integer_column_is_a_generic_timedelta_under_plus_and_minus(columns):
    calls = columns["__calls__"]
    e, extra = lower_case_functions(("add", "tms", "i"), columns)
    assert calls[-1] == ("tms", 1, "i", 1, 0, pa.timestamp("ms")) and extra[e].arrow_type == pa.timestamp("ms")
    lower_case_functions(("sub", "ds", "i"), columns)
    assert calls[-1] == ("ds", 1, "i", -1, 0, pa.duration("s"))
    assert (np.array([100], "M8[ms]") + np.array([5])).dtype == np.dtype("M8[ms]")
    with pytest.raises(TypeError):
        lower_case_functions(("sub", "i", "ts"), columns)
    # a list of plain integers over a timestamp column stays what it was: the storage integers
    node = ("in", "ts", (1, 2, 3))
    assert lower_case_functions(node, columns)[0] is node


def test_refusals(columns):
    for node in (("add", "ts", "tms"), ("mul", "ts", 2), ("mul", "ts", "ds"), ("div", "ts", 2), ("div", "ts", "ts"), ("mul", "ds", 1.5),
                 ("div", "ds", 2), ("add", "ts", 1.5), ("sub", "ts", "f"), ("add", "txt", "ts"), ("sub", "ds", "ts"), ("sub", 5, "ts"),
                 ("mul", "ds", "ds"), ("mod", "ts", 5), ("add", ("date", ("lit", "2020-01-01")), ("date", ("lit", "2020-01-02")))):
        with pytest.raises(TypeError, match="cannot use operands with types"):
            lower_case_functions(node, columns)
    with pytest.raises(TypeError, match=r"add\(\) cannot use operands with types datetime64\[s\] and datetime64\[ms\]"):
        lower_case_functions(("add", "ts", "tms"), columns)
    with pytest.raises(TypeError, match=r"the string column 'txt'"):
        lower_case_functions(("sub", "ts", "txt"), columns)
    with pytest.raises(OverflowError, match="does not fit int64"):
        lower_case_functions(("sub", "tns", ("date", ("lit", "9999-01-01"))), columns)
    with pytest.raises(TypeError, match="to_str"):                       # to_str of a duration stays refused
        lower_case_functions(("to_str", ("sub", "ts", "tms")), columns)
    for alone in (("timedelta", 5, ("lit", "s")), ("sub", ("date", ("lit", "2020-10-09")), ("timedelta", 7, ("lit", "D")))):
        with pytest.raises(NotImplementedError, match="no GPU lowering for the temporal constant"):
            lower_case_functions(alone, columns)
    with pytest.raises(NotImplementedError, match="folds once per query"):
        lower_case_functions(("gt", "ts", ("now",)), columns)
    # arithmetic without a temporal operand is nobody's business here
    node = ("add", "i", ("mul", "f", 2))
    assert lower_case_functions(node, columns)[0] is node


def test_a_result_is_an_operand_of_date_datetime_and_to_str(columns, monkeypatch):
    e, extra = lower_case_functions(("date", ("add", "ts", ("timedelta", 1, ("lit", "D")))), columns)
    assert e.startswith("__temporal_date_D___temporal_affine") and extra[e].arrow_type == pa.date32()
    assert columns["__calls__"][0] == ("ts", 1, None, 0, 86400, pa.timestamp("s")) and columns["__calls__"][1][0] == "rescale"
    e, extra = lower_case_functions(("is_null", ("sub", "ts", "tms")), columns)
    assert e[0] == "is_null" and extra[e[1]].arrow_type == pa.duration("ms")


# ---- timedelta() --------------------------------------------------------------------------------------------------------------------------
def test_timedelta_units_and_refusals():
    assert E.fold_timedelta(("timedelta", 30, ("lit", "m"))) == ("duration", 1800, "s")
    assert E.fold_timedelta(("timedelta", 2, ("lit", "h"))) == ("duration", 7200, "s")
    assert E.fold_timedelta(("timedelta", 2, ("lit", "W"))) == ("duration", 14, "D")
    assert E.fold_timedelta(("timedelta", -7, ("lit", "D"))) == ("duration", -7, "D")
    for u in ("s", "ms", "us", "ns"):
        assert E.fold_timedelta(("timedelta", 5, ("lit", u))) == ("duration", 5, u)
        assert np.timedelta64(5, u) == E.temporal_scalar(("duration", 5, u))
    assert E.fold_timedelta(("timedelta", 5)) == ("duration", 5, None) and E.fold_timedelta(("timedelta", ("strong", 5))) == ("duration", 5, None)
    assert np.timedelta64(30, "m") == np.timedelta64(1800, "s") and np.timedelta64(2, "W") == np.timedelta64(14, "D")
    for u in ("Y", "M"):
        with pytest.raises(ValueError, match="years and months"):
            E.fold_timedelta(("timedelta", 1, ("lit", u)))
        with pytest.raises(TypeError):
            np.datetime64("2020-01-01", "D") + np.timedelta64(1, u)
    with pytest.raises(ValueError, match="Unsupported timedelta unit: 'fortnight'"):
        E.fold_timedelta(("timedelta", 1, ("lit", "fortnight")))
    with pytest.raises(NotImplementedError, match="integer literal, not a column"):
        E.fold_timedelta(("timedelta", "i", ("lit", "s")))
    with pytest.raises(NotImplementedError, match="integer literal, not a column"):
        E.fold_timedelta(("timedelta", ("add", "i", 1)))
    with pytest.raises(TypeError, match="integer count"):
        E.fold_timedelta(("timedelta", 1.5, ("lit", "s")))
    with pytest.raises(OverflowError):
        E.fold_timedelta(("timedelta", 2**62, ("lit", "h")))
    assert E.operands(("duration", 5, "s")) == () and E.columns_of(("gt", ("sub", "a", "b"), ("timedelta", 30, ("lit", "m")))) == ["a", "b"]
    assert P._t(["fn", "timedelta", 30, ["lit", "m"]]) == ("timedelta", 30, ("lit", "m"))


# ---- now() --------------------------------------------------------------------------------------------------------------------------------
def _table():
    return pa.table({"ts": pa.array([1], pa.timestamp("s")), "ms": pa.array([1], pa.timestamp("ms")), "day": pa.array([1], pa.date32()),
                     "dur": pa.array([1], pa.duration("s")), "i": pa.array([1]), "f": pa.array([1.5]), "txt": pa.array(["x"])})


def test_now_folds_once_per_query():
    q = {"select": ["ts", ["sub", ["fn", "now"], "ts"]], "where": [">", "ts", ["sub", ["fn", "now"], ["fn", "timedelta", 1, ["lit", "D"]]]],
         "order_by": [["sub", ["fn", "now"], "ts"]]}
    before = int(time.time())
    plan = P.plan_query(q, _table())
    after = int(time.time())
    def walk(x):                                         # every tuple anywhere in the plan's steps
        if isinstance(x, (tuple, list)):
            yield x
            for y in x:
                yield from walk(y)
    consts = [n for n in walk(plan.steps) if len(n) == 3 and n[0] == "temporal"]
    assert len(consts) >= 2 and len(set(consts)) == 1 and consts[0][2] == "s" and before <= consts[0][1] <= after
    assert not any(n == ("now",) for n in walk(plan.steps))


def test_now_reads_the_clock_once_and_only_when_asked(monkeypatch):
    reads = []
    monkeypatch.setattr(E, "now_seconds", lambda: reads.append(1) or 1_600_000_000)
    assert E.fold_now([("gt", "ts", 5), None]) == [("gt", "ts", 5), None] and not reads
    a, b, c = E.fold_now([("gt", "ts", ("now",)), ("sub", ("now",), "ts"), None])
    assert a == ("gt", "ts", ("temporal", 1_600_000_000, "s")) and b == ("sub", ("temporal", 1_600_000_000, "s"), "ts") and c is None
    assert len(reads) == 1
    assert P._t(["fn", "now"]) == ("now",) and E.operands(("now",)) == ()
    assert np.datetime64("now").dtype == np.dtype("datetime64[s]")


# ---- is_busday() --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weekmask, holidays", [
    (None, ()), ("1111100", ("2020-10-09",)), ("Mon Tue Wed", ("2020-10-05", "2020-10-05", "NaT", "2020-10-10", "2020-01-01")),
    ("0000011", ("2020-10-10", "2020-10-05")), ("1000000", ()), ("Sat Sun", ("2020-10-11",))])
def test_is_busday_arguments_are_normalised_by_numpy(weekmask, holidays):
    bits, days = K.busday_calendar(weekmask, holidays)
    cal = np.busdaycalendar("1111100" if weekmask is None else weekmask, list(holidays))
    assert [(bits >> k) & 1 for k in range(7)] == [int(b) for b in cal.weekmask]
    assert days.dtype == np.int32 and days.tolist() == cal.holidays.astype(np.int64).tolist()
    assert np.all(np.diff(days) > 0)
    # the host model of the kernel's formula against np.is_busday, NaT included
    probe = np.arange(-20, 20).astype("datetime64[D]") + np.datetime64("2020-10-05", "D").astype(np.int64)
    d = probe.astype(np.int64)
    model = ((bits >> ((d + 3) % 7)) & 1).astype(bool) & ~np.isin(d, days)
    assert model.tolist() == np.is_busday(probe, busdaycal=cal).tolist()


def test_is_busday_refuses_a_list_that_does_not_fit_lds():
    days = [str(d) for d in np.arange(0, 3 * K.MAX_HOLIDAYS).astype("datetime64[D]")]
    business = [d for d in days if np.is_busday(d)]
    assert len(K.busday_calendar(None, business[:K.MAX_HOLIDAYS])[1]) == 8192
    with pytest.raises(ValueError, match="at most 8192 holidays"):
        K.busday_calendar(None, business[:K.MAX_HOLIDAYS + 1])
    with pytest.raises(ValueError, match="at most 8192 holidays"):
        P.plan_query({"select": [["fn", "is_busday", "day", ["lit", "1111100"], business[:K.MAX_HOLIDAYS + 1]]]}, _table())


def test_is_busday_lowers_to_a_mask_column(columns):
    e, extra = lower_case_functions(("is_busday", "tD"), columns)
    assert e[0] == "ne" and e[2] == 0 and extra[e[1]].arrow_type == pa.uint8()
    assert columns["__calls__"] == [("busday", "tD", None, ())]
    del columns["__calls__"][:]
    node = ("is_busday", ("date", "ts"), ("lit", "Mon Tue"), ("2020-10-05", ("lit", "2020-10-06")))
    extra = {}
    e, _ = lower_case_functions(("and", node, ("not", node)), columns, extra)
    assert e[1] == ("ne", e[1][1], 0) and e[2] == ("not", e[1])
    assert columns["__calls__"] == [("rescale", "ts", "D"), ("busday", "D(ts)", "Mon Tue", ("2020-10-05", "2020-10-06"))]
    for col, text in (("ts", r"timestamp\[s\].*write is_busday\(date\(ts\)\)"), ("txt", r"string.*write is_busday\(date\(txt\)\)")):
        with pytest.raises(TypeError, match=text):
            lower_case_functions(("is_busday", col), columns)
    with pytest.raises(TypeError):                                        # NumPy refuses the unsafe cast too
        np.is_busday(np.array([1], dtype="datetime64[s]"))
    with pytest.raises(TypeError, match="weekmask must be a string literal"):
        lower_case_functions(("is_busday", "tD", 5), columns)
    with pytest.raises(TypeError, match="list literal of date strings"):
        lower_case_functions(("is_busday", "tD", ("lit", "1111100"), ("lit", "2020-10-05")), columns)
    assert P._t(["fn", "is_busday", "d", ["lit", "1111100"], ["2020-10-05", ["lit", "2020-10-06"]]]) == \
        ("is_busday", "d", ("lit", "1111100"), ("2020-10-05", "2020-10-06"))
    assert E.columns_of(("is_busday", "d", ("lit", "1111100"), ("2020-10-05",))) == ["d"]


# ---- IN lists of temporal constants -------------------------------------------------------------------------------------------------------
def test_in_lists_are_aligned_to_the_finest_unit(columns):
    day = lambda s: int(np.datetime64(s, "D").astype(np.int64))
    e, _ = lower_case_functions(("in", "tD", (("date", ("lit", "2020-10-06")), ("date", ("lit", "2020-10-09")))), columns)
    assert e == ("in", "tD", (day("2020-10-06"), day("2020-10-09")))
    # a member finer than the column: the COLUMN is rescaled, the other members follow
    e, extra = lower_case_functions(("not_in", "tD", (("date", ("lit", "2020-10-06")), ("datetime", ("lit", "2020-10-09 12:00"), ("lit", "s")))), columns)
    sec = int(np.datetime64("2020-10-09 12:00", "s").astype(np.int64))
    assert e == ("not_in", "__temporal_datetime_s_tD", (day("2020-10-06") * 86400, sec)) and extra[e[1]].arrow_type == pa.timestamp("s")
    # a column finer than the members: the members are scaled
    e, _ = lower_case_functions(("in", "tms", (("date", ("lit", "2020-10-06")),)), columns)
    assert e == ("in", "tms", (day("2020-10-06") * 86_400_000,))
    e, _ = lower_case_functions(("in", ("date", "ts"), (("date", ("lit", "2020-10-06")),)), columns)
    assert e == ("in", "__temporal_date_D_ts", (day("2020-10-06"),))
    assert np.isin(np.array(["2020-10-06"], dtype="datetime64[D]"), np.array([day("2020-10-06") * 86400], dtype="datetime64[s]")).all()
    with pytest.raises(TypeError, match="needs date\\(\\) / datetime\\(\\) / from_timestamp\\(\\) constants, got 5"):
        lower_case_functions(("in", "tD", (("date", ("lit", "2020-10-06")), 5)), columns)
    with pytest.raises(TypeError, match="IN with temporal constants over the int64 column 'i'"):
        lower_case_functions(("in", "i", (("date", ("lit", "2020-10-06")),)), columns)
    node = ("in", "i", (1, 2, 3))
    assert lower_case_functions(node, columns)[0] is node
    assert P._t(["in", "d", [["fn", "date", ["lit", "2020-10-06"]], 5]]) == ("in", "d", (("date", ("lit", "2020-10-06")), 5))


# ---- the adapter --------------------------------------------------------------------------------------------------------------------------
def test_the_binding_mirrors_the_three_functions():
    assert B.FUNCTIONS_REGISTRY["timedelta"] == (np.timedelta64, B.FunctionType.NUMPY)
    assert B.FUNCTIONS_REGISTRY["is_busday"] == (np.is_busday, B.FunctionType.NUMPY)
    assert B.FUNCTIONS_REGISTRY["now"] == (B.NowFunction, B.FunctionType.CLASS) and issubclass(B.NowFunction, B.DatetimeFunction)
    for node in (("gt", ("sub", "dropoff", "pickup"), ("timedelta", 30, ("lit", "m"))),
                 ("is_busday", ("date", "pickup"), ("lit", "1111100"), ("2020-10-05", "2020-10-06")),
                 ("is_busday", "d"), ("timedelta", 5)):
        built = B.vectorize(node)
        got = B.lower(built)
        want = node if node[0] != "is_busday" or len(node) < 4 else node[:3] + (list(node[3]),)
        assert got == want, node
    td = B.vectorize(("timedelta", 30, ("lit", "m")))
    assert td._function is np.timedelta64 and td._is_numpy_function and not td._is_binary_func
    assert B.vectorize(("is_busday", "d"))._function is np.is_busday
    assert type(B.vectorize(("now",))) is B.NowFunction
    # the lowered holiday list is what the lowering takes
    assert lowering.busday_arguments(B.lower(B.vectorize(("is_busday", "d", ("lit", "Mon"), ("2020-10-05",))))) == ("Mon", ("2020-10-05",))


def test_the_binding_folds_now_once_per_tree(monkeypatch):
    ticks = iter(range(1_600_000_000, 1_600_000_100))
    monkeypatch.setattr(E, "now_seconds", lambda: next(ticks))
    tree = B.vectorize(("and", ("gt", "ts", ("sub", ("now",), ("timedelta", 1, ("lit", "D")))), ("lt", "ts", ("now",))))
    got = B.lower(tree)
    now = ("temporal", 1_600_000_000, "s")
    assert got == ("and", ("gt", "ts", ("sub", now, ("timedelta", 1, ("lit", "D")))), ("lt", "ts", now))
    a, b = B.lower_all([B.vectorize(("sub", ("now",), "ts")), B.vectorize(("now",))])
    assert a == ("sub", ("temporal", 1_600_000_001, "s"), "ts") and b == ("temporal", 1_600_000_001, "s")
    # a reference-shaped class of that name is the function; an impostor is not
    ref = type("NowFunction", (B.VectorizedExpression,), {"__init__": lambda self, arguments: B.VectorizedExpression.__init__(self, arguments)})
    assert B.lower(ref([]))[0] == "temporal"

    class Other(B.VectorizedExpression):
        pass
    node = Other([])
    node.__class__.__name__ = "NowFunction"
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        B.lower(node)


# ---- plan time ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select, exc, text", [
    (["add", "ts", "ms"], TypeError, r"add\(\) cannot use operands with types datetime64\[s\] and datetime64\[ms\]"),
    (["mul", "ts", 2], TypeError, "mul.*datetime64"),
    (["div", "dur", 2], TypeError, "div.*timedelta64"),
    (["mul", "dur", 1.5], TypeError, "mul.*float"),
    (["sub", "ts", "f"], TypeError, "the double column 'f'"),
    (["add", "txt", "ts"], TypeError, "the string column 'txt'"),
    (["sub", "ts", ["fn", "timedelta", 1, ["lit", "M"]]], ValueError, "years and months"),
    (["sub", "ts", ["fn", "timedelta", "i", ["lit", "s"]]], NotImplementedError, "integer literal, not a column"),
    (["fn", "is_busday", "ts"], TypeError, r"write is_busday\(date\(ts\)\)"),
    (["fn", "is_busday", "txt"], TypeError, r"write is_busday\(date\(txt\)\)"),
    (["fn", "is_busday", "day", ["lit", "Mon Funday"]], ValueError, "weekmask"),
    (["in", "day", [["fn", "date", ["lit", "2020-10-06"]], 5]], TypeError, "constants, got 5"),
    (["sub", ["fn", "datetime", "ts", ["lit", "ns"]], ["fn", "date", ["lit", "9999-01-01"]]], OverflowError, "does not fit int64"),
])
def test_plan_time_refusals(select, exc, text):
    with pytest.raises(exc, match=text):
        P.plan_query({"select": [select]}, _table())
    with pytest.raises(exc, match=text):
        P.plan_query({"select": ["i"], "where": ["is_not_null", select] if select[0] != "in" and select[1] != "is_busday" else select}, _table())


def test_plan_time_accepts_what_runs():
    for select in (["sub", "ts", "ms"], ["div", ["sub", "ts", "ms"], ["fn", "timedelta", 1, ["lit", "h"]]], ["sub", "day", ["fn", "timedelta", 7, ["lit", "D"]]],
                   ["add", "day", ["fn", "timedelta", 1, ["lit", "h"]]], ["sub", ["fn", "date", ["lit", "2021-01-01"]], "day"], ["mul", "dur", 3],
                   ["fn", "is_busday", ["fn", "date", "ts"]], ["fn", "is_busday", ["fn", "date", "txt"], ["lit", "Mon Tue"], ["2020-10-05"]],
                   ["in", ["fn", "date", "txt"], [["fn", "date", ["lit", "2020-10-06"]], ["fn", "date", ["lit", "2020-10-09"]]]],
                   ["sub", ["fn", "max", "ts"], ["fn", "min", "ms"]], ["add", "i", "f"]):
        plan = P.plan_query({"select": [select]}, _table())
        assert plan.steps[0][0] == "read"
    plan = P.plan_query({"select": ["i"], "where": [">", ["sub", "ts", "ms"], ["fn", "timedelta", 30, ["lit", "m"]]],
                         "order_by": [["sub", "ts", "ms"]]}, _table())
    assert [s[0] for s in plan.steps] == ["read", "filter", "sort", "project"]
    types = {f.name: f.type for f in _table().schema}
    assert lowering.check_temporal(("gt", ("sub", "ts", "ms"), ("timedelta", 30, ("lit", "m"))), types)[0] == "gt"
