"""date() / datetime() / from_timestamp() queries (as data, the vinum_amd.planner query format) for tests/golden/gen_golden_datetime.py
and tests/test_gpu_datetime.py, their input tables, and the restatement of DatetimeFunction over a column of strings
(parsed_on_host(): np.array(strings, dtype='datetime64[unit]'), NaT -> NULL).

The golden cases are the column queries of the reference's own tests (vinum/tests/test_query_results.py:1114-1154 and 1222-1266) and
the two counts tests/golden/planner_cases.py left out of the query of :1270-1301, over
  * "main": 1000 rows WITHOUT NULLs and without fractions, every string a full date and time, so that the unit NumPy picks for the
    reference is s in every batch (with a coarser or finer value in a batch its result type changes with how the batches were split);
  * "null": the reference's own NULL test table (planner_cases.null_table()).
gen_golden_datetime.py runs every case through the reference's own planner and executor and writes the result as a fixture;
datetime_cases.json records the shape of every result and, under "raised", the cases the reference itself raises on in the build
container (none of these: two aggregates over the SAME datetime(x) node trip its planner, so no case holds two)."""
import numpy as np
import pyarrow as pa

from tests.golden.planner_cases import null_table


def _texts(secs, sep=" "):
    return [str(s).replace("T", sep) for s in np.array(secs, dtype="datetime64[s]").astype("str")]


def datetime_main_table(n: int = 1000, seed: int = 15) -> pa.Table:
    rng = np.random.default_rng(seed)
    secs = (1602127614 + rng.integers(0, 12, n) * 86400 + rng.integers(0, 40, n) * 977).astype(np.int64)
    d = pa.array(_texts(secs), pa.string())
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 5, n).astype(np.int64)),
        "d": d,
        "dt": pa.array(_texts(secs, "T"), pa.string()),
        "dd": d.cast(pa.dictionary(pa.int16(), pa.string())),
        "timestamp": pa.array(secs),
        "t32": pa.array((secs - 1602000000).astype(np.int32)),
    })


def datetime_null_table(n: int = 2500, seed: int = 16) -> pa.Table:
    """the table of the restated queries: strings in every depth of the grammar, '' / NaT / nat and NULL rows, a dictionary-typed
    column, integers and timestamps with NULLs and with values before 1970"""
    rng = np.random.default_rng(seed)
    secs = (1602127614 + rng.integers(-5, 12, n) * 86400 + rng.integers(0, 30, n) * 1931).astype(np.int64)
    full = _texts(secs)
    d = []
    for i, s in enumerate(full):
        r = rng.random()
        d.append(None if r < 0.05 else "" if r < 0.08 else "NaT" if r < 0.10 else s[:10] if r < 0.2 else s.replace(" ", "T") if r < 0.4
                 else s + f".{int(rng.integers(0, 1000)):03d}" if r < 0.5 else s[:16] if r < 0.55 else s)
    dd = pa.array([None if rng.random() < 0.1 else s[:10] for s in full], pa.string()).cast(pa.dictionary(pa.int8(), pa.string()))
    ms = secs * 1000 + rng.integers(0, 1000, n) - np.where(rng.random(n) < 0.3, 1_700_000_000_000, 0)
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "d": pa.array(d, pa.string()),
        "dd": dd,
        "ym": pa.array([s[:7] for s in full], pa.large_string()),
        "i32": pa.array(rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), mask=rng.random(n) < 0.1),
        "i64": pa.array(rng.integers(-2**62, 2**62, n).astype(np.int64), mask=rng.random(n) < 0.1),
        "ts": pa.array(ms, pa.timestamp("ms"), mask=rng.random(n) < 0.1),
        "day": pa.array((secs // 86400).astype(np.int32), pa.date32(), mask=rng.random(n) < 0.1),
    })


def parsed_on_host(strings, unit: str) -> pa.Array:
    """DatetimeFunction over a column of strings (vinum/core/functions.py:112-119): np.array(strings, dtype='datetime64[unit]') as
    the Arrow array the reference makes of it -- date32 for D, timestamp[unit] otherwise, NaT (None, '', NaT in any case) NULL"""
    values = np.array([None if s is None else s.rstrip("\x00") for s in strings], dtype=f"datetime64[{unit}]")
    null = np.isnat(values)
    raw = np.where(null, 0, values.astype(np.int64))
    return pa.array(raw.astype(np.int32), pa.date32(), mask=null) if unit == "D" else pa.array(raw, pa.timestamp(unit), mask=null)


def _case(name, select, where=None, group_by=(), aliases=None, order_by=(), sort_order=None, distinct=False, table="main"):
    return {"name": name, "table": table, "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": distinct, "where": where, "group_by": list(group_by), "having": None, "order_by": list(order_by),
            "sort_order": list(sort_order or ["ASC"] * len(order_by)), "limit": None, "offset": 0}


def _fn(name, *x):
    return ["fn", name] + list(x)


def _lit(s):
    return ["lit", s]


CASES = [
    # test_query_results.py:1114-1154
    _case("select_datetime_D", [_fn("datetime", "d", _lit("D"))]),
    _case("select_datetime", [_fn("datetime", "d")]),
    _case("select_datetime_T", ["k", _fn("datetime", "dt"), _fn("date", "dt")], aliases=[None, "s", "day"]),
    _case("select_from_timestamp", [_fn("from_timestamp", "timestamp")]),
    _case("select_from_timestamp_int32_ms", ["k", _fn("from_timestamp", "t32", _lit("ms"))], aliases=[None, "ms"]),
    _case("select_date_of_dictionary_typed", ["k", _fn("date", "dd")], aliases=[None, "day"]),
    _case("where_date_ge_constant", ["k"], where=["ge", _fn("date", "d"), _fn("date", _lit("2020-10-12"))]),
    _case("where_datetime_lt_constant", ["k"], where=["lt", _fn("datetime", "d"), _fn("datetime", _lit("2020-10-12 04:00:00"), _lit("s"))]),
    _case("group_by_int_count_datetime", ["g", _fn("count", _fn("datetime", "d")), _fn("max", _fn("date", "d"))],
          aliases=[None, "n", "hi"], group_by=["g"], order_by=["g"]),
    _case("order_by_datetime", ["k"], order_by=[_fn("datetime", "d"), "k"], sort_order=["DESC", "ASC"]),
    # test_query_results.py:1222-1266
    _case("null_datetime_is_null", ["id"], where=["is_null", _fn("datetime", "date")], order_by=["id"], table="null"),
    _case("null_datetime_is_not_null", ["id"], where=["is_not_null", _fn("datetime", "date")], order_by=["id"], table="null"),
    _case("null_from_timestamp_is_null", ["id"], where=["is_null", _fn("from_timestamp", "timestamp")], order_by=["id"], table="null"),
    _case("null_from_timestamp_is_not_null", ["id"], where=["is_not_null", _fn("from_timestamp", "timestamp")], order_by=["id"], table="null"),
    _case("null_order_by_datetime", ["id"], order_by=[_fn("datetime", "date")], table="null"),
    _case("null_order_by_from_timestamp", ["id"], order_by=[_fn("from_timestamp", "timestamp")], table="null"),
    # the two counts of test_query_results.py:1270-1301 planner_cases.NULL_TABLE_EXPECTED leaves out, grouped by the integer code of the city
    _case("null_counts", ["city_id", _fn("count", _fn("datetime", "date")), _fn("count", _fn("from_timestamp", "timestamp"))],
          aliases=[None, "cnt_datetime", "cnt_timestamp"], group_by=["city_id"], order_by=["city_id"], table="null"),
]

TABLES = {"main": datetime_main_table, "null": null_table}
