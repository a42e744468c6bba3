"""Temporal arithmetic, timedelta(), is_busday() and now() queries (as data, the vinum_amd.planner query format) for
tests/golden/gen_golden_temporal_arith.py and tests/test_gpu_temporal_arith.py, and their input table.

"main": 1000 taxi-like rows WITHOUT NULLs -- pickup timestamp[s], dropoff timestamp[ms] up to three hours later, d the pickup's
date32 -- all in October 2020, so that `now() - timedelta(1, 'D')` lies after every row whenever the query is planned: the one now()
case is comparable although the reference reads the clock once per batch and this project once per query.
gen_golden_temporal_arith.py runs every case through the reference's own planner and executor and writes the result as a fixture;
temporal_arith_cases.json records the shape of every result and, under "raised", the cases the reference itself raises on in the
build container (a difference of dates has no Arrow type there, a date plus hours is datetime64[h])."""
import numpy as np
import pyarrow as pa


def temporal_arith_main_table(n: int = 1000, seed: int = 17) -> pa.Table:
    rng = np.random.default_rng(seed)
    pickup = (1601510400 + rng.integers(0, 31 * 86400, n)).astype(np.int64)               # 2020-10-01 ... 2020-10-31
    dropoff = pickup * 1000 + rng.integers(0, 3 * 3600 * 1000, n)
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 5, n).astype(np.int64)),
        "pickup": pa.array(pickup, pa.timestamp("s")),
        "dropoff": pa.array(dropoff, pa.timestamp("ms")),
        "d": pa.array((pickup // 86400).astype(np.int32), pa.date32()),
    })


def _case(name, select, where=None, group_by=(), aliases=None, order_by=(), sort_order=None, distinct=False, table="main"):
    return {"name": name, "table": table, "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": distinct, "where": where, "group_by": list(group_by), "having": None, "order_by": list(order_by),
            "sort_order": list(sort_order or ["ASC"] * len(order_by)), "limit": None, "offset": 0}


def _fn(name, *x):
    return ["fn", name] + list(x)


def _lit(s):
    return ["lit", s]


def _td(n, unit):
    return _fn("timedelta", n, _lit(unit))


TRIP = ["sub", "dropoff", "pickup"]
HOLIDAYS = ["2020-10-12", "2020-10-13", "2020-10-31", "2020-10-12"]

CASES = [
    _case("select_trip", ["k", TRIP], aliases=[None, "trip"]),
    _case("where_trip_gt_30m", ["k"], where=["gt", TRIP, _td(30, "m")]),
    _case("select_trip_in_hours", ["k", ["div", TRIP, _td(1, "h")]], aliases=[None, "hours"]),
    _case("select_date_minus_week", ["k", ["sub", "d", _td(7, "D")]], aliases=[None, "before"]),
    _case("select_date_plus_hour", ["k", ["add", "d", _td(1, "h")]], aliases=[None, "later"]),
    _case("select_constant_minus_date", ["k", ["sub", _fn("date", _lit("2021-01-01")), "d"]], aliases=[None, "left"]),
    _case("select_pickup_plus_90s", ["k", ["add", "pickup", _td(90, "s")]], aliases=[None, "later"]),
    _case("select_pickup_plus_ms", ["k", ["add", _td(250, "ms"), "pickup"]], aliases=[None, "later"]),
    _case("select_twice_the_trip", ["k", ["mul", TRIP, 2]], aliases=[None, "twice"]),
    _case("where_date_ge_constant_minus_week", ["k"], where=["ge", "d", ["sub", _fn("date", _lit("2020-10-16")), _td(7, "D")]]),
    _case("where_dropoff_before_pickup_plus_hour", ["k"], where=["lt", "dropoff", ["add", "pickup", _td(1, "h")]]),
    _case("order_by_trip", ["k"], order_by=[TRIP, "k"], sort_order=["DESC", "ASC"]),
    _case("min_trip_by_group", ["g", _fn("min", TRIP)], aliases=[None, "lo"], group_by=["g"], order_by=["g"]),
    _case("max_trip_by_group", ["g", _fn("max", TRIP)], aliases=[None, "hi"], group_by=["g"], order_by=["g"]),
    _case("where_is_busday", ["k"], where=_fn("is_busday", "d")),
    _case("where_is_busday_of_date_of_pickup", ["k"], where=_fn("is_busday", _fn("date", "pickup"), _lit("1111110"), HOLIDAYS)),
    _case("group_by_is_busday", [_fn("is_busday", _fn("date", "pickup")), _fn("count_star")], aliases=["busday", "n"],
          group_by=[_fn("is_busday", _fn("date", "pickup"))], order_by=[_fn("is_busday", _fn("date", "pickup"))]),
    _case("where_before_now_minus_day", ["k"], where=["lt", "pickup", ["sub", _fn("now"), _td(1, "D")]]),
    _case("where_date_in_list", ["k"], where=["in", "d", [_fn("date", _lit("2020-10-06")), _fn("date", _lit("2020-10-09"))]]),
]

TABLES = {"main": temporal_arith_main_table}
