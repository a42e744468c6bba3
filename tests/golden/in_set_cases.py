"""IN / NOT IN queries with lists of 40-300 members (as data, the vinum_amd.planner query format) for
tests/golden/gen_golden_in_set.py and tests/test_gpu_in_set.py.  The input table is in_set_table() below, stored as the fixture
in_set_in.arrow next to the reference's results (in_set_<case>.arrow): 400 rows of int64, int32 with NULLs, uint8, float64 with
NaN / +-0.0 / +-inf rows, float32 and utf8.  Every list is longer than the 16 members the projection interpreter's OR chain
holds, so every case runs through a set probe."""
import numpy as np
import pyarrow as pa

_CITIES = ["Berlin", "Bern", "Bonn", "Munich", "Riva", "San Francisco", "Naples", "Bérgamo", "B", "", "Oslo", "Lima"]


def in_set_table(n: int = 400, seed: int = 11) -> pa.Table:
    rng = np.random.default_rng(seed)
    f64 = rng.integers(-40, 40, n).astype(np.float64) / 4.0
    f64[rng.integers(0, n, 25)] = np.nan
    f64[rng.integers(0, n, 10)] = -0.0
    f64[rng.integers(0, n, 5)] = np.inf
    f64[rng.integers(0, n, 5)] = -np.inf
    i32 = rng.integers(-300, 300, n).astype(np.int32)
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 7, n).astype(np.int64)),
        "a": pa.array(rng.integers(-600, 600, n).astype(np.int64)),
        "i32n": pa.array(i32, mask=rng.random(n) < 0.2),
        "u8": pa.array(rng.integers(0, 256, n).astype(np.uint8)),
        "f64": pa.array(f64),
        "f32": pa.array((rng.integers(-50, 50, n).astype(np.float32) / np.float32(10.0))),
        "v": pa.array(rng.integers(0, 100, n).astype(np.float64)),
        "s": pa.array([_CITIES[i] for i in rng.integers(0, len(_CITIES), n)], pa.string()),
    })


def _case(name, select, where=None, group_by=(), aliases=None):
    return {"name": name, "table": "main", "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": False, "where": where, "group_by": list(group_by), "having": None, "order_by": [],
            "sort_order": [], "limit": None, "offset": 0}


_rng = np.random.default_rng(5)
INTS_SCATTERED = sorted({int(x) for x in _rng.integers(-700, 700, 150)})                    # a sorted table
INTS_DENSE = list(range(-100, 200))                                                         # 300 members: a bitmap
INTS_I32 = [int(x) for x in _rng.integers(-320, 320, 80)]                                   # duplicates stay in
INTS_U8 = [-1, 300, 256, 255, 0] + [int(x) for x in _rng.integers(0, 256, 45)]              # members outside uint8
FLOATS = [x / 4.0 for x in range(-30, 30, 2)] + [0.0, float("inf"), 1e300, 0.1] + [x + 0.125 for x in range(20)]
FLOATS_F32 = [x / 10.0 for x in range(-50, 0)] + [0.5, 1.5, 2.5, -0.0]                      # float32(0.1 * k) is seldom the float64
INTS_AND_ONE_FLOAT = list(range(-600, 600, 25)) + [2.5]
STRINGS = ["Berlin", "Bonn", "Riva", "", "Bérgamo"] + [f"city{i}" for i in range(40)]       # partly absent from the data
STRINGS_ABSENT = [f"nowhere{i}" for i in range(40)]

CASES = [
    _case("in_i64", ["k", "a"], ["in", "a", INTS_SCATTERED]),
    _case("not_in_i64", ["k", "a"], ["not_in", "a", INTS_SCATTERED]),
    _case("in_i64_dense", ["k"], ["in", "a", INTS_DENSE]),
    _case("in_i32_nulls", ["k"], ["in", "i32n", INTS_I32]),
    _case("not_in_i32_nulls", ["k"], ["not_in", "i32n", INTS_I32]),
    _case("in_u8", ["k", "u8"], ["in", "u8", INTS_U8]),
    _case("in_f64", ["k"], ["in", "f64", FLOATS]),
    _case("not_in_f64", ["k"], ["not_in", "f64", FLOATS]),
    _case("in_f32", ["k"], ["in", "f32", FLOATS_F32]),
    _case("int_col_one_float", ["k"], ["in", "a", INTS_AND_ONE_FLOAT]),
    _case("in_utf8", ["k", "s"], ["in", "s", STRINGS]),
    _case("not_in_utf8", ["k"], ["not_in", "s", STRINGS]),
    _case("in_utf8_all_absent", ["k"], ["not_in", "s", STRINGS_ABSENT]),
    _case("and_or", ["k"], ["or", ["and", ["in", "a", INTS_SCATTERED], ["gt", "v", 10]], ["in", "u8", INTS_U8]]),
    _case("select_list", ["k", ["in", "a", INTS_DENSE], ["not_in", "f64", FLOATS]], aliases=[None, "m", "nm"]),
    # (with GROUP BY g the reference's binder hashes the select expressions and a Literal holding a list is unhashable: the one-group
    # aggregate is the shape it can run)
    _case("sum_to_int", [["fn", "sum", ["fn", "to_int", ["in", "a", INTS_SCATTERED]]], ["fn", "count"]], aliases=["n", "rows"]),
]
