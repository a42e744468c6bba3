"""Whole-query cases for the built-in scalar functions (pure data + NumPy: no reference code).

Same form as planner_cases.py: tests/golden/gen_golden_scalar_fn.py runs each case through the reference's own
QueryPlanner + RecursiveExecutor (build container only) -> scalarfn_<name>.arrow; the GPU tests run it through
vinum_amd.planner and, for filter / projection cases, through the B2 adapter.  `approx` names the output columns that
hold a transcendental result (compared within 6 ULP: NumPy uses SVML there, up to 4 ULP; the GPU is within 2-3);
every other column is compared exactly.

The table mixes every numeric width with the values the functions treat specially: +-0, +-inf, NaN, negatives for
sqrt / log, subnormals, |x| up to 1e300 for sin / cos, finite values that overflow to_int, NULLs.
"""
import numpy as np
import pyarrow as pa

F64_SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.5, 5e-324, 2.2e-308, 1e300, -1e300, 1.5e19, -9.3e18,
               9.223372036854775808e18, 1e-300, 0.5, 3.0, 1e22, -7.0e15]
F32_SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 1e-40, 3e38, -3e38, 1e10, 0.5, 2.0]


def scalar_fn_table() -> pa.Table:
    rng = np.random.default_rng(2718)
    n = 5_000

    def ints(dt):
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        v[:4] = [0, 1, info.max, info.min]
        return v

    f64 = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 7, n)
    f64[:len(F64_SPECIAL)] = F64_SPECIAL
    f32 = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(np.float32)
    f32[:len(F32_SPECIAL)] = F32_SPECIAL
    return pa.table({
        "i8": ints(np.int8), "u8": ints(np.uint8), "i16": ints(np.int16), "i32": ints(np.int32), "i64": ints(np.int64),
        "u64": ints(np.uint64), "f32": f32, "f64": f64,
        "ni": pa.array(rng.integers(-10**6, 10**6, n), mask=rng.random(n) < 0.1),
        "nf": pa.array(rng.standard_normal(n) * 100, mask=rng.random(n) < 0.1),
        "e8": rng.integers(0, 10, n).astype(np.uint8),
        "fare": np.abs(rng.standard_normal(n)) * 40 + 0.01, "total": rng.standard_normal(n) * 30,
        "tip": rng.standard_normal(n) * 3, "lat": rng.uniform(-90, 90, n), "city_from": rng.integers(0, 9, n),
        "tax": np.round(rng.standard_normal(n) * 8, 2), "k": rng.integers(0, 60, n), "v": rng.uniform(0, 1000, n),
        "a": rng.standard_normal(n) * 50, "b": rng.standard_normal(n) * 50,
    })


def _q(name, select, aliases=None, where=None, group_by=(), having=None, order_by=(), sort_order=(), limit=None,
       approx=(), ordered=False):
    return {"name": name, "select": list(select), "aliases": list(aliases or [None] * len(select)), "distinct": False,
            "where": where, "group_by": list(group_by), "having": having, "order_by": list(order_by),
            "sort_order": list(sort_order), "limit": limit, "offset": 0, "approx": list(approx), "ordered": ordered}


def fn(name, *args):
    return ["fn", name] + list(args)


CASES = [
    # the reference's math_functions / cast groups (test_query_results.py:763-997), over columns instead of literals
    _q("exact_math", [fn("abs", "i8"), fn("abs", "i16"), fn("abs", "i64"), fn("abs", "f64"), fn("abs", "f32"),
                      fn("sqrt", "f64"), fn("sqrt", "i32"), fn("sqrt", "i16"), fn("sqrt", "f32"), fn("np.abs", "u64")],
       ["abs_i8", "abs_i16", "abs_i64", "abs_f64", "abs_f32", "sqrt_f64", "sqrt_i32", "sqrt_i16", "sqrt_f32", "abs_u64"]),
    _q("casts", [fn("to_int", "f64"), fn("to_int", "f32"), fn("to_int", "u64"), fn("to_int", "i8"), fn("to_float", "u64"),
                 fn("to_float", "i32"), fn("to_float", "f32")],
       ["int_f64", "int_f32", "int_u64", "int_i8", "float_u64", "float_i32", "float_f32"]),
    _q("to_bool_filter", ["i32", "f64"], where=["and", fn("to_bool", "f64"), fn("to_bool", "i8")]),
    _q("transcendental", [fn("sin", "f64"), fn("cos", "f64"), fn("tan", "f64"), fn("log", "f64"), fn("log2", "f64"),
                          fn("log10", "f64"), fn("np.sin", "i32"), fn("log", "i64"), fn("cos", "f32"), fn("log10", "i16")],
       ["sin", "cos", "tan", "log", "log2", "log10", "sin_i32", "log_i64", "cos_f32", "log10_i16"],
       approx=["sin", "cos", "tan", "log", "log2", "log10", "sin_i32", "log_i64", "cos_f32", "log10_i16"]),
    _q("power", [fn("power", "i16", 3), fn("power", "i64", "e8"), fn("power", "i32", 2), fn("power", "fare", 2.5),
                 fn("np.power", "f32", 2)],
       ["p_i16", "p_i64", "p_i32", "p_fare", "p_f32"], approx=["p_fare", "p_f32"]),
    _q("nullable", [fn("sqrt", "ni"), fn("abs", "nf"), fn("to_int", "nf"), fn("sqrt", "nf")], ["sq_ni", "abs_nf", "int_nf", "sq_nf"]),
    _q("constants", [["add", "i32", fn("pi")], ["mul", "fare", fn("e")], ["mul", fn("sqrt", 2), "fare"]], ["pi", "e", "sqrt2"]),
    _q("where_sqrt", ["fare", "total"], where=["gt", fn("sqrt", "fare"), 5]),
    # the issue's "Why" queries
    _q("why_project", [fn("sqrt", "fare"), fn("abs", ["sub", "total", "tip"]), fn("to_int", "total")],
       where=["gt", fn("log10", "fare"), 1]),
    _q("why_groupby", ["city_from", ["mod", fn("to_int", ["mul", fn("np.sin", "lat"), 100000]), 11], fn("count_star"),
                       fn("min", "tax")],
       [None, "grp_exp", None, None], group_by=["city_from", ["mod", fn("to_int", ["mul", fn("np.sin", "lat"), 100000]), 11]]),
    _q("order_abs_limit", ["a", "b"], order_by=[fn("abs", ["sub", "a", "b"])], sort_order=["ASC"], limit=25, ordered=True),
    _q("agg_sqrt_power", ["k", fn("sum", fn("sqrt", "v")), fn("avg", fn("power", "v", 2))], [None, "s", "p"], group_by=["k"],
       approx=["s", "p"]),
    # float16 results (8-bit integer inputs), carried through the whole query
    # (no function call appears twice in one query: the reference's planner names a call's column after id(expression))
    _q("float16", [fn("sqrt", "i8"), fn("sqrt", "u8"), fn("sin", "u8"), fn("log", "u8"), ["mul", fn("sqrt", "e8"), 3],
                   ["add", fn("log2", "e8"), 1.5]],
       ["sqrt_i8", "sqrt_u8", "sin_u8", "log_u8", "sqrt_mul", "log2_add"], approx=["sin_u8", "log_u8", "log2_add"]),
    _q("having_to_float", ["k", fn("count_star")], [None, "n"], group_by=["k"],
       having=["gt", fn("to_float", fn("count_star")), 83.0]),
]

