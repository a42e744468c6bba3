"""concat() / || queries (as data, the vinum_amd.planner query format) for tests/golden/gen_golden_concat.py and
tests/test_gpu_concat.py, their input table, and a Python restatement of ConcatFunction over rows (restate()).

CASES are the shapes the reference's own planner and executor answer: gen_golden_concat.py writes their results as fixtures.
RESTATED are the shapes the reference itself cannot run in the build container; tests/test_gpu_concat.py checks them against
restate() over the rows instead (gen_golden_concat.py tries them and records the error in concat_cases.json):
  * concat as a GROUP BY key: "GenericHashAggregate is not buildable against Arrow 25" (oracle/ref_build/Makefile);
  * DISTINCT over a function: AssertionError in Expression.get_shared_id (vinum/parser/query.py:314);
  * two concat() calls of one SELECT list that begin with the same column: 'ValueError: Column "concat_<id>" is not found.'
    (the planner shares the sub-expression and loses it);
  * ORDER BY a concat() whose values hold NULs: the reference sorts the materialised column, see below.

What a fixture holds for a SELECT-list column: ConcatFunction returns a NumPy 'U' array whose elements keep leading and embedded
NULs ('\0z' + 'c' is '\0zc'), and the reference's ProjectOperator then builds the output batch with pa.array(ndarray), which
cuts every element at its FIRST NUL code point ('' here).  This project returns the function's value.  So a fixture column equals
this project's column with each value cut at its first NUL, and the tests hold both: result == restate(), fixture == cut(result).
In WHERE the reference compares the NumPy array itself: the whole value counts there, as it does here."""
import numpy as np
import pyarrow as pa

_A = ["Ada", "Grace", "", "y\x00", "\x00z", "q\x00\x00", "x\x00y", "\x00", "Köln", "大阪", "ab", "a", "İ", "ß"]
_B = ["Lovelace", "Hopper", "", "c", "bc", "\x00", "tail\x00", "\x00lead", "straße", "🙂", "Z"]
_D = ["north", "south", "", "e\x00", "ö"]


def concat_main_table(n: int = 2000, seed: int = 13) -> pa.Table:
    rng = np.random.default_rng(seed)

    def col(pool, t, null_rate=0.06):
        idx, mask = rng.integers(0, len(pool), n), rng.random(n) < null_rate
        return pa.array([pool[i] for i in idx], pa.string(), mask=mask).cast(t)
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 5, n).astype(np.int64)),
        "v": pa.array(rng.integers(0, 100, n).astype(np.int64)),
        "a": col(_A, pa.string()),
        "b": col(_B, pa.large_string()),
        "d": col(_D, pa.dictionary(pa.int8(), pa.string())),
        "p": col(["ab", "a", "abc", ""], pa.string(), 0.02),          # 'ab' + 'c' and 'a' + 'bc' collide
        "q": col(["c", "bc", "", "abc"], pa.string(), 0.02),
    })


def _case(name, select, where=None, group_by=(), aliases=None, order_by=(), sort_order=None, distinct=False):
    return {"name": name, "table": "main", "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": distinct, "where": where, "group_by": list(group_by), "having": None, "order_by": list(order_by),
            "sort_order": list(sort_order or ["ASC"] * len(order_by)), "limit": None, "offset": 0}


def _fn(name, *x):
    return ["fn", name] + list(x)


def _lit(s):
    return ["lit", s]


def _cc(*x):
    """concat as the planner's query format spells it: the operator node (the "fn" spelling of that name stays an unknown function)"""
    return ["concat"] + list(x)


CASES = [
    _case("two_columns", ["k", _cc("a", "b"), _cc("p", "q")], aliases=[None, "ab", "pq"]),
    _case("column_literal_column", ["k", _cc("a", _lit(" "), "b")], aliases=[None, "c"]),
    _case("leading_literal", ["k", _cc(_lit("#"), "a"), _cc(_lit("<"), "a", _lit("-"), "b", _lit(">"))], aliases=[None, "c", "w"]),
    _case("trailing_numbers", ["k", _cc("a", 7), _cc("b", 2.5)], aliases=[None, "i", "f"]),
    _case("numbers_between", ["k", _cc("a", _lit("_"), 3, _lit("_"), "b", 1)], aliases=[None, "m"]),
    _case("one_operand", ["k", _cc("a"), _cc("b")], aliases=[None, "a1", "b1"]),
    _case("three_columns", ["k", _cc("a", "b", "p"), _cc("a", _lit("/"), "b", _lit("/"), "p", _lit("/"), "q")], aliases=[None, "abp", "abpq"]),
    _case("concat_of_upper", ["k", _cc(_fn("upper", "a"), "b")], aliases=[None, "c"]),
    _case("where_literal", ["k"], ["eq", _cc("a", _lit(" "), "b"), _lit("Ada Lovelace")]),
    _case("where_collision", ["k"], ["eq", _cc("p", "q"), _lit("abc")]),
    _case("order_by", ["k", "p"], order_by=[_cc("p", _lit("-"), "q"), "k"], sort_order=["ASC", "DESC"]),       # (p, q hold no NULs)
    _case("upper_of_concat", ["k", _fn("upper", _cc("a", "b"))], aliases=[None, "c"]),
    _case("dictionary_operand", ["k", _cc("d", _lit(":"), "a"), _cc("b", "d")], aliases=[None, "da", "bd"]),
    _case("dictionary_one_operand", ["k", _cc("d")], aliases=[None, "d1"]),
]

RESTATED = [
    _case("shared_first_column", ["k", _cc("a", 7), _cc("a", _lit("_"), 3), _cc("d", _lit(":"), "a"), _cc("d")],
          aliases=[None, "a7", "a3", "da", "d1"]),
    _case("group_by", [_cc("p", _lit("-"), "q"), _fn("count_star"), _fn("sum", "v"), _fn("count", _cc("p", "q"))],
          aliases=["c", "n", "s", "m"], group_by=[_cc("p", _lit("-"), "q")]),
    _case("distinct", [_cc("p", _lit("+"), "q")], aliases=["c"], distinct=True),
    _case("order_by_with_nuls", ["k", "a"], order_by=[_cc("a", "b"), "k"], sort_order=["DESC", "ASC"]),
]

# `a || b` (SQLExpression.CONCAT) for the adapter: binding.vectorize builds the registry's class for the "||" node
ADAPTER_PIPE = [("pipe", ["k", ["||", "a", "b"], ["||", ["||", "p", _lit("|")], "q"]], ["k", "ab", "pq"])]


def _text(x):
    """what np.array(x, dtype='U') holds for one row's value: str(None) for NULL, trailing NUL code points dropped"""
    return ("None" if x is None else str(x)).rstrip("\x00")


def cut_at_nul(values):
    """what pa.array(ndarray of dtype 'U') keeps of each element: everything before its first NUL code point"""
    return [v.split("\x00")[0] for v in values]


def restate(table: pa.Table, e):
    """ConcatFunction / UpperStringFunction / LowerStringFunction over the rows of `table`, as a list of Python strings: `e` is a
    column name, ["lit", s], a number, ["concat", operand...] (also ["||", x, y]) or ["fn", name, operand] with name upper / lower"""
    import pyarrow.compute as pc
    n = table.num_rows
    if isinstance(e, str):
        c = table[e].combine_chunks()
        c = c.dictionary_decode() if pa.types.is_dictionary(c.type) else c
        return c.cast(pa.string()).to_pylist()
    if isinstance(e, (int, float)):
        return [str(e)] * n
    if e[0] == "lit":
        return [e[1]] * n
    name, args = (e[1].lower(), e[2:]) if e[0] == "fn" else ("concat", e[1:])
    rows = [restate(table, x) for x in args]
    if name == "concat":
        return ["".join(_text(r[i]) for r in rows) for i in range(n)]
    kernel = {"upper": pc.utf8_upper, "lower": pc.utf8_lower}[name]
    return kernel(pa.array(rows[0], pa.string())).to_pylist()
