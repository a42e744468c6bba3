"""upper() / lower() queries (as data, the vinum_amd.planner query format) for tests/golden/gen_golden_strcase.py and
tests/test_gpu_strcase.py: the shapes the reference's own planner answers -- the SELECT list over utf8 and large_utf8 columns with
NULLs, nested functions, IN / NOT IN over a function result and ORDER BY lower(c), k.
Not here, because the reference itself raises on them: sum(to_int(lower(c) IN (...))) (its planner hashes the aggregate's argument,
and the Literal holding the IN list is unhashable: "TypeError: unhashable type: 'list'"), `upper(c) = 'X'` in WHERE (ArrowTypeError: pyarrow's == on an array is not
element-wise), LIKE over a function result with NULL rows, and a string GROUP BY key (its GenericHashAggregate does not build
against the Arrow of the build container); tests/test_gpu_strcase.py checks those against pyarrow.compute."""
import numpy as np
import pyarrow as pa

_POOL = ["Berlin", "BERLIN", "berlin", "Köln", "KÖLN", "straße", "STRASSE", "İzmir", "izmir", "ȿal", "大阪", "Oslo", "oslo", "", "a", "A",
         "Zürich", "x\x00y", "ǅ", "K"]


def strcase_main_table(n: int = 1500, seed: int = 3) -> pa.Table:
    rng = np.random.default_rng(seed)
    idx, mask = rng.integers(0, len(_POOL), n), rng.random(n) < 0.05
    vals = [_POOL[i] for i in idx]
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 7, n).astype(np.int64)),
        "c": pa.array(vals, pa.string(), mask=mask),
        "lc": pa.array(vals, pa.large_string(), mask=mask),
    })


def _case(name, select, where=None, group_by=(), aliases=None, order_by=(), sort_order=None):
    return {"name": name, "table": "main", "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": False, "where": where, "group_by": list(group_by), "having": None, "order_by": list(order_by),
            "sort_order": list(sort_order or ["ASC"] * len(order_by)), "limit": None, "offset": 0}


def _fn(name, x):
    return ["fn", name, x]


CASES = [
    _case("select_list", ["k", _fn("upper", "c"), _fn("lower", "c")], aliases=[None, "u", "l"]),
    _case("select_list_large", ["k", _fn("upper", "lc"), _fn("lower", "lc")], aliases=[None, "u", "l"]),
    _case("nested", ["k", _fn("upper", _fn("lower", "c")), _fn("lower", _fn("upper", "lc"))], aliases=[None, "ul", "lu"]),
    _case("in_list", ["k"], ["in", _fn("lower", "c"), ["berlin", "köln", "straße", "nowhere"]]),
    _case("not_in_list", ["k"], ["not_in", _fn("upper", "lc"), ["BERLIN", "A"]]),
    _case("order_by_lower", ["k", "c"], order_by=[_fn("lower", "c"), "k"], sort_order=["ASC", "DESC"]),
]
