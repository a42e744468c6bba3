"""Comparisons of two string columns (as data, the vinum_amd.planner query format) for tests/golden/gen_golden_strcmp.py and
tests/test_gpu_strcmp_golden.py.  One small input table, stored as a fixture next to the results: 40 rows, two city columns
drawn from overlapping value sets in different orders (so their dictionaries hand out different codes), a third one for BETWEEN
bounds; no NULLs in the compared columns (NumPy compares None with nothing) and no trailing NULs (a NumPy 'U' array drops them,
the GPU path compares bytes exactly)."""
import numpy as np
import pyarrow as pa

_CITIES = ["Berlin", "Bern", "Ber", "", "Zürich", "Zug", "München", "a", "ab", "Aachen", "Köln", "Kiel"]


def strcmp_table(n: int = 40, seed: int = 23) -> pa.Table:
    rng = np.random.default_rng(seed)
    frm = [_CITIES[i] for i in rng.integers(0, 9, n)]
    to = [_CITIES[::-1][i] for i in rng.integers(0, 9, n)]
    to = [f if s else t for f, t, s in zip(frm, to, rng.random(n) < 0.3)]
    via = [_CITIES[i] for i in rng.integers(2, 12, n)]
    return pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "g": pa.array(rng.integers(0, 4, n).astype(np.int64)),
                     "city_from": pa.array(frm, pa.string()), "city_to": pa.array(to, pa.string()), "city_via": pa.array(via, pa.string())})


def _case(name, select, where=None, group_by=(), having=None, aliases=None):
    return {"name": name, "table": "main", "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": False, "where": where, "group_by": list(group_by), "having": having, "order_by": [],
            "sort_order": [], "limit": None, "offset": 0}


_SAME = ["fn", "sum", ["fn", "to_int", ["eq", "city_from", "city_to"]]]

CASES = [
    _case("eq", ["k", "city_from"], ["eq", "city_from", "city_to"]),
    _case("ne", ["k", "city_to"], ["ne", "city_from", "city_to"]),
    _case("lt", ["k"], ["lt", "city_from", "city_to"]),
    _case("ge", ["k"], ["ge", "city_from", "city_to"]),
    _case("between", ["k"], ["between", "city_via", "city_from", "city_to"]),
    _case("select_list", ["k", ["eq", "city_from", "city_to"], ["gt", "city_from", "city_via"]], aliases=[None, "same", "after"]),
    _case("group_having", ["g", _SAME], group_by=["g"], having=["gt", _SAME, 2], aliases=[None, "n"]),
]
