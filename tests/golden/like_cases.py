"""LIKE / NOT LIKE queries (as data, the vinum_amd.planner query format) for tests/golden/gen_golden_like.py and
tests/test_gpu_like.py.  Two input tables, both stored as fixtures next to the results: like_in_ref.arrow is the table of the
reference's own result tests (its three LIKE queries run on it), like_in_main.arrow is like_main_table() below: ASCII,
multi-byte UTF-8, values with '\\n' and trailing '\\x00', utf8 and large_utf8 columns, no NULLs (the reference's re.match
raises on them).  A string GROUP BY key (HAVING s LIKE ...) is no case here: the reference's GenericHashAggregate does not build
against the Arrow of the build container, so tests/test_gpu_like.py checks it against pyarrow + re."""
import numpy as np
import pyarrow as pa

REF_COLUMNS = ["id", "timestamp", "vendor_id", "city_from", "city_to", "lat", "lng", "name", "tax", "tip", "total"]

_WORDS = ["abc", "abcd", "aXc", "a.c", "ab", "b", "bab", "cab", "", "a", "zabz", "a_c", "a%c", "acc", "ba"]
_UTF = ["üa", "ü", "üxé", "aé", "éé", "ü€é", "€", "😀é", "a😀", "üü"]
_NL = ["ab", "ab\n", "ab\nc", "\nab", "ab\x00", "ab\n\x00", "x\x00\x00", "abx", "ab\x00c", "\n", "x\n", "\x00"]


def like_main_table(n: int = 3000, seed: int = 7) -> pa.Table:
    rng = np.random.default_rng(seed)
    pick = lambda vals: [vals[i] for i in rng.integers(0, len(vals), n)]   # noqa: E731
    nl = pick(_NL)
    return pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(0, 7, n).astype(np.int64)),
        "v": pa.array(rng.integers(0, 100, n).astype(np.float64)),
        "s": pa.array(pick(_WORDS), pa.string()),
        "u": pa.array(pick(_UTF), pa.string()),
        "nl": pa.array(nl, pa.string()),
        "lnl": pa.array(nl, pa.large_string()),
    })


def _case(name, select, where=None, group_by=(), having=None, aliases=None, table="main", order_by=()):
    return {"name": name, "table": table, "select": list(select), "aliases": list(aliases or [None] * len(select)),
            "distinct": False, "where": where, "group_by": list(group_by), "having": having, "order_by": list(order_by),
            "sort_order": ["ASC"] * len(order_by), "limit": None, "offset": 0}


def _like(col, p):
    return ["like", col, ["lit", p]]


def _not_like(col, p):
    return ["not_like", col, ["lit", p]]


CASES = [
    # vinum/tests/test_query_results.py:209-232, 263-268
    _case("ref_like", REF_COLUMNS, _like("name", "Jos%"), table="ref"),
    _case("ref_not_like", REF_COLUMNS, _not_like("name", "Jos%"), table="ref"),
    _case("ref_or", ["id"], ["or", ["or", ["eq", "id", 4], ["gt", ["div", "total", 10], 10.1]], _like("city_from", "%iv%")], table="ref"),
    _case("underscore", ["k", "s"], _like("s", "a_c")),
    _case("both_ends", ["k", "s"], _like("s", "%ab%")),
    _case("empty_pattern", ["k", "s"], _like("s", "")),
    _case("dot", ["k", "s"], _like("s", "a.c%")),
    _case("not_like_or", ["k"], ["or", _not_like("s", "%b%"), ["gt", "v", 80]]),
    _case("group_count", ["g", ["fn", "count"]], _like("s", "%a%"), group_by=["g"], aliases=[None, "n"]),
    _case("select_list", ["k", _like("s", "a%")], aliases=[None, "m"]),
    _case("sum_to_int", ["g", ["fn", "sum", ["fn", "to_int", _like("s", "%b%")]]], group_by=["g"], aliases=[None, "n"]),
    _case("multibyte", ["k", "u"], ["and", _like("u", "ü_%"), _not_like("u", "%€%")]),
    _case("newline_nul", ["k"], ["or", _like("nl", "ab"), _like("nl", "%\n_")]),
    _case("large_newline_nul", ["k"], ["or", _like("lnl", "ab"), _like("lnl", "%\n_")]),
    _case("nul_prefix", ["k", _like("nl", "ab%"), _like("lnl", "ab%")], aliases=[None, "a", "b"]),
]
