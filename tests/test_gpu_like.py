"""LIKE / NOT LIKE on the GPU: the dictionary matcher (vnm_strdict_like) against a Python-`re` restatement of the reference,
whole queries through vinum_amd.planner and the B2 adapter against pyarrow + re and against the reference's own results
(tests/golden/like_*.arrow), a growing dictionary, the GPU CSV reader, the errors, and one full-size filter."""
import json
import os
import random
import re

import numpy as np
import pyarrow as pa
import pytest

from tests import util
from tests.golden import like_cases as C

pytestmark = pytest.mark.gpu


def ref_like(pattern, value, strip_nul):
    """LikeFunction._like (vinum/core/functions.py:322-338) on one value; a utf8 column reaches it as NumPy 'U' (trailing NULs gone)"""
    if strip_nul:
        value = value.rstrip("\x00")
    return bool(re.compile("^" + pattern.replace("_", ".").replace("%", ".*") + "$").match(value))


def like_mask(col: pa.ChunkedArray, pattern, invert=False):
    """row mask with the project's NULL rule: LIKE false, NOT LIKE true"""
    strip = pa.types.is_string(col.type)
    out = []
    for v in col.to_pylist():
        out.append(invert if v is None else ref_like(pattern, v, strip) != invert)
    return np.array(out, dtype=bool)


def _table_of(kd, pattern, top):
    return kd.like_table(pattern)._values.to_host(np.uint8, top)


# ---- 1. the matcher against re ---------------------------------------------------------------------------------------------
_ALPHA = ["a", "b", "c", "\n", "\x00", "ü", "é", "€", "😀", ".", "_", "%"]
_PALPHA = ["a", "b", "\n", "%", "%", "_", ".", "ü", "€", "😀", "ab"]


def _values(rng, n):
    vals = set()
    while len(vals) < n:
        k = rng.choice([0, 1, 2, 3, 5, 8, 13])
        v = "".join(rng.choice(_ALPHA) for _ in range(k))
        if rng.random() < 0.03:
            v = "".join(rng.choice(_ALPHA[:3]) for _ in range(rng.randint(1000, 1500))) + v   # over 1 KiB
        vals.add(v)
    return sorted(vals)


def _patterns(rng, n):
    pats = ["", "%", "_", "a%", "%a", "%a%", "a_c", "a.c", "%\n", "\n%", "%\n_", "ab", "%ü%", "_%_", "%%a%%b%%"]
    while len(pats) < n:
        pats.append("".join(rng.choice(_PALPHA) for _ in range(rng.randint(1, 7))))
    pats.append("a" * 600 + "%" + "b" * 500)                                # a pattern over 1 KiB
    return pats


@pytest.mark.parametrize("arrow_type", [pa.string(), pa.large_string()], ids=["utf8", "large_utf8"])
def test_matcher_against_re(arrow_type):
    from vinum_amd.vinum_lib import KeyDictionary
    from vinum_amd import _lib as L
    rng = random.Random(11)
    values = _values(rng, 3000)
    kd = KeyDictionary(arrow_type)
    codes = kd.encode(pa.array(values, arrow_type)).to_numpy(zero_copy_only=False)
    top = int(L.lib().vnm_strdict_ids(kd.handle()))
    strip = pa.types.is_string(arrow_type)
    for p in _patterns(rng, 60):
        tab = _table_of(kd, p, top)
        got = tab[codes].astype(bool)
        # (Python's re backtracks: `.*a.*b.*` over a 1.5 KB value is cubic -- values over 64 bytes meet the patterns with at
        #  most two `%` runs, every value meets the rest)
        check = np.array([len(v) <= 64 or len(re.findall("%+", p)) <= 2 for v in values])
        exp = np.array([ref_like(p, v, strip) if c else False for v, c in zip(values, check)])
        bad = np.flatnonzero((got != exp) & check)
        assert not len(bad), (p, [(values[i], bool(got[i])) for i in bad[:5]])


# ---- 2. WHERE through the planner, NULLs --------------------------------------------------------------------------------------
def _nullable_table(n=20000, seed=5):
    rng = np.random.default_rng(seed)
    words = ["Joseph", "Jonas", "Joe", "Jos", "jos", "José", "ab\n", "ab", "", "xJos", "Jo\nse"]
    s = [words[i] for i in rng.integers(0, len(words), n)]
    null = rng.random(n) < 0.05
    return pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(rng.integers(0, 100, n).astype(np.float64)),
                     "s": pa.array(s, pa.string(), mask=null), "ls": pa.array(s, pa.large_string(), mask=null)})


WHERE_CASES = [
    (["like", "s", ["lit", "Jos%"]], lambda t: like_mask(t["s"], "Jos%")),
    (["not_like", "s", ["lit", "Jos%"]], lambda t: like_mask(t["s"], "Jos%", True)),
    (["like", "ls", ["lit", "%o_e%"]], lambda t: like_mask(t["ls"], "%o_e%")),
    (["like", "s", ["lit", "nothing%here"]], lambda t: like_mask(t["s"], "nothing%here")),
    (["or", ["not_like", "s", ["lit", "J%"]], ["gt", "v", 90]],
     lambda t: like_mask(t["s"], "J%", True) | (t["v"].to_numpy() > 90)),
    (["and", ["like", "s", ["lit", "Jo%"]], ["not", ["like", "ls", ["lit", "%e"]]], ["ne", "s", ["lit", "Joe"]]],
     lambda t: like_mask(t["s"], "Jo%") & like_mask(t["ls"], "%e", True)
     & np.array([v is None or v != "Joe" for v in t["s"].to_pylist()])),
]


@pytest.mark.parametrize("where,oracle", WHERE_CASES, ids=[str(i) for i in range(len(WHERE_CASES))])
def test_where_through_the_planner(where, oracle):
    from vinum_amd import planner, set_batch_size
    t = _nullable_table()
    set_batch_size(3000)
    try:
        got = planner.execute({"select": ["k", "s"], "where": where}, t)
    finally:
        set_batch_size(1 << 24)
    exp = t.filter(pa.array(oracle(t))).select(["k", "s"])
    assert got.num_rows == exp.num_rows
    assert got.column("k").to_pylist() == exp.column("k").to_pylist()
    assert got.column("s").to_pylist() == exp.column("s").to_pylist()


def test_having_on_a_string_key_and_select_list():
    from vinum_amd import planner
    t = _nullable_table()
    got = planner.execute({"select": ["s", ["fn", "count"]], "group_by": ["s"], "having": ["like", "s", ["lit", "Jo%"]],
                           "aliases": [None, "n"]}, t)
    counts = {}
    for v in t["s"].to_pylist():
        counts[v] = counts.get(v, 0) + 1
    exp = {v: c for v, c in counts.items() if v is not None and ref_like("Jo%", v, True)}
    assert dict(zip(got["s"].to_pylist(), got["n"].to_pylist())) == exp
    got = planner.execute({"select": ["k", ["not_like", "s", ["lit", "%e"]]], "aliases": [None, "m"]}, t)
    assert got.schema.field("m").type == pa.uint8()
    assert np.array_equal(got["m"].to_numpy().astype(bool), like_mask(t["s"], "%e", True))


# ---- 3. a growing dictionary -------------------------------------------------------------------------------------------------
def test_growing_dictionary_extends_the_table():
    from vinum_amd import _lib as L
    from vinum_amd import set_batch_size
    from vinum_amd.core import FilterOperator, MaterializeTableOperator, TableReaderOperator
    n, batch = 40000, 2500
    # batch b brings the values v<b>_<i>: new values at every batch, half of them matching
    s = [f"{'a' if (i // 7) % 2 else 'b'}{i // batch}_{i % 53}" for i in range(n)]
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "s": pa.array(s, pa.string())})
    set_batch_size(batch)
    try:
        reader = TableReaderOperator(t)
        got = next(MaterializeTableOperator(FilterOperator(("like", "s", ("lit", "a%")), reader)).next())
    finally:
        set_batch_size(1 << 24)
    exp = [k for k, v in enumerate(s) if v.startswith("a")]
    assert got.column("k").to_pylist() == exp
    kd = reader._dicts["s"]
    top = int(L.lib().vnm_strdict_ids(kd.handle()))
    assert kd.like_launches == n // batch              # one launch per batch that brought new values ...
    assert kd.like_ids_matched == top                  # ... and every id matched exactly once (no rebuild per batch)


# ---- 4. the reference's own results -------------------------------------------------------------------------------------------
_TABLES = {}


def _input(name):
    if name not in _TABLES:
        _TABLES[name] = util.read_ipc(f"like_in_{name}.arrow")
    return _TABLES[name]


def _canon(t: pa.Table, case) -> pa.Table:
    cols = {}
    for name in t.schema.names:
        c = t.column(name)
        cols[name] = c.cast(pa.uint8()) if pa.types.is_boolean(c.type) else c   # (a predicate in SELECT: the uint8 mask here)
    t = pa.table(cols)
    keys = case["group_by"] or (["k"] if "k" in t.schema.names else [])
    return t.sort_by([(k, "ascending") for k in keys]) if keys else t


def _compare(got, exp, case):
    assert got.schema.names == exp.schema.names, (got.schema.names, exp.schema.names)
    got, exp = _canon(got, case), _canon(exp, case)
    for name in exp.schema.names:
        g, e = got.column(name).to_pylist(), exp.column(name).to_pylist()
        assert g == e, (case["name"], name, [(a, b) for a, b in zip(g, e) if a != b][:5])


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    from vinum_amd import planner, set_batch_size
    set_batch_size(700)
    try:
        got = planner.execute(case, _input(case["table"]))
    finally:
        set_batch_size(1 << 24)
    _compare(got, util.read_ipc(f"like_{case['name']}.arrow"), case)


@pytest.mark.parametrize("case", [c for c in C.CASES if not c["group_by"]], ids=lambda c: c["name"])
def test_reference_fixtures_through_the_adapter(case):
    from vinum_amd import binding as B
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    from vinum_amd.planner import _raw, _t, output_names
    op = TableReaderOperator(_input(case["table"]))
    if case["where"] is not None:
        op = B.GpuFilterOperator(B.vectorize(_t(case["where"])), op)
    sel = [_t(e) for e in case["select"]]
    op = B.GpuProjectOperator([B.vectorize(e) for e in sel], op,
                              col_names=output_names([_raw(e) for e in case["select"]], case["aliases"]))
    got = next(MaterializeTableOperator(op).next())
    _compare(got, util.read_ipc(f"like_{case['name']}.arrow"), case)


# ---- 5. the GPU CSV reader ---------------------------------------------------------------------------------------------------
def test_csv_reader(tmp_path):
    from vinum_amd import planner
    from vinum_amd.io import stream_csv
    rng = np.random.default_rng(3)
    words = ["Berlin", "Bern", "Bonn", "Munich", "Riva", "San Francisco", "Naples", "Bérgamo", "B"]
    n = 50000
    s = [words[i] for i in rng.integers(0, len(words), n)]
    v = rng.integers(0, 1000, n)
    path = str(tmp_path / "t.csv")
    with open(path, "w", encoding="utf-8") as f:
        f.write("s,v\n")
        for a, b in zip(s, v):
            f.write(f"{a},{b}\n")
    q = {"select": ["s", ["fn", "count"], ["fn", "sum", "v"]], "where": ["like", "s", ["lit", "B%n"]], "group_by": ["s"],
         "aliases": [None, "n", "t"]}
    got = planner.execute(q, stream_csv(path, block_size=1 << 18)).sort_by("s")
    exp = {}
    for a, b in zip(s, v):
        if ref_like("B%n", a, True):
            c, tot = exp.get(a, (0, 0))
            exp[a] = (c + 1, tot + int(b))
    assert got["s"].to_pylist() == sorted(exp)
    assert got["n"].to_pylist() == [exp[k][0] for k in sorted(exp)]
    assert got["t"].to_pylist() == [exp[k][1] for k in sorted(exp)]


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_errors():
    from vinum_amd import planner
    t = pa.table({"s": pa.array(["a", "b"]), "b": pa.array([b"a", b"b"]), "lb": pa.array([b"a", b"b"], pa.large_binary()),
                  "x": pa.array([1.0, 2.0]), "f": pa.array([True, False])})
    for col in ("b", "lb", "x", "f"):
        with pytest.raises(TypeError):
            planner.execute({"select": ["s"], "where": ["like", col, ["lit", "a%"]]}, t)
    for pat in ("a*", "(a)", "a|b", "^a", "a$", "a+", "a?", "[a]", "a{2}", "a\\d"):
        with pytest.raises(NotImplementedError, match="no GPU lowering"):
            planner.execute({"select": ["s"], "where": ["like", "s", ["lit", pat]]}, t)
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        planner.execute({"select": ["s"], "where": ["like", "s", "s"]}, t)         # a column pattern
    with pytest.raises(NotImplementedError, match="no GPU lowering"):
        planner.execute({"select": ["s"], "where": ["like", ["add", "x", 1], ["lit", "a"]]}, t)


# ---- 7. full size -----------------------------------------------------------------------------------------------------------
def test_full_size_filter():
    import torch
    from vinum_amd.core import FilterOperator
    from vinum_amd.core.base import DeviceRecordBatch
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    words = [f"{a}{b}{c}" for a in "JjK" for b in "oa" for c in ("seph", "nas", "e", "")]
    kd = KeyDictionary(pa.string())
    codes = np.unique(kd.encode(pa.array(words)).to_numpy(zero_copy_only=False)).astype(np.int32)
    n = 500_000_000
    g = torch.Generator(device="cuda").manual_seed(1)
    pick = torch.randint(0, len(codes), (n,), device="cuda", generator=g)
    rows = torch.from_numpy(codes).cuda()[pick].contiguous()
    del pick
    col = DeviceColumn.from_torch(rows)
    col.dictionary = kd
    batch = DeviceRecordBatch({"s": col}, n)
    out = FilterOperator(("like", "s", ("lit", "J%e%")), None)._kernel(batch)
    tab = torch.from_numpy(kd.like_table("J%e%")._values.to_host(np.uint8, int(codes.max()) + 1)).cuda()
    assert out.num_rows == int(tab[rows.long()].sum().item())
    assert out.num_rows > 0


def test_several_patterns_on_one_column_in_one_select_list():
    from vinum_amd import planner
    t = _nullable_table()
    got = planner.execute({"select": ["k", ["like", "s", ["lit", "Jo%"]], ["like", "s", ["lit", "%e"]],
                                      ["fn", "to_int", ["not_like", "s", ["lit", "J%"]]]],
                           "aliases": [None, "a", "b", "c"]}, t)
    assert np.array_equal(got["a"].to_numpy().astype(bool), like_mask(t["s"], "Jo%"))
    assert np.array_equal(got["b"].to_numpy().astype(bool), like_mask(t["s"], "%e"))
    assert np.array_equal(got["c"].to_numpy(), like_mask(t["s"], "J%", True).astype(np.int64))
    got = planner.execute({"select": ["v", ["fn", "sum", ["fn", "to_int", ["like", "s", ["lit", "Jo%"]]]],
                                      ["fn", "sum", ["fn", "to_int", ["like", "s", ["lit", "%s%"]]]]],
                           "group_by": ["v"], "aliases": [None, "a", "b"]}, t).sort_by("v")
    v = t["v"].to_numpy()
    a, b = like_mask(t["s"], "Jo%"), like_mask(t["s"], "%s%")
    keys = np.unique(v)
    assert got["a"].to_pylist() == [int(a[v == x].sum()) for x in keys]
    assert got["b"].to_pylist() == [int(b[v == x].sum()) for x in keys]
