"""Two dictionary-coded string / binary columns compared with each other on the GPU: the two dictionary primitives
(vnm_strdict_translate, vnm_strdict_ranks_joint) against host dict lookups and the sorted union, VNM_EX_LOOKUP_I32 against NumPy,
and `a <op> b` / BETWEEN through FilterOperator, ProjectOperator, the planner and an aggregate against pyarrow over the columns
cast to binary (NULL rows by the project's rule: compare False, `!=` True)."""

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

pytestmark = pytest.mark.gpu

N = 70_001          # more than one 1024-row tile, no multiple of 64
OPS = {"eq": pc.equal, "ne": pc.not_equal, "lt": pc.less, "le": pc.less_equal, "gt": pc.greater, "ge": pc.greater_equal}


# ---- 1. the primitives through raw ctypes ---------------------------------------------------------------------------------
def _special():
    """the empty string, the prefix triple, multi-byte code points, the 8-byte chunk boundary (7 / 8 / 9) and the 15-chunk
    boundary of the rank sort (120 / 121) and three rounds (300), with neighbours that differ in their LAST byte only"""
    out = ["", "a", "a\x00", "ab", "ü", "üa", "€", "😀é", "a😀"]
    for n in (7, 8, 9, 120, 121, 300):
        out += ["p" * (n - 1) + "a", "p" * (n - 1) + "b", "p" * n]
    return out


def _pools():
    """two value lists of about 3000 values each, half of them shared, each in an insertion order of its own"""
    rng = np.random.default_rng(3)
    words = [f"{'wxyz'[i % 4]}{i * 7919 % 100003:06d}{'q' * (i % 11)}" for i in range(4500)]
    sp = _special()
    a = words[:3000] + sp[::2] + sp[1::4]
    b = words[1500:] + sp[1::2] + sp[::4]
    a = [a[i] for i in rng.permutation(len(a))]
    b = [b[i] for i in rng.permutation(len(b))]
    assert len(set(a)) == len(a) and len(set(b)) == len(b)
    return a, b


def _dict_of(values, arrow_type=pa.string()):
    """(KeyDictionary, {bytes: id}) after one encode of distinct values"""
    from vinum_amd.vinum_lib import KeyDictionary
    kd = KeyDictionary(arrow_type)
    ids = {}
    _grow(kd, ids, values)
    return kd, ids


def _grow(kd, ids, values):
    if values:
        codes = kd.encode(pa.array(values, kd.type)).to_numpy(zero_copy_only=False)
        for v, c in zip(values, codes):
            ids[v.encode() if isinstance(v, str) else v] = int(c)


def _top(kd):
    from vinum_amd import _lib as L
    return int(L.lib().vnm_strdict_ids(kd.handle()))


def _translate(src, dst, id_begin=0, into=None):
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    top = _top(src)
    buf = DeviceBuffer.from_host(np.full(max(top, 1), -7, np.int32) if into is None else
                                 np.concatenate([into, np.full(max(top, 1) - len(into), -7, np.int32)]))
    L.check(L.lib().vnm_strdict_translate(src.handle(), dst.handle(), id_begin, buf.ptr, None))
    L.check(L.lib().vnm_device_synchronize())
    return buf.to_host(np.int32, top)


def _expected_translate(src_ids, dst_ids, top):
    exp = np.full(top, -2, np.int32)            # ids never handed out: -2 as well
    for v, i in src_ids.items():
        exp[i] = dst_ids.get(v, -2)
    return exp


def _joint(a, b):
    from vinum_amd import _lib as L
    from vinum_amd.device import DeviceBuffer
    ta, tb = _top(a), _top(b)
    ba, bb = DeviceBuffer.from_host(np.full(max(ta, 1), -7, np.int32)), DeviceBuffer.from_host(np.full(max(tb, 1), -7, np.int32))
    L.check(L.lib().vnm_strdict_ranks_joint(a.handle(), b.handle(), ba.ptr, bb.ptr, None))
    L.check(L.lib().vnm_device_synchronize())
    return ba.to_host(np.int32, ta), bb.to_host(np.int32, tb)


def _expected_joint(a_ids, b_ids, ta, tb):
    rank = {v: r for r, v in enumerate(sorted(set(a_ids) | set(b_ids)))}      # Python orders bytes byte-wise, a prefix first
    ea, eb = np.full(ta, -7, np.int32), np.full(tb, -7, np.int32)             # ids never handed out: left untouched
    for v, i in a_ids.items():
        ea[i] = rank[v]
    for v, i in b_ids.items():
        eb[i] = rank[v]
    return ea, eb


def test_translate_and_joint_ranks_against_the_host():
    va, vb = _pools()
    a, a_ids = _dict_of(va)
    b, b_ids = _dict_of(vb, pa.large_binary())              # (bytes are bytes: the Arrow types need not agree)
    got = _translate(a, b)
    assert np.array_equal(got, _expected_translate(a_ids, b_ids, _top(a)))
    assert (got == -2).sum() >= 1400 and (got >= 0).sum() >= 1400           # about half present, half absent
    assert np.array_equal(_translate(b, a), _expected_translate(b_ids, a_ids, _top(b)))
    ga, gb = _joint(a, b)
    ea, eb = _expected_joint(a_ids, b_ids, _top(a), _top(b))
    assert np.array_equal(ga, ea) and np.array_equal(gb, eb)
    # dst grows: values that were absent are present now -- the whole table again (id_begin = 0)
    _grow(b, b_ids, [v.encode() for v in va[:700] if v.encode() not in b_ids])
    again = _translate(a, b)
    assert np.array_equal(again, _expected_translate(a_ids, b_ids, _top(a))) and (again != got).sum() >= 300
    # only src grows: the table is extended from the id count it covers
    old = _top(a)
    _grow(a, a_ids, [f"late{i}" for i in range(500)] + [vb[i] for i in range(0, 2000, 3) if vb[i].encode() not in a_ids])
    assert _top(a) > old
    ext = _translate(a, b, id_begin=old, into=again)
    assert np.array_equal(ext, _expected_translate(a_ids, b_ids, _top(a)))
    ga, gb = _joint(a, b)
    ea, eb = _expected_joint(a_ids, b_ids, _top(a), _top(b))
    assert np.array_equal(ga, ea) and np.array_equal(gb, eb)


def test_translate_and_joint_ranks_edge_cases():
    from vinum_amd.vinum_lib import KeyDictionary
    va, vb = _pools()
    # disjoint dictionaries
    a, a_ids = _dict_of([v for v in va if v.startswith("w")][:300])
    b, b_ids = _dict_of([v for v in vb if v.startswith("x")][:300])
    assert (_translate(a, b) == -2).all()
    ga, gb = _joint(a, b)
    ea, eb = _expected_joint(a_ids, b_ids, _top(a), _top(b))
    assert np.array_equal(ga, ea) and np.array_equal(gb, eb)
    # identical contents in two handles, inserted in opposite orders
    c, c_ids = _dict_of(va[:1000])
    d, d_ids = _dict_of(va[:1000][::-1])
    assert np.array_equal(_translate(c, d), _expected_translate(c_ids, d_ids, _top(c)))
    gc, gd = _joint(c, d)
    ec, ed = _expected_joint(c_ids, d_ids, _top(c), _top(d))
    assert np.array_equal(gc, ec) and np.array_equal(gd, ed) and gc.max() == 999
    # one dictionary without a value
    z = KeyDictionary(pa.string())
    assert len(_translate(z, c)) == 0
    assert (_translate(c, z) == -2).all()
    gc, gz = _joint(c, z)
    assert np.array_equal(gc, _expected_joint(c_ids, {}, _top(c), 0)[0]) and len(gz) == 0
    gz, gc = _joint(z, c)
    assert np.array_equal(gc, _expected_joint(c_ids, {}, _top(c), 0)[0])


# ---- 2. the opcode ------------------------------------------------------------------------------------------------------------
def _opcode_inputs():
    from vinum_amd.device import DeviceColumn
    rng = np.random.default_rng(9)
    T = 1000
    table = rng.integers(-2, 500, T).astype(np.int32)
    codes = rng.integers(0, T, N).astype(np.int32)
    codes[rng.random(N) < 0.05] = -1
    codes[rng.random(N) < 0.05] = -2
    codes[rng.random(N) < 0.05] = T                  # just past the table
    codes[rng.random(N) < 0.02] = 2**31 - 1
    null = rng.random(N) < 0.1
    x = rng.integers(-2, 500, N).astype(np.int32)
    v = rng.integers(0, 100, N).astype(np.float64)
    inside = ~null & (codes >= 0) & (codes < T)
    val = np.where(inside, table[np.clip(codes, 0, T - 1)].astype(np.float64), np.nan)
    cols = {"c": DeviceColumn.from_arrow(pa.array(codes, pa.int32(), mask=null)), "t": DeviceColumn.from_numpy(table),
            "x": DeviceColumn.from_numpy(x), "v": DeviceColumn.from_numpy(v)}
    return cols, val, x, v


def test_lookup_i32_alone_and_composed():
    from vinum_amd import ops
    cols, val, x, v = _opcode_inputs()
    look = ("lookup_i32", "c", "t")
    with np.errstate(invalid="ignore"):
        cases = [
            (("eq", "x", look), x == val), (("ne", look, "x"), val != x), (("lt", look, "x"), val < x), (("ge", "x", look), x >= val),
            (("and", ("eq", "x", look), ("gt", "v", 50)), (x == val) & (v > 50)),
            (("or", ("not", ("le", look, "x")), ("lt", "v", 10)), ~(val <= x) | (v < 10)),
            (("not", ("or", ("eq", look, 7), ("and", ("gt", look, "x"), ("le", "v", 80)))), ~((val == 7) | ((val > x) & (v <= 80)))),
        ]
    for expr, exp in cases:
        got = ops.project(expr, {n: cols[n] for n in ops.columns_of(expr)}, length=N)
        assert got.arrow_type == pa.uint8()
        assert np.array_equal(got.to_numpy().astype(bool), exp), expr
    alone = ops.project(look, {"c": cols["c"], "t": cols["t"]}, length=N)
    assert alone.arrow_type == pa.float64() and np.array_equal(alone.to_numpy(), val, equal_nan=True)
    # in one pass with other outputs (vnm_project_multi)
    many = ops.project_many([("eq", "x", look), ("add", "v", 1), ("to_int", ("ne", "x", look))], cols, length=N)
    assert np.array_equal(many[0].to_numpy().astype(bool), x == val) and np.array_equal(many[1].to_numpy(), v + 1)
    assert np.array_equal(many[2].to_numpy(), (x != val).astype(np.int64))


def test_lookup_i32_refusals():
    from vinum_amd import _lib as L
    from vinum_amd import ops
    from vinum_amd.device import DeviceColumn
    cols, _, _, _ = _opcode_inputs()
    expr = ("eq", "x", ("lookup_i32", "c", "t"))

    def run(**swap):
        use = dict(cols, **swap)
        return ops.project(expr, {n: use[n] for n in ops.columns_of(expr)}, length=N)

    with pytest.raises(L.VinumHipError, match="int32 column without NULLs"):
        run(t=DeviceColumn.from_numpy(np.zeros(1000, np.uint8)))
    with pytest.raises(L.VinumHipError, match="int32 column without NULLs"):
        run(t=DeviceColumn.from_arrow(pa.array([1, None, 3], pa.int32())))
    with pytest.raises(L.VinumHipError, match="int32 dictionary codes"):
        run(c=DeviceColumn.from_numpy(np.zeros(N, np.int64)))
    with pytest.raises(L.VinumHipError, match="lookup table, not a row column"):
        ops.project(("and", expr, ("eq", "t", 1)), cols, length=N)


# ---- 3. the operators against pyarrow ---------------------------------------------------------------------------------------
_PAIRS = {"utf8_utf8": ("a", "b", "c"), "utf8_large": ("a", "lb", "c"), "binary_binary": ("ba", "bb", "bc")}
_TABLES = {}


def _table(nulls):
    """a, b, c draw from three overlapping pools in different insertion orders; lb / ba / bb / bc are b / a / b / c in another type"""
    if nulls in _TABLES:
        return _TABLES[nulls]
    rng = np.random.default_rng(17)
    pool = _special() + [f"v{i:03d}" for i in range(300)]
    pa_, pb_, pc_ = pool[:220], pool[100:], pool[50:280][::-1]
    a = [pa_[i] for i in rng.integers(0, len(pa_), N)]
    b = [pb_[i] for i in rng.integers(0, len(pb_), N)]
    c = [pc_[i] for i in rng.integers(0, len(pc_), N)]
    same = rng.random(N) < 0.3
    b = [x if s else y for x, y, s in zip(a, b, same)]
    na = rng.random(N) < 0.1 if nulls in ("a", "both") else None
    nb = rng.random(N) < 0.1 if nulls in ("b", "both") else None
    enc = lambda xs: [x.encode() for x in xs]   # noqa: E731
    t = pa.table({
        "k": pa.array(np.arange(N, dtype=np.int64)), "g": pa.array(rng.integers(0, 5, N).astype(np.int64)),
        "v": pa.array(rng.integers(0, 100, N).astype(np.float64)),
        "a": pa.array(a, pa.string(), mask=na), "b": pa.array(b, pa.string(), mask=nb), "c": pa.array(c, pa.string()),
        "lb": pa.array(b, pa.large_string(), mask=nb),
        "ba": pa.array(enc(a), pa.binary(), mask=na), "bb": pa.array(enc(b), pa.binary(), mask=nb), "bc": pa.array(enc(c), pa.binary()),
    })
    _TABLES[nulls] = t
    return t


def _bin(col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return col.cast(pa.large_binary())


def _mask(t, op, x, y):
    """pyarrow over the columns cast to binary; NULL rows by the project's rule"""
    m = OPS[op](_bin(t[x]), _bin(t[y]))
    return m.fill_null(op == "ne").to_numpy(zero_copy_only=False)


def _between(t, x, lo, hi, invert=False):
    return (_mask(t, "lt", x, lo) | _mask(t, "gt", x, hi)) if invert else (_mask(t, "ge", x, lo) & _mask(t, "le", x, hi))


@pytest.mark.parametrize("nulls", ["neither", "a", "b", "both"])
@pytest.mark.parametrize("pair", list(_PAIRS))
def test_select_list_through_the_planner(pair, nulls):
    """all six operators and both BETWEENs as SELECT-list predicates: plan_query -> ProjectOperator, several batches"""
    from vinum_amd import planner, set_batch_size
    t = _table(nulls)
    x, y, z = _PAIRS[pair]
    select = ["k"] + [[op, x, y] for op in OPS] + [["between", x, y, z], ["not_between", x, z, y]]
    names = [None] + list(OPS) + ["bt", "nbt"]
    set_batch_size(30_000)
    try:
        got = planner.execute({"select": select, "aliases": names}, t)
    finally:
        set_batch_size(1 << 24)
    assert got.column("k").to_pylist() == list(range(N))
    for op in OPS:
        assert got.schema.field(op).type == pa.uint8()             # a predicate in SELECT stays the uint8 mask
        assert np.array_equal(got[op].to_numpy().astype(bool), _mask(t, op, x, y)), (pair, nulls, op)
    assert np.array_equal(got["bt"].to_numpy().astype(bool), _between(t, x, y, z))
    assert np.array_equal(got["nbt"].to_numpy().astype(bool), _between(t, x, z, y, True))


@pytest.mark.parametrize("op", list(OPS) + ["between", "not_lt"])
def test_filter_operator(op):
    from vinum_amd import set_batch_size
    from vinum_amd.core import FilterOperator, MaterializeTableOperator, TableReaderOperator
    t = _table("both")
    if op == "between":
        pred, exp = ("between", "a", "b", "c"), _between(t, "a", "b", "c")
    elif op == "not_lt":
        pred, exp = ("and", ("not", ("lt", "a", "lb")), ("gt", "v", 20)), ~_mask(t, "lt", "a", "lb") & (t["v"].to_numpy() > 20)
    else:
        pred, exp = (op, "a", "b"), _mask(t, op, "a", "b")
    set_batch_size(25_000)
    try:
        got = next(MaterializeTableOperator(FilterOperator(pred, TableReaderOperator(t, ["k", "a", "b", "lb", "c", "v"]))).next())
    finally:
        set_batch_size(1 << 24)
    want = t.filter(pa.array(exp))
    assert got.column("k").to_pylist() == want.column("k").to_pylist()
    assert got.column("a").to_pylist() == want.column("a").to_pylist()


@pytest.mark.parametrize("where", [["eq", "a", "b"], ["or", ["lt", "ba", "bb"], ["eq", "a", ["lit", "ab"]]], ["between", "a", "lb", "c"]])
def test_where_through_the_planner(where):
    from vinum_amd import planner
    t = _table("both")
    exp = {"eq": lambda: _mask(t, "eq", "a", "b"), "or": lambda: _mask(t, "lt", "ba", "bb") | pc.equal(t["a"], "ab").fill_null(False).to_numpy(zero_copy_only=False),
           "between": lambda: _between(t, "a", "lb", "c")}[where[0]]()
    got = planner.execute({"select": ["k", "b"], "where": where}, t)
    want = t.filter(pa.array(exp))
    assert got.column("k").to_pylist() == want.column("k").to_pylist()
    assert got.column("b").to_pylist() == want.column("b").to_pylist()


@pytest.mark.parametrize("nulls", ["neither", "both"])
def test_sum_to_int_in_an_aggregate(nulls):
    from vinum_amd import planner, set_batch_size
    t = _table(nulls)
    q = {"select": ["g", ["fn", "sum", ["fn", "to_int", ["eq", "a", "b"]]], ["fn", "sum", ["fn", "to_int", ["lt", "a", "lb"]]]],
         "group_by": ["g"], "aliases": [None, "same", "less"]}
    set_batch_size(20_000)
    try:
        got = planner.execute(q, t)
    finally:
        set_batch_size(1 << 24)
    g = t["g"].to_numpy()
    eq, lt = _mask(t, "eq", "a", "b"), _mask(t, "lt", "a", "lb")
    exp = {int(k): (int(eq[g == k].sum()), int(lt[g == k].sum())) for k in np.unique(g)}
    assert {k: (s, l) for k, s, l in zip(got["g"].to_pylist(), got["same"].to_pylist(), got["less"].to_pylist())} == exp


def test_columns_sharing_one_dictionary_and_a_zero_row_batch():
    from vinum_amd.core import FilterOperator
    from vinum_amd.core.base import DeviceRecordBatch
    from vinum_amd.device import DeviceColumn
    from vinum_amd.vinum_lib import KeyDictionary
    t = _table("both")
    kd = KeyDictionary(pa.string())
    cols = {"k": DeviceColumn.from_arrow(t["k"]), "a": DeviceColumn.from_arrow(t["a"], dictionary=kd),
            "b": DeviceColumn.from_arrow(t["b"], dictionary=kd)}
    batch = DeviceRecordBatch(cols, N)
    for op in OPS:
        pred, extra = FilterOperator.lower_dictionary_predicates((op, "a", "b"), batch)
        assert not any("lookup_i32" in str(x) for x in pred) and kd.translate_builds == 0 and kd.joint_rank_builds == 0
        got = FilterOperator((op, "a", "b"), None)._kernel(batch)
        assert got.columns["k"].to_arrow().to_pylist() == np.flatnonzero(_mask(t, op, "a", "b")).tolist(), op
    schema = t.select(["k", "a", "b", "c"]).schema
    empty = DeviceRecordBatch.from_arrow(pa.RecordBatch.from_arrays([pa.array([], f.type) for f in schema], names=schema.names), {})
    for pred in (("eq", "a", "b"), ("lt", "a", "b"), ("between", "a", "b", "c")):
        assert FilterOperator(pred, None)._kernel(empty).num_rows == 0


# ---- 4. growing dictionaries ------------------------------------------------------------------------------------------------
def test_growing_dictionaries_rebuild_the_tables_once_per_growth():
    from vinum_amd import set_batch_size
    from vinum_amd.core import FilterOperator, MaterializeTableOperator, TableReaderOperator
    B = 5000
    w = lambda lo, hi: [f"s{i:04d}" for i in range(lo, hi)]   # noqa: E731
    rng = np.random.default_rng(2)
    draw = lambda vals: [vals[i] for i in rng.integers(0, len(vals), B)]   # noqa: E731
    # batch 0: both dictionaries start; 1: new values in a only; 2: new values in b only (some of them already in a);
    # 3: batch 2 again -- nothing new; 4: new values in both
    parts = [(draw(w(0, 100)), draw(w(50, 150))), (draw(w(0, 200)), draw(w(50, 150))), (draw(w(0, 200)), draw(w(50, 260)))]
    parts.append(parts[2])
    parts.append((draw(w(0, 400)), draw(w(300, 500))))
    a = sum((p[0] for p in parts), [])
    b = sum((p[1] for p in parts), [])
    t = pa.table({"k": pa.array(np.arange(len(a), dtype=np.int64)), "a": pa.array(a, pa.string()), "b": pa.array(b, pa.large_string())})
    for pred, op, counter in ((("eq", "a", "b"), "eq", "translate_builds"), (("lt", "a", "b"), "lt", "joint_rank_builds")):
        set_batch_size(B)
        try:
            reader = TableReaderOperator(t)
            got = next(MaterializeTableOperator(FilterOperator(pred, reader)).next())
        finally:
            set_batch_size(1 << 24)
        assert got.column("k").to_pylist() == np.flatnonzero(_mask(t, op, "a", "b")).tolist()       # correct in every batch
        da, db = reader._dicts["a"], reader._dicts["b"]
        builds = getattr(db if op == "eq" else da, counter)
        assert builds == 4, builds                       # one per batch in which a dictionary grew, none for the repeated batch
        assert getattr(da if op == "eq" else db, counter) == 0


# ---- 5. what comparing the codes would give -----------------------------------------------------------------------------------
def test_where_a_equals_b_with_opposite_insertion_orders():
    """a's dictionary meets the values in ascending order, b's in descending order: the codes of equal values differ and equal codes
    mean different values, so a comparison of the two code columns gives another mask than the values do"""
    from vinum_amd import planner
    from vinum_amd.core.base import DeviceRecordBatch
    vals = [f"city{i:03d}" for i in range(64)]
    n = 4096
    a = [vals[i % 64] for i in range(n)]
    b = [vals[63 - (i % 64)] if i % 3 else vals[i % 64] for i in range(n)]
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "a": pa.array(a, pa.string()), "b": pa.array(b, pa.string())})
    dev = DeviceRecordBatch.from_arrow(t.to_batches()[0], {})
    by_codes = dev.columns["a"].to_numpy() == dev.columns["b"].to_numpy()
    exp = np.array([x == y for x, y in zip(a, b)])
    assert (by_codes != exp).any()                               # (the data does tell the two apart)
    got = planner.execute({"select": ["k"], "where": ["eq", "a", "b"]}, t)
    assert got.column("k").to_pylist() == np.flatnonzero(exp).tolist()


# ---- 6. the reference's own results (tests/golden/strcmp_*.arrow, gen_golden_strcmp.py) ------------------------------------
def _fixture_cases():
    import json
    import os
    from tests.golden import strcmp_cases as C
    with open(os.path.join(os.path.dirname(os.path.abspath(C.__file__)), "strcmp_cases.json")) as f:
        written = json.load(f)["cases"]
    return [c for c in C.CASES if c["name"] in written]           # (a case the reference raised on has no fixture)


def _canon(t, case):
    cols = {n: (t.column(n).cast(pa.uint8()) if pa.types.is_boolean(t.column(n).type) else t.column(n)) for n in t.schema.names}
    key = case["group_by"][0] if case["group_by"] else "k"       # (a predicate in SELECT: the uint8 mask here)
    return pa.table(cols).sort_by(key)


def _compare(got, name, case):
    from tests import util
    exp = util.read_ipc(f"strcmp_{name}.arrow")
    assert got.schema.names == exp.schema.names
    got, exp = _canon(got, case), _canon(exp, case)
    for n in exp.schema.names:
        assert got.column(n).to_pylist() == exp.column(n).to_pylist(), (name, n)


@pytest.mark.parametrize("case", _fixture_cases(), ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    from tests import util
    from vinum_amd import planner, set_batch_size
    set_batch_size(16)
    try:
        got = planner.execute(case, util.read_ipc("strcmp_in_main.arrow"))
    finally:
        set_batch_size(1 << 24)
    _compare(got, case["name"], case)


@pytest.mark.parametrize("case", [c for c in _fixture_cases() if not c["group_by"]], ids=lambda c: c["name"])
def test_reference_fixtures_through_the_adapter(case):
    """The adapter's operators (binding.GpuFilterOperator / GpuProjectOperator over binding.vectorize trees, so binding.lower and
    the lowering behind it run) built by hand: binding.install() itself rebinds names inside the reference's package, which a GPU
    machine does not have, so the installed route is not exercised here, and neither is the GROUP BY / HAVING fixture, whose
    aggregate the adapter builds from the reference's planner classes (the planner test above replays it)."""
    from tests import util
    from vinum_amd import binding as B
    from vinum_amd.core import MaterializeTableOperator, TableReaderOperator
    from vinum_amd.planner import _raw, _t, output_names
    op = TableReaderOperator(util.read_ipc("strcmp_in_main.arrow"))
    if case["where"] is not None:
        op = B.GpuFilterOperator(B.vectorize(_t(case["where"])), op)
    sel = [_t(e) for e in case["select"]]
    op = B.GpuProjectOperator([B.vectorize(e) for e in sel], op, col_names=output_names([_raw(e) for e in case["select"]], case["aliases"]))
    _compare(next(MaterializeTableOperator(op).next()), case["name"], case)
