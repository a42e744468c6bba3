"""IN / NOT IN lists probed as device-resident sets (vnm_inset.hip): the probe against exact Python membership (integer
domains) and np.isin (float64 domain) over every column type, row count, offset and set size at which the kernel takes another
path; the operators with lists the projection interpreter cannot hold; chain and set route against each other; string columns;
the reference's own results (tests/golden/in_set_*.arrow) through the planner; one leg under the pool's guard mode."""
import ctypes
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from tests import util
from tests.golden import in_set_cases as C

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
INT_TYPES = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64,
             "uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32, "uint64": np.uint64}
TILE = 8192          # rows per workgroup of in_set_kernel: only full tiles of an aligned 8-byte column come in as 16-byte loads
ROWS = [1, 3, 1023, 1024, 1025, 4099, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]


def _route():
    from vinum_amd import _lib as L
    buf = ctypes.create_string_buffer(1024)
    L.lib().vnm_route_last(buf, len(buf))
    return buf.value.decode()


def _probe(col, values, invert=False):
    from vinum_amd import ops
    out = ops.in_set_probe(col, values, invert=invert)
    m = out.to_numpy()
    assert m.dtype == np.uint8 and len(m) == col.length and set(np.unique(m).tolist()) <= {0, 1}
    return m.astype(bool)


def _dev(arr, mask=None, t=None):
    from vinum_amd.device import DeviceColumn
    return DeviceColumn.from_arrow(pa.array(arr, type=t, mask=mask))


def _exact(values, members):
    """membership with Python ints: no promotion anywhere"""
    s = {int(m) for m in members}
    return np.array([int(v) in s for v in values.tolist()], bool)


def _check_int(arr, members, route=None):
    col = _dev(arr)
    exp = _exact(arr, members)
    got = _probe(col, members)
    if route is not None:
        assert _route().startswith(route + ":"), _route()
    assert np.array_equal(got, exp), (arr.dtype, np.flatnonzero(got != exp)[:5])
    assert np.array_equal(_probe(col, members, invert=True), ~exp)
    return exp


# ---- 1. what the parent commit cannot run -------------------------------------------------------------------------------------
def _operator_table(n=4099):
    rng = np.random.default_rng(1)
    return pa.table({"k": pa.array(np.arange(n, dtype=np.int64)),
                     "a": pa.array(rng.integers(0, 20000, n).astype(np.int64)),
                     "s": pa.array([f"w{i}" for i in rng.integers(0, 9000, n)], pa.string())})


@pytest.mark.parametrize("members", [17, 100, 5000])
@pytest.mark.parametrize("column", ["a", "s"])
def test_operators_with_lists_the_interpreter_cannot_hold(column, members):
    """fails on the parent commit: `vnm_project: program must have 1..63 instructions`"""
    from vinum_amd.core import FilterOperator, ProjectOperator
    from vinum_amd.core.base import DeviceRecordBatch
    t = _operator_table()
    rng = np.random.default_rng(members)
    if column == "a":
        vals = tuple(int(x) for x in rng.choice(20000, members, replace=False))
        lits = vals
    else:
        vals = tuple(f"w{i}" for i in rng.choice(12000, members, replace=False))      # a quarter of them is in no row
        lits = tuple(("lit", v) for v in vals)
    exp = np.array([v in set(vals) for v in t.column(column).to_pylist()], bool)
    assert 0 < exp.sum() < len(exp)
    batch = DeviceRecordBatch.from_arrow(t.to_batches()[0], {})
    kept = FilterOperator(("in", column, lits), None)._kernel(batch).to_arrow()
    assert kept.column("k").to_pylist() == np.flatnonzero(exp).tolist()
    assert kept.column(column).to_pylist() == [v for v, e in zip(t.column(column).to_pylist(), exp) if e]
    kept = FilterOperator(("and", ("not_in", column, vals), ("lt", "k", 3000)), None)._kernel(batch).to_arrow()
    assert kept.column("k").to_pylist() == [k for k in np.flatnonzero(~exp).tolist() if k < 3000]
    out = ProjectOperator(["k", ("in", column, vals), ("not_in", column, lits)], None, col_names=["k", "m", "nm"])._kernel(batch).to_arrow()
    assert out.column("m").type == pa.uint8()
    assert np.array_equal(out.column("m").to_numpy().astype(bool), exp)
    assert np.array_equal(out.column("nm").to_numpy().astype(bool), ~exp)


# ---- 2. integer domains: exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INT_TYPES))
@pytest.mark.parametrize("dense", [False, True], ids=["sorted", "bitmap"])
def test_integer_domains_are_exact(name, dense):
    dt = INT_TYPES[name]
    info = np.iinfo(dt)
    lo, hi = int(info.min), int(info.max)
    rng = np.random.default_rng(len(name) + dense)
    if dense:
        base = max(lo, min(hi - 70, 40)) if lo >= 0 else -20
        members = [base + d for d in range(0, 70) if d % 7 != 3]                     # gaps inside the range
    else:
        inside = sorted({int(x) for x in rng.integers(max(lo, -10**6), min(hi, 10**6), 40, endpoint=True)})
        # outside the column type's range (the column is widened, the member never narrowed), the int64 extremes, the type's own
        members = inside + [hi + 1 if hi < I64_MAX else hi, lo - 1 if lo > I64_MIN else lo, hi + 256, lo - 256 if lo > I64_MIN else lo,
                            I64_MIN, I64_MAX, lo, hi, 300, -1]
        members = [m for m in members if I64_MIN <= m <= I64_MAX]
    ms = sorted(set(members))
    probes = [ms[0], ms[-1], ms[0] - 1, ms[-1] + 1] + [m + 1 for m in ms] + [m - 1 for m in ms] + ms + [lo, hi, lo + 1, hi - 1, 0]
    if name == "uint64":
        probes += [2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1, 2**64 - 2]                 # values >= 2^63 match nothing
    if name == "int8":
        probes += [44]                                                                # what 300 would wrap to
    probes = [p for p in probes if lo <= p <= hi]
    arr = np.concatenate([np.array(probes, dtype=dt), rng.integers(lo, hi, 1025 - len(probes) % 1025, dtype=dt, endpoint=True)])
    exp = _check_int(arr, members, "in_set:bitmap_lds" if dense else "in_set:sorted_lds")
    assert exp.any() and not exp.all()
    assert ("domain=u64" if name == "uint64" else "domain=i64") in _route()


def test_int64_extremes_as_a_bitmap():
    arr = np.array([I64_MAX, I64_MAX - 1, I64_MAX - 2, I64_MIN, 0, -1, I64_MAX - 3] * 3, np.int64)
    _check_int(arr, [I64_MAX, I64_MAX - 2], "in_set:bitmap_lds")
    arr = np.array([I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX, 0, -1, I64_MIN + 65] * 3, np.int64)
    _check_int(arr, [I64_MIN, I64_MIN + 2, I64_MIN + 64], "in_set:bitmap_lds")
    _check_int(arr, [I64_MIN, I64_MAX, 0], "in_set:sorted_lds")


# ---- 3. the float64 domain against np.isin ---------------------------------------------------------------------------------
_TINY = np.float64(5e-324)
FLOAT_SPECIALS = [np.nan, 0.0, -0.0, np.inf, -np.inf, _TINY, -_TINY, 2.2250738585072014e-308, 1.0, -1.0, 0.1, 2.5, 1e300, -1e300]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("members", [[0.0, np.nan, np.inf, _TINY, 0.1, 2.5], [-0.0, -np.inf, 1, 7], [3, 1, 2**24 + 1, -1]],
                         ids=["floats", "neg_zero", "ints"])
def test_float_columns_against_numpy(dt, members):
    rng = np.random.default_rng(2)
    f32_specials = [np.float32(1e-45), np.float32(0.1), np.float32(2**24 + 1)]
    with np.errstate(over="ignore"):             # (1e300 is inf as a float32)
        arr = np.concatenate([np.array(FLOAT_SPECIALS, dt), np.array(f32_specials, dt), rng.integers(-8, 8, 1025).astype(dt) / dt(2)])
    members = [float(m) if isinstance(m, (float, np.floating)) else m for m in members]
    lst = np.array(members, np.float64 if any(isinstance(m, float) for m in members) else np.int64)
    with np.errstate(invalid="ignore"):
        exp = np.isin(arr, lst)
    col = _dev(arr)
    got = _probe(col, members)
    assert "domain=f64" in _route() and _route().startswith("in_set:sorted_lds:")
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]
    assert np.array_equal(_probe(col, members, invert=True), np.isin(arr, lst, invert=True))
    assert not got[0]                               # NaN is in no list, not even one that holds NaN


@pytest.mark.parametrize("name", list(INT_TYPES))
def test_integer_columns_with_nulls_compare_as_float64(name):
    dt = INT_TYPES[name]
    info = np.iinfo(dt)
    rng = np.random.default_rng(3)
    arr = rng.integers(max(info.min, -60), min(info.max, 60), 1500, dtype=dt, endpoint=True)
    null = rng.random(len(arr)) < 0.3
    members = list(range(-50, 50, 3)) + [min(int(info.max), I64_MAX), 1000]
    a = pa.array(arr, mask=null)
    as_numpy = a.to_numpy(zero_copy_only=False)           # float64 with NaN: what the reference hands np.isin
    assert as_numpy.dtype == np.float64
    from vinum_amd.device import DeviceColumn
    col = DeviceColumn.from_arrow(a)
    got = _probe(col, members)
    assert "domain=f64" in _route()
    assert np.array_equal(got, np.isin(as_numpy, np.array(members)))
    inv = _probe(col, members, invert=True)
    assert np.array_equal(inv, np.isin(as_numpy, np.array(members), invert=True))
    assert inv[null].all() and not got[null].any()        # a NULL row: IN is False, NOT IN is True


def test_int64_beyond_2_53_against_a_float_list():
    big = 2**53
    arr = np.array([big, big + 1, big + 2, big + 3, -big - 1, 7, I64_MAX, I64_MIN] * 130, np.int64)
    members = [float(big), 7.0, 2.0**63, 0.5]
    exp = np.isin(arr, np.array(members))                 # NumPy compares both as float64: big + 1 IS float(big)
    got = _probe(_dev(arr), members)
    assert np.array_equal(got, exp) and got[1] and got[6]
    u = np.array([2**64 - 1, 2**63, 2**63 + 1, 5], np.uint64)
    assert np.array_equal(_probe(_dev(u), [2.0**64, 2.0**63, 5.0]), np.isin(u, np.array([2.0**64, 2.0**63, 5.0])))


# ---- 4. row counts, offsets, validity offsets ------------------------------------------------------------------------------------
_ROW_MEMBERS = [5, 9, 12, 700, 701, 900, -3]           # a sorted table
_ROW_DENSE = list(range(0, 600, 2))                    # a bitmap


@pytest.mark.parametrize("n", ROWS)
def test_row_counts(n):
    from vinum_amd.device import DeviceColumn
    rng = np.random.default_rng(n)
    for dt in (np.int64, np.float64, np.int32, np.uint8):
        arr = rng.integers(0, 200, n + 1).astype(dt)
        for members in (_ROW_MEMBERS, _ROW_DENSE):
            exp = np.isin(arr.astype(np.int64), members)
            whole = DeviceColumn.from_numpy(arr)
            assert np.array_equal(_probe(whole.slice(0, n), members), exp[:n])
            # an odd Arrow offset: the first row is not 16-byte aligned
            assert np.array_equal(_probe(whole.slice(1, n), members), exp[1:])
            assert np.array_equal(_probe(whole.slice(1, n), members, invert=True), ~exp[1:])
    # with validity: an odd offset, and a bitmap whose first bit is not the first bit of a byte
    arr = rng.integers(0, 200, n + 11).astype(np.int64)
    null = rng.random(n + 11) < 0.25
    a = pa.array(arr, mask=null)
    exp = np.isin(arr, _ROW_MEMBERS) & ~null
    for off in (1, 3, 8):
        col = DeviceColumn.from_arrow(a.slice(off, n))
        assert col.length == n and (col.offset == off % 8 or not null[off:off + n].any())
        assert np.array_equal(_probe(col, _ROW_MEMBERS), exp[off:off + n])
        assert np.array_equal(_probe(col, _ROW_MEMBERS, invert=True), ~exp[off:off + n])
    col = DeviceColumn.from_arrow(a).slice(5, n)
    assert col.offset == 5 and np.array_equal(_probe(col, _ROW_MEMBERS), exp[5:5 + n])


def test_empty_batch():
    from vinum_amd import ops
    from vinum_amd.core import FilterOperator
    from vinum_amd.core.base import DeviceRecordBatch
    from vinum_amd.device import DeviceColumn
    col = DeviceColumn.from_numpy(np.zeros(0, np.int64))
    assert ops.in_set_probe(col, list(range(40))).length == 0
    batch = DeviceRecordBatch.from_arrow(pa.RecordBatch.from_arrays([pa.array([], pa.int64()), pa.array([], pa.string())], names=["a", "s"]), {})
    assert FilterOperator(("in", "a", tuple(range(40))), None)._kernel(batch).num_rows == 0


# ---- 5. set sizes and routes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4095, 4096, 4097, 5000])
def test_set_sizes(n):
    rng = np.random.default_rng(n)
    members = [int(x) for x in (np.arange(n, dtype=np.int64) * 1000 + rng.integers(0, 900, n))]
    rng.shuffle(members)
    ms = sorted(members)
    probes = np.array(ms + [m + 1 for m in ms] + [m - 1 for m in ms] + [ms[0] - 1000, ms[-1] + 1000], np.int64)
    arr = np.concatenate([probes, rng.integers(-5000, n * 1000 + 5000, 3 * TILE)])
    rng.shuffle(arr)
    want = "in_set:bitmap_lds" if n == 1 else "in_set:sorted_lds" if n <= 4096 else "in_set:sorted_global"
    exp = _check_int(arr, members, want)
    assert exp.sum() >= n
    assert f"n={n} " in _route()
    # the same members as floats over a float64 column: always a sorted table
    f = arr.astype(np.float64) / 2
    got = _probe(_dev(f), [m / 2 for m in members])
    assert _route().startswith(("in_set:sorted_lds:" if n <= 4096 else "in_set:sorted_global:")) and "domain=f64" in _route()
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("step,count,route", [(2, 100_000, "in_set:bitmap_lds"), (3, 333_334, "in_set:bitmap_global")])
def test_dense_lists_are_bitmaps(step, count, route):
    members = list(range(-7, -7 + step * count, step))
    rng = np.random.default_rng(step)
    arr = np.concatenate([rng.integers(-50, step * count + 50, 3 * TILE + 77), np.array([-8, -7, -6, members[-1], members[-1] + 1, I64_MIN, I64_MAX])])

    def expected(x):
        x = x.astype(object)                                       # Python ints: no wrap at the int64 extremes
        return np.array([(v + 7) % step == 0 and -7 <= v <= members[-1] for v in x], bool)
    exp = expected(arr)
    got = _probe(_dev(arr), members)
    assert _route().startswith(route + ":"), _route()
    assert np.array_equal(got, exp)
    u = (arr[arr >= 0]).astype(np.uint64)
    got = _probe(_dev(u), members)
    assert _route().startswith(route + ":") and "domain=u64" in _route()
    assert np.array_equal(got, exp[arr >= 0])
    narrow = arr.astype(np.int32)
    assert np.array_equal(_probe(_dev(narrow), members), expected(narrow))


# ---- 6. chain and set agree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_chain_and_set_agree(seed, monkeypatch):
    from vinum_amd import ops
    from vinum_amd.device import DeviceColumn
    rng = np.random.default_rng(1000 + seed)
    names = list(INT_TYPES) + ["float32", "float64"]
    name = names[seed % len(names)]
    n = int(rng.choice([1, 3, 1023, 1025, 4099, int(rng.integers(1, 4099))]))
    if name in INT_TYPES:
        info = np.iinfo(INT_TYPES[name])
        arr = rng.integers(max(info.min, -40), min(info.max, 40), n, dtype=INT_TYPES[name], endpoint=True)
        arr[rng.random(n) < 0.05] = info.max
    else:
        arr = (rng.integers(-40, 40, n) / 4).astype(name)
        arr[rng.random(n) < 0.1] = np.nan
        arr[rng.random(n) < 0.05] = -0.0
    mask = rng.random(n) < 0.3 if seed % 3 == 0 else None
    col = DeviceColumn.from_arrow(pa.array(arr, mask=mask))
    k = int(rng.integers(2, 17))
    pool = [int(x) for x in rng.integers(-45, 45, k)] + [300, -1, 2**40, I64_MAX, I64_MIN]
    if seed % 2:
        pool += [0.25, -0.0, float("nan"), 2.5, float("inf")]
    members = tuple(pool[i] for i in rng.choice(len(pool), k, replace=False))
    for op in ("in", "not_in"):
        expr = ("or", (op, "x", members), ("gt", "x", 35))
        monkeypatch.setenv("VNM_IN_SET_MIN", "17")                    # every list here compiles: the chain, as on the parent commit
        chain = ops.project(expr, {"x": col}).to_numpy()
        monkeypatch.setenv("VNM_IN_SET_MIN", "2")
        ops.in_set_probe(col, members)
        assert _route().startswith("in_set:")
        as_set = ops.project(expr, {"x": col}).to_numpy()
        assert np.array_equal(chain, as_set), (name, members, np.flatnonzero(chain != as_set)[:5])


# ---- 7. strings -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [pa.string(), pa.large_string(), pa.binary()], ids=str)
def test_string_columns_and_a_growing_dictionary(t):
    from vinum_amd.core import FilterOperator
    from vinum_amd.core.base import DeviceRecordBatch
    enc = (lambda s: s.encode()) if t == pa.binary() else (lambda s: s)
    members = tuple(enc(f"v{i}") for i in range(0, 120, 3))                       # 40 members
    first = [enc(f"v{i % 30}") for i in range(2000)] + [None, enc("")]            # v30.. are absent from the dictionary so far
    second = [enc(f"v{i % 130}") for i in range(2000)] + [None]                   # ... and arrive with the second batch
    dicts = {}
    for op in ("in", "not_in"):
        f = FilterOperator((op, "s", members), None)
        for vals in (first, second):
            batch = DeviceRecordBatch.from_arrow(pa.RecordBatch.from_arrays(
                [pa.array(np.arange(len(vals), dtype=np.int64)), pa.array(vals, t)], names=["k", "s"]), dicts)
            got = f._kernel(batch).to_arrow().column("k").to_pylist()
            inside = [v is not None and v in members for v in vals]
            assert got == [k for k, m in enumerate(inside) if m == (op == "in")]    # (a NULL row: NOT IN keeps it)
    absent = tuple(enc(f"nowhere{i}") for i in range(40))
    batch = DeviceRecordBatch.from_arrow(pa.RecordBatch.from_arrays([pa.array(np.arange(len(first), dtype=np.int64)), pa.array(first, t)],
                                                                     names=["k", "s"]), dicts)
    assert FilterOperator(("in", "s", absent), None)._kernel(batch).num_rows == 0
    assert FilterOperator(("not_in", "s", absent), None)._kernel(batch).num_rows == len(first)


# ---- 8. expression operands ------------------------------------------------------------------------------------------------------
def test_expression_operand():
    from vinum_amd import ops
    rng = np.random.default_rng(8)
    a, b = rng.integers(-100, 100, 4099).astype(np.int32), rng.integers(-100, 100, 4099).astype(np.int64)
    h = rng.integers(0, 100, 4099).astype(np.int8)
    cols = {"a": _dev(a), "b": _dev(b), "h": _dev(h)}
    members = tuple(range(-150, 150, 4))
    got = ops.project(("in", ("add", "a", "b"), members), cols, length=4099).to_numpy()
    assert np.array_equal(got.astype(bool), np.isin(a + b, members))
    got = ops.project(("to_int", ("not_in", ("div", "a", 2), tuple(m / 2 for m in members))), cols, length=4099).to_numpy()
    assert np.array_equal(got, np.isin(a / 2, [m / 2 for m in members], invert=True).astype(np.int64))
    mask = ops.predicate_mask(("and", ("in", ("mul", "a", 2), members), ("not_in", "b", members)), cols, 4099)
    assert np.array_equal(mask.to_host(np.uint8, 4099).astype(bool), np.isin(a * 2, members) & ~np.isin(b, members))
    with pytest.raises(TypeError, match="float16"):
        ops.project(("in", ("sqrt", "h"), tuple(range(17))), cols, length=4099)
    with pytest.raises(TypeError, match="predicate"):
        ops.project(("in", ("gt", "a", 1), tuple(range(17))), cols, length=4099)


# ---- 9. the reference's own results -----------------------------------------------------------------------------------------------
def _canon(t: pa.Table) -> pa.Table:
    cols = {}
    for name in t.schema.names:
        c = t.column(name)
        cols[name] = c.cast(pa.uint8()) if pa.types.is_boolean(c.type) else c       # (a predicate in SELECT: the uint8 mask here)
    t = pa.table(cols)
    return t.sort_by([("k", "ascending")]) if "k" in t.schema.names else t


def test_fixture_list_is_complete():
    with open(os.path.join(util.GOLDEN, "in_set_cases.json")) as f:
        meta = json.load(f)
    assert sorted(meta["cases"]) == sorted(c["name"] for c in C.CASES)
    stored, made = util.read_ipc("in_set_in.arrow"), C.in_set_table()
    assert stored.schema == made.schema
    assert str(stored.to_pydict()) == str(made.to_pydict())         # (str: the NaN rows compare equal)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["name"])
def test_reference_fixtures_through_the_planner(case):
    from vinum_amd import planner, set_batch_size
    set_batch_size(150)
    try:
        got = planner.execute(case, util.read_ipc("in_set_in.arrow"))
    finally:
        set_batch_size(1 << 24)
    exp = util.read_ipc(f"in_set_{case['name']}.arrow")
    assert got.schema.names == exp.schema.names
    got, exp = _canon(got), _canon(exp)
    assert got.num_rows == exp.num_rows
    for name in exp.schema.names:
        g, e = got.column(name).to_pylist(), exp.column(name).to_pylist()
        assert str(g) == str(e), (case["name"], name, [(a, b) for a, b in zip(g, e) if str(a) != str(b)][:5])    # (str: nan == nan)


# ---- 10. under the pool's guard mode ----------------------------------------------------------------------------------------------
def test_under_the_pool_guard():
    from vinum_amd import _lib as L
    from vinum_amd import ops
    lib = L.lib()
    lib.vnm_device_synchronize()
    ops.in_set_cache_clear()                     # every table is allocated (red-zoned, poisoned) inside this leg
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        test_set_sizes(3)
        test_set_sizes(4096)
        test_set_sizes(4097)
        test_dense_lists_are_bitmaps(2, 100_000, "in_set:bitmap_lds")
        test_dense_lists_are_bitmaps(3, 333_334, "in_set:bitmap_global")
        test_row_counts(1)
        test_row_counts(TILE + 1)
        test_integer_columns_with_nulls_compare_as_float64("uint64")
        test_operators_with_lists_the_interpreter_cannot_hold("s", 100)
        test_expression_operand()
        ops.in_set_cache_clear()                 # the tables go back to the pool: their zones are checked
        lib.vnm_device_synchronize()
        v, c = ctypes.c_int64(0), ctypes.c_int64(0)
        need = lib.vnm_pool_guard_report(None, 0, ctypes.byref(v), ctypes.byref(c))
        buf = ctypes.create_string_buffer(int(need) + 65536)
        lib.vnm_pool_guard_report(buf, len(buf), ctypes.byref(v), ctypes.byref(c))
        assert v.value == 0, buf.value.decode()
        assert c.value > 0
    finally:
        lib.vnm_pool_set_guard(0)
        lib.vnm_pool_guard_reset()
