"""Built-in scalar functions on the GPU (vnm_project's MATH instantiations) against NumPy 2.x.

Exact functions (abs, sqrt, the casts, integer power, float16 sqrt) must match NumPy bit for bit; NaNs compare as a class
(the sign and payload of a NaN an invalid operation creates is the x86 default NaN on the host and the canonical NaN on
the GPU -- neither is a value).  The transcendentals are checked against a correctly rounded reference (math.* in float64,
rounded to the result type) within the OCML error bounds: float64 sin / cos / log / log2 / log10 <= 2 ULP, tan / pow
<= 3 ULP; float32 <= 2 / <= 4 ULP; float16 <= 1 ULP.  Budget: a few seconds in total."""
import ctypes
import math

import numpy as np
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from vinum_amd import _lib as L  # noqa: E402
from vinum_amd import ops  # noqa: E402
from vinum_amd import planner as P  # noqa: E402
from vinum_amd.device import DeviceColumn  # noqa: E402

N = 4099
RNG = np.random.default_rng(7)


def _ints(dt):
    info = np.iinfo(dt)
    v = RNG.integers(info.min, info.max, N, dtype=dt, endpoint=True)
    v[:6] = np.array([0, 1, info.max, info.min, 2, 3], dtype=dt) if info.min < 0 else np.array([0, 1, info.max, 4, 2, 3], dtype=dt)
    return v


def _floats(dt):
    v = (RNG.standard_normal(N) * 10.0 ** RNG.integers(-3, 4, N)).astype(dt)
    big = [1e300, -1e300, 1.5e19, -9.3e18, 9.223372036854775808e18, 1e22] if dt == np.float64 else [3e38, -3e38, 1e19, -1e19]
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 1e-310 if dt == np.float64 else 1e-40, 1.0, 0.5] + big, dtype=dt)
    v[:len(sp)] = sp
    return v


COLS = {
    "i8": _ints(np.int8), "u8": _ints(np.uint8), "i16": _ints(np.int16), "u16": _ints(np.uint16),
    "i32": _ints(np.int32), "u32": _ints(np.uint32), "i64": _ints(np.int64), "u64": _ints(np.uint64),
    "f32": _floats(np.float32), "f64": _floats(np.float64),
}
NULLMASK = RNG.random(N) < 0.2


@pytest.fixture(scope="module")
def dev():
    d = {k: DeviceColumn.from_numpy(v) for k, v in COLS.items()}
    d["ni"] = DeviceColumn.from_arrow(pa.array(COLS["i32"], mask=NULLMASK))
    return d


def _run(exprs, dev):
    cols = {c: dev[c] for e in exprs for c in ops.columns_of(e)}
    outs = ops.project_many(exprs, cols, length=N)
    return [o.to_numpy() for o in outs]


def _same_bits(got, want):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    if want.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), np.flatnonzero(gn != wn)[:5]
        g, w = got[~gn], want[~wn]
        bad = g.view(f"u{g.dtype.itemsize}") != w.view(f"u{w.dtype.itemsize}")
        assert not bad.any(), (g[bad][:5], w[bad][:5])
    else:
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


def _ulps(got, ref, dt):
    """distance in units of the last place of `dt`, reference correctly rounded from float64"""
    g = got.astype(np.float64)
    r = ref.astype(np.float64)
    spacing = np.abs(np.spacing(r.astype(dt))).astype(np.float64)
    return np.abs(g - r) / spacing


def _np_fn(name):
    return {"abs": np.absolute, "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "tan": np.tan, "log": np.log,
            "log2": np.log2, "log10": np.log10}[name]


@pytest.mark.parametrize("col", list(COLS))
def test_exact_functions_bit_for_bit(dev, col):
    x = COLS[col]
    exprs = [("abs", col), ("sqrt", col), ("to_int", col), ("to_float", col), ("to_bool", col)]
    got = _run(exprs, dev)
    with np.errstate(all="ignore"):
        want = [np.absolute(x), np.sqrt(x), np.array(x, dtype="int"), np.array(x, dtype="float"), np.array(x, dtype="bool")]
    for g, w, e in zip(got, want, exprs):
        if w.dtype == np.bool_:
            assert np.array_equal(g.astype(bool), w), e
        else:
            _same_bits(g, w)


BOUND = {np.dtype(np.float64): {"tan": 3, "power": 3, None: 2}, np.dtype(np.float32): {"tan": 4, "power": 4, None: 2},
         np.dtype(np.float16): {"tan": 1, "power": 1, None: 1}}


@pytest.mark.parametrize("col", ["i8", "u8", "i16", "u16", "i32", "u64", "f32", "f64"])
@pytest.mark.parametrize("fn", ["sin", "cos", "tan", "log", "log2", "log10"])
def test_transcendentals_within_ulp_bound(dev, col, fn):
    x = COLS[col]
    (got,) = _run([(fn, col)], dev)
    with np.errstate(all="ignore"):
        want = _np_fn(fn)(x)
        assert got.dtype == want.dtype
        mf = {"sin": math.sin, "cos": math.cos, "tan": math.tan, "log": math.log, "log2": math.log2, "log10": math.log10}[fn]

        def ref1(v):
            try:
                return mf(v)
            except ValueError:
                return math.nan
        xs = x.astype(np.float64)
        if want.dtype == np.float16:
            xs = xs.astype(np.float16).astype(np.float64)
        ref = np.array([ref1(v) if np.isfinite(v) and (fn in ("sin", "cos", "tan") or v > 0) else float(want[i].astype(np.float64))
                        for i, v in enumerate(xs)])
    # special values: NaN / inf / +-0 exactly as NumPy (class and sign)
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(np.isnan(got[special]), np.isnan(want[special])), (fn, col)
    fin = special & ~np.isnan(want)
    assert np.array_equal(got[fin], want[fin]) and np.array_equal(np.signbit(got[fin]), np.signbit(want[fin])), (fn, col)
    ok = ~special & np.isfinite(ref)
    u = _ulps(got[ok], ref[ok], want.dtype)
    bound = BOUND[want.dtype].get(fn, BOUND[want.dtype][None])
    assert u.max(initial=0) <= bound, (fn, col, u.max(), x[ok][np.argmax(u)])


@pytest.mark.parametrize("col", ["i8", "u8", "i16", "i32", "i64", "u32", "u64"])
def test_integer_power_bit_for_bit(dev, col):
    x = COLS[col]
    e = np.abs(COLS["i8"]).astype(np.int64) % 70
    if col == "u64":
        e = e.astype(np.uint64)      # uint64 ** int64 promotes to float64 (a float power, not this test's subject)
    dev_e = DeviceColumn.from_numpy(e)
    got = ops.project_many([("power", col, 3), ("power", col, "e"), ("power", col, 0)], {col: dev[col], "e": dev_e}, length=N)
    with np.errstate(all="ignore"):
        want = [np.power(x, 3), np.power(x, e), np.power(x, 0)]
    for g, w in zip(got, want):
        _same_bits(g.to_numpy(), w)


def test_float_power_and_float16_arithmetic(dev):
    x8, f64, f32 = COLS["u8"], COLS["f64"], COLS["f32"]
    exprs = [("power", "f64", 2.5), ("power", "f32", 2), ("sqrt", "u8"), ("add", ("sqrt", "u8"), 1.5),
             ("mul", ("sqrt", "i8"), ("sqrt", "u8")), ("power", ("sqrt", "u8"), 2)]
    got = _run(exprs, dev)
    with np.errstate(all="ignore"):
        want = [np.power(f64, 2.5), np.power(f32, 2), np.sqrt(x8), np.sqrt(x8) + 1.5,
                np.sqrt(COLS["i8"]) * np.sqrt(x8), np.power(np.sqrt(x8), 2)]
    for (g, w, e) in zip(got, want, exprs):
        assert g.dtype == w.dtype, e
    _same_bits(got[2], want[2])            # float16 sqrt: exact
    _same_bits(got[3], want[3])
    _same_bits(got[4], want[4])
    for k in (0, 1, 5):
        g, w = got[k], want[k]
        fin = np.isfinite(w) & np.isfinite(g)
        assert np.array_equal(np.isnan(g), np.isnan(w)), exprs[k]
        ref = np.power(np.float64(1) * (f64 if k == 0 else f32 if k == 1 else np.sqrt(x8).astype(np.float64)),
                       2.5 if k == 0 else 2.0)
        u = _ulps(g[fin], ref[fin], w.dtype)
        assert u.max(initial=0) <= BOUND[w.dtype]["power"], (exprs[k], u.max())


def test_nulls_enter_as_nan(dev):
    (got, gi) = _run([("sqrt", "ni"), ("to_int", "ni")], dev)
    x = np.where(NULLMASK, np.nan, COLS["i32"].astype(np.float64))
    with np.errstate(all="ignore"):
        _same_bits(got, np.sqrt(x))
        _same_bits(gi, np.array(x, dtype="int"))


def test_negative_exponent_column_raises_and_leaves_no_fault(dev):
    e = np.arange(N, dtype=np.int64) - 5
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.project_many([("power", "i64", "e")], {"i64": dev["i64"], "e": DeviceColumn.from_numpy(e)}, length=N)
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.project_many([("power", "i32", -1)], {"i32": dev["i32"]}, length=N)
    (g,) = _run([("abs", "i64")], dev)        # the device is fine afterwards
    _same_bits(g, np.absolute(COLS["i64"]))


def test_where_log10_matches_numpy_mask():
    v = np.abs(RNG.standard_normal(20000)) * 1000
    t = pa.table({"v": v})
    got = P.execute({"select": ["v"], "where": ("gt", ("fn", "log10", "v"), 1.5)}, t).column(0).to_numpy()
    lv = np.log10(v)
    # rows within 2 ULP of the threshold may fall either way with a different (equally accurate) log10: excluded
    near = np.abs(lv - 1.5) <= 4 * np.spacing(1.5)
    want_strict = v[(lv > 1.5) & ~near]
    assert set(want_strict).issubset(set(got))
    assert set(got).issubset(set(v[(lv > 1.5) | near]))


def test_aggregates_over_functions_equal_project_then_aggregate():
    k = RNG.integers(0, 50, 30000)
    v = np.abs(RNG.standard_normal(30000)) * 100
    a, b = RNG.standard_normal(30000), RNG.standard_normal(30000)
    t = pa.table({"k": k, "v": v, "a": a, "b": b})
    q = {"select": ["k", ("fn", "sum", ("fn", "sqrt", "v")), ("fn", "avg", ("fn", "abs", ("sub", "a", "b"))),
                    ("fn", "sum", ("fn", "sin", "v"))], "aliases": [None, "s", "d", "n"], "group_by": ["k"],
         "order_by": ["k"], "sort_order": ["ASC"]}
    got = P.execute(q, t)
    pre = ops.project_many([("sqrt", "v"), ("abs", ("sub", "a", "b")), ("sin", "v")],
                           {c: DeviceColumn.from_numpy(t.column(c).to_numpy()) for c in ("v", "a", "b")}, length=30000)
    t2 = pa.table({"k": k, "sv": pre[0].to_numpy(), "ad": pre[1].to_numpy(), "sn": pre[2].to_numpy()})
    q2 = {"select": ["k", ("fn", "sum", "sv"), ("fn", "avg", "ad"), ("fn", "sum", "sn")], "aliases": [None, "s", "d", "n"],
          "group_by": ["k"], "order_by": ["k"], "sort_order": ["ASC"]}
    want = P.execute(q2, t2)
    for c in ("s", "d", "n"):
        assert np.array_equal(got.column(c).to_numpy(), want.column(c).to_numpy()), c


def test_issue_queries_through_the_planner():
    n = 5000
    t = pa.table({"fare": np.abs(RNG.standard_normal(n)) * 50, "total": RNG.standard_normal(n) * 30,
                  "tip": RNG.standard_normal(n), "lat": RNG.standard_normal(n) * 40,
                  "city_from": RNG.integers(0, 7, n), "tax": RNG.standard_normal(n)})
    got = P.execute({"select": [("fn", "sqrt", "fare"), ("fn", "abs", ("sub", "total", "tip")), ("fn", "to_int", "total")],
                     "where": ("gt", ("fn", "log10", "fare"), 1)}, t)
    fare, total, tip = (t.column(c).to_numpy() for c in ("fare", "total", "tip"))
    m = np.log10(fare) > 1
    assert got.schema.names == ["sqrt", "abs", "to_int"]
    _same_bits(got.column(0).to_numpy(), np.sqrt(fare[m]))
    _same_bits(got.column(1).to_numpy(), np.absolute(total[m] - tip[m]))
    _same_bits(got.column(2).to_numpy(), np.array(total[m], dtype="int"))
    grp = ("mod", ("fn", "to_int", ("mul", ("fn", "np.sin", "lat"), 100000)), 11)
    got = P.execute({"select": ["city_from", grp, ("fn", "count_star"), ("fn", "min", "tax")],
                     "aliases": [None, "grp_exp", None, None], "group_by": ["city_from", grp],
                     "order_by": ["city_from", grp], "sort_order": ["ASC", "ASC"]}, t)
    lat, city, tax = t.column("lat").to_numpy(), t.column("city_from").to_numpy(), t.column("tax").to_numpy()
    g = np.array(np.sin(lat) * 100000, dtype="int") % 11
    keys = sorted(set(zip(city.tolist(), g.tolist())))
    assert list(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == keys
    cnt = [int(((city == c) & (g == x)).sum()) for c, x in keys]
    assert got.column(2).to_pylist() == cnt
    assert got.column(3).to_pylist() == [float(tax[(city == c) & (g == x)].min()) for c, x in keys]


# ---- every kernel instantiation by name, the programs beyond 64 KB of LDS, the power flag: one tile and a tail ---------------------
PN = 1027            # one full tile of 1024 rows plus a three-row tail: the 16-byte path and the guarded path of push and store
PRNG = np.random.default_rng(17)
PX, PY = PRNG.standard_normal(PN + 1) * 10.0, PRNG.standard_normal(PN + 1) * 3.0
PK = PRNG.integers(-1000, 1000, PN + 1)
PCODES = PRNG.integers(-2, 10, PN + 1).astype(np.int32)           # negative codes and codes past both tables among them
PCODE_NULL = PRNG.random(PN + 1) < 0.2
TABLE_U8 = np.array([1, 0, 2, 0, 255], np.uint8)
TABLE_I32 = np.array([5, -7, 0, 2 ** 31 - 1, -2 ** 31, 11, 3], np.int32)
SPANS = ["project_kernel", "project_kernel_exact_fn", "project_kernel_math", "project_kernel_lookup", "project_kernel_lookup_i32"]


@pytest.fixture(scope="module")
def pdev():
    d = {"x": DeviceColumn.from_numpy(PX), "y": DeviceColumn.from_numpy(PY), "k": DeviceColumn.from_numpy(PK),
         "c": DeviceColumn.from_arrow(pa.array(PCODES, mask=PCODE_NULL))}
    return d, {"t8": DeviceColumn.from_numpy(TABLE_U8), "t32": DeviceColumn.from_numpy(TABLE_I32)}


def _prun(exprs, pdev, off):
    """the rows [off, off + PN) of the row columns: Arrow offset 1 turns the 16-byte push off"""
    rows, tables = pdev
    names = {c for e in exprs for c in ops.columns_of(e)}
    cols = {c: rows[c].slice(off, PN) if c in rows else tables[c] for c in names}
    return [o.to_numpy() for o in ops.project_many(exprs, cols, length=PN)]


def _span_counts():
    out = {}
    for name in SPANS:
        ms, count = ctypes.c_double(0), ctypes.c_int64(0)
        L.lib().vnm_profile_query(name.encode(), ctypes.byref(ms), ctypes.byref(count))
        out[name] = count.value
    return out


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("lookup", [None, "lookup", "lookup_i32"])
@pytest.mark.parametrize("fn", ["plain", "abs", "sin"])
def test_each_instantiation_runs_under_its_own_name(pdev, fn, lookup, off):
    x, y = PX[off:off + PN], PY[off:off + PN]
    exprs = [{"plain": ("add", "x", "y"), "abs": ("abs", ("sub", "x", "y")), "sin": ("sin", "x")}[fn]]
    if lookup:
        exprs.append((lookup, "c", "t8" if lookup == "lookup" else "t32"))
    name = {"lookup": "project_kernel_lookup", "lookup_i32": "project_kernel_lookup_i32"}.get(
        lookup, {"plain": "project_kernel", "abs": "project_kernel_exact_fn", "sin": "project_kernel_math"}[fn])
    L.lib().vnm_set_profiling(1)
    try:
        before = _span_counts()
        got = _prun(exprs, pdev, off)
        after = _span_counts()
    finally:
        L.lib().vnm_set_profiling(0)
    assert after == {n: before[n] + (1 if n == name else 0) for n in SPANS}
    if fn == "sin":
        assert got[0].dtype == np.float64
        ref = np.array([math.sin(v) for v in x])
        assert _ulps(got[0], ref, np.float64).max() <= BOUND[np.dtype(np.float64)][None]
    else:
        _same_bits(got[0], x + y if fn == "plain" else np.absolute(x - y))
    if lookup:
        codes, null = PCODES[off:off + PN], PCODE_NULL[off:off + PN]
        table = TABLE_U8 if lookup == "lookup" else TABLE_I32
        hit = ~null & (codes >= 0) & (codes < len(table))
        entry = table[np.where(hit, codes, 0)]
        if lookup == "lookup":
            assert got[1].dtype == np.uint8 and np.array_equal(got[1], (hit & (entry != 0)).astype(np.uint8))
        else:
            _same_bits(got[1], np.where(hit, entry.astype(np.float64), np.nan))


def _right_nested(names, innermost=None):
    e = innermost or names[-1]
    for n in reversed(names[:-1]):
        e = ("add", n, e)
    return e


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("depth,with_abs", [(10, False), (9, True), (12, False)])
def test_deep_programs_beyond_64k_of_lds(pdev, depth, with_abs, off):
    """a right-nested sum holds every operand on the stack at once: depth 10 (9 with a built-in, which stages the top through one
    more level) is the first whose LDS passes 64 KB, 12 the deepest a program may be"""
    names = [("x", "y", "k")[i % 3] for i in range(depth)]
    (got,) = _prun([_right_nested(names, ("abs", names[-1]) if with_abs else None)], pdev, off)
    arrays = {"x": PX[off:off + PN], "y": PY[off:off + PN], "k": PK[off:off + PN]}
    want = np.absolute(arrays[names[-1]]) if with_abs else arrays[names[-1]]
    for n in reversed(names[:-1]):
        want = arrays[n] + want
    _same_bits(got, want)


@pytest.mark.parametrize("off", [0, 1])
def test_integer_power_with_an_exponent_column(pdev, off):
    rows, _ = pdev
    base = PK[off:off + PN]
    e = np.abs(PK) % 9
    cols = {"k": rows["k"].slice(off, PN), "e": DeviceColumn.from_numpy(e).slice(off, PN)}
    (got,) = ops.project_many([("power", "k", "e")], cols, length=PN)
    _same_bits(got.to_numpy(), np.power(base, e[off:off + PN]))
    e[off + PN - 2] = -1          # in the tail, past the full tile
    cols["e"] = DeviceColumn.from_numpy(e).slice(off, PN)
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        np.power(base, e[off:off + PN])
    with pytest.raises(ValueError, match="Integers to negative integer powers are not allowed."):
        ops.project_many([("power", "k", "e")], cols, length=PN)
