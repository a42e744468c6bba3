"""32-bit entry words out of BOTH scatter levels of the dense group-by (route dense:fixed_point_narrow_levels): the
first level's words carry the value in a window of 32 - (remainder bits) bits above a base taken from the value sample.  Against the
oracle: the two geometries (2^24 codes: 64 rings; 2^27 codes: the first fan-out raised to 512 rings, the headline's plan), windows
at zero and with a negative base, values that must keep 8-byte words out of the first level, a row outside the window (one misfit
note, the first level alone goes back), the spill paths over biased words, and every pass-1 variant that takes the path.

The geometry follows the key RANGE: a few million rows reach it.  (The 2^27-code cases tell the operator how many groups to expect and
allow more codes per row than a batch of this size gets by default -- the full-size test runs that plan unaided.)"""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

from tests import util
from tests.test_gpu_agg import gpu_aggregate

pytestmark = pytest.mark.gpu

NARROW = "dense:fixed_point_narrow_levels"
LAST_ONLY = "dense:fixed_point_narrow_last_level"      # 32-bit words out of the last level, 8-byte words out of the first
RANGES = [12_000_000, 100_000_000]     # 24 code bits: p1 = 6, a window of 14 bits; 27 bits: p1 8 -> 9, 14 bits


def _routes():
    from vinum_amd import _lib as L
    lib = L.lib()
    need = lib.vnm_route_counts(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    lib.vnm_route_counts(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        k, _, v = line.rpartition("=")
        out[k] = int(v)
    return out


def _took(before, name):
    return _routes().get(name, 0) - before.get(name, 0)


def _funcs():
    from oracle import oracle as O
    return [(O.SUM, "v", "s"), (O.AVG, "v", "a"), (O.COUNT_STAR, "", "n")]


def _oracle(batches, pred=None):
    from oracle import oracle as O
    o = O.OracleAggregate(O.SINGLE, ["k"], ["k"], _funcs())
    for b in batches:
        if pred is not None:
            b = O.filter_batch(b, O.cmp_mask(b.column(b.schema.names.index(pred[0])), O.GT, pred[2]))
        o.next(b)
    return o.result()


def _setup(monkeypatch, key_range):
    monkeypatch.setenv("VNM_AGG_ESTIMATE_MIN_ROWS", "100000")
    if key_range > 20_000_000:      # (1.2e6-row batches over 1e8 codes)
        monkeypatch.setenv("VNM_DENSE_SPAN_PER_ROW", "128")
        return 6_000_000              # (the code range, 2^27, may be 32 times the expected groups)
    return 0


def _values(rng, n, values):
    if values == "k/128":
        return rng.integers(0, 2**14, n).astype(np.float64) / 128.0
    if values == "k/128_16bits":
        return rng.integers(0, 2**16, n).astype(np.float64) / 128.0
    if values == "halves_negative":
        return -rng.integers(0, 5000, n).astype(np.float64) / 2.0 + 100.0
    if values == "integers":
        return rng.integers(-10**6, 10**6, n).astype(np.float64)
    return np.zeros(n)


def _unsampled(at, batch_rows):
    # (the value sample reads rows i * rows / 65536 of the first batch)
    sampled = set(((np.arange(65536, dtype=np.int64) * batch_rows) // 65536).tolist())
    while at in sampled:
        at += 1
    return at


@pytest.mark.parametrize("key_range", RANGES)
@pytest.mark.parametrize("values,pred", [("k/128", False), ("k/128", True), ("halves_negative", False), ("zeros", False)])
def test_narrow_first_level_vs_oracle(key_range, values, pred, monkeypatch):
    """Values whose sampled span fits the window: the aligned window [0, 2^14) (k / 128, zeros), a window with a negative base
    (100 - j / 2: every decode adds the base back and must treat the field as unsigned).  Two batches; equal to the oracle."""
    from oracle import oracle as O
    hint = _setup(monkeypatch, key_range)
    rng = np.random.default_rng(key_range % 1009 + len(values) + int(pred))
    n = 2_400_000
    k = rng.integers(0, key_range, n).astype(np.int64) - 17
    t = pa.table({"k": pa.array(k), "v": pa.array(_values(rng, n, values))})
    batches = util.sliced_batches(t, n // 2)
    predicate = ("v", ">", 1.0) if pred else None
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches, predicate=predicate, expected_groups=hint)
    assert _took(before, NARROW) >= 1, _routes()
    assert _took(before, "dense:fixed_point_misfit") == 0
    util.assert_agg_equal(got, _oracle(batches, predicate), _funcs(), ["k"], what=f"narrow first level {values} range={key_range} pred={pred}")


@pytest.mark.parametrize("values", ["k/128_16bits", "integers"])
def test_wide_span_keeps_8_byte_words_out_of_the_first_level(values, monkeypatch):
    """2^27 codes leave the first level 14 bits: a span of 16 bits of quanta keeps its 8-byte words there and the 32-bit words out of
    the last level; integers up to 1e6 keep 8-byte words throughout."""
    from oracle import oracle as O
    hint = _setup(monkeypatch, RANGES[1])
    rng = np.random.default_rng(len(values))
    n = 2_400_000
    k = rng.integers(0, RANGES[1], n).astype(np.int64)
    t = pa.table({"k": pa.array(k), "v": pa.array(_values(rng, n, values))})
    batches = util.sliced_batches(t, n // 2)
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches, expected_groups=hint)
    assert _took(before, NARROW) == 0 and _took(before, "dense:fixed_point") == 2 and _took(before, "dense:fixed_point_misfit") == 0, _routes()
    assert _took(before, LAST_ONLY) == (2 if values == "k/128_16bits" else 0), _routes()      # (both batches; integers: 8-byte words throughout)
    util.assert_agg_equal(got, _oracle(batches), _funcs(), ["k"], what=f"wide span {values}")


@pytest.mark.parametrize("key_range", RANGES)
def test_knob_keeps_the_last_level_only(key_range, monkeypatch):
    """VNM_DENSE_FX_NARROW=2: values that would take the window keep 8-byte words out of the first level and 32-bit words out of the last."""
    from oracle import oracle as O
    hint = _setup(monkeypatch, key_range)
    monkeypatch.setenv("VNM_DENSE_FX_NARROW", "2")
    rng = np.random.default_rng(key_range % 1013)
    n = 2_400_000
    k = rng.integers(0, key_range, n).astype(np.int64)
    t = pa.table({"k": pa.array(k), "v": pa.array(_values(rng, n, "k/128"))})
    batches = util.sliced_batches(t, n // 2)
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches, expected_groups=hint)
    assert _took(before, NARROW) == 0 and _took(before, LAST_ONLY) == 2 and _took(before, "dense:fixed_point_misfit") == 0, _routes()
    util.assert_agg_equal(got, _oracle(batches), _funcs(), ["k"], what=f"last level only, range={key_range}")


@pytest.mark.parametrize("where", ["first_batch_late_row", "second_batch"])
def test_value_outside_the_window_costs_the_first_level_only(where, monkeypatch):
    """ONE value of 300.0 among k / 128 below 128: inside the 18 bits of the last level's words (quantum 2^-9), outside the first
    level's window.  Exactly one misfit note, the batch is redone with 8-byte words out of the first level, and a later batch of the
    same operator does not try the window again.  Equal to the oracle."""
    from oracle import oracle as O
    _setup(monkeypatch, RANGES[0])
    rng = np.random.default_rng(len(where))
    n = 2_400_000
    half = n // 2
    k = rng.integers(0, RANGES[0], n).astype(np.int64)
    v = _values(rng, n, "k/128")
    at = _unsampled(half - 12345, half) if where == "first_batch_late_row" else n - 777
    v[at] = 300.0
    t = pa.table({"k": pa.array(k), "v": pa.array(v)})
    batches = util.sliced_batches(t, half)
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches)
    assert _took(before, "dense:fixed_point_misfit") == 1, _routes()
    # (the first batch took the window only where the value came later; no batch takes it after the misfit)
    assert _took(before, NARROW) == (0 if where == "first_batch_late_row" else 1), _routes()
    util.assert_agg_equal(got, _oracle(batches), _funcs(), ["k"], what=f"window misfit {where}", source=batches)


def test_spill_paths_decode_biased_words(monkeypatch):
    """Keys floor(G u^4): heavy keys fill their rings (the round limit spills what stays pending) and their regions (whole blocks of
    ring words go to the spill buffer, partial ones when the kernel drains) -- over words with a negative base."""
    from oracle import oracle as O
    _setup(monkeypatch, RANGES[0])
    rng = np.random.default_rng(4)
    n = 3_000_000
    k = np.floor(RANGES[0] * rng.random(n) ** 4).astype(np.int64)
    k[rng.random(n) < 0.3] = 123456        # (at this size only a key this heavy fills pass 1's regions as well)
    t = pa.table({"k": pa.array(k), "v": pa.array(_values(rng, n, "halves_negative"))})
    batches = util.sliced_batches(t, n // 2)
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches)
    assert _took(before, NARROW) >= 1, _routes()
    assert _took(before, "scan:spilled_entries") >= 1 and _took(before, "dense:fixed_point_misfit") == 0, _routes()
    util.assert_agg_equal(got, _oracle(batches), _funcs(), ["k"], what="skewed keys over biased words", source=batches)


@pytest.mark.parametrize("what", ["null_keys", "null_values", "pred_on_other"])
def test_pass1_variants_take_the_narrow_first_level(what, monkeypatch):
    """The pass-1 kernels over a nullable key (12 % NULL), over a nullable value the query's own filter reads (1 % NULL) and with a
    predicate column of its own, at 2^24 codes with a negative base."""
    from oracle import oracle as O
    _setup(monkeypatch, RANGES[0])
    rng = np.random.default_rng(len(what))
    n = 2_400_000
    k = rng.integers(0, RANGES[0], n).astype(np.int64)
    v = _values(rng, n, "halves_negative")
    cols = {"k": pa.array(k, mask=(rng.random(n) < 0.12) if what == "null_keys" else None),
            "v": pa.array(v, mask=(rng.random(n) < 0.01) if what == "null_values" else None)}
    predicate = ("v", ">", -1000.0)
    if what == "pred_on_other":
        cols["p"] = pa.array(rng.integers(0, 2**14, n).astype(np.float64) / 128.0)
        predicate = ("p", ">", 64.0)
    batches = pa.table(cols).combine_chunks().to_batches()
    before = _routes()
    got = gpu_aggregate(O.SINGLE, ["k"], ["k"], _funcs(), batches, predicate=predicate)
    assert _took(before, NARROW) >= 1 and _took(before, "dense:fixed_point_misfit") == 0, _routes()
    util.assert_agg_equal(got, _oracle(batches, predicate), _funcs(), ["k"], what=f"narrow first level + {what}")


def test_stream_segments_take_the_narrow_first_level(monkeypatch):
    """The record batches of a stream as the segments of one pass-1 launch; a ragged last batch; predicate on the value column."""
    from oracle import oracle as O
    from vinum_amd.device import DeviceColumn
    from vinum_amd import ops
    _setup(monkeypatch, RANGES[0])
    rng = np.random.default_rng(21)
    n = 3_300_001
    k = rng.integers(0, RANGES[0], n).astype(np.int64)
    t = pa.table({"k": pa.array(k), "v": pa.array(_values(rng, n, "halves_negative"))})
    batches = util.sliced_batches(t, 1 << 20)
    funcs = _funcs()
    fspec = [(f, 1 if col else None, pa.float64() if col else None) for f, col, _ in funcs]
    before = _routes()
    agg = ops.DeviceAggregate(O.SINGLE, [pa.int64()], fspec, stream_mode=True)
    agg.set_predicate(">", -1000.0)
    keep = []
    for b in batches:
        kc, vc = DeviceColumn.from_arrow(b.column(0)), DeviceColumn.from_arrow(b.column(1))
        keep.append((kc, vc))
        agg.next([kc], [vc, vc, None], pred=vc, nrows=b.num_rows)
    res = agg.result_arrays([0], ["k"], [f[2] for f in funcs])
    agg.close()
    assert _took(before, NARROW) >= 1 and _took(before, "dense:stream_segments") >= 1, _routes()
    util.assert_agg_equal(res, _oracle(batches, ("v", ">", -1000.0)), funcs, ["k"], what="narrow first level, stream segments")
