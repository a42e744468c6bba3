"""KeyDictionary's four cached device tables -- like_table, translate_table, joint_rank_tables, mapped -- over ONE stream of
encodes: after every step each table is read back and compared with the host, entry by entry, and the launch counters say which
tables were extended, rebuilt or left alone.  Every test runs over the poisoned, red-zoned pool (vnm_pool_set_guard(2)): a table
that grows must carry exactly its covered prefix over, a longer copy lands in a red zone.  Public API only."""
import ctypes
import gc

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def pool_guard():
    from vinum_amd import _lib as L
    lib = L.lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(2) == 0
    lib.vnm_pool_guard_reset()
    try:
        yield
        gc.collect()
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


COUNTERS = ("like_launches", "like_ids_matched", "translate_builds", "joint_rank_builds", "map_launches", "map_ids_mapped")


def _counters(kd):
    return {c: getattr(kd, c) for c in COUNTERS}


def _by_id(kd):
    """the dictionary's values by id: None for an id never handed out"""
    return kd.values_by_code().to_pylist()


def _check_entries(what, table, by_id, want, absent):
    """table[id] == want(value) for every id handed out -- all of which the table covers --, `absent` for every other id it covers
    (None: unspecified).  The table and values_by_code() each end at the id count of the encode that last concerned them."""
    for i in range(max(len(table), len(by_id))):
        v = by_id[i] if i < len(by_id) else None
        if v is not None:
            assert i < len(table), f"{what}: id {i} ({v!r}) is beyond the table's {len(table)} entries"
            assert table[i] == want(v), f"{what}: id {i} ({v!r}) holds {table[i]}, not {want(v)}"
        elif absent is not None and i < len(table):
            assert table[i] == absent, f"{what}: id {i} was never handed out and holds {table[i]}"


def _read_and_check(A, B):
    """the four tables of A (and B's half of the joint ranks) against the host; returns them as NumPy arrays"""
    a_ids, b_ids = _by_id(A), _by_id(B)
    like = A.like_table("a%").to_numpy()
    assert len(like) >= len(a_ids)                                # (like_table covers every id after every call)
    _check_entries("like", like, a_ids, lambda v: v.startswith("a"), None)

    translate = A.translate_table(B).to_numpy()
    code_in_b = lambda v: -2 if B.code_of(v) is None else B.code_of(v)
    _check_entries("translate", translate, a_ids, code_in_b, -2)

    union = sorted({v.encode() for v in a_ids + b_ids if v is not None})
    rank = lambda v: union.index(v.encode())
    ja, jb = (t.to_numpy() for t in A.joint_rank_tables(B))
    _check_entries("joint ranks (own)", ja, a_ids, rank, -1)
    _check_entries("joint ranks (other's)", jb, b_ids, rank, -1)

    derived, table = A.mapped("upper")
    mapped = table.to_numpy()
    _check_entries("mapped", mapped, a_ids, lambda v: derived.code_of(pc.utf8_upper(pa.scalar(v)).as_py()), -2)
    return {"like": like, "translate": translate, "joint_a": ja, "joint_b": jb, "mapped": mapped}


def _live_prefix_unchanged(before, after, by_id_before):
    """what a table held for the ids handed out before is what it holds now"""
    live = np.array([i for i, v in enumerate(by_id_before) if v is not None], np.int64)
    for name in ("like", "translate", "mapped"):
        assert (after[name][live] == before[name][live]).all(), name


def test_one_stream_drives_all_four_tables():
    from vinum_amd.vinum_lib import KeyDictionary
    A, B = KeyDictionary(pa.string()), KeyDictionary(pa.string())
    enc = lambda kd, vals: kd.encode(pa.array(vals, pa.string()))
    # tables asked for before any value exists start with room for one entry: the first values take them past twice that
    assert len(A.like_table("B%").to_numpy()) == 0 and len(A.mapped("lower")[1].to_numpy()) == 0

    # 1. the first build
    enc(A, ["apple", "Berlin"])
    enc(B, ["apple"])
    derived = A.mapped("upper")[0]
    t1 = _read_and_check(A, B)
    assert t1["translate"][A.code_of("Berlin")] == -2
    c1 = _counters(A)
    assert c1["translate_builds"] == 1 and c1["joint_rank_builds"] == 1 and c1["map_launches"] == 1 and c1["like_launches"] == 1

    # 2. the same batch again: no new value (the id counter may move: only like_table follows it)
    enc(A, ["apple", "Berlin"])
    _read_and_check(A, B)
    c2 = _counters(A)
    for c in ("translate_builds", "joint_rank_builds", "map_launches", "map_ids_mapped"):
        assert c2[c] == c1[c], c

    # 3. every call again, nothing encoded in between: no counter moves, the same columns
    first = _read_and_check(A, B)
    c3 = _counters(A)
    again = _read_and_check(A, B)
    assert _counters(A) == c3
    for name in first:
        assert np.array_equal(first[name], again[name]), name

    # 4. three new values: one non-ASCII, one whose upper case the derived dictionary holds already ("APPLE")
    ids_before, n_ids_before, mapped_before = _by_id(A), len(_by_id(A)), c3["map_ids_mapped"]
    covered_before = len(first["mapped"])
    enc(A, ["ärger", "Apple", "avocado", "apple"])
    t4 = _read_and_check(A, B)
    c4 = _counters(A)
    assert A.mapped("upper")[0] is derived and derived.code_of("ÄRGER") is not None
    assert t4["mapped"][A.code_of("Apple")] == t4["mapped"][A.code_of("apple")] == derived.code_of("APPLE")
    assert c4["map_launches"] == c3["map_launches"] + 1
    assert c4["map_ids_mapped"] - mapped_before == len(_by_id(A)) - covered_before      # only the ids past what the table covered
    assert len(_by_id(A)) > n_ids_before
    assert c4["translate_builds"] == c3["translate_builds"] + 1 and c4["joint_rank_builds"] == c3["joint_rank_builds"] + 1
    _live_prefix_unchanged(first, t4, ids_before)

    # 5. B gains a value A holds, which translated to -2 so far: the whole table is built again, and the joint ranks
    assert t4["translate"][A.code_of("Berlin")] == -2
    enc(B, ["Berlin", "zebra"])
    t5 = _read_and_check(A, B)
    c5 = _counters(A)
    assert t5["translate"][A.code_of("Berlin")] == B.code_of("Berlin") >= 0
    assert c5["translate_builds"] == c4["translate_builds"] + 1 and c5["joint_rank_builds"] == c4["joint_rank_builds"] + 1
    assert c5["map_launches"] == c4["map_launches"] and c5["like_launches"] == c4["like_launches"]

    # 6. forty new values in one batch: every earlier entry survives the growth
    ids_before = _by_id(A)
    enc(A, [f"{'a' if i % 3 else 'q'}value{i:02d}" for i in range(40)] + ["Berlin"])
    t6 = _read_and_check(A, B)
    c6 = _counters(A)
    assert c6["map_launches"] == c5["map_launches"] + 1 and c6["translate_builds"] == c5["translate_builds"] + 1
    _live_prefix_unchanged(t5, t6, ids_before)
    # the tables of before the first value, read for the first time since
    other_like = A.like_table("B%").to_numpy()
    _check_entries("like 'B%'", other_like, _by_id(A), lambda v: v.startswith("B"), None)
    lower, lower_table = A.mapped("lower")
    _check_entries("mapped lower", lower_table.to_numpy(), _by_id(A), lambda v: lower.code_of(pc.utf8_lower(pa.scalar(v)).as_py()), -2)

    # 7. B dies; another dictionary -- at B's address or not -- gets a table of its own
    builds = A.translate_builds
    del B
    gc.collect()
    C = KeyDictionary(pa.string())
    enc(C, ["avocado", "nothing A holds"])
    _read_and_check(A, C)
    assert A.translate_builds == builds + 1
    assert A.translate_table(C).to_numpy()[A.code_of("avocado")] == C.code_of("avocado")
    assert A.translate_builds == builds + 1


def test_a_malformed_value_is_never_recorded_as_mapped():
    from vinum_amd.vinum_lib import KeyDictionary
    raw = pa.array([b"ok", b"a\xc3", b"fine"], pa.binary())
    bad = pa.Array.from_buffers(pa.string(), 3, raw.buffers())     # (no validation: what a file read without it delivers)
    kd = KeyDictionary(pa.string())
    derived, table = kd.mapped("upper")                           # (of the empty dictionary: the one derived dictionary, nothing launched)
    assert kd.map_launches == 0 and len(table.to_numpy()) == 0
    kd.encode(bad)
    for launches in (1, 2):                                       # nothing was recorded as covered: the second call maps, and raises, again
        with pytest.raises(ValueError, match="Invalid UTF8 sequence in input"):
            kd.mapped("upper")
        assert kd.map_launches == launches and kd.map_ids_mapped == launches * len(kd.values_by_code())
    # the well-formed values are in the derived dictionary all the same, and it decodes them
    assert sorted(derived.values_by_code().drop_null().to_pylist()) == ["FINE", "OK"]
    assert derived.decode(pa.array([derived.code_of("OK"), derived.code_of("FINE")], pa.int32())).to_pylist() == ["OK", "FINE"]
