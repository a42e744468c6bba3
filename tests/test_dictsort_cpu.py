"""The NumPy model of vnm_dict_take_compact (tests/dictsort_util.py: what tests/test_gpu_dictsort.py holds the kernels against) is
itself held against pyarrow, and the types vinum_lib.Sort hands to the library are listed.  No GPU."""
import numpy as np
import pyarrow as pa
import pytest

from tests.dictsort_util import INDEX_TYPES, OVERFLOW, VALUE_TYPES, sort_table, take_compact_model


@pytest.mark.parametrize("index_type", INDEX_TYPES)
@pytest.mark.parametrize("rows_kind", ["identity", "permutation", "prefix"])
def test_the_model_builds_the_array_arrow_would(index_type, rows_kind):
    rng = np.random.default_rng(len(index_type) * 7 + len(rows_kind))
    for n, n_ids, p_null in ((0, 5, 0.0), (1, 1, 0.0), (500, 300, 0.1), (500, 90, 1.0), (3000, 100, 0.3)):
        n_ids = min(n_ids, int(np.iinfo(np.dtype(index_type)).max))
        codes = rng.integers(0, n_ids, n).astype(np.int32)
        codes[rng.random(n) < p_null] = -1
        rows = None if rows_kind == "identity" else rng.permutation(n)[:n if rows_kind == "permutation" else n // 3]
        values = pa.array([f"value{i}" for i in range(n_ids)])
        m = take_compact_model(codes, rows, n_ids, index_type)
        assert m["bad"] == 0 and not m["overflow"]
        got = pa.DictionaryArray.from_arrays(pa.array(m["indices"], mask=~m["valid"]), values.take(pa.array(m["used_ids"])))
        got.validate(full=True)
        taken = codes if rows is None else codes[rows]
        want = values.take(pa.array(np.where(taken >= 0, taken, 0), mask=taken < 0))
        assert got.cast(pa.string()).equals(want)
        assert got.null_count == m["null_count"] == int((taken < 0).sum())
        # no duplicate, no unused entry
        assert len(set(m["used_ids"].tolist())) == len(m["used_ids"])
        assert set(np.unique(m["indices"][m["valid"]]).tolist()) == set(range(len(m["used_ids"])))
        assert np.array_equal(np.unpackbits(m["bitmap"], bitorder="little")[:len(taken)].astype(bool), taken >= 0)


@pytest.mark.parametrize("index_type, k", [("int8", 127), ("int8", 128), ("int8", 200), ("uint8", 255), ("uint8", 256), ("int16", 300)])
def test_overflow_is_where_arrow_refuses_to_unify(index_type, k):
    """two batches whose dictionaries together hold k distinct values: pa.concat_arrays raises exactly where the model says the used
    ids do not fit the index type (int8: two batches of 100 distinct values each)"""
    first = k // 2
    t = pa.from_numpy_dtype(np.dtype(index_type))
    a = pa.DictionaryArray.from_arrays(pa.array(np.arange(first), t), pa.array([f"a{i}" for i in range(first)]))
    b = pa.DictionaryArray.from_arrays(pa.array(np.arange(k - first), t), pa.array([f"b{i}" for i in range(k - first)]))
    m = take_compact_model(np.arange(k, dtype=np.int32), None, k + 3, index_type)
    assert len(m["used_ids"]) == k
    if m["overflow"]:
        with pytest.raises(pa.ArrowInvalid) as e:
            pa.concat_arrays([a, b])
        assert OVERFLOW in str(e.value)
    else:
        assert len(pa.concat_arrays([a, b]).dictionary) == k
    assert m["overflow"] == (k > np.iinfo(np.dtype(index_type)).max)


def test_a_code_past_the_ids_is_counted_not_used():
    m = take_compact_model([0, 5, 2, -1, 7], None, 5, "int32")
    assert m["bad"] == 2 and m["used_ids"].tolist() == [0, 2] and m["null_count"] == 1


def test_the_tables_of_the_gpu_tests_hold_what_they_promise():
    batches, decoded = sort_table(pa.string(), pa.int8())
    c = [b.column("c") for b in batches]
    assert [len(b) % 8 for b in batches].count(0) < len(batches) and c[0].offset == 13 and c[2].offset == 1
    assert all(x.dictionary.null_count == 1 for x in c)
    assert sum(x.null_count for x in c) < decoded["c"].null_count          # rows that are NULL only because their value is
    assert c[3].dictionary.buffers()[2].address == c[2].dictionary.buffers()[2].address
    assert c[0].dictionary.to_pylist() != c[1].dictionary.to_pylist()
    for x in c:                                                              # a value no row uses
        assert len(set(x.indices.drop_null().to_pylist())) < len(x.dictionary)


@pytest.mark.parametrize("value_type", VALUE_TYPES, ids=str)
@pytest.mark.parametrize("index_type", INDEX_TYPES)
def test_sort_and_aggregates_take_dictionary_typed_strings_below_the_abi(index_type, value_type):
    from vinum_amd.vinum_lib import Sort, _abi_generic_key
    for ordered in (False, True):
        t = pa.dictionary(pa.from_numpy_dtype(np.dtype(index_type)), value_type, ordered)
        assert Sort._below_the_abi(t) and _abi_generic_key(t)


def test_a_dictionary_over_other_values_stays_on_the_host_route():
    from vinum_amd.vinum_lib import Sort, _abi_generic_key
    assert not Sort._below_the_abi(pa.dictionary(pa.int32(), pa.int64()))
    assert not _abi_generic_key(pa.dictionary(pa.int32(), pa.int64()))
