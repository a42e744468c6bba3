"""The GPU differential tests once more, over a red-zoned (mode 1) and a red-zoned + poisoned (mode 2) device pool.

Every byte of HBM the library takes for itself comes from the caching allocator of vnm_runtime.cpp, and that allocator is forgiving:
it rounds every request up (1/8 of the leading power of two, at least 4096 bytes), serves it from a cached block of up to twice
that size, and hands a recycled block out with whatever its last owner left in it.  A kernel that writes past the end of what it
asked for, or reads scratch nobody cleared, computes the right result in a short test process.  The allocator's guard mode
(vnm_pool_set_guard) turns both into something a test can see: canaries in front of and behind the bytes asked
for, checked on the device at every release, and a NaN / huge-integer poison word in every block handed out.

  a. the detector detects: planted one-byte and sixteen-byte writes into the zones are reported, with zone, offset and count;
  b. SELECTION: the project's own differential tests (imported as modules, called with chosen parameters) run in mode 1, then in
     mode 2; a leg fails on its own assertions or on any violation the guard recorded while it ran;
  c. every route of tests/test_zz_route_coverage.REQUIRED was taken with mode 2 on, EXEMPT aside.
"""
import ctypes
import inspect
import re

import numpy as np
import pyarrow as pa
import pytest

from tests import test_gpu_agg as A
from tests import test_gpu_batch_layout as BL
from tests import test_gpu_csv as C
from tests import test_gpu_filter as F
from tests import test_gpu_like as K
from tests import test_gpu_round4 as R4
from tests import test_gpu_round5 as R5
from tests import test_gpu_round6 as R6
from tests import test_gpu_scalar_functions as S
from tests import test_gpu_sort_project as SP
from tests import test_gpu_vinum_lib as V
from tests import test_zz_route_coverage as ZZ

pytestmark = pytest.mark.gpu

POISON = 0x7FF8DEAD7FC0BEEF


def _lib():
    from vinum_amd import _lib as L
    return L.lib()


def _report():
    lib = _lib()
    v, c = ctypes.c_int64(0), ctypes.c_int64(0)
    need = lib.vnm_pool_guard_report(None, 0, ctypes.byref(v), ctypes.byref(c))
    buf = ctypes.create_string_buffer(int(need) + 65536)     # (the call itself checks the live blocks: it may find more)
    lib.vnm_pool_guard_report(buf, len(buf), ctypes.byref(v), ctypes.byref(c))
    return buf.value.decode(), v.value, c.value


def _layout(nbytes):
    block, front, back = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    assert _lib().vnm_pool_guard_layout(nbytes, ctypes.byref(block), ctypes.byref(front), ctypes.byref(back)) == 0
    return block.value, front.value, back.value


def _round_size(b):
    b = max(b, 1)
    if b < 4096:
        return 4096
    step = (1 << (b.bit_length() - 1)) // 8
    return (b + step - 1) // step * step


# ---- a. the detector detects ---------------------------------------------------------------------------------------------------
def _violations(text):
    out = []
    for line in text.splitlines():
        if line.startswith("violation "):
            f = dict(m.groups() for m in re.finditer(r"(\w+)=(\S+)", line.split(" site=")[0]))
            out.append((int(f["ptr"], 16), f["zone"], int(f["offset"]), int(f["bytes"]), int(f["requested"]), int(f["block"]), f["first"], line))
    return out


@pytest.mark.parametrize("case", ["1000_bytes", "5000000_bytes", "4097_bytes_from_a_cached_block_of_6000"])
def test_planted_writes_into_the_zones_are_reported(case):
    lib = _lib()
    nbytes = {"1000_bytes": 1000, "5000000_bytes": 5_000_000}.get(case, 4097)
    lib.vnm_device_synchronize()
    lib.vnm_pool_trim()                      # every block below is fresh, or the one this test cached itself
    assert lib.vnm_pool_set_guard(2) == 0
    try:
        lib.vnm_pool_guard_reset()
        block, front, back_min = _layout(nbytes)
        if case.startswith("4097"):
            raw = _layout(6000)[0]
            first = [lib.vnm_malloc(6000) for _ in range(4)]
            for p in first:
                lib.vnm_free(p)
            assert _report()[1:] == (0, 4)
            lib.vnm_pool_guard_reset()
            assert block <= raw <= 2 * block and raw > block          # the cached blocks serve the smaller request, with slack
        else:
            raw = block
        ptrs = [lib.vnm_malloc(nbytes) for _ in range(4)]
        assert all(ptrs) and all(p % 4096 == 0 for p in ptrs)
        if case.startswith("4097"):
            assert sorted(ptrs) == sorted(first)
        back = raw - front - nbytes              # the whole slack is red zone
        assert back >= back_min >= 4096
        body = np.zeros(nbytes, dtype=np.uint8)
        lib.vnm_memcpy_d2h(body.ctypes.data, ptrs[0], nbytes)
        want = np.frombuffer(np.uint64(POISON).tobytes() * (nbytes // 8 + 1), dtype=np.uint8)[:nbytes]
        assert np.array_equal(body, want), "mode 2 hands out a poisoned body"
        # three writes, all INSIDE the raw blocks: first byte behind the body, last byte before it, last 16 bytes of the raw block
        lib.vnm_memset(ptrs[0] + nbytes, 0x5A, 1)
        lib.vnm_memset(ptrs[1] - 1, 0x5A, 1)
        sixteen = bytes(range(1, 17))
        lib.vnm_memcpy_h2d(ptrs[2] - front + raw - 16, sixteen, 16)
        for p in ptrs:
            lib.vnm_free(p)
        text, violations, checked = _report()
        found = _violations(text)
        assert (violations, checked) == (3, 4), text
        assert sorted(v[:6] for v in found) == sorted([
            (ptrs[0], "back", 0, 1, nbytes, raw), (ptrs[1], "front", -1, 1, nbytes, raw), (ptrs[2], "back", back - 16, 16, nbytes, raw)]), text
        assert {v[0]: v[6] for v in found}[ptrs[2]] == sixteen.hex()
        assert ptrs[3] not in [v[0] for v in found]
        assert all("test_planted_writes" in v[7] and "libvinum_hip" in v[7] for v in found), text   # attributed to this test and to a call site
    finally:
        lib.vnm_pool_set_guard(0)
        lib.vnm_pool_guard_reset()


def test_guard_off_is_the_allocator_of_always():
    lib = _lib()
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(0) == 0
    for nbytes in [0, 1, 1000, 4097, 6000, 5_000_000]:
        assert _layout(nbytes) == (_round_size(nbytes), 0, 0)
    lib.vnm_pool_guard_reset()
    lib.vnm_pool_trim()
    p = lib.vnm_malloc(1000)
    lib.vnm_free(p)
    assert lib.vnm_pool_cached_bytes() == 4096 == _round_size(1000)     # (guarded it would be a 9216-byte raw block)
    assert lib.vnm_malloc(1000) == p                                    # and the freed block itself is handed out again, as it was left
    lib.vnm_free(p)
    assert _report()[1:] == (0, 0)                                      # nothing guarded, nothing checked


# ---- b. the differential tests under the guard --------------------------------------------------------------------------------
# (module, test function, its parameters) -- and which kernels / buffers the entry is there for
SELECTION = [
    # filter: tile edges with NULLs and a slice offset (bitmap tails, compacted outputs of 1 and 4097 rows)
    (F, "test_filter_edges_vs_oracle", dict(n=1, nulls=True, offset=3)),
    (F, "test_filter_edges_vs_oracle", dict(n=4097, nulls=True, offset=3)),
    (F, "test_random_filters_vs_oracle", dict(seed=16)),      # n = 0
    (F, "test_random_filters_vs_oracle", dict(seed=0)),       # n = 8193: one row into the third tile
    (F, "test_random_filters_vs_oracle", dict(seed=3)),       # n = 300001
    (F, "test_filter_emit_null_mask", {}),                    # the emitted validity bitmap
    (F, "test_int64_predicate_hot_path", dict(n=8193, kind="int64_with_payload", op=">")),
    (F, "test_int64_predicate_hot_path", dict(n=8193, kind="int64_nullable", op="!=")),
    (F, "test_filter_launch_schemes", dict(scheme="flat_gives_up")),   # the discarded first attempt wrote only where it may
    # projection: ragged last tiles behind full-tile 16-byte stores
    (SP, "test_random_expressions_vs_numpy", dict(seed=4)),    # n = 1
    (SP, "test_random_expressions_vs_numpy", dict(seed=7)),    # n = 1025
    (SP, "test_random_expressions_vs_numpy", dict(seed=16)),   # n = 1025, other trees
    (SP, "test_random_expressions_narrow_types_vs_numpy", dict(seed=1)),    # n = 1, 1- and 2-byte outputs
    (SP, "test_random_expressions_narrow_types_vs_numpy", dict(seed=0)),    # n = 4097
    (SP, "test_random_expressions_narrow_types_vs_numpy", dict(seed=11)),   # n = 4097, other types
    (SP, "test_project_many_equals_single_expression_kernels", {}),
    (S, "test_exact_functions_bit_for_bit", dict(col="i16")),                # N = 4099 in that module
    (S, "test_transcendentals_within_ulp_bound", dict(col="f32", fn="sin")),
    (S, "test_integer_power_bit_for_bit", dict(col="i32")),
    (S, "test_float_power_and_float16_arithmetic", {}),                      # 2-byte outputs
    (S, "test_negative_exponent_column_raises_and_leaves_no_fault", {}),     # the neg_pow flag block
    # LIKE: table per dictionary id, LOOKUP_U8 projection, codes past the table's length
    (K, "test_matcher_against_re", dict(arrow_type=pa.string())),
    (K, "test_having_on_a_string_key_and_select_list", {}),
    (K, "test_several_patterns_on_one_column_in_one_select_list", {}),
    (K, "test_growing_dictionary_extends_the_table", {}),
    # string dictionary: table, heap, id_off / id_len; high_cardinality grows the table inside a batch
    (V, "test_string_dictionary_on_the_device", dict(case="cities")),
    (V, "test_string_dictionary_on_the_device", dict(case="lengths_and_unicode")),
    (V, "test_string_dictionary_on_the_device", dict(case="all_null_and_empty")),
    (V, "test_string_dictionary_on_the_device", dict(case="high_cardinality")),
    # CSV parser: column outputs per block, quoted fields, string / date / timestamp columns
    (C, "test_gpu_csv_reader_equals_pyarrow", dict(block_size=1 << 16)),
    (C, "test_quoted_fields_stay_on_the_device", {}),
    (C, "test_string_date_and_timestamp_columns_stay_on_the_device", dict(block_size=1 << 15)),
    (C, "test_csv_fuzz_vs_pyarrow", dict(seed=0)),
    (C, "test_csv_fuzz_vs_pyarrow", dict(seed=1)),
    (C, "test_csv_fuzz_vs_pyarrow", dict(seed=2)),
    (C, "test_csv_fuzz_vs_pyarrow", dict(seed=3)),
    # sort: radix passes, histograms, sample sort buckets, top-K, ranks of string keys
    (SP, "test_random_sorts_vs_oracle", dict(seed=1)),     # n = 1
    (SP, "test_random_sorts_vs_oracle", dict(seed=9)),     # n = 63
    (SP, "test_random_sorts_vs_oracle", dict(seed=2)),     # n = 70 000
    (SP, "test_random_sorts_vs_oracle", dict(seed=15)),    # n = 260 000
    (SP, "test_topk_equals_full_sort_prefix", dict(n=70_000, k=10, desc=0, special=False)),
    (SP, "test_topk_equals_full_sort_prefix", dict(n=300_000, k=1000, desc=1, special=True)),
    (SP, "test_sample_sort_equals_the_lsd_sort", dict(case="f64_desc_nan_negzero")),
    (SP, "test_sample_sort_equals_the_lsd_sort", dict(case="heavy_value")),
    (SP, "test_sample_sort_of_a_four_byte_key_equals_the_lsd_sort", dict(case="f32_desc_nan_negzero")),
    (R6, "test_entry_word_sample_sort_equals_the_lsd_sort", dict(case="f64_uniform")),
    (R6, "test_entry_word_sample_sort_equals_the_lsd_sort", dict(case="odd_unaligned")),
    (R6, "test_entry_word_sample_sort_equals_the_lsd_sort", dict(case="already_sorted")),
    (R5, "test_raw_c_abi_sort_mixed_columns_vs_oracle", dict(seed=0)),     # 40 000 rows, long values: several rank rounds
    (R5, "test_raw_c_abi_sort_mixed_columns_vs_oracle", dict(seed=3)),     # 7 rows, long values
    (R5, "test_raw_c_abi_sort_mixed_columns_vs_oracle", dict(seed=2)),     # 250 000 rows
    (SP, "test_distributed_sample_sort_simulated", dict(world=3, desc=False)),   # vnm_partition_by_owner
    # aggregate -- NULL keys that first appear in a later batch, per route (side tables, packed-mode switch)
    (R4, "test_null_keys_first_appear_in_a_later_batch", dict(route="dense_two_level", later="null_keys", hint=0)),
    (R4, "test_null_keys_first_appear_in_a_later_batch", dict(route="dense_split_final", later="null_keys", hint=1)),
    (R4, "test_null_keys_first_appear_in_a_later_batch", dict(route="hash_partitions", later="null_keys", hint=1)),
    (R4, "test_null_keys_first_appear_in_a_later_batch", dict(route="split_program", later="null_keys_and_key_zero", hint=0)),
    (R4, "test_null_keys_first_appear_in_a_later_batch", dict(route="stream_table", later="null_keys", hint=0)),
    # a stream of batches in async mode: segments of one launch, batches singly, a shape that changes midstream
    (R4, "test_async_stream_of_batches", dict(route="dense_two_level", pred="none")),
    (R4, "test_async_stream_of_batches", dict(route="lds_scan_g7", pred="on_other")),
    (R4, "test_async_stream_of_batches", dict(route="hash_partitions", pred="on_input")),
    (R4, "test_async_stream_of_batches", dict(route="generic_program", pred="on_input")),
    (R4, "test_async_stream_of_batches", dict(route="shape_changes_midstream", pred="on_input")),
    (R4, "test_async_stream_of_batches", dict(route="stream_table_g3000", pred="none")),
    (R4, "test_async_stream_with_several_input_columns", dict(route="dense_per_column", pred="on_input")),
    # the fixed-point words of the dense path: the misfit redo, NULLs, two scatter levels, exact adds, two / three columns in one pass
    (R6, "test_fixed_point_misfit_falls_back", dict(misfit="tenth", where="second_batch")),
    (R6, "test_fixed_point_misfit_falls_back", dict(misfit="nan", where="first_batch_late_row")),
    (R6, "test_fixed_point_entries_vs_oracle", dict(groups=12_000_000, values="halves_negative", pred=True)),
    (R6, "test_fixed_point_entries_with_nulls_vs_oracle", dict(what="null_values_misfit", groups=1_500_000)),
    (R6, "test_exact_adds_without_compensation_words", dict(groups=6_000_000)),
    (R6, "test_fixed_point_columns_one_pass_vs_oracle", dict(ncols=2, groups=60_000, pred="none")),
    (R6, "test_fixed_point_columns_one_pass_vs_oracle", dict(ncols=3, groups=1_500_000, pred="own_column")),
    (R6, "test_fixed_point_columns_misfit_takes_the_per_column_route", {}),
    (R6, "test_fixed_point_stream_of_batches", dict(mode="stream")),
    # the ring form of the hash partitions and its way back
    (R6, "test_sparse_keys_through_the_ring_form_of_the_hash_partitions", dict(case="two_levels_2m")),
    (R6, "test_sparse_keys_through_the_ring_form_of_the_hash_partitions", dict(case="heavy_key_falls_back")),
    # ordered MIN / MAX mode (prefix / suffix composition), one-group kernels
    (R5, "test_ordered_min_max_fuzz_vs_oracle", dict(seed=14)),
    (R5, "test_ordered_min_max_fuzz_vs_oracle", dict(seed=22)),
    (R5, "test_ordered_min_max_fuzz_vs_oracle", dict(seed=9)),
    (R5, "test_ordered_min_max_fuzz_vs_oracle", dict(seed=31)),
    (R5, "test_ordered_min_max_fuzz_vs_oracle", dict(seed=7)),
    (R5, "test_ordered_min_max_result_then_more_batches", {}),
    # count(*) in byte counters: overflow into the wide counters, into the spilled entries, a second batch
    (R5, "test_count_star_over_many_groups_counts_in_bytes", dict(span_bits=23, variant="overflow")),
    (R5, "test_count_star_over_many_groups_counts_in_bytes", dict(span_bits=23, variant="overflow16")),
    (R5, "test_count_star_over_many_groups_counts_in_bytes", dict(span_bits=23, variant="two_batches")),
    # composite keys: the tuple dictionary (growing, merged, under a split program), dictionary-coded fields, the wide-key scan
    (A, "test_tuple_dictionary_for_keys_beyond_one_word", dict(scenario="dictionary_grows")),
    (A, "test_tuple_dictionary_for_keys_beyond_one_word", dict(scenario="nulls_and_floats")),
    (A, "test_tuple_dictionary_for_keys_beyond_one_word", dict(scenario="eight_columns")),
    (A, "test_tuple_dictionary_for_keys_beyond_one_word", dict(scenario="merged_afterwards")),
    (A, "test_multi_key_dictionary_coded_fields", dict(scenario="two_wide_int64")),
    (A, "test_multi_key_packed_composite_keys", dict(scenario="demote_on_later_batch")),
    (R5, "test_wide_key_table_scan_when_the_tuple_dictionary_is_switched_off", {}),
    # split programs and the scans over several columns
    (R4, "test_small_range_many_columns_split_per_column", dict(program="int_columns", pred="none", groups=5000, shape="one_batch")),
    (R4, "test_few_groups_under_more_than_six_columns", dict(ncols=7, groups=7, shape="one_batch")),
    (R4, "test_scan_over_three_to_six_float_columns", dict(ncols=5, pred="on_other", groups=5, shape="ragged_tail")),
    (R4, "test_dense_path_32_partitions_for_ranges_of_2e14_2e15_codes", dict(program="hot", groups=14_000, batches=3)),
    (R4, "test_random_programs_over_several_columns_vs_oracle", dict(seed=27)),
    (A, "test_gtest_known_answers", dict(name="int64_grp__int_overflow_arg_funcs")),
    (A, "test_random_plans_vs_oracle", dict(seed=29)),
    (A, "test_random_hot_shape_paths_vs_oracle", dict(seed=40)),
    (A, "test_heavy_keys_spill_from_wide_entries", dict(program="two_cols", heavy="null_key_half")),
    # results the library allocated (vnm_agg_result_device_alloc), adopted and freed by Python: every gpu_aggregate call above, and
    (A, "test_filter_groupby_vs_oracle", dict(groups=200_000, with_pred=True)),
    (A, "test_empty_inputs", {}),
    # batch plans x column layouts through the vinum_lib operators (string MIN / MAX below the ABI, drifting key ranges)
    (BL, "test_aggregate_is_independent_of_batch_plan_and_layout", dict(zip(("op", "funcset", "layout", "plan", "unused"), BL.CELLS[0]))),
    (BL, "test_aggregate_is_independent_of_batch_plan_and_layout", dict(zip(("op", "funcset", "layout", "plan", "unused"), BL.CELLS[-1]))),
    (BL, "test_min_max_of_a_string_next_to_an_unused_column", dict(op="generic", a_type="string")),
]

# Routes of test_zz_route_coverage.REQUIRED that no leg takes with mode 2 on, and why.  At most 6, never a whole family.
EXEMPT = {
}
MAX_EXEMPT = 6

_taken_in_mode_2 = {}      # route -> notes left while a mode 2 leg ran
_legs_run = {1: 0, 2: 0}


def _leg_id(p):
    mode, (mod, name, kw) = p
    args = "-".join("+".join(v) if isinstance(v, list) else str(v) for v in kw.values())
    return f"mode{mode}-{mod.__name__.rpartition('.')[2]}.{name}[{args}]"


@pytest.fixture
def pool_guard(request):
    """Switches the guard on for one leg; the leg fails with the guard's report if a zone was damaged while it ran."""
    lib = _lib()
    mode = request.node.callspec.params["leg"][0]
    lib.vnm_device_synchronize()
    assert lib.vnm_pool_set_guard(mode) == 0
    lib.vnm_pool_guard_reset()
    try:
        yield mode
        text, violations, _ = _report()
    finally:
        lib.vnm_pool_set_guard(0)
    lib.vnm_pool_guard_reset()
    if violations:
        pytest.fail(f"the pool guard found {violations} damaged zone(s) in mode {mode}:\n{text}", pytrace=False)


def _module_fixture(mod, name):
    """A fixture the imported test module defines for itself (test_gpu_scalar_functions.dev): its function, called directly."""
    fx = getattr(mod, name)
    fn = fx._get_wrapped_function() if hasattr(fx, "_get_wrapped_function") else getattr(fx, "__wrapped__", fx)
    return fn()


# mode 1 cannot change what a kernel computes, so all of its legs come first
@pytest.mark.parametrize("leg", [(mode, entry) for mode in (1, 2) for entry in SELECTION], ids=_leg_id)
def test_differential_test_under_the_guard(leg, pool_guard, request):
    mode, (mod, name, kw) = leg
    fn = getattr(mod, name)
    args = dict(kw)
    for p in inspect.signature(fn).parameters:
        if p in args:
            continue
        args[p] = request.getfixturevalue(p) if p in ("monkeypatch", "tmp_path", "capsys") else _module_fixture(mod, p)
    before = ZZ._counts()
    fn(**args)
    if mode == 2:
        for route, n in ZZ._counts().items():
            if n > before.get(route, 0):
                _taken_in_mode_2[route] = _taken_in_mode_2.get(route, 0) + n - before.get(route, 0)
    _legs_run[mode] += 1


# ---- c. the route condition (keep this test last) ----------------------------------------------------------------------------
def test_every_required_route_ran_over_the_poisoned_pool():
    family = lambda r: r.partition(":")[0]
    assert set(EXEMPT) <= set(ZZ.REQUIRED), sorted(set(EXEMPT) - set(ZZ.REQUIRED))
    assert len(EXEMPT) <= MAX_EXEMPT
    for fam in sorted({family(r) for r in ZZ.REQUIRED}):
        assert any(family(r) == fam and r not in EXEMPT for r in ZZ.REQUIRED), f"every route of {fam}: is exempt"
    if _legs_run[2] < len(SELECTION):
        pytest.skip(f"{_legs_run[2]} of {len(SELECTION)} mode 2 legs ran in this process: the route condition needs all of them")
    missing = sorted(r for r in ZZ.REQUIRED if r not in EXEMPT and not _taken_in_mode_2.get(r))
    assert not missing, f"routes no mode 2 leg took: {missing}"
    stale = sorted(r for r in EXEMPT if _taken_in_mode_2.get(r))
    assert not stale, f"exempt routes that were taken after all: {stale}"
