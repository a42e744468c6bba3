// C ABI: the dense path with a code range all ranks agree on (direct-addressed tables, their merge), host-only plan helpers.
// Part of the aggregate operator; included by vnm_agg.hip (one translation unit: the kernels and the host code share file-local helpers).
// ---- multi-GPU: the dense path with a code range all ranks agree on ---------------------------------------------------------
// vnm_agg_dense_range: this rank's sampled key range of a batch (order-preserving unsigned images; lo > hi: no dense path for this
// key type / range).  The ranks reduce lo by MIN and hi by MAX and hand the result to vnm_agg_set_dense_range: every rank then
// derives the SAME code map, so the direct-addressed tables of the final pass are slot-compatible across ranks.
int vnm_agg_dense_range(vnm_agg* h, int64_t nrows, const vnm_dcol* key, uint64_t* lo, uint64_t* hi, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !key || !lo || !hi) return set_error("vnm_agg_dense_range: bad argument");
    *lo = ~0ULL; *hi = 0;
    if (!h->single || h->plan.n_keys != 1 || nrows <= 0 || (key->type != VNM_I64 && key->type != VNM_U64) || key->validity) return 0;
    hipStream_t s = as_stream(stream);
    const uint64_t sign = key->type == VNM_I64 ? 0x8000000000000000ULL : 0ULL;
    PoolScope pool;   // (every early return gives the block back)
    unsigned long long* d = (unsigned long long*)pool.take(64);
    if (!d) return 1;
    const unsigned long long init[2] = {~0ULL, 0ULL};
    unsigned long long got[2];
    VNM_HIP(hipMemcpyAsync(d, init, 16, hipMemcpyHostToDevice, s));
    const int64_t m = std::min<int64_t>(nrows, 1 << 18);
    const int grid = (int)std::min<int64_t>((m + 255) / 256, (int64_t)device_info().num_cus * 4);
    dense_sample_range_kernel<<<grid, 256, 0, s>>>((const uint64_t*)key->values + key->offset, nrows, m, sign, d, nullptr, 0);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(got, d, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    *lo = got[0]; *hi = got[1];
    return 0;
}

int vnm_agg_set_dense_range(vnm_agg* h, int key_type, uint64_t lo, uint64_t hi) {
    if (!h) return set_error("vnm_agg_set_dense_range: null handle");
    h->range_given = false;
    h->dense_state = -1;
    if (lo > hi) return 0;
    VNM_TRY(plan_dense_from_range(h, key_type, lo, hi));
    h->range_given = h->dense_state == 1;
    return 0;
}

// The direct-addressed tables of the (deferred) final pass: *table = 2^bits slots of {sum f64, lo f32, count u32}, slot = code'.
// *table = nullptr when the handle holds anything else (no dense batch, spilled keys, several batches): use another exchange.
// The geometry words let the ranks check that they really derived the same map: {lo_u, bits, mul, sign}.
int vnm_agg_dense_table(vnm_agg* h, void** table, int* bits, uint64_t* geometry, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !table || !bits) return set_error("vnm_agg_dense_table: bad argument");
    *table = nullptr; *bits = 0;
    VNM_TRY(flush_queue(h, stream));
    DensePending* pd = h->inner ? nullptr : h->pending;
    if (!pd || h->have_table || h->have_run || h->n_groups >= 0 || (h->ex && h->ex->switched)) return 0;
    const int rc = complete_pending(h, as_stream(stream), DF_TABLE);
    if (rc == 2) return 0;
    if (rc) return rc;
    *table = pd->table;
    *bits = pd->df.map.bits;
    if (geometry) { geometry[0] = pd->df.map.lo_u; geometry[1] = (uint64_t)pd->df.map.bits; geometry[2] = pd->df.map.mul; geometry[3] = pd->df.map.sign; }
    return 0;
}

// Owner side: `nsrc` slices of such tables (slots [code0, code0 + n) of every rank, in rank order) -> this (empty) handle's result.
// The map is the one of `like` (any handle that produced one of the tables).
int vnm_agg_merge_dense_tables(vnm_agg* h, const vnm_agg* like, int nsrc, const void* const* slices, uint64_t code0, int64_t n, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !like || !like->pending || nsrc < 1 || nsrc > 64 || !slices || n < 0) return set_error("vnm_agg_merge_dense_tables: bad argument");
    if (h->have_table || h->have_run || h->pending) return set_error("vnm_agg_merge_dense_tables: the handle must be empty");
    if (h->plan.n_words != like->plan.n_words) return set_error("vnm_agg_merge_dense_tables: different aggregate programs");
    hipStream_t s = as_stream(stream);
    invalidate_result(h);
    const DFinalArgs& ld = like->pending->df;
    PoolScope pool;
    const int64_t dstride = n + 2;
    uint64_t* rk = (uint64_t*)pool.take((size_t)dstride * 8 * 2);
    uint64_t* ra = (uint64_t*)pool.take((size_t)dstride * 8 * h->plan.n_words);
    unsigned long long* flags = (unsigned long long*)pool.take(64);
    if (!rk || !ra || !flags) return 1;
    VNM_HIP(hipMemsetAsync(flags, 0, 64, s));
    DTabMergeArgs a{};
    a.map = ld.map;
    for (int r = 0; r < nsrc; r++) a.src[r] = (const DTabSlot*)slices[r];
    a.nsrc = nsrc; a.n = n; a.code0 = (uint32_t)code0;
    a.w_rows = ld.w_rows; a.w_valid = ld.w_valid; a.w_sum = ld.w_sum; a.w_lo = ld.w_lo;
    a.dkey = rk; a.dacc = ra; a.dstride = dstride; a.flags = flags;
    if (n > 0) {
        KernelTimer timer("agg_table_merge", s);
        dtable_merge_kernel<<<(int)((n + DTM_PER * DTM_BLOCK - 1) / (DTM_PER * DTM_BLOCK)), DTM_BLOCK, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long fl[2];
    VNM_HIP(hipMemcpyAsync(fl, flags, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (fl[0]) return set_error("vnm_agg_merge_dense_tables: output overflow (internal error)");
    pool.keep(rk); pool.keep(ra);
    adopt_run(h, rk, ra, dstride, (int64_t)fl[1]);
    return 0;
}

// host-only helpers: plan lowering and finalisation from accumulator words (no GPU needed)
int vnm_agg_plan_host(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs, const int* in_types,
                      const int* in_flags, const int* in_col_ids, int* n_key_words, int* n_acc_words,
                      int* merge_kinds /* >= 40 ints */, int* n_ops, int* op_kind_col_word /* >= 3 * 48 ints */) {
    AggPlan plan;
    FuncOut outs[AGG_MAX_FUNCS];
    VNM_TRY(build_plan(kind, n_keys, key_types, n_funcs, funcs, in_types, in_flags, in_col_ids, &plan, outs));
    if (n_key_words) *n_key_words = plan.kw;
    if (n_acc_words) *n_acc_words = plan.n_words;
    if (merge_kinds) for (int w = 0; w < plan.n_words; w++) merge_kinds[w] = plan.merge[w];
    if (n_ops) *n_ops = plan.n_ops;
    if (op_kind_col_word)
        for (int o = 0; o < plan.n_ops; o++) {
            op_kind_col_word[3 * o] = plan.ops[o].kind;
            op_kind_col_word[3 * o + 1] = plan.ops[o].col;
            op_kind_col_word[3 * o + 2] = plan.ops[o].word;
        }
    return 0;
}

int vnm_agg_finalize_host(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs, const int* in_types,
                          const int* in_flags, const int* in_col_ids, int func_idx, int64_t n,
                          const uint64_t* const* acc_words, void* cells16, uint8_t* valid, int* out_kind) {
    AggPlan plan;
    FuncOut outs[AGG_MAX_FUNCS];
    VNM_TRY(build_plan(kind, n_keys, key_types, n_funcs, funcs, in_types, in_flags, in_col_ids, &plan, outs));
    if (func_idx < 0 || func_idx >= n_funcs) return set_error("vnm_agg_finalize_host: function index out of range");
    return finalize_func(outs[func_idx], n, acc_words, cells16, valid, out_kind);
}
