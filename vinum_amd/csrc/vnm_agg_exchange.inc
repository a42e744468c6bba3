// C ABI: multi-GPU exchange helpers (owner bucketing, partition-aligned runs).
// Part of the aggregate operator; included by vnm_agg.hip (one translation unit: the kernels and the host code share file-local helpers).
// ---- partition-aligned exchange (multi-GPU, large G) ------------------------------------------------------
// Number of final partitions when the finished result is a partition-structured run (partitioned path,
// nothing merged into it since), else 0.  All ranks must report the same non-zero value to use this exchange.
int64_t vnm_agg_run_partitions(vnm_agg* h) {
    if (!h) return 0;
    int64_t n = 0;
    if (vnm_agg_finish(h, &n, nullptr) != 0) return 0;
    if (!(h->result_is_run && h->run_dir) || (h->ex && h->ex->switched)) return 0;
    // only what vnm_agg_merge_partitioned can merge: add-merge words (MIN / MAX programs and anything wider than the
    // LDS merge table go through the owner-bucketed exchange)
    if (h->plan.n_words > PM_MAX_WORDS) return 0;
    for (int w = 0; w < h->plan.n_words; w++)
        if (h->plan.merge[w] != M_ADD_U64 && h->plan.merge[w] != M_ADD_F64 && h->plan.merge[w] != M_ADD_F64C) return 0;
    return h->run_nfin;
}

// Rows of the run in partition order, row-major [n][2 + n_acc_words]; per-partition row counts (device,
// uint32[nfin]); rows per owner (host) with owner(f) = f * world / nfin.
int vnm_agg_run_reorder(vnm_agg* h, int world, uint64_t* out_rows, uint32_t* out_part_counts, int64_t* owner_counts_host,
                        void* stream) {
    VNM_TRY(ensure_init());
    if (!h || world < 1 || !out_part_counts || !owner_counts_host) return set_error("vnm_agg_run_reorder: bad argument");
    if (!vnm_agg_run_partitions(h)) return set_error("vnm_agg_run_reorder: the result is not a partition-structured run");
    hipStream_t s = as_stream(stream);
    RunReorderArgs a{};
    a.nw = 2 + h->plan.n_words;
    a.words[0] = h->run_key;
    a.words[1] = h->run_key + h->run_stride;
    for (int w = 0; w < h->plan.n_words; w++) a.words[2 + w] = h->run_acc + (size_t)w * h->run_stride;
    a.nfin = h->run_nfin;
    a.dir = h->run_dir;
    a.out = out_rows;
    a.part_counts = out_part_counts;
    PoolScope pool;   // (every way out frees the prefix)
    a.prefix = (unsigned long long*)pool.take((size_t)(a.nfin + 1) * 8);
    if (!a.prefix) return 1;
    run_prefix_kernel<<<1, 1024, 0, s>>>(a);
    run_reorder_kernel<<<(int)std::min<int64_t>(a.nfin, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(a);
    VNM_HIP(hipGetLastError());
    std::vector<unsigned long long> bounds((size_t)world + 1);
    for (int o = 0; o <= world; o++) {
        int64_t f = (int64_t)o * a.nfin / world;  // first partition of owner o (inverse of owner(f) = f * world / nfin)
        while (f < a.nfin && f > 0 && (f * world) / a.nfin < o) f++;
        VNM_HIP(hipMemcpyAsync(&bounds[o], a.prefix + f, 8, hipMemcpyDeviceToHost, s));
    }
    VNM_HIP(hipStreamSynchronize(s));
    for (int o = 0; o < world; o++) owner_counts_host[o] = (int64_t)(bounds[o + 1] - bounds[o]);
    return 0;
}

// Owner side: merge the segments received from all ranks.  rows: received rows grouped by source rank (each in
// partition order); src_row_offsets_host[world + 1]: row offset of every source block; part_counts: device
// uint32 [world][nlocal] rows per (source, owned partition).  The merged groups become this handle's result.
int vnm_agg_merge_partitioned(vnm_agg* h, int world, int64_t nlocal, const uint64_t* rows, const int64_t* src_row_offsets_host,
                              const uint32_t* part_counts, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || world < 1 || nlocal < 1) return set_error("vnm_agg_merge_partitioned: bad argument");
    if (h->have_table || h->have_run) return set_error("vnm_agg_merge_partitioned: the handle must be empty");
    if (h->plan.n_words > PM_MAX_WORDS) return set_error("vnm_agg_merge_partitioned: at most %d accumulator words", PM_MAX_WORDS);
    for (int w = 0; w < h->plan.n_words; w++)
        if (h->plan.merge[w] != M_ADD_U64 && h->plan.merge[w] != M_ADD_F64 && h->plan.merge[w] != M_ADD_F64C) return set_error("vnm_agg_merge_partitioned: add-merge words only");
    hipStream_t s = as_stream(stream);
    invalidate_result(h);
    // per-source exclusive prefix over the owned partitions -> absolute row offsets
    std::vector<uint32_t> pc((size_t)world * nlocal);
    VNM_HIP(hipMemcpyAsync(pc.data(), part_counts, pc.size() * 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> pre((size_t)world * (nlocal + 1));
    int64_t total = 0;
    for (int r = 0; r < world; r++) {
        unsigned long long run = (unsigned long long)src_row_offsets_host[r];
        for (int64_t f = 0; f < nlocal; f++) { pre[(size_t)r * (nlocal + 1) + f] = run; run += pc[(size_t)r * nlocal + f]; }
        pre[(size_t)r * (nlocal + 1) + nlocal] = run;
        if ((int64_t)run != src_row_offsets_host[r + 1]) return set_error("vnm_agg_merge_partitioned: partition counts of source %d do not add up", r);
        total = (int64_t)run;
    }
    PoolScope pool;   // every way out frees the four blocks; the run's two are handed to the handle (keep) on success
    unsigned long long* dpre = (unsigned long long*)pool.take(pre.size() * 8);
    unsigned long long* flags = (unsigned long long*)pool.take(64);
    const int64_t dstride = total + 2;
    uint64_t* rk = (uint64_t*)pool.take((size_t)dstride * 16);
    uint64_t* ra = (uint64_t*)pool.take((size_t)dstride * 8 * h->plan.n_words);
    if (!dpre || !flags || !rk || !ra) return 1;
    VNM_HIP(hipMemcpyAsync(dpre, pre.data(), pre.size() * 8, hipMemcpyHostToDevice, s));
    VNM_HIP(hipMemsetAsync(flags, 0, 64, s));
    PartMergeArgs m{};
    m.rows = rows; m.src_prefix = dpre; m.world = world; m.nlocal = nlocal;
    m.nw = 2 + h->plan.n_words; m.n_words = h->plan.n_words;
    for (int w = 0; w < h->plan.n_words; w++) m.merge[w] = h->plan.merge[w];
    m.dkey = rk; m.dacc = ra; m.dstride = dstride; m.flags = flags;
    {
        KernelTimer timer("agg_part_merge", s);
        int occ = 0;  // one resident set of workgroups, as in the final pass
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)part_merge_kernel, PA_BLOCK, 0) != hipSuccess || occ < 1) occ = 2;
        part_merge_kernel<<<(int)std::min<int64_t>(nlocal, (int64_t)device_info().num_cus * occ), PA_BLOCK, 0, s>>>(m);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long fl[2];
    VNM_HIP(hipMemcpyAsync(fl, flags, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (fl[0]) {
        set_error("vnm_agg_merge_partitioned: a partition holds more groups than the LDS table (use vnm_agg_merge_rows)");
        return 2;  // capacity, not an error of the data: the handle is still empty and the caller falls back
    }
    pool.keep(rk); pool.keep(ra);
    adopt_run(h, rk, ra, dstride, (int64_t)fl[1]);   // (no directory: the handle was empty)
    return 0;
}

int vnm_agg_layout(vnm_agg* h, int* n_key_words, int* n_acc_words) {
    if (!h) return set_error("vnm_agg_layout: null handle");
    if (n_key_words) *n_key_words = h->plan.kw;
    if (n_acc_words) *n_acc_words = h->plan.n_words;
    return 0;
}

int vnm_agg_dense_ptrs(vnm_agg* h, uint64_t** key_words, uint64_t** acc_words) {
    if (!h) return set_error("vnm_agg_dense_ptrs: null handle");
    if (h->n_groups < 0) return set_error("vnm_agg_dense_ptrs: call vnm_agg_finish first");
    for (int j = 0; j < h->plan.kw; j++) key_words[j] = h->dkey ? h->dkey + (size_t)j * h->dstride : nullptr;
    for (int w = 0; w < h->plan.n_words; w++) acc_words[w] = h->dacc ? h->dacc + (size_t)w * h->dstride : nullptr;
    return 0;
}

static int fetch_host(vnm_agg* h) {
    if (h->host_ready) return 0;
    int64_t n = 0;
    VNM_TRY(vnm_agg_finish(h, &n, nullptr));
    h->h_key.assign((size_t)(h->plan.kw ? h->plan.kw : 1) * (n ? n : 1), 0);
    h->h_acc.assign((size_t)h->plan.n_words * (n ? n : 1), 0);
    if (n > 0) {
        for (int j = 0; j < h->plan.kw; j++)
            VNM_HIP(hipMemcpy(h->h_key.data() + (size_t)j * n, h->dkey + (size_t)j * h->dstride, (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int w = 0; w < h->plan.n_words; w++)
            VNM_HIP(hipMemcpy(h->h_acc.data() + (size_t)w * n, h->dacc + (size_t)w * h->dstride, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    h->host_ready = true;
    return 0;
}

int vnm_agg_result_key(vnm_agg* h, int key_idx, uint64_t* vals, uint8_t* valid) {
    if (!h) return set_error("vnm_agg_result_key: null handle");
    if (key_idx < 0 || key_idx >= h->plan.n_keys) return set_error("vnm_agg_result_key: key index out of range");
    VNM_TRY(fetch_host(h));
    int64_t n = h->n_groups;
    const uint64_t* k = h->h_key.data() + (size_t)key_idx * n;
    const uint64_t* nm = h->h_key.data() + (size_t)h->plan.n_keys * n;
    for (int64_t r = 0; r < n; r++) {
        vals[r] = k[r];
        valid[r] = !((nm[r] >> key_idx) & 1);
    }
    return 0;
}

int vnm_agg_result_func(vnm_agg* h, int func_idx, void* cells16, uint8_t* valid, int* out_kind) {
    if (!h) return set_error("vnm_agg_result_func: null handle");
    if (func_idx < 0 || func_idx >= h->n_funcs) return set_error("vnm_agg_result_func: function index out of range");
    VNM_TRY(fetch_host(h));
    int64_t n = h->n_groups;
    const uint64_t* words[AGG_MAX_WORDS];
    for (int w = 0; w < h->plan.n_words; w++) words[w] = h->h_acc.data() + (size_t)w * n;
    return finalize_func(h->outs[func_idx], n, words, cells16, valid, out_kind);
}
