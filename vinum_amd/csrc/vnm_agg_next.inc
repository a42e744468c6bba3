// The batch router of the group-by operator: everything between vnm_agg_next_device (queue, widening: vnm_agg.hip) and the
// kernels.  next_device_impl at the end of this file is the driver; it tries the routes in the order DESIGN.md section 4 names
// them, one stage function per family of routes:
//
//   try_nullable_key_dense   a nullable 8-byte key through the dense path (runs the driver again with the validity set aside)
//   route_packed_keys        keys:*            multi-column / odd single keys -> one packed word, the tuple dictionary, or demoted
//   route_split_program      split_program:*   the program cut into parts by input column
//   run_onegroup             onegroup:*        no GROUP BY
//   classify_batch           (no route: what shape the batch has -> BatchShape and the hot_* / hn_* / part_* fields of AggArgs)
//   decide_dense             (no route: group-count estimate, code range, dense or not)
//   run_small_range_scan     dense_scan:*      the direct-addressed LDS scan
//   run_partitioned_paths    dense:two_values, hash_partitions:* (the dense ring scatter notes its routes in vnm_agg_routes.inc)
//   run_general_scan         scan:*            the LDS hash scans and the HBM table
//
// Return codes, here and in the route functions of vnm_agg_routes.inc / _multikey / _fxn that the stages call:
//   0              done: the batch is aggregated (or, decide_dense: decided)
//   1              error (set_error has the text)
//   VNM_RC_NA      not applicable: nothing of the batch is aggregated by this stage, the next one takes it
//   VNM_RC_MORE    more groups than hinted (a partition overflowed): estimate and partition again
//   VNM_RC_SINGLY  the waiting batches of a stream (h->segs_active), or a nullable key set aside (h->kn_valid), would have to
//                  take a path whose kernels read ONE batch of plain keys: nothing has been aggregated, the caller sends the
//                  batches one by one (flush_queue) or takes the packed route (try_nullable_key_dense)
constexpr int VNM_RC_NA = 2;
constexpr int VNM_RC_MORE = 3;
constexpr int VNM_RC_SINGLY = 77;

// does the handle hold stream segments or a nullable key that `what` cannot take?  (-> return VNM_RC_SINGLY)
static bool one_batch_only(const vnm_agg* h, const char* what) {
    if (!h->segs_active && !h->kn_valid) return false;
    if (env_on("VNM_AGG_TRACE")) fprintf(stderr, "[agg] %s: not this way (%s)\n", h->kn_valid ? "nullable key through the dense path" : "stream segments", what);
    return true;
}

// ---- column predicates: "a plain 8-byte column" in the strengths the routes ask for ----------------------------------------------
// an 8-byte element at an even Arrow offset (16-byte pairs); says nothing about NULLs.  (type_width is 8 for every type it does not know)
static inline bool even8(const vnm_dcol& c) { return type_width(c.type) == 8 && (c.offset & 1) == 0; }
// ... without a validity bitmap: what the kernels of the hot shape read as a KEY column
static inline bool plain8(const vnm_dcol& c) { return even8(c) && !c.validity; }
// ... whose values pointer is 16-byte aligned as well: what the stream segments and agg_hotn_kernel load in pairs
static inline bool aligned16(const vnm_dcol& c) { return ((uintptr_t)c.values & 15) == 0; }
static inline bool plain8_aligned(const vnm_dcol& c) { return plain8(c) && aligned16(c); }
// float64 / int64 / uint64: what the register kernels interpret as an INPUT column
static inline bool is_8byte_numeric(int type) { return type == VNM_F64 || type == VNM_I64 || type == VNM_U64; }
static inline bool even8_numeric(const vnm_dcol& c) { return is_8byte_numeric(c.type) && (c.offset & 1) == 0; }
static inline bool plain8_numeric(const vnm_dcol& c) { return even8_numeric(c) && !c.validity; }
// a float64 predicate column at an even offset compared as float64 (NULLs: the caller's business)
static inline bool even_f64_pred(const AggArgs& a) { return a.pred.type == VNM_F64 && (a.pred.offset & 1) == 0 && a.p.mode == CMP_F64; }
static inline bool plain_f64_pred(const AggArgs& a) { return even_f64_pred(a) && !a.pred.validity; }
// the very same values (the predicate reads the input column)
static inline bool same_values(const vnm_dcol& x, const vnm_dcol& y) { return x.values == y.values && x.offset == y.offset; }

// ---- thresholds read in more than one stage -------------------------------------------------------------------------------------
// rows a batch must bring before a sample of it is worth taking (estimate, code range, packing a single key)
static inline int64_t est_min_rows() { return env_i64("VNM_AGG_ESTIMATE_MIN_ROWS", 1 << 22); }
// groups from which the scan's hashed LDS table runs into flush storms: the partitioned paths take over
static inline int64_t part_min_groups(const AggPlan& plan) { return env_i64("VNM_AGG_PART_MIN_GROUPS", std::min<int64_t>(2400, (int64_t)lds_slots_for(plan) * 6 / 10)); }

// One call of the driver: the batch as the caller gave it.
struct Batch {
    vnm_agg* h;
    int64_t nrows;
    const vnm_dcol* keys;
    const vnm_dcol* inputs;
    const vnm_dcol* pred;
    void* stream;
    hipStream_t s;
    int64_t est_rows;   // rows the samplers may read through keys[0] (the first segment of a stream's waiting batches); thresholds take nrows
};

// What shape the batch has: which kernels could take it.  Filled by classify_batch; a later stage that legitimately changes a field
// says so where it does.
struct BatchShape {
    bool hot_scan;        // what agg_hot_kernel takes (any accumulator kind over at most TWO 8-byte columns without NULLs)
    bool hot;             // the subset {COUNT(*), COUNT, SUM, AVG} of a float64 column that part_agg_kernel is specialised for
    bool hot_prog;        // ... the PROGRAM, over a column that may be nullable (hot is false then)
    bool hot_two;         // hot_scan over two columns
    bool hot_vnull;       // ONE nullable input column: agg_hot_kernel<VNULL>
    bool hotn;            // three to six plain float64 columns under {COUNT(*), COUNT, SUM, AVG}: agg_hotn_kernel takes the scan
    bool part_ok;         // the hash-partitioned path has entries for this program
    bool narrow_generic;  // a generic program over (key, one plain 8-byte value or none): the dgen_* dense kernels take it too
    bool dense_vn;        // the dense path over ONE nullable 8-byte input column
    bool vn_fold;         // ... filtered by itself under the hot program: pass 1 drops the NULL rows
    bool dense_generic;   // a generic program through the dense kernels
    bool dense_two;       // TWO plain float64 input columns under {COUNT(*), COUNT, SUM, AVG} (dense_two_aggregate: two-value entries)
    bool dense_base;      // a dense shape, rows enough for a sample, not switched off
    int64_t part_min;
    int64_t est_min_rows;
};

// Entries the partitioned / dense paths could not place (heavy keys, keys outside the sampled range), aggregated by the general scan,
// and the scan's resume counters.  Everything goes back to the pool on every way out of the batch.
struct SpillState {
    ulonglong2* spill = nullptr;
    int64_t n_spill = 0;
    uint64_t* nspill = nullptr;   // dense path over a nullable value column: keys of the NULL-value rows it could not place
    int64_t n_nspill = 0;
    bool scan_no_pred = false;    // ... whose rows come back as columns with the predicate already applied
    unsigned int* progress = nullptr;
    PoolScope unzip;   // spilled wide entries as columns
    PoolSlotGuard<ulonglong2> spill_guard{&spill};
    PoolSlotGuard<uint64_t> nspill_guard{&nspill};
    PoolSlotGuard<unsigned int> progress_guard{&progress};

    // the scan runs over the spilled (key, value) entries only (predicate already applied)
    void scan_entries(AggArgs& a) const {
        a.ent = spill;
        a.nrows = n_spill;
        a.p.enabled = 0;
    }
    // the two spill lists of the nullable dense path -> key / value / validity columns for the scan
    int vn_spill_to_columns(AggArgs& a, hipStream_t s) {
        const int64_t n = n_spill + n_nspill;
        uint64_t* uk = (uint64_t*)unzip.take((size_t)n * 8);
        uint64_t* uv = (uint64_t*)unzip.take((size_t)n * 8);
        unsigned long long* ub = (unsigned long long*)unzip.take((size_t)((n + 63) / 64) * 8);
        if (!uk || !uv || !ub) return 1;
        const int ugrid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8);
        dense_vn_unzip_kernel<<<ugrid, 256, 0, s>>>(spill, n_spill, nspill, n_nspill, uk, uv, ub);
        VNM_HIP(hipGetLastError());
        a.keys[0].values = uk; a.keys[0].validity = nullptr; a.keys[0].offset = 0; a.keys[0].length = n;
        a.cols[0].values = uv; a.cols[0].validity = (const uint8_t*)ub; a.cols[0].offset = 0; a.cols[0].length = n;
        a.ent = nullptr;
        a.nrows = n;
        a.p.enabled = 0;
        scan_no_pred = true;
        return 0;
    }
    // spilled wide entries ([n][E] words of the wide scatter kernels) -> columns; the general scan takes them as a batch of its own
    int wide_spill_to_columns(AggArgs& a, hipStream_t s) {
        const int n_cols = a.plan.n_cols;
        const int E = 1 + n_cols + (a.part_vmask ? 1 : 0);
        UnzipArgs u{};
        u.ent = (const uint64_t*)spill; u.n = n_spill; u.E = E; u.nval = n_cols; u.has_vmask = a.part_vmask;
        u.key = (uint64_t*)unzip.take((size_t)n_spill * 8);
        bool ok = u.key != nullptr;
        for (int c = 0; c < n_cols && ok; c++) {
            u.widths[c] = type_width(a.cols[c].type);
            u.vals[c] = unzip.take((size_t)n_spill * u.widths[c]);
            u.valid[c] = a.cols[c].validity ? (unsigned long long*)unzip.take((size_t)((n_spill + 63) / 64) * 8) : nullptr;
            ok = u.vals[c] && (!a.cols[c].validity || u.valid[c]);
        }
        if (!ok) return 1;
        const int ugrid = (int)std::min<int64_t>((n_spill + 255) / 256, (int64_t)device_info().num_cus * 8);
        spill_unzip_kernel<<<ugrid, 256, 0, s>>>(u);
        VNM_HIP(hipGetLastError());
        a.keys[0].values = u.key; a.keys[0].validity = nullptr; a.keys[0].offset = 0; a.keys[0].length = n_spill;
        for (int c = 0; c < n_cols; c++) {
            a.cols[c].values = u.vals[c]; a.cols[c].validity = (const uint8_t*)u.valid[c]; a.cols[c].offset = 0; a.cols[c].length = n_spill;
        }
        a.nrows = n_spill;
        a.ntiles = (n_spill + AGG_TILE - 1) / AGG_TILE;
        a.p.enabled = 0;
        return 0;
    }
};

static bool queueable(const vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, bool* pred_is_v, bool* multi);
static int next_device_impl(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, void* stream);

// A NULLABLE single 8-byte key under the hot program: the dense path takes it as it is -- pass 1 reads the key's validity and
// sums the NULL-key rows up as the one group they are (single_numerical_hash_aggregate.cpp:24-32), everything after pass 1 never
// sees a NULL.  Before round 4 such a key was packed into one word first (key range + pack + unpack passes, the NULL code a
// heavy key of the inner operator, run + table merges at the end: 15.7 ms per 5e8 rows at G = 1e8 against 5.2 without NULLs).
// The attempt runs the driver again with the validity stripped from the key and kept aside; every path but the dense ring
// scatter declines (VNM_RC_SINGLY, before any side effect) and the batch takes the packed route (VNM_RC_NA here).
static int try_nullable_key_dense(const Batch& b) {
    vnm_agg* h = b.h;
    const vnm_dcol* keys = b.keys;
    if (!(!h->kn_valid && !h->kn_failed && !h->segs_active && h->single && h->plan.n_keys == 1 && !h->inner && keys && b.inputs && keys[0].validity &&
          even8(keys[0]) && b.nrows >= est_min_rows() && env_off("VNM_AGG_NO_DENSE_KN"))) return VNM_RC_NA;
    vnm_dcol k2 = keys[0];
    k2.validity = nullptr;
    bool piv = false, multi = false;
    if (!queueable(h, b.nrows, &k2, b.inputs, b.pred, &piv, &multi) || multi) return VNM_RC_NA;   // (the hot shape: one input column)
    h->kn_valid = keys[0].validity; h->kn_off = keys[0].offset;
    const int rc = next_device_impl(h, b.nrows, &k2, b.inputs, b.pred, b.stream);
    h->kn_valid = nullptr;
    if (rc != VNM_RC_SINGLY) return rc;
    h->kn_failed = true;
    return VNM_RC_NA;
}

// Multi-column keys: try the packed single-word form first (see PackParams).  A SINGLE key that the fast paths do
// not take as it is (int32 / int16 / float32 ..., NULLs, an odd Arrow offset) is packed the same way when the
// group count is large or unknown: one extra pass over the key column (12 B/row) buys the partitioned path instead
// of per-row HBM atomics (G = 1e6 int32 keys: 20x).
static int route_packed_keys(const Batch& b, bool key_plain) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    const vnm_dcol* keys = b.keys;
    hipStream_t s = b.s;
    const bool pack_single = h->single && h->plan.n_keys == 1 && !key_plain && (h->hint > 2400 || (h->hint == 0 && nrows >= est_min_rows()));
    if (!((!h->single && h->plan.n_keys >= 2) || pack_single || (h->single && h->inner))) return VNM_RC_NA;
    if (one_batch_only(h, "packed keys")) return VNM_RC_SINGLY;
    for (int j = 0; j < h->plan.n_keys; j++)
        if (keys[j].type != h->plan.key_types[j]) return set_error("vnm_agg_next_device: key %d changed type between batches", j);
    // ... only into an EMPTY handle: an operator that already holds groups of earlier batches in any form (HBM table, run,
    // deferred dense pass, stream table, the parts of a split program) keeps them -- a single key whose FIRST batch was plain
    // (no validity bitmap) and whose later batch brings NULL keys takes the general scan for that batch instead
    // (ADVICE r03: the inner operator's result used to replace, not join, what the handle held)
    const bool empty_handle = !h->have_table && !h->have_run && !h->pending && !h->scan_pending && h->parts.empty();
    if (!h->pack_tried && empty_handle && env_off("VNM_AGG_NO_PACK")) {
        h->pack_tried = true;
        int err = 0;
        if (plan_packing(h, keys, nrows, s, &err)) {
            const int kt = VNM_U64;
            h->inner = agg_create(VNM_SINGLE_NUMERICAL, 1, &kt, h->n_funcs, h->c_funcs, h->c_in_types, h->c_in_flags,
                                      h->c_has_ids ? h->c_in_col_ids : nullptr);
            if (!h->inner) return 1;
            h->inner->hint = h->hint;
            // a nullable key column: its NULL code may be a heavy key of the inner operator, whose estimator is not asked when
            // the caller gave a group count (the dense path then cuts pass 2 into more work items, see heavy_share)
            for (int j = 0; j < h->plan.n_keys; j++) if (keys[j].validity) h->inner->heavy_share = std::max(h->inner->heavy_share, 0.01);
        } else if (err) return err;
        else if (!h->single && env_off("VNM_AGG_NO_TUPLE")) {
            // too wide for one word even as per-column dictionary codes: tuple -> group id through a dictionary
            // (before: agg_wide_kernel, one HBM atomic per row and accumulator word)
            VNM_TRY(enter_tuple_mode(h, nrows, s));
        }
    }
    if (h->tuple_mode) { route_note("keys:tuple_dictionary", "%d key columns: tuple -> group id", h->plan.n_keys); return tuple_next(h, nrows, keys, b.inputs, b.pred, s); }
    if (!h->inner) return VNM_RC_NA;
    {
        int ndict = 0;
        for (int j = 0; j < h->plan.n_keys; j++) ndict += h->pack.dtab[j] != nullptr;
        route_note(ndict ? "keys:packed_with_dictionary_fields" : "keys:packed", "%d key columns in one 64-bit word (%d dictionary-coded)", h->plan.n_keys, ndict);
    }
    for (int j = 0; j < h->plan.n_keys; j++) { h->pack.cols[j] = keys[j]; if (keys[j].validity) h->pack_null_seen = true; }
    uint64_t* packed = (uint64_t*)pool_alloc((size_t)nrows * 8);
    unsigned long long* flag = (unsigned long long*)pool_alloc(64);
    if (!packed || !flag) return 1;
    VNM_HIP(hipMemsetAsync(flag, 0, 8, s));
    {
        KernelTimer timer("agg_pack_keys", s);
        int grid = (int)std::min<int64_t>((nrows + 255) / 256, (int64_t)device_info().num_cus * 8);
        key_pack_kernel<<<grid, 256, 0, s>>>(h->pack, nrows, packed, flag);
    }
    unsigned long long bad = 0;
    VNM_HIP(hipMemcpyAsync(&bad, flag, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    pool_free(flag);
    int rc = 0;
    if (!bad) {
        vnm_dcol pk{};
        pk.values = packed; pk.type = VNM_U64; pk.length = nrows;
        if (h->pred_set) rc = vnm_agg_set_predicate(h->inner, 1, h->pred_op, h->pred_is_float, h->pred_dval, h->pred_ival);
        if (!rc) { h->inner->child = true; h->inner->cur_seq = h->cur_seq; rc = vnm_agg_next_device(h->inner, nrows, &pk, b.inputs, b.pred, b.stream); }
        if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_error("aggregate: packed batch failed");
        pool_free(packed);
        if (!rc) h->rows_seen += nrows;
        return rc;
    }
    pool_free(packed);
    if (!h->single && env_off("VNM_AGG_NO_TUPLE")) {   // keys outside the packed ranges: on through the tuple dictionary
        VNM_TRY(packed_to_tuple(h, nrows, s));
        route_note("keys:tuple_dictionary", "a batch outgrew the packed ranges");
        return tuple_next(h, nrows, keys, b.inputs, b.pred, s);
    }
    VNM_TRY(demote_packed(h, s));  // (a packed SINGLE key: its own general path; or the dictionary switched off: the wide-key table)
    return VNM_RC_NA;
}

// the program cut into parts of `per` input columns each, and the batch into them
static int split_into_parts(const Batch& b, int per) {
    VNM_TRY(make_parts(b.h, per));
    if (b.h->segs_active) return VNM_RC_SINGLY;   // (the waiting batches of a stream: one by one into the parts, which record them)
    return next_parts(b.h, b.nrows, b.keys, b.inputs, b.pred, b.stream);
}

// More input columns than a partition entry carries (or as many, plus a validity word) and many groups: split the program.
static int route_split_program(const Batch& b, bool key_plain) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    const vnm_dcol* keys = b.keys;
    const vnm_dcol* inputs = b.inputs;
    hipStream_t s = b.s;
    if (!h->parts.empty()) {
        if (one_batch_only(h, "split program")) return VNM_RC_SINGLY;
        route_note("split_program:batch", "%zu parts", h->parts.size());
        return next_parts(h, nrows, keys, inputs, b.pred, b.stream);
    }
    if (!(!h->split_tried && key_plain && h->single && keys[0].type == h->plan.key_types[0] && !h->have_table && !h->have_run && !h->pending &&
          !h->expr_active && env_off("VNM_AGG_NO_SPLIT"))) return VNM_RC_NA;
    bool any_null = false, cols8 = true;
    for (int c = 0; c < h->plan.n_cols; c++) {
        const vnm_dcol& col = inputs[h->col_first_func[c]];
        any_null = any_null || col.validity != nullptr;
        cols8 = cols8 && is_8byte_numeric(col.type);
    }
    const bool est_ok = nrows >= est_min_rows();
    // (a) more columns than an entry carries; (b) two or more 8-byte columns over a key the dense paths take (round 4)
    const bool many = h->plan.n_cols + (any_null ? 1 : 0) > env_i64("VNM_AGG_SPLIT_MIN_COLS", 6);
    const bool by_column = h->plan.n_cols >= 2 && cols8 && !h->rank_aligned && (keys[0].type == VNM_I64 || keys[0].type == VNM_U64) && est_ok &&
                           env_off("VNM_AGG_NO_SPLIT_SMALL");
    if (!many && !by_column) return VNM_RC_NA;
    h->split_tried = true;
    if (h->hint == 0 && !h->estimated && est_ok && env_off("VNM_AGG_NO_ESTIMATE")) {
        int64_t est = 0;
        KernelTimer timer("agg_estimate", s);
        VNM_TRY(estimate_groups(h, keys[0], b.est_rows, &est, s));
        if (est) { h->hint = est; h->estimated = true; }
    }
    if (h->hint > part_min_groups(h->plan)) {
        if (by_column) {
            if (h->dense_state == 0) {
                KernelTimer timer("agg_estimate", s);
                VNM_TRY(plan_dense(h, keys[0], b.est_rows, s));
            }
            // A few thousand groups in a SMALL key range: too many for the scan's hashed LDS table of this many words (flush
            // storms), so the rows used to go through wide partition entries (C = 2 / 3 / 6 columns, G = 1000, 5e8 rows:
            // 7.9 / 12.3 / 23.6 ms).  One part per column instead: each is the direct-addressed 2^13-slot LDS scan (16 bytes per
            // row and column at the scan's rate: 3.3 / 4.9 / 9.8 ms incl. the join over a few thousand groups).
            if (h->dense_state == 2 && h->hint <= (1 << DP_TBITS_MAX)) {
                route_note("split_program:small_range_per_column", "%d columns, ~%lld groups in a range of <= 2^13 codes", h->plan.n_cols, (long long)h->hint);
                return split_into_parts(b, 1);
            }
            // MANY groups over a key the dense path takes, three or more columns: the dense path per column (16-byte entries,
            // LDS-resident final tables) -- or per PAIR of float64 columns under sums and counts (two-value entries) where
            // two scatter levels are needed anyway -- instead of wide entries through hash partitions; parts of the dense path
            // over one code map are joined by units of 64 codes (collapse_parts: no sorts, no random gathers).
            // 5e8 rows, 3 / 6 columns: G = 1e6 20.0 / 37.6 -> 13.9 / 26.8 ms, G = 1e8 30.1 / 360 -> 24.7 / 44.8.
            if (nrows >= env_i64("VNM_AGG_SPLIT_DENSE_MIN_ROWS", 1 << 24) && h->dense_state == 1 &&
                h->dense_span <= 32 * h->hint && h->dense_span <= env_i64("VNM_DENSE_SPAN_PER_ROW", 16) * nrows && env_off("VNM_AGG_NO_SPLIT_DENSE")) {
                bool sums = true;   // every function a sum / count of a plain float64 column: what the two-value entries carry
                for (int i = 0; i < h->n_funcs && sums; i++) {
                    const int f = h->c_funcs[i];
                    sums = f == VNM_COUNT_STAR || ((f == VNM_SUM || f == VNM_AVG || f == VNM_COUNT) && inputs[i].type == VNM_F64 && !inputs[i].validity);
                }
                // (the two-value entries have no deferred final pass and take no stream segments: every batch ends in a run that is
                // merged into the table -- 30 x 2^24 rows, three columns, G = 1e7: 107 ms against 17 for the same rows as one batch.
                // They are for BIG batches; a stream's batches go per column, whose parts record and defer like any one-column stream)
                const bool big = !h->segs_active && nrows >= env_i64("VNM_AGG_PAIRS_MIN_ROWS", (int64_t)1 << 27);
                const bool pairs = sums && big && h->hint >= env_i64("VNM_AGG_SPLIT_PAIRS_MIN_GROUPS", 4000000);
                // (TWO columns: the two-value entries themselves from ~1.5e6 groups on -- two scatter levels -- and one part per column
                // below: 5e8 rows, G = 1e4 / 1e5 / 5e5 / 1e6: 8.2 / 10.9 / 14.8 / 10.1 -> 7.3 / 7.8 / 8.1 / 8.7 ms; 2e6: 9.9 against 11.4)
                const bool split = h->plan.n_cols >= 3 || !sums || !big || (!pairs && h->hint <= env_i64("VNM_AGG_SPLIT_TWO_MAX_GROUPS", 1500000));
                // two or three float64 columns whose values are fixed-point words: ONE pass over the rows (vnm_agg_fxn.inc) before the
                // program is cut per column
                if (sums && h->plan.n_cols <= 3 && h->parts.empty()) {
                    const int frc = dense_fxn_aggregate(h, nrows, keys, inputs, b.pred, s);
                    if (frc == 1) return 1;
                    if (frc == 0) { h->rows_seen += nrows; return 0; }
                }
                if (split) {
                    route_note(pairs ? "split_program:dense_per_pair" : "split_program:dense_per_column", "%d columns, ~%lld groups over %lld codes, %lld rows", h->plan.n_cols, (long long)h->hint, (long long)h->dense_span, (long long)nrows);
                    return split_into_parts(b, pairs ? 2 : 1);
                }
            }
        }
        if (many) {
            route_note("split_program:many_columns", "%d columns (+%d validity word), ~%lld groups", h->plan.n_cols, any_null ? 1 : 0, (long long)h->hint);
            return split_into_parts(b, (int)env_i64("VNM_AGG_SPLIT_COLS", any_null ? 5 : 6));
        }
    } else if (many && cols8 && !any_null && h->hint > 0 && h->hint <= env_i64("VNM_AGG_SPLIT_FEW_MAX_GROUPS", 256) && !h->rank_aligned &&
               env_off("VNM_AGG_NO_SPLIT_FEW")) {
        // FEW groups under more than six plain 8-byte columns: parts of up to six columns, each through agg_hotn_kernel, instead of the
        // interpreted scan over all of them (5e8 rows, G = 7: 7 / 8 / 10 columns 11.5 / 12.9 / 15.7 ms at 2.8 TB/s)
        route_note("split_program:few_groups_many_columns", "%d columns, ~%lld groups", h->plan.n_cols, (long long)h->hint);
        return split_into_parts(b, 6);
    }
    return VNM_RC_NA;
}

// the kernels' view of the batch: plan, columns, predicate, tiles of the generic scan
static int fill_agg_args(const Batch& b, AggArgs& a) {
    const vnm_agg* h = b.h;
    a.plan = h->plan;
    for (int j = 0; j < h->plan.n_keys; j++) {
        a.keys[j] = b.keys[j];
        if (b.keys[j].type != h->plan.key_types[j]) return set_error("vnm_agg_next_device: key %d changed type between batches", j);
    }
    for (int c = 0; c < h->plan.n_cols; c++) a.cols[c] = b.inputs[h->col_first_func[c]];
    if (h->pred_set) {
        a.pred = *b.pred;
        a.p = make_predicate(b.pred->type, b.pred->validity != nullptr, h->pred_op, h->pred_is_float, h->pred_dval, h->pred_ival);
    }
    a.nrows = b.nrows;
    a.ntiles = (b.nrows + AGG_TILE - 1) / AGG_TILE;
    a.debug = (int)env_i64("VNM_AGG_DEBUG", 0);
    if (h->expr_active) { a.has_expr = 1; a.expr = h->expr_dev; }
    return 0;
}

// launch of a kernel that takes AggArgs and `lds` bytes of dynamic LDS (more than the default limit: the attribute first)
template <class K>
static int launch_lds(K kernel, int grid, int block, size_t lds, hipStream_t s, const AggArgs& a) {
    VNM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, block, lds, s>>>(a);
    return 0;
}

// pm, the predicate form of the register kernels: 0 none, 1 the float64 input column itself, 2 a column of its own
template <int VT>
static void launch_onegroup_hot(int pm, int grid, hipStream_t s, const AggArgs& a) {
    if (pm == 0) agg_onegroup_hot_kernel<VT, 0><<<grid, OG_BLOCK, 0, s>>>(a);
    else if (pm == 1) agg_onegroup_hot_kernel<VT, 1><<<grid, OG_BLOCK, 0, s>>>(a);
    else agg_onegroup_hot_kernel<VT, 2><<<grid, OG_BLOCK, 0, s>>>(a);
}

// No GROUP BY: the one-group kernels.
static int run_onegroup(const Batch& b, AggArgs& a) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    hipStream_t s = b.s;
    const int cus = device_info().num_cus;
    if (one_batch_only(h, "no GROUP BY")) return VNM_RC_SINGLY;
    VNM_TRY(ensure_table(h, nrows, s));
    a.g = h->g;
    int grid = cus * 8;
    int64_t need = (nrows + OG_BLOCK - 1) / OG_BLOCK;
    if (grid > need) grid = (int)need;
    KernelTimer timer("agg_scan", s);
    // every kind at most once over at most one plain 8-byte column, float64 predicate or none: the register kernel
    bool og_hot = h->plan.n_cols <= 1 && env_off("VNM_AGG_NO_HOT");
    int vt = -1;
    if (og_hot && h->plan.n_cols == 1) {
        og_hot = plain8_numeric(a.cols[0]);
        vt = a.cols[0].type;
    }
    for (int k = 0; k < 9; k++) a.hot_w[k] = -1;
    for (int o = 0; o < h->plan.n_ops && og_hot; o++) {
        const AccOp& op = h->plan.ops[o];
        if (op.kind < 0 || op.kind > A_MAX || a.hot_w[op.kind] >= 0 || (op.kind != A_COUNT_ROWS && vt < 0)) og_hot = false;
        else a.hot_w[op.kind] = op.word;
    }
    int pm = 0;
    if (og_hot && h->pred_set) {
        og_hot = plain_f64_pred(a);
        pm = og_hot && vt == VNM_F64 && same_values(a.pred, a.cols[0]) ? 1 : 2;
    }
    route_note(og_hot ? "onegroup:register_scan" : "onegroup:lds_scan", "%lld rows, %d columns, %d words", (long long)nrows, h->plan.n_cols, h->plan.n_words);
    if (og_hot) {
        const int g2 = (int)std::min<int64_t>((int64_t)cus * 8, std::max<int64_t>(1, (nrows / 2 + OG_BLOCK - 1) / OG_BLOCK));
        switch (vt) {
            case VNM_F64: launch_onegroup_hot<VNM_F64>(pm, g2, s, a); break;
            case VNM_I64: launch_onegroup_hot<VNM_I64>(pm, g2, s, a); break;
            case VNM_U64: launch_onegroup_hot<VNM_U64>(pm, g2, s, a); break;
            default: launch_onegroup_hot<-1>(pm, g2, s, a); break;
        }
    } else {
        agg_onegroup_kernel<<<grid, OG_BLOCK, (size_t)h->plan.n_words * OG_BLOCK * 8, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    h->rows_seen += nrows;
    return 0;
}

// hot shape: one 8-byte key, every function in {COUNT(*), COUNT, SUM, AVG} over ONE float64 column,
// float64 predicate column (or none), no validity bitmaps, even offsets (16-byte aligned pairs).
// Fills hot_scan / hot / hot_prog / hot_two / hot_vnull and the hot_* fields of AggArgs.
static void classify_hot(const vnm_agg* h, const vnm_dcol* keys, AggArgs& a, BatchShape& sh) {
    sh.hot_scan = h->single && h->plan.n_cols <= 2 && plain8(keys[0]) && env_off("VNM_AGG_NO_HOT");
    a.hot_has_val = h->plan.n_cols >= 1;
    a.hot_vtype = a.hot_vtype2 = VNM_U64;
    sh.hot_vnull = false;
    for (int c = 0; c < h->plan.n_cols && sh.hot_scan; c++) {
        const vnm_dcol& col = a.cols[c];
        if (col.validity && h->plan.n_cols == 1) sh.hot_vnull = true;
        sh.hot_scan = even8_numeric(col) && (!col.validity || sh.hot_vnull);
        (c == 0 ? a.hot_vtype : a.hot_vtype2) = col.type;
    }
    sh.hot_two = sh.hot_scan && h->plan.n_cols == 2;
    a.hot_w_rows = a.hot_w_valid = a.hot_w_sum = -1;
    a.hot_comp = 0;
    for (int w = 0; w < h->plan.n_words; w++) if (h->plan.merge[w] == M_ADD_F64C) a.hot_comp = 1;
    for (int k = 0; k < 9; k++) a.hot_w[k] = a.hot_w2[k] = -1;
    bool hot = sh.hot_scan && h->plan.n_cols == 1 && a.hot_vtype == VNM_F64;   // (a nullable column: hot_prog below)
    if (sh.hot_scan) {
        for (int o = 0; o < h->plan.n_ops; o++) {
            const AccOp& op = h->plan.ops[o];
            int* hw = op.col == 1 ? a.hot_w2 : a.hot_w;
            const int vt = op.col == 1 ? a.hot_vtype2 : a.hot_vtype;
            if (op.kind < 0 || op.kind > A_MAX || hw[op.kind] >= 0) { sh.hot_scan = false; break; }  // one word per kind and column
            if (op.kind == A_SUM_F64 && vt != VNM_F64) { sh.hot_scan = false; break; }
            hw[op.kind] = op.word;
            if (op.col == 1) { hot = false; continue; }
            if (op.kind == A_COUNT_ROWS) a.hot_w_rows = op.word;
            else if (op.kind == A_COUNT_VALID) a.hot_w_valid = op.word;
            else if (op.kind == A_SUM_F64) a.hot_w_sum = op.word;
            else hot = false;
        }
    }
    a.hot_wpack = a.hot_wpack2 = ~0ULL;
    for (int k = A_COUNT_VALID; k <= A_MAX; k++) {
        if (a.hot_w[k] >= 0) a.hot_wpack = (a.hot_wpack & ~(63ULL << (6 * k))) | ((unsigned long long)a.hot_w[k] << (6 * k));
        if (a.hot_w2[k] >= 0) a.hot_wpack2 = (a.hot_wpack2 & ~(63ULL << (6 * k))) | ((unsigned long long)a.hot_w2[k] << (6 * k));
    }
    hot = hot && sh.hot_scan;
    if (sh.hot_scan && h->pred_set) {
        a.hot_pred_is_v = a.hot_has_val && a.hot_vtype == VNM_F64 && same_values(a.pred, a.cols[0]);
        // a nullable predicate column only as the (nullable) input column itself
        sh.hot_scan = even_f64_pred(a) && (!a.pred.validity || (sh.hot_vnull && a.hot_pred_is_v));
        hot = hot && sh.hot_scan;
    }
    // the hot PROGRAM over a nullable column filtered by itself (`WHERE v > x`: a NULL fails the filter): the dense path drops the
    // NULL rows in pass 1 and everything after it is the hot shape (vn_fold); every other kernel of the hot shape reads no bitmap
    sh.hot_prog = hot;
    sh.hot = hot && !sh.hot_vnull;
}

// three to six plain float64 columns under {COUNT(*), COUNT, SUM, AVG}: agg_hotn_kernel takes the scan.  Fills hotn and the hn_* fields.
static void classify_hotn(const vnm_agg* h, const vnm_dcol* keys, AggArgs& a, BatchShape& sh) {
    bool hotn = !sh.hot_scan && h->single && h->plan.n_cols >= 3 && h->plan.n_cols <= 6 && plain8(keys[0]) && !a.has_expr &&
                env_off("VNM_AGG_NO_HOTN") && env_off("VNM_AGG_NO_HOT");
    int w_rows = -1, w_cnt[6] = {-1, -1, -1, -1, -1, -1};
    for (int c = 0; c < 6; c++) a.hn_w_sum[c] = -1;
    a.hn_any_int = a.hn_any_mm = 0;
    for (int c = 0; c < 6; c++) { a.hn_ctype[c] = VNM_F64; a.hn_wmm[c][0] = a.hn_wmm[c][1] = -1; for (int k = 0; k < 4; k++) a.hn_iw[c][k] = -1; }
    for (int c = 0; c < h->plan.n_cols && hotn; c++) {
        const vnm_dcol& col = a.cols[c];
        hotn = plain8_numeric(col) && aligned16(col);
        a.hn_ctype[c] = col.type;
        if (col.type != VNM_F64) a.hn_any_int = 1;   // (not the PLAIN instantiation: its values are float64 bit patterns)
    }
    for (int o = 0; o < h->plan.n_ops && hotn; o++) {
        const AccOp& op = h->plan.ops[o];
        if (op.kind == A_COUNT_ROWS && w_rows < 0) w_rows = op.word;
        else if (op.kind == A_COUNT_VALID && w_cnt[op.col] < 0) w_cnt[op.col] = op.word;
        else if (op.kind == A_SUM_F64 && a.hn_w_sum[op.col] < 0) a.hn_w_sum[op.col] = op.word;
        else if (op.kind >= A_SUM_I64 && op.kind <= A_SUM_HI32U && a.hn_ctype[op.col] != VNM_F64 && a.hn_iw[op.col][op.kind - A_SUM_I64] < 0) {
            a.hn_iw[op.col][op.kind - A_SUM_I64] = op.word;
            a.hn_any_int = 1;
        } else if ((op.kind == A_MIN || op.kind == A_MAX) && a.hn_wmm[op.col][op.kind - A_MIN] < 0) {
            a.hn_wmm[op.col][op.kind - A_MIN] = op.word;
            a.hn_any_mm = 1;
        } else hotn = false;
    }
    a.hn_w_base = w_rows;
    a.hn_n_copy = 0;
    for (int c = 0; c < h->plan.n_cols && hotn; c++) {
        if (w_cnt[c] < 0) continue;
        if (a.hn_w_base < 0) a.hn_w_base = w_cnt[c];
        else a.hn_w_copy[a.hn_n_copy++] = w_cnt[c];
    }
    hotn = hotn && a.hn_w_base >= 0 && aligned16(keys[0]);
    a.hn_pred_col = -1;
    if (hotn && h->pred_set) {
        hotn = plain_f64_pred(a) && aligned16(a.pred);
        for (int c = 0; c < h->plan.n_cols && hotn; c++)
            if (same_values(a.pred, a.cols[c])) a.hn_pred_col = c;
    }
    sh.hotn = hotn;
}

// The partitioned path also takes ANY accumulator program over at most one 8-byte input column: its entries
// carry (key, raw value bits) and only the final pass interprets them.  Fills part_ok / narrow_generic and the part_* fields.
static void classify_partitions(const vnm_agg* h, const vnm_dcol* keys, AggArgs& a, BatchShape& sh) {
    sh.part_ok = sh.hot;
    sh.narrow_generic = false;
    if (!(!sh.hot && h->single && h->plan.n_cols <= 6 && plain8(keys[0]) && env_off("VNM_AGG_NO_PART_GENERIC") &&
          (size_t)(256 + 1) * 8 * (1 + h->plan.n_words) <= 150 * 1024)) return;   // (the final pass shrinks its LDS table to fit)
    // narrow entries (key, value): at most one 8-byte input column without NULLs, float64 predicate column
    bool narrow = h->plan.n_cols <= 1;
    bool any_null = false;
    for (int c = 0; c < h->plan.n_cols; c++) {
        const vnm_dcol& col = a.cols[c];
        a.part_vtypes[c] = col.type;
        if (col.validity) any_null = true;
        if (!plain8_numeric(col)) narrow = false;
    }
    if (h->plan.n_cols >= 1) a.part_vtype = a.cols[0].type;
    if (narrow && h->pred_set) {
        narrow = plain_f64_pred(a);
        a.hot_pred_is_v = h->plan.n_cols == 1 && same_values(a.pred, a.cols[0]);   // (overwrites classify_hot's for generic narrow programs)
    }
    // wide entries take the rest: several columns, NULLs, narrow types, any predicate -- while key + values
    // (+ validity word) fit seven words
    const bool wide = !narrow && h->plan.n_cols >= 1 && h->plan.n_cols + (any_null ? 1 : 0) <= 6 && env_off("VNM_AGG_NO_PART_WIDE");
    sh.part_ok = narrow || wide;
    sh.narrow_generic = narrow;
    a.part_generic = sh.part_ok;
    a.part_wide = wide;
    a.part_vmask = wide && any_null;
    // no input column at all (COUNT(*) only): the entries are the keys alone -- 8 bytes instead of 16 through every
    // pass, via the wide kernels with E = 1.  Those cannot spill heavy keys; if a region overflows the operator goes
    // back to (key, unused word) entries with the spill buffer for good.
    if (narrow && h->plan.n_cols == 0 && !h->key_only_failed && env_off("VNM_AGG_NO_KEY_ONLY")) a.part_wide = 1;
}

// Which kernels could take this batch.  Reads the handle and the switches; no HIP call, nothing written to the handle.
static BatchShape classify_batch(const vnm_agg* h, const vnm_dcol* keys, AggArgs& a) {
    BatchShape sh{};
    a.lds_slots = lds_slots_for(h->plan);
    sh.part_min = part_min_groups(h->plan);
    sh.est_min_rows = est_min_rows();
    classify_hot(h, keys, a, sh);
    classify_hotn(h, keys, a, sh);
    classify_partitions(h, keys, a, sh);
    // Dense-key path (vnm_agg_dense.inc): the north-star shape over an int64 / uint64 key whose (sampled) range fits 29
    // bits.  (generic programs: only where the spilled entries -- keys outside the sampled range -- have a kernel to go to)
    // ... and ONE nullable 8-byte input column (hot_vnull; the predicate column, if any, without NULLs or that column itself): the
    // entries carry a NULL flag next to the code (vnm_agg_dense.inc, VN kernels); what the dense pass cannot place comes back as
    // two lists (entries, keys of NULL-value rows) and goes through the scan as columns
    sh.dense_vn = !sh.hot && sh.hot_scan && sh.hot_vnull && !sh.hot_two && !a.has_expr && sh.part_ok && h->plan.n_cols == 1 &&
                  env_off("VNM_AGG_NO_DENSE_VN");
    sh.vn_fold = sh.dense_vn && sh.hot_prog && h->pred_set && a.hot_pred_is_v && env_off("VNM_AGG_NO_VN_FOLD");
    sh.dense_generic = ((!sh.hot && sh.narrow_generic && sh.hot_scan && !sh.hot_two && !sh.hot_vnull && !a.has_expr) || sh.dense_vn) &&
                       env_off("VNM_AGG_NO_DENSE_GENERIC") && env_off("VNM_AGG_NO_SPILL");
    // ... and TWO plain float64 input columns under {COUNT(*), COUNT, SUM, AVG} (dense_two_aggregate: two-value entries)
    sh.dense_two = sh.hot_scan && sh.hot_two && !a.has_expr && !h->rank_aligned && !h->segs_active && !h->kn_valid && a.hot_vtype == VNM_F64 && a.hot_vtype2 == VNM_F64 &&
                   env_off("VNM_AGG_NO_DENSE_TWO");
    for (int o = 0; o < h->plan.n_ops && sh.dense_two; o++) {
        const int k = h->plan.ops[o].kind;
        sh.dense_two = k == A_COUNT_ROWS || k == A_COUNT_VALID || k == A_SUM_F64;
    }
    sh.dense_base = (sh.hot || sh.dense_generic || sh.dense_two) && sh.part_ok && a.nrows >= sh.est_min_rows && env_off("VNM_AGG_NO_DENSE");
    return sh;
}

// A batch must bring enough rows for its code range (a final pass over 2^b slots for a handful of rows is all overhead) -- unless a
// deferred pass over that very range is waiting anyway: a short batch of a stream then simply joins it (round 4; before, it took
// two hash levels -- and, with a nullable key, the general scan).  Evaluated where it is used: plan_dense may only just have set the range.
// (16 codes per row of the batch: a 2^24-row batch of a stream opens -- and later batches join -- a deferred pass over 2^27 codes; with 4
// such a stream took the hash partitions batch by batch: 59 x 2^24 rows, G = 1e8, synchronous next(): 132.6 -> 21.6 ms; a single
// 2^24-row batch over that range: 1.66 -> 1.10 ms)
static bool span_fits(const vnm_agg* h, int64_t nrows) {
    return h->dense_span <= env_i64("VNM_DENSE_SPAN_PER_ROW", 16) * nrows ||
           (h->pending != nullptr && h->dense_state == 1 && memcmp(&h->pending->df.map, &h->dmap, sizeof(DenseMap)) == 0);
}

// No hint from the caller: estimate the group count once from a sample of the first large batch -- and decide whether the batch goes
// dense.  The dense path needs to know that G is LARGE, not how large: when the small sample of the estimator cannot settle G, its
// lower bound is enough (span <= 32 G: the direct-addressed slots are reasonably filled) and the HyperLogLog pass
// (0.85 ms) is skipped; the hash-partitioned path still estimates properly if the dense attempt fails.
static int decide_dense(const Batch& b, const BatchShape& sh, bool* dense_shape_out, bool* dense_go_out) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    const vnm_dcol* keys = b.keys;
    hipStream_t s = b.s;
    bool dense_shape = sh.dense_base && (!h->rank_aligned || h->range_given);   // rank-aligned: only with a code range all ranks agreed on
    bool dense_go = false;
    // a stream that went dense on the sample's lower bound (no group count exists) and now brings a batch too short for the
    // code range: this batch and the rest need a number after all (without one they took the LDS scan and its flush storms)
    if (h->dense_by_bound && h->hint == 0 && !(dense_shape && h->dense_state == 1 && span_fits(h, nrows))) {
        h->estimated = false;
        h->dense_by_bound = false;
    }
    if (sh.part_ok && h->hint == 0 && !h->estimated && nrows >= sh.est_min_rows && env_off("VNM_AGG_NO_ESTIMATE")) {
        int64_t est = 0, dense_lb = 0;
        KernelTimer timer("agg_estimate", s);
        // the small sample first: a conclusive (small) group count needs neither the key range nor HyperLogLog
        VNM_TRY(estimate_groups(h, keys[0], b.est_rows, &est, s, dense_shape ? &dense_lb : nullptr));
        if (est == 0) {
            if (h->dense_state == 0) VNM_TRY(plan_dense(h, keys[0], b.est_rows, s));
            // (... or, under skew -- duplicates in the sample pull the bound down -- when the bound at least rules out the LDS scans and the
            // rows outnumber the code range four to one: the passes over the rows dominate whatever G is, the hash partitions would
            // cost the same, and the HyperLogLog pass (0.8 ms) buys nothing)
            const bool rows_dominate = dense_lb >= env_i64("VNM_DENSE_SKEW_MIN_LB", 100000) && h->dense_span * 4 <= nrows;
            if (h->dense_state == 1 && (h->dense_span <= 32 * dense_lb || rows_dominate) && span_fits(h, nrows)) dense_go = true;
            else VNM_TRY(estimate_groups(h, keys[0], b.est_rows, &est, s));   // too sparse (or not a code-able key): full estimate
        }
        if (est) { h->hint = est; h->estimated = true; }
        else if (dense_go) { h->estimated = true; h->dense_by_bound = true; }   // later batches of the stream: no sample again
    }
    if (dense_shape && !dense_go && h->dense_by_bound && h->hint == 0 && h->dense_state == 1 && span_fits(h, nrows)) dense_go = true;
    // rank-aligned operators (multi-GPU) keep hash partitions so that every rank cuts its result the same way -- which only
    // the partition-aligned exchange of LARGE results needs; small results travel by one all-gather and are merged by key
    // (widened AFTER the estimate: the hint may only just exist)
    if (sh.dense_base && h->rank_aligned && h->hint > 0 && h->hint <= env_i64("VNM_ALIGNED_DENSE_MAX", 1 << 19)) dense_shape = true;
    if (dense_shape && !dense_go && h->hint > sh.part_min) {
        if (h->dense_state == 0) {
            KernelTimer timer("agg_estimate", s);
            VNM_TRY(plan_dense(h, keys[0], b.est_rows, s));
        }
        if (h->dense_state == 1 && h->dense_span <= 32 * h->hint && span_fits(h, nrows)) dense_go = true;
    }
    *dense_shape_out = dense_shape;
    *dense_go_out = dense_go;
    return 0;
}

// A few hundred to a few thousand groups in a small key range: the direct-addressed LDS scan (vnm_agg_dense.inc).
// VNM_RC_NA: on to the next stage -- with *scan_spill set when only the entries this stage spilled are left to aggregate.
static int run_small_range_scan(const Batch& b, AggArgs& a, const BatchShape& sh, bool dense_shape, bool dense_go, SpillState& sp, bool* scan_spill) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    hipStream_t s = b.s;
    bool dscan_stream = false;   // the batch went into the stream table (h->scan_pending)
    if (dense_shape && !dense_go && !sh.dense_two && h->hint >= env_i64("VNM_DSCAN_MIN_GROUPS", 128) && h->hint <= (1 << DP_TBITS_MAX) &&
        env_off("VNM_AGG_NO_DSCAN")) {
        if (h->dense_state == 0) {
            KernelTimer timer("agg_estimate", s);
            VNM_TRY(plan_dense(h, b.keys[0], b.est_rows, s));
        }
        if (h->dense_state == 2) {
            // (the hot program's scan takes segments)
            if ((h->kn_valid || (h->segs_active && (sh.dense_generic || a.has_expr))) && one_batch_only(h, "small-range LDS scan")) return VNM_RC_SINGLY;
            if (h->pending) VNM_TRY(complete_pending(h, s));   // (this path makes a run of its own)
            if (h->have_run) VNM_TRY(merge_run_into_table(h, s));
            if (sh.dense_generic && h->scan_pending) VNM_TRY(flush_scan_pending(h, s));
            route_note(sh.dense_generic ? "dense_scan:generic" : "dense_scan:hot", "~%lld groups in a sampled range of %lld codes (<= 2^13): direct-addressed LDS table, no scatter", (long long)h->hint, (long long)h->dense_span);
            int prc = sh.dense_generic ? dense_scan_generic(h, a, nrows, s, &sp.spill, &sp.n_spill, &sp.nspill, &sp.n_nspill) : dense_scan_stream(h, a, nrows, s, &sp.spill, &sp.n_spill);
            dscan_stream = prc == 0 && !sh.dense_generic;
            // a generic program whose table for this range does not fit LDS: the same 2^13 codes through one scatter level
            // (four partitions of 2^11 slots, split final pass) instead
            if (prc == VNM_RC_NA && sh.dense_generic && h->dense_state == 2) prc = dense_partitioned_aggregate(h, a, nrows, s, &sp.spill, &sp.n_spill, true, &sp.nspill, &sp.n_nspill);
            if (prc == 1) return 1;
            if (prc == 0 && !sp.spill && !sp.nspill) { h->rows_seen += nrows; return 0; }
            if (prc == 0 && sh.dense_vn) {
                VNM_TRY(sp.vn_spill_to_columns(a, s));
                *scan_spill = true;
            } else if (prc == 0) {
                sp.scan_entries(a);
                *scan_spill = true;
            }
        }
    }
    // (a batch that went another way than the stream table of the small-range scan: that table becomes a run first)
    if (h->scan_pending && !dscan_stream) VNM_TRY(flush_scan_pending(h, s));
    return VNM_RC_NA;
}

// Many groups: the dense and the radix-partitioned paths (no per-row HBM atomics) ... from the point where the groups stop fitting
// the LDS table of the scan kernel (flush storms otherwise: MIN+MAX with 2000 groups and a 2048-slot table ran at 38 ms).
// VNM_RC_NA: the general scan takes the batch, or what these paths spilled of it.
static int run_partitioned_paths(const Batch& b, AggArgs& a, BatchShape& sh, bool dense_go, SpillState& sp) {
    vnm_agg* h = b.h;
    const int64_t nrows = b.nrows;
    hipStream_t s = b.s;
    if (!(sh.part_ok && (h->hint > sh.part_min || dense_go) && env_off("VNM_AGG_NO_PART"))) return VNM_RC_NA;
    if (h->have_run) VNM_TRY(merge_run_into_table(h, s));
    // wide entries (any program over up to six columns, key-only entries) spill as whole entries; they come back as
    // plain columns for the general scan (spill_unzip_kernel)
    const bool spill_wide = a.part_wide && h->single && !a.has_expr && env_off("VNM_AGG_NO_SPILL") && env_off("VNM_AGG_NO_WIDE_SPILL");
    const bool can_spill = (sh.hot_scan && !sh.hot_two && !sh.hot_vnull && env_off("VNM_AGG_NO_SPILL")) || spill_wide;
    int prc = VNM_RC_NA;
    bool vn_spill = false;        // the spill lists of the nullable dense path (entries + keys of NULL-value rows)
    bool spill_is_wide = false;   // the spill holds [n][E]-word entries of the wide scatter kernels (not the (key, value) pairs of the hot / dense paths)
    auto run_partitioned = [&]() {
        if (h->segs_active || h->kn_valid) return VNM_RC_SINGLY;   // (its kernels read one batch of plain keys)
        if (h->pending && complete_pending(h, s)) return 1;     // (the hash-partitioned path makes a run of its own)
        if (h->have_run && merge_run_into_table(h, s)) return 1;
        route_note(a.part_wide ? "hash_partitions:wide_entries" : (a.part_generic ? "hash_partitions:generic" : "hash_partitions:hot"), "~%lld groups > %lld (the scan's LDS table), dense path %s", (long long)h->hint, (long long)sh.part_min,
                   h->dense_state == 1 ? "declined or failed" : "not applicable");
        const int r = partitioned_aggregate(h, a, nrows, s, can_spill ? &sp.spill : nullptr, can_spill ? &sp.n_spill : nullptr);
        spill_is_wide = r == 0 && sp.spill != nullptr && a.part_wide != 0;
        return r;
    };
    // the dense attempt failed before G was ever estimated: the hash partitions need a number
    auto estimate_after_dense = [&]() {
        int64_t est = 0;
        VNM_TRY(estimate_groups(h, b.keys[0], b.est_rows, &est, s));
        h->hint = est;
        h->estimated = true;
        return 0;
    };
    if (dense_go && sh.dense_two && (h->hint > sh.part_min || h->hint == 0)) {
        if (h->pending && complete_pending(h, s)) return 1;     // (this path makes a run of its own)
        if (h->have_run && merge_run_into_table(h, s)) return 1;
        route_note("dense:two_values", "%lld codes, ~%lld groups, %lld rows: (value, value, code) entries", (long long)h->dense_span, (long long)h->hint, (long long)nrows);
        prc = dense_two_aggregate(h, a, nrows, s);
        if (prc == VNM_RC_NA) h->dense_state = -1;                      // (a key outside the range, a full region, a range it does not take: not again)
        if (prc == VNM_RC_NA && h->hint == 0) VNM_TRY(estimate_after_dense());
    } else if (dense_go && (h->hint > sh.part_min || h->hint == 0)) {
        prc = dense_partitioned_aggregate(h, a, nrows, s, &sp.spill, &sp.n_spill, sh.dense_generic && !sh.vn_fold, &sp.nspill, &sp.n_nspill, sh.vn_fold);
        vn_spill = prc == 0 && sh.dense_vn && (sp.spill || sp.nspill);
        if (prc == VNM_RC_NA && h->hint == 0) VNM_TRY(estimate_after_dense());
    }
    if (prc == VNM_RC_NA && h->hint > sh.part_min) prc = run_partitioned();
    if (prc == VNM_RC_NA && a.part_wide && h->plan.n_cols == 0) {  // key-only entries and a region overflowed: see classify_partitions
        h->key_only_failed = true;
        a.part_wide = 0;
        prc = run_partitioned();
    }
    // more groups than hinted (a partition overflowed its LDS table, or the dense output its allocation): estimate
    // the group count from the keys (< 1 ms) and partition again (~12 ms per attempt) before giving in to the HBM
    // table (~300 ms per 1e9 rows)
    for (int retry = 0; prc == VNM_RC_MORE && retry < 2; retry++) {
        int64_t est = 0;
        if (retry == 0 && !h->estimated) {
            VNM_TRY(estimate_groups(h, b.keys[0], b.est_rows, &est, s));
            h->estimated = true;
        }
        h->hint = std::min<int64_t>(std::max<int64_t>(h->hint * 4, est + est / 4), (int64_t)1600 * env_i64("VNM_AGG_PART_L1_MAX", 256) * 512);
        prc = run_partitioned();
    }
    if (prc == 0 && !sp.spill && !sp.nspill) { h->rows_seen += nrows; return 0; }
    if (prc == 1) return 1;
    if (prc == VNM_RC_SINGLY && one_batch_only(h, "hash partitions")) return VNM_RC_SINGLY;
    if (prc == 0 && vn_spill) {
        VNM_TRY(sp.vn_spill_to_columns(a, s));
    } else if (prc == 0 && spill_is_wide) {
        VNM_TRY(sp.wide_spill_to_columns(a, s));
        sh.hot_scan = false;
        sh.hotn = false;   // (columns with validity words, no predicate)
    } else if (prc == 0) {
        sp.scan_entries(a);
    }
    return VNM_RC_NA;
}

// agg_hot_kernel by predicate form (pm as above)
template <bool HAS_VAL, bool SIMPLE, bool TWO, bool VNULL>
static int launch_hot(int pm, int grid, size_t lds, hipStream_t s, const AggArgs& a) {
    if (pm == 0) return launch_lds(agg_hot_kernel<false, false, HAS_VAL, SIMPLE, false, TWO, VNULL>, grid, AGG_BLOCK, lds, s, a);
    if (pm == 1) return launch_lds(agg_hot_kernel<true, true, HAS_VAL, SIMPLE, false, TWO, VNULL>, grid, AGG_BLOCK, lds, s, a);
    return launch_lds(agg_hot_kernel<true, false, HAS_VAL, SIMPLE, false, TWO, VNULL>, grid, AGG_BLOCK, lds, s, a);
}

// agg_hotn_kernel over NC columns; plain: float64 columns under sums and counts only
template <int NC>
static int launch_hotn(bool has_pred, bool plain, int grid, size_t lds, hipStream_t s, const AggArgs& a) {
    if (has_pred) {
        if (plain) return launch_lds(agg_hotn_kernel<NC, true, true>, grid, AGG_BLOCK, lds, s, a);
        return launch_lds(agg_hotn_kernel<NC, true, false>, grid, AGG_BLOCK, lds, s, a);
    }
    if (plain) return launch_lds(agg_hotn_kernel<NC, false, true>, grid, AGG_BLOCK, lds, s, a);
    return launch_lds(agg_hotn_kernel<NC, false, false>, grid, AGG_BLOCK, lds, s, a);
}

// one launch of the scan the shape asks for
static int launch_scan(const vnm_agg* h, const AggArgs& a, const BatchShape& sh, bool scan_no_pred, int grid, hipStream_t s) {
    const size_t lds_bytes = (size_t)(a.lds_slots + 2) * 8 * (1 + h->plan.n_words);
    const int pm = !h->pred_set ? 0 : (a.hot_pred_is_v ? 1 : 2);
    if (sh.hot_scan) {
        if (a.ent) {  // spilled entries of the partitioned path
            if (sh.hot) return launch_lds(agg_hot_kernel<false, false, true, true, true>, grid, AGG_BLOCK, lds_bytes, s, a);
            return launch_lds(agg_hot_kernel<false, false, true, false, true>, grid, AGG_BLOCK, lds_bytes, s, a);
        }
        if (sh.hot && a.nseg > 0) {  // ... over the waiting batches of a stream
            if (pm == 0) return launch_lds(agg_hot_seg_kernel<false, false>, grid, AGG_BLOCK, lds_bytes, s, a);
            if (pm == 1) return launch_lds(agg_hot_seg_kernel<true, true>, grid, AGG_BLOCK, lds_bytes, s, a);
            return launch_lds(agg_hot_seg_kernel<true, false>, grid, AGG_BLOCK, lds_bytes, s, a);
        }
        if (sh.hot) return launch_hot<true, true, false, false>(pm, grid, lds_bytes, s, a);  // the north-star shape
        if (sh.hot_vnull) return launch_hot<true, false, false, true>(scan_no_pred ? 0 : pm, grid, lds_bytes, s, a);
        if (sh.hot_two) return launch_hot<true, false, true, false>(pm, grid, lds_bytes, s, a);
        if (!a.hot_has_val) {
            if (h->pred_set) return launch_lds(agg_hot_kernel<true, false, false, false>, grid, AGG_BLOCK, lds_bytes, s, a);
            return launch_lds(agg_hot_kernel<false, false, false, false>, grid, AGG_BLOCK, lds_bytes, s, a);
        }
        return launch_hot<true, false, false, false>(pm, grid, lds_bytes, s, a);
    }
    if (sh.hotn) {
        const bool plain = !a.hn_any_int && !a.hn_any_mm;
        switch (h->plan.n_cols) {
            case 3: return launch_hotn<3>(h->pred_set, plain, grid, lds_bytes, s, a);
            case 4: return launch_hotn<4>(h->pred_set, plain, grid, lds_bytes, s, a);
            case 5: return launch_hotn<5>(h->pred_set, plain, grid, lds_bytes, s, a);
            default: return launch_hotn<6>(h->pred_set, plain, grid, lds_bytes, s, a);
        }
    }
    if (h->single) return launch_lds(agg_lds_kernel<1024>, grid, 1024, lds_bytes, s, a);
    agg_wide_kernel<<<grid, 256, 0, s>>>(a);
    return 0;
}

static const char* scan_route_name(const vnm_agg* h, const AggArgs& a, const BatchShape& sh) {
    if (a.ent) return "scan:spilled_entries";
    if (sh.hot_scan) {
        if (sh.hot) return a.nseg > 0 ? "scan:hot_segments" : "scan:hot";
        if (sh.hot_vnull) return "scan:hot_nullable_value";
        return sh.hot_two ? "scan:hot_two_columns" : "scan:hot_generic";
    }
    if (sh.hotn) return "scan:hotn";
    return h->single ? "scan:lds_generic" : "scan:wide_keys";
}

// The general scan: per-workgroup LDS hash tables flushed into the HBM table, which grows until every tile went through.
// Takes the rows of the batch, or what the stages before it spilled (a.ent, or columns made of the spill).
static int run_general_scan(const Batch& b, AggArgs& a, BatchShape& sh, SpillState& sp) {
    vnm_agg* h = b.h;
    hipStream_t s = b.s;
    const int cus = device_info().num_cus;
    const int64_t scan_n = a.nrows;
    PoolScope seg_pool;
    if (h->segs_active && !a.ent) {   // the waiting batches of a stream as segments of one scan (agg_hot_kernel, the hot shape only)
        if ((!(sh.hot_scan && sh.hot) || sp.scan_no_pred || a.has_expr) && one_batch_only(h, "general scan")) return VNM_RC_SINGLY;
    }
    if (h->kn_valid && !a.ent && one_batch_only(h, "scan over the rows")) return VNM_RC_SINGLY;   // (only the dense path's pass 1 reads the key's validity)
    VNM_TRY(ensure_table(h, scan_n, s, sp.spill != nullptr || sp.nspill != nullptr));
    if (sh.hot_scan) a.ntiles = (scan_n + HOT_TILE - 1) / HOT_TILE;
    sh.hotn = sh.hotn && !a.ent && !sp.scan_no_pred && !sh.hot_scan;
    const int hotn_tile = AGG_BLOCK * 2 * (h->plan.n_cols == 3 && !h->pred_set ? 4 : 2);   // (agg_hotn_kernel's U)
    if (sh.hotn) a.ntiles = (scan_n + hotn_tile - 1) / hotn_tile;
    if (h->segs_active && !a.ent) VNM_TRY(upload_segs(h, HOT_TILE, &a.segs, &a.nseg, &a.ntiles, seg_pool, s));
    const int lds_tile = AGG_TILE;
    int grid = h->single ? cus : cus * 4;
    if (grid > a.ntiles) grid = (int)a.ntiles;
    a.margin = (int64_t)grid * (h->single ? (a.lds_slots + 2 + (sh.hot_scan || sh.hotn ? HOT_TILE : lds_tile)) : AGG_TILE);
    sp.progress = (unsigned int*)pool_alloc((size_t)grid * 4);
    if (!sp.progress) return 1;
    VNM_HIP(hipMemsetAsync(sp.progress, 0, (size_t)grid * 4, s));
    a.progress = sp.progress;
    for (int round = 0;; round++) {
        // keep the load factor below 0.7 for everything that can be in flight
        while ((int64_t)(h->g.cap * 7 / 10) < a.margin + 1) VNM_TRY(table_grow(h, h->g.cap * 4, s));
        VNM_HIP(hipMemsetAsync(h->g.ctl, 0, 16, s));  // [1] overflow flag; [2] fill persists
        a.g = h->g;
        a.fill_limit = (int64_t)(h->g.cap * 7 / 10);
        {
            if (round == 0)
                route_note(scan_route_name(h, a, sh), "%lld rows, hint %lld (<= %lld or no partition rule applied), %d words per group, %d LDS slots", (long long)scan_n, (long long)h->hint, (long long)sh.part_min, h->plan.n_words, a.lds_slots);
            KernelTimer timer("agg_scan", s);
            VNM_TRY(launch_scan(h, a, sh, sp.scan_no_pred, grid, s));
        }
        VNM_HIP(hipGetLastError());
        unsigned long long ctl[4];
        VNM_HIP(hipMemcpyAsync(ctl, h->g.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (ctl[1] == 2) return set_error("aggregate: HBM hash table overflow (internal error)");
        // a hint below the partitioning threshold with far more actual groups ran this scan into flush storms (77 ms per
        // 1e9 rows at G = 1e7): the table's fill is the lesson for the batches that follow (checking small hints up
        // front would cost every correctly hinted query ~0.3 ms)
        if (h->single && b.nrows >= (1 << 22) && (int64_t)ctl[2] > 2 * 2400 && (int64_t)ctl[2] > h->hint) h->hint = (int64_t)(ctl[2] + ctl[2] / 4);
        if (!ctl[1]) break;  // no block ran out of room: every tile was processed
        // grow (x4, or to the projected final size) and relaunch; blocks resume from progress[]
        uint64_t new_cap = h->g.cap * 4;
        if (h->hint <= 0 && round >= 1) new_cap = h->g.cap * 16;
        VNM_TRY(table_grow(h, new_cap, s));
    }
    h->rows_seen += b.nrows;
    return 0;
}

// One batch (or the waiting batches of a stream as one: h->segs_active) through the first route that takes it.
static int next_device_impl(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs,
                            const vnm_dcol* pred, void* stream) {
    VNM_TRY(ensure_init());
    if (!h) return set_error("vnm_agg_next_device: null handle");
    if (h->pred_set && !pred) return set_error("vnm_agg_next_device: predicate set but no predicate column given");
    invalidate_result(h);
    if (inputs && nrows > 0) for (int i = 0; i < h->n_funcs; i++) if (h->func_col[i] >= 0 && inputs[i].validity) h->null_inputs_seen = true;
    Batch b{h, nrows, keys, inputs, pred, stream, as_stream(stream), nrows};
    int rc = try_nullable_key_dense(b);
    if (rc != VNM_RC_NA) return rc;
    if (h->segs_active) b.est_rows = (*h->segs_active)[0].nrows;
    if (nrows <= 0) {
        if (h->plan.n_keys == 0 || h->hint <= 0) VNM_TRY(ensure_table(h, nrows, b.s));
        return 0;
    }
    if (nrows >= (1LL << 31)) return set_error("vnm_agg_next_device: batches must be < 2^31 rows (as in the reference, agg_funcs.h:45)");

    const bool key_plain = h->plan.n_keys == 1 && plain8(keys[0]);
    rc = route_packed_keys(b, key_plain);
    if (rc != VNM_RC_NA) return rc;
    rc = route_split_program(b, key_plain);
    if (rc != VNM_RC_NA) return rc;

    AggArgs a{};
    VNM_TRY(fill_agg_args(b, a));
    if (h->plan.n_keys == 0) return run_onegroup(b, a);

    BatchShape sh = classify_batch(h, keys, a);
    bool dense_shape = false, dense_go = false;
    VNM_TRY(decide_dense(b, sh, &dense_shape, &dense_go));
    SpillState sp;
    bool scan_spill = false;   // the small-range scan left only its spilled entries: straight to the general scan
    rc = run_small_range_scan(b, a, sh, dense_shape, dense_go, sp, &scan_spill);
    if (rc != VNM_RC_NA) return rc;
    if (!scan_spill) {
        rc = run_partitioned_paths(b, a, sh, dense_go, sp);
        if (rc != VNM_RC_NA) return rc;
    }
    return run_general_scan(b, a, sh, sp);
}
