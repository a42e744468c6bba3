// Host side of multi-column keys (packing, tuple dictionary) and of split programs (parts per column / pair / column group, joined by key).
// Part of the aggregate operator; included by vnm_agg.hip (one translation unit: the kernels and the host code share file-local helpers).
// ---- packed composite keys: host side ----------------------------------------------------------------------
extern "C" int vnm_agg_finish(vnm_agg* h, int64_t* n_groups, void* stream);
extern "C" int vnm_agg_merge_device(vnm_agg* h, int64_t n, uint64_t* const* key_words, uint64_t* const* acc_words, void* stream);
extern "C" int vnm_agg_next_device(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, void* stream);
extern "C" vnm_agg* vnm_agg_create(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                                   const int* in_types, const int* in_flags, const int* in_col_ids);
extern "C" void vnm_agg_destroy(vnm_agg* h);
static int agg_finish_core(vnm_agg* h, int64_t* n_groups, void* stream);
static int flush_queue(vnm_agg* h, void* stream);

namespace {

// vnm_agg_create without the ordered MIN / MAX engine: the operators the library builds for itself (packed keys, program parts,
// the suffix / merge operators of vnm_agg_exact.inc)
vnm_agg* agg_create(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs, const int* in_types, const int* in_flags,
                    const int* in_col_ids);

// Decide the packing from the key ranges of the first batch: field j holds value codes [0, cap_j) + the NULL code.
// Spare bits are spread over the fields and the observed range is centred in its field, so later batches may
// drift in both directions.  Returns true and fills h->pack when the keys fit 63 bits.
void free_pack_tables(vnm_agg* h) {
    for (int j = 0; j < AGG_MAX_KEYS; j++) {
        if (h->pack.dtab[j]) pool_free(h->pack.dtab[j]);
        h->pack.dtab[j] = nullptr;
    }
}

bool plan_packing(vnm_agg* h, const vnm_dcol* keys, int64_t nrows, hipStream_t s, int* err) {
    *err = 0;
    const int n = h->plan.n_keys;
    PackParams& p = h->pack;
    p.n = n;
    for (int j = 0; j < n; j++) p.cols[j] = keys[j];
    unsigned long long* d = (unsigned long long*)pool_alloc(16 * AGG_MAX_KEYS);
    if (!d) { *err = 1; return false; }
    unsigned long long init[2 * AGG_MAX_KEYS], got[2 * AGG_MAX_KEYS];
    for (int j = 0; j < AGG_MAX_KEYS; j++) { init[2 * j] = ~0ULL; init[2 * j + 1] = 0; }
    bool ok = hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, s) == hipSuccess;
    int grid = (int)std::min<int64_t>((nrows + 255) / 256, (int64_t)device_info().num_cus * 8);
    if (ok) key_range_kernel<<<grid, 256, 0, s>>>(p, nrows, d);
    ok = ok && hipMemcpyAsync(got, d, sizeof(got), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    pool_free(d);
    if (!ok) { *err = set_error("aggregate: key range kernel failed"); return false; }
    int need_bits[AGG_MAX_KEYS];
    uint64_t span[AGG_MAX_KEYS];
    int64_t mn[AGG_MAX_KEYS];
    int total = 0;
    for (int j = 0; j < n; j++) {
        const bool any = got[2 * j] <= got[2 * j + 1];
        mn[j] = any ? (int64_t)(got[2 * j] ^ 0x8000000000000000ULL) : 0;
        const int64_t mx = any ? (int64_t)(got[2 * j + 1] ^ 0x8000000000000000ULL) : 0;
        span[j] = (uint64_t)mx - (uint64_t)mn[j];
        int b = 1;
        if (span[j] >= (1ULL << 61)) b = 64;   // only as a dictionary-coded field
        else {
            const uint64_t need = span[j] + 2;  // values + the NULL code
            while ((1ULL << b) < need) b++;
        }
        need_bits[j] = b;
        total += b;
    }
    // ranges too wide for one word: the widest columns become dictionary-coded fields (see PackParams) until the rest
    // fits.  Each table gets 2.5x the column's estimated distinct count (the estimator reads 8-byte columns;
    // others are taken as all-distinct up to 2^27), at least 2^12 slots -- and up to 2^20 where bits are left over, so
    // that a dictionary planned from a small first batch has room for what later batches bring.
    for (int j = 0; j < AGG_MAX_KEYS; j++) { p.dtab[j] = nullptr; p.dbits[j] = 0; }
    bool is_dict[AGG_MAX_KEYS] = {};
    int range_bits[AGG_MAX_KEYS];
    for (int j = 0; j < n; j++) range_bits[j] = need_bits[j];
    while (total > 63) {
        int w = -1;
        for (int j = 0; j < n; j++)
            if (!is_dict[j] && (w < 0 || need_bits[j] > need_bits[w])) w = j;
        if (w < 0 || getenv("VNM_AGG_NO_DICT") != nullptr) return false;
        int64_t est = std::min<int64_t>(nrows, 1 << 27);
        if (type_width(keys[w].type) == 8 && (keys[w].offset & 1) == 0) {   // (whatever NULL slots hold only adds to the estimate)
            if (estimate_groups(h, keys[w], nrows, &est, s)) { *err = 1; return false; }
        }
        h->widest_est = std::max<int64_t>(h->widest_est, est);   // (a lower bound of the tuple count: sizes the tuple dictionary)
        int tb = 12;
        while (tb < 30 && (1LL << tb) < est * 5 / 2) tb++;
        if (tb + 1 >= need_bits[w]) return false;   // no narrower than its range: nothing left to gain
        is_dict[w] = true;
        p.dbits[w] = tb;
        total += tb + 1 - need_bits[w];
        need_bits[w] = tb + 1;
        span[w] = 0;
        mn[w] = 0;
    }
    for (bool grew = true; grew && total < 63;) {
        grew = false;
        for (int j = 0; j < n && total < 63; j++)
            if (is_dict[j] && p.dbits[j] < 20 && p.dbits[j] + 2 < range_bits[j]) { p.dbits[j]++; need_bits[j]++; total++; grew = true; }
    }
    for (int j = 0; j < n; j++) {
        if (!is_dict[j]) continue;
        const size_t bytes = ((size_t)(1ULL << p.dbits[j]) + 1) * 8;
        p.dtab[j] = (uint64_t*)pool_alloc(bytes);
        if (!p.dtab[j]) { *err = 1; free_pack_tables(h); return false; }
        if (hipMemsetAsync(p.dtab[j], 0xFF, bytes, s) != hipSuccess) {
            *err = set_error("aggregate: key dictionary memset failed");
            free_pack_tables(h);
            return false;
        }
    }
    // A SINGLE packed key (NULLs, a narrow type, an odd offset): ONE spare bit only -- later batches may drift by half the range on
    // either side, and the packed codes (NULL = the field's top code) stay a DENSE range for the inner operator (with all 62 bits the
    // values sat at 2^61 and the NULL code at 2^62 - 1: hash partitions, 21 ms per 5e8 rows at G = 1e8 instead of ~7)
    // SEVERAL fields whose codes together fit the dense path's code range (round 6): one spare bit per field as well -- the packed words
    // then are a dense range the inner operator takes through the ring scatter and direct-addressed tables (with every spare bit spread
    // over the fields the words sat all over 2^62: hash partitions, two int64 keys at G = 1e8: 15.5 ms per 5e8 rows).  A later batch that
    // drifts by more than half a field's range demotes the operator as before.
    bool any_dict = false;
    for (int j = 0; j < n; j++) any_dict = any_dict || p.dtab[j] != nullptr;
    const bool dense_fields = n > 1 && !any_dict && total + n <= DP_MAX_BITS && env_i64("VNM_PACK_DENSE_FIELDS", 1) != 0;
    const int extra = n == 1 ? std::min(1, 63 - total) : (dense_fields ? 1 : (63 - total) / n);
    int shift = 0;
    for (int j = 0; j < n; j++) {
        int b = need_bits[j] + extra;
        if (b > 62) b = 62;
        p.bits[j] = b;
        p.shift[j] = shift;
        shift += b;
        const uint64_t cap = (1ULL << b) - 1;
        const uint64_t slack = cap - (span[j] + 1);
        p.lo[j] = p.dtab[j] ? 0 : (uint64_t)mn[j] - slack / 2;
    }
    return true;
}

// ---- tuple dictionary: host side (tuple_gid_kernel) ---------------------------------------------------------------------
int tdict_alloc(TDict* d, uint64_t cap, int kwt, hipStream_t s) {
    memset(d, 0, sizeof(*d));
    d->cap = cap; d->kwt = kwt; d->sw = kwt <= 6 ? 8 : 16;
    d->slot = (uint64_t*)pool_alloc((size_t)cap * d->sw * 8);
    d->ctl = (unsigned long long*)pool_alloc(64);
    if (!d->slot || !d->ctl || hipMemsetAsync(d->slot, 0xFF, (size_t)cap * d->sw * 8, s) != hipSuccess || hipMemsetAsync(d->ctl, 0, 64, s) != hipSuccess) {
        pool_free(d->slot); pool_free(d->ctl);   // (nothing half-allocated is left behind)
        memset(d, 0, sizeof(*d));
        return set_error("aggregate: tuple dictionary allocation failed");
    }
    return 0;
}

void tdict_free(TDict* d) {
    pool_free(d->slot);
    pool_free(d->ctl);
    memset(d, 0, sizeof(*d));
}

int tdict_grow(TDict* d, uint64_t new_cap, hipStream_t s) {
    TDict nd;
    VNM_TRY(tdict_alloc(&nd, new_cap, d->kwt, s));
    VNM_HIP(hipMemcpyAsync(nd.ctl + 2, d->ctl + 2, 8, hipMemcpyDeviceToDevice, s));   // the fill carries over
    tdict_rehash_kernel<<<(int)std::min<int64_t>(((int64_t)d->cap + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(*d, nd);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    tdict_free(d);
    *d = nd;
    return 0;
}

int enter_tuple_mode(vnm_agg* h, int64_t nrows, hipStream_t s) {
    uint64_t want = h->hint > 0 ? (uint64_t)h->hint * 2 : std::max<uint64_t>((uint64_t)1 << 21, (uint64_t)h->widest_est * 2);
    if (h->hint <= 0 && (uint64_t)nrows * 2 < want) want = (uint64_t)(nrows > 512 ? nrows : 512) * 2;
    VNM_TRY(tdict_alloc(&h->tdict, pow2_at_least(want < 1024 ? 1024 : want), h->plan.n_keys + 1, s));
    const int kt = VNM_U64;
    h->inner = agg_create(VNM_SINGLE_NUMERICAL, 1, &kt, h->n_funcs, h->c_funcs, h->c_in_types, h->c_in_flags,
                              h->c_has_ids ? h->c_in_col_ids : nullptr);
    if (!h->inner) return 1;
    h->inner->hint = h->hint;
    h->tnext = (unsigned long long*)pool_alloc(64);
    if (!h->tnext) return 1;
    VNM_HIP(hipMemsetAsync(h->tnext, 0, 8, s));
    h->tuple_mode = true;
    return 0;
}

void leave_tuple_mode(vnm_agg* h) {
    if (h->tdict.slot) tdict_free(&h->tdict);
    pool_free(h->tnext);
    h->tnext = nullptr;
    h->tuple_mode = false;
}

// one batch: every row's tuple -> group id (find-or-insert in the dictionary), then the ids through the single-key operator
int tuple_next(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, hipStream_t s) {
    TDict* d = &h->tdict;
    PoolScope pool;
    TupArgs a{};
    a.out = (uint64_t*)pool.take((size_t)nrows * 8);
    if (!a.out) return 1;
    a.nk = h->plan.n_keys;
    for (int j = 0; j < a.nk; j++) a.keys[j] = keys[j];
    if (h->pred_set) {
        a.pred = *pred;
        a.p = make_predicate(pred->type, pred->validity != nullptr, h->pred_op, h->pred_is_float, h->pred_dval, h->pred_ival);
    }
    a.nrows = nrows;
    a.ntiles = (nrows + AGG_TILE - 1) / AGG_TILE;
    a.gnext = h->tnext;
    int grid = device_info().num_cus * (int)env_i64("VNM_TUPLE_GRID_PER_CU", 4)   /* (more workgroups = a larger margin of free slots = a larger table: 8 per CU 11.9 ms, 4 per CU 7.8 ms per 2e8 rows at G = 1e6) */;
    if (grid > a.ntiles) grid = (int)a.ntiles;
    a.margin = (int64_t)grid * AGG_TILE;
    a.progress = (unsigned int*)pool.take((size_t)grid * 4);
    if (!a.progress) return 1;
    VNM_HIP(hipMemsetAsync(a.progress, 0, (size_t)grid * 4, s));
    for (int round = 0;; round++) {
        while ((int64_t)(d->cap * 7 / 10) < a.margin + 1) VNM_TRY(tdict_grow(d, d->cap * 4, s));
        VNM_HIP(hipMemsetAsync(d->ctl, 0, 16, s));   // [1] the flag; [2] fill persists
        a.d = *d;
        a.fill_limit = (int64_t)(d->cap * 7 / 10);
        {
            KernelTimer timer("agg_tuple_ids", s);
            switch (d->kwt) {
#define VNM_TG(K) case K: tuple_gid_kernel<K><<<grid, 256, 0, s>>>(a); break;
                VNM_TG(3) VNM_TG(4) VNM_TG(5) VNM_TG(6) VNM_TG(7) VNM_TG(8) VNM_TG(9)
#undef VNM_TG
                default: return set_error("aggregate: tuple dictionary over %d key columns (internal error)", d->kwt - 1);
            }
        }
        VNM_HIP(hipGetLastError());
        unsigned long long ctl[4];
        VNM_HIP(hipMemcpyAsync(ctl, d->ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (!ctl[1]) break;   // no workgroup ran out of room
        VNM_TRY(tdict_grow(d, d->cap * (round >= 1 ? 16 : 4), s));   // the workgroups resume from progress[]
    }
    vnm_dcol gk{};
    gk.values = a.out; gk.type = VNM_U64; gk.length = nrows;
    int rc = vnm_agg_set_predicate(h->inner, h->pred_set ? 1 : 0, h->pred_op, h->pred_is_float, h->pred_dval, h->pred_ival);
    if (!rc) { h->inner->child = true; h->inner->cur_seq = h->cur_seq; rc = vnm_agg_next_device(h->inner, nrows, &gk, inputs, pred, (void*)s); }
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_error("aggregate: tuple-dictionary batch failed");
    if (!rc) h->rows_seen += nrows;
    return rc;
}

// the key words of the inner operator's n finished groups in this operator's wide layout: keys [kw][stride]
int inner_keys(vnm_agg* h, const vnm_agg* in, int64_t n, uint64_t* keys, int64_t stride, hipStream_t s) {
    const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8);
    if (!h->tuple_mode) {
        key_unpack_kernel<<<grid, 256, 0, s>>>(h->pack, in->dkey, n, keys, stride);
        VNM_HIP(hipGetLastError());
        return 0;
    }
    unsigned long long ngid = 0;
    VNM_HIP(hipMemcpyAsync(&ngid, h->tnext, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    const TDict& g = h->tdict;
    PoolScope pool;
    if (g.cap >= (1ULL << 32)) return set_error("aggregate: tuple dictionary beyond 2^32 slots");
    uint32_t* slot_of = (uint32_t*)pool.take((size_t)(ngid ? ngid : 1) * 4);
    if (!slot_of) return 1;
    KernelTimer timer("agg_tuple_keys", s);
    tuple_sweep_kernel<<<(int)std::min<int64_t>(((int64_t)g.cap + 255) / 256, (int64_t)device_info().num_cus * 16), 256, 0, s>>>(g, slot_of, (int64_t)ngid);
    tuple_keys_kernel<<<grid, 256, 0, s>>>(g, slot_of, (int64_t)ngid, in->dkey, n, keys, stride);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

// A later batch does not fit the packing (a key outside the packed ranges, a per-column dictionary that is full): the operator
// moves to the tuple dictionary -- the finished groups' tuples are inserted there and their partial state is re-keyed by id --
// instead of to the wide-key table and its per-row atomics for the rest of the stream.
int packed_to_tuple(vnm_agg* h, int64_t nrows, hipStream_t s) {
    vnm_agg* in = h->inner;
    int64_t n = 0;
    VNM_TRY(vnm_agg_finish(in, &n, (void*)s));
    h->inner = nullptr;   // (enter_tuple_mode makes the new one)
    const int kw = h->plan.kw;
    PoolScope pool;
    uint64_t* words = nullptr;
    int rc = 0;
    if (n > 0) {
        words = (uint64_t*)pool.take((size_t)kw * n * 8);
        if (!words) rc = 1;
        if (!rc) {
            KernelTimer timer("agg_demote", s);
            key_unpack_kernel<<<(int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(h->pack, in->dkey, n, words, n);
        }
        if (!rc && (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) rc = set_error("aggregate: unpacking the groups failed");
    }
    free_pack_tables(h);   // the unpack above was their last reader
    h->widest_est = std::max<int64_t>(h->widest_est, n);
    if (!rc) rc = enter_tuple_mode(h, std::max<int64_t>(nrows, n), s);
    if (!rc && n > 0) {
        TDict* d = &h->tdict;
        while (!rc && (int64_t)(d->cap * 7 / 10) < n + 1) rc = tdict_grow(d, d->cap * 4, s);
        uint64_t* gid = (uint64_t*)pool.take((size_t)n * 16);   // ids, then the (all-zero) null-mask word of the single id key
        if (!rc && !gid) rc = 1;
        if (!rc && hipMemsetAsync(gid + n, 0, (size_t)n * 8, s) != hipSuccess) rc = set_error("aggregate: memset failed");
        if (!rc) {
            const int grid = (int)std::min<int64_t>((n + 2047) / 2048, (int64_t)device_info().num_cus * 8);
            const int64_t per_block = (n + grid - 1) / grid;
            KernelTimer timer("agg_tuple_ids", s);
            switch (d->kwt) {
#define VNM_TW(K) case K: tuple_words_kernel<K><<<grid, 256, 0, s>>>(*d, words, n, per_block, gid, h->tnext); break;
                VNM_TW(3) VNM_TW(4) VNM_TW(5) VNM_TW(6) VNM_TW(7) VNM_TW(8) VNM_TW(9)
#undef VNM_TW
                default: rc = set_error("aggregate: tuple dictionary over %d key columns (internal error)", d->kwt - 1);
            }
        }
        if (!rc) {
            uint64_t* kp[2] = {gid, gid + n};
            uint64_t* ap[AGG_MAX_WORDS];
            for (int w = 0; w < h->plan.n_words; w++) ap[w] = in->dacc + (size_t)w * in->dstride;
            rc = vnm_agg_merge_device(h->inner, n, kp, ap, (void*)s);
        }
        if (!rc && (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) rc = set_error("aggregate: moving the groups to the tuple dictionary failed");
    }
    vnm_agg_destroy(in);
    return rc;
}

// leave packed mode: the groups aggregated so far are unpacked and merged into h's own (wide-key) table
int demote_packed(vnm_agg* h, hipStream_t s) {
    vnm_agg* in = h->inner;
    h->inner = nullptr;
    int64_t n = 0;
    int rc = vnm_agg_finish(in, &n, (void*)s);
    if (!rc && n > 0) {
        const int kw = h->plan.kw;
        uint64_t* keys = (uint64_t*)pool_alloc((size_t)kw * n * 8);
        if (!keys) rc = 1;
        if (!rc) {
            int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8);
            {
                KernelTimer timer("agg_demote", s);
                rc = inner_keys(h, in, n, keys, n, s);
            }
            uint64_t* kp[AGG_MAX_KEYS + 1];
            uint64_t* ap[AGG_MAX_WORDS];
            for (int j = 0; j < kw; j++) kp[j] = keys + (size_t)j * n;
            for (int w = 0; w < h->plan.n_words; w++) ap[w] = in->dacc + (size_t)w * in->dstride;
            if (!rc) rc = vnm_agg_merge_device(h, n, kp, ap, (void*)s);
            if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_error("aggregate: demotion failed");
        }
        pool_free(keys);
    }
    vnm_agg_destroy(in);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = set_error("aggregate: demotion failed");
    free_pack_tables(h);   // the unpack above was their last reader
    leave_tuple_mode(h);
    return rc;
}


// ---- program split --------------------------------------------------------------------------------------------------------
struct PartJoinArgs {
    int64_t n;
    const int64_t* perm;          // perm[i] = the part's group with the i-th smallest key
    const uint64_t* key_src;      // the part's key words
    const uint64_t* mask_src;     // ... and its null-mask words (1 = the NULL-key group, whose key word is 0)
    uint64_t* key_out;            // first part: writes the joined key column; the others compare with it (same rows -> same keys)
    uint64_t* mask_out;
    int check;
    unsigned long long* flag;
    int nw;
    const uint64_t* src[AGG_MAX_WORDS];
    uint64_t* dst[AGG_MAX_WORDS];
};
// one pass per part: the permutation is read once and the part's words of a group are gathered together (one kernel per
// word: 20 ms for 18 words x 2e7 groups, the random 8-byte reads one after the other)
__global__ __launch_bounds__(256) void part_join_kernel(PartJoinArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    // The parts are sorted by key word alone; the NULL-key group (key word 0, mask 1) and a real key 0 are then the first two
    // rows in an order each part decides for itself: the real key goes first, the NULL group second, in every part.
    bool swap01 = false;
    if (a.n >= 2 && a.perm) {
        const int64_t g0 = a.perm[0], g1 = a.perm[1];
        swap01 = a.key_src[g0] == 0 && a.key_src[g1] == 0 && a.mask_src[g0] != 0 && a.mask_src[g1] == 0;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const int64_t g = a.perm ? a.perm[swap01 && i < 2 ? 1 - i : i] : i;   // (no permutation: the parts agree on the order)
        const uint64_t k = a.key_src[g], m = a.mask_src[g];
        if (a.check) bad = bad || a.key_out[i] != k || a.mask_out[i] != m;
        else { a.key_out[i] = k; a.mask_out[i] = m; }
        for (int w = 0; w < a.nw; w++) a.dst[w][i] = a.src[w][g];
    }
    if (bad) __hip_atomic_store(a.flag, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Parts that took the dense path over the SAME code map write their groups in runs of ascending code: the final passes place a
// partition's groups 64 slots (one wave's ballot) at a time, the partitions wherever their workgroup's claim landed.  So a UNIT of 64
// codes is one contiguous, equally ordered stretch of rows in every part, and the join needs neither sorts nor random gathers: a
// table of every unit's first row per part (part_unit_starts_kernel), then row i of part 0 = row start_p[u] + (i - start_0[u]) of
// part p (part_unit_join_kernel, which compares the keys it pairs: anything else -- groups outside the code range, a NULL-key group,
// a part that took another path -- fails the attempt and the sort join below does the work).
struct PartUnitArgs {
    DenseMap map;
    int64_t n;
    const uint64_t* key0;   // part 0: its order is the order of the joined run
    const uint64_t* mask0;
    const uint64_t* key;    // the part being placed
    const uint64_t* mask;
    const uint32_t* start0;
    uint32_t* start;
    uint64_t* key_out;      // (written with part 0)
    uint64_t* mask_out;
    unsigned long long* bad;
    int nw;
    const uint64_t* src[AGG_MAX_WORDS];
    uint64_t* dst[AGG_MAX_WORDS];
};
__device__ __forceinline__ bool part_unit_of(const DenseMap& m, uint64_t key, uint64_t mask, uint32_t* unit) {
    const uint64_t d = (key ^ m.sign) - m.lo_u;
    *unit = (((uint32_t)d * m.mul) & m.mask) >> 6;
    return mask == 0 && d <= (uint64_t)m.mask;
}
__global__ __launch_bounds__(256) void part_unit_starts_kernel(PartUnitArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        uint32_t u, up = ~0u;
        bad = bad || !part_unit_of(a.map, a.key[i], a.mask[i], &u);
        if (i > 0) part_unit_of(a.map, a.key[i - 1], 0, &up);
        if (u != up) a.start[u] = (uint32_t)i;
    }
    if (bad) __hip_atomic_store(a.bad, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(256) void part_unit_join_kernel(PartUnitArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const uint64_t k = a.key0[i];
        uint32_t u;
        part_unit_of(a.map, k, 0, &u);
        const int64_t j = (int64_t)a.start[u] + (i - (int64_t)a.start0[u]);
        if (j < 0 || j >= a.n || a.key[j] != k || a.mask[j] != 0) { bad = true; continue; }
        if (a.key_out) { a.key_out[i] = k; a.mask_out[i] = 0; }
        for (int w = 0; w < a.nw; w++) a.dst[w][i] = a.src[w][j];
    }
    if (bad) __hip_atomic_store(a.bad, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void drop_parts(vnm_agg* h) {
    for (vnm_agg* c : h->parts) vnm_agg_destroy(c);
    h->parts.clear();
    h->part_funcs.clear();
}

// cut the function list by input column: `per` columns to a part (balanced), COUNT(*) with the first one
int make_parts(vnm_agg* h, int per) {
    const int nc = h->plan.n_cols;
    const int k = (nc + per - 1) / per;
    std::vector<int> part_of_col(nc);
    for (int c = 0; c < nc; c++) part_of_col[c] = (int)((int64_t)c * k / nc);
    h->part_funcs.assign(k, std::vector<int>());
    for (int i = 0; i < h->n_funcs; i++) h->part_funcs[h->func_col[i] < 0 ? 0 : part_of_col[h->func_col[i]]].push_back(i);
    const int kt = h->plan.key_types[0];
    for (int p = 0; p < k; p++) {
        int funcs[AGG_MAX_FUNCS], types[AGG_MAX_FUNCS], flags[AGG_MAX_FUNCS], ids[AGG_MAX_FUNCS];
        const int nf = (int)h->part_funcs[p].size();
        for (int q = 0; q < nf; q++) {
            const int i = h->part_funcs[p][q];
            funcs[q] = h->c_funcs[i]; types[q] = h->c_in_types[i]; flags[q] = h->c_in_flags[i]; ids[q] = h->func_col[i];   // (the distinct column: sharing survives)
        }
        vnm_agg* c = agg_create(VNM_SINGLE_NUMERICAL, 1, &kt, nf, funcs, types, flags, ids);
        if (!c) { drop_parts(h); return 1; }
        c->hint = h->hint;
        c->estimated = h->estimated;
        c->split_tried = true;
        c->async = h->async;   // (a stream: the parts record their batches like the parent would -- one launch per part over all of them)
        c->heavy_share = h->heavy_share;   // (the parent's sample saw the same key column)
        if (h->dense_state >= 1 && !h->range_given) {   // ... and its code map: no second range sample, and the parts' maps agree by construction
            c->dense_state = h->dense_state; c->dmap = h->dmap; c->dense_span = h->dense_span; c->dense_rlo = h->dense_rlo; c->dense_rhi = h->dense_rhi;
        }
        h->parts.push_back(c);
    }
    return 0;
}

int next_parts(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, void* stream) {
    const bool bound = (int64_t)h->parts.size() * nrows * 14 > env_i64("VNM_SPLIT_PENDING_BYTES", (int64_t)64 << 30);
    for (size_t p = 0; p < h->parts.size(); p++) {
        vnm_agg* c = h->parts[p];
        vnm_dcol in[AGG_MAX_FUNCS];
        const int nf = (int)h->part_funcs[p].size();
        for (int q = 0; q < nf; q++) in[q] = inputs[h->part_funcs[p][q]];
        VNM_TRY(vnm_agg_set_predicate(c, h->pred_set ? 1 : 0, h->pred_op, h->pred_is_float, h->pred_dval, h->pred_ival));
        c->child = true; c->cur_seq = h->cur_seq;
        VNM_TRY(vnm_agg_next_device(c, nrows, keys, in, pred, stream));
        // every part of the dense path keeps its scatter output (~10-18 bytes per row) for a deferred final pass: many parts over a
        // very large batch run their final passes right away instead of holding all of that at once
        if (bound && c->pending) VNM_TRY(complete_pending(c, as_stream(stream)));
    }
    h->rows_seen += nrows;
    return 0;
}

// The parts' results joined by key into ONE run of this operator (ascending key bits), the parts destroyed.  Every part
// grouped the same rows, so every part holds the same keys: sorting each part's keys gives the permutation that lines its
// accumulator words up with the others'.
int collapse_parts(vnm_agg* h, hipStream_t s) {
    if (h->parts.empty()) return 0;
    KernelTimer timer("agg_split_join", s);
    const int k = (int)h->parts.size();
    int64_t n = -1;
    for (int p = 0; p < k; p++) {
        int64_t np = 0;
        KernelTimer t2("agg_split_finish", s);
        VNM_TRY(vnm_agg_finish(h->parts[p], &np, (void*)s));
        if (n >= 0 && np != n) return set_error("aggregate: the parts of a split program disagree on the group count (%lld / %lld; internal error)", (long long)n, (long long)np);
        n = np;
    }
    if (h->have_run || h->have_table || h->pending) return set_error("aggregate: split program with state of its own (internal error)");
    if (n > 0) {
        PoolScope pool;
        const int64_t stride = n + 2;
        uint64_t* rk = (uint64_t*)pool_alloc((size_t)stride * 8 * 2);
        uint64_t* ra = (uint64_t*)pool_alloc((size_t)stride * 8 * h->plan.n_words);
        unsigned long long* flag = (unsigned long long*)pool.take(64);
        std::vector<int64_t*> perm(k, nullptr);
        bool ok = rk && ra && flag;
        if (!ok) { pool_free(rk); pool_free(ra); return 1; }
        int rc = hipMemsetAsync(flag, 0, 16, s) != hipSuccess;
        const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8);
        // word lists of every part (parent word <- part word)
        std::vector<PartJoinArgs> jas(k);
        {
            std::vector<char> done(h->plan.n_words, 0);
            for (int p = 0; p < k && !rc; p++) {
                const vnm_agg* c = h->parts[p];
                PartJoinArgs& ja = jas[p];
                ja = PartJoinArgs{};
                ja.n = n; ja.key_src = c->dkey; ja.mask_src = c->dkey + c->dstride; ja.key_out = rk; ja.mask_out = rk + stride;
                ja.check = p > 0; ja.flag = flag;
                for (size_t q = 0; q < h->part_funcs[p].size() && !rc; q++) {
                    const FuncOut& mine = h->outs[h->part_funcs[p][q]];
                    const FuncOut& theirs = c->outs[q];
                    const int pw[3] = {mine.w_valid, mine.w_a, mine.w_b}, cw[3] = {theirs.w_valid, theirs.w_a, theirs.w_b};
                    for (int j = 0; j < 3; j++) {
                        if (pw[j] < 0 || done[pw[j]]) continue;
                        if (cw[j] < 0) { rc = set_error("aggregate: split program, accumulator layouts differ (internal error)"); break; }
                        done[pw[j]] = 1;
                        ja.src[ja.nw] = c->dacc + (size_t)cw[j] * c->dstride;
                        ja.dst[ja.nw++] = ra + (size_t)pw[j] * stride;
                    }
                }
            }
            for (int w = 0; w < h->plan.n_words && !rc; w++)
                if (!done[w]) rc = set_error("aggregate: split program, accumulator word %d has no source (internal error)", w);
        }
        // the join by units of 64 codes (parts of the dense path over one code map: see part_unit_starts_kernel)
        bool joined = false;
        DenseMap umap = h->parts[0]->dmap;
        const int ustate = h->parts[0]->dense_state;
        if (ustate == 2) { umap.mul = 1; umap.mul_inv = 1; }   // (the small-range scans address their tables by the plain code; a generic program that
                                                               // re-centred its range fails the key comparison below and takes the sort join)
        bool by_units = !rc && (ustate == 1 || ustate == 2) && n < ((int64_t)1 << 31) && getenv("VNM_AGG_NO_UNIT_JOIN") == nullptr;
        for (int p = 1; p < k && by_units; p++) by_units = h->parts[p]->dense_state == ustate && memcmp(&h->parts[p]->dmap, &h->parts[0]->dmap, sizeof(DenseMap)) == 0;
        if (by_units) {
            KernelTimer t2("agg_split_units", s);
            const size_t units = ((size_t)umap.mask + 1 + 63) >> 6;
            std::vector<uint32_t*> start(k, nullptr);
            for (int p = 0; p < k && by_units; p++) by_units = (start[p] = (uint32_t*)pool.take(units * 4)) != nullptr;
            for (int p = 0; p < k && by_units && !rc; p++) {
                PartUnitArgs ua{};
                ua.map = umap; ua.n = n; ua.key = jas[p].key_src; ua.mask = jas[p].mask_src; ua.start = start[p]; ua.bad = flag + 1;
                rc = hipMemsetAsync(start[p], 0xff, units * 4, s) != hipSuccess;
                if (!rc) part_unit_starts_kernel<<<grid, 256, 0, s>>>(ua);
            }
            for (int p = 0; p < k && by_units && !rc; p++) {
                PartUnitArgs ua{};
                ua.map = umap; ua.n = n; ua.key0 = jas[0].key_src; ua.mask0 = jas[0].mask_src; ua.key = jas[p].key_src; ua.mask = jas[p].mask_src;
                ua.start0 = start[0]; ua.start = start[p]; ua.bad = flag + 1;
                if (p == 0) { ua.key_out = rk; ua.mask_out = rk + stride; }
                ua.nw = jas[p].nw;
                for (int w = 0; w < ua.nw; w++) { ua.src[w] = jas[p].src[w]; ua.dst[w] = jas[p].dst[w]; }
                part_unit_join_kernel<<<grid, 256, 0, s>>>(ua);
            }
            unsigned long long ubad = 0;
            if (by_units && !rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(&ubad, flag + 1, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                                    hipStreamSynchronize(s) != hipSuccess))
                rc = set_error("aggregate: joining the parts of a split program failed");
            joined = by_units && !rc && ubad == 0;
        }
        const bool same_order = joined;
        const int asc = VNM_ASC;
        for (int p = 0; p < k && !rc && !same_order; p++) {
            vnm_dcol kc{};
            kc.values = h->parts[p]->dkey; kc.type = VNM_U64; kc.length = n;
            KernelTimer t2("agg_split_sort", s);
            if (!(perm[p] = (int64_t*)pool.take((size_t)n * 8))) { pool_free(rk); pool_free(ra); return 1; }
            rc = vnm_sort_indices(1, &kc, &asc, n, 0, perm[p], (void*)s);
        }
        for (int p = 0; p < k && !rc && !joined; p++) {
            jas[p].perm = perm[p];
            part_join_kernel<<<grid, 256, 0, s>>>(jas[p]);
        }
        unsigned long long bad = 0;
        if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, flag, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipStreamSynchronize(s) != hipSuccess))
            rc = set_error("aggregate: joining the parts of a split program failed");
        if (!rc && bad) rc = set_error("aggregate: the parts of a split program hold different keys (internal error)");
        if (rc) { pool_free(rk); pool_free(ra); return rc; }
        adopt_run(h, rk, ra, stride, n);   // (no directory: the handle held no run)
    }
    drop_parts(h);
    return 0;
}

vnm_agg* agg_create(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                    const int* in_types, const int* in_flags, const int* in_col_ids) {
    if (ensure_init()) return nullptr;
    vnm_agg* h = new vnm_agg();
    if (build_plan(kind, n_keys, key_types, n_funcs, funcs, in_types, in_flags, in_col_ids, &h->plan, h->outs)) {
        delete h;
        return nullptr;
    }
    h->n_funcs = n_funcs;
    // distinct column index per func: replay build_plan's assignment
    int ids[AGG_MAX_COLS], nc = 0;
    for (int i = 0; i < n_funcs; i++) {
        h->func_col[i] = -1;
        if (funcs[i] == VNM_COUNT_STAR) continue;
        int id = in_col_ids ? in_col_ids[i] : (1000 + i);
        if (id < 0) id = -1000 - i;   // as build_plan: negative = this function's own column
        for (int c = 0; c < nc; c++) if (ids[c] == id) h->func_col[i] = c;
        if (h->func_col[i] < 0) { ids[nc] = id; h->col_first_func[nc] = i; h->func_col[i] = nc++; }
    }
    h->single = (kind == VNM_SINGLE_NUMERICAL) || (kind == VNM_MULTI_NUMERICAL && n_keys == 1);
    for (int i = 0; i < n_funcs; i++) {
        h->c_funcs[i] = funcs[i];
        h->c_in_types[i] = in_types ? in_types[i] : 0;
        h->c_in_flags[i] = in_flags ? in_flags[i] : 0;
        h->c_in_col_ids[i] = in_col_ids ? in_col_ids[i] : 0;
    }
    h->c_has_ids = in_col_ids != nullptr;
    return h;
}

}  // namespace
