// Host side of the partitioned routes, each a driver over stage functions (plan -> blocks -> passes -> hand-over): the hash partitions
// (partitioned_aggregate), the scans of small ranges (dense_scan_generic, dense_scan_stream), the deferred final pass (complete_pending), the
// dense-key path (dense_partitioned_aggregate: one / two levels) and its two-value form (dense_two_aggregate).
// Part of the aggregate operator; included by vnm_agg.hip (one translation unit: the kernels and the host code share file-local helpers).
namespace {
// ---- typed launches ----------------------------------------------------------------------------------------------
// Run-time values as template arguments: `f` is a generic lambda that gets a std::integral_constant and names the kernel ONCE.
// Only the values a caller can pass are instantiated (a ladder must not add kernels to the code object).
template <class F>
int pick_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// an int in LO .. HI (below LO: LO, above HI: HI) -- table bits 7 .. 13, 8-byte words of a wide entry 1 .. 7
template <int LO, int HI, class F>
int pick_int(int v, F&& f) {
    if constexpr (LO < HI) { if (v > LO) return pick_int<LO + 1, HI>(v, f); }
    return f(std::integral_constant<int, LO>{});
}
// output mode of a dense final pass: DF_COLS, DF_TABLE, anything else DF_RUN
template <class F>
int pick_out(int out, F&& f) {
    if (out == DF_COLS) return f(std::integral_constant<int, DF_COLS>{});
    if (out == DF_TABLE) return f(std::integral_constant<int, DF_TABLE>{});
    return f(std::integral_constant<int, DF_RUN>{});
}
// A final-pass kernel as ONE resident set of workgroups (they loop over their work items): at most `occ_max` per CU of what the
// occupancy of `occ_kernel` allows.  `lds` bytes of dynamic LDS (more than the default limit: the attribute first).
template <class K, class Q, class... A>
int launch_resident_as(K kernel, Q occ_kernel, int64_t work, int block, size_t lds, int occ_max, hipStream_t s, const A&... args) {
    if (lds) VNM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)occ_kernel, block, lds) != hipSuccess || occ < 1) occ = 1;
    const int grid = (int)std::min<int64_t>(work, (int64_t)device_info().num_cus * std::min(occ, occ_max));
    kernel<<<grid, block, lds, s>>>(args...);
    return 0;
}
template <class K, class... A>
int launch_resident(K kernel, int64_t work, int block, size_t lds, int occ_max, hipStream_t s, const A&... args) {
    return launch_resident_as(kernel, kernel, work, block, lds, occ_max, s, args...);
}
// a kernel with `lds` bytes of dynamic LDS (more than the default limit: the attribute first)
template <class K, class... A>
int launch_dyn(K kernel, int grid, int block, size_t lds, hipStream_t s, const A&... args) {
    VNM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, block, lds, s>>>(args...);
    return 0;
}
// The final pass of the hash partitions: one resident set of workgroups (they loop over the partitions) -- a grid larger than what
// fits leaves a second, partly filled round.  Four workgroups per CU where the occupancy is not to be had.
template <class K>
int launch_part_final(K kernel, int64_t work, size_t lds, hipStream_t s, const PartAggArgs& pa) {
    const int cus = device_info().num_cus;
    if (lds) VNM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int grid = (int)std::min<int64_t>(work, (int64_t)cus * 4), occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)kernel, PA_BLOCK, lds) == hipSuccess && occ > 0)
        grid = (int)std::min<int64_t>(work, (int64_t)cus * std::min(occ, (int)env_i64("VNM_PA_OCC", 8)));
    kernel<<<grid, PA_BLOCK, lds, s>>>(pa);
    return 0;
}

// ---- the ring scatter of the dense path (dring_scatter_kernel) ----------------------------------------------------------
// One launch: the grid, the entries per ring, the sub-tile (pairs of rows per lane), and what picks the kernel at run time.
// limit: VNM_DENSE_RING_LIMIT, spill what two insert / flush rounds of a sub-tile leave pending (skew); seg / kn: pass 1 over the
// waiting batches of a stream (DPartArgs::segs) / over a nullable key
struct RingLaunch { int grid, cap, pairs; bool limit, seg, kn; hipStream_t s; };
// entries per flushed block: 32-bit words leave in blocks of 32
constexpr int ring_flush_block(bool w32) { return w32 ? 32 : DR_FB; }
// an even spread of a sub-tile's entries (every row surviving) fits ONE insert / flush round of the rings
inline bool ring_one_round(int pairs, int nparts, int cap, bool w32) { return 2 * pairs * 1024 <= nparts * (cap - ring_flush_block(w32)); }
// sub-tile = the largest of 4 / 2 / 1 pairs of rows per lane (at most `want`) whose entries, evenly spread, fit one round of the
// rings: the round limit then applies (64 partitions: 2 pairs, 32: 1 pair).  A predicate column of its own (pv): three loads per
// pair of rows, at most two pairs per lane and sub-tile fit the registers.
inline int ring_sub_tile_pairs(int want, bool pv, bool limit, int nparts, int cap, bool w32) {
    int pr = want >= 4 && !pv ? 4 : (want >= 2 ? 2 : 1);
    while (limit && pr > 1 && !ring_one_round(pr, nparts, cap, w32)) pr >>= 1;
    return pr;
}
// Ring capacity = what fits 128 KB of LDS, whole 16-entry blocks only; fan-outs that leave less than two blocks per ring (0) keep
// the tile-sorting kernel.
inline int ring_cap_for(int np, size_t esize) {
    int cap = (int)((size_t)(env_i64("VNM_DENSE_RING_LDS", 128) * 1024) / ((size_t)np * esize) / DR_FB) * DR_FB;
    // at most 80 entries per ring -- more where few partitions share the LDS, so that an even spread of a four-pair sub-tile
    // (8192 entries) still fits one round: 32 partitions 272, 64 partitions 144
    cap = std::min(cap, (int)env_i64("VNM_DENSE_RING_CAP", std::max(80, ((8192 / np + DR_FB + DR_FB - 1) / DR_FB) * DR_FB)));
    // few partitions: long runs anyway (and 8192 entries per sub-tile on a handful of ring cursors: G = 1e4, four partitions,
    // pass 1 8.6 ms against 5.0 with the tile-sorting kernel)
    if (np < env_i64("VNM_DENSE_RING_MIN_NP", 32)) return 0;
    return cap >= 2 * DR_FB ? cap : 0;
}
// (32-bit words: blocks of 32, rings of at least two blocks, at most 256 entries)
inline int ring_cap_w32(int np) {
    const int cap = std::min(256, (int)((size_t)128 * 1024 / ((size_t)np * 4) / 32) * 32);
    return cap >= 64 ? cap : 0;
}

// the attribute and the launch of one kernel of the family (1024 threads; the rings take nparts * cap entries of LDS)
template <bool FR, typename CT, bool HV, int PR, bool PV, bool VN, int MAXR, bool SEG, bool KN, bool V2, bool FX, bool W32, bool IN32 = false, bool WIN = false>
int launch_ring(int grid, const DPartArgs& d, int cap, hipStream_t s) {
    constexpr size_t esize = FX ? (W32 ? 4 : 8) : (HV ? (V2 ? 16 : 8) : 0) + sizeof(CT);
    const size_t lds = (((size_t)d.nparts * cap * esize) + 15) & ~(size_t)15;
    return launch_dyn(dring_scatter_kernel<FR, CT, HV, 1024, PR, PV, VN, MAXR, SEG, KN, V2, FX, W32, IN32, WIN>, grid, 1024, lds, s, d, cap);
}
// ... with PR pairs per lane.  MAXR = 2 (round limit: two insert / flush rounds per sub-tile) where one round takes an even spread;
// the SEG and KN kernels exist for pass 1 over a plain value column only (same shapes otherwise).
template <bool FR, typename CT, bool HV, bool PV, bool VN, bool FX, bool W32, int PR, bool IN32 = false, bool WIN = false>
int ring_scatter_pairs(const RingLaunch& r, const DPartArgs& d) {
    auto go = [&](auto lim, auto seg, auto kn) {
        return launch_ring<FR, CT, HV, PR, PV, VN, decltype(lim)::value ? 2 : 0, decltype(seg)::value, decltype(kn)::value, false, FX, W32, IN32, WIN>(r.grid, d, r.cap, r.s);
    };
    return pick_bool(r.limit && ring_one_round(PR, d.nparts, r.cap, W32), [&](auto lim) {
        if constexpr (FR && HV && !VN) {
            if (r.kn) return go(lim, std::false_type{}, std::true_type{});
            if (r.seg) return go(lim, std::true_type{}, std::false_type{});
        }
        return go(lim, std::false_type{}, std::false_type{});
    });
}
// FR: pass 1 (from rows); CT: the code remainders; HV: entries carry a value; PV: a predicate column of its own; VN: a nullable
// value column; FX / W32: fixed-point entry words / of 32 bits; IN32: pass 2 over 32-bit words; WIN: pass 1 writes window words.  r.pairs comes from ring_sub_tile_pairs (never 4 with PV).
template <bool FR, typename CT, bool HV, bool PV, bool VN, bool FX = false, bool W32 = false, bool IN32 = false, bool WIN = false>
int ring_scatter(const RingLaunch& r, const DPartArgs& d) {
    if constexpr (!PV) {
        if (r.pairs == 4) return ring_scatter_pairs<FR, CT, HV, PV, VN, FX, W32, 4, IN32, WIN>(r, d);
    }
    if (r.pairs >= 2) return ring_scatter_pairs<FR, CT, HV, PV, VN, FX, W32, 2, IN32, WIN>(r, d);
    return ring_scatter_pairs<FR, CT, HV, PV, VN, FX, W32, 1, IN32, WIN>(r, d);
}

// ---- what the routes share --------------------------------------------------------------------------------------------
// the WHERE comparison of a kernel's arguments (the hash partitions' wide entries add PartArgs::wp / wpred beside the call)
template <class X> void fill_pred(X& x, const vnm_agg* h, const AggArgs& a) {
    x.pp = h->pred_set ? (const double*)a.pred.values + a.pred.offset : nullptr;
    x.has_pred = h->pred_set; x.pred_is_v = a.hot_pred_is_v; x.op = a.p.op; x.thr = a.p.dval;
}
// the first words of a flags block, as many as `fl` holds, once the stream has run dry
template <size_t N> int read_flags(unsigned long long (&fl)[N], const unsigned long long* flags, hipStream_t s) {
    VNM_HIP(hipMemcpyAsync(fl, flags, N * 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}
// Every pool block of one attempt: what has not been keep()-ed goes back on every return path; free_all() before the batch is tried again.
struct AttemptBlocks {
    PoolScope pool;
    template <class T> void take(T*& p, size_t bytes) { p = (T*)pool.take(bytes); }
    void free_all() { while (pool.n > 0) pool.done(pool.blocks[pool.n - 1]); }
};
constexpr int ATTEMPT_REDO = 4;   // a stage's answer: free everything, then the same batch once more (the handle says what changes)

// ---- the hash partitions, stage by stage (partitioned_aggregate below is the driver) ----------------------------------------
// The whole geometry of one attempt.  Filled by plan_hash_partitions, which makes no HIP call and leaves the handle alone.
struct HashPlan {
    int pa_slots;                            // slots of the final pass's LDS table
    int64_t per_final, nfin;                 // groups per final partition; final partitions (np1, or np1 * np2)
    int E; bool wide; size_t ebytes;         // 8-byte words per entry; generic column accessors (any width, NULLs, any predicate column)
    int levels, np1, np2, lg1;               // fan-out of the levels, np1 <= 2^lg1
    int grid1, split2, fin_regions;          // pass-1 workgroups; pass-2 workgroups per first-level partition; regions per final partition
    int64_t tile1, rows_per_wg; double slack;
    int64_t cap1, cap2, spill_cap;           // entries per region after pass 1 / pass 2; of the spill buffer (0: none wanted)
    bool ring1, ring2, ring2_512;            // (key, value) entries through LDS rings (pring_scatter_kernel), per level
    int rcap1, rcap2; size_t rlds1, rlds2;   // ... entries per ring, bytes of LDS
    // hash_plan_final, after the scatters: workgroups that share a final partition; these merge through the HBM table / write partial groups into the run
    int splits; bool to_table, dup_run; int64_t dstride;
};
// Stage 1: partitions, levels, regions, rings.  0, or 2 = would need a third level.
int plan_hash_partitions(const vnm_agg* h, const AggArgs& a, int64_t nrows, bool want_spill, HashPlan* p) {
    const int cus = device_info().num_cus;
    // final partitions sized for ~900 groups each: enough keys per partition that their sizes concentrate
    // (few keys per partition -> Poisson imbalance overflows the fixed-capacity regions), few enough for
    // the 2048-slot LDS table of pass 3
    // Generic programs with three or more accumulator words: a 2048-slot table is 65+ KB, i.e. one or two resident
    // workgroups per CU in a latency-bound pass (5 words, G=1e5: 10 ms).  They get 1024-slot tables and half the groups
    // per partition while two levels still provide enough partitions.
    const int64_t l1_max = env_i64("VNM_AGG_PART_L1_MAX", 256);
    const bool small_tables = a.part_generic && (size_t)(PA_SLOTS + 1) * 8 * (1 + h->plan.n_words) > 54 * 1024 &&
                              h->hint / 450 < l1_max * 512 && getenv("VNM_AGG_NO_SMALL_TABLES") == nullptr;
    int pa_slots = small_tables ? PA_SLOTS / 2 : PA_SLOTS;
    // ... and programs with so many words that even that table exceeds the LDS (three compensated float SUMs + their
    // counts + COUNT(*) = 10 words: 180 KB at 2048 slots) halve it until it fits: more, smaller partitions instead of
    // the HBM-atomics path (300 ms per 1e9 rows)
    while (a.part_generic && pa_slots > 256 && (size_t)(pa_slots + 1) * 8 * (1 + h->plan.n_words) > 150 * 1024) pa_slots /= 2;
    p->pa_slots = pa_slots;
    p->per_final = env_i64("VNM_AGG_PART_GROUPS", 900 * pa_slots / PA_SLOTS);
    int64_t nfin = 2;
    while (nfin * p->per_final < h->hint) nfin *= 2;
    if (nfin > l1_max * 512) {
        // two levels give at most l1_max * 512 partitions: still fine while a partition's groups fit the LDS table
        if (h->hint / (l1_max * 512) > 1600 * pa_slots / PA_SLOTS) return 2;  // would need a third level
        nfin = l1_max * 512;
    }
    // entry = key + one value (16 bytes, tuned kernels) or key + 2-3 values (wide entries)
    p->E = a.part_wide ? 1 + h->plan.n_cols + (a.part_vmask ? 1 : 0) : 2;
    p->wide = a.part_wide != 0; p->ebytes = (size_t)p->E * 8;
    p->tile1 = p->wide ? pw_tile(p->E) : PT_TILE;
    // twice the usual first-level fan-out still beats a second level that would only split in two (G = 3e5 sparse keys:
    // 512 partitions in one pass 7.4 + 1.9 ms; 256 x 2: 6.7 + 3.7 + 2.0)
    p->levels = nfin > std::min<int64_t>(l1_max * 2, PT_MAXP) ? 2 : 1;
    const int np1 = p->np1 = p->levels == 2 ? (int)l1_max : (int)nfin;
    const int np2 = p->np2 = p->levels == 2 ? (int)(nfin / l1_max) : 0;
    p->nfin = p->levels == 2 ? (int64_t)np1 * np2 : np1;
    while ((1 << p->lg1) < np1) p->lg1++;
    const int64_t tiles = (nrows + p->tile1 - 1) / p->tile1;
    p->grid1 = (int)std::min<int64_t>((int64_t)cus * 2, tiles);
    p->split2 = std::max(2, (p->grid1 + PT_MAX_REGIONS - 1) / PT_MAX_REGIONS);
    p->fin_regions = p->levels == 2 ? p->split2 : p->grid1;
    p->rows_per_wg = (tiles + p->grid1 - 1) / p->grid1 * p->tile1;
    // region slack: a partition holds per_final / 2 ... per_final keys, so its share of the rows scatters by 1 / sqrt(keys)
    // around the mean (small LDS tables -> few keys per partition -> up to +42 %; measured: 225 keys per partition
    // overflowed the 25 % regions of pass 2 at G = 3e5 and 1e6)
    p->slack = std::max(0.0, 4.5 / std::sqrt((double)std::max<int64_t>(p->per_final, 16) / 2.0));
    p->cap1 = p->rows_per_wg / np1 + (int64_t)((double)(p->rows_per_wg / np1) * std::max(0.2, p->slack)) + 512;
    if (p->levels == 2) {   // worst case: every row survived and spread evenly; 25 % slack + constant
        const int64_t per_pg = (int64_t)p->grid1 * p->rows_per_wg / np1 / p->split2;
        p->cap2 = per_pg / np2 + (int64_t)((double)(per_pg / np2) * std::max(0.25, p->slack)) + 256;
    }
    p->spill_cap = want_spill ? nrows / 2 + (1 << 20) : 0;
    // (key, value) entries through LDS rings where a level has at most 256 partitions: rings of >= 32 entries, 256-byte blocks
    // (512 partitions: 16 entries, blocks of 8, one pair per lane)
    auto ring_cap = [](int np) { return std::min((int)((size_t)128 * 1024 / 16 / (size_t)np), 64) / 16 * 16; };
    const int64_t use_ring = env_i64("VNM_PART_RING", 7);   // bit 0: level 1, bit 1: level 2, bit 2: level 2 of 512 partitions
    const bool ring_ok = !p->wide && !a.has_expr && !h->pring_off && use_ring != 0 && (a.keys[0].offset & 1) == 0 && (!h->plan.n_cols || (a.cols[0].offset & 1) == 0) &&
                         (!h->pred_set || a.hot_pred_is_v || (a.pred.offset & 1) == 0) && h->plan.n_cols > 0;
    // (... and at least 128: a sub-tile's 4096 entries must fit the rings' free room in one or two rounds -- 8 rings of 64 entries took 8)
    p->ring1 = ring_ok && np1 <= 256 && np1 >= 128 && (use_ring & 1);
    p->ring2 = ring_ok && p->levels == 2 && np2 <= 256 && np2 >= 128 && (use_ring & 2);
    p->ring2_512 = ring_ok && p->levels == 2 && np2 == 512 && (use_ring & 4);
    if (p->ring1) { p->rcap1 = ring_cap(np1); p->rlds1 = (size_t)np1 * p->rcap1 * 16; }
    if (p->ring2 || p->ring2_512) { p->rcap2 = ring_cap(np2); p->rlds2 = (size_t)np2 * p->rcap2 * 16; }
    return 0;
}

struct HashBuffers : AttemptBlocks {
    unsigned long long* flags = nullptr;                // [0] failure, [1] groups written, [2] entries spilled
    ulonglong2* e1 = nullptr; uint32_t* c1 = nullptr;   // regions of level 1: entries, counts
    ulonglong2* e2 = nullptr; uint32_t* c2 = nullptr;   // ... of level 2
    ulonglong2* spill = nullptr;                        // entries that did not fit their region: the caller's on success (wide: [spill_cap][E] words)
    uint64_t* rk = nullptr; uint64_t* ra = nullptr; unsigned long long* dir = nullptr;   // the run the final pass writes, its partition directory
    // once the final pass has read them: the regions and the flags go back before the hand-over (folding a run allocates)
    void release_regions() { for (void* blk : {(void*)e1, (void*)c1, (void*)e2, (void*)c2, (void*)flags}) pool.done(blk); }
};
// After a scatter level.  A region overflowed (skewed keys, or more rows per partition than the hint implied): stop here (2).  Carrying
// on would aggregate partitions that are about to be thrown away -- and the partition holding a heavy key is processed by ONE workgroup
// (measured: 1.6 s for 1e8 rows with a power-law key distribution).  ATTEMPT_REDO: it went through the rings, which have no spill buffer.
int hash_check_overflow(const HashBuffers& b, bool rings, hipStream_t s) {
    unsigned long long f = 0;
    if (hipMemcpyAsync(&f, b.flags, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return set_error("aggregate: partition pass failed");
    return !f ? 0 : (rings ? ATTEMPT_REDO : 2);
}
// what the arguments of both scatter levels share
PartArgs hash_part_args(const vnm_agg* h, const AggArgs& a, const HashPlan& p, const HashBuffers& b) {
    PartArgs x{};
    x.nval = h->plan.n_cols; x.has_vmask = a.part_vmask; x.flags = b.flags; x.debug = (int)env_i64("VNM_PART_DEBUG", 0);
    x.spill = b.spill; x.spill_cap = p.spill_cap;
    return x;
}

// Stage 2: scatter level 1 (takes its blocks), rows -> np1 partitions by the top hash bits.
int hash_scatter1(const vnm_agg* h, const AggArgs& a, int64_t nrows, const HashPlan& p, HashBuffers& b, hipStream_t s) {
    b.take(b.flags, 64); b.take(b.e1, (size_t)p.np1 * p.grid1 * p.cap1 * p.ebytes); b.take(b.c1, (size_t)p.np1 * p.grid1 * 4);
    if (!b.flags || !b.e1 || !b.c1) return 1;
    VNM_HIP(hipMemsetAsync(b.flags, 0, 64, s));
    if (p.spill_cap) b.take(b.spill, (size_t)p.spill_cap * (p.wide ? p.ebytes : 16));
    if (p.spill_cap && !b.spill) return 1;
    PartArgs p1 = hash_part_args(h, a, p, b);
    p1.kp = (const uint64_t*)a.keys[0].values + a.keys[0].offset;
    p1.vp = h->plan.n_cols ? (const double*)a.cols[0].values + a.cols[0].offset : (const double*)p1.kp;
    p1.has_expr = a.has_expr; p1.expr = a.expr;
    fill_pred(p1, h, a);
    p1.nrows = nrows; p1.nparts = p.np1; p1.shift = 32 - p.lg1;
    p1.out_entries = b.e1; p1.out_counts = b.c1; p1.out_cap = p.cap1;
    if (p.wide) {
        for (int c = 0; c < h->plan.n_cols; c++) p1.vcols[c] = a.cols[c];
        p1.wp = a.p; p1.wpred = a.pred;
    }
    {
        KernelTimer timer("agg_part_scatter1", s);
        if (p.ring1) VNM_TRY(pick_bool(p1.has_pred && !p1.pred_is_v, [&](auto pv) { return launch_dyn(pring_scatter_kernel<true, 2, 16, decltype(pv)::value>, p.grid1, PT_BLOCK, p.rlds1, s, p1, p.rcap1); }));
        else if (!p.wide) part_scatter_kernel<true><<<p.grid1, PT_BLOCK, 0, s>>>(p1);
        else VNM_TRY((pick_int<1, 7>(p.E, [&](auto e) { return launch_dyn(part_scatter_wide_kernel<true, decltype(e)::value, pw_items(decltype(e)::value)>, p.grid1, PT_BLOCK, (size_t)pw_tile(p.E) * p.ebytes, s, p1); })));
    }
    VNM_HIP(hipGetLastError());
    return hash_check_overflow(b, p.ring1, s);
}

// Stage 3: scatter level 2 (takes its blocks), every first-level partition -> np2 partitions by the hash bits [23:15] (pass 1 used [31:24]).
int hash_scatter2(const vnm_agg* h, const AggArgs& a, const HashPlan& p, HashBuffers& b, hipStream_t s) {
    b.take(b.e2, (size_t)p.np1 * p.np2 * p.split2 * p.cap2 * p.ebytes); b.take(b.c2, (size_t)p.np1 * p.np2 * p.split2 * 4);
    if (!b.e2 || !b.c2) return 1;
    PartArgs p2 = hash_part_args(h, a, p, b);
    p2.in_entries = b.e1; p2.in_counts = b.c1; p2.in_cap = p.cap1; p2.in_regions = p.grid1; p2.in_split = p.split2;
    p2.out_entries = b.e2; p2.out_counts = b.c2; p2.out_cap = p.cap2;
    p2.nparts = p.np2; p2.shift = 15;
    {
        KernelTimer timer("agg_part_scatter2", s);
        const int g2 = p.np1 * p.split2;
        const int np2 = p.np2; const size_t ebytes = p.ebytes;
        if (p.ring2) VNM_TRY(launch_dyn(pring_scatter_kernel<false, 2, 16, false>, g2, PT_BLOCK, p.rlds2, s, p2, p.rcap2));
        else if (p.ring2_512) VNM_TRY(launch_dyn(pring_scatter_kernel<false, 1, 8, false>, g2, PT_BLOCK, p.rlds2, s, p2, p.rcap2));
        else if (!p.wide) part_scatter_kernel<false><<<g2, PT_BLOCK, 0, s>>>(p2);
        else VNM_TRY((pick_int<1, 7>(p.E, [&](auto e) {   // (one- and two-word entries: 8 items per lane only where the level has many sub-partitions)
            constexpr int EW = decltype(e)::value;
            if constexpr (EW <= 2) { if (np2 < 128) return launch_dyn(part_scatter_wide_kernel<false, EW, 4>, g2, PT_BLOCK, (size_t)PT_BLOCK * 4 * ebytes, s, p2); }
            return launch_dyn(part_scatter_wide_kernel<false, EW, pw_items(EW)>, g2, PT_BLOCK, (size_t)PT_BLOCK * pw_items(EW) * ebytes, s, p2);
        })));
    }
    VNM_HIP(hipGetLastError());
    return hash_check_overflow(b, p.ring2 || p.ring2_512, s);
}

// Stage 4: how the final pass writes -- after the scatters, because it goes by what the handle holds NOW.
void hash_plan_final(const vnm_agg* h, int64_t nrows, HashPlan& p) {
    const int cus = device_info().num_cus;
    // few final partitions cannot fill the chip with one workgroup each: split them and merge through the HBM table
    p.splits = p.nfin < (int64_t)cus * 4 ? std::min((int)std::min<int64_t>(256, ((int64_t)cus * 8 + p.nfin - 1) / p.nfin), p.fin_regions) : 1;
    // ... which is only legal while the table holds nothing else (a failed attempt is then simply dropped).  With groups already in
    // the table -- every batch of a stream after the first -- the split workgroups write their PARTIAL groups (a key may appear once
    // per split) into a dense run instead, which is folded into the table like any other run: no flush storms for streamed input
    // with 2.4 K ... 900 K groups (ADVICE r01).
    p.to_table = p.splits > 1 && !(h->have_table || h->have_run);
    p.dup_run = p.splits > 1 && !p.to_table;
    // dense output sized from the hint (guarded in the kernel)
    p.dstride = p.to_table ? 2 : std::min<int64_t>(nrows, (h->hint * 2 + (1 << 20)) * (p.dup_run ? p.splits : 1)) + 2;
}

// Stage 5: the final pass (takes the run and its directory), one LDS hash table per (share of a) partition.
int hash_final(vnm_agg* h, const AggArgs& a, int64_t nrows, const HashPlan& p, HashBuffers& b, hipStream_t s) {
    const int cus = device_info().num_cus;
    b.take(b.rk, (size_t)p.dstride * 8 * 2); b.take(b.ra, (size_t)p.dstride * 8 * h->plan.n_words);
    if (!b.rk || !b.ra) return 1;
    if (!p.to_table && !p.dup_run) b.take(b.dir, (size_t)p.nfin * 16);   // the partition directory only describes runs with ONE workgroup per partition
    if (!p.to_table && !p.dup_run && !b.dir) return 1;
    PartAggArgs pa{};
    pa.dir = b.dir; pa.splits = p.splits; pa.to_table = p.to_table;
    if (p.to_table) {
        VNM_TRY(ensure_table(h, nrows, s));
        // every resident workgroup may pass the room check and then insert a full LDS table at once
        const int64_t g3max = std::min<int64_t>(p.nfin * p.splits, (int64_t)cus * 4);
        const uint64_t want = pow2_at_least(std::max<uint64_t>((uint64_t)h->hint * 4 + 8192, (uint64_t)(g3max * PA_SLOTS * 2)));
        if (h->g.cap < want) VNM_TRY(table_grow(h, want, s));
        pa.g = h->g;
        pa.table_limit = (int64_t)(h->g.cap * 8 / 10) - g3max * PA_SLOTS;
    }
    const bool two = p.levels == 2;   // the last level's regions
    pa.entries = two ? b.e2 : b.e1; pa.counts = two ? b.c2 : b.c1; pa.cap = two ? p.cap2 : p.cap1; pa.regions = p.fin_regions; pa.nfinal = p.nfin;
    pa.w_rows = a.hot_w_rows; pa.w_valid = a.hot_w_valid; pa.w_sum = a.hot_w_sum; pa.n_words = h->plan.n_words;
    pa.w_lo = a.hot_comp && a.hot_w_sum >= 0 ? a.hot_w_sum + 1 : -1; pa.comp = a.hot_comp;
    pa.dkey = b.rk; pa.dacc = b.ra; pa.dstride = p.dstride; pa.flags = b.flags;
    KernelTimer timer("agg_part_final", s);
    if (!a.part_generic) return launch_part_final(part_agg_kernel, p.nfin * p.splits, 0, s, pa);
    pa.n_ops = h->plan.n_ops; pa.nval = h->plan.n_cols; pa.vtype = a.part_vtype; pa.has_vmask = a.part_vmask;
    pa.slots = p.pa_slots; pa.ent_words = p.E; pa.wide = p.wide;
    for (int o = 0; o < h->plan.n_ops; o++) pa.ops[o] = h->plan.ops[o];
    for (int w = 0; w < h->plan.n_words; w++) pa.merge[w] = h->plan.merge[w];
    for (int c = 0; c < 6; c++) pa.vtypes[c] = a.part_vtypes[c];
    const size_t lds_bytes = (size_t)(p.pa_slots + 1) * 8 * (1 + h->plan.n_words);
    pa.w_rows_g = -1;
    pa.use_table = getenv("VNM_AGG_NO_PART_TABLE") == nullptr;
    // 6 bits per AccKind and column: the word its op accumulates in, 63 = none (dgen_program: ONE column, LDS places, COUNT(*) first)
    for (int c = 0; c < 6; c++) pa.wpack[c] = ~0ULL;
    for (int o = 0; o < h->plan.n_ops && pa.use_table; o++) {
        const AccOp& op = h->plan.ops[o];
        if (op.kind == A_COUNT_ROWS) { if (pa.w_rows_g >= 0) pa.use_table = 0; pa.w_rows_g = op.word; continue; }
        const int c = op.col < 0 ? 0 : op.col;
        if (c > 5 || op.kind < 0 || op.kind > A_MAX || op.word >= 63 || ((pa.wpack[c] >> (6 * op.kind)) & 63ULL) != 63) { pa.use_table = 0; break; }
        pa.wpack[c] = (pa.wpack[c] & ~(63ULL << (6 * op.kind))) | ((unsigned long long)op.word << (6 * op.kind));
    }
    return pick_int<1, 7>(p.E, [&](auto e) {
        return pick_bool(pa.use_table != 0, [&](auto t) { return launch_part_final(part_agg_generic_kernel<decltype(e)::value, decltype(t)::value>, p.nfin * p.splits, lds_bytes, s, pa); });
    });
}

// Stage 6.  0 = done, 3 = more groups than hinted / spill buffer full (only the final pass fails so: more partitions would do).
int hash_hand_over(vnm_agg* h, const HashPlan& p, HashBuffers& b, hipStream_t s, ulonglong2** spill_out, int64_t* n_spill_out) {
    VNM_HIP(hipGetLastError());
    unsigned long long fl[3]; VNM_TRY(read_flags(fl, b.flags, s));
    b.release_regions();
    if (fl[0] && p.to_table) { table_free(&h->g); h->have_table = false; }  // drop the partial merge
    if (fl[0]) return 3;   // use the general path for this batch
    if (spill_out) {
        if (fl[2]) { b.pool.keep(b.spill); *spill_out = b.spill; *n_spill_out = (int64_t)fl[2]; }   // the caller owns it now
        else { *spill_out = nullptr; *n_spill_out = 0; }
    }
    if (p.to_table) return 0;  // the groups already live in the HBM table
    b.pool.keep(b.rk); b.pool.keep(b.ra); b.pool.keep(b.dir);
    adopt_run(h, b.rk, b.ra, p.dstride, (int64_t)fl[1], b.dir, b.dir ? p.nfin : 0);
    // keys repeat inside a dup_run: it must never be handed out as a result, fold it into the table now
    return p.dup_run && merge_run_into_table(h, s) ? 1 : 0;
}

// The driver.  returns 0 = done (run stored), 2 = not applicable / overflowed (caller uses the general path), 3 = hint too small, 1 = error
// spill_out / n_spill_out (optional): entries that did not fit their partition region (heavy keys); the caller
// aggregates them with agg_hot_kernel<FROM_ENT> and owns the buffer.  Without them a full region fails the attempt.
int partitioned_aggregate(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s, ulonglong2** spill_out = nullptr, int64_t* n_spill_out = nullptr) {
    HashPlan p{};
    VNM_TRY(plan_hash_partitions(h, a, nrows, spill_out != nullptr, &p));
    HashBuffers b;
    // a level's rings failed (a full region, a heavy key): the same batch once more without them, the blocks back in the pool first
    auto redo = [&](const char* level) {
        h->pring_off = true;
        route_note("hash_partitions:rings_failed", "%sa region overflowed or a sub-tile needed too many rounds: the tile-sorting scatter takes the batch and every later one", level);
        b.free_all();
        return partitioned_aggregate(h, a, nrows, s, spill_out, n_spill_out);
    };
    int rc = hash_scatter1(h, a, nrows, p, b, s);
    if (rc) return rc == ATTEMPT_REDO ? redo("") : rc;
    if (p.ring1) route_note("hash_partitions:rings", "%d x %d partitions: (key, value) entries through LDS rings, whole 256-byte blocks out", p.np1, p.np2);
    if (p.levels == 2) {
        rc = hash_scatter2(h, a, p, b, s);
        if (rc) return rc == ATTEMPT_REDO ? redo("level 2: ") : rc;
    }
    hash_plan_final(h, nrows, p);
    VNM_TRY(hash_final(h, a, nrows, p, b, s));
    return hash_hand_over(h, p, b, s, spill_out, n_spill_out);
}

// ---- dense-key partitioned path: host side (kernels in vnm_agg_dense.inc) ------------------------------------
// Sample the key range of the first large batch and derive the code map.  dense_state = 1 when the (widened) range fits
// DP_MAX_BITS bits and is large enough to fill the chip with final partitions.
int plan_dense_from_range(vnm_agg* h, int key_type, uint64_t got0, uint64_t got1);
int plan_dense(vnm_agg* h, const vnm_dcol& key, int64_t nrows, hipStream_t s) {
    if (h->range_given) return 0;   // vnm_agg_set_dense_range: the map stays the one all ranks derived
    h->dense_state = -1;
    if (key.type != VNM_I64 && key.type != VNM_U64) return 0;
    const uint64_t sign = key.type == VNM_I64 ? 0x8000000000000000ULL : 0ULL;
    const uint64_t* kp = (const uint64_t*)key.values + key.offset;
    unsigned long long* d = (unsigned long long*)pool_alloc(64);
    if (!d) return 1;
    const unsigned long long init[2] = {~0ULL, 0ULL};
    unsigned long long got[2];
    VNM_HIP(hipMemcpyAsync(d, init, 16, hipMemcpyHostToDevice, s));
    const int64_t m = std::min<int64_t>(nrows, 1 << 18);
    const int grid = (int)std::min<int64_t>((m + 255) / 256, (int64_t)device_info().num_cus * 4);
    dense_sample_range_kernel<<<grid, 256, 0, s>>>(kp, nrows, m, sign, d, h->kn_valid, h->kn_off);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(got, d, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    pool_free(d);
    if (got[0] > got[1]) return 0;
    return plan_dense_from_range(h, key.type, got[0], got[1]);
}

// The code map from a (sampled) key range [got0, got1] of order-preserving unsigned images.
int plan_dense_from_range(vnm_agg* h, int key_type, uint64_t got0, uint64_t got1) {
    h->dense_state = -1;
    if (key_type != VNM_I64 && key_type != VNM_U64) return 0;
    const uint64_t sign = key_type == VNM_I64 ? 0x8000000000000000ULL : 0ULL;
    const unsigned long long got[2] = {got0, got1};
    // widen by 1/8 of the sampled span on both sides (the sample misses the true extremes), then centre the range in
    // the next power of two
    const uint64_t span_s = got[1] - got[0];
    if (span_s >= (1ULL << DP_MAX_BITS)) return 0;
    // (small ranges: a tighter margin, so that up to ~7000 sampled codes still fit the 2^13-slot scan table)
    const uint64_t margin = span_s < (1ULL << 13) ? span_s / 16 + 64 : span_s / 8 + 4096;
    uint64_t lo = got[0] > margin ? got[0] - margin : 0;
    uint64_t hi = got[1] < ~0ULL - margin ? got[1] + margin : ~0ULL;
    int bits = 1;
    while (bits < 64 && ((hi - lo) >> bits) != 0) bits++;
    if (bits > DP_MAX_BITS) return 0;
    // ranges below 2^20 leave too few final partitions to fill the chip with one workgroup each: their final pass splits
    // every partition over several workgroups and merges the partial tables (dpart_merge_kernel).  Up to 2^13 codes need
    // no partitioning at all (dense_state = 2).
    h->dense_rlo = lo; h->dense_rhi = hi;
    const bool small = bits < (int)env_i64("VNM_DENSE_MIN_BITS", 14);   // at most 2^13 codes: the direct-addressed LDS scan (dscan_kernel)
    if (small) bits = DP_TBITS_MAX;   // always the 2^13-slot table: one 1024-thread workgroup per CU measured fastest at every G
                                      // (G = 300 / 1000: 2.83 / 2.84 ms; 2^12 slots, two 512-thread workgroups: 3.04 / 3.07; 2^11, four: 3.50 / 3.65)
    const uint64_t extra = ((1ULL << bits) - 1) - (hi - lo);
    lo = lo > extra / 2 ? lo - extra / 2 : 0;
    DenseMap& mp = h->dmap;
    mp.lo_u = lo;
    mp.sign = sign;
    mp.bits = bits;
    mp.mask = (uint32_t)((1ULL << bits) - 1);
    mp.mul = (uint32_t)((double)(1ULL << bits) * 0.6180339887498949) | 1u;  // Fibonacci hashing on `bits` bits
    uint32_t inv = mp.mul;                                                     // Newton: inverse modulo 2^32
    for (int it = 0; it < 5; it++) inv *= 2u - mp.mul * inv;
    mp.mul_inv = inv;
    h->dense_span = (int64_t)1 << bits;
    h->dense_state = small ? 2 : 1;
    return 0;
}

// Generic accumulator programs on the dense paths (dgen_* kernels): every AccKind at most once over at most one plain
// 8-byte input column, at most one COUNT(*) word (it lives in the slot's row counter).  Fills the program part of `g`;
// false = not expressible.
bool dgen_program(const vnm_agg* h, const AggArgs& a, DGenArgs* g) {
    const AggPlan& p = h->plan;
    if (p.n_cols > 1 || p.n_words > AGG_MAX_WORDS) return false;
    g->has_val = p.n_cols == 1;
    g->vtype = p.n_cols == 1 ? a.cols[0].type : VNM_F64;
    g->comp = 0;
    g->wpack = ~0ULL;
    g->n_words = p.n_words;
    int w_rows = -1;
    for (int o = 0; o < p.n_ops; o++) {
        const AccOp& op = p.ops[o];
        if (op.kind == A_COUNT_ROWS) { if (w_rows >= 0) return false; w_rows = op.word; }
    }
    int n_lds = 0;
    for (int w = 0; w < p.n_words; w++) {
        g->merge[w] = p.merge[w];
        g->lds_word[w] = w == w_rows ? -1 : n_lds++;
        if (p.merge[w] == M_ADD_F64C) g->comp = 1;
    }
    if (n_lds > DG_MAX_WORDS - 1) return false;
    g->n_lds = n_lds;
    for (int o = 0; o < p.n_ops; o++) {
        const AccOp& op = p.ops[o];
        if (op.kind == A_COUNT_ROWS) continue;
        if (op.col != 0 || op.kind < 0 || op.kind > A_MAX || op.word >= 63 || ((g->wpack >> (6 * op.kind)) & 63ULL) != 63) return false;
        g->wpack = (g->wpack & ~(63ULL << (6 * op.kind))) | ((unsigned long long)g->lds_word[op.word] << (6 * op.kind));
    }
    // a compensated sum's lo word must follow its hi word in LDS as well
    for (int w = 0; w + 1 < p.n_words; w++)
        if (p.merge[w] == M_ADD_F64C && (g->lds_word[w] < 0 || g->lds_word[w + 1] != g->lds_word[w] + 1)) return false;
    return true;
}
// bytes of LDS per slot of a generic table
inline int dgen_slot_bytes(const DGenArgs& g) { return 8 * g.n_lds + 4; }

int upload_segs(vnm_agg* h, int64_t tile, const VSeg** dev, int* nseg, int64_t* ntiles, PoolScope& pool, hipStream_t s);
// ---- ranges of at most 2^13 codes: one scan with the whole table in LDS, no scatter ----------------------------------------------
// dense_scan_generic: any program dgen_program can express, a run of its own; dense_scan_stream: the hot program, into the stream's table.
// Same return convention as the partitioned variant.  Their code map: the plain code, no Fibonacci mix; false = not a small range.
inline bool dense_scan_map(const vnm_agg* h, DenseMap* map) { *map = h->dmap; map->mul = 1; map->mul_inv = 1; return h->dmap.bits == DP_TBITS_MAX; }
// the largest table (<= 2^13 slots) that fits 144 KB of LDS must hold the sampled range (2: it does not), centred in a smaller one
int plan_scan_generic(const vnm_agg* h, DGenArgs* g) {
    int tb = DP_TBITS_MAX;
    while (tb > 9 && ((size_t)dgen_slot_bytes(*g) << tb) > 144 * 1024) tb--;
    const uint64_t need = h->dense_rhi - h->dense_rlo;
    if (need >= (1ULL << tb)) return 2;
    if (tb != DP_TBITS_MAX) {
        const uint64_t extra = ((1ULL << tb) - 1) - need;
        g->map.lo_u = h->dense_rlo > extra / 2 ? h->dense_rlo - extra / 2 : 0;
        g->map.bits = tb;
        g->map.mask = (uint32_t)((1ULL << tb) - 1);
    }
    g->tbits = tb;
    return 0;
}

// (nspill_out / n_nspill_out: keys of NULL-value rows, a nullable value column; without them such a column is not taken)
int dense_scan_generic(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s, ulonglong2** spill_out, int64_t* n_spill_out, uint64_t** nspill_out, int64_t* n_nspill_out) {
    DenseMap map;
    if (!dense_scan_map(h, &map)) return 2;
    if (nspill_out) { *nspill_out = nullptr; *n_nspill_out = 0; }
    DGenArgs g{};
    if (!dgen_program(h, a, &g)) return 2;
    const bool vn = g.has_val && a.cols[0].validity != nullptr;   // nullable value column
    if (vn && !nspill_out) return 2;
    g.map = map;
    VNM_TRY(plan_scan_generic(h, &g));
    const int block = 1024, slots = 1 << g.tbits;
    const size_t lds = (size_t)slots * dgen_slot_bytes(g);
    const int grid = (int)std::min<int64_t>((int64_t)device_info().num_cus * (lds <= 72 * 1024 ? 2 : 1), std::max<int64_t>(1, (nrows / 2 + block - 1) / block));
    const int64_t spill_cap = nrows / 2 + (1 << 20), nspill_cap = vn ? nrows / 4 + (1 << 20) : 0, dstride = slots + 2;
    AttemptBlocks b;
    unsigned long long* flags; uint64_t *pw, *rk, *ra, *nspill = nullptr; uint32_t* pc; ulonglong2* spill;
    b.take(flags, 64); b.take(pw, std::max<size_t>(8, (size_t)grid * g.n_lds * slots * 8)); b.take(pc, (size_t)grid * slots * 4);
    b.take(spill, (size_t)spill_cap * 16); if (vn) b.take(nspill, (size_t)nspill_cap * 8);
    b.take(rk, (size_t)dstride * 8 * 2); b.take(ra, (size_t)dstride * 8 * std::max(1, h->plan.n_words));
    if (!flags || !pw || !pc || !spill || !rk || !ra || (vn && !nspill)) return 1;
    VNM_HIP(hipMemsetAsync(flags, 0, 64, s));
    g.kp = (const uint64_t*)a.keys[0].values + a.keys[0].offset;
    g.vp = g.has_val ? (const double*)a.cols[0].values + a.cols[0].offset : nullptr;
    fill_pred(g, h, a);
    g.nrows = nrows; g.spill = spill; g.spill_cap = spill_cap;
    if (vn) { g.vvalid = a.cols[0].validity; g.voff = a.cols[0].offset; g.nspill = nspill; g.nspill_cap = nspill_cap; }
    g.dkey = rk; g.dacc = ra; g.dstride = dstride; g.flags = flags;
    g.nfinal = 1; g.splits = grid; g.part_w = pw; g.part_cnt = pc;
    {
        KernelTimer timer("agg_scan", s);
        VNM_TRY(pick_bool(g.has_val != 0, [&](auto hv) {
            if constexpr (decltype(hv)::value) { if (vn) return launch_dyn(dgen_scan_kernel<true, true>, grid, block, lds, s, g); }
            return launch_dyn(dgen_scan_kernel<decltype(hv)::value>, grid, block, lds, s, g);
        }));
        dgen_merge_kernel<<<std::max(1, slots / 512), 512, 0, s>>>(g);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long fl[4]; VNM_TRY(read_flags(fl, flags, s));
    if (fl[0]) return 2;
    if (fl[2]) { b.pool.keep(spill); *spill_out = spill; *n_spill_out = (int64_t)fl[2]; }
    else { *spill_out = nullptr; *n_spill_out = 0; }
    if (vn && fl[3]) { b.pool.keep(nspill); *nspill_out = nspill; *n_nspill_out = (int64_t)fl[3]; }
    if ((int64_t)(fl[2] + fl[3]) > nrows / 16) h->dense_state = -1;
    b.pool.keep(rk); b.pool.keep(ra);
    adopt_run(h, rk, ra, dstride, (int64_t)fl[1]);
    return 0;
}

// The table a stream of small-range batches accumulates in, empty (h->scan_pending).
int scan_pending_create(vnm_agg* h, const DenseMap& map, const AggArgs& a, hipStream_t s) {
    const int cus = device_info().num_cus, slots = 1 << DP_TBITS_MAX;
    std::unique_ptr<DScanPending> sp(new DScanPending());
    sp->slots = slots; sp->df.map = map;
    sp->df.w_rows = a.hot_w_rows; sp->df.w_valid = a.hot_w_valid; sp->df.w_sum = a.hot_w_sum;
    sp->df.w_lo = a.hot_comp && a.hot_w_sum >= 0 ? a.hot_w_sum + 1 : -1;
    sp->t.sum = (double*)pool_alloc((size_t)slots * 8); sp->t.lo = (double*)pool_alloc((size_t)slots * 8);
    sp->t.cnt = (unsigned long long*)pool_alloc((size_t)slots * 8);
    sp->part_sum = (uint64_t*)pool_alloc((size_t)cus * slots * 8);
    sp->part_lo = (float*)pool_alloc((size_t)cus * slots * 4); sp->part_cnt = (uint32_t*)pool_alloc((size_t)cus * slots * 4);
    sp->flags = (unsigned long long*)pool_alloc(64);
    if (!sp->t.sum || !sp->t.lo || !sp->t.cnt || !sp->part_sum || !sp->part_lo || !sp->part_cnt || !sp->flags) return 1;
    fill_u64_kernel<<<(slots + 255) / 256, 256, 0, s>>>((uint64_t*)sp->t.sum, F64_NEG_ZERO, (int64_t)slots);   // (sums start at -0.0: merge_init)
    if (hipGetLastError() != hipSuccess || hipMemsetAsync(sp->t.lo, 0, (size_t)slots * 8, s) != hipSuccess ||
        hipMemsetAsync(sp->t.cnt, 0, (size_t)slots * 8, s) != hipSuccess) return set_error("aggregate: memset of the stream table failed");
    h->scan_pending = sp.release();
    return 0;
}

// The batch's per-workgroup tables are added into the table of the STREAM (h->scan_pending, dscan_accumulate_kernel); the groups
// are written when something else needs them (flush_scan_pending).  59 x 2^24-row batches, G = 1000: 17.1 -> 5.5 ms per 1e9 rows.
int dense_scan_stream(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s, ulonglong2** spill_out, int64_t* n_spill_out) {
    DenseMap map;
    if (!dense_scan_map(h, &map)) return 2;
    const int block = 1024, slots = 1 << DP_TBITS_MAX;   // always the 2^13-slot table, one workgroup per CU
    const int grid = (int)std::min<int64_t>((int64_t)device_info().num_cus, std::max<int64_t>(1, (nrows / 2 + block - 1) / block));
    if (h->scan_pending && memcmp(&h->scan_pending->df.map, &map, sizeof(DenseMap)) != 0) VNM_TRY(flush_scan_pending(h, s));
    if (!h->scan_pending) VNM_TRY(scan_pending_create(h, map, a, s));
    DScanPending* sp = h->scan_pending;
    const int64_t spill_cap = nrows / 2 + (1 << 20);
    ulonglong2* spill = (ulonglong2*)pool_alloc((size_t)spill_cap * 16);
    if (!spill) return 1;
    PoolSlotGuard<ulonglong2> spill_guard(&spill);
    VNM_HIP(hipMemsetAsync(sp->flags, 0, 64, s));
    DScanArgs d{}; d.map = map;
    d.kp = (const uint64_t*)a.keys[0].values + a.keys[0].offset;
    d.vp = (const double*)a.cols[0].values + a.cols[0].offset;
    d.has_expr = a.has_expr; d.expr = a.expr;
    fill_pred(d, h, a);
    d.nrows = nrows; d.comp = a.hot_comp && a.hot_w_sum >= 0;
    d.part_sum = sp->part_sum; d.part_lo = sp->part_lo; d.part_cnt = sp->part_cnt;
    d.flags = sp->flags; d.spill = spill; d.spill_cap = spill_cap;
    PoolScope seg_pool;
    if (h->segs_active) {   // the waiting batches of a stream: one launch (round 5; 59 launches + 59 table merges were 5.3 of the 6.3 ms at G = 1000)
        int64_t ntiles = 0;
        if (a.has_expr || upload_segs(h, (int64_t)1 << 20, &d.segs, &d.nseg, &ntiles, seg_pool, s)) return 1;
    }
    unsigned long long fl[3];
    {
        KernelTimer timer("agg_scan", s);
        dscan_kernel<DP_TBITS_MAX><<<grid, block, 0, s>>>(d);
        VNM_HIP(hipGetLastError());
        VNM_TRY(read_flags(fl, sp->flags, s));
        if (fl[0]) return 2;   // spill buffer full or a compensation term beyond float range: the batch goes another way, the stream's table is untouched
        // (segments: keys outside the sampled range would have to go through the scan as entries of their own while the segment table is
        // in force -- rare enough to send the batches another way instead, before anything has been added to the stream's table)
        if (h->segs_active && fl[2]) { h->dense_state = -1; return 2; }
        dscan_accumulate_kernel<<<slots / 64, 512, 0, s>>>(sp->part_sum, sp->part_lo, sp->part_cnt, grid, slots, sp->t);
        VNM_HIP(hipGetLastError());
    }
    if (fl[2]) { *spill_out = spill; *n_spill_out = (int64_t)fl[2]; spill = nullptr; }
    else { *spill_out = nullptr; *n_spill_out = 0; }
    if ((int64_t)fl[2] > nrows / 16) h->dense_state = -1;  // the sampled range does not describe the data: stop trying
    return 0;
}

// The plain (one workgroup per partition) final pass of the dense path in one of its output modes.
enum { DFF_LEAN, DFF_FIXED, DFF_LO64, DFF_EXACT, DFF_PLAIN };   // its forms; which (TB, OUT) a form has kernels for is the `if constexpr` in front of it
template <int TB, int OUT>
int launch_dense_final_as(int form, const DFinalArgs& df, const DSet* only_set, hipStream_t s) {
    constexpr int blk = TB >= 13 ? 1024 : (TB == 12 ? VNM_DF12_BLOCK : 512);
    constexpr int OUT_RC = OUT == DF_COLS ? DF_COLS : DF_RUN;   // the forms that have no DF_TABLE kernel
    const int occ_max = (int)env_i64("VNM_PA_OCC", 8);
    switch (form) {
    case DFF_LEAN: {   // (the grid goes by the occupancy of the form without narrow words or side table, whichever runs)
        constexpr int lean_blk = TB >= 13 ? 1024 : 512;
        return pick_bool(df.fx_w32 != 0, [&](auto w32) {
            if constexpr (OUT != DF_TABLE) {
                if (df.has_side) return launch_resident_as(dfx_final_kernel<TB, OUT, decltype(w32)::value, true>, dfx_final_kernel<TB, OUT>, df.nfinal, lean_blk, 0, occ_max, s, df, *only_set);
            }
            return launch_resident_as(dfx_final_kernel<TB, OUT, decltype(w32)::value>, dfx_final_kernel<TB, OUT>, df.nfinal, lean_blk, 0, occ_max, s, df, *only_set);
        });
    }
    case DFF_FIXED:   // fixed-point entry words: integer sums
        return launch_resident(dpart_final_kernel<uint16_t, TB, false, OUT, float, true, true>, df.nfinal, blk, 0, occ_max, s, df);
    case DFF_LO64:    // compensation terms beyond the float range (|sum| > ~1e54): 64-bit terms, tables of at most 2^12 slots
        if constexpr (TB >= 9 && TB <= 12) return launch_resident(dpart_final_kernel<uint16_t, TB, false, OUT_RC, double>, df.nfinal, blk, 0, occ_max, s, df);
        break;
    case DFF_EXACT:   // every add proved exact: {sum, count} slots, non-returning atomics
        if constexpr (TB >= 12) return launch_resident(dpart_final_kernel<uint16_t, TB, false, OUT_RC, float, true>, df.nfinal, blk, 0, occ_max, s, df);
        break;
    default:
        if constexpr (TB >= 9) return launch_resident(dpart_final_kernel<uint16_t, TB, false, OUT, float>, df.nfinal, blk, 0, occ_max, s, df);
        break;
    }
    return set_error("aggregate: no dense final pass of form %d for tables of 2^%d slots (internal error)", form, TB);
}
int launch_dense_final(const DFinalArgs& df, int tb, int out, bool lo64, hipStream_t s, bool exact = false, const DSet* only_set = nullptr) {
    KernelTimer timer("agg_part_final", s);
    int form = DFF_PLAIN, tbk = tb;
    // fixed-point words of ONE batch in large regions, no side table: the lean kernel (dfx_final_kernel)
    if (df.fx_q != 0.0 && only_set && !only_set->pad && only_set->regions > 0 && only_set->regions <= 512 && tb >= 7 && tb <= 13 &&
        (!df.has_side || (out != DF_TABLE && env_i64("VNM_DFX_LEAN_SIDE", 1))) && env_i64("VNM_DFX_LEAN", 1)) form = DFF_LEAN;
    else if (df.fx_q == 0.0 && lo64) {
        if (tb < 9 || tb > 12) return set_error("aggregate: no 64-bit compensation variant for this table size (internal error)");
        form = DFF_LO64;
    } else if (df.fx_q != 0.0) {
        if (tb < 7 || tb > 13) return set_error("aggregate: fixed-point entries with this table size (internal error)");
        form = DFF_FIXED;
    } else if (exact && (tb == 12 || tb == 13) && out != DF_TABLE) form = DFF_EXACT;
    else if (tb < 9 || tb > 12) tbk = 13;
    VNM_TRY((pick_int<7, 13>(tbk, [&](auto tbc) {
        return pick_out(out, [&](auto outc) { return launch_dense_final_as<decltype(tbc)::value, decltype(outc)::value>(form, df, only_set, s); });
    })));
    VNM_HIP(hipGetLastError());
    return 0;
}

// The waiting batches of a stream (h->segs_active) as the segment table of one launch whose tiles hold `tile` rows: every segment
// starts a tile of its own.  The table lives in `pool` (freed in stream order); its host copy stays in the handle until the next one.
int upload_segs(vnm_agg* h, int64_t tile, const VSeg** dev, int* nseg, int64_t* ntiles, PoolScope& pool, hipStream_t s) {
    const std::vector<vnm_agg::QBatch>& q = *h->segs_active;
    h->seg_host.resize(q.size());
    int64_t t = 0;
    for (size_t i = 0; i < q.size(); i++) {
        VSeg& g = h->seg_host[i];
        g.kp = (const uint64_t*)q[i].key.values + q[i].key.offset;
        g.vp = (const uint64_t*)q[i].col.values + q[i].col.offset;
        g.pp = h->pred_set ? (const double*)q[i].pred.values + q[i].pred.offset : nullptr;
        g.vvalid = nullptr; g.voff = 0;
        g.nrows = q[i].nrows;
        g.first_tile = t;
        t += (q[i].nrows + tile - 1) / tile;
    }
    VSeg* d = (VSeg*)pool.take(q.size() * sizeof(VSeg));
    if (!d) return 1;
    VNM_HIP(hipMemcpyAsync(d, h->seg_host.data(), q.size() * sizeof(VSeg), hipMemcpyHostToDevice, s));
    *dev = d; *nseg = (int)q.size(); *ntiles = t;
    return 0;
}

// ---- the deferred final pass of the dense path, stage by stage (complete_pending below is the driver) -------------------------
// Stage 1: where the groups go (DF_RUN: a run of `pool`'s blocks, df.dkey / df.dacc), its capacity, a fresh device copy of the sets.
int pending_bind_output(const vnm_agg* h, DensePending* pd, int out, const DFinalArgs* cols, DFinalArgs& df, PoolScope& pool, hipStream_t s) {
    if (out == DF_RUN) {
        df.dkey = (uint64_t*)pool.take((size_t)pd->dstride * 8 * 2);
        df.dacc = (uint64_t*)pool.take((size_t)pd->dstride * 8 * h->plan.n_words);
        if (!df.dkey || !df.dacc) return 1;
    } else if (out == DF_COLS) {
        df.n_out = cols->n_out; df.pack_n = cols->pack_n;
        for (int c = 0; c < cols->n_out; c++) { df.out_kind[c] = cols->out_kind[c]; df.out_ptr[c] = cols->out_ptr[c]; df.key_field[c] = cols->key_field[c]; }
        for (int j = 0; j < cols->pack_n; j++) { df.pack_shift[j] = cols->pack_shift[j]; df.pack_bits[j] = cols->pack_bits[j]; df.pack_lo[j] = cols->pack_lo[j]; }
        if (cols->has_side) { df.has_side = 1; df.side = cols->side; df.side_bloom = cols->side_bloom; df.side_bloom_mask = cols->side_bloom_mask; df.side_found = cols->side_found; }
    } else {
        if (!pd->table) pd->table = (DTabSlot*)pool_alloc(sizeof(DTabSlot) << df.map.bits);
        if (!pd->table) return 1;
        df.table = pd->table;
    }
    df.dstride = (out == DF_COLS && cols->dstride > 0) ? cols->dstride : pd->dstride;   // (capacity of the output: + the side table's groups)
    pool_free(pd->dsets);
    pd->dsets = (DSet*)pool_alloc(pd->sets.size() * sizeof(DSet));
    if (!pd->dsets) return 1;
    VNM_HIP(hipMemcpyAsync(pd->dsets, pd->sets.data(), pd->sets.size() * sizeof(DSet), hipMemcpyHostToDevice, s));
    df.sets = pd->dsets; df.nsets = (int)pd->sets.size();
    return 0;
}

// Stage 2, few final partitions: each is shared by `fsplits` workgroups (partial tables + dpart_merge_kernel).
int pending_final_split(const DensePending* pd, int out, const DFinalArgs& df, PoolScope& pool, hipStream_t s) {
    const size_t cells = (size_t)pd->nfinal * pd->fsplits << pd->tb;
    DFinalArgs ds = df; ds.splits = pd->fsplits;
    ds.part_sum = (uint64_t*)pool.take(cells * 8); ds.part_lo = (float*)pool.take(cells * 4); ds.part_cnt = (uint32_t*)pool.take(cells * 4);
    if (!ds.part_sum || !ds.part_lo || !ds.part_cnt) return 1;
    KernelTimer timer("agg_part_final", s);
    const int g3 = (int)std::min<int64_t>(pd->nfinal * pd->fsplits, (int64_t)device_info().num_cus * 8);
    pick_int<9, 13>(pd->tb >= 9 && pd->tb <= 12 ? pd->tb : 13, [&](auto tbc) {
        constexpr int TB = decltype(tbc)::value, blk = TB == 13 ? 1024 : (TB == 12 ? VNM_DF12_BLOCK : 512);
        dpart_final_kernel<uint16_t, TB, true><<<g3, blk, 0, s>>>(ds);
        return 0;
    });
    if (out != DF_COLS) ds.n_out = 0;
    dpart_merge_kernel<<<(int)(pd->nfinal << (pd->tb - 9)), 512, 0, s>>>(ds, pd->tb);
    VNM_HIP(hipGetLastError());
    return 0;
}
// Stage 2, second attempt: 64-bit compensation terms only fit 2^12-slot tables -- partitions of 2^13 slots in two halves (slot bit 12).
int pending_final_halves(DFinalArgs& df, int out, hipStream_t s) {
    df.sub_bits = 1;
    for (int sub = 0; sub < 2; sub++) { df.sub = sub; VNM_TRY(launch_dense_final(df, 12, out, true, s)); }
    return 0;
}
// Stage 2, the usual one (attempt 1: with 64-bit compensation terms): one workgroup per partition, then the side table's groups.
int pending_final_plain(const DensePending* pd, int out, int attempt, const DFinalArgs& df, hipStream_t s) {
    if (df.has_side) {
        VNM_HIP(hipMemsetAsync(df.side_found, 0, (size_t)df.side.cap + 2, s));
        VNM_HIP(hipMemsetAsync(df.flags + 4, 0, 8, s));
    }
    // every add of the pass proved exact by the scatter passes (exact_track): {sum, count} slots, non-returning atomics
    // (VNM_DF_EXACT: 0 = never, 2 = assume it without proof -- measurements only)
    const int xmode = (int)env_i64("VNM_DF_EXACT", 1);
    const bool exact = attempt == 0 && df.w_sum >= 0 && df.w_lo >= 0 && !df.sub_bits && (xmode == 2 || (xmode == 1 && pd->exact_ok()));
    if (exact) route_note("dense:exact_adds", "2^%d-slot tables without compensation words: %lld rows, values below 2^%d with lowest bits >= 2^%d", pd->tb, (long long)pd->rows, (int)pd->x_exp - 1022, (int)(0xFFFFu - pd->x_inv) - 1075);
    VNM_TRY(launch_dense_final(df, pd->tb, out, attempt == 1, s, exact, pd->sets.size() == 1 ? &pd->sets[0] : nullptr));
    if (df.has_side) {
        KernelTimer timer("agg_side_append", s);
        dside_append_kernel<<<(int)std::min<int64_t>(((int64_t)df.side.cap + 2 + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(df, 0);
        dside_append_kernel<<<1, 256, 0, s>>>(df, 1);
        VNM_HIP(hipGetLastError());
    }
    return 0;
}

// Runs the deferred final pass of the dense path.  DF_RUN: the pending state becomes the handle's run (and is released);
// DF_COLS: `cols` names the output columns (capacity pending->dstride), *n_out = groups written, the pending entries STAY (a later
// finish() can still produce the partial state); DF_TABLE: the tables go to pending->table (rc 2: compensation terms out of the
// float range -- the caller uses another exchange).
int complete_pending(vnm_agg* h, hipStream_t s, int out = DF_RUN, const DFinalArgs* cols = nullptr, int64_t* n_out = nullptr) {
    DensePending* pd = h->pending;
    if (!pd) return 0;
    if (out == DF_RUN && h->have_run) VNM_TRY(merge_run_into_table(h, s));   // (a run of another path: it has to make room)
    DFinalArgs df = pd->df;
    PoolScope pool;
    VNM_TRY(pending_bind_output(h, pd, out, cols, df, pool, s));
    if (pd->fsplits > 1 && df.has_side) return set_error("aggregate: side table with a split final pass (internal error)");
    unsigned long long fl[5] = {0, 0, 0, 0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {   // (the second: compensation terms beyond the float range)
        VNM_HIP(hipMemsetAsync(df.flags, 0, 16, s));   // [0] failure, [1] dense count ([2]: the scatter passes' spill count, consumed)
        if (attempt == 0 && pd->fsplits > 1) VNM_TRY(pending_final_split(pd, out, df, pool, s));
        else if (attempt == 1 && pd->tb == 13 && df.fx_q == 0.0) VNM_TRY(pending_final_halves(df, out, s));
        else VNM_TRY(pending_final_plain(pd, out, attempt, df, s));
        VNM_TRY(read_flags(fl, df.flags, s));
        if (!fl[0]) break;
        if (out == DF_TABLE) return 2;
        if (attempt == 1) return set_error("aggregate: dense final pass failed (internal error)");
    }
    if (getenv("VNM_AGG_TRACE")) fprintf(stderr, "[agg] dense final (deferred, %zu batch%s): mode %d -> groups %llu\n", pd->sets.size(), pd->sets.size() == 1 ? "" : "es", out, fl[1]);
    if (n_out) *n_out = (int64_t)fl[1];
    if (out == DF_COLS && cols->null_pos) *cols->null_pos = df.has_side ? (int64_t)fl[4] : 0;
    if (out == DF_RUN) {
        pool.keep(df.dkey); pool.keep(df.dacc);
        adopt_run(h, df.dkey, df.dacc, pd->dstride, (int64_t)fl[1]);
        delete pd; h->pending = nullptr;
    }
    return 0;
}

// ---- the dense-key partitioned route, stage by stage (dense_partitioned_aggregate below is the driver) ---------------------
// What one attempt does with a batch: the form of its entries and the whole geometry of the passes.  Filled by plan_dense_entries
// and plan_dense_geometry -- or, the geometry alone, by plan_dense_two -- which make no HIP call and leave the handle alone; read-only afterwards.
struct DensePlan {
    bool generic, has_val;
    bool vn, vn_lists;       // nullable value column; ... whose NULL rows may end up in a list of their own (nspill), not vn_fold
    bool fx_base;            // fixed-point entry words are an option (then the sample decides: h->fx_state)
    int tb, pbits, levels;   // 2^tb slots per final table, 2^pbits final partitions through one or two scatter levels
    int p1, p2, np1, np2;
    int64_t nfinal;
    int fsplits;             // workgroups that share a final partition (split final pass + merge kernel), 1 = none
    bool count8;             // COUNT(*) alone: one level of 512 partitions, then one- or two-byte counters over sub-ranges
    int c8_cb, c8_sub;       // ... bits of a counter; a partition of 2^c8_sub times the table's codes is read once per part
    bool fx;                 // fixed-point words, of the quantum fx_q = 2^qe (0: float64 entries)
    double fx_q;
    bool w32, w32_1;         // the LAST level's words are 32 bits; pass 1 writes 32-bit words (its only level, or the first of two: narrow1)
    bool narrow1;            // two levels, 32-bit words out of BOTH: the first level's value field is a window of 32 - (remainder bits) bits
    int fx_qe;               // the quantum of this attempt's words, 2^fx_qe: the operator's, or coarser by the bits narrow1 cannot spare
    int fx_wbits, fx_wbase;  // narrow1: bits and base of the window, in quanta of 2^fx_qe
    int grid1, split2;       // pass-1 workgroups; pass-2 workgroups per first-level partition
    int64_t cap1, cap2;      // entries per region after pass 1 / pass 2
    bool c16_1;              // pass-1 remainders fit 16 bits when they are the final slots
    int pmajor;              // VNM_DENSE_PRODUCER_MAJOR
    int64_t spill_cap, nspill_cap, dstride;
    int rcap1, rcap2;        // entries per ring of the ring scatter (0 = the tile-sorting kernel takes the level; two values: never 0)
    bool ring_limit;
    int ring_pairs1, ring_pairs2;   // pairs of rows per lane and sub-tile, at most
};

// Stage 2a: is the route applicable, and with which form of entries?  0, or 2 = not applicable.
int plan_dense_entries(const vnm_agg* h, const AggArgs& a, bool generic, const DGenArgs& g, bool vn_fold, bool null_lists, DensePlan* p) {
    p->generic = generic;
    p->has_val = generic ? g.has_val != 0 : true;
    // nullable value column: NULL flags travel with the entries (generic programs) -- or, vn_fold, the hot program filtered by that
    // column itself: pass 1 drops the NULL rows with the filter and nothing after it ever sees a flag
    if ((h->segs_active || h->kn_valid) && generic) return 2;   // (stream segments, nullable keys: the hot program's ring scatter only)
    if (h->kn_valid && h->segs_active) return 2;
    p->vn = p->has_val && a.cols[0].validity != nullptr && (generic || vn_fold);
    if (p->vn && ((!vn_fold && !null_lists) || a.has_expr)) return 2;
    if (vn_fold && (generic || !a.hot_pred_is_v)) return 2;
    p->vn_lists = p->vn && !vn_fold;
    // FIXED-POINT entries (round 6): when every value of the column is m * 2^qe with |m| < 2^31 -- integers stored as float64, halves,
    // the benchmark's k / 128 -- an entry is ONE 64-bit word (m << remainder bits | remainder): 8 bytes instead of 12 after pass 1 and 10
    // after pass 2, one region stream instead of two, integer adds in the final pass (exact by construction, no compensation words).
    // The quantum comes from a sample of the first batch; every row is checked in pass 1 (fx_encode), and one that does not fit (a
    // finer fraction, a larger magnitude, -0.0, Inf / NaN) fails the attempt: the batch is redone with float64 entries and the operator
    // never tries again.  Same result bits: the correctly rounded exact sum either way.
    // (a nullable KEY: pass 1 sums the NULL-key rows aside as ever; a nullable VALUE filtered by itself, vn_fold: the NULL rows never become entries)
    p->fx_base = !generic && p->has_val && (!p->vn || vn_fold) && !a.has_expr && !(h->kn_valid && p->vn) && a.hot_comp && a.hot_w_sum >= 0 &&
                 env_i64("VNM_DENSE_DEFER", 1) && env_i64("VNM_DENSE_FX", 1) && a.cols[0].type == VNM_F64 && (env_i64("VNM_DENSE_RING", 3) & 3) == 3;
    return 0;
}

// Stage 1: the quantum of the fixed-point words from a sample of the first batch (h->fx_state, h->fx_qe, h->fx_narrow).
int sample_fixed_point(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s) {
    h->fx_state = -1;
    PoolScope pool;
    unsigned long long* d = (unsigned long long*)pool.take(64);
    if (!d) return 1;
    unsigned long long got3[3] = {0, 0, 0};   // exact_track statistics; ~image of the smallest sampled value; image of the largest
    VNM_HIP(hipMemsetAsync(d, 0, 24, s));
    const int64_t srows = h->segs_active ? (*h->segs_active)[0].nrows : nrows;
    const int64_t m = std::min<int64_t>(srows, 1 << 16);
    fx_sample_kernel<<<(int)std::min<int64_t>((m + 255) / 256, 256), 256, 0, s>>>((const double*)a.cols[0].values + a.cols[0].offset, srows, m, d, d + 1);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(got3, d, 24, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    const unsigned long long got = got3[0];
    const uint32_t xinv = (uint32_t)got, xexp = (uint32_t)(got >> 32);
    const bool zeros = xinv == 0 && xexp == 0;
    if (zeros || xexp < 2047) {
        // (zeros only: as if the sample held ones -- narrow words with nine bits on either side of the quantum)
        const int L = zeros ? 0 : (int)(0xFFFFu - xinv) - 1075, E = zeros ? 0 : (int)xexp - 1022;   // lowest bit 2^L, |v| < 2^E
        // what the first of two levels needs for a window of its own (plan_narrow_first_level)
        h->fx_L = L; h->fx_E = E;
        h->fx_vmin = zeros ? 0.0 : f64_of_ordered(~got3[1]); h->fx_vmax = zeros ? 0.0 : f64_of_ordered(got3[2]);
        // NARROW words (round 6): up to 16 bits of quanta in the sample leave two spare bits inside 18 -- the words of the LAST scatter
        // level then are 32 bits, (m << slot bits) | slot with at most 13 slot bits: 4 bytes per entry into the final pass
        const bool narrow = E - L <= 16 && env_i64("VNM_DENSE_FX_NARROW", 1) != 0;
        const int room = narrow ? 18 : 31;
        const int spare = room - (E - L);
        if (spare >= 0) {
            int qe = L - spare / 2;          // half of the spare bits below the sampled quantum, the rest above the sampled magnitude
            if (qe > 0) qe = 0;              // (fx_encode: 2^-qe >= 1)
            if (qe >= -1000 && E - qe <= room) { h->fx_state = 1; h->fx_qe = qe; h->fx_narrow = narrow; }
        }
    }
    if (getenv("VNM_AGG_TRACE")) fprintf(stderr, "[agg] fixed-point entries: sample says %s (qe %d, values %g .. %g)\n", h->fx_state == 1 ? "yes" : "no", h->fx_qe, h->fx_vmin, h->fx_vmax);
    return 0;
}

// Two levels of fixed-point words whose LAST level is narrow: may the FIRST level write 32-bit words as well?  After a fan-out of 2^p1
// its words keep R1 = bits - p1 remainder bits and V1 = 32 - R1 bits for the value -- an unsigned window [base, base + 2^V1) of quanta that
// must hold the sampled minimum and maximum.  The quantum: the sampler's rule with min(18, V1) bits instead of 18 (never finer than the
// operator's: pass 1 checks every row at that one first, so a row that misfits there costs what it always did).  p1 rises, up to 9 and
// while the second level keeps 32 rings, where that is what makes the span fit (2^27 codes: p1 8 -> 9, V1 13 -> 14).  The window is
// [0, 2^V1) where that holds the sample -- the exponent bound then promises the fit for every |v| < 2^E -- or its mirror image for
// negative data; otherwise the sampled span sits in its middle.  false: the first level keeps 8-byte words.
bool plan_narrow_first_level(const vnm_agg* h, int bits, int pbits, bool p1_given, int* p1, int* qe_out, int* wbits, int* wbase) {
    if (!h->fx_narrow || h->fx_narrow1_off || env_i64("VNM_DENSE_FX_NARROW", 1) == 2) return false;
    for (int pc = *p1; pc <= 9 && (pc == *p1 || (!p1_given && pbits - pc >= 5)); pc++) {
        const int v1 = 32 - (bits - pc);
        if (v1 < 1 || v1 > 24) continue;
        const int room = std::min(18, v1);
        int qe = h->fx_E - h->fx_L <= room ? h->fx_L - (room - (h->fx_E - h->fx_L)) / 2 : h->fx_L;
        qe = std::max(std::min(qe, 0), h->fx_qe);
        // (every sampled value is a multiple of 2^L >= 2^qe below 2^18 quanta of the operator's quantum: exact)
        const int64_t mn = (int64_t)std::ldexp(h->fx_vmin, -qe), mx = (int64_t)std::ldexp(h->fx_vmax, -qe);
        const int64_t w = (int64_t)1 << v1;
        if (mx - mn >= w) continue;
        *p1 = pc; *qe_out = qe; *wbits = v1;
        *wbase = mn >= 0 && mx < w ? 0 : (mx <= 0 && mn > -w ? (int)(1 - w) : (int)(mn - (w - 1 - (mx - mn)) / 2));
        return true;
    }
    return false;
}

// Stage 2b: tables, fan-out, regions and rings of the attempt.  0, or 2 = not applicable.
int plan_dense_geometry(const vnm_agg* h, const AggArgs& a, int64_t nrows, const DGenArgs& g, DensePlan* p) {
    const int cus = device_info().num_cus;
    const DenseMap& mp = h->dmap;
    const bool generic = p->generic, has_val = p->has_val;
    const bool fx_ok = p->fx_base && h->fx_state == 1;
    // slots per final partition: the largest table that still leaves >= 2048 final partitions (8 per CU)
    int tb = (int)env_i64("VNM_DENSE_TBITS", 12);
    tb = std::max(DP_TBITS_MIN, std::min(DP_TBITS_MAX, tb));
    while (tb > DP_TBITS_MIN && mp.bits - tb < 11) tb--;
    while (tb < DP_TBITS_MAX && mp.bits - tb > 18) tb++;
    // ranges of up to 2^22 codes: ONE scatter level (at most 512 partitions) with the largest table that allows it
    // (... 2^21 for entries that carry a value: 512 rings of 10-byte entries do not fit the LDS with two flush blocks each, and the tile-sorting
    // scatter that takes such a level runs at half the ring scatter's speed -- 1e9 rows, G = 2e6: 9.0 ms against 7.2 through two levels)
    const int one_level_bits = DP_TBITS_MAX + (has_val && env_i64("VNM_DENSE_ONE_LEVEL_512", 0) == 0 ? 8 : 9);
    if (mp.bits <= one_level_bits && env_i64("VNM_DENSE_ONE_LEVEL", 1)) tb = std::max(DP_TBITS_MIN, std::min(DP_TBITS_MAX, mp.bits - (int)env_i64("VNM_DENSE_ONE_P", 8)));
    if (mp.bits < 20) tb = (int)env_i64("VNM_DENSE_SMALL_TBITS", 11);   // split final pass: few partitions, long write runs in pass 1 (r03: 2^11-slot tables, G = 2e4 / 5e4 / 1e5 / 3e5: 7.4 / 6.5 / 6.3 / 6.1 -> 5.8 / 5.6 / 5.5 / 5.8 ms with the ring scatter; 2^12 was the r02 optimum)
    // ranges of 2^14 / 2^15 codes (G ~ 1e4 .. 3e4): 32 partitions of 2^9 / 2^10 slots, so that the ring scatter applies (round 4; before:
    // 8 / 16 partitions through the tile-sorting scatter, pass 1 at 5.7 ms -- the G = 1e4 cliff of the sweep, 7.0 ms between 2.9 at
    // G = 1e3 and 5.2 at G = 1e5)
    if (mp.bits - tb < 5 && env_i64("VNM_DENSE_MIN_PARTS32", 1)) tb = std::max(9, mp.bits - 5);
    // fixed-point entry words are 8 bytes: 512 rings of two flush blocks fit the LDS, so ranges of 2^20 .. 2^22 codes take ONE level of 512
    // partitions straight into 2^11 .. 2^13-slot tables, one workgroup per partition (no split final pass, no merge kernel)
    if (fx_ok && mp.bits >= 20 && mp.bits <= 22 && env_i64("VNM_DENSE_FX_ONE_LEVEL", 1)) tb = mp.bits - 9;
    // ... and SMALLER ranges, 2^16 .. 2^19 codes (G ~ 6e4 .. 5e5), the same way: 128 .. 512 partitions of 2^9 / 2^10 slots, one workgroup each -- they took
    // 32 .. 256 partitions of float64 entries and a split final pass: 6.0-6.4 ms per 1e9 rows where G = 1e6 takes 4.3 (round 6, the sweep of tuning log S20)
    // (2^15 .. 2^17 codes: tables of 2^7 / 2^8 slots -- fewer slots than the final workgroup has threads -- keep 256 .. 512 partitions)
    const bool fx_small = fx_ok && mp.bits >= (int)env_i64("VNM_DENSE_FX_SMALL_MIN_BITS", 15) && mp.bits <= 19 && env_i64("VNM_DENSE_FX_SMALL", 1) != 0;
    if (fx_small) tb = std::max(7, mp.bits - 9);
    if (generic) {   // the table must fit 64 KB of LDS (80 KB at most: one workgroup per CU less)
        int tmax = DP_TBITS_MAX;
        while (tmax > 9 && ((size_t)dgen_slot_bytes(g) << tmax) > 64 * 1024) tmax--;   // (the generic kernels take the table size at run time)
        // ... unless that means ONE level of 512 partitions: the ring scatter cannot hold two blocks of (value, code) entries for 512 rings
        // in LDS, the tile-sorting scatter that takes over runs at half its speed (min + max, 1e9 rows, G = 5e5: pass 1 7.9 ms against
        // 4.3), and a table of twice the slots -- 256 partitions, one workgroup per CU in the final pass -- costs less (round 5)
        if (mp.bits - tmax == 9 && tmax < DP_TBITS_MAX && ((size_t)dgen_slot_bytes(g) << (tmax + 1)) <= (size_t)env_i64("VNM_DGEN_BIG_LDS_KB", 128) * 1024) tmax++;
        if (((size_t)dgen_slot_bytes(g) << tmax) > 128 * 1024) return 2;
        if (tb > tmax) tb = tmax;
        if (mp.bits - tb > 18) return 2;
    }
    // COUNT(*) alone over many groups (round 5): ONE scatter level of at most 512 partitions, then one-byte counters over sub-ranges of
    // 2^17 codes (dcount8_final_kernel).  A handful of rows per group is what it is for: no heavy keys in the estimator's sample, at most
    // 64 rows per estimated group; a byte that overflows after all sends the batch through the two levels and switches this off.
    // counter width: a byte for up to 64 rows per estimated group (or no estimate: the dense path went by the sample's lower bound), two
    // bytes up to 16384
    p->c8_cb = h->count_cb ? h->count_cb : ((h->hint == 0 || nrows <= 64 * h->hint) ? 8 : (nrows <= 16384 * h->hint ? 16 : 0));
    const int c8_tmax = p->c8_cb == 8 ? DC8_BITS : DC8_BITS - 1;
    p->count8 = generic && !has_val && g.n_lds == 0 && !p->vn && !h->count8_off && h->heavy_share == 0.0 && p->c8_cb != 0 && mp.bits >= DP_TBITS_MAX + 10 &&
                mp.bits <= c8_tmax + 9 + 1 && env_i64("VNM_DENSE_COUNT8", 1);
    p->c8_sub = p->count8 ? std::max(0, mp.bits - c8_tmax - 9) : 0;       // a partition of twice the table's codes is read once per half
    if (p->count8) tb = mp.bits - 9 - p->c8_sub;                            // 2^14 .. 2^17 counters per table
    p->tb = tb;
    p->pbits = p->count8 ? 9 : mp.bits - tb;
    p->levels = p->pbits > 9 ? 2 : 1;
    const int pbits = p->pbits, levels = p->levels;
    p->nfinal = (int64_t)1 << pbits;
    // pass 1 moves 12-byte entries out of 16-byte rows, pass 2 moves 10-byte entries out of 12: the SMALLER fan-out goes
    // to pass 1, whose write runs are the shorter ones (measured at b = 27: p1 = 7 / 8 -> 4.9 / 5.6 ms for pass 1)
    // (fixed-point words: 8 bytes in BOTH passes -- the larger fan-out goes first: G = 1e8, p1 = 7 / 8: 7.53 / 7.37 ms)
    int p1 = levels == 2 ? (int)env_i64("VNM_DENSE_P1", fx_ok ? (pbits + 1) / 2 : pbits / 2) : pbits;
    if (levels == 2) { if (p1 > 9) p1 = 9; if (pbits - p1 > 9) p1 = pbits - 9; }
    // (two levels never share a final partition and never count bytes: this is what p->fx comes to below)
    p->fx_qe = h->fx_qe; p->fx_wbits = 0; p->fx_wbase = 0;
    p->narrow1 = fx_ok && levels == 2 && tb >= 11 && tb <= 13 && plan_narrow_first_level(h, mp.bits, pbits, getenv("VNM_DENSE_P1") != nullptr, &p1, &p->fx_qe, &p->fx_wbits, &p->fx_wbase);
    p->p1 = p1; p->p2 = pbits - p1;
    p->np1 = 1 << p1; p->np2 = levels == 2 ? 1 << p->p2 : 0;
    const int np1 = p->np1, np2 = p->np2;
    const int64_t tile1 = PT_TILE;
    const int grid1 = (int)std::min<int64_t>((int64_t)cus * env_i64("VNM_DENSE_GRID1_PER_CU", 2), (nrows + tile1 - 1) / tile1);
    int split2 = std::max(2, (grid1 + PT_MAX_REGIONS - 1) / PT_MAX_REGIONS);
    split2 = std::max(split2, std::min(grid1, (cus * 2 + np1 - 1) / np1));
    // skewed keys (the estimator's sample saw heavy keys): more, smaller work items for pass 2 -- the partition that holds a heavy key
    // has a multiple of the others' entries, and with cus * 2 work items for cus * 2 resident workgroups the heaviest sets the time
    if (h->heavy_share > 0.0) split2 = std::min(grid1, split2 * (int)env_i64("VNM_DENSE_SKEW_SPLIT", 8));
    p->grid1 = grid1; p->split2 = split2;
    const int64_t tiles_per_wg = ((nrows + tile1 - 1) / tile1 + grid1 - 1) / grid1;
    const int64_t rows_per_wg = tiles_per_wg * tile1;
    int64_t cap1 = ((rows_per_wg / np1 + rows_per_wg / np1 / 5 + 512) + 15) & ~15LL;
    // region stride = an ODD number of 128-byte lines: the lines the resident workgroups keep open in one partition then spread
    // over the L2 sets instead of sharing their low index bits (two sessions of 5-6 process pairs: 11.73 -> 11.25 and 11.27 -> 11.17 ms)
    const bool odd_cap = env_i64("VNM_DENSE_ODD_CAP", 1) != 0;
    if (odd_cap && ((cap1 / 16) & 1) == 0) cap1 += 16;
    if (fx_ok && h->fx_narrow && (levels == 1 || p->narrow1)) { cap1 = (cap1 + 31) & ~31LL; if (((cap1 / 32) & 1) == 0) cap1 += 32; }   // (32-bit words: blocks of 32)
    p->cap1 = cap1;
    p->c16_1 = levels == 1 && !p->count8;
    // final partitions x splits >= ~4 workgroups per CU
    int fsplits = 1;
    if (levels == 1 && !p->count8 && ((int64_t)1 << pbits) < (int64_t)cus * 2) {
        fsplits = (int)std::min<int64_t>(grid1, ((int64_t)cus * env_i64("VNM_DENSE_SPLIT_WGS", 4) + ((int64_t)1 << pbits) - 1) >> pbits);
        if (fsplits < 2) fsplits = 1;
    }
    if (fx_small && levels == 1) fsplits = 1;   // (128 .. 512 lean final workgroups: a short pass either way)
    p->fsplits = fsplits;
    p->fx = fx_ok && fsplits == 1 && !p->count8 && tb >= (fx_small ? 7 : 11) && tb <= 13;
    if (!p->fx) p->narrow1 = false;
    p->fx_q = p->fx ? std::ldexp(1.0, p->fx_qe) : 0.0;
    p->w32 = p->fx && h->fx_narrow;
    p->w32_1 = p->w32 && (levels == 1 || p->narrow1);
    if (levels == 2) {
        const int64_t per_pg = (int64_t)grid1 * rows_per_wg / np1 / split2;
        int64_t cap2 = ((per_pg / np2 + per_pg / np2 / 4 + 256) + 15) & ~15LL;
        if (odd_cap && ((cap2 / 16) & 1) == 0) cap2 += 16;
        if (p->w32) { cap2 = (cap2 + 31) & ~31LL; if (((cap2 / 32) & 1) == 0) cap2 += 32; }   // (32-bit words: blocks of 32)
        p->cap2 = cap2;
    }
    p->spill_cap = nrows / 2 + (1 << 20);
    p->nspill_cap = p->vn_lists ? nrows / 4 + (1 << 20) : 0;
    p->dstride = std::min<int64_t>(h->dense_span, nrows) + 2;
    // producer-major regions (a workgroup's 128 output regions adjacent) were tried against TLB pressure: pass 1 unchanged,
    // pass 2 and the final pass 15-20 % slower (their reads become 150 KB chunks 75 MB apart) -> partition-major stays
    p->pmajor = (int)env_i64("VNM_DENSE_PRODUCER_MAJOR", 0);
    // ring-buffer scatter (dring_scatter_kernel): VNM_DENSE_RING bit 0: pass 1, bit 1: pass 2
    const int use_ring = (int)env_i64("VNM_DENSE_RING", 3);
    p->ring_limit = env_i64("VNM_DENSE_RING_LIMIT", 1) != 0;
    p->rcap1 = p->w32_1 ? ring_cap_w32(np1) : ((use_ring & 1) && !a.has_expr ? ring_cap_for(np1, p->fx ? 8 : (has_val ? 8 : 0) + (p->c16_1 ? 2 : 4)) : 0);
    if (levels == 2) p->rcap2 = p->fx ? (p->w32 ? ring_cap_w32(np2) : ring_cap_for(np2, 8)) : ((use_ring & 2) ? ring_cap_for(np2, (has_val ? 8 : 0) + 2) : 0);
    // (pass 1 of TWO levels of fixed-point words: sub-tiles of two pairs -- 4.07-4.19 -> 3.85-3.90 ms at G = 1e8, A/B x 3; one level
    // of 512 rings: four pairs as before)
    p->ring_pairs1 = (int)env_i64("VNM_DENSE_RING_PAIRS", 4);
    // (32-bit window words out of the first of two levels: two pairs as well -- 6.22-6.23 ms against 6.21-6.23 with four at G = 1e8, and every
    // two-pair kernel of the family, nullable key included, stays clear of scratch: the four-pair nullable-key kernel spills 12 VGPRs)
    if (p->fx && levels == 2 && getenv("VNM_DENSE_RING_PAIRS") == nullptr) p->ring_pairs1 = 2;
    // (32-bit words out of pass 2: 128 rings of up to 256 words take four pairs per lane in one round -- half the barriers: 1.74-1.76 -> 1.56 ms)
    p->ring_pairs2 = levels == 2 ? (int)env_i64("VNM_DENSE_RING_PAIRS2", p->fx && p->w32 ? 4 : 2) : 0;
    return 0;
}

// Stage 3 owns every pool block of the attempt (AttemptBlocks), these by name:
struct DenseBuffers : AttemptBlocks {
    unsigned long long* flags = nullptr;   // [0..3] status words, [6] exact-add statistics, [7] fixed-point misfit, [8..12] the NULL-key rows of this attempt (nullable key)
    double* v1 = nullptr; void* c1 = nullptr; uint32_t* n1 = nullptr;    // regions of level 1: values / words, code remainders, counts
    double* v2 = nullptr; void* c2 = nullptr; uint32_t* n2 = nullptr;    // ... of level 2
    double* w1 = nullptr; double* w2 = nullptr;                          // the second value of two-value entries (dense_two_aggregate)
    ulonglong2* spill = nullptr;           // entries without a place: the caller's on success
    uint64_t* nspill = nullptr;            // keys of NULL-value rows without a place: the caller's on success
    uint64_t* rk = nullptr; uint64_t* ra = nullptr;                      // the run a final pass of this call writes
};

int dense_allocate(const DensePlan& p, DenseBuffers& b, hipStream_t s) {
    b.take(b.flags, 128);
    b.take(b.v1, p.has_val ? (size_t)p.np1 * p.grid1 * p.cap1 * (p.w32_1 ? 4 : 8) : 8);
    b.take(b.c1, p.fx ? 16 : (size_t)p.np1 * p.grid1 * p.cap1 * (p.c16_1 ? 2 : 4));
    b.take(b.n1, (size_t)p.np1 * p.grid1 * 4);
    b.take(b.spill, (size_t)p.spill_cap * 16);
    if (p.vn_lists) b.take(b.nspill, (size_t)p.nspill_cap * 8);
    if (!b.flags || !b.v1 || !b.c1 || !b.n1 || !b.spill || (p.vn_lists && !b.nspill)) return 1;
    VNM_HIP(hipMemsetAsync(b.flags, 0, 128, s));
    fill_u64_kernel<<<1, 1, 0, s>>>((uint64_t*)b.flags + 11, F64_NEG_ZERO, 1);   // (the NULL-key rows' sum starts at -0.0: merge_init)
    VNM_HIP(hipGetLastError());
    return 0;
}

// A nullable key: pass 1 sums the NULL-key rows of this ATTEMPT into scratch words; only an attempt that is known good adds them to
// the NULL slot of the operator's HBM table (here).  A failed attempt -- full spill buffer, output too small, a compensation term
// out of range: all known only after pass 1 -- leaves the table untouched, and the route that takes the batch instead counts those
// rows itself (they used to be counted twice: ADVICE r04).
int fold_null_rows(const vnm_agg* h, const AggArgs& a, const unsigned long long* flags, hipStream_t s) {
    if (!h->kn_valid) return 0;
    const GTable& gt = h->g;
    const uint64_t slot = gt.cap + 1;
    dnull_fold_kernel<<<1, 64, 0, s>>>(flags + 8, gt.tag + slot,
                                       a.hot_w_rows >= 0 ? gt.acc + (uint64_t)a.hot_w_rows * gt.stride + slot : nullptr,
                                       a.hot_w_valid >= 0 ? gt.acc + (uint64_t)a.hot_w_valid * gt.stride + slot : nullptr,
                                       a.hot_w_sum >= 0 ? gt.acc + (uint64_t)a.hot_w_sum * gt.stride + slot : nullptr,
                                       a.hot_comp && a.hot_w_sum >= 0 ? (int64_t)gt.stride : 0);
    VNM_HIP(hipGetLastError());
    return 0;
}

// The kernel of level 1: the ring scatter where the rings take the fan-out (p.rcap1), the tile-sorting scatter otherwise.
int dense_scatter1_launch(vnm_agg* h, const DensePlan& p, DenseBuffers& b, DPartArgs& d1, hipStream_t s) {
    const bool pv = d1.has_pred && !d1.pred_is_v;   // a predicate column of its own
    if (!p.rcap1)
        return pick_bool(p.c16_1, [&](auto c16) {
            using CT = std::conditional_t<decltype(c16)::value, uint16_t, uint32_t>;
            if (p.vn) { dpart_scatter_kernel<true, CT, true, true><<<p.grid1, PT_BLOCK, 0, s>>>(d1); return 0; }
            return pick_bool(p.has_val, [&](auto hv) { dpart_scatter_kernel<true, CT, decltype(hv)::value><<<p.grid1, PT_BLOCK, 0, s>>>(d1); return 0; });
        });
    const bool plain_val = p.has_val && !p.vn;   // what the kernels for stream segments and nullable keys read
    const RingLaunch r{p.grid1, p.rcap1, ring_sub_tile_pairs(p.ring_pairs1, pv, p.ring_limit, p.np1, p.rcap1, p.w32_1), p.ring_limit,
                       plain_val && h->segs_active != nullptr, plain_val && h->kn_valid != nullptr, s};
    // the waiting batches of a stream: one segment each, sub-tiles of 2 * pairs * 1024 rows
    if (r.seg && !r.kn && upload_segs(h, (int64_t)2 * r.pairs * 1024, &d1.segs, &d1.nseg, &d1.nsub, b.pool, s)) return 1;
    if (p.fx && p.narrow1) {   // window words out of the first of two levels
        if (p.vn) return ring_scatter<true, uint32_t, true, false, true, true, true, false, true>(r, d1);
        return pick_bool(pv, [&](auto pvc) { return ring_scatter<true, uint32_t, true, decltype(pvc)::value, false, true, true, false, true>(r, d1); });
    }
    if (p.fx && p.vn)   // (vn_fold: the predicate column is the value column)
        return pick_bool(p.w32_1, [&](auto w32) { return ring_scatter<true, uint32_t, true, false, true, true, decltype(w32)::value>(r, d1); });
    if (p.fx)
        return pick_bool(p.w32_1, [&](auto w32) {
            return pick_bool(pv, [&](auto pvc) { return ring_scatter<true, uint32_t, true, decltype(pvc)::value, false, true, decltype(w32)::value>(r, d1); });
        });
    return pick_bool(p.c16_1, [&](auto c16) {
        using CT = std::conditional_t<decltype(c16)::value, uint16_t, uint32_t>;
        return pick_bool(pv, [&](auto pvc) {
            if (p.vn) return ring_scatter<true, CT, true, decltype(pvc)::value, true>(r, d1);
            return pick_bool(p.has_val, [&](auto hv) { return ring_scatter<true, CT, decltype(hv)::value, decltype(pvc)::value, false>(r, d1); });
        });
    });
}

// Stage 4: scatter level 1, rows -> np1 partitions (d1 stays: level 2 takes its fixed-point parameters from it).
int dense_scatter1(vnm_agg* h, const AggArgs& a, int64_t nrows, const DensePlan& p, DenseBuffers& b, DPartArgs& d1, hipStream_t s) {
    d1.map = h->dmap;
    d1.kp = (const uint64_t*)a.keys[0].values + a.keys[0].offset;
    d1.vp = p.has_val ? (const double*)a.cols[0].values + a.cols[0].offset : nullptr;
    d1.has_expr = a.has_expr; d1.expr = a.expr;
    fill_pred(d1, h, a);
    d1.nrows = nrows;
    d1.out_vals = b.v1; d1.out_codes = b.c1; d1.out_counts = b.n1; d1.out_cap = p.cap1;
    d1.nparts = p.np1; d1.out_bits = h->dmap.bits - p.p1;
    d1.producer_major = p.pmajor;
    // Non-temporal stores for pass 1's runs when a wide second level follows: pass 2 then reads them 15-20 % faster and the query
    // gains 0.4 ms (1.1 ms in sustained runs) at G = 1e8 (p2 = 8); with p2 = 6 (G = 1e7) or a single level it is neutral to
    // slightly worse, so it stays off there.  In pass 2 itself such stores cost 0.3 ms.  (VNM_DENSE_NT: bit 0 pass 1, bit 1 pass 2)
    d1.nt_store = (int)env_i64("VNM_DENSE_NT", p.levels == 2 && p.np2 >= 256 ? 1 : 0) & 1;
    d1.ready_list = (int)env_i64("VNM_DENSE_READY_LIST", 1) & 1;
    d1.flags = b.flags; d1.spill = b.spill; d1.spill_cap = p.spill_cap;
    d1.fx_q = p.fx_q; d1.fx_inv_q = p.fx ? std::ldexp(1.0, -h->fx_qe) : 0.0;   // (the per-row check is at the operator's quantum)
    d1.fx_lim = p.w32 ? (1LL << 18) - 1 : 2147483647LL;
    if (p.narrow1) { d1.fx_wbits = p.fx_wbits; d1.fx_wbase = p.fx_wbase; d1.fx_wuns = 1; d1.fx_sh = p.fx_qe - h->fx_qe; }
    if (p.vn) { d1.vvalid = a.cols[0].validity; d1.voff = a.cols[0].offset; d1.nspill = b.nspill; d1.nspill_cap = p.nspill_cap; }
    if (h->kn_valid) {   // the NULL-key rows go to scratch words of the flags block (fold_null_rows)
        if (ensure_table(h, 1024, s, true)) return 1;
        uint64_t* scr = (uint64_t*)(b.flags + 8);
        d1.kvalid = h->kn_valid; d1.koff = h->kn_off;
        d1.nk_tag = scr;
        d1.nk_rows = a.hot_w_rows >= 0 ? scr + 1 : nullptr;
        d1.nk_valid = a.hot_w_valid >= 0 ? scr + 2 : nullptr;
        d1.nk_sum = a.hot_w_sum >= 0 ? scr + 3 : nullptr;
        d1.nk_lo_stride = a.hot_comp && a.hot_w_sum >= 0 ? 1 : 0;
    }
    {
        KernelTimer timer("agg_part_scatter1", s);
        VNM_TRY(dense_scatter1_launch(h, p, b, d1, s));
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

// Stage 5: scatter level 2, every first-level partition -> np2 partitions.
int dense_scatter2(const vnm_agg* h, const DensePlan& p, DenseBuffers& b, const DPartArgs& d1, hipStream_t s) {
    b.take(b.v2, p.has_val ? (size_t)p.np1 * p.np2 * p.split2 * p.cap2 * (p.w32 ? 4 : 8) : 8);
    b.take(b.c2, p.fx ? 16 : (size_t)p.np1 * p.np2 * p.split2 * p.cap2 * 2);
    b.take(b.n2, (size_t)p.np1 * p.np2 * p.split2 * 4);
    if (!b.v2 || !b.c2 || !b.n2) return 1;
    DPartArgs d2{};
    d2.map = h->dmap;
    d2.in_vals = b.v1; d2.in_codes = (const uint32_t*)b.c1; d2.in_counts = b.n1; d2.in_cap = p.cap1;
    d2.in_regions = p.grid1; d2.in_split = p.split2; d2.in_bits = h->dmap.bits - p.p1;
    d2.in_pstride = p.pmajor ? 1 : p.grid1; d2.in_rstride = p.pmajor ? p.np1 : 1;
    d2.out_vals = b.v2; d2.out_codes = b.c2; d2.out_counts = b.n2; d2.out_cap = p.cap2;
    d2.nparts = p.np2; d2.out_bits = p.tb;
    d2.flags = b.flags; d2.spill = b.spill; d2.spill_cap = p.spill_cap;
    d2.nspill = b.nspill; d2.nspill_cap = p.nspill_cap;
    d2.nt_store = ((int)env_i64("VNM_DENSE_NT", 0) >> 1) & 1;
    d2.ready_list = ((int)env_i64("VNM_DENSE_READY_LIST", 1) >> 1) & 1;   // (pass 2: every ring completes a block in every round -- the list only costs its atomics: 1.71 -> 1.78 ms)
    d2.fx_q = d1.fx_q; d2.fx_inv_q = d1.fx_inv_q; d2.fx_lim = d1.fx_lim;
    d2.fx_in_base = d1.fx_wbase;
    const int grid2 = p.np1 * p.split2;
    const RingLaunch r{grid2, p.rcap2, ring_sub_tile_pairs(p.ring_pairs2, false, p.ring_limit, p.np2, p.rcap2, p.w32), p.ring_limit, false, false, s};
    {
        KernelTimer timer("agg_part_scatter2", s);
        if (p.fx && p.narrow1) VNM_TRY((ring_scatter<false, uint32_t, true, false, false, true, true, true>(r, d2)));
        else if (p.fx) VNM_TRY(pick_bool(p.w32, [&](auto w32) { return ring_scatter<false, uint32_t, true, false, false, true, decltype(w32)::value>(r, d2); }));
        else if (p.rcap2) VNM_TRY(pick_bool(p.has_val, [&](auto hv) { return ring_scatter<false, uint16_t, decltype(hv)::value, false, false>(r, d2); }));
        else VNM_TRY(pick_bool(p.has_val, [&](auto hv) { dpart_scatter_kernel<false, uint16_t, decltype(hv)::value><<<grid2, PT_BLOCK, 0, s>>>(d2); return 0; }));
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

// Stage 6, COUNT(*) alone: byte counters over the level's partitions.
int dense_final_count8(vnm_agg* h, const DensePlan& p, const DenseBuffers& b, DGenArgs& g, hipStream_t s) {
    // one-byte counters that overflow (a group of 256 rows or more: flags[5]) hand the SAME entries to two-byte counters -- tables of at
    // most 2^16 codes, so a partition may be read once more often -- before the batch would go back through two scatter levels
    for (int cb = p.c8_cb;;) {
        const int tbc = std::min(p.tb, cb == 8 ? DC8_BITS : DC8_BITS - 1), subc = p.c8_sub + (p.tb - tbc);
        g.tbits = tbc;
        const size_t lds = ((size_t)1 << tbc) * (size_t)(cb / 8);
        {
            KernelTimer timer("agg_part_final", s);
            VNM_TRY(launch_resident(cb == 8 ? dcount8_final_kernel<8> : dcount8_final_kernel<16>, p.nfinal << subc, 1024, lds, 2, s, g, subc));
        }
        VNM_HIP(hipGetLastError());
        if (cb == 16) break;
        unsigned long long f6[6]; VNM_TRY(read_flags(f6, b.flags, s));
        if (!(f6[0] && f6[5])) break;
        cb = 16;
        h->count_cb = 16;
        VNM_HIP(hipMemsetAsync(b.flags, 0, 16, s));          // [0] failure, [1] rows claimed ([2], the scatter's spill count, stays)
        VNM_HIP(hipMemsetAsync(b.flags + 5, 0, 8, s));
    }
    return 0;
}

// Stage 6, generic programs: tables of 2^tb slots in dynamic LDS; few final partitions are shared by `fsplits` workgroups each
// (partial tables + dgen_merge_kernel).
int dense_final_generic(const DensePlan& p, DenseBuffers& b, DGenArgs& g, hipStream_t s) {
    const size_t slots = (size_t)1 << p.tb;
    const size_t lds = slots * dgen_slot_bytes(g);
    if (p.fsplits > 1) {
        const size_t work = (size_t)p.nfinal * p.fsplits;
        g.part_w = (uint64_t*)b.pool.take(std::max<size_t>(8, work * g.n_lds * slots * 8));
        g.part_cnt = (uint32_t*)b.pool.take(work * slots * 4);
        if (!g.part_w || !g.part_cnt) return 1;
        g.splits = p.fsplits;
    }
    KernelTimer timer("agg_part_final", s);
    VNM_TRY(pick_bool(p.has_val, [&](auto hv) {
        return pick_bool(p.fsplits > 1, [&](auto sp) {
            return launch_resident(dgen_final_kernel<decltype(hv)::value, decltype(sp)::value>, p.nfinal * (decltype(sp)::value ? p.fsplits : 1), 512, lds, 8, s, g);
        });
    }));
    if (p.fsplits > 1) dgen_merge_kernel<<<(int)(p.nfinal << (p.tb - 9)), 512, 0, s>>>(g);
    return 0;
}

// Stage 6, few final partitions and a run of this call's own: `fsplits` workgroups per partition (partial tables + dpart_merge_kernel).
int dense_final_split(const DensePlan& p, DenseBuffers& b, DFinalArgs& df, hipStream_t s) {
    const size_t cells = (size_t)p.nfinal * p.fsplits << p.tb;
    df.part_sum = (uint64_t*)b.pool.take(cells * 8); df.part_lo = (float*)b.pool.take(cells * 4); df.part_cnt = (uint32_t*)b.pool.take(cells * 4);
    if (!df.part_sum || !df.part_lo || !df.part_cnt) return 1;
    df.splits = p.fsplits;
    KernelTimer timer("agg_part_final", s);
    VNM_TRY((pick_int<9, 13>(p.tb >= 9 && p.tb <= 12 ? p.tb : 13, [&](auto tbc) {
        constexpr int TB = decltype(tbc)::value;
        return launch_resident(dpart_final_kernel<uint16_t, TB, true>, p.nfinal * p.fsplits, TB >= 13 ? 1024 : (TB == 12 ? VNM_DF12_BLOCK : 512), 0, 8, s, df);
    })));
    dpart_merge_kernel<<<(int)(p.nfinal << (p.tb - 9)), 512, 0, s>>>(df, p.tb);
    return 0;
}

// Stage 6, the usual one: the final pass is DEFERRED -- what it should write depends on what comes next (complete_pending), and the
// batches of a stream share ONE final pass.  The scatter passes have to be known good first; then the entries join the pending pass
// of the handle.  0 = done, 2 = the scatter failed, ATTEMPT_REDO = a fixed-point misfit (32-bit words out of both levels -> out of the last only -> 8-byte words -> float64 entries).
int dense_defer_final(vnm_agg* h, const AggArgs& a, int64_t nrows, const DensePlan& p, DenseBuffers& b, const DSet& fin, DFinalArgs& df, hipStream_t s,
                      ulonglong2** spill_out, int64_t* n_spill_out) {
    const DenseMap& mp = h->dmap;
    unsigned long long fl0[8]; VNM_TRY(read_flags(fl0, b.flags, s));
    route_note(h->kn_valid ? "dense:nullable_key" : (h->segs_active ? "dense:stream_segments" : (p.vn ? "dense:nullable_value" : (p.levels == 1 && p.p1 == 5 && p.tb <= 10 ? "dense:32_partitions" :
               (p.fsplits > 1 ? "dense:split_final" : (p.levels == 2 ? "dense:two_levels" : "dense:one_level"))))),
               "2^%d codes, 2^%d-slot final tables, p1 %d p2 %d, final pass deferred%s: %s", mp.bits, p.tb, p.p1, p.p2, p.vn ? ", nullable value" : "", fl0[0] || (p.fx && fl0[7]) ? "scatter FAILED (the batch goes another way)" : "ok");
    if (getenv("VNM_AGG_TRACE"))
        fprintf(stderr, "[agg] dense: bits %d tb %d levels %d p1 %d p2 %d -> scatter fail %llu spilled %llu, final pass deferred (bound %lld)\n",
                mp.bits, p.tb, p.levels, p.p1, p.p2, fl0[0], fl0[2], (long long)p.dstride);
    if (p.fx && fl0[7] == 2) {   // every value fits the words of the last level, one is outside the first level's window: that level alone goes back to 8-byte words, for this batch and every later one
        h->fx_narrow1_off = true;
        route_note("dense:fixed_point_misfit", "a value outside the first level's window, 2^%d * [%d, %d + 2^%d): the batch is redone with 8-byte words out of that level", p.fx_qe, p.fx_wbase, p.fx_wbase, p.fx_wbits);
        return ATTEMPT_REDO;
    }
    if (p.fx && fl0[7]) {   // a value that is not m * 2^qe with |m| < 2^31: float64 entries for this batch and every later one
        if (h->fx_narrow) {   // (outside the 18 bits of the narrow words: 64-bit words with six more bits below the quantum and 13 more above)
            h->fx_narrow = false;
            h->fx_qe = std::max(h->fx_qe - 6, -1000);
            route_note("dense:fixed_point_misfit", "a value outside 2^%d * [-2^18, 2^18): the batch is redone with 64-bit entry words", h->fx_qe + 6);
            return ATTEMPT_REDO;
        }
        h->fx_state = -1;
        route_note("dense:fixed_point_misfit", "a value outside 2^%d * [-2^31, 2^31): the batch is redone with float64 entries", h->fx_qe);
        return ATTEMPT_REDO;
    }
    if (fl0[0]) return 2;
    if (p.fx) route_note("dense:fixed_point", "%s entry words, quantum 2^%d", p.w32 ? (p.levels == 1 ? "4-byte" : (p.narrow1 ? "4-byte, then 4-byte" : "8-byte, then 4-byte")) : "8-byte", p.fx_qe);
    if (p.w32 && !p.narrow1) route_note("dense:fixed_point_narrow_last_level", "32-bit words out of the last of %d level(s) only", p.levels);
    if (p.narrow1) route_note("dense:fixed_point_narrow_levels", "32-bit words out of both levels: p1 %d, a window of %d bits from %d quanta of 2^%d", p.p1, p.fx_wbits, p.fx_wbase, p.fx_qe);
    if (fold_null_rows(h, a, b.flags, s)) return 1;
    b.pool.done(b.rk); b.pool.done(b.ra);   // (the run is allocated when the pass runs)
    if (fl0[2]) { b.pool.keep(b.spill); *spill_out = b.spill; *n_spill_out = (int64_t)fl0[2]; }   // the caller owns it now
    else { *spill_out = nullptr; *n_spill_out = 0; }
    if ((int64_t)fl0[2] > nrows / 16) h->dense_state = -1;
    DensePending* pd = h->pending;
    // batches join a pending pass of the same geometry; anything else (or a very long stream) runs it first.  A pass holds the
    // entries of its batches (10-12 bytes per row) until it runs: at most 1.5 * 2^30 rows of them, so that a stream of any length
    // keeps a bounded amount of HBM (and far below the 2^32 rows the 32-bit row counts of the final pass's slots could take)
    const int64_t pending_max_rows = std::min<int64_t>(env_i64("VNM_DENSE_PENDING_MAX_ROWS", 3LL << 29), (1LL << 32) - 1);
    if (pd && (pd->tb != p.tb || pd->levels != p.levels || pd->p1 != p.p1 || pd->fsplits != p.fsplits || pd->sets.size() >= DP_MAX_SETS ||
               pd->rows + nrows > pending_max_rows || pd->df.fx_q != p.fx_q || pd->df.fx_w32 != (p.w32 ? 1 : 0) || memcmp(&pd->df.map, &mp, sizeof(DenseMap)) != 0)) {
        VNM_TRY(complete_pending(h, s));
        pd = nullptr;
    }
    if (!pd) {
        pd = new DensePending();
        df.dkey = nullptr; df.dacc = nullptr;
        pd->df = df; pd->tb = p.tb; pd->levels = p.levels; pd->p1 = p.p1; pd->fsplits = p.fsplits; pd->nfinal = p.nfinal; pd->dstride = 0;
        b.pool.keep(b.flags); pd->blocks.push_back(b.flags);   // the pass's flags block from here on
        h->pending = pd;
    }
    pd->dstride = std::min<int64_t>(h->dense_span, pd->dstride + nrows) + 2;
    pd->rows += nrows;
    // exact-add statistics of this batch's entries (kept by the ring scatter over plain value columns only)
    if (p.rcap1 && p.has_val && !a.has_expr && !p.fx) { pd->x_inv = std::max(pd->x_inv, (uint32_t)fl0[6]); pd->x_exp = std::max(pd->x_exp, (uint32_t)(fl0[6] >> 32)); }
    else pd->x_known = false;
    pd->sets.push_back(fin);
    // the entries belong to the pass (two levels: the first level's regions have been consumed by the second scatter pass)
    void* const held[3] = {p.levels == 2 ? (void*)b.v2 : (void*)b.v1, p.levels == 2 ? b.c2 : b.c1, p.levels == 2 ? (void*)b.n2 : (void*)b.n1};
    for (void* blk : held) { b.pool.keep(blk); pd->blocks.push_back(blk); }
    return 0;
}

// Stage 7 (the passes that wrote a run of their own): read the flags, hand the run to the handle and the lists to the caller.
// 0 = done, 2 = failed (the batch goes another way), ATTEMPT_REDO = byte counters overflowed (two scatter levels take the batch).
int dense_hand_over(vnm_agg* h, const AggArgs& a, int64_t nrows, const DensePlan& p, DenseBuffers& b, hipStream_t s, ulonglong2** spill_out, int64_t* n_spill_out,
                    uint64_t** nspill_out, int64_t* n_nspill_out) {
    VNM_HIP(hipGetLastError());
    unsigned long long fl[4]; VNM_TRY(read_flags(fl, b.flags, s));
    if (!fl[0]) {
        if (fold_null_rows(h, a, b.flags, s)) return 1;
        VNM_HIP(hipStreamSynchronize(s));   // (the fold reads the flags block, which goes back when this attempt's owner does)
    }
    route_note(p.count8 ? "dense:count_bytes" : p.generic ? (p.fsplits > 1 ? "dense:generic_split_final" : "dense:generic") : (p.vn ? "dense:nullable_value" : (p.fsplits > 1 ? "dense:split_final" : "dense:run")),
               "2^%d codes, 2^%d-slot final tables, levels %d, p1 %d p2 %d, %d final splits: %s", h->dmap.bits, p.tb, p.levels, p.p1, p.p2, p.fsplits, fl[0] ? "FAILED (the batch goes another way)" : "ok");
    if (getenv("VNM_AGG_TRACE"))
        fprintf(stderr, "[agg] dense%s%s: bits %d tb %d levels %d p1 %d p2 %d splits %d -> fail %llu groups %llu spilled %llu + %llu NULL-value rows (dstride %lld)\n",
                p.generic ? " generic" : "", p.vn ? " nullable" : "", h->dmap.bits, p.tb, p.levels, p.p1, p.p2, p.fsplits, fl[0], fl[1], fl[2], fl[3], (long long)p.dstride);
    if (fl[0]) {  // spill buffer full, dense output too small, or a compensation term beyond float range
        if (!p.count8) return 2;
        h->count8_off = true;   // (a group of 256 rows or more, most likely: flags[5]) the two scatter levels take the batch, and every later one
        return ATTEMPT_REDO;
    }
    if (fl[2]) { b.pool.keep(b.spill); *spill_out = b.spill; *n_spill_out = (int64_t)fl[2]; }   // the caller owns the lists now
    else { *spill_out = nullptr; *n_spill_out = 0; }
    if (p.vn && fl[3]) { b.pool.keep(b.nspill); *nspill_out = b.nspill; *n_nspill_out = (int64_t)fl[3]; }
    if ((int64_t)(fl[2] + fl[3]) > nrows / 16) h->dense_state = -1;  // the sampled range does not describe the data: stop trying
    b.pool.keep(b.rk); b.pool.keep(b.ra);   // the run belongs to the handle
    adopt_run(h, b.rk, b.ra, p.dstride, (int64_t)fl[1]);
    return 0;
}

// The driver.  returns 0 = done (run stored), 2 = not applicable / failed (caller continues with the hash-partitioned path), 1 = error
// (nspill_out / n_nspill_out: keys of NULL-value rows that found no place -- nullable value column, generic programs only)
int dense_partitioned_aggregate(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s, ulonglong2** spill_out, int64_t* n_spill_out,
                                bool generic = false, uint64_t** nspill_out = nullptr, int64_t* n_nspill_out = nullptr, bool vn_fold = false) {
    DGenArgs g{};
    if (generic && !dgen_program(h, a, &g)) return 2;
    DensePlan p{};
    VNM_TRY(plan_dense_entries(h, a, generic, g, vn_fold, nspill_out != nullptr, &p));
    if (nspill_out) { *nspill_out = nullptr; *n_nspill_out = 0; }
    if (p.fx_base && h->fx_state == 0) VNM_TRY(sample_fixed_point(h, a, nrows, s));
    VNM_TRY(plan_dense_geometry(h, a, nrows, g, &p));
    DenseBuffers b;
    // the same batch once more, by what the handle says now: the blocks go back first, so that the retry finds them
    auto redo = [&]() { b.free_all(); return dense_partitioned_aggregate(h, a, nrows, s, spill_out, n_spill_out, generic, nspill_out, n_nspill_out, vn_fold); };
    VNM_TRY(dense_allocate(p, b, s));
    if (p.fx && (!p.rcap1 || (p.levels == 2 && !p.rcap2))) { h->fx_state = -1; return redo(); }   // (a fan-out the rings cannot take: float64 entries through the other scatter)
    if ((h->segs_active || h->kn_valid) && (!p.rcap1 || p.vn)) return 2;   // (only the ring scatter reads segments / key validity)
    DPartArgs d1{};
    VNM_TRY(dense_scatter1(h, a, nrows, p, b, d1, s));
    if (p.levels == 2) VNM_TRY(dense_scatter2(h, p, b, d1, s));
    // the entries the final pass reads: the last level's regions
    DSet fin{b.v1, b.c1, b.n1, p.cap1, p.grid1, 1, p.grid1, 0};
    if (p.levels == 2) fin = DSet{b.v2, b.c2, b.n2, p.cap2, p.split2, 1, p.split2, 0};
    else if (p.pmajor) { fin.pstride = 1; fin.rstride = p.np1; }
    fin.pad = fin.cap < 2048 ? 1 : 0;   // small regions: one wave per region in the final pass
    b.take(b.rk, (size_t)p.dstride * 8 * 2);
    b.take(b.ra, (size_t)p.dstride * 8 * h->plan.n_words);
    if (!b.rk || !b.ra) return 1;
    DFinalArgs df{};
    df.map = h->dmap;
    df.vals = fin.vals; df.codes = fin.codes; df.counts = fin.counts; df.cap = fin.cap; df.regions = fin.regions; df.nfinal = p.nfinal;
    df.pstride = fin.pstride; df.rstride = fin.rstride;
    df.w_rows = a.hot_w_rows; df.w_valid = a.hot_w_valid; df.w_sum = a.hot_w_sum;
    df.w_lo = a.hot_comp && a.hot_w_sum >= 0 ? a.hot_w_sum + 1 : -1;
    df.dkey = b.rk; df.dacc = b.ra; df.dstride = p.dstride; df.flags = b.flags;
    df.fx_q = p.fx_q; df.fx_w32 = p.w32 ? 1 : 0;
    // the branches that write a run of their own: a pending (deferred) pass of earlier batches runs first and its run makes room
    const bool own_run = generic || !env_i64("VNM_DENSE_DEFER", 1);
    if (own_run && h->pending) {
        int rc = complete_pending(h, s);
        if (!rc) rc = merge_run_into_table(h, s);
        if (rc) return 1;
    }
    if (generic) {   // (count8 included: the generic kernels' view of the entries and the run)
        g.map = h->dmap; g.tbits = p.tb;
        g.pstride = fin.pstride; g.rstride = fin.rstride;
        g.vals = p.count8 ? nullptr : fin.vals; g.codes = fin.codes; g.counts = fin.counts; g.cap = fin.cap; g.regions = fin.regions; g.nfinal = p.nfinal;
        g.dkey = b.rk; g.dacc = b.ra; g.dstride = p.dstride; g.flags = b.flags;
    }
    if (p.count8) VNM_TRY(dense_final_count8(h, p, b, g, s));
    else if (generic) VNM_TRY(dense_final_generic(p, b, g, s));
    else if (p.fsplits > 1 && own_run) VNM_TRY(dense_final_split(p, b, df, s));
    else if (env_i64("VNM_DENSE_DEFER", 1)) {
        const int rc = dense_defer_final(h, a, nrows, p, b, fin, df, s, spill_out, n_spill_out);
        return rc == ATTEMPT_REDO ? redo() : rc;
    } else VNM_TRY(launch_dense_final(df, p.tb, DF_RUN, false, s));
    const int rc = dense_hand_over(h, a, nrows, p, b, s, spill_out, n_spill_out, nspill_out, n_nspill_out);
    return rc == ATTEMPT_REDO ? redo() : rc;
}

// ---- the dense-key path for TWO plain float64 input columns (round 4, VERDICT r03 #6): `SELECT k, sum(a), sum(b) [, avg, count ...]` used
// to take the hash partitions' wide entries (24-byte entries through two tile-sorting levels and LDS hash tables: 24 ms per 5e8 rows
// at G = 1e8).  Here the entry is (value 1, value 2, code remainder) -- 20 bytes after pass 1, 18 after pass 2 -- through the ring
// scatter (dring_scatter_kernel<..., V2>: a second ring array, 32-48 entries per ring in 148 KB of LDS) and a direct-addressed
// final pass with two compensated sums per slot (dpart_final2_kernel).  Ranges of 2^21 .. 2^27 codes; no spill buffer: an entry
// without a place (a key outside the sampled range, a full region) fails the pass and the batch takes the hash partitions.
// Its geometry, in the DensePlan fields of that name (no HIP call, the handle is left alone).  0, or 2 = not a range, a program or a fan-out it takes.
int plan_dense_two(const vnm_agg* h, const AggArgs& a, int64_t nrows, DensePlan* p) {
    const int cus = device_info().num_cus;
    const int bits = h->dmap.bits;
    p->tb = bits - 11 > 15 ? 12 : 11;
    const int pbits = bits - p->tb;
    if (pbits > 15 || pbits < 10 || a.has_expr) return 2;
    p->p2 = std::min(8, (pbits + 1) / 2); p->p1 = pbits - p->p2;      // (pass 1 moves the 20-byte entries: at most 128 rings of them fit)
    if (p->p1 > 7 || p->p1 < 5) return 2;
    const int np1 = p->np1 = 1 << p->p1, np2 = p->np2 = 1 << p->p2;
    const int64_t tiles = (nrows + PT_TILE - 1) / PT_TILE;
    const int grid1 = p->grid1 = (int)std::min<int64_t>((int64_t)cus * 2, tiles);
    p->split2 = std::max(2, (grid1 + PT_MAX_REGIONS - 1) / PT_MAX_REGIONS);
    p->split2 = std::max(p->split2, std::min(grid1, (cus * 2 + np1 - 1) / np1));
    const int64_t rows_per_wg = (tiles + grid1 - 1) / grid1 * PT_TILE;
    p->cap1 = ((rows_per_wg / np1 + rows_per_wg / np1 / 5 + 512) + 15) & ~15LL;
    if (((p->cap1 / 16) & 1) == 0) p->cap1 += 16;
    const int64_t per_pg = (int64_t)grid1 * rows_per_wg / np1 / p->split2;
    p->cap2 = ((per_pg / np2 + per_pg / np2 / 4 + 256) + 15) & ~15LL;
    if (((p->cap2 / 16) & 1) == 0) p->cap2 += 16;
    p->nfinal = (int64_t)1 << pbits;
    p->dstride = std::min<int64_t>(h->dense_span, nrows) + 2;
    // the rings of both levels (20- and 18-byte entries) must hold two flush blocks each
    const int lds_budget = (int)env_i64("VNM_DENSE_RING_LDS2", 148) * 1024;
    auto ring_cap = [&](int np, int esize) { return std::min(80, lds_budget / (np * esize) / DR_FB * DR_FB); };
    p->rcap1 = ring_cap(np1, 20); p->rcap2 = ring_cap(np2, 18);
    return p->rcap1 < 2 * DR_FB || p->rcap2 < 2 * DR_FB ? 2 : 0;
}

// Both scatter levels: rows -> (value 1, value 2, code remainder) entries in np1, then np1 x np2 partitions.  Two-value entries (V2):
// no round limit, no segments; two pairs of rows per lane where an even spread of the sub-tile fits one round.
int dense_two_scatters(const vnm_agg* h, const AggArgs& a, int64_t nrows, const DensePlan& p, const DenseBuffers& b, hipStream_t s) {
    DPartArgs d1{}, d2{};
    d1.map = d2.map = h->dmap; d1.flags = d2.flags = b.flags;
    d1.kp = (const uint64_t*)a.keys[0].values + a.keys[0].offset;
    d1.vp = (const double*)a.cols[0].values + a.cols[0].offset;
    d1.vp2 = (const double*)a.cols[1].values + a.cols[1].offset;
    fill_pred(d1, h, a);
    d1.nrows = nrows; d1.nt_store = 1; d1.ready_list = (int)env_i64("VNM_DENSE_READY_LIST", 1) & 1;
    d1.out_vals = b.v1; d1.out_vals2 = b.w1; d1.out_codes = b.c1; d1.out_counts = b.n1; d1.out_cap = p.cap1;
    d1.nparts = p.np1; d1.out_bits = h->dmap.bits - p.p1;
    {
        KernelTimer timer("agg_part_scatter1", s);
        VNM_TRY(pick_bool(h->pred_set && !a.hot_pred_is_v, [&](auto pv) {
            return pick_bool(ring_one_round(2, p.np1, p.rcap1, false), [&](auto two) {
                return launch_ring<true, uint32_t, true, decltype(two)::value ? 2 : 1, decltype(pv)::value, false, 0, false, false, true, false, false>(p.grid1, d1, p.rcap1, s);
            });
        }));
    }
    VNM_HIP(hipGetLastError());
    d2.in_vals = b.v1; d2.in_vals2 = b.w1; d2.in_codes = (const uint32_t*)b.c1; d2.in_counts = b.n1; d2.in_cap = p.cap1;
    d2.in_regions = p.grid1; d2.in_split = p.split2; d2.in_bits = d1.out_bits; d2.in_pstride = p.grid1; d2.in_rstride = 1;
    d2.out_vals = b.v2; d2.out_vals2 = b.w2; d2.out_codes = b.c2; d2.out_counts = b.n2; d2.out_cap = p.cap2;
    d2.nparts = p.np2; d2.out_bits = p.tb;
    {
        KernelTimer timer("agg_part_scatter2", s);
        VNM_TRY(pick_bool(ring_one_round(2, p.np2, p.rcap2, false), [&](auto two) {
            return launch_ring<false, uint16_t, true, decltype(two)::value ? 2 : 1, false, false, 0, false, false, true, false, false>(p.np1 * p.split2, d2, p.rcap2, s);
        }));
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

// returns 0 = done (run stored), 2 = not applicable / failed, 1 = error
int dense_two_aggregate(vnm_agg* h, const AggArgs& a, int64_t nrows, hipStream_t s) {
    const int cus = device_info().num_cus;
    DensePlan p{};
    VNM_TRY(plan_dense_two(h, a, nrows, &p));
    const size_t n1e = (size_t)p.np1 * p.grid1 * p.cap1, n2e = (size_t)p.np1 * p.np2 * p.split2 * p.cap2;   // entries of the levels' regions
    DenseBuffers b;
    b.take(b.flags, 64);
    b.take(b.v1, n1e * 8); b.take(b.w1, n1e * 8); b.take(b.c1, n1e * 4); b.take(b.n1, (size_t)p.np1 * p.grid1 * 4);
    b.take(b.v2, n2e * 8); b.take(b.w2, n2e * 8); b.take(b.c2, n2e * 2); b.take(b.n2, (size_t)p.np1 * p.np2 * p.split2 * 4);
    b.take(b.rk, (size_t)p.dstride * 8 * 2); b.take(b.ra, (size_t)p.dstride * 8 * h->plan.n_words);
    if (!b.flags || !b.v1 || !b.w1 || !b.c1 || !b.n1 || !b.v2 || !b.w2 || !b.c2 || !b.n2 || !b.rk || !b.ra) return 1;
    VNM_HIP(hipMemsetAsync(b.flags, 0, 64, s));
    VNM_TRY(dense_two_scatters(h, a, nrows, p, b, s));
    DFinalArgs df{};
    df.map = h->dmap; df.nfinal = p.nfinal; df.w_rows = a.hot_w[A_COUNT_ROWS];
    df.vals = b.v2; df.vals2 = b.w2; df.codes = b.c2; df.counts = b.n2; df.cap = p.cap2; df.regions = p.split2; df.pstride = p.split2; df.rstride = 1;
    df.w_valid = a.hot_w[A_COUNT_VALID]; df.w_sum = a.hot_w[A_SUM_F64]; df.w_lo = a.hot_comp && df.w_sum >= 0 ? df.w_sum + 1 : -1;
    df.w_valid2 = a.hot_w2[A_COUNT_VALID]; df.w_sum2 = a.hot_w2[A_SUM_F64]; df.w_lo2 = a.hot_comp && df.w_sum2 >= 0 ? df.w_sum2 + 1 : -1;
    df.dkey = b.rk; df.dacc = b.ra; df.dstride = p.dstride; df.flags = b.flags;
    {
        KernelTimer timer("agg_part_final", s);
        if (p.tb == 11) dpart_final2_kernel<uint16_t, 11><<<(int)std::min<int64_t>(p.nfinal, (int64_t)cus * 2), 512, 0, s>>>(df);
        else dpart_final2_kernel<uint16_t, 12><<<(int)std::min<int64_t>(p.nfinal, (int64_t)cus), 1024, 0, s>>>(df);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long fl[2] = {0, 0}; VNM_TRY(read_flags(fl, b.flags, s));
    if (getenv("VNM_AGG_TRACE"))
        fprintf(stderr, "[agg] dense, two columns: bits %d tb %d p1 %d p2 %d rings %d / %d -> fail %llu groups %llu\n", h->dmap.bits, p.tb, p.p1, p.p2, p.rcap1, p.rcap2, fl[0], fl[1]);
    if (fl[0]) return 2;
    b.pool.keep(b.rk); b.pool.keep(b.ra);
    adopt_run(h, b.rk, b.ra, p.dstride, (int64_t)fl[1]);
    return 0;
}

}  // namespace
