// Hash-partitioned path kernels (scatter levels, per-partition LDS aggregation), group-count sampling / HyperLogLog, multi-GPU bucketing and partition-aligned merge kernels.
// Part of the aggregate operator; included by vnm_agg.hip (one translation unit: the kernels and the host code share file-local helpers).
// =======================================================================================================
// Radix-partitioned aggregation for LARGE group counts (hot shape only).
//
// When the groups do not fit an LDS table, per-row updates would have to go to the HBM table, and agent
// scope atomics cap at ~24 G/s (profiles/microbench_r01.txt) -- 285 ms for the 1e9-row / 1e8-group query.
// Instead the surviving (key, value) pairs are radix partitioned by hash bits, streaming and atomic-free:
//   pass 1  rows -> 256 partitions           (filter fused; LDS counting sort per 8192-row tile, runs of
//                                              consecutive 16-byte entries written per partition)
//   pass 2  each partition -> 512 sub-parts   (same kernel, next hash bits; only when G > ~280k)
//   pass 3  one workgroup per final partition aggregates it in an LDS table and appends dense groups.
// Every (partition, producer) pair owns a private output region, so no cursor is shared.
// Traffic: 16 N read + 16 sN written/read per level + 24 G' written.
// =======================================================================================================
constexpr int PT_BLOCK = 1024;
#ifndef VNM_PT_ITEMS
#define VNM_PT_ITEMS 8   // 8192-item tiles: one workgroup per CU, but write runs twice as long (measured 14.1 vs 15.3 ms at G=1e8)
#endif
constexpr int PT_ITEMS = VNM_PT_ITEMS;
constexpr int PT_PAIRS = PT_ITEMS / 2;
constexpr int PT_TILE = PT_BLOCK * PT_ITEMS;  // 8192 rows or entries per tile
constexpr int PT_MAXP = 512;
constexpr int PT_MAX_REGIONS = 256;  // input regions per pass-2 workgroup (keeps two workgroups per CU in LDS)
constexpr int PA_BLOCK = 512;
constexpr int PA_SLOTS = 2048;

struct PartArgs {
    // source A: raw columns (pass 1)
    const uint64_t* kp;
    const double* vp;
    const double* pp;
    int has_pred, pred_is_v, op;
    double thr;
    int64_t nrows;
    int has_expr;        // the value is `expr` evaluated per row pair instead of vp[row]
    ExprProg expr;
    // source B: entry regions written by the previous level (pass 2)
    const ulonglong2* in_entries;
    const uint32_t* in_counts;
    int64_t in_cap;
    int in_regions;      // regions per input partition
    int in_split;        // workgroups per input partition (each takes in_regions / in_split regions)
    // output regions: region id = out_base(blockIdx) + p * out_stride
    ulonglong2* out_entries;
    uint32_t* out_counts;
    int64_t out_cap;
    int nparts;          // 256 or 512
    int shift;           // partition = (hash >> shift) & (nparts - 1)
    unsigned long long* flags;  // [0] failure (spill buffer full)  [2] entries in the spill buffer
    // entries that do not fit their region (skewed keys) are appended here and aggregated by agg_entries_kernel
    ulonglong2* spill;
    int64_t spill_cap;
    int debug;
    // wide entries (part_scatter_wide_kernel): key + nval raw values per entry
    vnm_dcol vcols[6];   // input columns (any numeric type, NULLs allowed)
    int nval;
    int has_vmask;       // last entry word = validity bits of the input columns (some column has a bitmap)
    Predicate wp;        // generic predicate over wpred (any type)
    vnm_dcol wpred;  // timing experiments (VNM_PART_DEBUG): 1 = no copy-out stores, 2 = no staging / copy-out at all
};

template <bool FROM_ROWS>
__global__ __launch_bounds__(PT_BLOCK) void part_scatter_kernel(PartArgs a) {
    __shared__ ulonglong2 stage[PT_TILE];
    __shared__ uint16_t part_of[PT_TILE];
    __shared__ uint32_t cnt[PT_MAXP], off[PT_MAXP], cursor[PT_MAXP];
    __shared__ uint32_t s_total, s_spill;
    __shared__ unsigned long long s_spill_base;
    __shared__ uint32_t wtot[PT_MAXP / 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int np = a.nparts;
    const uint32_t pmask = (uint32_t)np - 1;
    const int npad = np < 64 ? 64 : np;  // scan width: whole waves (counts beyond np stay zero)
    for (int i = tid; i < PT_MAXP; i += PT_BLOCK) { cnt[i] = 0; cursor[i] = 0; }
    if (tid == 0) s_spill = 0;
    __syncthreads();

    // output region of partition p for this producer
    int64_t out_base, out_stride;
    int64_t ntiles = 0, src_first = 0;
    if (FROM_ROWS) {
        out_base = blockIdx.x; out_stride = gridDim.x;
        ntiles = (a.nrows + PT_TILE - 1) / PT_TILE;
    } else {
        const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split;
        src_first = (int64_t)pin * a.in_regions;
    }

    // One tile = PT_TILE items.  get_item(k, &e) extracts item k of the CURRENT tile from registers;
    // prefetch_next() is called right after the last use of those registers (end of phase A) and issues the
    // loads of the NEXT tile into the same registers, so HBM reads stay in flight during phases B..E.
    auto process_tile = [&](auto&& get_item, auto&& prefetch_next) {
        // A: local rank inside the partition (LDS returning atomic)
        uint32_t myp[PT_ITEMS], myr[PT_ITEMS];
        ulonglong2 mye[PT_ITEMS];
#pragma unroll
        for (int k = 0; k < PT_ITEMS; k++) {
            myp[k] = 0xFFFFFFFFu;
            ulonglong2 e;
            if (get_item(k, &e)) {
                uint32_t p = (hash_u64(e.x) >> a.shift) & pmask;
                myp[k] = p;
                mye[k] = e;
                myr[k] = atomicAdd(&cnt[p], 1u);
            }
        }
        prefetch_next();
        __syncthreads();
        if (a.debug & 2) {
            if (tid < np) { cursor[tid] += cnt[tid]; cnt[tid] = 0; }
            __syncthreads();
            return;
        }
        // B: exclusive scan of cnt[0..np): wave scans, then the totals of the preceding waves are added
        if (tid < npad) {
            uint32_t c = cnt[tid], inc = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            off[tid] = inc - c;
            if (lane == 63) wtot[tid >> 6] = inc;
        }
        __syncthreads();
        if (tid < npad) {
            uint32_t add = 0;
            for (int w = 0; w < (tid >> 6); w++) add += wtot[w];
            off[tid] += add;
            if (tid == npad - 1) s_total = off[tid] + cnt[tid];
        }
        __syncthreads();
        // C: entries -> LDS stage, grouped by partition
#pragma unroll
        for (int k = 0; k < PT_ITEMS; k++) {
            if (myp[k] != 0xFFFFFFFFu) {
                uint32_t pos = off[myp[k]] + myr[k];
                stage[pos] = mye[k];
                part_of[pos] = (uint16_t)myp[k];
            }
        }
        __syncthreads();
        // D: copy out: consecutive lanes write consecutive 16-byte entries of one partition's run
        const uint32_t total = (a.debug & 1) ? 0 : s_total;
#pragma unroll
        for (int q = 0; q < PT_ITEMS; q++) {
            const uint32_t i = (uint32_t)q * PT_BLOCK + tid;
            if (i < total) {
                uint32_t p = part_of[i];
                uint32_t j = cursor[p] + (i - off[p]);
                if (j < (uint32_t)a.out_cap) a.out_entries[(out_base + (int64_t)p * out_stride) * a.out_cap + j] = stage[i];
                else atomicAdd(&s_spill, 1u);
            }
        }
        __syncthreads();
        // D2: regions that are full (a heavy key, an uneven split) spill into one global buffer: one global atomic per
        // tile.  The entries are found again here instead of being remembered above (that cost the common path 24
        // bytes of scratch per lane and 0.5 ms).
        const uint32_t nspill = s_spill;  // uniform: read by everyone before thread 0 resets it
        if (nspill) {
            __syncthreads();
            if (tid == 0) { s_spill_base = atomicAdd(&a.flags[2], (unsigned long long)nspill); s_spill = 0; }
            __syncthreads();
            const unsigned long long sb = s_spill_base;
            // the spill buffer itself full (more than half of the rows in overflowing regions): one flag store per tile,
            // not one per lost entry (agent-scope stores to one address serialise: 50 ms per 1e8 of them)
            if (tid == 0 && (int64_t)(sb + nspill) > a.spill_cap) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (uint32_t i = tid; i < total; i += PT_BLOCK) {
                uint32_t p = part_of[i];
                uint32_t j = cursor[p] + (i - off[p]);
                if (j < (uint32_t)a.out_cap) continue;
                const unsigned long long pos = sb + atomicAdd(&s_spill, 1u);
                if ((int64_t)pos < a.spill_cap) a.spill[pos] = stage[i];
            }
            __syncthreads();
            if (tid == 0) s_spill = 0;
            __syncthreads();
        }
        // E: advance cursors
        if (tid < np) { cursor[tid] += cnt[tid]; cnt[tid] = 0; }
        __syncthreads();
    };

    if (FROM_ROWS) {
        // two 16-byte loads per column: rows (base + 2 tid, +1) and (base + 2048 + 2 tid, +1)
        ulonglong2 kk[PT_PAIRS];
        double2 vv[PT_PAIRS], pv[PT_PAIRS];
        auto load_rows = [&](int64_t tile) {
            const int64_t base = tile * PT_TILE;
            if (tile < ntiles && base + PT_TILE <= a.nrows) {
#pragma unroll
                for (int u = 0; u < PT_PAIRS; u++) {
                    int64_t r = base + (int64_t)u * 2 * PT_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(a.kp + r);
                    vv[u] = a.has_expr ? expr_eval2(a.expr, r) : *(const double2*)(a.vp + r);
                    if (a.has_pred && !a.pred_is_v) pv[u] = *(const double2*)(a.pp + r);
                }
            }
        };
        load_rows(blockIdx.x);
        for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const int64_t base = tile * PT_TILE;
            const bool full = base + PT_TILE <= a.nrows;
            process_tile([&](int k, ulonglong2* e) -> bool {
                const int u = k >> 1, el = k & 1;
                int64_t r = base + (int64_t)u * 2 * PT_BLOCK + 2 * tid + el;
                if (r >= a.nrows) return false;
                uint64_t key; double v, p;
                if (full) {
                    key = el ? kk[u].y : kk[u].x;
                    v = el ? vv[u].y : vv[u].x;
                    p = a.pred_is_v ? v : (el ? pv[u].y : pv[u].x);
                } else {
                    key = a.kp[r]; v = a.has_expr ? expr_eval1(a.expr, r) : a.vp[r]; p = a.has_pred ? (a.pred_is_v ? v : a.pp[r]) : 0.0;
                }
                if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) return false;
                e->x = key;
                e->y = (unsigned long long)__double_as_longlong(v);
                return true;
            }, [&]() { load_rows(tile + gridDim.x); });
        }
    } else {
        // the input regions of this workgroup are read as ONE concatenated stream (prefix sums of the region
        // counts in LDS, binary search per item), so every tile is full
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        const int per_max = (a.in_regions + a.in_split - 1) / a.in_split;
        const int g = blockIdx.x % a.in_split;
        const int first = g * per_max;
        const int per = first + per_max <= a.in_regions ? per_max : (a.in_regions > first ? a.in_regions - first : 0);
        const int64_t region0 = src_first + first;
        if (tid == 0) {
            uint32_t run = 0;
            for (int rj = 0; rj < per; rj++) { rstart[rj] = run; run += a.in_counts[region0 + rj]; }
            rstart[per] = run;
        }
        __syncthreads();
        const uint32_t total_in = rstart[per];
        ulonglong2 eb[PT_ITEMS];
        // region of item k of the current tile: v grows by PT_TILE per tile, so the region index only ever moves
        // forward by a step or two -- a per-item cursor replaces a binary search over rstart (8 dependent LDS
        // reads per item, which made this pass load-latency bound: 3.9 of its 4.5 ms)
        int reg[PT_ITEMS];
#pragma unroll
        for (int k = 0; k < PT_ITEMS; k++) reg[k] = 0;
        auto load_entries = [&](uint32_t t0) {
#pragma unroll
            for (int k = 0; k < PT_ITEMS; k++) {
                uint32_t v = t0 + (uint32_t)k * PT_BLOCK + tid;
                if (v < total_in) {
                    int lo = reg[k];  // largest rj with rstart[rj] <= v (rstart[per] = total_in > v)
                    while (rstart[lo + 1] <= v) lo++;
                    reg[k] = lo;
                    eb[k] = a.in_entries[(region0 + lo) * a.in_cap + (v - rstart[lo])];
                }
            }
        };
        load_entries(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += PT_TILE) {
            process_tile([&](int k, ulonglong2* e) -> bool {
                uint32_t v = t0 + (uint32_t)k * PT_BLOCK + tid;
                if (v >= total_in) return false;
                *e = eb[k];
                return true;
            }, [&]() { load_entries(t0 + PT_TILE); });
        }
    }
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid] < (uint32_t)a.out_cap ? cursor[tid] : (uint32_t)a.out_cap;
}

// -------------------------------------------------------------------------------------------------------
// The RING form of part_scatter_kernel (round 6): (key, value) entries of 16 bytes go through per-partition rings in LDS and leave them in
// whole blocks of FB entries, as in the dense path's dring_scatter_kernel -- the tile-sorting scatter above stages a tile, sorts it by
// partition and writes runs of ~16-32 entries that start anywhere (half the ring scatter's rate: sparse keys, G = 1e8: 16.5 ms per 1e9 rows
// against 6.5 over a dense key range).  np partitions (<= 512) x cap entries fill 128 KB: cap = 32, FB = 16 (256-byte blocks) up to 256
// partitions, cap = 16, FB = 8 beyond.  No spill buffer and no expressions here: a full region, or a sub-tile that needs more than a few
// rounds (a heavy key), fails the attempt (flags[0]) and the batch is redone by part_scatter_kernel.  The flush walks the round's list of
// rings that completed a block.  Same regions, counts and entry format: part_agg_kernel reads either.
// -------------------------------------------------------------------------------------------------------
template <bool FROM_ROWS, int PAIRS, int FB, bool PV>
__global__ __launch_bounds__(PT_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void pring_scatter_kernel(PartArgs a, int ring_cap) {
    extern __shared__ ulonglong2 pr_ring[];              // [np][ring_cap]
    __shared__ uint32_t fill[PT_MAXP], head[PT_MAXP], cursor[PT_MAXP], s_retry[2], s_nready[2];
    __shared__ uint16_t ready[PT_MAXP];
    const RingState<uint32_t> rs{fill, head, cursor, s_retry, s_nready, ready};
    constexpr int NE = 2 * PAIRS;
    const int np = a.nparts, tid = threadIdx.x;
    const uint32_t pmask = (uint32_t)np - 1;
    ring_init<PT_BLOCK, PT_MAXP>(rs);
    int ph = 0;
    __syncthreads();
    int64_t out_base, out_stride;
    if (FROM_ROWS) { out_base = blockIdx.x; out_stride = gridDim.x; }
    else { const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split; out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split; }
    const uint32_t ocap = (uint32_t)a.out_cap;
    bool failed = false;

    // whole blocks of the listed rings (drain: of every ring, the partial last block too) -> the partition's region: FB lanes per ring, one entry each
    auto flush = [&](bool drain) {
        ring_flush<FB, FB, PT_BLOCK, false>(rs, ph, drain, true, np, (uint32_t)ring_cap, ocap, [&](int p, uint32_t src, int64_t dst, uint32_t n_here, int j, bool room) {
            if (!room) failed = true;     // (a full region: the attempt fails)
            else if ((uint32_t)j < n_here) a.out_entries[(out_base + (int64_t)p * out_stride) * a.out_cap + dst + j] = pr_ring[(size_t)p * ring_cap + src + j];
        });
    };
    auto rounds = [&](const ulonglong2 (&e)[NE], uint32_t okmask) {
        ring_rounds<NE>(rs, ph, okmask, [&](int k) -> bool {
            const uint32_t p = (hash_u64(e[k].x) >> a.shift) & pmask;
            const uint32_t slot = ring_reserve<FB>(rs, ph, p, (uint32_t)ring_cap, true);
            if (slot != RING_FULL) pr_ring[(size_t)p * ring_cap + slot] = e[k];
            return slot != RING_FULL;
        }, [&]() { flush(false); }, [&](int nr, uint32_t) {
            if (nr >= 6) failed = true;      // (skew: one ring takes a sub-tile's worth of entries -- part_scatter_kernel's business)
            return nr >= 6;
        });
    };

    if (FROM_ROWS) {
        const int64_t sub = (int64_t)NE * PT_BLOCK;
        const int64_t nsub = (a.nrows + sub - 1) / sub, nfull = a.nrows / sub;
        ulonglong2 kk[PAIRS];
        double2 vv[PAIRS], pv[PV ? PAIRS : 1];
        auto load_sub = [&](int64_t st) {
            if (st < nfull) {
#pragma unroll
                for (int u = 0; u < PAIRS; u++) {
                    const int64_t r = st * sub + (int64_t)u * 2 * PT_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(a.kp + r);
                    vv[u] = *(const double2*)(a.vp + r);
                    if (PV) pv[u] = *(const double2*)(a.pp + r);
                }
            }
        };
        load_sub(blockIdx.x);
        for (int64_t st = blockIdx.x; st < nsub; st += gridDim.x) {
            ulonglong2 e[NE]; uint32_t okmask = 0;
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const int u = k >> 1, el = k & 1;
                const int64_t r = st * sub + (int64_t)u * 2 * PT_BLOCK + 2 * tid + el;
                e[k] = make_ulonglong2(0ULL, 0ULL);
                if (r >= a.nrows) continue;
                uint64_t key; double v, p;
                if (st < nfull) {
                    key = el ? kk[u].y : kk[u].x;
                    v = el ? vv[u].y : vv[u].x;
                    p = PV ? (el ? pv[PV ? u : 0].y : pv[PV ? u : 0].x) : v;
                } else {
                    key = a.kp[r]; v = a.vp[r]; p = a.has_pred ? (a.pred_is_v ? v : a.pp[r]) : 0.0;
                }
                if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) continue;
                e[k].x = key; e[k].y = (unsigned long long)__double_as_longlong(v);
                okmask |= 1u << k;
            }
            load_sub(st + gridDim.x);
            rounds(e, okmask);
        }
    } else {
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        const RingRegions rg = ring_regions<1>(rstart, a.in_counts, a.in_regions, a.in_split, a.in_regions, 1);
        const uint32_t total_in = rg.total;
        ulonglong2 ev[NE];
        uint32_t okm = 0;
        int reg = 0;
        auto load_ent = [&](uint32_t t0) {
            okm = 0;
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const uint32_t v = t0 + (uint32_t)k * PT_BLOCK + tid;
                if (v < total_in) {
                    uint32_t e0;
                    const int64_t r = rg.region0 + ring_region_of<1>(rstart, reg, v, &e0);
                    ev[k] = a.in_entries[r * a.in_cap + e0];
                    okm |= 1u << k;
                }
            }
        };
        load_ent(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += NE * PT_BLOCK) {
            ulonglong2 e[NE];
#pragma unroll
            for (int k = 0; k < NE; k++) e[k] = ev[k];
            const uint32_t okmask = okm;
            load_ent(t0 + NE * PT_BLOCK);
            rounds(e, okmask);
        }
    }
    flush(true);
    __syncthreads();
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid];
    if (__syncthreads_or(failed ? 1 : 0) && tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// -------------------------------------------------------------------------------------------------------
// Wide entries: aggregates over 2-6 input columns carry (key, v1, v2[, v3 ...]) = E <= 7 8-byte words per entry.  Same
// passes and region bookkeeping as part_scatter_kernel, 4096-entry tiles (the LDS stage holds E words per entry),
// 8-byte column loads, no prefetch and no spill buffer: a straightforward version -- it only has to beat the HBM
// atomics of the general path (two input columns, G >= 1e5: 217-250 ms per 1e9 rows).
// -------------------------------------------------------------------------------------------------------
// items per lane and tile: one- and two-word entries get 8192-entry tiles (twice the run length), wider ones 4096
constexpr int pw_items(int E) { return E <= 2 ? 8 : (E <= 4 ? 4 : 2); }   // 2048-entry tiles for 5- to 7-word entries (up to 112 KB of LDS)
constexpr int pw_tile(int E) { return PT_BLOCK * pw_items(E); }
// IT: items per lane and tile (8 only for one- and two-word entries; pass 2 keeps 4 when it has few sub-partitions:
// its runs are long anyway and three resident workgroups beat one)
template <bool FROM_ROWS, int E, int IT>
__global__ __launch_bounds__(PT_BLOCK) void part_scatter_wide_kernel(PartArgs a) {
    constexpr int PW_ITEMS = IT, PW_TILE = PT_BLOCK * IT;
    extern __shared__ uint64_t wstage[];  // [PW_TILE][E]
    __shared__ uint16_t part_of[PW_TILE];
    __shared__ uint32_t cnt[PT_MAXP], off[PT_MAXP], cursor[PT_MAXP];
    __shared__ uint32_t s_total;
    __shared__ uint32_t s_over;   // a region of this workgroup is full and there is no spill buffer (or it is full too): the attempt is lost, stop working on it
    __shared__ uint32_t s_spill;
    __shared__ unsigned long long s_spill_base;
    __shared__ uint32_t wtot[PT_MAXP / 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int np = a.nparts;
    const uint32_t pmask = (uint32_t)np - 1;
    const int npad = np < 64 ? 64 : np;
    for (int i = tid; i < PT_MAXP; i += PT_BLOCK) { cnt[i] = 0; cursor[i] = 0; }
    if (tid == 0) { s_over = 0; s_spill = 0; }
    __syncthreads();
    uint64_t* const oute = (uint64_t*)a.out_entries;
    uint64_t* const spill = (uint64_t*)a.spill;   // [spill_cap][E] words: entries of full regions (heavy keys), as in part_scatter_kernel
    const uint64_t* const ine = (const uint64_t*)a.in_entries;
    int64_t out_base, out_stride;
    if (FROM_ROWS) { out_base = blockIdx.x; out_stride = gridDim.x; }
    else {
        const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split;
    }
    uint64_t ent[PW_ITEMS][E];
    auto process_tile = [&](uint32_t valid) {
        uint32_t myp[PW_ITEMS], myr[PW_ITEMS];
#pragma unroll
        for (int k = 0; k < PW_ITEMS; k++) {
            myp[k] = 0xFFFFFFFFu;
            if ((valid >> k) & 1u) {
                uint32_t p = (hash_u64(ent[k][0]) >> a.shift) & pmask;
                myp[k] = p;
                myr[k] = atomicAdd(&cnt[p], 1u);
            }
        }
        __syncthreads();
        if (tid < npad) {
            uint32_t c = cnt[tid], inc = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            off[tid] = inc - c;
            if (lane == 63) wtot[tid >> 6] = inc;
        }
        __syncthreads();
        if (tid < npad) {
            uint32_t add = 0;
            for (int w = 0; w < (tid >> 6); w++) add += wtot[w];
            off[tid] += add;
            if (tid == npad - 1) s_total = off[tid] + cnt[tid];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PW_ITEMS; k++) {
            if (myp[k] != 0xFFFFFFFFu) {
                uint32_t pos = off[myp[k]] + myr[k];
#pragma unroll
                for (int e = 0; e < E; e++) wstage[pos * E + e] = ent[k][e];
                part_of[pos] = (uint16_t)myp[k];
            }
        }
        __syncthreads();
        const uint32_t total = s_total;
        for (uint32_t i = tid; i < total; i += PT_BLOCK) {
            uint32_t p = part_of[i];
            uint32_t j = cursor[p] + (i - off[p]);
            if (j < (uint32_t)a.out_cap) {
                uint64_t* dst = oute + (((out_base + (int64_t)p * out_stride) * a.out_cap + j) * E);
#pragma unroll
                for (int e = 0; e < E; e++) dst[e] = wstage[i * E + e];
            } else if (spill) atomicAdd(&s_spill, 1u);
            else s_over = 1;   // (an agent-scope store per lost entry here: 1e8 rows of one heavy key = 50 ms of stores to one address)
        }
        __syncthreads();
        const uint32_t nspill = s_spill;  // uniform: read by everyone before thread 0 resets it
        if (nspill) {   // one global atomic per tile reserves the spilled entries' places; they are found again here
            __syncthreads();
            if (tid == 0) {
                s_spill_base = atomicAdd(&a.flags[2], (unsigned long long)nspill);
                s_spill = 0;
                if ((int64_t)(s_spill_base + nspill) > a.spill_cap) s_over = 1;
            }
            __syncthreads();
            const unsigned long long sb = s_spill_base;
            for (uint32_t i = tid; i < total; i += PT_BLOCK) {
                uint32_t p = part_of[i];
                uint32_t j = cursor[p] + (i - off[p]);
                if (j < (uint32_t)a.out_cap) continue;
                const unsigned long long pos = sb + atomicAdd(&s_spill, 1u);
                if ((int64_t)pos < a.spill_cap) {
#pragma unroll
                    for (int e = 0; e < E; e++) spill[pos * E + e] = wstage[i * E + e];
                }
            }
            __syncthreads();
            if (tid == 0) s_spill = 0;
        }
        __syncthreads();
        if (tid < np) { cursor[tid] += cnt[tid]; cnt[tid] = 0; }
        __syncthreads();
    };
    if (FROM_ROWS) {
        const int64_t ntiles = (a.nrows + PW_TILE - 1) / PW_TILE;
        for (int64_t tile = blockIdx.x; tile < ntiles && !s_over; tile += gridDim.x) {
            uint32_t valid = 0;
#pragma unroll
            for (int k = 0; k < PW_ITEMS; k++) {
                const int64_t row = tile * PW_TILE + (int64_t)k * PT_BLOCK + tid;
                const int64_t rc = row < a.nrows ? row : a.nrows - 1;
                if (row < a.nrows && (!a.wp.enabled || pred_eval(a.wp, a.wpred, rc))) valid |= 1u << k;
                ent[k][0] = a.kp[rc];
                uint64_t vmask = 0;
#pragma unroll
                for (int c = 0; c < E - 1; c++) {
                    if (c < a.nval) {
                        ent[k][1 + c] = col_raw_bits(a.vcols[c], rc);
                        if (col_valid(a.vcols[c], rc)) vmask |= 1ULL << c;
                    }
                }
                if (a.has_vmask) ent[k][E - 1] = vmask;
            }
            process_tile(valid);
        }
    } else {
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        const int pin = blockIdx.x / a.in_split;
        const int per_max = (a.in_regions + a.in_split - 1) / a.in_split;
        const int g = blockIdx.x % a.in_split;
        const int first = g * per_max;
        const int per = first + per_max <= a.in_regions ? per_max : (a.in_regions > first ? a.in_regions - first : 0);
        const int64_t region0 = (int64_t)pin * a.in_regions + first;
        if (tid == 0) {
            uint32_t run = 0;
            for (int rj = 0; rj < per; rj++) { rstart[rj] = run; run += a.in_counts[region0 + rj]; }
            rstart[per] = run;
        }
        __syncthreads();
        const uint32_t total_in = rstart[per];
        int reg[PW_ITEMS];
#pragma unroll
        for (int k = 0; k < PW_ITEMS; k++) reg[k] = 0;
        for (uint32_t t0 = 0; t0 < total_in && !s_over; t0 += PW_TILE) {
            uint32_t valid = 0;
#pragma unroll
            for (int k = 0; k < PW_ITEMS; k++) {
                uint32_t v = t0 + (uint32_t)k * PT_BLOCK + tid;
                if (v < total_in) {
                    int lo = reg[k];
                    while (rstart[lo + 1] <= v) lo++;
                    reg[k] = lo;
                    const uint64_t* src = ine + (((region0 + lo) * a.in_cap + (v - rstart[lo])) * E);
#pragma unroll
                    for (int e = 0; e < E; e++) ent[k][e] = src[e];
                    valid |= 1u << k;
                }
            }
            process_tile(valid);
        }
    }
    if (tid == 0 && s_over) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid] < (uint32_t)a.out_cap ? cursor[tid] : (uint32_t)a.out_cap;
}

struct PartAggArgs {
    const ulonglong2* entries;
    const uint32_t* counts;
    int64_t cap;
    int regions;          // regions per final partition
    int64_t nfinal;       // number of final partitions
    int w_rows, w_valid, w_sum, n_words;
    int w_lo;             // compensation word of the float64 sum (w_sum + 1), -1 = plain sum
    uint64_t* dkey;       // [2][dstride]
    uint64_t* dacc;       // [W][dstride]
    int64_t dstride;
    unsigned long long* flags;  // [0] overflow  [1] dense count
    // few final partitions: `splits` workgroups share one partition (regions rj % splits == part) and merge
    // their LDS tables into the HBM table instead of appending dense groups
    int splits;
    int to_table;
    GTable g;
    int64_t table_limit;
    unsigned long long* dir;  // [2 * nfinal]: (first dense row, row count) of every final partition, or NULL
    // generic accumulator program over the entry's value bits (part_agg_generic_kernel)
    int n_ops, vtype;
    int ent_words;   // 2 = (key, value); 3 / 4 = key + values [+ validity word] (wide entries)
    int has_vmask;   // wide entries: last word = validity bits of the input columns
    int wide;        // values are raw bits of any numeric width (vtypes[]), not 8-byte values of type vtype
    int vtypes[6];
    AccOp ops[AGG_MAX_OPS];
    int merge[AGG_MAX_WORDS];
    // the same program as a table (part_agg_generic_kernel, when every (kind, column) occurs once): 6 bits per
    // AccKind = accumulator word, 63 = absent; COUNT(*) separately.  Two scalar registers per column instead of
    // kernel-argument loads (and their lgkmcnt waits) inside the entry loop.
    unsigned long long wpack[6];
    int w_rows_g, use_table, nval;
    int slots;  // LDS table size of part_agg_generic_kernel
    int comp;   // float64 sums are compensated (hi, lo) pairs
};

// Find-or-claim the slot of `key` in a final-pass LDS table (PA_SLOTS keys).  The pass is bound by the number of
// instructions a wave issues per entry (PMC: ~250, half of them scalar exec-mask bookkeeping, at one instruction per
// ~4 cycles and SIMD), so the loop has ONE divergent region (the claim) and one exit; the number of claimed slots is
// counted per lane (*ins) and summed once per partition instead of one LDS atomic per claim.  -1 = no room.
constexpr int PA_MAX_PROBES = 256;
__device__ __forceinline__ int pa_find_slot(uint64_t* lkey, uint32_t smask, uint64_t key, uint32_t* ins, uint32_t* s_fail) {
    const uint32_t hv = hash_u64(key);
    uint32_t h = hv & smask;
    // double hashing: an odd step from hash bits the partitioning did not use ([14:11]).  A wave runs as long as its
    // unluckiest lane, and linear probing's clusters make that lane's chain long.
    const uint32_t step = ((hv >> 11) & 15u) * 2u + 1u;
    for (int probe = 0; probe < PA_MAX_PROBES; probe++) {
        uint64_t k = __hip_atomic_load(&lkey[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == EMPTY) {
            uint64_t expected = EMPTY;
            const bool won = __hip_atomic_compare_exchange_strong(&lkey[h], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            *ins += won ? 1u : 0u;
            k = won ? key : expected;
        }
        if (k == key) return (int)h;
        h = (h + step) & smask;
        if ((probe & 31) == 31 && __hip_atomic_load(s_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;  // the partition is lost anyway
    }
    return -1;
}

// sum of v over the block's lanes that call it (all of them), added to *dst by one lane per wave
__device__ __forceinline__ void pa_block_add(uint32_t* dst, uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__global__ __launch_bounds__(PA_BLOCK) __attribute__((amdgpu_waves_per_eu(6, 8))) void part_agg_kernel(PartAggArgs a) {
    // 48 KB per workgroup (40 KB before the compensation terms of the float64 sums: FOUR fitted a CU then, three now;
    // the pass is latency-bound: 1 / 2 / 3 / 4 resident workgroups ran at 5.6 / 3.3 / 2.6 / 2.4 ms).  The last PA_DEAD slots of the key table are never used (they hold a reserved marker that
    // probes step over), which pays for the scalars below and for the accumulators of the two keys that cannot live in
    // the table: EMPTY (the free marker) and PA_RESERVED itself, at lsum / lcnt [PA_LIVE] and [PA_LIVE + 1].
    constexpr int PA_DEAD = 8, PA_LIVE = PA_SLOTS - PA_DEAD;
    constexpr uint64_t PA_RESERVED = EMPTY - 1;
    __shared__ uint64_t lkey[PA_SLOTS];
    __shared__ uint64_t lsum[PA_LIVE + 2];
    // compensation terms of the float64 sums (M_ADD_F64C) in SINGLE precision: they are ~2^-53 of the sum, so 24 bits of
    // them keep hi + lo within 2^-77; a float64 array would cost the fourth resident workgroup.  An error term beyond
    // float range (|sum| > ~1e54) fails the partition over to the general path; one below it (|sum| < ~1e-22) is dropped.
    __shared__ float llo[PA_LIVE + 2];
    __shared__ uint32_t lcnt[PA_LIVE + 2];
    __shared__ uint32_t s_n, s_fail, s_sp[2];
    __shared__ unsigned s_new;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t smask = PA_SLOTS - 1;
    if (tid == 0) s_new = 0;
    for (int64_t unit = blockIdx.x; unit < a.nfinal * a.splits; unit += gridDim.x) {
        const int64_t f = unit / a.splits;
        const int part = (int)(unit % a.splits);
        for (int i = tid; i < PA_SLOTS; i += PA_BLOCK) {
            lkey[i] = i < PA_LIVE ? EMPTY : PA_RESERVED;
            if (i < PA_LIVE + 2) { lsum[i] = F64_NEG_ZERO; lcnt[i] = 0; llo[i] = 0.0f; }
        }
        if (tid == 0) { s_n = 0; s_fail = 0; s_sp[0] = 0; s_sp[1] = 0; }
        __syncthreads();
        uint32_t ins = 0;  // slots this lane claimed in this partition's table
        for (int rj = part; rj < a.regions; rj += a.splits) {
            const int64_t region = f * a.regions + rj;
            const uint32_t n = a.counts[region];
            const ulonglong2* src = a.entries + region * a.cap;
            for (uint32_t i0 = 0; i0 < n; i0 += PA_BLOCK * 4) {
              // four independent 16-byte loads in flight per lane before the (serial) LDS insertions
              ulonglong2 eb[4];
#pragma unroll
              for (int u = 0; u < 4; u++) {
                  uint32_t i = i0 + (uint32_t)u * PA_BLOCK + tid;
                  if (i < n) eb[u] = src[i];
              }
#pragma unroll
              for (int u = 0; u < 4; u++) {
                uint32_t i = i0 + (uint32_t)u * PA_BLOCK + tid;
                if (i >= n) continue;
                ulonglong2 e = eb[u];
                const uint64_t key = e.x;
                int slot;
                if (key >= PA_RESERVED) { const int sp = key == EMPTY ? 0 : 1; slot = PA_LIVE + sp; s_sp[sp] = 1; }
                else {
                    slot = pa_find_slot(lkey, smask, key, &ins, &s_fail);
                    if (slot < 0) s_fail = 1;
                }
                if (slot >= 0) {
                    const double x = __longlong_as_double((long long)e.y);
                    if (a.w_lo >= 0) {
                        const double old = __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const double er = two_sum_err(old, x, old + x);
                        if (er != 0.0) {
                            const float ef = (float)er;
                            if (ef - ef != 0.0f) s_fail = 1;
                            __hip_atomic_fetch_add(&llo[slot], ef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    } else __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    atomicAdd(&lcnt[slot], 1u);
                }
              }
            }
        }
        pa_block_add(&s_n, ins);
        __syncthreads();
        if (s_fail) {  // more groups than the LDS table holds: tell the host to use the general path
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (a.to_table) {
            // merge this workgroup's table into the HBM table (G * splits * words atomics in total: small)
            if (tid == 0) {
                fold_new(a.g, &s_new);
                unsigned long long fill = __hip_atomic_load(&a.g.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int64_t)(fill + s_n) > a.table_limit) s_fail = 1;
            }
            __syncthreads();
            if (s_fail) {
                if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            for (int i = tid; i < PA_LIVE + 2; i += PA_BLOCK) {
                uint64_t k = i < PA_LIVE ? lkey[i] : (s_sp[i - PA_LIVE] ? (i == PA_LIVE ? 0 : PA_RESERVED) : EMPTY);
                if (k == EMPTY) continue;
                uint64_t slot;
                if (i != PA_LIVE) slot = gt_find_single(a.g, k, &s_new);
                else { slot = a.g.cap; if (ld_agent(&a.g.tag[slot]) == EMPTY) st_agent(&a.g.tag[slot], 0); }
                if (a.w_rows >= 0) g_merge(&a.g.acc[(uint64_t)a.w_rows * a.g.stride + slot], M_ADD_U64, lcnt[i], 0);
                if (a.w_valid >= 0) g_merge(&a.g.acc[(uint64_t)a.w_valid * a.g.stride + slot], M_ADD_U64, lcnt[i], 0);
                if (a.w_sum >= 0) g_merge(&a.g.acc[(uint64_t)a.w_sum * a.g.stride + slot], a.w_lo >= 0 ? M_ADD_F64C : M_ADD_F64, lsum[i], (int64_t)a.g.stride);
                if (a.w_lo >= 0 && llo[i] != 0.0f)
                    g_merge(&a.g.acc[(uint64_t)a.w_lo * a.g.stride + slot], M_ADD_F64, (uint64_t)__double_as_longlong((double)llo[i]), 0);
            }
            __syncthreads();
            if (tid == 0) fold_new(a.g, &s_new);
            continue;
        }
        // compact: reserve a dense range for this partition's groups, then write them
        const uint32_t ngroups = s_n + s_sp[0] + s_sp[1];
        __syncthreads();
        if (tid == 0) {
            s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups);
            s_n = 0;
            if (a.dir) { a.dir[2 * f] = s_base; a.dir[2 * f + 1] = ngroups; }
        }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < PA_LIVE + 2; i0 += PA_BLOCK) {
            int i = i0 + tid;
            bool occ = i < PA_LIVE ? lkey[i] != EMPTY : (i < PA_LIVE + 2 && s_sp[i - PA_LIVE] != 0);
            uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                a.dkey[pos] = i < PA_LIVE ? lkey[i] : (i == PA_LIVE ? EMPTY : PA_RESERVED);
                a.dkey[a.dstride + pos] = 0;
                if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = lcnt[i];
                if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = lcnt[i];
                if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = lsum[i];
                if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong((double)llo[i]);
            }
        }
        __syncthreads();
    }
}

// value an op contributes for an entry whose input value has the raw bits `vb` (type `vtype`, never NULL here)
__device__ __forceinline__ uint64_t op_value_bits(int kind, int vtype, uint64_t vb) {
    switch (kind) {
        case A_COUNT_ROWS:
        case A_COUNT_VALID: return 1;
        case A_SUM_F64: return vtype == VNM_F64 ? vb : (uint64_t)__double_as_longlong((double)(int64_t)vb);
        case A_SUM_I64: return vb;
        case A_SUM_LO32: return vb & 0xFFFFFFFFULL;
        case A_SUM_HI32S: return (uint64_t)((int64_t)vb >> 32);
        case A_SUM_HI32U: return vb >> 32;
        default:  // A_MIN / A_MAX on the order-preserving encoding
            if (vtype == VNM_F64) return enc_f64(__longlong_as_double((long long)vb));
            if (vtype == VNM_U64) return vb;
            return enc_i64((int64_t)vb);
    }
}

// every accumulator word of ONE input column (packed word table, see PartAggArgs::wpack) for a non-NULL value with
// the raw bits `raw` of type `type`
__device__ __forceinline__ void pa_accumulate_col(unsigned long long pack, int type, uint64_t* lw, int ST, int slot, uint64_t raw, int comp) {
#define VNM_WI(K) ((int)((pack >> (6 * (K))) & 63ULL))
#define VNM_W(K) (lw + VNM_WI(K) * ST + slot)
#define VNM_ADD(K, V) if (VNM_WI(K) != 63) __hip_atomic_fetch_add(VNM_W(K), (uint64_t)(V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
    VNM_ADD(A_COUNT_VALID, 1ULL);
    if (VNM_WI(A_SUM_F64) != 63) {
        if (comp) l_add_f64c(VNM_W(A_SUM_F64), ST, raw_to_f64(type, raw));  // (hi, lo) pair: lo is the next word
        else __hip_atomic_fetch_add((double*)VNM_W(A_SUM_F64), raw_to_f64(type, raw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (((pack >> (6 * A_SUM_I64)) & 0xFFFFFFULL) != 0xFFFFFFULL) {  // any of the four integer-sum kinds (consecutive AccKinds)
        const uint64_t iv = (uint64_t)raw_to_i64(type, raw);
        VNM_ADD(A_SUM_I64, iv);
        VNM_ADD(A_SUM_LO32, iv & 0xFFFFFFFFULL);
        VNM_ADD(A_SUM_HI32S, (int64_t)iv >> 32);
        VNM_ADD(A_SUM_HI32U, iv >> 32);
    }
    if (VNM_WI(A_MIN) != 63 || VNM_WI(A_MAX) != 63) {
        const uint64_t e = type_is_float(type) ? enc_f64(raw_to_f64(type, raw))
                                               : (type_is_unsigned(type) ? (uint64_t)raw_to_i64(type, raw) : enc_i64(raw_to_i64(type, raw)));
        if (VNM_WI(A_MIN) != 63) __hip_atomic_fetch_min(VNM_W(A_MIN), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (VNM_WI(A_MAX) != 63) __hip_atomic_fetch_max(VNM_W(A_MAX), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#undef VNM_ADD
#undef VNM_W
#undef VNM_WI
}

// Final pass of the partitioned path for ANY accumulator program over one 8-byte input column (or none):
// same protocol as part_agg_kernel, W accumulator words per LDS slot.  LDS: lkey[S + 1], lw[W][S + 1].
// TABLE: the accumulator program as packed word tables (PartAggArgs::wpack) -- the normal case; the op loop is only
// compiled into the <E, false> instances (it costs registers: 89+ VGPRs and scratch left two workgroups per CU).
template <int E, bool TABLE>
__global__ __launch_bounds__(PA_BLOCK) __attribute__((amdgpu_waves_per_eu(6, 8))) void part_agg_generic_kernel(PartAggArgs a) {
    extern __shared__ uint64_t pa_lds[];
    __shared__ uint32_t s_n, s_fail;
    __shared__ unsigned s_new;
    __shared__ unsigned long long s_base;
    const int SL = a.slots;  // 2048, or 1024 for programs with many accumulator words (LDS per workgroup decides how many are resident)
    const int ST = SL + 1;
    uint64_t* lkey = pa_lds;
    uint64_t* lw = pa_lds + ST;
    const int W = a.n_words;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t smask = (uint32_t)SL - 1;
    if (tid == 0) s_new = 0;
    for (int64_t unit = blockIdx.x; unit < a.nfinal * a.splits; unit += gridDim.x) {
        const int64_t f = unit / a.splits;
        const int part = (int)(unit % a.splits);
        for (int i = tid; i < ST; i += PA_BLOCK) lkey[i] = EMPTY;
        for (int w = 0; w < W; w++) {
            const uint64_t init = merge_init(a.merge[w]);
            for (int i = tid; i < ST; i += PA_BLOCK) lw[w * ST + i] = init;
        }
        if (tid == 0) { s_n = 0; s_fail = 0; }
        __syncthreads();
        uint32_t ins = 0;  // slots this lane claimed in this partition's table
        for (int rj = part; rj < a.regions; rj += a.splits) {
            const int64_t region = f * a.regions + rj;
            const uint32_t n = a.counts[region];
            const uint64_t* src = (const uint64_t*)a.entries + region * a.cap * E;
            for (uint32_t i0 = 0; i0 < n; i0 += PA_BLOCK * 4) {
                uint64_t eb[4][E];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t i = i0 + (uint32_t)u * PA_BLOCK + tid;
                    if (i < n) {
                        if (E == 2) { const ulonglong2 t = ((const ulonglong2*)src)[i]; eb[u][0] = t.x; eb[u][1] = t.y; }
                        else {
#pragma unroll
                            for (int e = 0; e < E; e++) eb[u][e] = src[(size_t)i * E + e];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t i = i0 + (uint32_t)u * PA_BLOCK + tid;
                    if (i >= n) continue;
                    const uint64_t key = eb[u][0];
                    int slot;
                    if (key == EMPTY) { slot = SL; lkey[slot] = 0; }
                    else {
                        slot = pa_find_slot(lkey, smask, key, &ins, &s_fail);
                        if (slot < 0) s_fail = 1;
                    }
                    if (slot >= 0 && TABLE) {
                        const uint64_t vmask = (E > 2 && a.has_vmask) ? eb[u][E - 1] : ~0ULL;
                        if (a.w_rows_g >= 0) __hip_atomic_fetch_add(&lw[a.w_rows_g * ST + slot], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                        for (int c = 0; c < E - 1; c++) {
                            if (c < a.nval && (E == 2 || ((vmask >> c) & 1ULL)))  // a NULL input updates nothing of its column
                                pa_accumulate_col(a.wpack[c], a.vtypes[c], lw, ST, slot, eb[u][1 + c], a.comp);
                        }
                    } else if (slot >= 0 && !TABLE) {
                        const uint64_t vmask = (E > 2 && a.has_vmask) ? eb[u][E - 1] : ~0ULL;
                        for (int o = 0; o < a.n_ops; o++) {
                            const int w = a.ops[o].word;
                            const int c = E == 2 ? 0 : (a.ops[o].col < 0 ? 0 : a.ops[o].col);
                            if (E > 2 && a.ops[o].kind != A_COUNT_ROWS && !((vmask >> c) & 1ULL)) continue;  // NULL input
                            uint64_t vb = E >= 2 ? eb[u][E >= 2 ? 1 : 0] : 0;
#pragma unroll
                            for (int e = 2; e < E; e++) if (c == e - 1) vb = eb[u][e];
                            const uint64_t v = a.wide ? op_value_raw(a.ops[o].kind, a.vtypes[c], vb)  // any numeric type
                                                      : op_value_bits(a.ops[o].kind, a.vtype, vb);
                            l_merge(&lw[w * ST + slot], a.merge[w], v, ST);
                        }
                    }
                }
            }
        }
        pa_block_add(&s_n, ins);
        __syncthreads();
        if (s_fail) {  // more groups than the LDS table holds: tell the host to use the general path
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (a.to_table) {
            if (tid == 0) {
                fold_new(a.g, &s_new);
                unsigned long long fill = __hip_atomic_load(&a.g.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int64_t)(fill + s_n) > a.table_limit) s_fail = 1;
            }
            __syncthreads();
            if (s_fail) {
                if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            for (int i = tid; i < ST; i += PA_BLOCK) {
                uint64_t k = lkey[i];
                if (k == EMPTY) continue;
                uint64_t slot;
                if (i < SL) slot = gt_find_single(a.g, k, &s_new);
                else { slot = a.g.cap; if (ld_agent(&a.g.tag[slot]) == EMPTY) st_agent(&a.g.tag[slot], 0); }
                for (int w = 0; w < W; w++) {
                    uint64_t v = lw[w * ST + i];
                    if (v != merge_init(a.merge[w])) g_merge(&a.g.acc[(uint64_t)w * a.g.stride + slot], a.merge[w], v, (int64_t)a.g.stride);
                }
            }
            __syncthreads();
            if (tid == 0) fold_new(a.g, &s_new);
            continue;
        }
        const uint32_t ngroups = s_n + (lkey[SL] != EMPTY ? 1u : 0u);
        __syncthreads();
        if (tid == 0) {
            s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups);
            s_n = 0;
            if (a.dir) { a.dir[2 * f] = s_base; a.dir[2 * f + 1] = ngroups; }
        }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < ST; i0 += PA_BLOCK) {
            int i = i0 + tid;
            bool occ = i < ST && lkey[i] != EMPTY;
            uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                a.dkey[pos] = i == SL ? EMPTY : lkey[i];
                a.dkey[a.dstride + pos] = 0;
                for (int w = 0; w < W; w++) a.dacc[(int64_t)w * a.dstride + pos] = lw[w * ST + i];
            }
        }
        __syncthreads();
    }
}

// Cardinality estimate for operators that were given no hint: insert a strided sample of the keys into a
// scratch table (tags only) and count the distinct ones.  Solving d = G (1 - exp(-m / G)) for G (uniform
// model) on the host then sizes the partitions; an underestimate only costs the fallback to the general path.
// (kvalid: the key column's validity bitmap or null -- rows whose key is NULL are not part of any sample: their value words are garbage)
__device__ __forceinline__ bool key_row_valid(const uint8_t* kvalid, int64_t koff, int64_t row) {
    return !kvalid || ((kvalid[(koff + row) >> 3] >> ((koff + row) & 7)) & 1);
}
__global__ void agg_sample_kernel(const uint64_t* keys, int64_t nrows, int64_t m, GTable g, unsigned int* cnt, const uint8_t* kvalid, int64_t koff) {
    __shared__ unsigned s_new;
    if (threadIdx.x == 0) s_new = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        int64_t row = (int64_t)(((__int128)i * nrows) / m);
        uint64_t key = keys[row];
        uint64_t slot = ~0ULL;
        if (key != EMPTY && key_row_valid(kvalid, koff, row)) {
            slot = gt_find_single(g, key, &s_new);
            if (slot >= g.cap) slot = ~0ULL;
        }
        // per-key sample counts (the heavy keys' share of the rows).  A heavy key means most lanes of a wave hold the
        // same slot, and atomics on one address serialise (half of the sample one key: 3 ms; seven groups: +0.2 ms on a 3 ms
        // query): up to eight rounds pick the first pending lane's slot and add all its lanes at once.
        const int lane = threadIdx.x & 63;
        for (int r = 0; r < 8; r++) {
            const unsigned long long pending = __ballot(slot != ~0ULL);
            if (!pending) break;
            const uint64_t first = __shfl(slot, __ffsll((long long)pending) - 1);
            const unsigned long long same = __ballot(slot == first);
            if (slot == first) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&cnt[first], (unsigned int)__popcll(same));
                slot = ~0ULL;
            }
        }
        if (slot != ~0ULL) atomicAdd(&cnt[slot], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) fold_new(g, &s_new);
}
// keys with more than `thresh` sample rows: ctl[4] += their rows, ctl[5] += their number
__global__ void agg_sample_heavy_kernel(const unsigned int* cnt, int64_t slots, unsigned int thresh, unsigned long long* ctl) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long rows = 0, keys = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
        const unsigned int c = cnt[i];
        if (c > thresh) { rows += c; keys++; }
    }
    if (rows) { atomicAdd(&ctl[4], rows); atomicAdd(&ctl[5], keys); }
}

// HyperLogLog over a strided sample (4096 registers, ~1.6 % error): LDS max per workgroup, then one
// agent-scope max per register per workgroup.  Used for the large sample tier, where inserting every key into
// a scratch table would cost tens of milliseconds of atomics.
constexpr int HLL_BITS = 12;
constexpr int HLL_M = 1 << HLL_BITS;
__global__ __launch_bounds__(1024) void agg_hll_kernel(const uint64_t* keys, int64_t nrows, int64_t m, unsigned int* regs, const uint8_t* kvalid, int64_t koff) {
    __shared__ unsigned int lreg[HLL_M];
    for (int i = threadIdx.x; i < HLL_M; i += blockDim.x) lreg[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        int64_t row = (int64_t)(((__int128)i * nrows) / m);
        if (!key_row_valid(kvalid, koff, row)) continue;
        uint64_t key = keys[row];
        uint64_t h = ((uint64_t)hash_u64(key) << 32) | hash_u64(key * 0x9E3779B97F4A7C15ULL + 0x7F4A7C15ULL);
        unsigned idx = (unsigned)(h & (HLL_M - 1));
        uint64_t rest = h >> HLL_BITS;
        unsigned rank = rest ? (unsigned)__clzll((long long)(rest << HLL_BITS)) + 1u : (unsigned)(64 - HLL_BITS + 1);
        atomicMax(&lreg[idx], rank);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HLL_M; i += blockDim.x)
        if (lreg[i]) atomicMax(&regs[i], lreg[i]);
}

// ---- multi-GPU: bucket the dense run by owner rank -------------------------------------------------------
// owner(key words) must equal vinum_amd/distributed.py::owner_of (int64 wrap-around arithmetic).
__device__ __forceinline__ int owner_of_words(const uint64_t* const* kw, int nkw, int64_t i, int world) {
    int64_t hh = 0;
    for (int j = 0; j < nkw; j++) {
        hh = (int64_t)(((uint64_t)hh ^ kw[j][i]) * 0x9E3779B97F4A7C15ULL);
        hh ^= (hh >> 29);  // arithmetic shift, like torch's int64 >>
    }
    return (int)(((hh >> 17) & 0x7FFFFFFF) % world);
}

struct BucketArgs {
    const uint64_t* words[AGG_MAX_KEYS + 1 + AGG_MAX_WORDS];
    int nkw, nw;      // key words, total words
    int64_t n, per;   // rows, rows per block (block b owns the contiguous rows [b*per, (b+1)*per))
    int world, nb;
    unsigned long long* blk;       // [world][nb] per-block counts (pass 0) -> exclusive offsets (after the scan)
    unsigned long long* totals;    // [world]
    uint64_t* out;                 // [n][nw] row-major, grouped by owner
};

// A stable, atomic-free partition by owner (a one-digit radix scatter): per-block counts, one scan, then every
// block re-reads its rows and places them with ballot ranks.  (A shared cursor per owner serialises on one
// atomic word: 37 ms per 1e8 groups.)
constexpr int BK_MAX_WORLD = 64;

__global__ __launch_bounds__(256) void agg_bucket_count_kernel(BucketArgs b) {
    __shared__ unsigned cnt[BK_MAX_WORLD];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < BK_MAX_WORLD) cnt[tid] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * b.per, hi = lo + b.per < b.n ? lo + b.per : b.n;
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t i = base + tid;
        const int own = i < hi ? owner_of_words(b.words, b.nkw, i, b.world) : -1;
        for (int o = 0; o < b.world; o++) {
            uint64_t m = __ballot(own == o);
            if (m && lane == 0) atomicAdd(&cnt[o], (unsigned)__popcll(m));
        }
    }
    __syncthreads();
    if (tid < b.world) b.blk[(int64_t)tid * b.nb + blockIdx.x] = cnt[tid];
}

__global__ void agg_bucket_scan_kernel(BucketArgs b) {
    __shared__ unsigned long long tot[BK_MAX_WORLD];
    const int o = threadIdx.x;
    if (o < b.world) {
        unsigned long long s = 0;
        for (int k = 0; k < b.nb; k++) s += b.blk[(int64_t)o * b.nb + k];
        tot[o] = s;
        b.totals[o] = s;
    }
    __syncthreads();
    if (o < b.world) {
        unsigned long long run = 0;
        for (int k = 0; k < o; k++) run += tot[k];
        for (int k = 0; k < b.nb; k++) {
            unsigned long long c = b.blk[(int64_t)o * b.nb + k];
            b.blk[(int64_t)o * b.nb + k] = run;
            run += c;
        }
    }
}

__global__ __launch_bounds__(256) void agg_bucket_scatter_kernel(BucketArgs b) {
    __shared__ unsigned long long run[BK_MAX_WORLD];
    __shared__ unsigned wcount[4][BK_MAX_WORLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < b.world) run[tid] = b.blk[(int64_t)tid * b.nb + blockIdx.x];
    for (int i = tid; i < 4 * BK_MAX_WORLD; i += 256) (&wcount[0][0])[i] = 0;
    __syncthreads();
    const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
    const int64_t lo = (int64_t)blockIdx.x * b.per, hi = lo + b.per < b.n ? lo + b.per : b.n;
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t i = base + tid;
        const int own = i < hi ? owner_of_words(b.words, b.nkw, i, b.world) : -1;
        unsigned rank = 0;
        for (int o = 0; o < b.world; o++) {
            uint64_t m = __ballot(own == o);
            if (own == o) rank = __popcll(m & lt);
            if (m && lane == 0) wcount[wave][o] = (unsigned)__popcll(m);
        }
        __syncthreads();
        if (own >= 0) {
            unsigned long long pos = run[own] + rank;
            for (int w = 0; w < wave; w++) pos += wcount[w][own];
            for (int w = 0; w < b.nw; w++) b.out[pos * b.nw + w] = b.words[w][i];
        }
        __syncthreads();
        if (tid < b.world) {
            unsigned s = 0;
            for (int w = 0; w < 4; w++) { s += wcount[w][tid]; wcount[w][tid] = 0; }
            run[tid] += s;
        }
        __syncthreads();
    }
}

// ---- partition-aligned multi-GPU exchange ------------------------------------------------------------------
// The partitioned path leaves the groups of final partition f contiguous (directory dir[f] = (first row, rows)).
// Every rank uses the same hash bits, so partition f holds the same keys everywhere and owner(f) = f * P / F.
// Sender: rows are copied in partition order (row-major [key, nullmask, words...]).  Owner: one workgroup per
// owned partition loads that partition's segments from all P sources into an LDS table and writes the merged
// groups -- streaming, no HBM atomics.
struct RunReorderArgs {
    const uint64_t* words[2 + AGG_MAX_WORDS];
    int nw;                            // 2 key words + accumulator words
    int64_t nfin;
    const unsigned long long* dir;     // [2 * nfin]
    unsigned long long* prefix;        // [nfin + 1] exclusive prefix of the row counts (in partition order)
    uint64_t* out;                     // [n][nw]
    uint32_t* part_counts;             // [nfin]
};

__global__ void run_prefix_kernel(RunReorderArgs a) {  // single block: serial over chunks, parallel inside
    __shared__ unsigned long long carry;
    __shared__ unsigned long long wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < a.nfin; base += blockDim.x) {
        int64_t f = base + tid;
        unsigned long long c = f < a.nfin ? a.dir[2 * f + 1] : 0, inc = c;
        for (int d = 1; d < 64; d <<= 1) { unsigned long long o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned long long add = carry;
        for (int w = 0; w < wave; w++) add += wsum[w];
        if (f < a.nfin) { a.prefix[f] = add + inc - c; a.part_counts[f] = (uint32_t)c; }
        __syncthreads();
        if (tid == blockDim.x - 1) carry = add + inc;
        __syncthreads();
    }
    if (tid == 0) a.prefix[a.nfin] = carry;
}

__global__ __launch_bounds__(256) void run_reorder_kernel(RunReorderArgs a) {
    for (int64_t f = blockIdx.x; f < a.nfin; f += gridDim.x) {
        const unsigned long long src = a.dir[2 * f], cnt = a.dir[2 * f + 1], dst = a.prefix[f];
        for (unsigned long long e = threadIdx.x; e < cnt * a.nw; e += blockDim.x) {
            unsigned long long r = e / a.nw;
            int w = (int)(e % a.nw);
            a.out[(dst + r) * a.nw + w] = a.words[w][src + r];
        }
    }
}

struct PartMergeArgs {
    const uint64_t* rows;              // all received rows, grouped by source rank, each in partition order
    const unsigned long long* src_prefix;  // [world][nlocal + 1] row offsets (absolute, into rows)
    int world;
    int64_t nlocal;
    int nw, n_words;
    int merge[AGG_MAX_WORDS];
    uint64_t* dkey;                    // [2][dstride]
    uint64_t* dacc;                    // [W][dstride]
    int64_t dstride;
    unsigned long long* flags;         // [0] overflow [1] dense count
};
constexpr int PM_MAX_WORDS = 3;

__global__ __launch_bounds__(PA_BLOCK) void part_merge_kernel(PartMergeArgs a) {
    __shared__ uint64_t lkey[PA_SLOTS + 1];
    __shared__ uint64_t lw[PM_MAX_WORDS][PA_SLOTS + 1];
    __shared__ uint32_t s_n, s_fail;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t smask = PA_SLOTS - 1;
    for (int64_t f = blockIdx.x; f < a.nlocal; f += gridDim.x) {
        for (int i = tid; i <= PA_SLOTS; i += PA_BLOCK) {
            lkey[i] = EMPTY;
            for (int w = 0; w < a.n_words; w++) lw[w][i] = 0;
        }
        if (tid == 0) { s_n = 0; s_fail = 0; }
        __syncthreads();
        for (int r = 0; r < a.world; r++) {
            const unsigned long long lo = a.src_prefix[(int64_t)r * (a.nlocal + 1) + f];
            const unsigned long long hi = a.src_prefix[(int64_t)r * (a.nlocal + 1) + f + 1];
            for (unsigned long long i = lo + tid; i < hi; i += PA_BLOCK) {
                const uint64_t* row = a.rows + i * a.nw;
                const uint64_t key = row[0];
                int slot = -1;
                if (key == EMPTY) { slot = PA_SLOTS; lkey[slot] = 0; }
                else {
                    uint32_t h = hash_u64(key) & smask;
                    for (int probe = 0; probe < PA_SLOTS; probe++) {
                        uint64_t k = __hip_atomic_load(&lkey[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (k == key) { slot = (int)h; break; }
                        if (k == EMPTY) {
                            uint64_t expected = EMPTY;
                            if (__hip_atomic_compare_exchange_strong(&lkey[h], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_WORKGROUP)) {
                                if (atomicAdd(&s_n, 1u) >= (uint32_t)(PA_SLOTS * 9 / 10)) s_fail = 1;
                                slot = (int)h;
                                break;
                            }
                            if (expected == key) { slot = (int)h; break; }
                        }
                        h = (h + 1) & smask;
                        if ((probe & 15) == 15 && s_fail) break;
                    }
                }
                if (slot >= 0)
                    for (int w = 0; w < a.n_words; w++) l_merge(&lw[w][slot], a.merge[w], row[2 + w], PA_SLOTS + 1);
            }
        }
        __syncthreads();
        if (s_fail) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const uint32_t ngroups = s_n + (lkey[PA_SLOTS] != EMPTY ? 1u : 0u);
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 <= PA_SLOTS; i0 += PA_BLOCK) {
            int i = i0 + tid;
            bool occ = i <= PA_SLOTS && lkey[i] != EMPTY;
            uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                a.dkey[pos] = i == PA_SLOTS ? EMPTY : lkey[i];
                a.dkey[a.dstride + pos] = 0;
                for (int w = 0; w < a.n_words; w++) a.dacc[(int64_t)w * a.dstride + pos] = lw[w][i];
            }
        }
        __syncthreads();
    }
}

__global__ void fill_u64_kernel(uint64_t* p, uint64_t v, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
