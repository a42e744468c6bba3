// Dense-key partitioned aggregation (included by vnm_agg.hip inside namespace vnm).
//
// The large-G path of vnm_agg.hip partitions 16-byte (key, value) entries by HASH bits and ends in an LDS hash table
// per partition.  When the keys of a batch are DENSE in their range -- the benchmark's int64 key uniform in [0, 1e8), a
// dimension / surrogate key in general: span <= a few times the group count and < 2^29 -- the key is replaced by a
// CODE of b = ceil(log2(span)) bits,
//        code  = (key - lo)                                   (order-preserving unsigned arithmetic)
//        code' = (code * M) mod 2^b,   M odd                  (a bijection on b-bit codes: Fibonacci scrambling, so that
//                                                              sorted / clustered keys still spread over the partitions)
// and everything downstream works on code':
//   * partition = high bits of code', entry = (value, remaining low bits): 12 bytes after pass 1 (8 + 4), 10 bytes
//     after pass 2 (8 + 2) instead of 16 -- SoA regions, same private (partition, producer) regions as the hash path;
//   * the final pass needs NO hash table: inside a final partition the low 11 bits of code' are unique per key, so the
//     group's accumulators are DIRECT-ADDRESSED in LDS (2048 x {sum f64, compensation f32, count u32} = 32 KB per
//     workgroup, no keys stored, no probe chain), and the key is rebuilt from (partition, slot) with the inverse
//     multiplier when the groups are written.
// Keys outside the code range (the range comes from a SAMPLE of the first batch) and entries that overflow a region go
// to the same spill buffer the hash path uses (agg_hot_kernel<FROM_ENT> aggregates them into the HBM table).
//
// Traffic per 1e9 rows, s = 0.5, G = 1e8: 16 (rows) + 6 + 6 (level 1) + 5 + 5 (level 2) + 4 (groups) = 42 GB against
// 51.7 GB for 16-byte hash-partitioned entries.

// Direct-addressed slots per final partition: 2^11 (32 KB of LDS: four 512-thread workgroups per CU), 2^12 (two) or
// 2^13 (128 KB: one 1024-thread workgroup per CU).  More slots = fewer partitions = LONGER WRITE RUNS in the scatter
// passes (tools/copybench.hip: runs under 256 bytes cost 10-30 % of the store bandwidth), fewer resident waves in the
// final pass -- which has no dependent probe chain to hide.  The host picks (VNM_DENSE_TBITS overrides).
constexpr int DP_TBITS_MIN = 11, DP_TBITS_MAX = 13;
constexpr int DP_MAX_BITS = DP_TBITS_MAX + 18;  // two levels of at most 512 partitions each

struct DenseMap {
    uint64_t lo_u;      // order-preserving unsigned image of the key with code 0
    uint64_t sign;      // 0x8000000000000000 for int64 keys (ku = key ^ sign), 0 for uint64
    uint32_t mul;       // odd
    uint32_t mul_inv;   // mul * mul_inv == 1 mod 2^32
    uint32_t mask;      // 2^bits - 1
    int bits;
};

__device__ __forceinline__ uint64_t dense_key_of(const DenseMap& m, uint32_t codep) {
    const uint32_t code = (codep * m.mul_inv) & m.mask;
    return (m.lo_u + code) ^ m.sign;
}

struct DPartArgs {
    DenseMap map;
    // source A: raw columns (pass 1)
    const uint64_t* kp;
    const double* vp;
    const double* pp;
    int has_pred, pred_is_v, op;
    double thr;
    int64_t nrows;
    // ... or, nseg > 0, the record batches of a STREAM as one logical batch (dring_scatter_kernel only): segment i holds rows
    // [0, segs[i].nrows) of its own columns and owns the sub-tiles from segs[i].first_tile on; nrows = the total; nsub = all sub-tiles
    const VSeg* segs;
    int nseg;
    int64_t nsub;
    // a NULLABLE key column (dring_scatter_kernel<..., KN>, round 4): validity bitmap of the key (bit of row r = kvalid[(koff + r) >> 3]
    // >> ((koff + r) & 7); koff even) -- rows whose key is NULL (and that pass the predicate) are ONE group of their own
    // (single_numerical_hash_aggregate.cpp:24-32: null_group): every workgroup sums them up and adds them to the NULL slot of the
    // operator's HBM table (nk_tag: its tag word; nk_rows / nk_valid / nk_sum: its accumulator words or null, nk_lo_stride: from the sum
    // word to its compensation word, 0 = none)
    // TWO input columns (dring_scatter_kernel<..., V2>, round 4): a second value travels beside the first -- 20-byte entries after
    // pass 1, 18-byte entries after pass 2 -- through a second ring array and a second values region
    const double* vp2;
    const double* in_vals2;
    double* out_vals2;
    const uint8_t* kvalid;
    int64_t koff;
    uint64_t* nk_tag;
    uint64_t* nk_rows;
    uint64_t* nk_valid;
    uint64_t* nk_sum;
    int64_t nk_lo_stride;
    int has_expr;         // the value is `expr` evaluated per row pair instead of vp[row] (expressions inside aggregates)
    ExprProg expr;
    // source B: SoA regions written by pass 1 (values + 32-bit code remainders)
    const double* in_vals;
    const uint32_t* in_codes;
    const uint32_t* in_counts;
    int64_t in_cap;
    int in_regions, in_split;
    int64_t in_pstride, in_rstride;   // input region of (partition pin, producer rj) = pin * in_pstride + rj * in_rstride
    int nt_store;         // non-temporal stores for the runs (host: pass 1 when a wide second level follows)
    int ready_list;       // dring_scatter_kernel: the flush walks the round's list of rings that completed a block (round 6)
    int producer_major;   // pass 1 output: region of (partition p, producer b) = b * nparts + p (a producer's regions adjacent:
                          // each workgroup then writes inside ONE ~20 MB window instead of 128 windows 75 MB apart)
    int in_bits;          // bits of an incoming remainder
    // output regions: region id = out_base(blockIdx) + p * out_stride
    double* out_vals;
    void* out_codes;      // uint32_t or uint16_t remainders
    uint32_t* out_counts;
    int64_t out_cap;
    int nparts;
    int out_bits;         // remainder bits after this level
    int in_pairs;         // pass 2: input regions are read as pairs of entries (16 + 8 byte loads)
    unsigned long long* flags;  // [0] failure (spill buffer full)  [2] entries in the spill buffer  [3] keys in the NULL spill
    ulonglong2* spill;
    int64_t spill_cap;
    // nullable value column (VN kernels): validity bitmap, bit of row r = vvalid[(voff + r) >> 3] >> ((voff + r) & 7); voff even.
    // A row whose value is NULL travels as an entry with the NULL flag in the top bit of its remainder (bit 31 / bit 15: the
    // remainders themselves never reach those bits) -- it counts for COUNT(*) and makes its group exist, nothing else.
    const uint8_t* vvalid;
    int64_t voff;
    uint64_t* nspill;           // keys of NULL-value rows that could not be placed (outside the sampled range, region full)
    int64_t nspill_cap;
    // FIXED-POINT entries (dring_scatter_kernel<..., FX>, round 6): every value is m * 2^fx_qe with |m| < 2^31 (checked per row: fx_encode;
    // a row that does not fit raises flags[7] and the batch is redone with float64 entries), and an entry is ONE 64-bit word
    // (m << remainder bits) | remainder -- 8 bytes instead of 12 after pass 1 and 10 after pass 2, no separate code regions.
    double fx_q, fx_inv_q;      // 2^fx_qe, 2^-fx_qe
    int64_t fx_lim;             // |m| <= fx_lim: 2^31 - 1, or 2^18 - 1 when the words of the LAST scatter level are 32 bits (W32)
    // 32-bit words out of the FIRST of two levels: the value field is a WINDOW of fx_wbits bits, ((m - fx_wbase) << remainder bits) | remainder,
    // unsigned (fx_wuns).  Pass 1 checks every row against fx_lim at the operator's quantum first, as ever, then drops fx_sh bits the
    // sample found unused (the attempt's quantum fx_q is 2^fx_sh times the operator's) and checks the window: flags[7] bit 0 = outside
    // fx_lim or off the lattice, bit 1 = only outside the window.  fx_wbits = 0: no window (fx_wbase = fx_wuns = fx_sh = 0, signed field).
    // Pass 2 over such words (IN32) takes the window's base as fx_in_base.
    int fx_wbits, fx_wbase, fx_wuns, fx_sh, fx_in_base;
};
constexpr uint32_t DP_NULL32 = 0x80000000u;
// v == m * q exactly, |m| < 2^31, v is not -0.0 (its sign would be lost) and finite?  inv_q = 2^-qe with qe <= 0, so t = v * inv_q is
// exact and never underflows to zero; t + 1.5 * 2^52 holds an integer t in its low mantissa bits (|t| < 2^51) and rounds anything else.
__device__ __forceinline__ bool fx_encode(double v, double inv_q, int64_t* m, int64_t lim = 2147483647LL) {
    const double MAGIC = 6755399441055744.0;
    const double t = v * inv_q;
    const double u = t + MAGIC;
    const int64_t mm = (int64_t)(__double_as_longlong(u) - __double_as_longlong(MAGIC));
    *m = mm;
    return (u - MAGIC == t) && mm >= -lim && mm <= lim && __double_as_longlong(v) != (long long)0x8000000000000000ULL;
}
__device__ __forceinline__ double fx_bits(int64_t m) { return __longlong_as_double((long long)m); }        // the value slot of an entry carries m
__device__ __forceinline__ int64_t fx_of(double carried) { return (int64_t)__double_as_longlong(carried); }
// total * q as a two-term expansion: hi = the correctly rounded product (|total| < 2^62: the conversion rounds to nearest even, the
// scaling by a power of two is exact), lo = what the rounding dropped (a small integer times q: exact)
__device__ __forceinline__ void fx_expand(int64_t total, double q, double* hi, double* lo) {
    const double h = (double)total;
    const double l = (double)(total - (int64_t)h);
    *hi = h * q; *lo = l * q;
}

__device__ __forceinline__ void dense_spill(const DPartArgs& a, uint64_t key, double v, bool isnull = false) {
    if (isnull) {
        const unsigned long long pos = atomicAdd(&a.flags[3], 1ULL);
        if ((int64_t)pos < a.nspill_cap) a.nspill[pos] = key;
        else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const unsigned long long pos = atomicAdd(&a.flags[2], 1ULL);
    if ((int64_t)pos < a.spill_cap) a.spill[pos] = make_ulonglong2(key, (unsigned long long)__double_as_longlong(v));
    else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The same for the lanes of a wave at once: ONE atomic per wave and call instead of one per entry (a skewed key distribution
// spills millions of entries: k = G u^4 left 7.4e6 of 2.5e8 entries in full regions, and that many atomics on one address took
// ~45 ms).  Every lane of the wave that is active at the call site must call it (want = false: nothing to spill).
__device__ __forceinline__ void dense_spill_wave(const DPartArgs& a, bool want, uint64_t key, double v) {
    const unsigned long long m = __ballot(want);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&a.flags[2], (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (want) {
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
        if ((int64_t)pos < a.spill_cap) a.spill[pos] = make_ulonglong2(key, (unsigned long long)__double_as_longlong(v));
        else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// remainder + NULL flag as stored (CT = uint32_t: flag in bit 31, uint16_t: bit 15)
template <typename CT>
__device__ __forceinline__ CT dense_rem(uint32_t c, uint32_t remmask) {
    return (CT)((c & remmask) | ((c >> 31) << (sizeof(CT) * 8 - 1)));
}
template <typename CT>
__device__ __forceinline__ uint32_t dense_rem_code(CT r) { return (uint32_t)r & ((1u << (sizeof(CT) * 8 - 1)) - 1u); }
template <typename CT>
__device__ __forceinline__ bool dense_rem_null(CT r) { return ((uint32_t)r >> (sizeof(CT) * 8 - 1)) != 0; }

// FROM_ROWS: pass 1 (filter fused, key -> code').  CT: type of the remainders written (uint16_t when they fit 16 bits).
// HAS_VAL = false: the entries are the codes alone (COUNT(*) / DISTINCT programs: 4 and 2 bytes instead of 12 and 10).
// The value travels as raw 64-bit content -- the generic final pass (dgen_*) reads int64 / uint64 inputs out of it as well.
template <bool FROM_ROWS, typename CT, bool HAS_VAL = true, bool VN = false>
__global__ __launch_bounds__(PT_BLOCK) void dpart_scatter_kernel(DPartArgs a) {
    __shared__ double stage_v[HAS_VAL ? PT_TILE : 1];
    __shared__ uint32_t stage_c[PT_TILE];   // code' bits below this level's prefix (partition bits included)
    __shared__ uint32_t cnt[PT_MAXP], off[PT_MAXP], cursor[PT_MAXP];
    __shared__ uint32_t s_total;
    __shared__ uint32_t wtot[PT_MAXP / 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int np = a.nparts;
    const int npad = np < 64 ? 64 : np;
    const uint32_t remmask = (1u << a.out_bits) - 1u;
    for (int i = tid; i < PT_MAXP; i += PT_BLOCK) { cnt[i] = 0; cursor[i] = 0; }
    __syncthreads();

    int64_t out_base, out_stride;
    int64_t ntiles = 0;
    uint32_t prefix = 0;  // pass 2: the partition bits pass 1 stripped (for rebuilding spilled keys)
    if (FROM_ROWS) {
        if (a.producer_major) { out_base = (int64_t)blockIdx.x * np; out_stride = 1; }
        else { out_base = blockIdx.x; out_stride = gridDim.x; }
        ntiles = (a.nrows + PT_TILE - 1) / PT_TILE;
    } else {
        const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split;
        prefix = (uint32_t)pin << a.in_bits;
    }
    double* const ov = a.out_vals;
    CT* const oc = (CT*)a.out_codes;

    // get_item(k, &c, &v): item k of the current tile from registers -- c = code' below the incoming prefix
    auto process_tile = [&](auto&& get_item, auto&& prefetch_next) {
        uint32_t myc[PT_ITEMS], myr[PT_ITEMS];
        double myv[PT_ITEMS];
#pragma unroll
        for (int k = 0; k < PT_ITEMS; k++) {
            myr[k] = 0xFFFFFFFFu;
            uint32_t c; double v;
            if (get_item(k, &c, &v)) {
                myc[k] = c;
                if (HAS_VAL) myv[k] = v;
                myr[k] = atomicAdd(&cnt[(c & ~DP_NULL32) >> a.out_bits], 1u);
            }
        }
        prefetch_next();
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
        for (int k = 0; k < PT_ITEMS; k++) {
            if (myr[k] != 0xFFFFFFFFu) {
                const uint32_t pos = off[(myc[k] & ~DP_NULL32) >> a.out_bits] + myr[k];
                if (HAS_VAL) stage_v[pos] = myv[k];
                stage_c[pos] = myc[k];
            }
        }
        __syncthreads();
        const uint32_t total = s_total;
#pragma unroll
        for (int q = 0; q < PT_ITEMS; q++) {
            const uint32_t i = (uint32_t)q * PT_BLOCK + tid;
            bool lost = false;   // region full (heavy key, uneven split)
            uint32_t c = 0;
            if (i < total) {
                c = stage_c[i];
                const uint32_t p = (c & ~DP_NULL32) >> a.out_bits;
                const uint32_t j = cursor[p] + (i - off[p]);
                if (j < (uint32_t)a.out_cap) {
                    const int64_t at = (out_base + (int64_t)p * out_stride) * a.out_cap + j;
                    if (a.nt_store) {
                        if (HAS_VAL) __builtin_nontemporal_store(stage_v[i], &ov[at]);
                        __builtin_nontemporal_store(dense_rem<CT>(c, remmask), &oc[at]);
                    } else {
                        if (HAS_VAL) ov[at] = stage_v[i];
                        oc[at] = dense_rem<CT>(c, remmask);
                    }
                } else lost = true;
            }
            if (lost && (c >> 31)) { dense_spill(a, dense_key_of(a.map, prefix | (c & ~DP_NULL32)), 0.0, true); lost = false; }   // (a NULL value: its own list)
            dense_spill_wave(a, lost, dense_key_of(a.map, prefix | (c & ~DP_NULL32)), HAS_VAL && lost ? stage_v[i] : 0.0);
        }
        __syncthreads();
        if (tid < np) { cursor[tid] += cnt[tid]; cnt[tid] = 0; }
        __syncthreads();
    };

    if (FROM_ROWS) {
        ulonglong2 kk[PT_PAIRS];
        double2 vv[PT_PAIRS], pv[PT_PAIRS];
        uint8_t vb[VN ? PT_PAIRS : 1];   // the pair's two validity bits (voff and the pair's first row are even: one byte)
        auto load_rows = [&](int64_t tile) {
            const int64_t base = tile * PT_TILE;
            if (tile < ntiles && base + PT_TILE <= a.nrows) {
#pragma unroll
                for (int u = 0; u < PT_PAIRS; u++) {
                    const int64_t r = base + (int64_t)u * 2 * PT_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(a.kp + r);
                    if (HAS_VAL) vv[u] = a.has_expr ? expr_eval2(a.expr, r) : *(const double2*)(a.vp + r);
                    if (a.has_pred && !a.pred_is_v) pv[u] = *(const double2*)(a.pp + r);
                    if (VN) vb[VN ? u : 0] = (uint8_t)(a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7));
                }
            }
        };
        load_rows(blockIdx.x);
        for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const int64_t base = tile * PT_TILE;
            const bool full = base + PT_TILE <= a.nrows;
            process_tile([&](int k, uint32_t* c, double* v) -> bool {
                const int u = k >> 1, el = k & 1;
                const int64_t r = base + (int64_t)u * 2 * PT_BLOCK + 2 * tid + el;
                if (r >= a.nrows) return false;
                uint64_t key; double val, p;
                bool isnull = false;
                if (full) {
                    key = el ? kk[u].y : kk[u].x;
                    val = HAS_VAL ? (el ? vv[u].y : vv[u].x) : 0.0;
                    p = a.pred_is_v ? val : (a.has_pred ? (el ? pv[u].y : pv[u].x) : 0.0);
                    if (VN) isnull = !((vb[VN ? u : 0] >> el) & 1);
                } else {
                    key = a.kp[r]; val = HAS_VAL ? (a.has_expr ? expr_eval1(a.expr, r) : a.vp[r]) : 0.0; p = a.has_pred ? (a.pred_is_v ? val : a.pp[r]) : 0.0;
                    if (VN) isnull = !((a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7)) & 1);
                }
                if (VN && isnull && a.pred_is_v) return false;   // NULL > x is not true
                if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) return false;
                const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
                if (d > (uint64_t)a.map.mask) { dense_spill(a, key, val, isnull); return false; }  // outside the sampled range
                *c = (((uint32_t)d * a.map.mul) & a.map.mask) | (isnull ? DP_NULL32 : 0u);
                *v = isnull ? 0.0 : val;
                return true;
            }, [&]() { load_rows(tile + gridDim.x); });
        }
    } else {
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        const int pin = blockIdx.x / a.in_split;
        const int per_max = (a.in_regions + a.in_split - 1) / a.in_split;
        const int g = blockIdx.x % a.in_split;
        const int first = g * per_max;
        const int per = first + per_max <= a.in_regions ? per_max : (a.in_regions > first ? a.in_regions - first : 0);
        const int64_t region0 = (int64_t)pin * a.in_pstride + (int64_t)first * a.in_rstride;
        if (tid == 0) {
            uint32_t run = 0;
            for (int rj = 0; rj < per; rj++) { rstart[rj] = run; run += (a.in_counts[region0 + rj * a.in_rstride] + 1) / 2; }
            rstart[per] = run;
        }
        __syncthreads();
        // The concatenated input stream counts PAIRS of entries: region r holds ceil(count_r / 2) of them (the second
        // half of its last pair may be beyond the count), so that every lane issues a 16-byte + an 8-byte load per pair
        // instead of four narrow ones (8-byte accesses run at 0.54-0.70x the 16-byte rate, MI355X_MICROARCH.md).
        const uint32_t total_in = rstart[per];   // pairs
        double2 ev[PT_PAIRS];
        uint2 ec[PT_PAIRS];
        uint32_t ok[PT_PAIRS];  // bit 0 / 1: first / second entry of the pair exists
        int reg[PT_PAIRS];
#pragma unroll
        for (int k = 0; k < PT_PAIRS; k++) reg[k] = 0;
        auto load_entries = [&](uint32_t t0) {
#pragma unroll
            for (int k = 0; k < PT_PAIRS; k++) {
                const uint32_t v = t0 + (uint32_t)k * PT_BLOCK + tid;
                ok[k] = 0;
                if (v < total_in) {
                    int lo = reg[k];
                    while (rstart[lo + 1] <= v) lo++;
                    reg[k] = lo;
                    const uint32_t e0 = 2u * (v - rstart[lo]);
                    const int64_t rg = region0 + lo * a.in_rstride;
                    const int64_t at = rg * a.in_cap + e0;
                    if (HAS_VAL) ev[k] = *(const double2*)(a.in_vals + at);
                    ec[k] = *(const uint2*)(a.in_codes + at);
                    ok[k] = e0 + 1 < a.in_counts[rg] ? 3u : 1u;
                }
            }
        };
        load_entries(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += PT_TILE / 2) {
            process_tile([&](int k, uint32_t* c, double* v) -> bool {
                const int u = k >> 1, el = k & 1;
                if (!((ok[u] >> el) & 1u)) return false;
                *c = el ? ec[u].y : ec[u].x;
                *v = HAS_VAL ? (el ? ev[u].y : ev[u].x) : 0.0;
                return true;
            }, [&]() { load_entries(t0 + PT_TILE / 2); });
        }
    }
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid] < (uint32_t)a.out_cap ? cursor[tid] : (uint32_t)a.out_cap;
}

// ---- scatter with per-partition ring buffers in LDS (round 3) ------------------------------------------------------------
// dpart_scatter_kernel sorts a tile by partition in LDS and writes every partition's run behind the previous tile's run:
// the runs (~32 entries) start and end in the middle of cache lines, and whether the L2 still holds the first half of a
// line when the next tile completes it ~10 us later -- 32 workgroups per XCD stream 4 MB of rows through a 4 MB L2 in
// between -- decides between a merged line and a partial write-back + a second, read-modify-write one (PMC, round 2:
// 9.8 GB written for 6.0 GB of entries and 4.7 GB of extra fetches in the "slow state", which follows where the regions
// land in HBM: pass 1 at 6.0-6.4 ms instead of 4.97).
// Here a workgroup keeps a RING of `ring_cap` entries per partition in LDS.  Rows are inserted straight into their
// partition's ring (one LDS atomic hands out the position -- no sort, no prefix scan) and only WHOLE BLOCKS of
// DR_FB = 16 entries ever leave it: 128 bytes of values = one full, aligned cache line; 64 (uint32) / 32 (uint16) bytes
// of codes = full aligned sectors.  Every sector of a region is written exactly once, completely, whatever the L2 does
// in between -- the traffic no longer depends on placement.  Region layout and counts are what the plain kernel writes
// (SoA values + codes, regions private to a (partition, producer) pair), so the readers are unchanged.
// A ring that cannot take an entry (more than ring_cap - 15 new entries of one partition in one sub-tile: skew) leaves
// it pending in its thread's registers for another insert / flush round of the same sub-tile; a full REGION spills
// whole blocks as before.
// ---- exact-add statistics (round 6) -------------------------------------------------------------------------------------------
// The final pass keeps every float sum as a compensated (hi, lo) pair: a returning LDS atomic, TwoSum, a second atomic -- a dependent
// chain per entry.  When every add is EXACT the lo words stay zero and the chain is not needed.  A sufficient condition that the
// scatter passes can check while they hold the values anyway: every value v != 0 that reaches the final pass is finite, its lowest
// set bit has weight >= q = 2^(L - 1075) and |v| < 2^(E - 1022); then every partial sum of at most R of them, in any order, is a
// multiple of q of magnitude < R 2^(E - 1022), hence exactly representable when  ceil(log2 R) + E <= L  (53 bits above q).
// L = (biased exponent, 1 for subnormals) + (trailing zeros of the 53-bit significand), E = biased exponent (2047 for Inf / NaN: the
// test then fails).  Pass 1 tracks max(0xFFFF - L) and max(E) per thread and leaves their maxima in flags[6] (low / high half).
__device__ __forceinline__ void exact_track(double v, uint32_t& xinv, uint32_t& xexp) {
    const uint64_t b = (uint64_t)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFULL;
    if (b == 0) return;
    const uint32_t hi = (uint32_t)(b >> 32), lo = (uint32_t)b;
    const uint32_t e = hi >> 20;
    const uint32_t mh = (hi & 0xFFFFFu) | (e ? 0x100000u : 0u);
    const uint32_t tz = lo ? (uint32_t)__builtin_ctz(lo) : 32u + (uint32_t)__builtin_ctz(mh);
    const uint32_t low = (e ? e : 1u) + tz;
    xinv = max(xinv, 0xFFFFu - low);
    xexp = max(xexp, e);
}
// host side: are all adds of `rows` such values exact?  (word = flags[6] as the kernel left it)
static inline bool exact_adds_proved(unsigned long long word, int64_t rows) {
    const uint32_t xinv = (uint32_t)word, xexp = (uint32_t)(word >> 32);
    if (xinv == 0 && xexp == 0) return true;          // no value other than zeros
    if (xexp >= 2047) return false;                   // Inf / NaN
    int lg = 0;
    while (((int64_t)1 << lg) < rows) lg++;
    return (int64_t)lg + (int64_t)xexp <= (int64_t)(0xFFFFu - xinv);
}

constexpr int DR_FB = 16;          // entries per flushed block
// DR_BLOCK threads per workgroup, DR_PAIRS pairs of rows (or entries) per lane and sub-tile.  Every use of a loaded register
// waits for ALL outstanding memory operations of the wave (the flush phase issues a data-dependent number of stores, so the
// compiler cannot count past them: s_waitcnt vmcnt(0)); what is in flight per CU is therefore ONE sub-tile, loaded right after
// the previous one was consumed.  2048-row sub-tiles (32 KB per CU in flight) ran pass 1 at 6.6 ms; smaller workgroups made it
// worse (the flush phase walks every partition whatever the sub-tile size: 512 threads 7.1 ms, 256 threads 14-18 ms).
typedef double dr_v2 __attribute__((ext_vector_type(2)));
typedef uint32_t dr_u2 __attribute__((ext_vector_type(2)));
// PV: pass 1 with a predicate column of its own (three loads per pair of rows instead of two: its registers are only there then)
// VN: pass 1 over a nullable value column (one validity byte per pair of rows; NULL rows travel with the NULL flag, see DPartArgs)
// MAXR = 2: a sub-tile gets two insert / flush rounds, then what is still pending is spilled (skew; see `rounds`); 0 = as many
// rounds as it takes.  The host sets 2 where an even spread of a sub-tile's entries fits ONE round (and sizes the sub-tile for
// that).  A compile-time number: the same test at run time, or three rounds, cost pass 1 a third of its speed (4.1 -> 5.4 ms:
// 74 registers spilled to scratch; with 2 the 4-pair kernel needs 122 and spills none).
// SEG: pass 1 over the waiting batches of a stream (a.segs), see VSeg -- the one-batch kernels keep their registers
// KN: pass 1 over a NULLABLE key column (see DPartArgs::kvalid)
// V2: entries carry TWO values (see DPartArgs::vp2); nothing spills in that mode -- an entry without a place fails the pass (flags[0])
// and the batch takes the hash partitions
// FX: fixed-point entries -- ONE 64-bit word per entry, (m << remainder bits) | remainder, in the rings and in the regions (DPartArgs::fx_q)
// The ring protocol below (fill / head / cursor, insert, flush, rounds) is this kernel's OWN COPY of what vnm_ring.inc holds for the four
// other ring scatters; only the level-2 region walk comes from there.  The four-pair pass-1 instances sit at 127-128 VGPRs: built on the
// core's reserve / flush / rounds they spilled 62-99 registers and the one-pair instances lost an occupancy step, and the core's
// bookkeeping alone (one ready list, ring_init) still left five of them with 12 spilled registers (profiles/r12_ring_core.txt, section 2).
// A change to the protocol is made there AND here.
template <bool FROM_ROWS, typename CT, bool HAS_VAL, int DR_BLOCK, int DR_PAIRS, bool PV = false, bool VN = false, int MAXR = 0, bool SEG = false, bool KN = false,
          bool V2 = false, bool FX = false, bool W32 = false, bool IN32 = false, bool WIN = false>
__global__ __launch_bounds__(DR_BLOCK) void dring_scatter_kernel(DPartArgs a, int ring_cap) {
    extern __shared__ uint64_t dr_lds[];
    static_assert(!FX || (HAS_VAL && !V2), "fixed-point entries: one value (VN: only where the filter drops the NULL rows, vn_fold)");
    static_assert(!W32 || FX, "32-bit entry words are fixed-point words");
    // IN32: the words this pass READS are 32 bits, the first level's window words (DPartArgs::fx_wbits) -- 16 bytes per load all the same
    static_assert(!IN32 || (W32 && !FROM_ROWS), "32-bit input words: the second of two levels of 32-bit fixed-point words");
    // WIN: the 32-bit words this pass WRITES are the first level's window words (DPartArgs::fx_wbits; base and signedness are arguments) -- a
    // compile-time switch so that the one-level kernels, whose words have no window, keep the code they had
    static_assert(!WIN || (W32 && FROM_ROWS), "window words: 32-bit words out of the first of two levels");
    // W32: the words this pass WRITES are 32 bits -- (m << remainder bits) | remainder with m of at most 32 - remainder bits (the host
    // checks the sampled magnitude, pass 1 every row: DPartArgs::fx_lim) -- in blocks of 32 (128 bytes), four per lane
    constexpr int FB = W32 ? 32 : DR_FB, EPL = FB / 8;
    constexpr int NE = 2 * DR_PAIRS;   // entries per lane and sub-tile
    const int np = a.nparts;
    double* const rv = (double*)dr_lds;                                        // [np][ring_cap]   (HAS_VAL; FX: the entry words)
    double* const rv2 = rv + (V2 ? (size_t)np * ring_cap : 0);                 // [np][ring_cap]   (V2)
    CT* const rc = (CT*)(dr_lds + (HAS_VAL ? (size_t)np * ring_cap * (V2 ? 2 : 1) : 0));        // [np][ring_cap]   (not FX)
    __shared__ uint32_t fill[PT_MAXP], head[PT_MAXP], cursor[PT_MAXP];
    __shared__ uint32_t s_retry[2];
    __shared__ uint32_t s_nready[2];            // rings that completed a block in this round (phase ph), and which: every ring starts a round
    __shared__ uint16_t ready[2][PT_MAXP];      // with less than one block (the flush takes all whole blocks), so it completes its first block of the
                                                // round exactly once -- the lane whose entry is that block's last lists the ring, and the flush walks
                                                // the list instead of asking every ring for its fill (the sort's scatters: 4.5 -> 3.9 ms, round 6)
    __shared__ uint32_t s_spill[3];   // entries a sub-tile spills when its rounds are used up (see rounds); the workgroup's reservation (lo, hi)
    const int tid = threadIdx.x;
    const uint32_t remmask = (1u << a.out_bits) - 1u;
    for (int i = tid; i < PT_MAXP; i += DR_BLOCK) { fill[i] = 0; head[i] = 0; cursor[i] = 0; }
    if (tid < 2) { s_retry[tid] = 0; s_nready[tid] = 0; }
    int ph = 0;
    const bool use_list = a.ready_list != 0;
    if (tid == 0) s_spill[0] = 0;
    __syncthreads();

    int64_t out_base, out_stride;
    uint32_t prefix = 0;
    if (FROM_ROWS) {
        if (a.producer_major) { out_base = (int64_t)blockIdx.x * np; out_stride = 1; }
        else { out_base = blockIdx.x; out_stride = gridDim.x; }
    } else {
        const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split;
        prefix = (uint32_t)pin << a.in_bits;
    }
    double* const ov = a.out_vals;
    double* const ov2 = a.out_vals2;
    CT* const oc = (CT*)a.out_codes;
    const uint32_t ocap = (uint32_t)a.out_cap;

    // one entry into its ring; false = the ring is full (the entry stays pending)
    auto insert = [&](uint32_t c, double v, double w2) -> bool {
        const uint32_t p = (c & ~DP_NULL32) >> a.out_bits;
        const uint32_t r = atomicAdd(&fill[p], 1u);
        if (r == (uint32_t)FB - 1u && use_list) ready[ph][atomicAdd(&s_nready[ph], 1u)] = (uint16_t)p;
        if (r >= (uint32_t)ring_cap) return false;
        uint32_t slot = head[p] + r;
        if (slot >= (uint32_t)ring_cap) slot -= ring_cap;
        if (W32) {
            ((uint32_t*)rv)[(size_t)p * ring_cap + slot] = ((uint32_t)((int32_t)fx_of(v) - (WIN ? a.fx_wbase : 0)) << a.out_bits) | (c & remmask);
            return true;
        }
        if (FX) {
            ((uint64_t*)rv)[(size_t)p * ring_cap + slot] = ((uint64_t)fx_of(v) << a.out_bits) | (uint64_t)(c & remmask);
            return true;
        }
        if (HAS_VAL) rv[(size_t)p * ring_cap + slot] = v;
        if (V2) rv2[(size_t)p * ring_cap + slot] = w2;
        rc[(size_t)p * ring_cap + slot] = dense_rem<CT>(c, remmask);
        return true;
    };
    // (FX) remainder and value of the entry word at ring index li
    auto fx_rem = [&](size_t li) -> uint32_t { return W32 ? ((const uint32_t*)rv)[li] & remmask : (uint32_t)(((const uint64_t*)rv)[li] & (uint64_t)remmask); };
    auto fx_val = [&](size_t li) -> double {
        if (W32) {   // (a signed field, or the first level's window: unsigned, above its base)
            const uint32_t w = ((const uint32_t*)rv)[li];
            if (WIN) return (double)((a.fx_wuns ? (int32_t)(w >> a.out_bits) : (int32_t)w >> a.out_bits) + a.fx_wbase) * a.fx_q;
            return (double)((int32_t)w >> a.out_bits) * a.fx_q;
        }
        return (double)((int64_t)((const uint64_t*)rv)[li] >> a.out_bits) * a.fx_q;
    };
    // whole blocks of every ring -> the partition's region.  Eight lanes per partition: lane j moves entries 2j, 2j + 1 of a block
    // (16 bytes of values, 8 / 4 bytes of codes).  `drain`: the last, partial block as well (end of the kernel).
    auto flush = [&](bool drain) {
        const int j = tid & 7;
        const bool listed = use_list && !drain;
        const int nwalk = listed ? (int)s_nready[ph] : np;
        for (int q = tid >> 3; q < nwalk; q += DR_BLOCK / 8) {
            const int p = listed ? (int)ready[ph][q] : q;
            uint32_t f = fill[p];
            if (f > (uint32_t)ring_cap) f = ring_cap;
            const uint32_t nb = drain ? (f + FB - 1) / FB : f / FB;
            if (nb == 0) continue;
            const uint32_t h = head[p], cur = cursor[p];
            const int64_t rbase = (out_base + (int64_t)p * out_stride) * a.out_cap;
            uint32_t done = 0, wrote = 0;
            for (uint32_t b = 0; b < nb; b++) {
                uint32_t src = h + b * FB;
                if (src >= (uint32_t)ring_cap) src -= ring_cap;
                const uint32_t n_here = f - b * FB < (uint32_t)FB ? f - b * FB : FB;   // < FB only when draining
                const size_t li = (size_t)p * ring_cap + src + EPL * j;
                if (cur + wrote + FB <= ocap) {
                    const int64_t at = rbase + cur + wrote + EPL * j;
                    if ((uint32_t)(EPL * j) < n_here) {
                        if (W32) {
                            const dr_v2 x = *(const dr_v2*)((const uint32_t*)rv + li);          // four 32-bit words
                            if (a.nt_store) __builtin_nontemporal_store(x, (dr_v2*)((uint32_t*)ov + at)); else *(dr_v2*)((uint32_t*)ov + at) = x;
                        } else if (HAS_VAL) {
                            const dr_v2 x = *(const dr_v2*)(rv + li);
                            if (a.nt_store) __builtin_nontemporal_store(x, (dr_v2*)(ov + at)); else *(dr_v2*)(ov + at) = x;
                        }
                        if (V2) {
                            const dr_v2 x2 = *(const dr_v2*)(rv2 + li);
                            if (a.nt_store) __builtin_nontemporal_store(x2, (dr_v2*)(ov2 + at)); else *(dr_v2*)(ov2 + at) = x2;
                        }
                        if (FX) {
                        } else if (sizeof(CT) == 4) {
                            const dr_u2 y = *(const dr_u2*)(rc + li);
                            if (a.nt_store) __builtin_nontemporal_store(y, (dr_u2*)(oc + at)); else *(dr_u2*)(oc + at) = y;
                        } else {
                            const uint32_t y = *(const uint32_t*)(rc + li);
                            if (a.nt_store) __builtin_nontemporal_store(y, (uint32_t*)(oc + at)); else *(uint32_t*)(oc + at) = y;
                        }
                    }
                    wrote += n_here;
                } else if (V2) {   // (two-value entries have no spill buffer: the pass fails, the batch takes the hash partitions)
                    if (j == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (!drain && a.nspill == nullptr) {
                    // region full (heavy keys, a skewed distribution, an uneven split): the block goes to the spill buffer.  All
                    // lanes of the wave that are in this iteration hold whole blocks of FB entries (eight lanes each): ONE
                    // reservation for all of them.
                    const unsigned long long m = __ballot(j == 0);
                    const int lane = tid & 63;
                    const int leader = __ffsll((long long)m) - 1;
                    unsigned long long base = 0;
                    if (lane == leader) base = atomicAdd(&a.flags[2], (unsigned long long)__popcll(m) * FB);
                    base = __shfl(base, leader);
                    const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ULL << (lane - j)) - 1ULL)) * FB + EPL * j;
                    if ((int64_t)(pos + EPL) <= a.spill_cap) {
                        for (int e = 0; e < EPL; e++)
                            a.spill[pos + e] = make_ulonglong2(dense_key_of(a.map, prefix | (p << a.out_bits) | (FX ? fx_rem(li + e) : dense_rem_code<CT>(rc[FX ? 0 : li + e]))),
                                                               (unsigned long long)__double_as_longlong(FX ? fx_val(li + e) : (HAS_VAL ? rv[li + e] : 0.0)));
                    } else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {   // ... entry by entry at the end of the kernel (partial blocks) and with NULL flags (two lists)
                    for (int e = 0; e < EPL; e++)
                        if ((uint32_t)(EPL * j + e) < n_here) {
                            if (FX) dense_spill(a, dense_key_of(a.map, prefix | (p << a.out_bits) | fx_rem(li + e)), fx_val(li + e));
                            else dense_spill(a, dense_key_of(a.map, prefix | (p << a.out_bits) | dense_rem_code<CT>(rc[FX ? 0 : li + e])), HAS_VAL ? rv[li + e] : 0.0,
                                             dense_rem_null<CT>(rc[FX ? 0 : li + e]));
                        }
                }
                done += n_here;
            }
            if (j == 0) {
                uint32_t nh = h + nb * FB;
                while (nh >= (uint32_t)ring_cap) nh -= ring_cap;
                head[p] = drain ? 0 : nh;
                fill[p] = f - done;
                cursor[p] = cur + wrote;
            }
        }
    };
    // one sub-tile: insert, flush, and as many more rounds as entries are left pending (more than ring_cap - 15 new entries of
    // one partition: every row surviving the predicate, skew).  Round k raises s_retry[k & 1]; the flag of round k + 1 is cleared
    // between the two barriers of round k, when nobody reads or raises it.
    int maxr = MAXR;
    auto rounds = [&](const uint32_t (&c)[NE], const double (&v)[NE], const double (&w2)[V2 ? NE : 1], uint32_t okmask) {
        uint32_t pend = 0;
        int nr = 0;
#pragma unroll
        for (int e = 0; e < NE; e++) if (((okmask >> e) & 1u) && !insert(c[e], v[e], w2[V2 ? e : 0])) pend |= 1u << e;
        for (;;) {
            if (pend) s_retry[ph] = 1;
            __syncthreads();
            flush(false);
            if (tid == 0) { s_retry[ph ^ 1] = 0; s_nready[ph ^ 1] = 0; }
            __syncthreads();
            const bool again = s_retry[ph] != 0;
            ph ^= 1;
            if (!again) break;
            if (MAXR > 0 && ++nr >= maxr) {
                // Skew: a key that holds a few per cent of the rows sends hundreds of a sub-tile's entries to ONE ring of ring_cap
                // slots -- dozens of rounds, each two barriers and a walk over every partition (k = G u^4, G = 1e7: pass 2 at 33 ms
                // instead of 1.3).  What is still pending after two rounds goes to the spill buffer -- ONE reservation per workgroup (one per
                // wave and entry slot: 7.8e6 atomics on one address, pass 1 at 60 ms for k = G u^8) -- and the scan over the
                // spilled entries pre-aggregates such keys in LDS.
                uint32_t mine = 0;
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    if (((pend >> e) & 1u) && (c[e] >> 31)) {   // (a NULL value: the list of its own, entry by entry)
                        dense_spill(a, dense_key_of(a.map, prefix | (c[e] & ~DP_NULL32)), 0.0, true);
                        pend &= ~(1u << e);
                    }
                }
                mine = (uint32_t)__popc(pend);
                uint32_t at = mine ? atomicAdd(&s_spill[0], mine) : 0u;
                __syncthreads();
                if (tid == 0) {
                    const unsigned long long base = atomicAdd(&a.flags[2], (unsigned long long)s_spill[0]);
                    s_spill[1] = (uint32_t)base; s_spill[2] = (uint32_t)(base >> 32);
                }
                __syncthreads();
                const unsigned long long base = ((unsigned long long)s_spill[2] << 32) | s_spill[1];
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    if ((pend >> e) & 1u) {
                        const unsigned long long pos = base + at++;
                        if ((int64_t)pos < a.spill_cap)
                            a.spill[pos] = make_ulonglong2(dense_key_of(a.map, prefix | c[e]),
                                                           (unsigned long long)__double_as_longlong(FX ? (double)fx_of(v[e]) * a.fx_q : (HAS_VAL ? v[e] : 0.0)));
                        else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                __syncthreads();
                if (tid == 0) s_spill[0] = 0;   // (read again only after the barriers of the next sub-tile's first round)
                maxr = MAXR - 1;   // skew persists: from now on this workgroup spills what an even spread's rounds leave pending
                break;
            }
#pragma unroll
            for (int e = 0; e < NE; e++) if (((pend >> e) & 1u) && insert(c[e], v[e], w2[V2 ? e : 0])) pend &= ~(1u << e);
        }
    };

    double nk_hi = -0.0, nk_lo = 0.0;   // KN: this thread's share of the NULL-key group (sum as a TwoSum pair, rows)
    uint32_t nk_cnt = 0;
    constexpr bool XT = FROM_ROWS && HAS_VAL && !V2 && !FX;   // exact-add statistics of the values that become entries (exact_track)
    uint32_t xinv = 0, xexp = 0;
    uint32_t fx_bad = 0;   // FX: a value of this thread's rows is not m * q with |m| <= fx_lim (bit 0), or only outside the first level's window (bit 1): flags[7]
    // (FX) the value as the entry carries it: m in quanta of fx_q; false = the row does not fit (the attempt fails: fx_bad)
    auto fx_entry = [&](double val, double* out) -> bool {
        int64_t m;
        if (!fx_encode(val, a.fx_inv_q, &m, a.fx_lim)) { fx_bad |= 1u; return false; }
        if (WIN) {
            const int64_t m1 = m >> a.fx_sh;
            if ((m1 << a.fx_sh) != m || (uint64_t)(m1 - (int64_t)a.fx_wbase) >> a.fx_wbits) { fx_bad |= 2u; return false; }
            m = m1;
        }
        *out = fx_bits(m);
        return true;
    };
    if (FROM_ROWS && !SEG) {
        const int64_t sub = (int64_t)NE * DR_BLOCK;
        const int64_t nsub = (a.nrows + sub - 1) / sub;
        const int64_t nfull = a.nrows / sub;
        ulonglong2 kk[DR_PAIRS];
        double2 vv[DR_PAIRS], pv[PV ? DR_PAIRS : 1], vv2[V2 ? DR_PAIRS : 1];
        uint32_t vbits = 0;   // VN: two validity bits per pair (voff and a pair's first row are even: both sit in one byte)
        uint32_t kbits = 0;   // KN: the same for the key column
        auto load_sub = [&](int64_t st) {
            if (st < nfull) {
                if (VN) vbits = 0;
                if (KN) kbits = 0;
#pragma unroll
                for (int u = 0; u < DR_PAIRS; u++) {
                    const int64_t r = st * sub + (int64_t)u * 2 * DR_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(a.kp + r);
                    if (HAS_VAL) vv[u] = *(const double2*)(a.vp + r);   // (expressions inside aggregates keep dpart_scatter_kernel)
                    if (V2) vv2[V2 ? u : 0] = *(const double2*)(a.vp2 + r);
                    if (PV) pv[u] = *(const double2*)(a.pp + r);
                    if (VN) vbits |= (((uint32_t)a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7)) & 3u) << (2 * u);
                    if (KN) kbits |= (((uint32_t)a.kvalid[(a.koff + r) >> 3] >> ((a.koff + r) & 7)) & 3u) << (2 * u);
                }
            }
        };
        load_sub(blockIdx.x);
        for (int64_t st = blockIdx.x; st < nsub; st += gridDim.x) {
            uint32_t c[NE]; double v[NE]; double w2[V2 ? NE : 1]; uint32_t okmask = 0;
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const int u = e >> 1, el = e & 1;
                const int64_t r = st * sub + (int64_t)u * 2 * DR_BLOCK + 2 * tid + el;
                c[e] = 0; v[e] = 0.0;
                if (r >= a.nrows) continue;
                uint64_t key; double val, p, val2 = 0.0;
                bool isnull = false, keynull = false;
                if (st < nfull) {
                    if (KN) keynull = !((kbits >> e) & 1u);
                    key = el ? kk[u].y : kk[u].x;
                    val = HAS_VAL ? (el ? vv[u].y : vv[u].x) : 0.0;
                    if (V2) val2 = el ? vv2[V2 ? u : 0].y : vv2[V2 ? u : 0].x;
                    p = PV ? (el ? pv[PV ? u : 0].y : pv[PV ? u : 0].x) : val;
                    if (VN) isnull = !((vbits >> e) & 1u);
                } else {
                    key = a.kp[r]; val = HAS_VAL ? a.vp[r] : 0.0; p = a.has_pred ? (a.pred_is_v ? val : a.pp[r]) : 0.0;
                    if (V2) val2 = a.vp2[r];
                    if (VN) isnull = !((a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7)) & 1);
                    if (KN) keynull = !((a.kvalid[(a.koff + r) >> 3] >> ((a.koff + r) & 7)) & 1);
                }
                if (VN && isnull && a.pred_is_v) continue;   // NULL > x is not true
                if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) continue;
                if (KN && keynull) {   // the NULL-key group: summed up here, added to the table's NULL slot at the end of the kernel
                    nk_cnt++;
                    const double t = nk_hi + val;
                    nk_lo += two_sum_err(nk_hi, val, t);
                    nk_hi = t;
                    continue;
                }
                const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
                if (d > (uint64_t)a.map.mask) {   // outside the sampled range (rare: it comes from a sample)
                    if (V2) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (no spill buffer for two-value entries)
                    else dense_spill(a, key, val, isnull);
                    continue;
                }
                c[e] = (((uint32_t)d * a.map.mul) & a.map.mask) | (VN && isnull ? DP_NULL32 : 0u);
                v[e] = VN && isnull ? 0.0 : val;
                if (FX && !fx_entry(val, &v[e])) continue;
                if (V2) w2[V2 ? e : 0] = val2;
                if (XT) exact_track(v[e], xinv, xexp);
                okmask |= 1u << e;
            }
            load_sub(st + gridDim.x);   // the registers are free: the workgroup's next sub-tile is in flight during the rounds below
            rounds(c, v, w2, okmask);
        }
    } else if (FROM_ROWS) {   // SEG: the record batches of a stream as the segments of one logical batch
        const int64_t sub = (int64_t)NE * DR_BLOCK;
        // The rows of sub-tile st: a (segment, local sub-tile) pair -- one record batch of a stream per segment.  Sub-tiles never span segments; a segment's last one is partial.  Everything here is uniform
        // over the workgroup (scalar registers); the segment cursor only moves forward.
        struct Cur { const uint64_t* kp; const double* vp; const double* pp; const uint8_t* vvalid; int64_t voff; int64_t nrows; int64_t lst; };
        const int nseg = a.nseg;
        const VSegConst segs = seg_table(a.segs);
        const int64_t nsub = a.nsub;
        int sg = 0;
        auto locate = [&](int64_t st, Cur& c) {
            while (sg + 1 < nseg && st >= segs[sg + 1].first_tile) sg++;      // (scalar loads: see seg_table)
            c.kp = segs[sg].kp; c.vp = (const double*)segs[sg].vp; c.pp = segs[sg].pp;
            c.vvalid = VN ? segs[sg].vvalid : nullptr; c.voff = VN ? segs[sg].voff : 0;
            c.nrows = segs[sg].nrows;
            c.lst = st - segs[sg].first_tile;
        };
        ulonglong2 kk[DR_PAIRS];
        double2 vv[DR_PAIRS], pv[PV ? DR_PAIRS : 1];
        uint32_t vbits = 0;   // VN: two validity bits per pair (voff and a pair's first row are even: both sit in one byte)
        auto load_sub = [&](const Cur& c) {
            if (c.lst < c.nrows / sub) {
                if (VN) vbits = 0;
#pragma unroll
                for (int u = 0; u < DR_PAIRS; u++) {
                    const int64_t r = c.lst * sub + (int64_t)u * 2 * DR_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(c.kp + r);
                    if (HAS_VAL) vv[u] = *(const double2*)(c.vp + r);   // (expressions inside aggregates keep dpart_scatter_kernel)
                    if (PV) pv[u] = *(const double2*)(c.pp + r);
                    if (VN) vbits |= (((uint32_t)c.vvalid[(c.voff + r) >> 3] >> ((c.voff + r) & 7)) & 3u) << (2 * u);
                }
            }
        };
        Cur cur{}, nxt{};
        if ((int64_t)blockIdx.x < nsub) { locate(blockIdx.x, cur); load_sub(cur); }
        for (int64_t st = blockIdx.x; st < nsub; st += gridDim.x) {
            uint32_t c[NE]; double v[NE]; uint32_t okmask = 0;
            const bool full = cur.lst < cur.nrows / sub;
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const int u = e >> 1, el = e & 1;
                const int64_t r = cur.lst * sub + (int64_t)u * 2 * DR_BLOCK + 2 * tid + el;
                c[e] = 0; v[e] = 0.0;
                if (r >= cur.nrows) continue;
                uint64_t key; double val, p;
                bool isnull = false;
                if (full) {
                    key = el ? kk[u].y : kk[u].x;
                    val = HAS_VAL ? (el ? vv[u].y : vv[u].x) : 0.0;
                    p = PV ? (el ? pv[PV ? u : 0].y : pv[PV ? u : 0].x) : val;
                    if (VN) isnull = !((vbits >> e) & 1u);
                } else {
                    key = cur.kp[r]; val = HAS_VAL ? cur.vp[r] : 0.0; p = a.has_pred ? (a.pred_is_v ? val : cur.pp[r]) : 0.0;
                    if (VN) isnull = !((cur.vvalid[(cur.voff + r) >> 3] >> ((cur.voff + r) & 7)) & 1);
                }
                if (VN && isnull && a.pred_is_v) continue;   // NULL > x is not true
                if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) continue;
                const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
                if (d > (uint64_t)a.map.mask) { dense_spill(a, key, val, isnull); continue; }  // outside the sampled range (rare: it comes from a sample)
                c[e] = (((uint32_t)d * a.map.mul) & a.map.mask) | (VN && isnull ? DP_NULL32 : 0u);
                v[e] = VN && isnull ? 0.0 : val;
                if (FX && !fx_entry(val, &v[e])) continue;
                if (XT) exact_track(v[e], xinv, xexp);
                okmask |= 1u << e;
            }
            // the registers are free: the workgroup's next sub-tile is in flight during the rounds below
            if (st + gridDim.x < nsub) { locate(st + gridDim.x, nxt); load_sub(nxt); }
            const double w2[V2 ? NE : 1] = {};      // (stream segments carry one value)
            rounds(c, v, w2, okmask);
            cur = nxt;
        }
    } else {
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        // the concatenated input stream counts load UNITS: pairs of entries (16 + 8 byte loads), as in dpart_scatter_kernel -- or, IN32,
        // 16 bytes of 32-bit words: four entries (two for the one-pair sub-tile).  Counts and region cursors are in entries either way.
        constexpr int IU = IN32 ? (DR_PAIRS >= 2 ? 4 : 2) : 2, NU = NE / IU;
        const RingRegions rgs = ring_regions<IU>(rstart, a.in_counts, a.in_regions, a.in_split, a.in_pstride, a.in_rstride);
        const uint32_t total_in = rgs.total;
        double2 ev[IN32 ? 1 : DR_PAIRS], ev2[V2 ? DR_PAIRS : 1];
        uint2 ec[IN32 ? 1 : DR_PAIRS];
        uint32_t ew[IN32 ? NE : 1];   // IN32: the words of this lane's units
        uint32_t okm = 0;
        int reg = 0;   // units are visited in ascending order: the region cursor only moves forward
        auto load_pairs = [&](uint32_t t0) {
            okm = 0;
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const uint32_t v = t0 + (uint32_t)u * DR_BLOCK + tid;
                if (v < total_in) {
                    uint32_t e0;
                    const int64_t rg = rgs.region0 + ring_region_of<IU>(rstart, reg, v, &e0) * a.in_rstride;
                    const int64_t at = rg * a.in_cap + e0;
                    if (IN32) {   // (in_cap is a multiple of 32 words and e0 of IU: aligned, and inside the region whatever its count)
                        const uint32_t* src = (const uint32_t*)a.in_vals + at;
                        if (IU == 4) { const uint4 x = *(const uint4*)src; ew[IN32 ? 4 * u : 0] = x.x; ew[IN32 ? 4 * u + 1 : 0] = x.y; ew[IN32 ? 4 * u + 2 : 0] = x.z; ew[IN32 ? 4 * u + 3 : 0] = x.w; }
                        else { const uint2 x = *(const uint2*)src; ew[IN32 ? 2 * u : 0] = x.x; ew[IN32 ? 2 * u + 1 : 0] = x.y; }
                        const uint32_t left = a.in_counts[rg] - e0;   // >= 1
                        okm |= (left >= (uint32_t)IU ? (1u << IU) - 1u : (1u << left) - 1u) << (IU * u);
                        continue;
                    }
                    if (HAS_VAL) ev[IN32 ? 0 : u] = *(const double2*)(a.in_vals + at);
                    if (V2) ev2[V2 ? u : 0] = *(const double2*)(a.in_vals2 + at);
                    if (!FX) ec[IN32 ? 0 : u] = *(const uint2*)(a.in_codes + at);
                    okm |= (e0 + 1 < a.in_counts[rg] ? 3u : 1u) << (2 * u);
                }
            }
        };
        load_pairs(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += NU * DR_BLOCK) {
            uint32_t c[NE]; double v[NE]; double w2[V2 ? NE : 1];
            if (IN32) {   // window word = ((m - fx_in_base) << in_bits) | remainder of in_bits bits, the field unsigned
                const uint32_t inmask = (1u << a.in_bits) - 1u;
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    const uint32_t w = ew[IN32 ? e : 0];
                    c[e] = w & inmask;
                    v[e] = fx_bits((int64_t)((int32_t)(w >> a.in_bits) + a.fx_in_base));
                }
            } else {
#pragma unroll
                for (int u = 0; u < DR_PAIRS; u++) {
                    if (FX) {   // entry word = (m << in_bits) | remainder of in_bits bits
                        const uint64_t w0 = (uint64_t)__double_as_longlong(ev[IN32 ? 0 : u].x), w1 = (uint64_t)__double_as_longlong(ev[IN32 ? 0 : u].y);
                        const uint64_t inmask = ((uint64_t)1 << a.in_bits) - 1;
                        c[2 * u] = (uint32_t)(w0 & inmask); c[2 * u + 1] = (uint32_t)(w1 & inmask);
                        v[2 * u] = fx_bits((int64_t)w0 >> a.in_bits); v[2 * u + 1] = fx_bits((int64_t)w1 >> a.in_bits);
                        continue;
                    }
                    c[2 * u] = ec[IN32 ? 0 : u].x; c[2 * u + 1] = ec[IN32 ? 0 : u].y;
                    v[2 * u] = HAS_VAL ? ev[IN32 ? 0 : u].x : 0.0; v[2 * u + 1] = HAS_VAL ? ev[IN32 ? 0 : u].y : 0.0;
                    if (V2) { w2[V2 ? 2 * u : 0] = ev2[V2 ? u : 0].x; w2[V2 ? 2 * u + 1 : 0] = ev2[V2 ? u : 0].y; }
                }
            }
            const uint32_t okmask = okm;
            load_pairs(t0 + NU * DR_BLOCK);
            rounds(c, v, w2, okmask);
        }
    }
    flush(true);
    __syncthreads();
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid];
    if (FX && FROM_ROWS) {
        const int bad0 = __syncthreads_or((int)(fx_bad & 1u)), bad1 = WIN ? __syncthreads_or((int)(fx_bad & 2u)) : 0;
        if ((bad0 || bad1) && tid == 0) __hip_atomic_fetch_or(&a.flags[7], (bad0 ? 1ULL : 0ULL) | (bad1 ? 2ULL : 0ULL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (XT) {   // the workgroup's exact-add statistics -> flags[6] (two 32-bit maxima; s_spill is free by now)
        if (tid < 2) s_spill[tid] = 0;
        __syncthreads();
        if (xinv) atomicMax(&s_spill[0], xinv);
        if (xexp) atomicMax(&s_spill[1], xexp);
        __syncthreads();
        if (tid < 2 && s_spill[tid]) atomicMax((uint32_t*)&a.flags[6] + tid, s_spill[tid]);
    }
    if (KN) {   // the workgroup's NULL-key rows -> the NULL slot of the operator's HBM table (one set of global atomics per workgroup)
        __shared__ uint64_t s_nk[3];   // sum hi, sum lo (compensated), rows
        __syncthreads();
        if (tid < 3) s_nk[tid] = tid == 0 ? F64_NEG_ZERO : 0;   // (the sum starts at -0.0: merge_init)
        __syncthreads();
        if (nk_cnt) {
            l_add_f64c(&s_nk[0], 1, nk_hi);
            __hip_atomic_fetch_add((double*)&s_nk[1], nk_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_nk[2], (uint64_t)nk_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        if (tid == 0 && s_nk[2]) {
            if (ld_agent(a.nk_tag) == EMPTY) st_agent(a.nk_tag, 0);
            if (a.nk_rows) __hip_atomic_fetch_add(a.nk_rows, s_nk[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.nk_valid) __hip_atomic_fetch_add(a.nk_valid, s_nk[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.nk_sum) {
                if (a.nk_lo_stride) {
                    g_add_f64c(a.nk_sum, a.nk_lo_stride, __longlong_as_double((long long)s_nk[0]));
                    __hip_atomic_fetch_add((double*)(a.nk_sum + a.nk_lo_stride), __longlong_as_double((long long)s_nk[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else __hip_atomic_fetch_add((double*)a.nk_sum, __longlong_as_double((long long)s_nk[0]) + __longlong_as_double((long long)s_nk[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// The NULL-key rows one dense attempt summed up (dring_scatter_kernel<..., KN> into scratch words [-, rows, valid, sum hi, sum lo]) ->
// the NULL slot of the operator's HBM table, once the attempt is known good (one thread).
__global__ void dnull_fold_kernel(const unsigned long long* scr, uint64_t* tag, uint64_t* rows, uint64_t* valid, uint64_t* sum, int64_t lo_stride) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!(scr[1] | scr[2])) return;   // (every hot program counts rows or valid inputs: no count, no NULL-key row)
    if (ld_agent(tag) == EMPTY) st_agent(tag, 0);
    if (rows) __hip_atomic_fetch_add(rows, scr[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (valid) __hip_atomic_fetch_add(valid, scr[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sum) {
        if (lo_stride) {
            g_add_f64c(sum, lo_stride, __longlong_as_double((long long)scr[3]));
            __hip_atomic_fetch_add((double*)(sum + lo_stride), __longlong_as_double((long long)scr[4]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else __hip_atomic_fetch_add((double*)sum, __longlong_as_double((long long)scr[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Entries of ONE batch waiting for the final pass (the deferred pass runs over the sets of every batch since the last one: a
// stream of record batches costs its scatter passes plus ONE final pass, like a single batch)
struct DSet {
    const double* vals; const void* codes; const uint32_t* counts;
    int64_t cap, pstride, rstride;
    int regions, pad;
};
// base of a region's entries: float64 values / 64-bit words, or 32-bit words (W32)
__device__ __forceinline__ const double* dfin_words(const double* base, int64_t entries, bool w32) {
    return w32 ? (const double*)((const uint32_t*)base + entries) : base + entries;
}
constexpr int DF_MAX_OUT = 8;
enum { DF_RUN = 0, DF_COLS = 1, DF_TABLE = 2 };
enum { DF_KEY = 0, DF_SUM = 1, DF_AVG = 2, DF_COUNT = 3 };
struct DTabSlot { double sum; float lo; uint32_t cnt; };   // 16 bytes; cnt == 0: no such group
struct DFinalArgs {
    int64_t pstride, rstride;   // region of (final partition f, producer rj) = f * pstride + rj * rstride
    DenseMap map;
    const double* vals;
    const void* codes;    // CT remainders: the slot inside the final partition
    const uint32_t* counts;
    int64_t cap;
    int regions;          // regions per final partition
    int64_t nfinal;
    int w_rows, w_valid, w_sum, w_lo;
    uint64_t* dkey;       // [2][dstride]
    uint64_t* dacc;       // [W][dstride]
    int64_t dstride;
    unsigned long long* flags;  // [0] overflow  [1] dense count
    // few final partitions (ranges of 2^14 .. 2^19 codes): `splits` workgroups share a partition's regions, each writes its
    // LDS table to part_* [(f * splits + split) * slots + slot] and dpart_merge_kernel adds them up
    int splits;
    uint64_t* part_sum;
    float* part_lo;
    uint32_t* part_cnt;
    // OUT = DF_COLS: the groups leave the final pass as RESULT COLUMNS (BaseAggregate::Result, base_aggregate.cpp:47-68, fused into
    // the pass: key, sum, avg, count written once, no dense partial state and no separate finalisation kernel re-reading it)
    int n_out;
    int out_kind[DF_MAX_OUT];     // DF_KEY / DF_SUM / DF_AVG / DF_COUNT
    int key_width;                // bytes of a DF_KEY cell (0 / 8: 64-bit cells; 4 / 2 / 1: a narrow key type the operator widened on arrival)
    void* out_ptr[DF_MAX_OUT];    // 8-byte cells, capacity dstride
    // OUT = DF_TABLE: the direct-addressed tables themselves, slot (f << TB | slot) = code' of the group (multi-GPU exchange:
    // every rank derives the same code map, so tables add up elementwise and a key's owner is a range of code')
    DTabSlot* table;
    // several batches (deferred pass): sets[0 .. nsets) in device memory replace vals / codes / counts / cap / regions / strides
    const DSet* sets;
    int nsets;
    // the table of a partition holds 2^(TB + sub_bits) slots, this launch covers the entries whose slot bits above TB equal `sub`
    // (64-bit compensation terms for 2^13-slot partitions: two launches of the 2^12-slot kernel)
    int sub_bits, sub;
    // A FEW groups next to the pass, in the operator's HBM table (round 4): what the scatter passes spilled (heavy keys of a skewed
    // distribution, keys outside the sampled code range), the NULL-key group, rows of batches that went through the scan.  The
    // pass folds them into its own output -- a group whose key it holds adds the table's words when it writes its row (a 2^16-bit
    // filter in LDS sends only possible matches to the table) and marks the slot; dside_append_kernel appends the unmarked ones --
    // instead of leaving fused result columns for run + table merge + a separate finalisation (skewed keys: +2.5 ms at G = 1e8).
    int has_side;
    GTable side;
    const uint32_t* side_bloom;   // [side_bloom_bits / 32]: one bit per table key; 2^16 bits are copied into LDS, a larger filter (many spilled
    uint32_t side_bloom_mask;     //  keys: ~64 bits per key, at most 8 MB) is read where it lies -- L2-resident, one 4-byte read per group
    uint8_t* side_found;          // [cap + 2]
    int64_t* null_pos;            // HOST (complete_pending): row of the NULL-key group + 1, 0 = none
    // two input columns (dpart_final2_kernel): the second value of an entry and the second column's words
    const double* vals2;
    int w_valid2, w_sum2, w_lo2;
    double fx_q;                  // fixed-point entries (dpart_final_kernel<..., FX>): the quantum 2^qe; 0 = float64 entries
    int fx_w32;                   // ... as 32-bit words (m << TB) | slot
    // PACKED composite keys (round 6): the pass belongs to the inner single-key operator of a multi-column GROUP BY whose key word holds
    // pack_n fields (PackParams: no dictionary-coded field, no NULL code in the data); a DF_KEY output column c then is field
    // key_field[c] of the word -- ((word >> shift) & mask) + lo, what key_unpack_kernel writes -- instead of the word itself
    int pack_n;
    int key_field[DF_MAX_OUT];
    int pack_shift[AGG_MAX_KEYS], pack_bits[AGG_MAX_KEYS];
    uint64_t pack_lo[AGG_MAX_KEYS];
};
__device__ __forceinline__ uint64_t df_key_cell(const DFinalArgs& a, int c, uint64_t key) {
    if (!a.pack_n) return key;
    const int f = a.key_field[c];
    return ((key >> a.pack_shift[f]) & ((1ULL << a.pack_bits[f]) - 1ULL)) + a.pack_lo[f];
}
// one cell of a result column; a KEY column of a narrow declared type (the operator widened the key on arrival: key_width = 4 / 2 / 1) gets
// cells of that width -- the low bytes of the widened value
__device__ __forceinline__ void df_store_cell(const DFinalArgs& a, int c, int64_t pos, uint64_t cell) {
    if (a.out_kind[c] == DF_KEY && a.key_width && a.key_width != 8) {
        if (a.key_width == 4) ((uint32_t*)a.out_ptr[c])[pos] = (uint32_t)cell;
        else if (a.key_width == 2) ((uint16_t*)a.out_ptr[c])[pos] = (uint16_t)cell;
        else ((uint8_t*)a.out_ptr[c])[pos] = (uint8_t)cell;
        return;
    }
    ((uint64_t*)a.out_ptr[c])[pos] = cell;
}
constexpr int DSIDE_BLOOM_BITS = 1 << 16;
// (a blocked filter: TWO bits per key inside one 32-bit word -- one load per test; ~64 filter bits per key leave ~0.2 % false positives.
// One bit per key left 1.5 %: about one lane per wave of the final pass went to the table for nothing, each a DRAM-latency probe, and
// the pass took twice its time)
__device__ __forceinline__ uint32_t dside_bloom_bit(uint64_t k, uint32_t mask) { return hash_u64(k ^ 0xD6E8FEB86659FD93ULL) & mask; }
__device__ __forceinline__ uint32_t dside_bloom_pattern(uint64_t k, uint32_t b) {
    const uint32_t h2 = hash_u64(k * 0x9E3779B97F4A7C15ULL + 0x632BE59BD9B4E019ULL);
    return (1u << (b & 31)) | (1u << ((h2 >> 7) & 31));
}
// the side table's group of `key` (if any) merged into (hi, lo, cnt) -- the TwoSum step of every other merge -- and marked found
__device__ __forceinline__ void dside_merge(const DFinalArgs& a, const uint32_t* lb, uint64_t key, double& hi, double& lo, uint64_t& cnt) {
    const GTable& g = a.side;
    uint64_t slot = ~0ULL;
    if (key == EMPTY) { if (g.tag[g.cap] != EMPTY) slot = g.cap; }
    else {
        const uint32_t bb = dside_bloom_bit(key, a.side_bloom_mask);
        const uint32_t word = (lb && a.side_bloom_mask == DSIDE_BLOOM_BITS - 1) ? lb[bb >> 5] : a.side_bloom[bb >> 5];   // (lb: the filter's LDS copy, if the kernel keeps one)
        const uint32_t pat = dside_bloom_pattern(key, bb);
        if ((word & pat) != pat) return;
        const uint64_t mask = g.cap - 1;
        uint64_t h = hash_u64(key) & mask;
        for (uint64_t probes = 0; probes <= mask; probes++) {
            const uint64_t t = g.tag[h];
            if (t == key) { slot = h; break; }
            if (t == EMPTY) break;
            h = (h + 1) & mask;
        }
    }
    if (slot == ~0ULL) return;
    const int wc = a.w_rows >= 0 ? a.w_rows : a.w_valid;
    if (wc >= 0) cnt += g.acc[(uint64_t)wc * g.stride + slot];
    if (a.w_sum >= 0) {
        const double sh = __longlong_as_double((long long)g.acc[(uint64_t)a.w_sum * g.stride + slot]);
        const double t = hi + sh;
        lo += two_sum_err(hi, sh, t);
        if (a.w_lo >= 0) lo += __longlong_as_double((long long)g.acc[(uint64_t)a.w_lo * g.stride + slot]);
        hi = t;
    }
    a.side_found[slot] = 1;
}
__global__ __launch_bounds__(256) void dside_bloom_kernel(GTable g, uint32_t* bloom, uint32_t bmask) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x; slot < (int64_t)g.cap; slot += stride) {
        const uint64_t t = g.tag[slot];
        if (t == EMPTY) continue;
        const uint32_t b = dside_bloom_bit(t, bmask);
        atomicOr(&bloom[b >> 5], dside_bloom_pattern(t, b));
    }
}
// the side table's groups the pass did not hold: appended behind its rows (result columns or dense partial state).  The NULL-key
// group leaves its row number + 1 in flags[4] (the caller gives the key column a validity bitmap).
// (null_only: a second, one-thread launch for the NULL-key slot -- that group comes LAST, as in the reference's single-key operator:
// single_numerical_hash_aggregate.cpp:24-32 appends null_group behind the map's groups)
__global__ __launch_bounds__(256) void dside_append_kernel(DFinalArgs a, int null_only) {
    const GTable& g = a.side;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t nslots = null_only ? (int64_t)g.cap + 2 : (int64_t)g.cap + 1;
    const int lane = threadIdx.x & 63;
    // Every workgroup owns a contiguous share of the slots and claims its output rows with ONE atomic on the global counter (a claim
    // per wave and 64 slots was 2.6e5 atomics on one address for a 2^24-slot table: ~10 ns each, 2.9 ms): count, claim, then write
    // behind a cursor in LDS.
    __shared__ unsigned long long s_claim;
    __shared__ uint32_t s_cnt, s_cur;
    const int64_t per = (nslots + gridDim.x - 1) / gridDim.x;
    const int64_t lo_s = null_only ? (int64_t)g.cap + 1 : (int64_t)blockIdx.x * per;
    const int64_t hi_s = null_only ? nslots : (lo_s + per < nslots ? lo_s + per : nslots);
    if (threadIdx.x == 0) { s_cnt = 0; s_cur = 0; }
    __syncthreads();
    uint32_t mine = 0;
    for (int64_t slot = lo_s + threadIdx.x; slot < hi_s; slot += 256) mine += (g.tag[slot] != EMPTY && !a.side_found[slot]) ? 1u : 0u;
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (s_cnt == 0) return;
    if (threadIdx.x == 0) s_claim = atomicAdd(&a.flags[1], (unsigned long long)s_cnt);
    __syncthreads();
    for (int64_t base = lo_s; base < hi_s; base += 256) {
        const int64_t slot = base + threadIdx.x;
        const uint64_t t = slot < hi_s ? g.tag[slot] : EMPTY;
        const bool want = t != EMPTY && !a.side_found[slot];
        const unsigned long long m = __ballot(want);
        if (!m) continue;
        uint32_t wbase = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) wbase = atomicAdd(&s_cur, (uint32_t)__popcll(m));
        wbase = __shfl(wbase, leader);
        if (!want) continue;
        const int64_t pos = (int64_t)(s_claim + wbase + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL)));
        if (pos >= a.dstride) { __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); continue; }
        const bool isnull = slot == (int64_t)g.cap + 1;
        const uint64_t key = slot < (int64_t)g.cap ? t : (isnull ? 0ULL : EMPTY);
        if (isnull) a.flags[4] = (unsigned long long)pos + 1ULL;
        const int wc = a.w_rows >= 0 ? a.w_rows : a.w_valid;
        const uint64_t cnt = wc >= 0 ? g.acc[(uint64_t)wc * g.stride + slot] : 0;
        const uint64_t hib = a.w_sum >= 0 ? g.acc[(uint64_t)a.w_sum * g.stride + slot] : 0;
        const uint64_t lob = a.w_lo >= 0 ? g.acc[(uint64_t)a.w_lo * g.stride + slot] : 0;
        if (a.n_out > 0) {
            const double sum = __longlong_as_double((long long)hib) + (a.w_lo >= 0 ? __longlong_as_double((long long)lob) : 0.0);
            for (int c = 0; c < a.n_out; c++) {
                uint64_t cell;
                switch (a.out_kind[c]) {
                    case DF_KEY: cell = df_key_cell(a, c, key); break;
                    case DF_SUM: cell = (uint64_t)__double_as_longlong(sum); break;
                    case DF_AVG: cell = (uint64_t)__double_as_longlong(sum / (double)cnt); break;
                    default: cell = cnt; break;
                }
                df_store_cell(a, c, pos, cell);
            }
        } else {
            a.dkey[pos] = key;
            a.dkey[a.dstride + pos] = isnull ? 1 : 0;
            if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = g.acc[(uint64_t)a.w_rows * g.stride + slot];
            if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = g.acc[(uint64_t)a.w_valid * g.stride + slot];
            if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = hib;
            if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = lob;
        }
    }
}

// Final pass: one workgroup per final partition, accumulators direct-addressed by the entry's slot.
// TB: log2 of the slots per partition; DF_BLOCK threads (512, or 1024 for the 128 KB table).
// OUT: what leaves the pass (DF_RUN: dense partial state; DF_COLS: result columns; DF_TABLE: the tables).  LOT: type of the
// compensation terms in LDS -- float (they are ~2^-53 of the sum: 24 bits of them keep hi + lo within 2^-77), or double for the
// rare data whose error terms leave the float range (s_bad: sums beyond ~1e54).
// EXACT (round 6): the scatter passes PROVED that every float add of this pass is exact (DensePending::exact_ok: all surviving values are
// multiples of one power of two q and rows x max|v| < 2^53 q, so every partial sum in any order is representable) -- the compensation
// words would stay zero, so they are not kept: {sum, count} slots (48 KB at 2^12 slots: three workgroups per CU), and the two LDS
// atomics of an entry are NON-RETURNING (ds_add_f64 + ds_add_u32: no load -> returning atomic -> TwoSum -> second atomic chain, which
// had the waves of this pass waiting 74 % of their cycles, profiles/r04_pmc_sq_headline.txt).  Same result bits as the compensated pass.
// FX (round 6): the entries are fixed-point words (m << TB) | slot (dring_scatter_kernel<..., FX>); the sums are 64-bit INTEGER adds of m
// (exact by construction: |m| < 2^31, fewer than 2^31 rows per pass), and a group's sum leaves as (hi, lo) = the two-term float
// expansion of total * 2^qe -- hi is the correctly rounded exact sum, what the compensated float pass produces.
template <typename CT, int TB, bool SPLIT = false, int OUT = DF_RUN, typename LOT = float, bool EXACT = false, bool FX = false>
// (at least four waves per SIMD = two 512-thread workgroups per CU: the double-buffered chunk registers must not cost the second workgroup)
#ifndef VNM_DF12_BLOCK
#define VNM_DF12_BLOCK 512
#endif
__global__ __launch_bounds__(TB >= 13 ? 1024 : (TB == 12 ? VNM_DF12_BLOCK : 512)) __attribute__((amdgpu_waves_per_eu(TB == 12 && VNM_DF12_BLOCK == 1024 ? 8 : 4, 8))) void dpart_final_kernel(DFinalArgs a) {
    constexpr int DP_SLOTS = 1 << TB, DP_TBITS = TB, DF_BLOCK = TB >= 13 ? 1024 : (TB == 12 ? VNM_DF12_BLOCK : 512);
    __shared__ uint64_t lsum[DP_SLOTS];
    static_assert(!FX || (EXACT && !SPLIT), "fixed-point entries: no compensation words, no split tables");
    __shared__ LOT llo[EXACT ? 1 : DP_SLOTS];        // compensation terms in single precision, see part_agg_kernel
    __shared__ uint32_t lcnt[DP_SLOTS];
    __shared__ uint32_t s_n, s_bad;
    __shared__ unsigned long long s_base;
    __shared__ uint32_t sbloom[(!SPLIT && OUT != DF_TABLE && !FX) ? DSIDE_BLOOM_BITS / 32 : 1];   // the side table's key filter (has_side; FX: read where it lies -- 8 KB less LDS, three workgroups per CU)
    const int tid = threadIdx.x, lane = tid & 63;
    const CT* const codes = (const CT*)a.codes;
    const int64_t nwork = SPLIT ? a.nfinal * a.splits : a.nfinal;
    if (!SPLIT && OUT != DF_TABLE && !FX && a.has_side && a.side_bloom_mask == DSIDE_BLOOM_BITS - 1) {
        for (int i = tid; i < DSIDE_BLOOM_BITS / 32; i += DF_BLOCK) sbloom[i] = a.side_bloom[i];
        __syncthreads();
    }
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t f = SPLIT ? w / a.splits : w;
        const int sp = SPLIT ? (int)(w % a.splits) : 0;
        const int r0 = SPLIT ? (int)((int64_t)sp * a.regions / a.splits) : 0;
        const int r1 = SPLIT ? (int)((int64_t)(sp + 1) * a.regions / a.splits) : a.regions;
        for (int i = tid; i < DP_SLOTS; i += DF_BLOCK) { lsum[i] = FX ? 0ULL : F64_NEG_ZERO; if (!EXACT) llo[i] = (LOT)0; lcnt[i] = 0; }   // (sums start at -0.0: merge_init; FX: integer totals)
        if (tid == 0) { s_n = 0; s_bad = 0; }
        __syncthreads();
        const int nsets = a.sets ? a.nsets : 1;
        for (int si = 0; si < nsets; si++) {
        DSet st;
        if (a.sets) st = a.sets[si];
        else { st.vals = a.vals; st.codes = a.codes; st.counts = a.counts; st.cap = a.cap; st.pstride = a.pstride; st.rstride = a.rstride; st.regions = a.regions; st.pad = 0; }
        // SPLIT over several batches: the (batch, region) pairs of the partition are dealt round-robin to its `splits` workgroups
        const int rr0 = (SPLIT && !a.sets) ? r0 : 0, rr1 = (SPLIT && !a.sets) ? r1 : st.regions;
        auto accum = [&](uint32_t codev, double x) {
            if (a.sub_bits && ((codev >> DP_TBITS) & ((1u << a.sub_bits) - 1u)) != (uint32_t)a.sub) return;
            const uint32_t slot = codev & (DP_SLOTS - 1);
            if (FX) {
                atomicAdd((unsigned long long*)&lsum[slot], (unsigned long long)fx_of(x));
            } else if (!EXACT && a.w_lo >= 0) {
                const double old = __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const double er = two_sum_err(old, x, old + x);
                if (er != 0.0) {
                    const LOT ef = (LOT)er;
                    if (sizeof(LOT) == 4 && ef - ef != (LOT)0) s_bad = 1;
                    __hip_atomic_fetch_add(&llo[slot], ef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            atomicAdd(&lcnt[slot], 1u);
        };
        auto load_pair = [&](const double* sv, const CT* sc, uint32_t i, double2* pv, uint32_t* c0, uint32_t* c1) {
            if (!(FX && a.fx_w32)) *pv = *(const double2*)(sv + i);
            if (FX && a.fx_w32) {   // 32-bit words: sv points at this region's words, i counts words
                const uint2 t = *(const uint2*)((const uint32_t*)sv + i);
                *c0 = t.x & (DP_SLOTS - 1); *c1 = t.y & (DP_SLOTS - 1);
                pv->x = fx_bits((int64_t)((int32_t)t.x >> DP_TBITS)); pv->y = fx_bits((int64_t)((int32_t)t.y >> DP_TBITS));
                return;
            }
            if (FX) {   // entry word = (m << TB) | slot: the value slot carries m
                const uint64_t w0 = (uint64_t)__double_as_longlong(pv->x), w1 = (uint64_t)__double_as_longlong(pv->y);
                *c0 = (uint32_t)w0 & (DP_SLOTS - 1); *c1 = (uint32_t)w1 & (DP_SLOTS - 1);
                pv->x = fx_bits((int64_t)w0 >> DP_TBITS); pv->y = fx_bits((int64_t)w1 >> DP_TBITS);
                return;
            }
            if (sizeof(CT) == 2) { const ushort2 t = *(const ushort2*)(sc + i); *c0 = t.x; *c1 = t.y; }
            else { const uint2 t = *(const uint2*)(sc + i); *c0 = t.x; *c1 = t.y; }
        };
        if (a.sets && st.pad) {
            // SMALL regions (a stream of 2^24-row batches leaves ~64 entries per region, thousands of regions per partition): a
            // region per WAVE, the waves of the workgroup side by side; every wave fetches the counts of its next 64 regions with one
            // load (lane l: region l) and keeps FOUR regions' entries in flight -- a whole workgroup walking region after region
            // paid a dependent count load + data load ~8000 times per partition (42 ms for 60 batches of a 1e9-row stream).
            const int splits_ = SPLIT ? a.splits : 1;
            const int n_groups = DF_BLOCK / 64, my_group = tid >> 6;
            const int r_first = SPLIT ? (((sp - si) % splits_) + splits_) % splits_ : 0;
            const int stride_r = n_groups * splits_;
            const int r_w = r_first + my_group * splits_;
            const int cntr = r_w < st.regions ? (st.regions - r_w + stride_r - 1) / stride_r : 0;
            for (int base = 0; base < cntr; base += 64) {
                const int rl = r_w + (base + lane) * stride_r;
                const uint32_t cl = base + lane < cntr ? st.counts[f * st.pstride + (int64_t)rl * st.rstride] : 0u;
                const int m = cntr - base < 64 ? cntr - base : 64;
                for (int k = 0; k < m; k += 4) {
                    double2 pv[4];
                    uint32_t pc0[4], pc1[4], nn[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        nn[u] = k + u < m ? (uint32_t)__shfl((int)cl, k + u) : 0u;
                        if (2u * lane < nn[u]) {
                            const int64_t region = f * st.pstride + (int64_t)(r_w + (base + k + u) * stride_r) * st.rstride;
                            load_pair(dfin_words(st.vals, region * st.cap, FX && a.fx_w32), (const CT*)st.codes + region * st.cap, 2u * lane, &pv[u], &pc0[u], &pc1[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (2u * lane < nn[u]) accum(pc0[u], pv[u].x);
                        if (2u * lane + 1 < nn[u]) accum(pc1[u], pv[u].y);
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {   // (a region beyond 128 entries: the rest of it, 128 entries per step)
                        if (nn[u] <= 128u) continue;
                        const int64_t region = f * st.pstride + (int64_t)(r_w + (base + k + u) * stride_r) * st.rstride;
                        for (uint32_t i = 128u + 2u * lane; i < nn[u]; i += 128u) {
                            double2 x; uint32_t c0, c1;
                            load_pair(dfin_words(st.vals, region * st.cap, FX && a.fx_w32), (const CT*)st.codes + region * st.cap, i, &x, &c0, &c1);
                            accum(c0, x.x);
                            if (i + 1 < nn[u]) accum(c1, x.y);
                        }
                    }
                }
            }
        } else {
        // Large regions (one batch of 1e9 rows: ~4000 entries each, a handful per partition): the whole workgroup walks them chunk by
        // chunk -- two pairs of entries per lane and chunk (16-byte + 4-byte loads; regions are 16-byte aligned: their capacity is a multiple
        // of 8 entries) -- and the NEXT chunk's loads (and the count of the region after next) are in flight while this chunk's
        // entries go through the LDS atomics (round 4).  Before, every region was a dependent chain count -> loads -> atomics, one
        // after the other: 2^15 partitions x 4 regions paid a DRAM latency each with nothing else to do (the pass moved its 7.4 GB at
        // 3.9 TB/s).
        {
        constexpr int NP = (TB == 12 && VNM_DF12_BLOCK == 1024) ? 1 : 2;   // pairs of entries per lane and chunk: two chunks (this one, the next) are live
        constexpr uint32_t CH = DF_BLOCK * 2 * NP;
        auto region_ok = [&](int rj) { return !(SPLIT && a.sets && (rj + si) % a.splits != sp); };
        auto count_of = [&](int rj) -> uint32_t { return rj < rr1 ? st.counts[f * st.pstride + (int64_t)rj * st.rstride] : 0u; };
        auto after = [&](int rj) { rj++; while (rj < rr1 && !region_ok(rj)) rj++; return rj; };
        int cr = rr0;
        while (cr < rr1 && !region_ok(cr)) cr++;
        uint32_t cn = count_of(cr), ci = 0;
        int nr = after(cr);
        uint32_t nn = count_of(nr);           // one region ahead: its latency is hidden behind a chunk
        auto norm = [&]() { while (cr < rr1 && ci >= cn) { cr = nr; cn = nn; ci = 0; nr = after(cr); nn = count_of(nr); } };
        auto issue = [&](int rj, uint32_t n, uint32_t i0s, double2* pv, uint32_t* c0, uint32_t* c1) {
            const int64_t region = f * st.pstride + (int64_t)rj * st.rstride;
            const double* sv = dfin_words(st.vals, region * st.cap, FX && a.fx_w32);
            const CT* sc = (const CT*)st.codes + region * st.cap;
#pragma unroll
            for (int u = 0; u < NP; u++) {
                const uint32_t i = i0s + 2u * ((uint32_t)u * DF_BLOCK + tid);
                if (i < n) load_pair(sv, sc, i, &pv[u], &c0[u], &c1[u]);
            }
        };
        double2 pvA[NP], pvB[NP];
        uint32_t c0A[NP], c1A[NP], c0B[NP], c1B[NP];
        uint32_t nA = 0, iA = 0, nB = 0, iB = 0;
        norm();
        bool haveA = cr < rr1;
        if (haveA) { issue(cr, cn, ci, pvA, c0A, c1A); nA = cn; iA = ci; ci += CH; norm(); }
        while (haveA) {
            const bool haveB = cr < rr1;
            if (haveB) { issue(cr, cn, ci, pvB, c0B, c1B); nB = cn; iB = ci; ci += CH; norm(); }
#pragma unroll
            for (int u = 0; u < NP; u++) {
                const uint32_t i = iA + 2u * ((uint32_t)u * DF_BLOCK + tid);
                if (i < nA) accum(c0A[u], pvA[u].x);
                if (i + 1 < nA) accum(c1A[u], pvA[u].y);
            }
            if (!haveB) break;
#pragma unroll
            for (int u = 0; u < NP; u++) { pvA[u] = pvB[u]; c0A[u] = c0B[u]; c1A[u] = c1B[u]; }
            nA = nB; iA = iB;
        }
        }
        }
        }
        __syncthreads();
        if (s_bad) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (SPLIT) {   // this workgroup saw only a share of the partition's entries: the tables go out as they are
            uint64_t* ps = a.part_sum + (size_t)w * DP_SLOTS;
            float* pl = a.part_lo + (size_t)w * DP_SLOTS;
            uint32_t* pc = a.part_cnt + (size_t)w * DP_SLOTS;
            for (int i = tid; i < DP_SLOTS; i += DF_BLOCK) { ps[i] = lsum[i]; pl[i] = EXACT ? 0.0f : (float)llo[EXACT ? 0 : i]; pc[i] = lcnt[i]; }
            __syncthreads();
            continue;
        }
        if (OUT == DF_TABLE) {   // (a float compensation term, as in the split tables: the double variant is not exchanged)
            DTabSlot* t = a.table + ((size_t)f << DP_TBITS);
            for (int i = tid; i < DP_SLOTS; i += DF_BLOCK) {
                DTabSlot o;
                o.sum = __longlong_as_double((long long)lsum[i]); o.lo = EXACT ? 0.0f : (float)llo[EXACT ? 0 : i]; o.cnt = lcnt[i];
                if (FX) { double fh, fl; fx_expand((int64_t)lsum[i], a.fx_q, &fh, &fl); o.sum = o.cnt ? fh : -0.0; o.lo = (float)fl; }
                t[i] = o;
            }
            __syncthreads();
            continue;
        }
        // groups of this partition -> dense rows, in slot order
        uint32_t mine = 0;
        for (int i = tid; i < DP_SLOTS; i += DF_BLOCK) mine += lcnt[i] != 0 ? 1u : 0u;   // (tables of fewer slots than threads: 2^7 / 2^8, round 6)
        pa_block_add(&s_n, mine);
        __syncthreads();
        const uint32_t ngroups = s_n;
        __syncthreads();
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < DP_SLOTS; i0 += DF_BLOCK) {
            const int i = i0 + tid;
            const bool occ = i < DP_SLOTS && lcnt[i] != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                const uint64_t key = dense_key_of(a.map, (((uint32_t)f << a.sub_bits | (uint32_t)a.sub) << DP_TBITS) | (uint32_t)i);
                double ghi = __longlong_as_double((long long)lsum[i]), glo = (!EXACT && a.w_lo >= 0) ? (double)llo[EXACT ? 0 : i] : 0.0;
                if (FX) fx_expand((int64_t)lsum[i], a.fx_q, &ghi, &glo);
                uint64_t gcnt = lcnt[i];
                if (OUT != DF_TABLE && a.has_side) dside_merge(a, FX ? nullptr : sbloom, key, ghi, glo, gcnt);   // (+ what the operator's HBM table holds for this key)
                if (OUT == DF_COLS) {
                    // the same expressions as fin_cell (vnm_agg.hip): sum = hi + lo, avg = (hi + lo) / count
                    const double sum = fsum2(ghi, glo);
                    for (int c = 0; c < a.n_out; c++) {
                        uint64_t cell;
                        switch (a.out_kind[c]) {
                            case DF_KEY: cell = df_key_cell(a, c, key); break;
                            case DF_SUM: cell = (uint64_t)__double_as_longlong(sum); break;
                            case DF_AVG: cell = (uint64_t)__double_as_longlong(sum / (double)gcnt); break;
                            default: cell = gcnt; break;
                        }
                        df_store_cell(a, c, pos, cell);
                    }
                } else {
                    a.dkey[pos] = key;
                    a.dkey[a.dstride + pos] = 0;
                    if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = gcnt;
                    if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = gcnt;
                    if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(ghi);
                    if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong(glo);
                }
            }
        }
        __syncthreads();
    }
}

// ---- the final pass over fixed-point entry words, lean form (round 6) -------------------------------------------------------------
// dpart_final_kernel serves every shape (several batches, small regions, split tables, side table, three entry formats) and pays for
// it: 121-128 VGPRs, two workgroups per CU, and at the start of EVERY partition a count load followed by a data load with nothing
// else in flight -- the headline's final pass took 1.8 ms whether its entries were 10 or 8 bytes.  This kernel is the common case
// only: ONE batch of fixed-point words in large regions, no side table.  {int64 sum, u32 count} slots (48 KB at 2^12 slots: three
// workgroups per CU), one pair of entries per lane and chunk, the NEXT chunk always in flight -- across partition boundaries: the
// counts of the workgroup's next partition are fetched while this one is accumulated, its first chunk while this one's groups are
// written.  Output as dpart_final_kernel's (slot order, one ballot per 64 slots: collapse_parts' units of 64 codes hold).
// W32: the entries are 32-bit words (m << TB) | slot -- four per lane and chunk
// SIDE: the operator's HBM table holds groups as well (the NULL-key group of a nullable key, spilled heavy keys, keys outside the code
// range): a group that is written looks its key up there (the filter is read where it lies) and takes the table's words along, as
// dpart_final_kernel does; the table's other groups are appended by dside_append_kernel afterwards.
template <int TB, int OUT, bool W32 = false, bool SIDE = false>
__global__ __launch_bounds__(TB >= 13 ? 1024 : 512) void dfx_final_kernel(DFinalArgs a, DSet st) {
    constexpr int SLOTS = 1 << TB, BLOCK = TB >= 13 ? 1024 : 512;
    constexpr int MAXR = 512, CQ = (MAXR + BLOCK - 1) / BLOCK;   // regions per partition (the host checks), count registers per thread
    __shared__ unsigned long long lsum[SLOTS];
    __shared__ uint32_t lcnt[SLOTS];
    __shared__ uint32_t s_cnt[2][MAXR];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = st.regions;
    const int64_t nwork = a.nfinal;
    const unsigned long long* const words = (const unsigned long long*)st.vals;
    auto region_of = [&](int64_t f, int rj) -> int64_t { return f * st.pstride + (int64_t)rj * st.rstride; };
    int buf = 0;
    if ((int64_t)blockIdx.x < nwork) for (int r = tid; r < R && r < MAXR; r += BLOCK) s_cnt[0][r] = st.counts[region_of(blockIdx.x, r)];
    __syncthreads();
    // (uniform) the chunk cursor of a partition: region rj, first entry ci of the chunk; a chunk is 2 * BLOCK entries of one region
    auto first_region = [&](const uint32_t* cnt) { int r = 0; while (r < R && cnt[r] == 0) r++; return r; };
    constexpr uint32_t EPL = W32 ? 4u : 2u, CHK = EPL * BLOCK;   // entries per lane / per chunk (16 bytes per lane either way)
    ulonglong2 pa, pb;                 // this chunk's entries, the next chunk's
    uint32_t na = 0, ia = 0, nb = 0, ib = 0;
    auto load_chunk = [&](int64_t f, int rj, uint32_t ci, uint32_t n, ulonglong2* p) {
        const uint32_t i = ci + EPL * tid;
        if (i < n) *p = W32 ? *(const ulonglong2*)((const uint32_t*)words + region_of(f, rj) * st.cap + i) : *(const ulonglong2*)(words + region_of(f, rj) * st.cap + i);
    };
    auto add_entry = [&](uint32_t slot, long long m) {
        atomicAdd(&lsum[slot], (unsigned long long)m);
        atomicAdd(&lcnt[slot], 1u);
    };
    // the first chunk of the first partition
    int rj = 0; uint32_t ci = 0;
    bool have = false;
    if ((int64_t)blockIdx.x < nwork) {
        rj = first_region(s_cnt[0]);
        have = rj < R;
        if (have) { na = s_cnt[0][rj]; ia = 0; load_chunk(blockIdx.x, rj, 0, na, &pa); ci = CHK; }
    }
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t f = w, wn = w + gridDim.x;
        for (int i = tid; i < SLOTS; i += BLOCK) { lsum[i] = 0ULL; lcnt[i] = 0; }
        if (tid == 0) s_n = 0;
        // the counts of the workgroup's next partition: in flight during the accumulation below
        uint32_t cnext[CQ];
        if (wn < nwork) {
#pragma unroll
            for (int q = 0; q < CQ; q++) { const int r = q * BLOCK + tid; cnext[q] = r < R ? st.counts[region_of(wn, r)] : 0u; }
        }
        __syncthreads();
        const uint32_t* cnt = s_cnt[buf];
        while (have) {
            // the chunk after this one (same region, or the next non-empty one)
            int rn = rj; uint32_t cin = ci;
            while (rn < R && cin >= cnt[rn]) { rn++; cin = 0; }
            const bool more = rn < R;
            if (more) { nb = cnt[rn]; ib = cin; load_chunk(f, rn, cin, nb, &pb); }
            const uint32_t i = ia + EPL * tid;
            if (i < na) {
                if (W32) {
                    const uint32_t w0 = (uint32_t)pa.x, w1 = (uint32_t)(pa.x >> 32), w2 = (uint32_t)pa.y, w3 = (uint32_t)(pa.y >> 32);
                    add_entry(w0 & (SLOTS - 1), (long long)((int32_t)w0 >> TB));
                    if (i + 1 < na) add_entry(w1 & (SLOTS - 1), (long long)((int32_t)w1 >> TB));
                    if (i + 2 < na) add_entry(w2 & (SLOTS - 1), (long long)((int32_t)w2 >> TB));
                    if (i + 3 < na) add_entry(w3 & (SLOTS - 1), (long long)((int32_t)w3 >> TB));
                } else {
                    add_entry((uint32_t)pa.x & (SLOTS - 1), (long long)pa.x >> TB);
                    if (i + 1 < na) add_entry((uint32_t)pa.y & (SLOTS - 1), (long long)pa.y >> TB);
                }
            }
            have = more;
            if (more) { pa = pb; na = nb; ia = ib; rj = rn; ci = cin + CHK; }
        }
        if (wn < nwork) {
#pragma unroll
            for (int q = 0; q < CQ; q++) { const int r = q * BLOCK + tid; if (r < R) s_cnt[buf ^ 1][r] = cnext[q]; }
        }
        __syncthreads();
        // the first chunk of the next partition: in flight while this partition's groups are written
        if (wn < nwork) {
            const uint32_t* cn2 = s_cnt[buf ^ 1];
            rj = first_region(cn2);
            have = rj < R;
            if (have) { na = cn2[rj]; ia = 0; load_chunk(wn, rj, 0, na, &pa); ci = CHK; }
        }
        buf ^= 1;
        if (OUT == DF_TABLE) {
            DTabSlot* t = a.table + ((size_t)f << TB);
            for (int i = tid; i < SLOTS; i += BLOCK) {
                DTabSlot o;
                double fh, fl;
                fx_expand((long long)lsum[i], a.fx_q, &fh, &fl);
                o.cnt = lcnt[i]; o.sum = o.cnt ? fh : -0.0; o.lo = (float)fl;
                t[i] = o;
            }
            __syncthreads();
            continue;
        }
        uint32_t mine = 0;
        for (int i = tid; i < SLOTS; i += BLOCK) mine += lcnt[i] != 0 ? 1u : 0u;
        pa_block_add(&s_n, mine);
        __syncthreads();
        const uint32_t ngroups = s_n;
        __syncthreads();
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < SLOTS; i0 += BLOCK) {
            const int i = i0 + tid;
            const uint32_t gc = i < SLOTS ? lcnt[i] : 0u;
            const bool occ = gc != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                const uint64_t key = dense_key_of(a.map, ((uint32_t)f << TB) | (uint32_t)i);
                double ghi, glo;
                fx_expand((long long)lsum[i], a.fx_q, &ghi, &glo);
                uint64_t gcnt = gc;
                if (SIDE && OUT != DF_TABLE) dside_merge(a, nullptr, key, ghi, glo, gcnt);
                if (OUT == DF_COLS) {
                    const double sum = SIDE ? fsum2(ghi, glo) : ghi;          // (without a side table hi IS the correctly rounded total: fsum2(hi, lo) == hi)
                    for (int c = 0; c < a.n_out; c++) {
                        uint64_t cell;
                        switch (a.out_kind[c]) {
                            case DF_KEY: cell = df_key_cell(a, c, key); break;
                            case DF_SUM: cell = (uint64_t)__double_as_longlong(sum); break;
                            case DF_AVG: cell = (uint64_t)__double_as_longlong(sum / (double)gcnt); break;
                            default: cell = gcnt; break;
                        }
                        df_store_cell(a, c, pos, cell);
                    }
                } else {
                    a.dkey[pos] = key;
                    a.dkey[a.dstride + pos] = 0;
                    if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = gcnt;
                    if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = gcnt;
                    if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(ghi);
                    if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong(glo);
                }
            }
        }
        __syncthreads();
    }
}

// The final pass for entries that carry TWO values (SELECT k, sum(a), sum(b) [, count ...]: round 4): 2^11 (2^12) direct-addressed slots of
// {sum1, sum2: f64; lo1, lo2: f32 compensation; rows: u32} = 56 (112) KB of LDS, two 512-thread workgroups per CU; one batch, dense partial
// state out (DF_RUN).  The regions of a partition are walked one after the other, two pairs of entries per lane in flight.
template <typename CT, int TB>
__global__ __launch_bounds__(TB >= 12 ? 1024 : 512) void dpart_final2_kernel(DFinalArgs a) {
    constexpr int DP_SLOTS = 1 << TB, DF_BLOCK = TB >= 12 ? 1024 : 512;   // (2^12 slots: 112 KB, one 1024-thread workgroup per CU)
    __shared__ uint64_t lsum[DP_SLOTS], lsum2[DP_SLOTS];
    __shared__ float llo[DP_SLOTS], llo2[DP_SLOTS];
    __shared__ uint32_t lcnt[DP_SLOTS];
    __shared__ uint32_t s_n, s_bad;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t f = blockIdx.x; f < a.nfinal; f += gridDim.x) {
        for (int i = tid; i < DP_SLOTS; i += DF_BLOCK) { lsum[i] = F64_NEG_ZERO; lsum2[i] = F64_NEG_ZERO; llo[i] = 0.f; llo2[i] = 0.f; lcnt[i] = 0; }
        if (tid == 0) { s_n = 0; s_bad = 0; }
        __syncthreads();
        auto add_comp = [&](uint64_t* sum, float* lo, uint32_t slot, double x) {
            const double old = __hip_atomic_fetch_add((double*)&sum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const double er = two_sum_err(old, x, old + x);
            if (er != 0.0) {
                const float ef = (float)er;
                if (ef - ef != 0.f) s_bad = 1;
                __hip_atomic_fetch_add(&lo[slot], ef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
        auto accum = [&](uint32_t codev, double x, double y) {
            const uint32_t slot = codev & (DP_SLOTS - 1);
            add_comp(lsum, llo, slot, x);
            add_comp(lsum2, llo2, slot, y);
            atomicAdd(&lcnt[slot], 1u);
        };
        for (int rj = 0; rj < a.regions; rj++) {
            const int64_t region = f * a.pstride + rj * a.rstride;
            const uint32_t n = a.counts[region];
            const double* sv = a.vals + region * a.cap;
            const double* sw = a.vals2 + region * a.cap;
            const CT* sc = (const CT*)a.codes + region * a.cap;
            for (uint32_t i0 = 0; i0 < n; i0 += DF_BLOCK * 4) {
                double2 pv[2], pw[2];
                uint32_t c0[2], c1[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t i = i0 + 2u * ((uint32_t)u * DF_BLOCK + tid);
                    if (i < n) {
                        pv[u] = *(const double2*)(sv + i);
                        pw[u] = *(const double2*)(sw + i);
                        if (sizeof(CT) == 2) { const ushort2 t = *(const ushort2*)(sc + i); c0[u] = t.x; c1[u] = t.y; }
                        else { const uint2 t = *(const uint2*)(sc + i); c0[u] = t.x; c1[u] = t.y; }
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t i = i0 + 2u * ((uint32_t)u * DF_BLOCK + tid);
                    if (i < n) accum(c0[u], pv[u].x, pw[u].x);
                    if (i + 1 < n) accum(c1[u], pv[u].y, pw[u].y);
                }
            }
        }
        __syncthreads();
        if (s_bad) {   // a compensation term beyond the float range: the caller takes the hash partitions
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < DP_SLOTS / DF_BLOCK; q++) mine += lcnt[q * DF_BLOCK + tid] != 0 ? 1u : 0u;
        pa_block_add(&s_n, mine);
        __syncthreads();
        const uint32_t ngroups = s_n;
        __syncthreads();
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < DP_SLOTS; i0 += DF_BLOCK) {
            const int i = i0 + tid;
            const bool occ = lcnt[i] != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                a.dkey[pos] = dense_key_of(a.map, ((uint32_t)f << TB) | (uint32_t)i);
                a.dkey[a.dstride + pos] = 0;
                const uint64_t cnt = lcnt[i];
                if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = cnt;
                if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = cnt;
                if (a.w_valid2 >= 0) a.dacc[(int64_t)a.w_valid2 * a.dstride + pos] = cnt;
                if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = lsum[i];
                if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong((double)llo[i]);
                if (a.w_sum2 >= 0) a.dacc[(int64_t)a.w_sum2 * a.dstride + pos] = lsum2[i];
                if (a.w_lo2 >= 0) a.dacc[(int64_t)a.w_lo2 * a.dstride + pos] = (uint64_t)__double_as_longlong((double)llo2[i]);
            }
        }
        __syncthreads();
    }
}

// Owner-side merge of the multi-GPU exchange: `nsrc` table slices [n] (one per rank, same code' range) add up slot by slot --
// counts plainly, (sum, lo) pairs with the TwoSum step of every other merge, in rank order, so the result does not depend on
// which rank holds it -- and the occupied slots leave as a dense run (key rebuilt from code' = code0 + slot).
// One thread per slot, the output rows in slot order inside a workgroup's share; no atomics but the claim of that share's rows.
struct DTabMergeArgs {
    DenseMap map;
    const DTabSlot* src[64];
    int nsrc;
    int64_t n;            // slots of the slice
    uint32_t code0;       // code' of slot 0
    int w_rows, w_valid, w_sum, w_lo;
    uint64_t* dkey;
    uint64_t* dacc;
    int64_t dstride;
    unsigned long long* flags;   // [0] overflow  [1] dense count
};
// 1024 threads x DTM_PER slots each per workgroup: ONE claim of output rows per 8192 slots (a claim per 512 slots -- 262 144
// same-address atomics for a 2^27-slot table -- made this pass 3.2 ms; it moves 6 GB).
constexpr int DTM_PER = 8, DTM_BLOCK = 1024;
__global__ __launch_bounds__(DTM_BLOCK) void dtable_merge_kernel(DTabMergeArgs a) {
    __shared__ uint32_t wcnt[DTM_PER][DTM_BLOCK / 64];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * (DTM_PER * DTM_BLOCK);
    double hi[DTM_PER], lo[DTM_PER];
    uint32_t cnt[DTM_PER];
    uint64_t ball[DTM_PER];
    if (tid == 0) s_n = 0;
#pragma unroll
    for (int j = 0; j < DTM_PER; j++) {
        const int64_t i = base + (int64_t)j * DTM_BLOCK + tid;
        hi[j] = -0.0; lo[j] = 0.0; cnt[j] = 0;
        if (i < a.n) {
            for (int r = 0; r < a.nsrc; r++) {
                const ulonglong2 raw = *(const ulonglong2*)(a.src[r] + i);   // {sum bits, lo f32 | count << 32}
                const uint32_t c = (uint32_t)(raw.y >> 32);
                if (c == 0) continue;
                cnt[j] += c;
                const double x = __longlong_as_double((long long)raw.x);
                const double s2 = hi[j] + x;
                lo[j] += two_sum_err(hi[j], x, s2) + (double)__uint_as_float((uint32_t)raw.y);
                hi[j] = s2;
            }
        }
        ball[j] = __ballot(cnt[j] != 0);
        if (lane == 0) wcnt[j][wave] = (uint32_t)__popcll(ball[j]);
    }
    __syncthreads();
    if (tid < 64) {   // exclusive scan of the DTM_PER x 16 wave counts, in slot order (j major): one wave, two entries per lane
        constexpr int NW = DTM_PER * (DTM_BLOCK / 64);   // 128
        uint32_t* flat = &wcnt[0][0];
        const uint32_t a0 = flat[2 * tid], a1 = flat[2 * tid + 1];
        uint32_t inc = a0 + a1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        const uint32_t ex = inc - (a0 + a1);
        flat[2 * tid] = ex; flat[2 * tid + 1] = ex + a0;
        if (tid == 63) { s_n = inc; s_base = atomicAdd(&a.flags[1], (unsigned long long)inc); }
        (void)NW;
    }
    __syncthreads();
    if ((int64_t)(s_base + s_n) > a.dstride) {
        if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
#pragma unroll
    for (int j = 0; j < DTM_PER; j++) {
        if (cnt[j] == 0) continue;
        const int64_t i = base + (int64_t)j * DTM_BLOCK + tid;
        const int64_t pos = (int64_t)s_base + wcnt[j][wave] + __popcll(ball[j] & lt);
        a.dkey[pos] = dense_key_of(a.map, a.code0 + (uint32_t)i);
        a.dkey[a.dstride + pos] = 0;
        if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = cnt[j];
        if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = cnt[j];
        if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(hi[j]);
        if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong(lo[j]);
        else if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(fsum2(hi[j], lo[j]));
    }
}

// Adds up the `splits` partial tables of every final partition (dpart_final_kernel<.., SPLIT = true>) and writes the groups:
// one workgroup per 512 slots, every thread owns one slot -- no atomics; (sum, lo) pairs are merged with the same TwoSum
// step the accumulation uses, so the result is still the correctly rounded exact sum.
__global__ __launch_bounds__(512) void dpart_merge_kernel(DFinalArgs a, int tbits) {
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int slots = 1 << tbits, chunks = slots / 512;
    const int64_t f = blockIdx.x / chunks;
    const int i = (blockIdx.x % chunks) * 512 + tid;
    if (tid == 0) s_n = 0;
    __syncthreads();
    double hi = -0.0, lo = 0.0;
    uint32_t cnt = 0;
    for (int sp = 0; sp < a.splits; sp++) {
        const size_t at = ((size_t)f * a.splits + sp) * slots + i;
        const uint32_t c = a.part_cnt[at];
        if (c == 0) continue;
        cnt += c;
        const double x = __longlong_as_double((long long)a.part_sum[at]);
        const double t = hi + x;
        lo += two_sum_err(hi, x, t) + (double)a.part_lo[at];
        hi = t;
    }
    if (a.table) {   // DF_TABLE (multi-GPU exchange): the slot itself, occupied or not -- slot = code' of the group
        DTabSlot o;
        o.sum = hi; o.lo = (float)lo; o.cnt = cnt;
        a.table[((size_t)f << tbits) | (size_t)i] = o;
        return;
    }
    const bool occ = cnt != 0;
    pa_block_add(&s_n, occ ? 1u : 0u);
    __syncthreads();
    const uint32_t ngroups = s_n;
    __syncthreads();
    if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
    __syncthreads();
    if ((int64_t)(s_base + ngroups) > a.dstride) {
        if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint64_t b = __ballot(occ);
    uint32_t wbase = 0;
    if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
    wbase = __shfl(wbase, 0);
    if (occ) {
        const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
        const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
        const uint64_t key = dense_key_of(a.map, ((uint32_t)f << tbits) | (uint32_t)i);
        if (a.n_out > 0) {   // result columns (the fused finalisation of dpart_final_kernel<.., DF_COLS>, same expressions)
            const double sum = fsum2(hi, lo);
            for (int c = 0; c < a.n_out; c++) {
                uint64_t cell;
                switch (a.out_kind[c]) {
                    case DF_KEY: cell = df_key_cell(a, c, key); break;
                    case DF_SUM: cell = (uint64_t)__double_as_longlong(sum); break;
                    case DF_AVG: cell = (uint64_t)__double_as_longlong(sum / (double)cnt); break;
                    default: cell = cnt; break;
                }
                df_store_cell(a, c, pos, cell);
            }
            return;
        }
        a.dkey[pos] = key;
        a.dkey[a.dstride + pos] = 0;
        if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = cnt;
        if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = cnt;
        if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(hi);
        if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong(lo);
        else if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(fsum2(hi, lo));
    }
}

// ---- small ranges (at most 2^13 codes): no scatter at all ---------------------------------------------------------------
// Every workgroup keeps the WHOLE direct-addressed table in LDS (slot = key - lo), scans its share of the rows once
// (16 B/row, predicate / expression fused as in pass 1) and writes the table out as one partial; dpart_merge_kernel (one
// "partition", splits = workgroups) adds the partials up.  No hash, no probe chain, no key compare: the LDS scan kernels
// need all three, and stop at ~2400 groups.
struct DScanArgs {
    DenseMap map;         // mul = mul_inv = 1: the slot is the code itself
    const uint64_t* kp;
    const double* vp;
    const double* pp;
    int has_pred, pred_is_v, op;
    double thr;
    int64_t nrows;
    int has_expr;
    ExprProg expr;
    int comp;             // compensated float sums
    uint64_t* part_sum;
    float* part_lo;
    uint32_t* part_cnt;
    unsigned long long* flags;  // [0] failure  [2] entries in the spill buffer
    ulonglong2* spill;
    int64_t spill_cap;
    const VSeg* segs;     // the waiting batches of a stream as ONE launch (round 5): segment i = (kp, vp, pp, nrows); nseg = 0: the columns above
    int nseg;
};

template <int TB>
__global__ __launch_bounds__(TB >= 13 ? 1024 : 512) void dscan_kernel(DScanArgs a) {
    constexpr int SLOTS = 1 << TB, BLOCK = TB >= 13 ? 1024 : 512, U = 4;
    __shared__ uint64_t lsum[SLOTS];
    __shared__ float llo[SLOTS];
    __shared__ uint32_t lcnt[SLOTS];
    __shared__ uint32_t s_bad;
    const int tid = threadIdx.x;
    for (int i = tid; i < SLOTS; i += BLOCK) { lsum[i] = F64_NEG_ZERO; llo[i] = 0.0f; lcnt[i] = 0; }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    auto add = [&](uint64_t key, double x, double p) {
        if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) return;
        const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
        if (d >= (uint64_t)SLOTS) {   // outside the sampled range
            const unsigned long long pos = atomicAdd(&a.flags[2], 1ULL);
            if ((int64_t)pos < a.spill_cap) a.spill[pos] = make_ulonglong2(key, (unsigned long long)__double_as_longlong(x));
            else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const uint32_t slot = (uint32_t)d;
        if (a.comp) {
            const double old = __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const double er = two_sum_err(old, x, old + x);
            if (er != 0.0) {
                const float ef = (float)er;
                if (ef - ef != 0.0f) s_bad = 1;
                __hip_atomic_fetch_add(&llo[slot], ef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else __hip_atomic_fetch_add((double*)&lsum[slot], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        atomicAdd(&lcnt[slot], 1u);
    };
    const VSegConst segs = seg_table(a.segs);
    const int nseg = a.nseg > 0 ? a.nseg : 1;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int sg = 0; sg < nseg; sg++) {   // (every workgroup takes its share of every segment: the stream's batches as one launch)
        const uint64_t* kp = a.nseg > 0 ? segs[sg].kp : a.kp;
        const double* vp = a.nseg > 0 ? (const double*)segs[sg].vp : a.vp;
        const double* pp = a.nseg > 0 ? segs[sg].pp : a.pp;
        const int64_t nrows = a.nseg > 0 ? segs[sg].nrows : a.nrows;
        const int64_t npairs = nrows >> 1;
        for (int64_t q0 = (int64_t)blockIdx.x * BLOCK + tid; q0 < npairs; q0 += stride * U) {
            ulonglong2 kk[U];
            double2 vv[U], pv[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t q = q0 + (int64_t)u * stride;
                if (q < npairs) {
                    const int64_t r = 2 * q;
                    kk[u] = *(const ulonglong2*)(kp + r);
                    vv[u] = a.has_expr ? expr_eval2(a.expr, r) : *(const double2*)(vp + r);
                    if (a.has_pred && !a.pred_is_v) pv[u] = *(const double2*)(pp + r);
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (q0 + (int64_t)u * stride < npairs) {
                    add(kk[u].x, vv[u].x, a.pred_is_v ? vv[u].x : pv[u].x);
                    add(kk[u].y, vv[u].y, a.pred_is_v ? vv[u].y : pv[u].y);
                }
            }
        }
        if ((nrows & 1) && blockIdx.x == 0 && tid == 0) {
            const int64_t r = nrows - 1;
            const double x = a.has_expr ? expr_eval1(a.expr, r) : vp[r];
            add(kp[r], x, a.has_pred ? (a.pred_is_v ? x : pp[r]) : 0.0);
        }
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    uint64_t* ps = a.part_sum + (size_t)blockIdx.x * SLOTS;
    float* pl = a.part_lo + (size_t)blockIdx.x * SLOTS;
    uint32_t* pc = a.part_cnt + (size_t)blockIdx.x * SLOTS;
    for (int i = tid; i < SLOTS; i += BLOCK) { ps[i] = lsum[i]; pl[i] = llo[i]; pc[i] = lcnt[i]; }
}

// ---- any accumulator program over at most one 8-byte input column (dgen_*) --------------------------------------------
// COUNT(*) / COUNT / SUM / AVG of int64 / uint64 / float64, MIN / MAX, DISTINCT: the same code map, scatter passes and
// direct-addressed tables, with the accumulator words of the plan (all 64-bit, as in the LDS tables of the hash path) laid
// out word-major behind a row counter per slot.  The counter is the group's presence flag AND its COUNT(*) word, so a
// COUNT(*)-only program keeps 4 bytes per slot and its entries are the codes alone.
constexpr int DG_MAX_WORDS = 8;
struct DGenArgs {
    DenseMap map;
    int tbits;            // log2 of the slots per table
    // entries (final pass)
    int64_t pstride, rstride;
    const double* vals;
    const void* codes;    // uint16_t remainders
    const uint32_t* counts;
    int64_t cap;
    int regions;
    int64_t nfinal;
    // rows (scan)
    const uint64_t* kp;
    const double* vp;
    const double* pp;
    int has_pred, pred_is_v, op;
    double thr;
    int64_t nrows;
    ulonglong2* spill;
    int64_t spill_cap;
    const uint8_t* vvalid;        // nullable value column (scan, VN): see DPartArgs
    int64_t voff;
    uint64_t* nspill;
    int64_t nspill_cap;
    // program
    int has_val, vtype, comp;
    unsigned long long wpack;     // AccKind -> LDS word (pa_accumulate_col)
    int n_words;                  // accumulator words of the plan
    int n_lds;                    // ... of which live in LDS (every word but the COUNT(*) one)
    int lds_word[AGG_MAX_WORDS];  // plan word -> LDS word, -1 for the COUNT(*) word (taken from the row counter)
    int merge[AGG_MAX_WORDS];     // MergeKind per plan word
    // output
    uint64_t* dkey;
    uint64_t* dacc;
    int64_t dstride;
    unsigned long long* flags;    // [0] failure  [1] dense count  [2] entries in the spill buffer
    // split final pass / scan: partial tables part_w[(work * n_lds + word) * slots + slot], part_cnt[work * slots + slot]
    int splits;
    uint64_t* part_w;
    uint32_t* part_cnt;
};

__device__ __forceinline__ void dgen_init(const DGenArgs& a, uint64_t* lw, uint32_t* lcnt, int slots, int tid, int nthreads) {
    for (int i = tid; i < slots; i += nthreads) lcnt[i] = 0;
    for (int w = 0; w < a.n_words; w++) {
        if (a.lds_word[w] < 0) continue;
        const uint64_t init = merge_init(a.merge[w]);
        uint64_t* dst = lw + (size_t)a.lds_word[w] * slots;
        for (int i = tid; i < slots; i += nthreads) dst[i] = init;
    }
}

// groups of one table -> dense rows (slot order); `f` = final partition (0 for the scan), tables in LDS or merged registers
__device__ __forceinline__ void dgen_write_group(const DGenArgs& a, int64_t pos, uint32_t codep, uint32_t cnt, const uint64_t* words /* [n_lds] */) {
    a.dkey[pos] = dense_key_of(a.map, codep);
    a.dkey[a.dstride + pos] = 0;
    for (int w = 0; w < a.n_words; w++)
        a.dacc[(int64_t)w * a.dstride + pos] = a.lds_word[w] < 0 ? (uint64_t)cnt : words[a.lds_word[w]];
}

// compaction of a block's occupied slots: returns this lane's output row or -1 (all threads of the block must call, ONCE per
// block: *s_n must be 0 on entry)
__device__ __forceinline__ int64_t dgen_claim_rows(const DGenArgs& a, bool occ, uint32_t* s_n, unsigned long long* s_base, int tid) {
    const int lane = tid & 63;
    pa_block_add(s_n, occ ? 1u : 0u);
    __syncthreads();
    const uint32_t ngroups = *s_n;
    __syncthreads();
    if (tid == 0) { *s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); *s_n = 0; }
    __syncthreads();
    if ((int64_t)(*s_base + ngroups) > a.dstride) {
        if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return -2;
    }
    const uint64_t b = __ballot(occ);
    uint32_t wbase = 0;
    if (lane == 0 && b) wbase = atomicAdd(s_n, (uint32_t)__popcll(b));
    wbase = __shfl(wbase, 0);
    const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
    return occ ? (int64_t)*s_base + wbase + __popcll(b & lt) : -1;
}

// Final pass over (value, remainder) entries.  512 threads, dynamic LDS = slots * (8 * n_lds + 4).
template <bool HAS_VAL, bool SPLIT>
__global__ __launch_bounds__(512) void dgen_final_kernel(DGenArgs a) {
    extern __shared__ uint64_t dg_lds[];
    const int slots = 1 << a.tbits;
    uint64_t* lw = dg_lds;                                   // [n_lds][slots]
    uint32_t* lcnt = (uint32_t*)(dg_lds + (size_t)a.n_lds * slots);
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const uint16_t* const codes = (const uint16_t*)a.codes;
    const int64_t nwork = SPLIT ? a.nfinal * a.splits : a.nfinal;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t f = SPLIT ? w / a.splits : w;
        const int sp = SPLIT ? (int)(w % a.splits) : 0;
        const int r0 = SPLIT ? (int)((int64_t)sp * a.regions / a.splits) : 0;
        const int r1 = SPLIT ? (int)((int64_t)(sp + 1) * a.regions / a.splits) : a.regions;
        dgen_init(a, lw, lcnt, slots, tid, 512);
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int rj = r0; rj < r1; rj++) {
            const int64_t region = f * a.pstride + rj * a.rstride;
            const uint32_t n = a.counts[region];
            const double* sv = a.vals + region * a.cap;
            const uint16_t* sc = codes + region * a.cap;
            for (uint32_t i0 = 0; i0 < n; i0 += 512 * 8) {   // pairs of entries per lane, four pairs in flight
                double2 pv[4];
                ushort2 pc[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + 2u * ((uint32_t)u * 512 + tid);
                    if (i < n) {
                        if (HAS_VAL) pv[u] = *(const double2*)(sv + i);
                        pc[u] = *(const ushort2*)(sc + i);
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const int u = q >> 1, el = q & 1;
                    const uint32_t i = i0 + 2u * ((uint32_t)u * 512 + tid) + el;
                    if (i >= n) continue;
                    const uint32_t code = el ? pc[u].y : pc[u].x;
                    const int slot = (int)(code & (slots - 1));
                    atomicAdd(&lcnt[slot], 1u);
                    // (bit 15: the entry's value is NULL -- the row counts for COUNT(*) and makes the group exist)
                    if (HAS_VAL && !(code >> 15)) pa_accumulate_col(a.wpack, a.vtype, lw, slots, slot, (uint64_t)__double_as_longlong(el ? pv[u].y : pv[u].x), a.comp);
                }
            }
        }
        __syncthreads();
        if (SPLIT) {   // this workgroup saw only a share of the partition's entries: the tables go out as they are
            uint32_t* pc = a.part_cnt + (size_t)w * slots;
            for (int i = tid; i < slots; i += 512) pc[i] = lcnt[i];
            uint64_t* pw = a.part_w + (size_t)w * a.n_lds * slots;
            for (int i = tid; i < a.n_lds * slots; i += 512) pw[i] = lw[i];
            __syncthreads();
            continue;
        }
        // groups of this partition -> dense rows, in slot order: one claim for the whole table, then chunk by chunk
        uint32_t mine = 0;
        for (int i = tid; i < slots; i += 512) mine += lcnt[i] != 0 ? 1u : 0u;
        pa_block_add(&s_n, mine);
        __syncthreads();
        const uint32_t ngroups = s_n;
        __syncthreads();
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (int i0 = 0; i0 < slots; i0 += 512) {
            const int i = i0 + tid;
            const bool occ = lcnt[i] != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if ((tid & 63) == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const int lane = tid & 63;
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                uint64_t words[DG_MAX_WORDS];
                for (int k = 0; k < a.n_lds; k++) words[k] = lw[(size_t)k * slots + i];
                dgen_write_group(a, (int64_t)s_base + wbase + __popcll(b & lt), ((uint32_t)f << a.tbits) | (uint32_t)i, lcnt[i], words);
            }
        }
        __syncthreads();
    }
}

// Small ranges: the whole table per workgroup, rows scanned directly (the generic twin of dscan_kernel).  1024 threads.
template <bool HAS_VAL, bool VN = false>
__global__ __launch_bounds__(1024) void dgen_scan_kernel(DGenArgs a) {
    extern __shared__ uint64_t dg_lds[];
    const int slots = 1 << a.tbits;
    uint64_t* lw = dg_lds;
    uint32_t* lcnt = (uint32_t*)(dg_lds + (size_t)a.n_lds * slots);
    const int tid = threadIdx.x;
    constexpr int U = 4;
    dgen_init(a, lw, lcnt, slots, tid, 1024);
    __syncthreads();
    auto add = [&](uint64_t key, double x, double p, bool isnull) {
        if (VN && isnull && a.pred_is_v) return;   // NULL > x is not true
        if (a.has_pred && !cmp_apply<double>(a.op, p, a.thr)) return;
        const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
        if (d >= (uint64_t)slots) {   // outside the sampled range
            if (VN && isnull) {
                const unsigned long long pos = atomicAdd(&a.flags[3], 1ULL);
                if ((int64_t)pos < a.nspill_cap) a.nspill[pos] = key;
                else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            const unsigned long long pos = atomicAdd(&a.flags[2], 1ULL);
            if ((int64_t)pos < a.spill_cap) a.spill[pos] = make_ulonglong2(key, (unsigned long long)__double_as_longlong(x));
            else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        atomicAdd(&lcnt[(int)d], 1u);
        if (HAS_VAL && !(VN && isnull)) pa_accumulate_col(a.wpack, a.vtype, lw, slots, (int)d, (uint64_t)__double_as_longlong(x), a.comp);
    };
    const int64_t npairs = a.nrows >> 1;
    const int64_t stride = (int64_t)gridDim.x * 1024;
    for (int64_t q0 = (int64_t)blockIdx.x * 1024 + tid; q0 < npairs; q0 += stride * U) {
        ulonglong2 kk[U];
        double2 vv[U], pv[U];
        uint32_t vbits = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t q = q0 + (int64_t)u * stride;
            if (q < npairs) {
                const int64_t r = 2 * q;
                kk[u] = *(const ulonglong2*)(a.kp + r);
                if (HAS_VAL) vv[u] = *(const double2*)(a.vp + r);
                if (a.has_pred && !a.pred_is_v) pv[u] = *(const double2*)(a.pp + r);
                if (VN) vbits |= (((uint32_t)a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7)) & 3u) << (2 * u);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (q0 + (int64_t)u * stride < npairs) {
                const double x0 = HAS_VAL ? vv[u].x : 0.0, x1 = HAS_VAL ? vv[u].y : 0.0;
                add(kk[u].x, x0, a.pred_is_v ? x0 : (a.has_pred ? pv[u].x : 0.0), VN && !((vbits >> (2 * u)) & 1u));
                add(kk[u].y, x1, a.pred_is_v ? x1 : (a.has_pred ? pv[u].y : 0.0), VN && !((vbits >> (2 * u + 1)) & 1u));
            }
        }
    }
    if ((a.nrows & 1) && blockIdx.x == 0 && tid == 0) {
        const int64_t r = a.nrows - 1;
        const double x = HAS_VAL ? a.vp[r] : 0.0;
        add(a.kp[r], x, a.has_pred ? (a.pred_is_v ? x : a.pp[r]) : 0.0, VN && !((a.vvalid[(a.voff + r) >> 3] >> ((a.voff + r) & 7)) & 1));
    }
    __syncthreads();
    uint32_t* pc = a.part_cnt + (size_t)blockIdx.x * slots;
    for (int i = tid; i < slots; i += 1024) pc[i] = lcnt[i];
    uint64_t* pw = a.part_w + (size_t)blockIdx.x * a.n_lds * slots;
    for (int i = tid; i < a.n_lds * slots; i += 1024) pw[i] = lw[i];
}

// Adds up the `splits` partial tables of every final partition, word by word with the word's own merge kind (a compensated
// float sum is a (hi, lo) pair of consecutive words: TwoSum on hi, the error joins lo), and writes the groups.
__global__ __launch_bounds__(512) void dgen_merge_kernel(DGenArgs a) {
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int slots = 1 << a.tbits, chunks = slots / 512;
    const int64_t f = blockIdx.x / chunks;
    const int i = (blockIdx.x % chunks) * 512 + tid;
    if (tid == 0) s_n = 0;
    __syncthreads();
    uint64_t acc[DG_MAX_WORDS];
    int mk[DG_MAX_WORDS];
    for (int w = 0; w < a.n_words; w++)
        if (a.lds_word[w] >= 0) { mk[a.lds_word[w]] = a.merge[w]; acc[a.lds_word[w]] = merge_init(a.merge[w]); }
    uint32_t cnt = 0;
    for (int sp = 0; sp < a.splits; sp++) {
        const size_t work = (size_t)f * a.splits + sp;
        const uint32_t c = a.part_cnt[work * slots + i];
        if (c == 0) continue;
        cnt += c;
        const uint64_t* pw = a.part_w + work * a.n_lds * slots + i;
        for (int k = 0; k < a.n_lds; k++) {
            const uint64_t v = pw[(size_t)k * slots];
            switch (mk[k]) {
                case M_ADD_U64: acc[k] += v; break;
                case M_ADD_F64: acc[k] = (uint64_t)__double_as_longlong(__longlong_as_double((long long)acc[k]) + __longlong_as_double((long long)v)); break;
                case M_ADD_F64C: {   // the error of this add joins the NEXT word (its own partial is added when k gets there)
                    const double hi = __longlong_as_double((long long)acc[k]), x = __longlong_as_double((long long)v), t = hi + x;
                    acc[k] = (uint64_t)__double_as_longlong(t);
                    acc[k + 1] = (uint64_t)__double_as_longlong(__longlong_as_double((long long)acc[k + 1]) + two_sum_err(hi, x, t));
                    break;
                }
                case M_MIN_U64: acc[k] = v < acc[k] ? v : acc[k]; break;
                default: acc[k] = v > acc[k] ? v : acc[k]; break;
            }
        }
    }
    const bool occ = cnt != 0;
    const int64_t pos = dgen_claim_rows(a, occ, &s_n, &s_base, tid);
    if (pos >= 0) dgen_write_group(a, pos, ((uint32_t)f << a.tbits) | (uint32_t)i, cnt, acc);
}

// ---- COUNT(*)-only programs over MANY groups: one scatter level, one-byte counters (round 5, VERDICT r04 #8) ---------------------
// `SELECT k, count(*) GROUP BY k` at G = 1e8 took the two scatter levels of every dense program although its entries are bare codes:
// pass 2 (1e9 four-byte entries in, two-byte entries out) is bound by its LDS atomics, 3.4 ms of the query's 7.4.  A group of such a
// query holds a handful of rows, so its counter fits a BYTE and a table of 2^17 codes fits 128 KB of LDS: after ONE scatter level
// (512 partitions of 2^14 .. 2^18 codes each) a work item = (partition, sub-range of at most 2^17 codes) streams the partition's
// regions (one wave per region, 16-byte loads), adds 1 << 8 * (code & 3) to word code >> 2 for the codes of its sub-range -- a
// partition with more than 2^17 codes is read once per sub-range -- and writes its groups in ascending code like every final pass.
// The adds RETURN the old word: a byte that stood at 255 would carry into its neighbour, so the lane that sees that raises flags[5]
// (and flags[0]): the host runs the batch through the two-level path instead and never tries this one again for the operator.
// While no lane sees 255, no carry has happened and every byte is exact.
// CB = 16: the same with two-byte counters (2^16 codes per 128 KB table) for groups of up to a few thousand rows -- between the ranges the
// ordinary one-level geometry covers (2^22 codes) and the group sizes bytes hold, COUNT(*) over 5e6 groups of 200 rows each took two
// levels of 32 / 64 rings that overflow when every row survives: 10.4 ms, against 4.0 at 2e6 and at 1e7 groups.
constexpr int DC8_BITS = 17;      // the largest table: 2^17 one-byte counters (2^16 two-byte ones)
template <int CB>
__global__ __launch_bounds__(1024) void dcount8_final_kernel(DGenArgs a, int sub_bits) {
    extern __shared__ uint32_t dc_tab[];     // 2^tbits counters of CB bits
    constexpr int PER = 32 / CB, PSH = CB == 8 ? 2 : 1;       // counters per word
    constexpr uint32_t CMASK = CB == 8 ? 0xFFu : 0xFFFFu;
    const int tb8 = a.tbits;
    __shared__ uint32_t s_n, s_over;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* const codes = (const uint32_t*)a.codes;
    const int64_t nwork = a.nfinal << sub_bits;
    const uint32_t submask = (1u << sub_bits) - 1u;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t p = w >> sub_bits;
        const uint32_t sub = (uint32_t)w & submask;
        for (int i = tid; i < (1 << (tb8 - PSH)); i += 1024) dc_tab[i] = 0;
        if (tid == 0) { s_n = 0; s_over = 0; }
        __syncthreads();
        bool over = false;
        for (int rj = wave; rj < a.regions; rj += 16) {
            const int64_t region = p * a.pstride + rj * a.rstride;
            const uint32_t n = a.counts[region];
            const uint32_t* sc = codes + region * a.cap;
            for (uint32_t i0 = 0; i0 < n; i0 += 64 * 4 * 2) {   // two 16-byte loads per lane in flight (region capacities are multiples of 16 entries)
                uint4 q[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t i = i0 + ((uint32_t)u * 64 + lane) * 4;
                    if (i < n) q[u] = *(const uint4*)(sc + i);
                }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t i = i0 + ((uint32_t)u * 64 + lane) * 4;
                    const uint32_t c4[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (i + k >= n) continue;
                        const uint32_t code = c4[k];
                        if ((code >> tb8) != sub) continue;
                        const uint32_t b = code & ((1u << tb8) - 1u), sh = (b & (uint32_t)(PER - 1)) * (uint32_t)CB;
                        const uint32_t old = atomicAdd(&dc_tab[b >> PSH], 1u << sh);
                        over |= ((old >> sh) & CMASK) == CMASK;
                    }
                }
            }
        }
        if (over) s_over = 1;
        __syncthreads();
        if (s_over) {   // a group with 256 rows or more: not this kernel's case
            if (tid == 0) { __hip_atomic_store(&a.flags[5], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            return;
        }
        // groups of this sub-range -> dense rows in ascending code: one claim for the table, then 1024 codes at a time
        uint32_t mine = 0;
        for (int i = tid; i < (1 << (tb8 - PSH)); i += 1024) {
            const uint32_t x = dc_tab[i];
            if (CB == 8) mine += ((x & 0xffu) != 0) + ((x & 0xff00u) != 0) + ((x & 0xff0000u) != 0) + ((x >> 24) != 0);
            else mine += ((x & 0xffffu) != 0) + ((x >> 16) != 0);
        }
        pa_block_add(&s_n, mine);
        __syncthreads();
        const uint32_t ngroups = s_n;
        __syncthreads();
        if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
        __syncthreads();
        if ((int64_t)(s_base + ngroups) > a.dstride) {
            if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const uint32_t prefix = ((uint32_t)p << (tb8 + sub_bits)) | (sub << tb8);
        for (int i0 = 0; i0 < (1 << tb8); i0 += 1024) {
            const int i = i0 + tid;
            const uint32_t cnt = (dc_tab[i >> PSH] >> ((i & (PER - 1)) * CB)) & CMASK;
            const bool occ = cnt != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                dgen_write_group(a, (int64_t)s_base + wbase + __popcll(b & lt), prefix | (uint32_t)i, cnt, nullptr);
            }
        }
        __syncthreads();
    }
}

// ---- a STREAM of batches over a small dense range (dscan_kernel per batch) ----------------------------------------------------
// The per-workgroup partial tables of a batch are added into ONE table that lives across the batches of the stream (sum, lo as
// float64, 64-bit counts) -- every thread owns one slot, no atomics -- and the groups are written once, when something else needs
// them.  (Before: a merge kernel + a run + that run folded into the HBM hash table per batch, 285 us per 2^24-row batch at
// G = 1000 against 60 us for the scan itself.)
struct DScanTable {
    double* sum;
    double* lo;
    unsigned long long* cnt;
};
// 64 slots per workgroup x 8 thread groups that share the partial tables between them (group g takes tables g, g + 8, ...: four
// independent loads in flight per thread), combined through LDS -- one thread per slot over all 256 tables took 150 us (16
// workgroups, 256 dependent-latency rounds), more than the scan of the batch itself (60 us).
__global__ __launch_bounds__(512) void dscan_accumulate_kernel(const uint64_t* part_sum, const float* part_lo, const uint32_t* part_cnt,
                                                                int splits, int slots, DScanTable t) {
    __shared__ double s_hi[8][64], s_lo[8][64];
    __shared__ unsigned long long s_cnt[8][64];
    const int li = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + li;
    double hi = -0.0, lo = 0.0;
    unsigned long long cnt = 0;
    constexpr int U = 4;
    for (int sp0 = g; sp0 < splits; sp0 += 8 * U) {
        uint32_t c[U]; uint64_t xs[U]; float xl[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int sp = sp0 + 8 * u;
            c[u] = 0; xs[u] = 0; xl[u] = 0.0f;
            if (sp < splits && i < slots) {
                const size_t at = (size_t)sp * slots + i;
                c[u] = part_cnt[at]; xs[u] = part_sum[at]; xl[u] = part_lo[at];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (c[u] == 0) continue;
            cnt += c[u];
            const double x = __longlong_as_double((long long)xs[u]);
            const double s = hi + x;
            lo += two_sum_err(hi, x, s) + (double)xl[u];
            hi = s;
        }
    }
    s_hi[g][li] = hi; s_lo[g][li] = lo; s_cnt[g][li] = cnt;
    __syncthreads();
    if (g != 0 || i >= slots) return;
    for (int gg = 1; gg < 8; gg++) {
        const unsigned long long c = s_cnt[gg][li];
        if (c == 0) continue;
        cnt += c;
        const double x = s_hi[gg][li];
        const double s = hi + x;
        lo += two_sum_err(hi, x, s) + s_lo[gg][li];
        hi = s;
    }
    if (cnt == 0) return;
    const double old = t.sum[i], s = old + hi;
    t.lo[i] += two_sum_err(old, hi, s) + lo;
    t.sum[i] = s;
    t.cnt[i] += cnt;
}
// the stream's table -> groups of a run (same words as dpart_merge_kernel writes)
__global__ __launch_bounds__(512) void dscan_emit_kernel(DFinalArgs a, int slots, DScanTable t) {
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * 512 + tid;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const unsigned long long cnt = i < slots ? t.cnt[i] : 0ULL;
    const bool occ = cnt != 0;
    pa_block_add(&s_n, occ ? 1u : 0u);
    __syncthreads();
    const uint32_t ngroups = s_n;
    __syncthreads();
    if (tid == 0) { s_base = atomicAdd(&a.flags[1], (unsigned long long)ngroups); s_n = 0; }
    __syncthreads();
    if ((int64_t)(s_base + ngroups) > a.dstride) {
        if (tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint64_t b = __ballot(occ);
    uint32_t wbase = 0;
    if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
    wbase = __shfl(wbase, 0);
    if (occ) {
        const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
        const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
        const double hi = t.sum[i], lo = t.lo[i];
        a.dkey[pos] = dense_key_of(a.map, (uint32_t)i);
        a.dkey[a.dstride + pos] = 0;
        if (a.w_rows >= 0) a.dacc[(int64_t)a.w_rows * a.dstride + pos] = cnt;
        if (a.w_valid >= 0) a.dacc[(int64_t)a.w_valid * a.dstride + pos] = cnt;
        if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(hi);
        if (a.w_lo >= 0) a.dacc[(int64_t)a.w_lo * a.dstride + pos] = (uint64_t)__double_as_longlong(lo);
        else if (a.w_sum >= 0) a.dacc[(int64_t)a.w_sum * a.dstride + pos] = (uint64_t)__double_as_longlong(fsum2(hi, lo));
    }
}

// exact_track statistics of a strided sample of a float64 column (fixed-point entries: which quantum? -- dense_partitioned_aggregate)
// order-preserving unsigned image of a float64 (never 0 for a number; -0.0 < +0.0), and back
__host__ __device__ __forceinline__ unsigned long long f64_ordered(double v) {
    unsigned long long b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : b | 0x8000000000000000ULL;
}
__host__ __device__ __forceinline__ double f64_of_ordered(unsigned long long u) {
    const unsigned long long b = (u >> 63) ? u & 0x7FFFFFFFFFFFFFFFULL : ~u;
    double v;
    memcpy(&v, &b, 8);
    return v;
}
// (mm, optional: mm[0] = max of the complemented images = the smallest sampled value, mm[1] = the largest; both start at 0)
__global__ __launch_bounds__(256) void fx_sample_kernel(const double* vals, int64_t nrows, int64_t m, unsigned long long* out, unsigned long long* mm = nullptr) {
    __shared__ uint32_t sx[2];
    __shared__ unsigned long long smm[2];
    if (threadIdx.x < 2) { sx[threadIdx.x] = 0; smm[threadIdx.x] = 0; }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t xinv = 0, xexp = 0;
    unsigned long long nmin = 0, vmax = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const double v = vals[(int64_t)(((__int128)i * nrows) / m)];
        exact_track(v, xinv, xexp);
        const unsigned long long u = f64_ordered(v);
        nmin = ~u > nmin ? ~u : nmin;
        vmax = u > vmax ? u : vmax;
    }
    if (xinv) atomicMax(&sx[0], xinv);
    if (xexp) atomicMax(&sx[1], xexp);
    if (mm && vmax) { atomicMax(&smm[0], nmin); atomicMax(&smm[1], vmax); }
    __syncthreads();
    if (threadIdx.x < 2 && sx[threadIdx.x]) atomicMax((uint32_t*)out + threadIdx.x, sx[threadIdx.x]);
    if (mm && threadIdx.x < 2 && smm[threadIdx.x]) atomicMax(&mm[threadIdx.x], smm[threadIdx.x]);
}

// min / max of the order-preserving unsigned images of a strided sample of the keys: out[0] = min, out[1] = max.
// One atomic pair per WORKGROUP (a pair per wave -- 8192 same-address atomics -- made this 100 us kernel 90 us slower).
__global__ __launch_bounds__(256) void dense_sample_range_kernel(const uint64_t* keys, int64_t nrows, int64_t m, uint64_t sign,
                                                                 unsigned long long* out, const uint8_t* kvalid, int64_t koff) {
    __shared__ unsigned long long smn[4], smx[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t mn = ~0ULL, mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int64_t row = (int64_t)(((__int128)i * nrows) / m);
        if (!key_row_valid(kvalid, koff, row)) continue;   // (a NULL key's value word is garbage)
        const uint64_t ku = keys[row] ^ sign;
        mn = ku < mn ? ku : mn;
        mx = ku > mx ? ku : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t omn = __shfl_xor(mn, o), omx = __shfl_xor(mx, o);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) { mn = smn[w] < mn ? smn[w] : mn; mx = smx[w] > mx ? smx[w] : mx; }
        atomicMin(&out[0], (unsigned long long)mn);
        atomicMax(&out[1], (unsigned long long)mx);
    }
}
