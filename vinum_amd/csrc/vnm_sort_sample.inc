// Sample sort for one 8-byte key (included by vnm_sort.hip inside namespace vnm) -- Sort::Sorted, sort.cpp:15-63, over 1e9 rows.
//
// The LSD radix sort moves every (code, row id) pair once per 8-bit digit: eight passes of 24 bytes per row plus the encode
// pass, 208 GB per 1e9 keys, 52 ms.  Here the rows are brought NEAR their final place first and sorted inside LDS:
//   1. a strided sample of 2^23 keys is sorted (the existing radix sort, ~1 ms) and every 32nd sample is a SPLITTER: 2^18 buckets of
//      ~3800 rows each (+- 18 %), as 512 level-1 buckets x 512 sub-buckets;
//   2. two scatter passes (ssort_scatter_kernel) move 12-byte entries (code 8 + row id 4) into their bucket: the bucket of a
//      row is a 9-step binary search over 512 splitters in LDS; the entries travel through per-partition RINGS in LDS and
//      leave them in whole 8-entry blocks (64 bytes of codes, 32 of row ids: full aligned sectors), the write-combining of the
//      dense group-by path (vnm_agg_dense.inc);
//   3. one workgroup per bucket (ssort_local_kernel) loads its <= 8192 entries, orders them ENTIRELY in LDS -- interpolation
//      slots + a rank by (code, row id) inside each slot; stable 8-bit counting passes when a slot is crowded (the scatter passes do
//      not keep the row order; equal codes always share a bucket and a slot) -- and writes the int64 row ids and, for a key
//      without NaN / -0.0, the sorted key values rebuilt from the codes, to their final positions.
// Traffic: 8 + 12 | 12 + 12 | 12 + 8 (+ 8) = 64-72 GB.  Any bucket that outgrows its region or the LDS (heavily duplicated keys:
// equal splitters) fails the attempt and the caller runs the LSD sort: results are identical either way (the order is total:
// code, then row id).
constexpr int SS_B = 512;          // fan-out of each scatter level
constexpr int SS_FB = 8;           // entries per flushed ring block
constexpr int SS_CAP = 24;         // ring entries per partition (144 KB of LDS)
constexpr int SS_BLOCK = 1024;
constexpr int SS_LOCAL = 8192;     // entries a final bucket may hold
constexpr int SS_MAX_REGIONS = 256;
constexpr uint64_t SS_NAN_CODE = ~0ULL;   // NaN sorts after every number in both directions (no real key encodes to all ones)

struct SsArgs {
    vnm_dcol key; int desc; int64_t nrows;                     // level 1 input
    const uint64_t* in_code; const uint32_t* in_row; const uint32_t* in_counts; int64_t in_cap; int in_regions, in_split;   // level 2 input
    const uint64_t* split;                                     // [SS_B * l2] bucket lower bounds (split[0] unused: -inf)
    int l2;                                                    // fan-out of the second level (8 .. SS_B): buckets of ~2000-4200 rows whatever n
    uint64_t* out_code; uint32_t* out_row; uint32_t* out_counts; int64_t out_cap;
    unsigned long long* flags;                                 // [0] failure  [1] bit 0: a NaN key, bit 1: a -0.0 key  [2] side-list length
    // HEAVY codes (a value holding a bucket's worth of rows or more: equal neighbouring splitters): their rows bypass the buckets.
    // Level 1 appends (heavy index << 32 | row id) to `side`; sorted, that list IS their part of the output (ssort_heavy_*).
    const uint64_t* heavy; int nheavy;                         // ascending codes, at most SS_MAX_HEAVY
    int has_null;                                              // the key has a validity bitmap: NULL rows travel as heavy class `nheavy` (after everything)
    unsigned long long* side; int64_t side_cap;
};
constexpr int SS_MAX_HEAVY = 64;

__device__ __forceinline__ uint64_t ss_encode(int type, uint64_t raw, int desc, unsigned* special) {
    if (type == VNM_F64) {
        double d = __longlong_as_double((long long)raw);
        if (d != d) { *special |= 1u; return SS_NAN_CODE; }
        if (d == 0.0) { if (raw != 0) *special |= 2u; d = 0.0; }   // -0.0 sorts as +0.0 (Arrow's comparison): ties keep the row order
        const uint64_t e = enc_f64(d);
        return desc ? ~e : e;
    }
    const uint64_t e = type == VNM_U64 ? raw : enc_i64((int64_t)raw);
    return desc ? ~e : e;
}
__device__ __forceinline__ uint64_t ss_code_of(const vnm_dcol& c, int64_t row, int desc, unsigned* special) {
    return ss_encode(c.type, ((const uint64_t*)c.values)[c.offset + row], desc, special);
}

// largest j in [0, SS_B) with sp[j] <= code; sp[0] counts as -infinity
__device__ __forceinline__ int ss_bucket(const uint64_t* sp, uint64_t code) {
    int lo = 0;
#pragma unroll
    for (int step = SS_B / 2; step > 0; step >>= 1)
        if (sp[lo + step] <= code) lo += step;
    return lo;
}
// The same through a table over SS_LUT equal-width cells of the code range [sp[1], sp[SS_B - 1]]: lut[c] = bucket of the cell's
// lower edge, so the answer lies in [lut[c], lut[c + 1]] -- usually one or two candidates where nine dependent LDS reads of a
// binary search stood (PMC: the LDS was busy 55 % of the scatter passes' time, a third of that in bank conflicts of those
// reads).  Any distribution is still answered correctly: a cell that spans many buckets is searched by bisection.
constexpr int SS_LUT = 2048;
__device__ __forceinline__ int ss_bucket_lut(const uint64_t* sp, const uint16_t* lut, uint64_t base, int shift, uint64_t code) {
    if (code < base) return 0;
    uint64_t cell = (code - base) >> shift;
    if (cell > (uint64_t)(SS_LUT - 1)) cell = SS_LUT - 1;
    int lo = lut[cell], hi = lut[cell + 1];
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sp[mid] <= code) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool FROM_KEYS, int SP>
__global__ __launch_bounds__(SS_BLOCK) void ssort_scatter_kernel(SsArgs a) {
    constexpr int NE = 2 * SP;   // entries per lane and sub-tile
    extern __shared__ uint64_t ss_lds[];
    uint64_t* const rv = ss_lds;                                   // [SS_B][SS_CAP] codes
    uint32_t* const rc = (uint32_t*)(ss_lds + SS_B * SS_CAP);       // [SS_B][SS_CAP] row ids
    __shared__ uint64_t sp[SS_B];
    __shared__ uint16_t lut[SS_LUT + 2];
    __shared__ uint32_t fill[SS_B], cursor[SS_B], s_retry[2], s_nready[2];
    __shared__ uint16_t head[SS_B], ready[SS_B];   // (16-bit heads: the kernel sits 1 KB below the 160 KB of LDS)
    const RingState<uint16_t> rs{fill, head, cursor, s_retry, s_nready, ready};
    __shared__ uint32_t s_hcnt[2];
    __shared__ unsigned long long s_hbase;
    __shared__ uint64_t aux64[(SS_MAX_REGIONS + 2) / 2 + 1];   // level 2: region starts (uint32); level 1: the heavy codes
    uint32_t* const rstart = (uint32_t*)aux64;
    uint64_t* const hv = aux64;
    const int tid = threadIdx.x;
    int64_t out_base, out_stride;
    int pin = 0;
    if (FROM_KEYS) { out_base = blockIdx.x; out_stride = gridDim.x; }
    else {
        pin = blockIdx.x / a.in_split;
        const int g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * a.l2 * a.in_split + g; out_stride = a.in_split;
    }
    ring_init<SS_BLOCK, SS_B>(rs);
    // (level 2 with fewer than SS_B partitions: the rest get an unreachable lower bound)
    for (int i = tid; i < SS_B; i += SS_BLOCK) sp[i] = FROM_KEYS ? a.split[(size_t)i * a.l2] : (i < a.l2 ? a.split[(size_t)pin * a.l2 + i] : ~0ULL);
    if (tid < 2) s_hcnt[tid] = 0;
    int ph = 0;
    if (FROM_KEYS && tid < a.nheavy) hv[tid] = a.heavy[tid];
    __syncthreads();
    const uint64_t lut_base = sp[1];
    int lut_shift = 0;
    const int np = FROM_KEYS ? SS_B : a.l2;
    while (lut_shift < 63 && ((sp[np - 1] - lut_base) >> lut_shift) >= (uint64_t)SS_LUT) lut_shift++;
    for (int i = tid; i <= SS_LUT; i += SS_BLOCK)
        lut[i] = i == SS_LUT ? (uint16_t)(np - 1) : (uint16_t)min(ss_bucket(sp, lut_base + ((uint64_t)i << lut_shift)), np - 1);
    __syncthreads();
    const uint32_t ocap = (uint32_t)a.out_cap;

    // four lanes per partition, lane j moves entries 2j, 2j + 1 of a block (16 bytes of codes, 8 of row ids).  A full region fails
    // the sort (flags[0]); its count runs on, capped at out_cap.  Every pass lists its ready rings.
    auto flush = [&](bool drain) {
        ring_flush<SS_FB, 4, SS_BLOCK, true>(rs, ph, drain, true, np, SS_CAP, ocap, [&](int p, uint32_t src, int64_t dst, uint32_t n_here, int j, bool room) {
            if (!room) { if (j == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            else if ((uint32_t)(2 * j) < n_here) {
                const int li = p * SS_CAP + (int)src + 2 * j;
                const int64_t at = (out_base + (int64_t)p * out_stride) * a.out_cap + dst + 2 * j;
                *(ulonglong2*)(a.out_code + at) = *(const ulonglong2*)(rv + li);
                *(uint2*)(a.out_row + at) = *(const uint2*)(rc + li);
            }
        });
    };
    int hp = 0;
    auto rounds = [&](const uint64_t (&c)[NE], const uint32_t (&r)[NE], uint32_t okmask) {
        ring_rounds<NE>(rs, ph, okmask, [&](int e) -> bool {
            const int p = min(ss_bucket_lut(sp, lut, lut_base, lut_shift, c[e]), np - 1);   // (the all-ones code meets the unreachable bounds)
            const uint32_t slot = ring_reserve<SS_FB>(rs, ph, (uint32_t)p, SS_CAP, true);
            if (slot != RING_FULL) { rv[p * SS_CAP + slot] = c[e]; rc[p * SS_CAP + slot] = r[e]; }
            return slot != RING_FULL;
        }, [&]() { flush(false); }, [](int, uint32_t) { return false; });
    };

    if (FROM_KEYS) {
        // sub-tiles of NE * 1024 rows (16-byte loads); the next sub-tile of the workgroup is in flight during the rounds
        const int64_t sub = (int64_t)NE * SS_BLOCK;
        const int64_t nsub = (a.nrows + sub - 1) / sub, nfull = a.nrows / sub;
        const bool aligned = (a.key.offset & 1) == 0;
        unsigned special = 0;
        ulonglong2 kk[SP];
        auto load_sub = [&](int64_t st) {
            if (st < nfull && aligned) {
#pragma unroll
                for (int u = 0; u < SP; u++) kk[u] = *(const ulonglong2*)((const uint64_t*)a.key.values + a.key.offset + st * sub + (int64_t)u * 2 * SS_BLOCK + 2 * tid);
            }
        };
        load_sub(blockIdx.x);
        for (int64_t st = blockIdx.x; st < nsub; st += gridDim.x) {
            uint64_t c[NE]; uint32_t rr[NE]; uint32_t okmask = 0;
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const int u = e >> 1, el = e & 1;
                const int64_t r = st * sub + (int64_t)u * 2 * SS_BLOCK + 2 * tid + el;
                c[e] = 0; rr[e] = (uint32_t)r;
                if (r < a.nrows) {
                    okmask |= 1u << e;
                    if (st < nfull && aligned) c[e] = ss_encode(a.key.type, el ? kk[u].y : kk[u].x, a.desc, &special);
                    else c[e] = ss_code_of(a.key, r, a.desc, &special);
                }
            }
            load_sub(st + gridDim.x);
            if (a.nheavy || a.has_null) {   // rows of a heavy code (and NULL rows: class nheavy) go to the side list
                int hidx[NE];
                okmask &= ~ring_side_list<NE>(s_hcnt, s_hbase, hp, &a.flags[2], [&](int e) -> bool {
                    int lo = 0, hi = a.nheavy - 1, hit = -1;
                    if ((okmask >> e) & 1u) {
                        const int64_t vr = a.key.offset + (int64_t)rr[e];
                        if (a.has_null && !((a.key.validity[vr >> 3] >> (vr & 7)) & 1)) hit = a.nheavy;
                        else
                        while (lo <= hi) { const int mid = (lo + hi) >> 1; const uint64_t x = hv[mid]; if (x == c[e]) { hit = mid; break; } if (x < c[e]) lo = mid + 1; else hi = mid - 1; }
                    }
                    hidx[e] = hit;
                    return hit >= 0;
                }, [&](int e, unsigned long long pos) {
                    if ((int64_t)pos < a.side_cap) a.side[pos] = ((unsigned long long)hidx[e] << 32) | rr[e];
                    else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                });
            }
            rounds(c, rr, okmask);
        }
        if (special) atomicOr(&a.flags[1], (unsigned long long)special);
    } else {
        const RingRegions rg2 = ring_regions<2>(rstart, a.in_counts, a.in_regions, a.in_split, a.in_regions, 1);   // pairs of entries
        const uint32_t total_in = rg2.total;
        ulonglong2 ec[SP];
        uint2 er[SP];
        uint32_t okm = 0;
        int reg = 0;
        auto load_pairs = [&](uint32_t t0) {
            okm = 0;
#pragma unroll
            for (int u = 0; u < SP; u++) {
                const uint32_t v = t0 + (uint32_t)u * SS_BLOCK + tid;
                if (v < total_in) {
                    uint32_t e0;
                    const int64_t rg = rg2.region0 + ring_region_of<2>(rstart, reg, v, &e0);
                    const int64_t at = rg * a.in_cap + e0;
                    ec[u] = *(const ulonglong2*)(a.in_code + at);
                    er[u] = *(const uint2*)(a.in_row + at);
                    okm |= (e0 + 1 < a.in_counts[rg] ? 3u : 1u) << (2 * u);
                }
            }
        };
        load_pairs(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += SP * SS_BLOCK) {
            uint64_t c[NE]; uint32_t rr[NE];
#pragma unroll
            for (int u = 0; u < SP; u++) { c[2 * u] = ec[u].x; c[2 * u + 1] = ec[u].y; rr[2 * u] = er[u].x; rr[2 * u + 1] = er[u].y; }
            const uint32_t okmask = okm;
            load_pairs(t0 + SP * SS_BLOCK);
            rounds(c, rr, okmask);
        }
    }
    flush(true);
    __syncthreads();
    for (int i = tid; i < np; i += SS_BLOCK) a.out_counts[out_base + (int64_t)i * out_stride] = cursor[i];
}

// Are the rows CLUSTERED in arrival order (an already sorted / reverse sorted / run-wise sorted column)?  A sub-tile of the scatter passes is
// 2048-4096 consecutive rows; when they all belong to a sliver of the distribution they all go to the same few rings (24-32 entries each) and
// the sub-tile takes hundreds of insert / flush rounds: 1e9 sorted keys would take ~250 ms where the LSD passes take 52.  64 tiles of 4096
// consecutive rows, spread over the column: the SPAN of a tile = the share of the sorted sample between the tile's smallest and largest code
// (~1 for rows in random order); the smallest span is handed back (in samples).
__global__ __launch_bounds__(256) void ssort_cluster_kernel(vnm_dcol key, int desc, int64_t n, const uint64_t* S, int64_t m, unsigned long long* out_min_span) {
    __shared__ unsigned long long s_mn[4], s_mx[4];
    constexpr int64_t TILE = 4096;
    const int64_t ntiles = n / TILE;
    if (ntiles < 1) return;
    const int64_t t = (int64_t)(((__int128)blockIdx.x * ntiles) / gridDim.x);
    unsigned special = 0;
    uint64_t mn = ~0ULL, mx = 0;
    for (int i = threadIdx.x; i < TILE; i += 256) {
        const uint64_t c = ss_code_of(key, t * TILE + i, desc, &special);
        if (c == SS_NAN_CODE) continue;
        mn = c < mn ? c : mn; mx = c > mx ? c : mx;
    }
    for (int o = 32; o > 0; o >>= 1) { const uint64_t a = __shfl_xor(mn, o), b = __shfl_xor(mx, o); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) { mn = s_mn[w] < mn ? s_mn[w] : mn; mx = s_mx[w] > mx ? s_mx[w] : mx; }
        if (mn > mx) return;   // (a tile of NaNs)
        auto rank_of = [&](uint64_t c) -> int64_t { int64_t lo = 0, hi = m; while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (S[mid] < c) lo = mid + 1; else hi = mid; } return lo; };
        const int64_t span = rank_of(mx) - rank_of(mn);
        atomicMin(out_min_span, (unsigned long long)(span < 0 ? 0 : span));
    }
}

// splitters: split[b] = sorted sample[b * m / nb]  (b >= 1)
// Equal neighbouring splitters = a code that holds a bucket's worth of rows or more (a popular value, NaNs): a HEAVY code.  The
// first splitter of every such run is appended to heavy[] (unordered; the host sorts the few of them); more than SS_MAX_HEAVY
// raise flags[0] (such data is the LSD sort's home ground: few distinct digits).
__global__ void ssort_splitters_kernel(const uint64_t* sorted, int64_t m, int64_t nb, uint64_t* split, unsigned long long* flags,
                                       uint64_t* heavy, unsigned int* nheavy) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    auto at = [&](int64_t j) -> uint64_t { return sorted[(int64_t)(((__int128)j * m) / nb)]; };
    const uint64_t mine = b == 0 ? 0 : at(b);
    split[b] = mine;
    if (b >= 1 && b + 1 < nb && mine == at(b + 1)) atomicAdd(&flags[3], 1ULL);     // (sizes the side list)
    if (b >= 1 && b + 1 < nb && mine == at(b + 1) && (b == 1 || at(b - 1) != mine)) {
        const unsigned int k = atomicAdd(nheavy, 1u);
        if (k < (unsigned int)SS_MAX_HEAVY) heavy[k] = mine;
        else __hip_atomic_store(&flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Heavy codes after their rows were collected and the side list sorted (entries: heavy index << 32 | row id): lb[i] = first
// entry of heavy i (lb[nheavy] = length), hb[i] = the bucket a row of that code would have gone to (largest j with split[j] <= code).
__global__ void ssort_heavy_bounds_kernel(const unsigned long long* side, int64_t len, const uint64_t* heavy, int nheavy, const uint64_t* split,
                                          int64_t nb, unsigned long long* lb, unsigned int* hb, int has_null) {
    const int i = threadIdx.x;
    if (i > nheavy + has_null) return;     // (with NULL rows: lb[nheavy] = their first entry, lb[nheavy + 1] = the length)
    int64_t lo = 0, hi = len;
    const unsigned long long key = (unsigned long long)i << 32;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (side[mid] < key) lo = mid + 1; else hi = mid; }
    lb[i] = (unsigned long long)lo;
    if (i < nheavy) {
        int64_t a = 0, b = nb - 1;   // split[0] = -inf
        while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (split[mid] <= heavy[i]) a = mid; else b = mid - 1; }
        hb[i] = (unsigned int)a;
    }
}

// the heavy rows' part of the output: entry q of the sorted side list is row q - lb[i] of heavy code i's block
__global__ void ssort_heavy_write_kernel(const unsigned long long* side, int64_t len, const uint64_t* heavy, const unsigned long long* lb,
                                         const unsigned long long* hstart, int64_t* idx_out, uint64_t* key_out, int key_type, int key_desc, int nheavy) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < len; q += stride) {
        const unsigned long long e = side[q];
        const int i = (int)(e >> 32);
        const unsigned long long pos = hstart[i] + ((unsigned long long)q - lb[i]);
        idx_out[pos] = (int64_t)(e & 0xFFFFFFFFULL);
        if (key_out && i < nheavy) {
            const uint64_t en = key_desc ? ~heavy[i] : heavy[i];
            key_out[pos] = key_type == VNM_F64 ? (uint64_t)__double_as_longlong(dec_f64(en)) : (key_type == VNM_I64 ? (uint64_t)dec_i64(en) : en);
        }
    }
}

// NULL rows of the key, exactly (the side list is sized from it; the sample's share can be far off for periodic patterns)
__global__ __launch_bounds__(256) void ssort_count_nulls_kernel(const uint8_t* valid, int64_t first, int64_t n, unsigned long long* out) {
    __shared__ unsigned long long s_sum[256];
    const int64_t nbytes = (first + n + 7) / 8 - first / 8;
    const uint8_t* p = valid + first / 8;
    const int lead = (int)(first & 7), tail = (int)((first + n) & 7);
    unsigned long long zeros = 0;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes; b += (int64_t)gridDim.x * blockDim.x) {
        unsigned int v = p[b], care = 0xFFu;
        if (b == 0) care &= 0xFFu << lead;
        if (b == nbytes - 1 && tail) care &= 0xFFu >> (8 - tail);
        zeros += (unsigned long long)__popc(~v & care);
    }
    s_sum[threadIdx.x] = zeros;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0 && s_sum[0]) atomicAdd(out, s_sum[0]);
}

// strided sample of the key, encoded; NULL rows give the all-ones code and are counted (after the sort they stand at the end: the
// splitters come from the samples in front of them)
__global__ __launch_bounds__(256) void ssort_sample_kernel(vnm_dcol c, int desc, int64_t n, int64_t m, uint64_t* code, unsigned long long* nulls) {
    __shared__ unsigned int s_nulls;
    if (threadIdx.x == 0) s_nulls = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned special = 0;
    unsigned int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int64_t row = (int64_t)(((__int128)i * n) / m);
        const int64_t vr = c.offset + row;
        if (c.validity && !((c.validity[vr >> 3] >> (vr & 7)) & 1)) { code[i] = ~0ULL; mine++; }
        else code[i] = ss_code_of(c, row, desc, &special);
    }
    if (mine) atomicAdd(&s_nulls, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_nulls) atomicAdd(nulls, (unsigned long long)s_nulls);
}

// exclusive prefix of the bucket sizes (sum of a bucket's `split` region counts): one workgroup, 1024 threads.  With heavy codes
// (hb ascending, lb = prefix of their row counts) the bucket's own entries start behind every heavy block up to and including the
// ones that belong in front of it: offs[b] += lb[#heavy with hb <= b]; heavy block i starts at hstart[i] = plain offs[hb[i]] + lb[i].
__global__ __launch_bounds__(1024) void ssort_offsets_kernel(const uint32_t* counts, int split, int64_t nbuckets, unsigned long long* offs,
                                                            unsigned long long* flags, int nheavy, const unsigned int* hb,
                                                            const unsigned long long* lb, unsigned long long* hstart, int has_null) {
    __shared__ unsigned long long part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (nbuckets + 1023) / 1024;
    const int64_t lo = (int64_t)tid * per, hi = lo + per < nbuckets ? lo + per : nbuckets;
    unsigned long long s = 0;
    bool too_big = false;
    for (int64_t b = lo; b < hi; b++) {
        unsigned long long c = 0;
        for (int g = 0; g < split; g++) c += counts[b * split + g];
        too_big = too_big || c > (unsigned long long)SS_LOCAL;
        s += c;
    }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < 1024; i++) { const unsigned long long x = part[i]; part[i] = run; run += x; }
        offs[nbuckets] = run + (nheavy ? lb[nheavy] : 0ULL);
        if (has_null) hstart[nheavy] = offs[nbuckets];     // the NULL rows: behind every value (NaNs included), in row order
    }
    __syncthreads();
    unsigned long long run = part[tid];
    int k = 0;                      // heavy codes with hb < b seen so far ...
    while (k < nheavy && (int64_t)hb[k] < lo) k++;
    for (int64_t b = lo; b < hi; b++) {
        while (k < nheavy && (int64_t)hb[k] == b) { hstart[k] = run + lb[k]; k++; }     // ... and the ones in front of bucket b
        offs[b] = run + (nheavy ? lb[k] : 0ULL);
        for (int g = 0; g < split; g++) run += counts[b * split + g];
    }
    if (too_big) __hip_atomic_store(&flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SsLocalArgs {
    const uint64_t* code; const uint32_t* row; const uint32_t* counts; int64_t cap; int split;
    const unsigned long long* offs;
    int64_t nbuckets;
    int64_t* idx_out;
    uint64_t* key_out;      // optional: sorted key values rebuilt from the codes
    int key_type, key_desc;
    unsigned long long* flags;
    int debug;
    const uint32_t* todo; vnm_dcol key;   // APX (vnm_sort_apx.inc): `code` holds entry words (a32 << 32 | row id); only the buckets with todo[f] set
    uint32_t* crowded;                    // [nbuckets], zeroed: the SMALL shape leaves a bucket with a crowded slot to the BIG one (which has the registers for the counting passes)
    const uint32_t* list; const unsigned long long* list_n;   // APX: the buckets the word kernel left, as a list (the kernel walks the list, not all buckets)
};

constexpr int SL_MAX_RUN = 48;    // entries per interpolation slot that are ordered by counting; more: the LSD passes
// Two shapes of the kernel share the buckets: SMALL (512 threads x 10 entries = 5120, 4096 slots: 78 KB of LDS, TWO workgroups
// per CU -- a bucket's phases are a chain of dependent barriers, a second workgroup fills the waits) takes every bucket that fits;
// BIG (1024 x 8 = 8192 entries and slots, one workgroup per CU) the few per cent that do not.
constexpr int SS_SMALL = 5120;

// Local sort of one bucket.  The codes of a bucket cover a sliver of the key distribution (1 / 2^18 of the rows), inside which
// they are spread almost evenly: an INTERPOLATION slot  floor((code - min) * SLOTS / (max - min + 1))  is a monotone function of
// the code that puts ~0.5 entries into each of 8192 slots.  One returning LDS atomic per entry counts the slots and hands out the
// entry's index inside its slot, one scan turns the counts into slot starts, the entries are placed, and every entry finds its
// rank inside its slot by comparing (code, row id) with the slot's few other entries -- five barriers for the whole bucket,
// whatever the width of the keys (eight-bit counting passes over the ~5 bytes that differ inside a bucket took 37 ms per 1e9
// rows; this takes the time in the table of DESIGN.md).  Rows of equal code share a slot, so the same comparison orders them by
// row id.  A slot with more than SL_MAX_RUN entries (duplicated keys, a lumpy distribution) sends the bucket through stable
// counting passes instead: row-id bytes, then code bytes.
// APX: the entries are the words of vnm_sort_apx.inc; the full codes are fetched from the key column by row id (the few buckets the
// word kernel leaves: beyond its room, a crowded slot)
template <int SL_BLOCK, int SL_SUB, int SL_SLOTS, bool BIG, bool APX = false>
__global__ __launch_bounds__(SL_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void ssort_local_kernel(SsLocalArgs a) {
    constexpr int SL_CAP = SL_BLOCK * SL_SUB, SL_WAVES = SL_BLOCK / 64;
    extern __shared__ uint64_t sl_lds[];
    uint64_t* const lcode = sl_lds;                                      // [SL_CAP]
    uint32_t* const lrow = (uint32_t*)(sl_lds + SL_CAP);                 // [SL_CAP]
    uint32_t* const cnt = lrow + SL_CAP;                                 // [SL_SLOTS] slot counts -> slot starts; the LSD passes' [SL_WAVES][256]
    uint32_t* const wcnt = cnt;
    __shared__ uint32_t off[256];
    __shared__ uint32_t wtot[SL_WAVES];
    __shared__ uint32_t rst[2][SS_MAX_REGIONS + 1];
    __shared__ unsigned long long s_min, s_max;
    __shared__ uint32_t s_long, s_ror, s_rand, s_crowd[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* mycnt = wcnt + wave * 256;
    // Round 6: the rank pass walks the PLACED entries (position i of the LDS arrays: conflict-free reads, neighbouring output addresses), so
    // the registers that held the bucket's entries are free once they are placed -- the NEXT bucket of this workgroup is loaded into
    // them while this one is ranked and written (two dependent DRAM latencies per bucket -- counts, then entries -- used to stand
    // in front of every bucket: 11.5 ms per 1e9 rows).
    uint64_t c[SL_SUB];
    uint32_t v[SL_SUB];
    // does bucket fb (n entries) belong to this kernel?  (n > SS_LOCAL: ssort_offsets_kernel has raised the flag; the SMALL shape leaves
    // buckets beyond its capacity to the BIG one; APX: only the buckets the word kernel left)
    auto mine = [&](uint32_t n, uint32_t crowd) -> bool {
        return n != 0 && n <= (uint32_t)SS_LOCAL && (APX || (BIG ? (n > (uint32_t)SS_SMALL || crowd != 0) : n <= (uint32_t)SS_SMALL));
    };
    auto meta = [&](int64_t fb, int buf) {   // (thread 0) region starts of bucket fb; APX: a bucket that is not on the list counts as empty
        uint32_t run = 0;
        if (!APX || a.todo[fb]) for (int g = 0; g < a.split; g++) { rst[buf][g] = run; run += a.counts[fb * a.split + g]; }
        rst[buf][a.split] = run;
        s_crowd[buf] = (BIG && !APX && a.crowded) ? a.crowded[fb] : 0u;
    };
    auto load_entries = [&](int64_t fb, int buf, uint32_t n) {   // wave w owns entries [w * 64 SUB, (w + 1) * 64 SUB), entry e = w * 64 SUB + k * 64 + lane
#pragma unroll
        for (int k = 0; k < SL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
            c[k] = ~0ULL; v[k] = ~0u;
            if (e < n) {
                int g = 0;
                while (rst[buf][g + 1] <= e) g++;
                const int64_t at = (fb * a.split + g) * a.cap + (e - rst[buf][g]);
                if (APX) { unsigned spc = 0; v[k] = (uint32_t)a.code[at]; c[k] = ss_code_of(a.key, (int64_t)v[k], a.key_desc, &spc); }
                else { c[k] = a.code[at]; v[k] = a.row[at]; }
            }
        }
    };
    int cur = 0;
    // work items: every bucket -- or, APX, the entries of the list
    const int64_t nwork = APX ? (int64_t)*a.list_n : a.nbuckets;
    auto bucket_of = [&](int64_t w) -> int64_t { return APX ? (int64_t)a.list[w] : w; };
    int64_t wi = blockIdx.x;
    if (wi >= nwork) return;
    int64_t f = bucket_of(wi);
    if (tid == 0) meta(f, 0);
    __syncthreads();
    uint32_t n = rst[0][a.split];
    bool have = mine(n, s_crowd[0]);
    if (have) load_entries(f, 0, n);
    for (; wi < nwork; wi += gridDim.x) {
        f = bucket_of(wi);
        const bool more = wi + gridDim.x < nwork;
        const int64_t fn = more ? bucket_of(wi + gridDim.x) : 0;
        if (tid == 0) {
            if (more) meta(fn, cur ^ 1); else { rst[cur ^ 1][a.split] = 0; s_crowd[cur ^ 1] = 0; }
            s_min = ~0ULL; s_max = 0; s_long = 0; s_ror = 0; s_rand = ~0u;
        }
        for (int i = tid; i < SL_SLOTS; i += SL_BLOCK) cnt[i] = 0;
        __syncthreads();
        const uint32_t n_next = rst[cur ^ 1][a.split];
        const bool have_next = more && mine(n_next, s_crowd[cur ^ 1]);
        if (!have) {
            if (have_next) load_entries(fn, cur ^ 1, n_next);
            __syncthreads();
            cur ^= 1; n = n_next; have = have_next;
            continue;
        }
        // ---- the bucket's code range, the bits of the row ids that differ
        uint64_t my_min = ~0ULL, my_max = 0;
        uint32_t r_or = 0, r_and = ~0u;
#pragma unroll
        for (int k = 0; k < SL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
            if (e < n) {
                my_min = c[k] < my_min ? c[k] : my_min; my_max = c[k] > my_max ? c[k] : my_max;
                r_or |= v[k]; r_and &= v[k];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t omn = __shfl_xor(my_min, o), omx = __shfl_xor(my_max, o);
            my_min = omn < my_min ? omn : my_min; my_max = omx > my_max ? omx : my_max;
            r_or |= __shfl_xor(r_or, o); r_and &= __shfl_xor(r_and, o);
        }
        if (lane == 0) { atomicMin(&s_min, my_min); atomicMax(&s_max, my_max); atomicOr(&s_ror, r_or); atomicAnd(&s_rand, r_and); }
        __syncthreads();
        const uint64_t lo = s_min, range = s_max - s_min;
        const unsigned long long obase = a.offs[f];
        // ---- interpolation slots
        const double scale = (double)SL_SLOTS / ((double)range + 1.0);
        auto slot_of = [&](uint64_t code) -> uint32_t {
            const uint32_t sidx = (uint32_t)((double)(code - lo) * scale);
            return sidx < (uint32_t)SL_SLOTS ? sidx : (uint32_t)SL_SLOTS - 1u;
        };
        uint32_t sp[SL_SUB];   // slot | index inside the slot << 16
#pragma unroll
        for (int k = 0; k < SL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
            sp[k] = 0;
            if (e < n) {
                const uint32_t sl = slot_of(c[k]);
                const uint32_t pi = atomicAdd(&cnt[sl], 1u);
                if (pi >= (uint32_t)SL_MAX_RUN) s_long = 1;
                sp[k] = sl | (pi << 16);
            }
        }
        __syncthreads();
        if (!s_long) {
            // ---- slot counts -> slot starts (exclusive scan of the counters: SLOTS / BLOCK per thread, waves, workgroup)
            uint32_t mine_c[SL_SLOTS / SL_BLOCK], sum = 0;
#pragma unroll
            for (int q = 0; q < SL_SLOTS / SL_BLOCK; q++) { mine_c[q] = cnt[tid * (SL_SLOTS / SL_BLOCK) + q]; sum += mine_c[q]; }
            uint32_t inc = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            uint32_t base = inc - sum;
            for (int w = 0; w < wave; w++) base += wtot[w];
#pragma unroll
            for (int q = 0; q < SL_SLOTS / SL_BLOCK; q++) { cnt[tid * (SL_SLOTS / SL_BLOCK) + q] = base; base += mine_c[q]; }
            __syncthreads();
            // ---- place
#pragma unroll
            for (int k = 0; k < SL_SUB; k++) {
                const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
                if (e < n) { const uint32_t p = cnt[sp[k] & 0xFFFFu] + (sp[k] >> 16); lcode[p] = c[k]; lrow[p] = v[k]; }
            }
            __syncthreads();
            // ---- the next bucket's entries on their way; rank the placed entries inside their slots by (code, row id); straight to the output
            if (have_next) load_entries(fn, cur ^ 1, n_next);
            for (uint32_t i = tid; i < n; i += SL_BLOCK) {
                const uint64_t ci = lcode[i];
                const uint32_t vi = lrow[i];
                const uint32_t sl = slot_of(ci);
                const uint32_t s0 = cnt[sl], s1 = sl + 1 < (uint32_t)SL_SLOTS ? cnt[sl + 1] : n;
                uint32_t rank = 0;
                for (uint32_t j = s0; j < s1; j++) {
                    const uint64_t cj = lcode[j];
                    rank += (cj < ci || (cj == ci && lrow[j] < vi)) ? 1u : 0u;
                }
                const unsigned long long pos = obase + s0 + rank;
                a.idx_out[pos] = (int64_t)vi;
                if (a.key_out) {
                    const uint64_t en = a.key_desc ? ~ci : ci;
                    a.key_out[pos] = a.key_type == VNM_F64 ? (uint64_t)__double_as_longlong(dec_f64(en)) : (a.key_type == VNM_I64 ? (uint64_t)dec_i64(en) : en);
                }
            }
            __syncthreads();
            cur ^= 1; n = n_next; have = have_next;
            continue;
        }
        if (!BIG && !APX) {   // the SMALL shape: such a bucket is the BIG shape's (launched behind this kernel)
            if (tid == 0) a.crowded[f] = 1;
            if (have_next) load_entries(fn, cur ^ 1, n_next);
            __syncthreads();
            cur ^= 1; n = n_next; have = have_next;
            continue;
        }
        // ---- a crowded slot: stable 8-bit counting passes in LDS (ballot ranks as in onesweep_kernel) -- the row-id bytes first,
        // then the code bytes; bytes that are the same in every entry of the bucket are skipped.  Only the n real entries take
        // part (lanes beyond them sit out of the ballots), so they occupy positions 0 .. n - 1 after every pass.
        uint64_t my_or = 0, my_and = ~0ULL;
#pragma unroll
        for (int k = 0; k < SL_SUB; k++)
            if ((uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane < n) { my_or |= c[k]; my_and &= c[k]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { my_or |= __shfl_xor(my_or, o); my_and &= __shfl_xor(my_and, o); }
        __syncthreads();
        if (tid == 0) { s_min = 0; s_max = ~0ULL; }     // reused as the OR / AND accumulators of the codes
        __syncthreads();
        if (lane == 0) { atomicOr(&s_min, my_or); atomicAnd(&s_max, my_and); }
        __syncthreads();
        const uint64_t diff = s_min ^ s_max;
        const uint32_t rdiff = s_ror ^ s_rand;
        for (int q = 0; q < 12; q++) {
            const int which = q < 4 ? 1 : 0, byte = q < 4 ? q : q - 4;
            const bool live = which ? ((rdiff >> (8 * byte)) & 255u) != 0 : ((diff >> (8 * byte)) & 255ULL) != 0;
            if (!live) continue;
            for (int i = tid; i < SL_WAVES * 256; i += SL_BLOCK) wcnt[i] = 0;
            __syncthreads();
            uint32_t lp[SL_SUB];
#pragma unroll
            for (int k = 0; k < SL_SUB; k++) {
                const bool in = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane < n;
                const uint32_t dg = which ? (v[k] >> (8 * byte)) & 255u : (uint32_t)(c[k] >> (8 * byte)) & 255u;
                uint64_t m = __ballot(in);
#pragma unroll
                for (int bit = 0; bit < 8; bit++) {
                    const uint64_t bb = __ballot((dg >> bit) & 1u);
                    m &= ((dg >> bit) & 1u) ? bb : ~bb;
                }
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                lp[k] = 0;
                if (in) {
                    lp[k] = mycnt[dg] + before;                    // LDS ops of one wave execute in order
                    if (before == 0) mycnt[dg] += (uint32_t)__popcll(m);
                }
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t s2 = 0;
#pragma unroll
                for (int w = 0; w < SL_WAVES; w++) { const uint32_t x = wcnt[w * 256 + tid]; wcnt[w * 256 + tid] = s2; s2 += x; }
                uint32_t inc = s2;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
                off[tid] = inc - s2;
                if (lane == 63) wtot[wave] = inc;
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t add = 0;
                for (int w = 0; w < wave; w++) add += wtot[w];
                off[tid] += add;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SL_SUB; k++) {
                if ((uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane < n) {
                    const uint32_t dg = which ? (v[k] >> (8 * byte)) & 255u : (uint32_t)(c[k] >> (8 * byte)) & 255u;
                    const uint32_t p = lp[k] + off[dg] + mycnt[dg];
                    lcode[p] = c[k];
                    lrow[p] = v[k];
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SL_SUB; k++) {
                const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
                if (e < n) { c[k] = lcode[e]; v[k] = lrow[e]; }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < SL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * SL_SUB) + (uint32_t)k * 64 + lane;
            if (e < n) {
                a.idx_out[obase + e] = (int64_t)v[k];
                if (a.key_out) {
                    const uint64_t en = a.key_desc ? ~c[k] : c[k];
                    a.key_out[obase + e] = a.key_type == VNM_F64 ? (uint64_t)__double_as_longlong(dec_f64(en)) : (a.key_type == VNM_I64 ? (uint64_t)dec_i64(en) : en);
                }
            }
        }
        if (have_next) load_entries(fn, cur ^ 1, n_next);
        __syncthreads();
        cur ^= 1; n = n_next; have = have_next;
    }
}

// debugging aid (VNM_SSORT_DEBUG = 7 / 8): every row id of the regions of a scatter level is counted in seen[]
__global__ void ssort_check_kernel(const uint32_t* row, const uint32_t* counts, int64_t cap, int64_t nregions, uint32_t* seen, int64_t n, unsigned long long* bad) {
    for (int64_t r = blockIdx.x; r < nregions; r += gridDim.x) {
        const uint32_t c = counts[r];
        for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
            const uint32_t x = row[r * cap + i];
            if ((int64_t)x < n) atomicAdd(&seen[x], 1u); else atomicAdd(bad, 1ULL);
        }
    }
}

// ---- what the two sample sorts (sample_sort in vnm_sort.hip, sample_sort_apx in vnm_sort_apx.inc) do alike ----------------------------
// m strided keys of the column as codes, sorted.  They stay in r->code[r->cur] for as long as the caller's `r` lives; the sample's NULL rows
// are counted into *sample_nulls (device) and stand at the end with the all-ones code.
static int sorted_sample(const vnm_dcol& key, int desc, int64_t n, int64_t m, unsigned long long* sample_nulls, RadixBufs* r, hipStream_t s) {
    VNM_TRY(radix_alloc(r, m));
    {
        KernelTimer timer("sort_sample", s);
        ssort_sample_kernel<<<grid_for(m), 256, 0, s>>>(key, desc, n, m, r->code[0], sample_nulls);
    }
    sort_iota_kernel<<<grid_for(m), 256, 0, s>>>(r->val[0], m);
    r->cur = 0;
    return radix_sort_codes(r, m, s);
}
// The smallest number of sorted samples S[0 .. m) that a tile of 4096 consecutive rows spans, into *span (device) and, once the caller has
// synchronised the stream, into *span_host (~0: no tile was looked at).
static int sample_cluster_span(const vnm_dcol& key, int desc, int64_t n, const uint64_t* S, int64_t m, unsigned long long* span,
                               unsigned long long* span_host, hipStream_t s) {
    VNM_HIP(hipMemsetAsync(span, 0xFF, 8, s));
    ssort_cluster_kernel<<<64, 256, 0, s>>>(key, desc, n, S, m, span);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(span_host, span, 8, hipMemcpyDeviceToHost, s));
    return 0;
}
// rows that arrive clustered (a sorted column): the ring scatters would crawl -- the LSD passes do not care
static bool rows_arrive_clustered(unsigned long long span, int64_t m_valid) {
    return span != ~0ULL && (int64_t)span < m_valid / 8 && env_sort_i64("VNM_SSORT_CLUSTER_CHECK", 1);
}

// Level 1 of either sort: `grid1` workgroups of SS_BLOCK threads, each scattering `rows_per_wg` rows in sub-tiles of `sub`; level 2 reads
// the grid1 regions of a level-1 bucket in `split2` parts (at most SS_MAX_REGIONS regions per workgroup).
struct Level1Geometry { int pairs1; int64_t sub; int grid1; int64_t rows_per_wg; int split2; };
static Level1Geometry level1_geometry(int64_t n, int64_t pairs1, int64_t grid1_per_cu, int64_t split2_min) {
    Level1Geometry g{};
    g.pairs1 = pairs1 >= 2 ? 2 : 1;
    g.sub = 2 * SS_BLOCK * g.pairs1;
    g.grid1 = (int)std::min<int64_t>((int64_t)device_info().num_cus * grid1_per_cu, std::max<int64_t>(1, (n + g.sub - 1) / g.sub));
    g.rows_per_wg = (((n + g.sub - 1) / g.sub + g.grid1 - 1) / g.grid1) * g.sub;
    g.split2 = std::max(std::max(1, (g.grid1 + SS_MAX_REGIONS - 1) / SS_MAX_REGIONS), (int)split2_min);
    return g;
}
