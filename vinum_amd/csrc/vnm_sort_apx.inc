// Sample sort over 8-byte ENTRY WORDS (round 6; included by vnm_sort.hip after vnm_sort_sample.inc, inside namespace vnm) --
// Sort::Sorted's SortIndices (sort.cpp:22-37) for one 8-byte key when only the ORDER is asked for (vnm_sort_indices;
// the keyed variant, which also hands back the sorted key column, needs the full codes and keeps vnm_sort_sample.inc).
//
// The splitter sort moves (code 8, row id 4) = 12 bytes per row and level and looks every row up among 512 splitters twice (LDS
// searches: twice the vector and three times the LDS instructions of the aggregate's ring scatter, profiles/r05_pmc_sq_sort.txt).
// Here a row travels as ONE 64-bit word (a32 << 32 | row id) where the 41-bit value F = (bucket9 << 32 | a32) is a monotone,
// piecewise-linear function of the code that EQUALISES the distribution:
//   * a 2^21-key strided sample is sorted; XS_K = 2048 equal-width cells cover its range -- in CODE space or in VALUE space, see below --;
//     fb[c] = the share of the sample below cell c's lower edge, scaled to 2^41 (+ a defensive mixture, xsort_map_kernel);
//     F(row) = fb[c] + (offset in the cell) * (fb[c + 1] - fb[c]): ONE 16-byte LDS read, one 64 x 64 -> high multiply;
//   * level 1 scatters by F >> 32 (512 rings of 32 words in LDS, whole 128-byte blocks out, as dring_scatter_kernel<..., FX>), level 2 by
//     the next bits of a32 -- no lookup at all --, and the bucket sort in LDS takes its 4096 interpolation slots straight from the bits
//     below (no min / max pass): 8 + 8 | 8 + 8 | 8 + 8 = 48 GB per 1e9 rows where the splitter sort moves 64;
//   * a32 is LOSSY (2^32 levels per level-1 bucket): two entries of one bucket with the same a32 are ordered by their FULL codes,
//     fetched from the key column by row id inside the rank loop (5e-4 of the rows of 1e9 distinct keys).  Data with many
//     duplicated keys would fetch for every row: the sorted sample's equal neighbours decide (xsort_prep_kernel), such data -- and
//     data whose distribution is not linear at the scale of a cell (the sample's own buckets under F are counted) -- keeps the
//     splitter sort.  A bucket that outgrows its room at run time fails the attempt the same way.
// The result is the same total order (code, then row id) whichever path produced it.
constexpr int XS_K = 2048;                       // cells of the map
constexpr uint64_t XS_FMAX = (1ULL << 41) - 1;   // F: 9 bucket bits + 32
constexpr int XS_CAP = 32, XS_FB = 16;           // ring words per partition, words per flushed block (128 bytes)

// The map works in one of two spaces, whichever the sample's own buckets come out more even in:
//   mode 0, CODE space: cells of 2^sh codes (aligned, so the binades of a float64 key end on cell edges) -- floats spread over many
//           orders of magnitude (a log-like code), integers;
//   mode 1, VALUE space: cells of equal width in the key's value u (as a double; -v for descending order) -- floats around zero or
//           within a few binades (N(11, 3): the codes between -3 and +25 cross 2 x 1026 binades, all but a dozen of them empty), and
//           integers again.  (double)key is not injective for 64-bit integers, but monotone: ties are ordered through the key column.
// Both are monotone, non-decreasing functions of the code.  The cells span the sample minus `trim` samples at either end (outliers
// would stretch them); what lies outside maps to 0 / XS_FMAX and is ordered through the key column.
struct XsMap { int mode; int sh; uint64_t base; double u_lo, inv_w; };
struct XsHdr {   // what the sample says (device -> host, one copy)
    unsigned long long base; long long sh; double u_lo, inv_w; long long m_eff; unsigned long long eq_pairs; unsigned long long max_group[2]; long long ok[2];
};

__device__ __forceinline__ double xs_u_of_code(int type, int desc, uint64_t code) {
    const uint64_t e = desc ? ~code : code;
    if (type == VNM_F64) { const double d = dec_f64(e); return desc ? -d : d; }
    if (type == VNM_I64) { const double x = (double)dec_i64(e); return desc ? -x : x; }
    const double x = (double)e;
    return desc ? -x : x;
}

// F of a row: MODE 0 from its code, MODE 1 from its value u
template <int MODE>
__device__ __forceinline__ uint64_t xs_map(const uint64_t* fb, const XsMap& mp, uint64_t code, double u) {
    if (MODE == 0) {
        if (code < mp.base) return 0;
        const uint64_t d = code - mp.base, cell = d >> mp.sh;
        if (cell >= (uint64_t)XS_K) return XS_FMAX;
        const uint64_t f0 = fb[cell], f1 = fb[cell + 1];
        return f0 + __umul64hi((d & ((1ULL << mp.sh) - 1ULL)) << (64 - mp.sh), f1 - f0);   // (1 <= sh <= 53)
    }
    const double t = (u - mp.u_lo) * mp.inv_w;
    if (!(t >= 0.0)) return 0;
    if (t >= (double)XS_K) return XS_FMAX;
    const int cell = (int)t;
    const uint64_t f0 = fb[cell], f1 = fb[cell + 1];
    return f0 + __umul64hi((uint64_t)((t - (double)cell) * 18446744073709551616.0), f1 - f0);   // (t - cell <= 1 - 2^-42: the product is below 2^64)
}
// the cell of a SAMPLE (a code): -1 below the cells, XS_K above them
__device__ __forceinline__ int xs_cell_of_code(int mode, const XsHdr* h, int type, int desc, uint64_t code) {
    if (mode == 0) {
        if (code < h->base) return -1;
        const uint64_t cell = (code - h->base) >> (int)h->sh;
        return cell >= (uint64_t)XS_K ? XS_K : (int)cell;
    }
    const double t = (xs_u_of_code(type, desc, code) - h->u_lo) * h->inv_w;
    if (!(t >= 0.0)) return -1;
    return t >= (double)XS_K ? XS_K : (int)t;
}
__device__ __forceinline__ uint64_t xs_map_sample(int mode, const XsHdr* h, const uint64_t* fb, int type, int desc, uint64_t code) {
    XsMap mp; mp.mode = mode; mp.sh = (int)h->sh; mp.base = h->base; mp.u_lo = h->u_lo; mp.inv_w = h->inv_w;
    return mode == 0 ? xs_map<0>(fb, mp, code, 0.0) : xs_map<1>(fb + (XS_K + 1), mp, 0, xs_u_of_code(type, desc, code));
}

// the sorted sample -> cell geometry of both modes, the number of equal neighbours
__global__ __launch_bounds__(256) void xsort_prep_kernel(const uint64_t* S, int64_t m, XsHdr* h, int type, int desc) {
    __shared__ long long s_meff;
    if (threadIdx.x == 0) {   // samples in front of the all-ones codes (NaN): every workgroup finds it by itself
        int64_t lo = 0, hi = m;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (S[mid] < ~0ULL) lo = mid + 1; else hi = mid; }
        s_meff = lo;
    }
    __syncthreads();
    const int64_t me = s_meff;
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        h->m_eff = me;
        h->ok[0] = 0; h->ok[1] = 0;
        if (me >= 4096) {
            const int64_t trim = me >> 19 > 2 ? me >> 19 : 2;
            const uint64_t cmin = S[trim], cmax = S[me - 1 - trim];
            int sh = 1;
            while (sh < 53 && ((cmax - (cmin & ~((1ULL << sh) - 1ULL))) >> sh) >= (uint64_t)XS_K) sh++;
            const uint64_t base = cmin & ~((1ULL << sh) - 1ULL);
            h->base = base; h->sh = sh;
            h->ok[0] = ((cmax - base) >> sh) < (uint64_t)XS_K ? 1 : 0;
            const double ulo = xs_u_of_code(type, desc, cmin), uhi = xs_u_of_code(type, desc, cmax);
            const double span = uhi - ulo;
            h->u_lo = ulo;
            h->inv_w = 0.0;
            if (span > 0.0 && span < 1.7e308 && ulo == ulo) {
                const double iw = (double)XS_K / span * (1.0 - 1.0 / 1048576.0);
                if (iw > 0.0 && iw < 1.7e308) { h->inv_w = iw; h->ok[1] = 1; }
            }
        }
    }
    unsigned int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < me; i += (int64_t)gridDim.x * blockDim.x) mine += S[i] == S[i - 1] ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&h->eq_pairs, (unsigned long long)mine);
}

// fb[mode][c] = the share of the sample in front of cell c, scaled to 2^41   (blockIdx.y = mode)
__global__ __launch_bounds__(256) void xsort_map_kernel(const uint64_t* S, const XsHdr* h, uint64_t* fb, int type, int desc, uint64_t reserve) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, mode = blockIdx.y;
    if (c > XS_K || !h->ok[mode]) return;
    uint64_t* const out = fb + (size_t)mode * (XS_K + 1);
    if (c == XS_K) { out[c] = XS_FMAX - reserve; return; }
    const int64_t me = h->m_eff;
    int64_t lo = 0, hi = me;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (xs_cell_of_code(mode, h, type, desc, S[mid]) < c) lo = mid + 1; else hi = mid; }
    // (the rows outside the cells -- F = 0 and XS_FMAX -- get the first and the last final bucket to themselves: `reserve` values of F at
    //  either end; they are a few samples' worth of rows, all with one a32, and would crowd a regular bucket beyond its room)
    // A DEFENSIVE MIXTURE: 15 / 16 of the F range follows the sample's distribution, 1 / 16 is dealt evenly to the cells.  Where a cell holds
    // fewer samples than its even share is worth (m / 16 K: 64 of 2^21) the even share decides, so the buckets of thinly sampled regions (the
    // tails: eight samples per final bucket's worth of rows, +- 35 %) are many and nearly empty instead of few and as noisy as the sample;
    // the buckets of the dense regions grow by 1 / 15.
    const uint64_t span = (XS_FMAX + 1) - 2 * reserve, even = span / 16;
    const uint64_t f = reserve + (uint64_t)(((unsigned __int128)(uint64_t)lo * (unsigned __int128)(span - even)) / (unsigned __int128)(uint64_t)me)
                     + (uint64_t)(((unsigned __int128)(unsigned)c * (unsigned __int128)even) / (unsigned)XS_K);
    out[c] = f < XS_FMAX - reserve ? f : XS_FMAX - reserve;
}

// the sample's own rows per group of final buckets under the map (groups of 2^(41 - gbits) values of F): the largest one   (blockIdx.y = mode)
__global__ __launch_bounds__(256) void xsort_balance_kernel(const uint64_t* S, XsHdr* h, const uint64_t* fb, int gbits, int type, int desc) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int mode = blockIdx.y;
    if (g >= ((int64_t)1 << gbits) || !h->ok[mode]) return;
    const int64_t me = h->m_eff;
    auto first_at = [&](uint64_t fv) -> int64_t {   // first sample whose F is >= fv
        int64_t lo = 0, hi = me;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (xs_map_sample(mode, h, fb, type, desc, S[mid]) < fv) lo = mid + 1; else hi = mid; }
        return lo;
    };
    const int64_t a = first_at((uint64_t)g << (41 - gbits));
    const int64_t b = g + 1 == ((int64_t)1 << gbits) ? me : first_at((uint64_t)(g + 1) << (41 - gbits));
    atomicMax(&h->max_group[mode], (unsigned long long)(b - a));
}

struct XsArgs {
    vnm_dcol key; int desc; int64_t nrows;                                                              // level 1 input
    const uint64_t* in_words; const uint32_t* in_counts; int64_t in_cap; int in_regions, in_split;      // level 2 input
    const uint64_t* fb; XsMap map;                                                                      // the map (level 1)
    int qbits;                                                                                          // level 2: 2^qbits sub-buckets from the top bits of a32
    uint64_t* out_words; uint32_t* out_counts; int64_t out_cap;
    unsigned long long* flags;                                                                          // [0] failure (a region is full)  [2] length of the side list
    int nt; int ready_list;
    int has_null; unsigned long long* side; int64_t side_cap;                                           // level 1: the rows whose key is NULL go to `side` (row ids), behind every value
};

typedef uint64_t xs_w2 __attribute__((ext_vector_type(2)));

template <bool FROM_KEYS, int SP, int MODE = 0>
__global__ __launch_bounds__(SS_BLOCK) void xsort_scatter_kernel(XsArgs a) {
    constexpr int NE = 2 * SP;   // entries per lane and sub-tile
    extern __shared__ uint64_t xs_lds[];
    uint64_t* const ring = xs_lds;                              // [SS_B][XS_CAP]
    uint64_t* const lut = xs_lds + SS_B * XS_CAP;               // [XS_K + 1] (level 1)
    __shared__ uint32_t fill[SS_B], head[SS_B], cursor[SS_B], s_retry[2], s_nready[2];
    __shared__ uint16_t ready[SS_B];
    const RingState<uint32_t> rs{fill, head, cursor, s_retry, s_nready, ready};
    __shared__ uint32_t s_hcnt[2];
    __shared__ unsigned long long s_hbase;
    __shared__ uint32_t rstart[SS_MAX_REGIONS + 2];
    const int tid = threadIdx.x;
    const int np = FROM_KEYS ? SS_B : (1 << a.qbits);
    int64_t out_base, out_stride;
    int pin = 0;
    if (FROM_KEYS) { out_base = blockIdx.x; out_stride = gridDim.x; }
    else {
        pin = blockIdx.x / a.in_split;
        const int g = blockIdx.x % a.in_split;
        out_base = (int64_t)pin * np * a.in_split + g; out_stride = a.in_split;
    }
    ring_init<SS_BLOCK, SS_B>(rs);
    if (FROM_KEYS) for (int i = tid; i <= XS_K; i += SS_BLOCK) lut[i] = a.fb[(size_t)MODE * (XS_K + 1) + i];
    if (tid < 2) s_hcnt[tid] = 0;
    __syncthreads();
    const uint32_t ocap = (uint32_t)a.out_cap;
    int hp = 0;
    int ph = 0;
    const bool use_list = a.ready_list != 0;

    // whole blocks of the rings -> the partition's region: eight lanes per partition, lane j moves words 2j, 2j + 1 of a block.  A full
    // region fails the sort (flags[0]); its count runs on, capped at out_cap
    auto flush = [&](bool drain) {
        ring_flush<XS_FB, 8, SS_BLOCK, true>(rs, ph, drain, use_list, np, XS_CAP, ocap, [&](int p, uint32_t src, int64_t dst, uint32_t n_here, int j, bool room) {
            if (!room) { if (j == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            else if ((uint32_t)(2 * j) < n_here) {
                const xs_w2 x = *(const xs_w2*)(ring + p * XS_CAP + (int)src + 2 * j);
                xs_w2* const to = (xs_w2*)(a.out_words + (out_base + (int64_t)p * out_stride) * a.out_cap + dst + 2 * j);
                if (a.nt) __builtin_nontemporal_store(x, to); else *to = x;
            }
        });
    };
    auto rounds = [&](const uint32_t (&p)[NE], const uint64_t (&w)[NE], uint32_t okmask) {
        ring_rounds<NE>(rs, ph, okmask, [&](int e) -> bool {
            const uint32_t slot = ring_reserve<XS_FB>(rs, ph, p[e], XS_CAP, use_list);
            if (slot != RING_FULL) ring[p[e] * XS_CAP + slot] = w[e];
            return slot != RING_FULL;
        }, [&]() { flush(false); }, [](int, uint32_t) { return false; });
    };

    if (FROM_KEYS) {
        const int64_t sub = (int64_t)NE * SS_BLOCK;
        const int64_t nsub = (a.nrows + sub - 1) / sub, nfull = a.nrows / sub;
        const bool aligned = (a.key.offset & 1) == 0;
        const XsMap mp = a.map;
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
            uint32_t p[NE]; uint64_t w[NE]; uint32_t okmask = 0;
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const int u = e >> 1, el = e & 1;
                const int64_t r = st * sub + (int64_t)u * 2 * SS_BLOCK + 2 * tid + el;
                p[e] = 0; w[e] = 0;
                if (r < a.nrows) {
                    okmask |= 1u << e;
                    const uint64_t raw = (st < nfull && aligned) ? (el ? kk[u].y : kk[u].x) : ((const uint64_t*)a.key.values)[a.key.offset + r];
                    uint64_t F;
                    if (MODE == 0) F = xs_map<0>(lut, mp, ss_encode(a.key.type, raw, a.desc, &special), 0.0);
                    else {
                        double uu;
                        if (a.key.type == VNM_F64) uu = __longlong_as_double((long long)raw);
                        else if (a.key.type == VNM_I64) uu = (double)(int64_t)raw;
                        else uu = (double)raw;
                        F = uu != uu ? XS_FMAX : xs_map<1>(lut, mp, 0, a.desc ? -uu : uu);
                    }
                    p[e] = (uint32_t)(F >> 32);
                    w[e] = (F << 32) | (uint64_t)(uint32_t)r;
                }
            }
            load_sub(st + gridDim.x);
            if (a.has_null) {   // rows whose key is NULL: their row ids go to the side list
                okmask &= ~ring_side_list<NE>(s_hcnt, s_hbase, hp, &a.flags[2], [&](int e) -> bool {
                    if (!((okmask >> e) & 1u)) return false;
                    const int64_t vr = a.key.offset + (int64_t)(uint32_t)w[e];
                    return !((a.key.validity[vr >> 3] >> (vr & 7)) & 1);
                }, [&](int e, unsigned long long pos) {
                    if ((int64_t)pos < a.side_cap) a.side[pos] = (unsigned long long)(uint32_t)w[e];
                    else __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                });
            }
            rounds(p, w, okmask);
        }
    } else {
        const RingRegions rg2 = ring_regions<2>(rstart, a.in_counts, a.in_regions, a.in_split, a.in_regions, 1);   // pairs of entries
        const uint32_t total_in = rg2.total;
        const int qsh = 32 - a.qbits;
        xs_w2 ew[SP];
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
                    ew[u] = *(const xs_w2*)(a.in_words + rg * a.in_cap + e0);
                    okm |= (e0 + 1 < a.in_counts[rg] ? 3u : 1u) << (2 * u);
                }
            }
        };
        load_pairs(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += SP * SS_BLOCK) {
            uint32_t p[NE]; uint64_t w[NE];
#pragma unroll
            for (int u = 0; u < SP; u++) {
                w[2 * u] = ew[u].x; w[2 * u + 1] = ew[u].y;
                p[2 * u] = (uint32_t)(w[2 * u] >> 32) >> qsh; p[2 * u + 1] = (uint32_t)(w[2 * u + 1] >> 32) >> qsh;
            }
            const uint32_t okmask = okm;
            load_pairs(t0 + SP * SS_BLOCK);
            rounds(p, w, okmask);
        }
    }
    flush(true);
    __syncthreads();
    for (int i = tid; i < np; i += SS_BLOCK) a.out_counts[out_base + (int64_t)i * out_stride] = cursor[i];
}

// the NULL rows' part of the output: the sorted side list (row ids) behind every value
__global__ __launch_bounds__(256) void xsort_nulls_kernel(const unsigned long long* side, int64_t len, const unsigned long long* offs_total, int64_t* idx_out) {
    const unsigned long long base = *offs_total;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < len; q += (int64_t)gridDim.x * blockDim.x) idx_out[base + q] = (int64_t)(side[q] & 0xFFFFFFFFULL);
}

// exclusive prefix of the bucket sizes over many workgroups: partial sums per chunk of XO_CHUNK buckets, then every workgroup adds the
// chunks in front of its own (ssort_offsets_kernel is one workgroup: 0.46 ms for 2^18 buckets)
constexpr int XO_CHUNK = 1024;
__global__ __launch_bounds__(256) void xsort_sizes_kernel(const uint32_t* counts, int split, int64_t nbuckets, unsigned long long* part, unsigned long long* flags, int limit) {
    __shared__ unsigned long long s_w[4];
    const int64_t b0 = (int64_t)blockIdx.x * XO_CHUNK;
    unsigned long long s = 0;
    bool too_big = false;
    for (int64_t b = b0 + threadIdx.x; b < b0 + XO_CHUNK && b < nbuckets; b += 256) {
        unsigned long long c = 0;
        for (int g = 0; g < split; g++) c += counts[b * split + g];
        too_big = too_big || c > (unsigned long long)limit;
        s += c;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (too_big) __hip_atomic_store(&flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(256) void xsort_offsets_kernel(const uint32_t* counts, int split, int64_t nbuckets, const unsigned long long* part, unsigned long long* offs) {
    __shared__ unsigned long long s_w[4], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long before = 0;
    for (int i = tid; i < (int)blockIdx.x; i += 256) before += part[i];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) s_w[wave] = before;
    __syncthreads();
    if (tid == 0) s_base = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    // thread t: buckets [b0 + 4 t, b0 + 4 t + 4)
    const int64_t b0 = (int64_t)blockIdx.x * XO_CHUNK + (int64_t)tid * (XO_CHUNK / 256);
    unsigned long long c[XO_CHUNK / 256], sum = 0;
#pragma unroll
    for (int q = 0; q < XO_CHUNK / 256; q++) {
        c[q] = 0;
        if (b0 + q < nbuckets) for (int g = 0; g < split; g++) c[q] += counts[(b0 + q) * split + g];
        sum += c[q];
    }
    unsigned long long inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned long long run = s_base + inc - sum;
    for (int w = 0; w < wave; w++) run += s_w[w];
#pragma unroll
    for (int q = 0; q < XO_CHUNK / 256; q++) {
        if (b0 + q < nbuckets) offs[b0 + q] = run;
        run += c[q];
        if (b0 + q == nbuckets - 1) offs[nbuckets] = run;
    }
}

// The bucket sort over entry words.  Every entry of a bucket shares the bits of F above `rbits`; below them the distribution is even
// by construction, so the 4096 interpolation slots are the next twelve bits -- no min / max pass.  One returning LDS atomic per entry
// counts the slots, a scan turns the counts into slot starts, the entries are placed, and every entry ranks itself inside its slot by
// comparing WORDS (a32, then row id); an entry that meets its own a32 in another word fetches the full codes (see the header).
// 36 KB + 16 KB of LDS, 512 threads: three workgroups per CU.  A bucket beyond XL_CAP entries or with a crowded slot is left to
// ssort_local_kernel<..., APX> (todo[f] = 1).
constexpr int XL_BLOCK = 512, XL_SUB = 9, XL_CAP = XL_BLOCK * XL_SUB, XL_SLOTS = 4096, XL_MAX_RUN = 32, XL_MAX_SPLIT = 8;
struct XlArgs {
    const uint64_t* words; const uint32_t* counts; int64_t cap; int split;
    const unsigned long long* offs; int64_t nbuckets;
    int64_t* idx_out;
    vnm_dcol key; int desc;
    int rbits;
    uint32_t* todo; uint32_t* list;   // the buckets left to the long kernel: a flag per bucket, and their list (flags[4] entries)
    unsigned long long* flags;   // [4] buckets left to the long kernel  [5] entries ordered through the key column
};

__global__ __launch_bounds__(XL_BLOCK) __attribute__((amdgpu_waves_per_eu(6, 6))) void xsort_local_kernel(XlArgs a) {
    __shared__ uint64_t lw[XL_CAP];
    __shared__ uint32_t cnt[XL_SLOTS];
    __shared__ uint32_t wtot[XL_BLOCK / 64];
    __shared__ uint32_t rst[2][XL_MAX_SPLIT + 1];
    __shared__ uint32_t s_long;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t rmask = a.rbits >= 32 ? ~0u : ((1u << a.rbits) - 1u);
    const int sshift = a.rbits > 12 ? a.rbits - 12 : 0;
    uint32_t nties = 0;
    // The words of a bucket are in registers only until they are placed; the rank pass walks the PLACED entries (lane i takes position i:
    // conflict-free LDS reads, and the row ids of neighbouring positions go to neighbouring output addresses).  So the next bucket's
    // words are loaded into the same registers while this one is ranked and written.
    uint64_t w[XL_SUB];
    auto meta = [&](int64_t f, int buf) {   // (thread 0)
        uint32_t run = 0;
        for (int g = 0; g < a.split; g++) { rst[buf][g] = run; run += a.counts[f * a.split + g]; }
        rst[buf][a.split] = run;
    };
    auto load_words = [&](int64_t f, int buf, uint32_t n) {
#pragma unroll
        for (int k = 0; k < XL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * XL_SUB) + (uint32_t)k * 64 + lane;
            w[k] = ~0ULL;
            if (e < n) {
                int g = 0;
                while (rst[buf][g + 1] <= e) g++;
                w[k] = a.words[(f * a.split + g) * a.cap + (e - rst[buf][g])];
            }
        }
    };
    int cur = 0;
    int64_t f = blockIdx.x;
    if (f >= a.nbuckets) return;
    if (tid == 0) meta(f, 0);
    __syncthreads();
    uint32_t n = rst[0][a.split];
    if (n && n <= (uint32_t)XL_CAP) load_words(f, 0, n);
    for (; f < a.nbuckets; f += gridDim.x) {
        const int64_t fn = f + gridDim.x;
        if (tid == 0) { if (fn < a.nbuckets) meta(fn, cur ^ 1); s_long = 0; }
        for (int i = tid; i < XL_SLOTS; i += XL_BLOCK) cnt[i] = 0;
        __syncthreads();
        const uint32_t n_next = fn < a.nbuckets ? rst[cur ^ 1][a.split] : 0u;
        const bool next_here = n_next && n_next <= (uint32_t)XL_CAP;
        bool skip = n == 0 || n > (uint32_t)XL_CAP;
        uint32_t sp[XL_SUB];   // slot | index inside the slot << 12
        if (!skip) {
#pragma unroll
            for (int k = 0; k < XL_SUB; k++) {
                const uint32_t e = (uint32_t)wave * (64 * XL_SUB) + (uint32_t)k * 64 + lane;
                sp[k] = 0;
                if (e < n) {
                    uint32_t slot = ((uint32_t)(w[k] >> 32) & rmask) >> sshift;
                    slot = slot < (uint32_t)XL_SLOTS ? slot : (uint32_t)XL_SLOTS - 1u;
                    const uint32_t pos = atomicAdd(&cnt[slot], 1u);
                    if (pos >= (uint32_t)XL_MAX_RUN) s_long = 1;
                    sp[k] = slot | (pos << 12);
                }
            }
            __syncthreads();
            skip = s_long != 0;
        }
        if (skip) {   // nothing here, or a bucket for the long kernel
            if (n && tid == 0) { a.todo[f] = 1; a.list[atomicAdd(&a.flags[4], 1ULL)] = (uint32_t)f; }
            if (next_here) load_words(fn, cur ^ 1, n_next);
            __syncthreads();
            cur ^= 1; n = n_next;
            continue;
        }
        // ---- slot counts -> slot starts
        uint32_t mine[XL_SLOTS / XL_BLOCK], sum = 0;
#pragma unroll
        for (int q = 0; q < XL_SLOTS / XL_BLOCK; q++) { mine[q] = cnt[tid * (XL_SLOTS / XL_BLOCK) + q]; sum += mine[q]; }
        uint32_t inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t base = inc - sum;
        for (int q = 0; q < wave; q++) base += wtot[q];
#pragma unroll
        for (int q = 0; q < XL_SLOTS / XL_BLOCK; q++) { cnt[tid * (XL_SLOTS / XL_BLOCK) + q] = base; base += mine[q]; }
        __syncthreads();
        // ---- place
#pragma unroll
        for (int k = 0; k < XL_SUB; k++) {
            const uint32_t e = (uint32_t)wave * (64 * XL_SUB) + (uint32_t)k * 64 + lane;
            if (e < n) lw[cnt[sp[k] & 4095u] + (sp[k] >> 12)] = w[k];
        }
        __syncthreads();
        // ---- the next bucket's words on their way; rank the placed entries inside their slots, straight to the output
        const unsigned long long obase = a.offs[f];
        if (next_here) load_words(fn, cur ^ 1, n_next);
        for (uint32_t i = tid; i < n; i += XL_BLOCK) {
            const uint64_t wi = lw[i];
            uint32_t slot = ((uint32_t)(wi >> 32) & rmask) >> sshift;
            slot = slot < (uint32_t)XL_SLOTS ? slot : (uint32_t)XL_SLOTS - 1u;
            const uint32_t s0 = cnt[slot], s1 = slot + 1 < (uint32_t)XL_SLOTS ? cnt[slot + 1] : n;
            uint32_t rank = 0;
            bool tie = false;
            for (uint32_t j = s0; j < s1; j++) {
                const uint64_t wj = lw[j];
                rank += wj < wi ? 1u : 0u;
                tie = tie || (((wj ^ wi) >> 32) == 0 && wj != wi);
            }
            if (tie) {   // the same a32 in another entry: the full codes decide (then the row id)
                unsigned special = 0;
                const uint64_t cme = ss_code_of(a.key, (int64_t)(uint32_t)wi, a.desc, &special);
                rank = 0;
                for (uint32_t j = s0; j < s1; j++) {
                    const uint64_t wj = lw[j];
                    if (((wj ^ wi) >> 32) != 0) rank += wj < wi ? 1u : 0u;
                    else if (wj != wi) {
                        const uint64_t cj = ss_code_of(a.key, (int64_t)(uint32_t)wj, a.desc, &special);
                        rank += (cj < cme || (cj == cme && (uint32_t)wj < (uint32_t)wi)) ? 1u : 0u;
                    }
                }
                nties++;
            }
            a.idx_out[obase + s0 + rank] = (int64_t)(uint32_t)wi;
        }
        __syncthreads();
        cur ^= 1; n = n_next;
    }
    if (nties) atomicAdd(&a.flags[5], (unsigned long long)nties);
}

// ---- the entry-word sample sort, stage by stage -----------------------------------------------------------------------------------------------
// What the stages hand to each other.  `pool` and `side` own every block named here: they go back when sample_sort_apx returns.
constexpr size_t XS_LDS1 = ((size_t)SS_B * XS_CAP + XS_K + 1) * 8, XS_LDS2 = (size_t)SS_B * XS_CAP * 8;
struct XsRun {
    vnm_dcol key; int desc; int64_t n; hipStream_t s;
    int has_null; bool trace;
    int l2, qbits, gbits; int64_t nb, m;        // 512 x l2 = 2^(9 + qbits) buckets, m sampled keys, 2^gbits groups of the sample judge the map
    PoolScope pool;
    unsigned long long* flags; XsHdr* hdr; uint64_t* fb;
    XsHdr hh; int xmode; unsigned long long null_counts[2];   // what the sample said; [0] NULL rows of the sample, [1] of the column
    RadixBufs side;                                           // the NULL rows bypass the buckets
    Level1Geometry g; int64_t cap1, cap2; int nt, ready_list;
    uint64_t *w1, *w2; uint32_t *n1, *n2, *todo, *todo_list; unsigned long long* offs;
    int64_t side_len;
};

static void xsort_plan(XsRun* st) {
    int l2 = 8;
    while (l2 < SS_B && st->n / ((int64_t)SS_B * l2) > 4200) l2 *= 2;
    const int64_t want = env_sort_i64("VNM_XSORT_L2", l2);   // (a power of two, 8 .. 512)
    for (l2 = 8; l2 < SS_B && l2 < want;) l2 *= 2;
    st->l2 = l2;
    while ((1 << st->qbits) < l2) st->qbits++;
    st->nb = (int64_t)SS_B * l2;
    st->m = std::min<int64_t>(st->n, env_sort_i64("VNM_XSORT_SAMPLE", (int64_t)1 << 21));
    while (((int64_t)1 << st->gbits) < st->nb / 8 && st->gbits < 15) st->gbits++;
}

static int xsort_allow_lds() {
    static bool attr_set = false;
    if (attr_set) return 0;
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<true, 1, 0>, XS_LDS1));
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<true, 2, 0>, XS_LDS1));
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<true, 1, 1>, XS_LDS1));
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<true, 2, 1>, XS_LDS1));
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<false, 1>, XS_LDS2));
    VNM_TRY(allow_dynamic_lds(xsort_scatter_kernel<false, 2>, XS_LDS2));
    VNM_TRY(allow_dynamic_lds(ssort_local_kernel<1024, 8, 8192, true, true>, (size_t)SS_LOCAL * 12 + 8192 * 4));
    attr_set = true;
    return 0;
}

// Stage 1: the map from a sorted sample, in both spaces, and what the sample says about it.  2 = declined: no map equalises the sample,
// too many equal keys or NULLs, or the rows arrive clustered (*clustered).  The sample itself goes back to the pool on return.
static int xsort_map_from_sample(XsRun* st, bool* clustered) {
    hipStream_t s = st->s;
    const int64_t n = st->n, m = st->m;
    st->flags = (unsigned long long*)st->pool.take(64);
    st->hdr = (XsHdr*)st->pool.take(sizeof(XsHdr));
    st->fb = (uint64_t*)st->pool.take((size_t)(XS_K + 1) * 8 * 2);   // [mode][XS_K + 1]
    if (!st->flags || !st->hdr || !st->fb) return 1;
    unsigned long long* flags = st->flags;
    VNM_HIP(hipMemsetAsync(flags, 0, 64, s));
    VNM_HIP(hipMemsetAsync(st->hdr, 0, sizeof(XsHdr), s));
    const XsHdr& hh = st->hh;
    unsigned long long min_span = ~0ULL;
    RadixBufs sr{};
    VNM_TRY(sorted_sample(st->key, st->desc, n, m, flags + 6, &sr, s));
    const uint64_t* S = sr.code[sr.cur];
    xsort_prep_kernel<<<64, 256, 0, s>>>(S, m, st->hdr, st->key.type, st->desc);
    xsort_map_kernel<<<dim3((XS_K + 1 + 255) / 256, 2), 256, 0, s>>>(S, st->hdr, st->fb, st->key.type, st->desc, (uint64_t)1 << (41 - 9 - st->qbits));
    xsort_balance_kernel<<<dim3((unsigned)((((int64_t)1 << st->gbits) + 255) / 256), 2), 256, 0, s>>>(S, st->hdr, st->fb, st->gbits, st->key.type, st->desc);
    VNM_HIP(hipGetLastError());
    if (st->has_null) ssort_count_nulls_kernel<<<grid_for((n + 7) / 8), 256, 0, s>>>(st->key.validity, st->key.offset, n, flags + 7);
    VNM_TRY(sample_cluster_span(st->key, st->desc, n, S, m, flags + 3, &min_span, s));
    VNM_HIP(hipMemcpyAsync(&st->hh, st->hdr, sizeof(XsHdr), hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(st->null_counts, flags + 6, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    // equal neighbours in the sample: values of multiplicity k leave (k - 1) m^2 / 2n of them -- and every row of such a value would
    // fetch k codes from the key column.  Fetches for up to ~3 % of the rows are accepted.
    const double me = (double)std::max<long long>(1, hh.m_eff);
    const double eq_limit = std::max(16.0, (double)env_sort_i64("VNM_XSORT_EQ_PERMILLE", 15) / 1000.0 * me * me / (double)n);
    const double gmean = me / (double)((int64_t)1 << st->gbits);
    const double glimit = gmean * 1.25 + 6.0 * std::sqrt(gmean) + 8.0;
    int mode = -1;
    for (int q = 0; q < 2; q++)
        if (hh.ok[q] && (double)hh.max_group[q] <= glimit && (mode < 0 || hh.max_group[q] < hh.max_group[mode])) mode = q;
    if (env_sort_i64("VNM_XSORT_MODE", -1) >= 0) { const int want = (int)env_sort_i64("VNM_XSORT_MODE", -1) & 1; mode = hh.ok[want] && (double)hh.max_group[want] <= glimit ? want : -1; }
    // (NULL rows of the sample carry the all-ones code like NaN: with NULLs, a sample without NaN has m - nulls codes in front of them)
    *clustered = rows_arrive_clustered(min_span, (int64_t)hh.m_eff);
    if (*clustered && st->trace) fprintf(stderr, "[sort] entry-word sample sort: the rows arrive clustered (a tile of 4096 consecutive rows spans %llu of %lld samples)\n", min_span, hh.m_eff);
    const bool ok = mode >= 0 && !*clustered && (double)hh.eq_pairs <= eq_limit && hh.m_eff == m - (long long)st->null_counts[0] && (!st->has_null || st->null_counts[1] < (unsigned long long)n / 2);
    if (st->trace) fprintf(stderr, "[sort] entry-word sample sort: sample %lld (%lld in front of NaN), %llu equal neighbours (limit %.0f); largest group of the sample: code cells (2^%lld) %s%llu, "
                                   "value cells %s%llu (mean %.1f, limit %.0f) -> %s\n",
                           (long long)m, hh.m_eff, hh.eq_pairs, eq_limit, hh.sh, hh.ok[0] ? "" : "n/a ", hh.max_group[0], hh.ok[1] ? "" : "n/a ", hh.max_group[1], gmean, glimit,
                           ok ? (mode ? "taken (value cells)" : "taken (code cells)") : "declined");
    st->xmode = mode;
    return ok ? 0 : 2;
}

// Stage 2: level 1, rows -> entry words in 512 buckets per workgroup region.  2 = more level-1 regions than the local sort reads.
static int xsort_level1(XsRun* st) {
    hipStream_t s = st->s;
    const XsHdr& hh = st->hh;
    st->g = level1_geometry(st->n, env_sort_i64("VNM_XSORT_PAIRS1", 2), env_sort_i64("VNM_XSORT_GRID1_PER_CU", 1), env_sort_i64("VNM_XSORT_SPLIT2", 1));
    const int grid1 = st->g.grid1;
    st->cap1 = ((st->g.rows_per_wg / SS_B + st->g.rows_per_wg / SS_B / 4 + 2 * XS_FB * 4) + XS_FB - 1) & ~(int64_t)(XS_FB - 1);
    if (st->g.split2 > XL_MAX_SPLIT) return 2;
    st->w1 = (uint64_t*)st->pool.take((size_t)SS_B * grid1 * st->cap1 * 8);
    st->n1 = (uint32_t*)st->pool.take((size_t)SS_B * grid1 * 4);
    if (!st->w1 || !st->n1) return 1;
    st->nt = (int)env_sort_i64("VNM_XSORT_NT", 0); st->ready_list = (int)env_sort_i64("VNM_XSORT_READY_LIST", 1);
    XsArgs a1{};
    a1.key = st->key; a1.desc = st->desc; a1.nrows = st->n; a1.fb = st->fb; a1.qbits = st->qbits;
    a1.map.mode = st->xmode; a1.map.sh = (int)hh.sh; a1.map.base = hh.base; a1.map.u_lo = hh.u_lo; a1.map.inv_w = hh.inv_w;
    a1.out_words = st->w1; a1.out_counts = st->n1; a1.out_cap = st->cap1; a1.flags = st->flags; a1.nt = st->nt; a1.ready_list = st->ready_list;
    if (st->has_null) {
        const int64_t side_cap = (int64_t)st->null_counts[1] + 64;
        VNM_TRY(radix_alloc(&st->side, side_cap));
        a1.has_null = 1; a1.side = (unsigned long long*)st->side.code[0]; a1.side_cap = side_cap;
    }
    {
        KernelTimer timer("sort_scatter1", s);
        if (st->xmode == 0) {
            if (st->g.pairs1 == 2) xsort_scatter_kernel<true, 2, 0><<<grid1, SS_BLOCK, XS_LDS1, s>>>(a1);
            else xsort_scatter_kernel<true, 1, 0><<<grid1, SS_BLOCK, XS_LDS1, s>>>(a1);
        } else {
            if (st->g.pairs1 == 2) xsort_scatter_kernel<true, 2, 1><<<grid1, SS_BLOCK, XS_LDS1, s>>>(a1);
            else xsort_scatter_kernel<true, 1, 1><<<grid1, SS_BLOCK, XS_LDS1, s>>>(a1);
        }
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

// Stages 3 and 4: level 2 by the next bits of the words, then the buckets' sizes and offsets.  2 = a region or a bucket overflowed.
static int xsort_level2_and_offsets(XsRun* st) {
    hipStream_t s = st->s;
    const int64_t nb = st->nb;
    const int split2 = st->g.split2;
    const int64_t avg_bucket = st->n / nb + 1;
    st->cap2 = ((std::min<int64_t>(SS_LOCAL, avg_bucket * 3 / 2 / split2 + avg_bucket / 4 + 256)) + XS_FB - 1) & ~(int64_t)(XS_FB - 1);
    st->w2 = (uint64_t*)st->pool.take((size_t)nb * split2 * st->cap2 * 8);
    st->n2 = (uint32_t*)st->pool.take((size_t)nb * split2 * 4);
    st->offs = (unsigned long long*)st->pool.take((size_t)(nb + 1) * 8);
    const int nchunks = (int)((nb + XO_CHUNK - 1) / XO_CHUNK);
    unsigned long long* part = (unsigned long long*)st->pool.take((size_t)nchunks * 8);
    st->todo = (uint32_t*)st->pool.take((size_t)nb * 4);
    st->todo_list = (uint32_t*)st->pool.take((size_t)nb * 4);
    if (!st->w2 || !st->n2 || !st->offs || !part || !st->todo || !st->todo_list) return 1;
    VNM_HIP(hipMemsetAsync(st->todo, 0, (size_t)nb * 4, s));
    XsArgs a2{};
    a2.qbits = st->qbits; a2.in_words = st->w1; a2.in_counts = st->n1; a2.in_cap = st->cap1; a2.in_regions = st->g.grid1; a2.in_split = split2;
    a2.out_words = st->w2; a2.out_counts = st->n2; a2.out_cap = st->cap2; a2.flags = st->flags; a2.nt = st->nt; a2.ready_list = st->ready_list;
    {
        KernelTimer timer("sort_scatter2", s);
        if (env_sort_i64("VNM_XSORT_PAIRS2", 2) >= 2) xsort_scatter_kernel<false, 2><<<SS_B * split2, SS_BLOCK, XS_LDS2, s>>>(a2);
        else xsort_scatter_kernel<false, 1><<<SS_B * split2, SS_BLOCK, XS_LDS2, s>>>(a2);
    }
    VNM_HIP(hipGetLastError());
    xsort_sizes_kernel<<<nchunks, 256, 0, s>>>(st->n2, split2, nb, part, st->flags, SS_LOCAL);
    xsort_offsets_kernel<<<nchunks, 256, 0, s>>>(st->n2, split2, nb, part, st->offs);
    VNM_HIP(hipGetLastError());
    unsigned long long fl[3] = {0, 0, 0};
    VNM_HIP(hipMemcpyAsync(fl, st->flags, 24, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (st->trace) fprintf(stderr, "[sort] entry-word sample sort: n %lld grid1 %d cap1 %lld split2 %d cap2 %lld buckets %lld -> fail %llu\n",
                           (long long)st->n, st->g.grid1, (long long)st->cap1, split2, (long long)st->cap2, (long long)nb, fl[0]);
    st->side_len = (int64_t)fl[2];
    return fl[0] ? 2 : 0;
}

// Stage 5: per-bucket LDS sort, straight into the caller's buffer; the NULL rows behind everything
static int xsort_local(XsRun* st, int64_t* idx_out) {
    hipStream_t s = st->s;
    const int cus = device_info().num_cus;
    const int64_t nb = st->nb;
    XlArgs la{};
    la.words = st->w2; la.counts = st->n2; la.cap = st->cap2; la.split = st->g.split2; la.offs = st->offs; la.nbuckets = nb; la.idx_out = idx_out;
    la.key = st->key; la.desc = st->desc; la.rbits = 32 - st->qbits; la.todo = st->todo; la.list = st->todo_list; la.flags = st->flags;
    SsLocalArgs lb{};
    lb.code = st->w2; lb.row = nullptr; lb.counts = st->n2; lb.cap = st->cap2; lb.split = st->g.split2; lb.offs = st->offs; lb.nbuckets = nb; lb.idx_out = idx_out;
    lb.key_out = nullptr; lb.key_type = st->key.type; lb.key_desc = st->desc; lb.flags = st->flags; lb.debug = 0; lb.todo = st->todo; lb.key = st->key; lb.crowded = nullptr; lb.list = st->todo_list; lb.list_n = st->flags + 4;
    {
        KernelTimer timer("sort_local", s);
        xsort_local_kernel<<<(int)std::min<int64_t>(nb, (int64_t)cus * env_sort_i64("VNM_XSORT_LOCAL_PER_CU", 48)), XL_BLOCK, 0, s>>>(la);
        ssort_local_kernel<1024, 8, 8192, true, true><<<(int)std::min<int64_t>(nb, (int64_t)cus * 16), 1024, (size_t)SS_LOCAL * 12 + 8192 * 4, s>>>(lb);
    }
    VNM_HIP(hipGetLastError());
    if (st->has_null && st->side_len > 0) {   // the NULL rows, in row order, behind every value (NaN included): Arrow's SortIndices puts them last in both directions
        st->side.cur = 0;
        if (st->side_len > 1) VNM_TRY(radix_sort_codes(&st->side, st->side_len, s));
        xsort_nulls_kernel<<<grid_for(st->side_len), 256, 0, s>>>((const unsigned long long*)st->side.code[st->side.cur], st->side_len, st->offs + nb, idx_out);
        VNM_HIP(hipGetLastError());
    }
    unsigned long long f8[8];
    VNM_HIP(hipMemcpyAsync(f8, st->flags, 64, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (st->trace) fprintf(stderr, "[sort] entry-word sample sort: %llu buckets through the long kernel, %llu entries ordered through the key column\n", f8[4], f8[5]);
    return 0;
}

// 0 = done, 1 = error, 2 = declined / failed (the caller goes on with the splitter sort); *clustered: the rows arrive clustered
static int sample_sort_apx(const vnm_dcol& key, int desc, int64_t n, int64_t* idx_out, bool* clustered, hipStream_t s) {
    if (n >= ((int64_t)1 << 32)) return 2;
    XsRun st{};
    st.key = key; st.desc = desc; st.n = n; st.s = s; st.has_null = key.validity != nullptr; st.trace = getenv("VNM_SORT_TRACE") != nullptr;
    xsort_plan(&st);
    VNM_TRY(xsort_allow_lds());
    VNM_TRY(xsort_map_from_sample(&st, clustered));
    VNM_TRY(xsort_level1(&st));
    VNM_TRY(xsort_level2_and_offsets(&st));
    return xsort_local(&st, idx_out);
}
