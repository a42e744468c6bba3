// Several input columns in ONE pass over the rows: fixed-point entries of two or three values (round 6; included by vnm_agg.hip
// inside namespace vnm, after vnm_agg_routes.inc).
//
// BaseAggregate::Next (base_aggregate.cpp:23-45) updates every function of a row in one loop.  `SELECT k, sum(a), avg(b), sum(c),
// count(*) ... GROUP BY k` over many groups used to be cut into one dense-path operator per input column (split_program:
// dense_per_column), each re-reading the key and the predicate column: 64 bytes per row read where 32 are needed, plus three sets of
// scatter passes and a join (59 x 2^24 rows, G = 1e6, three columns: 22.5 ms).  What kept the columns apart was the entry size: the
// ring scatter stages whole entries in LDS, and (3 float64 values + code) = 28 bytes leaves one flush block per ring.
// With fixed-point values (every value of a column is m * 2^qe with |m| < 2^31: DPartArgs::fx_q, checked per row) an entry of up to
// THREE values is 16 bytes -- {m1, m2, m3, code remainder} as one fxn_u4 -- and the machinery of the one-column path applies as it
// is: rings of fxn_u4 entries flushed in whole blocks of 16 (256 contiguous bytes), direct-addressed final tables of
// {int64 sum x NV, u32 rows}, integer adds (exact by construction).  The rows are read ONCE: 8 (key) + 8 NV bytes.
//
// Scope: one plain int64 / uint64 key; {COUNT(*), COUNT, SUM, AVG} over two or three plain float64 columns (no NULLs: every count
// is the row count); a float64 predicate column (one of the inputs or its own) or none; one batch or the recorded batches of a
// stream as segments.  No spill buffer: a key outside the sampled code range, a region or a ring that overflows (skew), or a
// value that does not fit the fixed-point words fails the attempt -- nothing has been written to the operator's state -- and the
// batch takes the per-column route as before.  The result of a call is a run (dense partial state in the plan's word layout).
constexpr int FXN_MAXV = 3;
constexpr int FXN_BLOCK = 1024;
constexpr int FXN_FB = 16;                 // entries per flushed block (256 bytes)
typedef uint32_t fxn_u4 __attribute__((ext_vector_type(4)));   // an entry: {m1, m2, m3, code remainder} (a native vector: arrays of it stay in registers)

struct VSegN { const uint64_t* kp; const double* vp[FXN_MAXV]; const double* pp; int64_t nrows; int64_t first_tile; };
typedef const VSegN __attribute__((address_space(4)))* VSegNConst;

struct FxnArgs {
    DenseMap map;
    // pass 1: the rows
    const uint64_t* kp;
    const double* vp[FXN_MAXV];
    const double* pp;             // a predicate column of its own (pred_col < 0)
    int has_pred, pred_col, op;
    double thr;
    int64_t nrows;
    const VSegN* segs;            // the recorded batches of a stream (nseg > 0): segment i owns the sub-tiles from first_tile on
    int nseg;
    int64_t nsub;
    double inv_q[FXN_MAXV];
    // pass 2: the regions pass 1 wrote
    const fxn_u4* in_ent;
    const uint32_t* in_counts;
    int64_t in_cap;
    int in_regions, in_split;
    int in_bits;
    // output regions: region of (partition p, producer b) = p * out_pstride + b
    fxn_u4* out_ent;
    uint32_t* out_counts;
    int64_t out_cap;
    int64_t out_pstride;
    int nparts, out_bits;
    unsigned long long* flags;    // [0] failure (key outside the code range, region / ring overflow)  [7] a value that is not a fixed-point word
    int ready_list;               // the flush walks the round's list of rings that completed a block
};

// FROM_ROWS: pass 1 (filter fused, key -> code', values -> fixed-point words).  NV: values per entry.  PAIRS: pairs of rows (pass 1) or
// of entries (pass 2) per lane and sub-tile.  SEG: pass 1 over the segments of a stream.  PV: a predicate column of its own.
template <bool FROM_ROWS, int NV, int PAIRS, bool SEG, bool PV>
// (one 1024-thread workgroup per CU by its rings: four waves per SIMD, 128 VGPRs each -- left to itself the compiler aims at eight and spills)
__global__ __launch_bounds__(FXN_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void fxn_scatter_kernel(FxnArgs a, int ring_cap) {
    extern __shared__ fxn_u4 fxn_ring[];                 // [np][ring_cap]
    __shared__ uint32_t fill[PT_MAXP], head[PT_MAXP], cursor[PT_MAXP], s_retry[2], s_nready[2];
    __shared__ uint16_t ready[PT_MAXP];
    const RingState<uint32_t> rs{fill, head, cursor, s_retry, s_nready, ready};
    constexpr int NE = 2 * PAIRS;
    const int np = a.nparts, tid = threadIdx.x;
    const uint32_t remmask = (1u << a.out_bits) - 1u;
    ring_init<FXN_BLOCK, PT_MAXP>(rs);
    int ph = 0;
    const bool use_list = a.ready_list != 0;
    __syncthreads();
    int64_t out_base;
    if (FROM_ROWS) out_base = blockIdx.x;
    else { const int pin = blockIdx.x / a.in_split, g = blockIdx.x % a.in_split; out_base = (int64_t)pin * np * a.in_split + g; }
    const int64_t out_stride = FROM_ROWS ? a.out_pstride : a.in_split;
    const uint32_t ocap = (uint32_t)a.out_cap;
    bool failed = false, misfit = false;

    // whole blocks of the rings -> the partition's region: sixteen lanes per partition, one entry (16 bytes) each
    auto flush = [&](bool drain) {
        ring_flush<FXN_FB, 16, FXN_BLOCK, false>(rs, ph, drain, use_list, np, (uint32_t)ring_cap, ocap, [&](int p, uint32_t src, int64_t dst, uint32_t n_here, int j, bool room) {
            if (!room) failed = true;     // (a full region: no spill buffer -- the attempt fails)
            else if ((uint32_t)j < n_here) a.out_ent[(out_base + (int64_t)p * out_stride) * a.out_cap + dst + j] = fxn_ring[(size_t)p * ring_cap + src + j];
        });
    };
    auto rounds = [&](const fxn_u4 (&e)[NE], const uint32_t (&c)[NE], uint32_t okmask) {
        ring_rounds<NE>(rs, ph, okmask, [&](int k) -> bool {
            const uint32_t p = c[k] >> a.out_bits;
            const uint32_t slot = ring_reserve<FXN_FB>(rs, ph, p, (uint32_t)ring_cap, use_list);
            if (slot != RING_FULL) { fxn_u4 w = e[k]; w.w = c[k] & remmask; fxn_ring[(size_t)p * ring_cap + slot] = w; }
            return slot != RING_FULL;
        }, [&]() { flush(false); }, [&](int nr, uint32_t) {
            if (nr >= 6) failed = true;      // (skew: one ring takes a sub-tile's worth of entries -- not this path's business)
            return nr >= 6;
        });
    };

    if (FROM_ROWS) {
        const int64_t sub = (int64_t)NE * FXN_BLOCK;
        struct Cur { const uint64_t* kp; const double* vp0; const double* vp1; const double* vp2; const double* pp; int64_t nrows; int64_t lst; };
        const int nseg = SEG ? a.nseg : 0;
        const VSegNConst segs = (VSegNConst)(uintptr_t)a.segs;
        const int64_t nsub = SEG ? a.nsub : (a.nrows + sub - 1) / sub;
        int sg = 0;
        auto locate = [&](int64_t st, Cur& c) {
            if (SEG) {
                while (sg + 1 < nseg && st >= segs[sg + 1].first_tile) sg++;
                c.kp = segs[sg].kp; c.pp = segs[sg].pp; c.nrows = segs[sg].nrows; c.lst = st - segs[sg].first_tile;
                c.vp0 = segs[sg].vp[0]; c.vp1 = segs[sg].vp[1]; c.vp2 = segs[sg].vp[2];
            } else {
                c.kp = a.kp; c.pp = a.pp; c.nrows = a.nrows; c.lst = st;
                c.vp0 = a.vp[0]; c.vp1 = a.vp[1]; c.vp2 = a.vp[2];
            }
        };
        ulonglong2 kk[PAIRS];
        double2 v0[PAIRS], v1[PAIRS], v2[NV > 2 ? PAIRS : 1], pv[PV ? PAIRS : 1];
        auto load_sub = [&](const Cur& c) {
            if (c.lst < c.nrows / sub) {
#pragma unroll
                for (int u = 0; u < PAIRS; u++) {
                    const int64_t r = c.lst * sub + (int64_t)u * 2 * FXN_BLOCK + 2 * tid;
                    kk[u] = *(const ulonglong2*)(c.kp + r);
                    v0[u] = *(const double2*)(c.vp0 + r);
                    v1[u] = *(const double2*)(c.vp1 + r);
                    if (NV > 2) v2[NV > 2 ? u : 0] = *(const double2*)(c.vp2 + r);
                    if (PV) pv[u] = *(const double2*)(c.pp + r);
                }
            }
        };
        Cur cur{}, nxt{};
        if ((int64_t)blockIdx.x < nsub) { locate(blockIdx.x, cur); load_sub(cur); }
        for (int64_t st = blockIdx.x; st < nsub; st += gridDim.x) {
            fxn_u4 e[NE]; uint32_t c[NE]; uint32_t okmask = 0;
            const bool full = cur.lst < cur.nrows / sub;
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const int u = k >> 1, el = k & 1;
                const int64_t r = cur.lst * sub + (int64_t)u * 2 * FXN_BLOCK + 2 * tid + el;
                e[k] = fxn_u4{0u, 0u, 0u, 0u}; c[k] = 0;
                if (r >= cur.nrows) continue;
                uint64_t key; double x0, x1, x2 = 0.0, p = 0.0;
                if (full) {
                    key = el ? kk[u].y : kk[u].x;
                    x0 = el ? v0[u].y : v0[u].x;
                    x1 = el ? v1[u].y : v1[u].x;
                    if (NV > 2) x2 = el ? v2[NV > 2 ? u : 0].y : v2[NV > 2 ? u : 0].x;
                    if (PV) p = el ? pv[PV ? u : 0].y : pv[PV ? u : 0].x;
                } else {
                    key = cur.kp[r];
                    x0 = cur.vp0[r]; x1 = cur.vp1[r];
                    if (NV > 2) x2 = cur.vp2[r];
                    if (PV) p = cur.pp[r];
                }
                if (a.has_pred) {
                    if (!PV) p = a.pred_col == 0 ? x0 : (a.pred_col == 1 ? x1 : x2);   // (the predicate reads one of the input columns: uniform)
                    if (!cmp_apply<double>(a.op, p, a.thr)) continue;
                }
                const uint64_t d = (key ^ a.map.sign) - a.map.lo_u;
                if (d > (uint64_t)a.map.mask) { failed = true; continue; }     // outside the sampled range: no spill buffer here
                int64_t m0 = 0, m1 = 0, m2 = 0;
                bool fits = fx_encode(x0, a.inv_q[0], &m0);
                fits = fx_encode(x1, a.inv_q[1], &m1) && fits;
                if (NV > 2) fits = fx_encode(x2, a.inv_q[2], &m2) && fits;
                if (!fits) { misfit = true; continue; }
                e[k] = fxn_u4{(uint32_t)(int32_t)m0, (uint32_t)(int32_t)m1, (uint32_t)(int32_t)m2, 0u};
                c[k] = ((uint32_t)d * a.map.mul) & a.map.mask;
                okmask |= 1u << k;
            }
            if (st + gridDim.x < nsub) { locate(st + gridDim.x, nxt); load_sub(nxt); }
            rounds(e, c, okmask);
            cur = nxt;
        }
    } else {
        __shared__ uint32_t rstart[PT_MAX_REGIONS + 1];
        const RingRegions rg = ring_regions<1>(rstart, a.in_counts, a.in_regions, a.in_split, a.in_regions, 1);
        const uint32_t total_in = rg.total;
        const uint32_t inmask = (1u << a.in_bits) - 1u;
        fxn_u4 ev[NE];
        uint32_t okm = 0;
        int reg = 0;
        auto load_ent = [&](uint32_t t0) {
            okm = 0;
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const uint32_t v = t0 + (uint32_t)k * FXN_BLOCK + tid;
                if (v < total_in) {
                    uint32_t e0;
                    const int64_t r = rg.region0 + ring_region_of<1>(rstart, reg, v, &e0);
                    ev[k] = a.in_ent[r * a.in_cap + e0];
                    okm |= 1u << k;
                }
            }
        };
        load_ent(0);
        for (uint32_t t0 = 0; t0 < total_in; t0 += NE * FXN_BLOCK) {
            fxn_u4 e[NE]; uint32_t c[NE];
#pragma unroll
            for (int k = 0; k < NE; k++) { e[k] = ev[k]; c[k] = ev[k].w & inmask; }
            const uint32_t okmask = okm;
            load_ent(t0 + NE * FXN_BLOCK);
            rounds(e, c, okmask);
        }
    }
    flush(true);
    __syncthreads();
    if (tid < np) a.out_counts[out_base + (int64_t)tid * out_stride] = cursor[tid];
    if (__syncthreads_or(failed ? 1 : 0) && tid == 0) __hip_atomic_store(&a.flags[0], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (FROM_ROWS) { if (__syncthreads_or(misfit ? 1 : 0) && tid == 0) __hip_atomic_store(&a.flags[7], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

// Final pass: one workgroup per final partition, {int64 sum x NV, u32 rows} direct-addressed by the entry's slot; the groups leave as
// a run (dense partial state).  Lean like dfx_final_kernel: the next chunk is always in flight, across partition boundaries.
struct FxnFinalArgs {
    DenseMap map;
    const fxn_u4* ent;
    const uint32_t* counts;
    int64_t cap;
    int regions;
    int64_t nfinal;
    double q[FXN_MAXV];
    int w_sum[FXN_MAXV];      // the column's sum word (its compensation word follows), -1: the column is only counted
    int n_cnt;
    int w_cnt[FXN_MAXV + 1];  // every count word of the plan (COUNT(*), COUNT(col)): all equal the row count
    uint64_t* dkey;           // [2][dstride]
    uint64_t* dacc;           // [W][dstride]
    int64_t dstride;
    unsigned long long* flags;   // [0] overflow  [1] groups written
};
template <int NV, int TB>
__global__ __launch_bounds__(TB >= 12 ? 1024 : 512) void fxn_final_kernel(FxnFinalArgs a) {
    constexpr int SLOTS = 1 << TB, BLOCK = TB >= 12 ? 1024 : 512, MAXR = 512, CQ = (MAXR + BLOCK - 1) / BLOCK;
    __shared__ unsigned long long lsum[NV][SLOTS];
    __shared__ uint32_t lcnt[SLOTS];
    __shared__ uint32_t s_cnt[2][MAXR];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = a.regions;
    const int64_t nwork = a.nfinal;
    int buf = 0;
    if ((int64_t)blockIdx.x < nwork) for (int r = tid; r < R && r < MAXR; r += BLOCK) s_cnt[0][r] = a.counts[(int64_t)blockIdx.x * R + r];
    __syncthreads();
    auto first_region = [&](const uint32_t* cnt) { int r = 0; while (r < R && cnt[r] == 0) r++; return r; };
    fxn_u4 pa = fxn_u4{0u, 0u, 0u, 0u}, pb = pa;
    uint32_t na = 0, ia = 0, nb = 0, ib = 0;
    auto load_chunk = [&](int64_t f, int rj, uint32_t ci, uint32_t n, fxn_u4* p) {
        const uint32_t i = ci + tid;
        if (i < n) *p = a.ent[(f * R + rj) * a.cap + i];
    };
    int rj = 0; uint32_t ci = 0;
    bool have = false;
    if ((int64_t)blockIdx.x < nwork) {
        rj = first_region(s_cnt[0]);
        have = rj < R;
        if (have) { na = s_cnt[0][rj]; ia = 0; load_chunk(blockIdx.x, rj, 0, na, &pa); ci = BLOCK; }
    }
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t f = w, wn = w + gridDim.x;
        for (int i = tid; i < SLOTS; i += BLOCK) {
#pragma unroll
            for (int v = 0; v < NV; v++) lsum[v][i] = 0ULL;
            lcnt[i] = 0;
        }
        if (tid == 0) s_n = 0;
        uint32_t cnext[CQ];
        if (wn < nwork) {
#pragma unroll
            for (int q = 0; q < CQ; q++) { const int r = q * BLOCK + tid; cnext[q] = r < R ? a.counts[wn * R + r] : 0u; }
        }
        __syncthreads();
        const uint32_t* cnt = s_cnt[buf];
        while (have) {
            int rn = rj; uint32_t cin = ci;
            while (rn < R && cin >= cnt[rn]) { rn++; cin = 0; }
            const bool more = rn < R;
            if (more) { nb = cnt[rn]; ib = cin; load_chunk(f, rn, cin, nb, &pb); }
            if (ia + tid < na) {
                const uint32_t slot = pa.w & (SLOTS - 1);
                atomicAdd(&lsum[0][slot], (unsigned long long)(long long)(int32_t)pa.x);
                if (NV > 1) atomicAdd(&lsum[NV > 1 ? 1 : 0][slot], (unsigned long long)(long long)(int32_t)pa.y);
                if (NV > 2) atomicAdd(&lsum[NV > 2 ? 2 : 0][slot], (unsigned long long)(long long)(int32_t)pa.z);
                atomicAdd(&lcnt[slot], 1u);
            }
            have = more;
            if (more) { pa = pb; na = nb; ia = ib; rj = rn; ci = cin + BLOCK; }
        }
        if (wn < nwork) {
#pragma unroll
            for (int q = 0; q < CQ; q++) { const int r = q * BLOCK + tid; if (r < R) s_cnt[buf ^ 1][r] = cnext[q]; }
        }
        __syncthreads();
        if (wn < nwork) {
            const uint32_t* cn2 = s_cnt[buf ^ 1];
            rj = first_region(cn2);
            have = rj < R;
            if (have) { na = cn2[rj]; ia = 0; load_chunk(wn, rj, 0, na, &pa); ci = BLOCK; }
        }
        buf ^= 1;
        uint32_t mine = 0;
#pragma unroll
        for (int q = 0; q < SLOTS / BLOCK; q++) mine += lcnt[q * BLOCK + tid] != 0 ? 1u : 0u;
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
            const uint32_t gc = lcnt[i];
            const bool occ = gc != 0;
            const uint64_t b = __ballot(occ);
            uint32_t wbase = 0;
            if (lane == 0 && b) wbase = atomicAdd(&s_n, (uint32_t)__popcll(b));
            wbase = __shfl(wbase, 0);
            if (occ) {
                const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
                const int64_t pos = (int64_t)s_base + wbase + __popcll(b & lt);
                a.dkey[pos] = dense_key_of(a.map, ((uint32_t)f << TB) | (uint32_t)i);
                a.dkey[a.dstride + pos] = 0;
                for (int k = 0; k < a.n_cnt; k++) a.dacc[(int64_t)a.w_cnt[k] * a.dstride + pos] = gc;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    if (a.w_sum[v] < 0) continue;
                    double hi, lo;
                    fx_expand((long long)lsum[v][i], a.q[v], &hi, &lo);
                    a.dacc[(int64_t)a.w_sum[v] * a.dstride + pos] = (uint64_t)__double_as_longlong(hi);
                    a.dacc[(int64_t)(a.w_sum[v] + 1) * a.dstride + pos] = (uint64_t)__double_as_longlong(lo);
                }
            }
        }
        __syncthreads();
    }
}

// host side ------------------------------------------------------------------------------------------------------------------------
// 0 = done (the batch's groups are the handle's run), 2 = not this path (nothing touched), 1 = error
int dense_fxn_aggregate(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, hipStream_t s) {
    if (env_i64("VNM_DENSE_FXN", 1) == 0 || h->fxn_state < 0) return 2;
    const AggPlan& pl = h->plan;
    const int NV = pl.n_cols;
    if (!h->single || pl.n_keys != 1 || NV < 2 || NV > FXN_MAXV || h->rank_aligned || h->kn_valid || h->expr_col >= 0 || h->dense_state != 1) return 2;
    auto plain8 = [](const vnm_dcol& c) { return !c.validity && (c.offset & 1) == 0 && ((uintptr_t)c.values & 15) == 0; };
    if ((keys[0].type != VNM_I64 && keys[0].type != VNM_U64) || !plain8(keys[0])) return 2;
    // the program: COUNT(*) / COUNT / SUM / AVG words only; compensated float sums (the word after a sum word is its compensation word)
    FxnFinalArgs fa{};
    for (int v = 0; v < FXN_MAXV; v++) fa.w_sum[v] = -1;
    for (int o = 0; o < pl.n_ops; o++) {
        const AccOp& op = pl.ops[o];
        if (op.kind == A_COUNT_ROWS || op.kind == A_COUNT_VALID) { if (fa.n_cnt > FXN_MAXV) return 2; fa.w_cnt[fa.n_cnt++] = op.word; }
        else if (op.kind == A_SUM_F64 && op.col >= 0 && op.col < NV && fa.w_sum[op.col] < 0 && pl.merge[op.word] == M_ADD_F64C) fa.w_sum[op.col] = op.word;
        else return 2;
    }
    if (fa.n_cnt == 0) return 2;   // (a group's existence is its row count)
    vnm_dcol cols[FXN_MAXV];
    for (int c = 0; c < NV; c++) {
        cols[c] = inputs[h->col_first_func[c]];
        if (cols[c].type != VNM_F64 || !plain8(cols[c])) return 2;
    }
    int pred_col = -1;
    double thr = 0.0;
    if (h->pred_set) {
        if (!pred || pred->type != VNM_F64 || !plain8(*pred)) return 2;
        for (int c = 0; c < NV; c++) if (pred->values == cols[c].values && pred->offset == cols[c].offset) pred_col = c;
        thr = h->pred_is_float ? h->pred_dval : (double)h->pred_ival;
    }
    const std::vector<vnm_agg::QBatch>* q = h->segs_active;
    if (q) {
        for (const auto& b : *q) {
            if (b.ins.size() != (size_t)h->n_funcs || !plain8(b.key)) return 2;
            for (int c = 0; c < NV; c++) if (b.ins[h->col_first_func[c]].type != VNM_F64 || !plain8(b.ins[h->col_first_func[c]])) return 2;
            if (h->pred_set) {
                if (b.pred.type != VNM_F64 || !plain8(b.pred)) return 2;
                const vnm_dcol& pc = pred_col >= 0 ? b.ins[h->col_first_func[pred_col]] : b.pred;
                if (pred_col >= 0 && (b.pred.values != pc.values || b.pred.offset != pc.offset)) return 2;
            }
        }
    } else if (nrows < env_i64("VNM_FXN_MIN_ROWS", (int64_t)1 << 24)) return 2;   // (every call ends in a run: this is for big batches and streams)
    const int cus = device_info().num_cus;
    // the quanta: a sample of every column of the first batch, once per operator
    if (h->fxn_state == 0) {
        h->fxn_state = -1;
        unsigned long long* d = (unsigned long long*)pool_alloc(64);
        if (!d) return 1;
        unsigned long long got[FXN_MAXV] = {0, 0, 0};
        VNM_HIP(hipMemsetAsync(d, 0, 8 * FXN_MAXV, s));
        const int64_t srows = q ? (*q)[0].nrows : nrows;
        const int64_t m = std::min<int64_t>(srows, 1 << 16);
        for (int c = 0; c < NV; c++)
            fx_sample_kernel<<<(int)std::min<int64_t>((m + 255) / 256, 256), 256, 0, s>>>((const double*)cols[c].values + cols[c].offset, srows, m, d + c);
        VNM_HIP(hipGetLastError());
        VNM_HIP(hipMemcpyAsync(got, d, 8 * FXN_MAXV, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        pool_free(d);
        bool ok = true;
        for (int c = 0; c < NV && ok; c++) {
            const uint32_t xinv = (uint32_t)got[c], xexp = (uint32_t)(got[c] >> 32);
            if (xinv == 0 && xexp == 0) { h->fxn_qe[c] = -16; continue; }
            ok = false;
            if (xexp >= 2047) break;
            const int L = (int)(0xFFFFu - xinv) - 1075, E = (int)xexp - 1022;
            const int spare = 31 - (E - L);
            if (spare < 0) break;
            int qe = L - spare / 2;
            if (qe > 0) qe = 0;
            if (qe < -1000 || E - qe > 31) break;
            h->fxn_qe[c] = qe;
            ok = true;
        }
        if (!ok) return 2;
        h->fxn_state = 1;
    }
    // geometry: 2^tb-slot tables of {int64 x NV, u32}, at most 256 rings of 16-byte entries per level
    const DenseMap& mp = h->dmap;
    int tb = (int)env_i64("VNM_FXN_TBITS", 11);
    tb = std::max(10, std::min(12, tb));
    if (mp.bits - tb > 16) tb = mp.bits - 16;
    if (tb > 12 || mp.bits - tb < 5) return 2;
    const int pbits = mp.bits - tb;
    const int levels = pbits > 8 ? 2 : 1;
    const int p1 = levels == 2 ? pbits / 2 : pbits, p2 = pbits - p1;
    const int np1 = 1 << p1, np2 = levels == 2 ? 1 << p2 : 0;
    auto ring_cap_for = [&](int np) { int cap = (int)((size_t)128 * 1024 / ((size_t)np * 16) / FXN_FB) * FXN_FB; return std::min(cap, 128); };
    const int rcap1 = ring_cap_for(np1), rcap2 = levels == 2 ? ring_cap_for(np2) : 0;
    if (rcap1 < 2 * FXN_FB || (levels == 2 && rcap2 < 2 * FXN_FB)) return 2;
    const int pairs1 = 2;
    const int64_t sub1 = (int64_t)2 * pairs1 * FXN_BLOCK;
    // segments
    PoolScope seg_pool;
    std::vector<VSegN> hseg;
    int64_t nsub = (nrows + sub1 - 1) / sub1;
    const VSegN* dseg = nullptr;
    if (q) {
        hseg.resize(q->size());
        int64_t t = 0;
        for (size_t i = 0; i < q->size(); i++) {
            const auto& b = (*q)[i];
            VSegN& g = hseg[i];
            g.kp = (const uint64_t*)b.key.values + b.key.offset;
            for (int c = 0; c < FXN_MAXV; c++) { const vnm_dcol& x = b.ins[h->col_first_func[c < NV ? c : 0]]; g.vp[c] = (const double*)x.values + x.offset; }
            g.pp = h->pred_set ? (const double*)b.pred.values + b.pred.offset : nullptr;
            g.nrows = b.nrows; g.first_tile = t;
            t += (b.nrows + sub1 - 1) / sub1;
        }
        nsub = t;
        VSegN* d = (VSegN*)seg_pool.take(hseg.size() * sizeof(VSegN));
        if (!d) return 1;
        VNM_HIP(hipMemcpyAsync(d, hseg.data(), hseg.size() * sizeof(VSegN), hipMemcpyHostToDevice, s));
        dseg = d;
    }
    const int grid1 = (int)std::min<int64_t>((int64_t)cus * 2, nsub);
    int split2 = std::max(2, (grid1 + PT_MAX_REGIONS - 1) / PT_MAX_REGIONS);
    split2 = std::max(split2, std::min(grid1, (cus * 2 + np1 - 1) / np1));
    const int64_t subs_per_wg = (nsub + grid1 - 1) / grid1;
    const int64_t rows_per_wg = subs_per_wg * sub1;
    int64_t cap1 = ((rows_per_wg / np1 + rows_per_wg / np1 / 5 + 512) + 15) & ~15LL;
    if (((cap1 / 16) & 1) == 0) cap1 += 16;
    if (levels == 1 && grid1 > 512) return 2;     // (the final pass keeps the counts of a partition's regions in LDS)
    PoolScope pool;
    // (declared after the scopes: runs first on every way out -- nothing a launched kernel still reads or writes goes back to the pool early)
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { (void)hipStreamSynchronize(s); } } sync_on_exit{s};
    unsigned long long* flags = (unsigned long long*)pool.take(128);
    fxn_u4* e1 = (fxn_u4*)pool.take((size_t)np1 * grid1 * cap1 * 16);
    uint32_t* n1 = (uint32_t*)pool.take((size_t)np1 * grid1 * 4);
    if (!flags || !e1 || !n1) return 1;
    if (h->pending && complete_pending(h, s)) return 1;     // (this path makes a run of its own)
    if (h->have_run && merge_run_into_table(h, s)) return 1;
    VNM_HIP(hipMemsetAsync(flags, 0, 128, s));
    FxnArgs d1{};
    d1.map = mp;
    d1.kp = (const uint64_t*)keys[0].values + keys[0].offset;
    for (int c = 0; c < FXN_MAXV; c++) { const vnm_dcol& x = cols[c < NV ? c : 0]; d1.vp[c] = (const double*)x.values + x.offset; d1.inv_q[c] = std::ldexp(1.0, -h->fxn_qe[c < NV ? c : 0]); }
    d1.pp = h->pred_set ? (const double*)pred->values + pred->offset : nullptr;
    d1.has_pred = h->pred_set ? 1 : 0; d1.pred_col = pred_col; d1.op = h->pred_op; d1.thr = thr;
    d1.nrows = nrows; d1.segs = dseg; d1.nseg = q ? (int)q->size() : 0; d1.nsub = nsub;
    d1.out_ent = e1; d1.out_counts = n1; d1.out_cap = cap1; d1.out_pstride = grid1;
    d1.nparts = np1; d1.out_bits = mp.bits - p1;
    d1.flags = flags; d1.ready_list = (int)env_i64("VNM_FXN_READY_LIST", 1) & 1;
    const bool pv = h->pred_set && pred_col < 0;
    {
        KernelTimer timer("agg_part_scatter1", s);
        const size_t lds = (size_t)np1 * rcap1 * 16;
#define VNM_FXN1(NV_, SEG_, PV_)                                                                                        \
    do {                                                                                                              \
        VNM_HIP(hipFuncSetAttribute((const void*)fxn_scatter_kernel<true, NV_, 2, SEG_, PV_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        fxn_scatter_kernel<true, NV_, 2, SEG_, PV_><<<grid1, FXN_BLOCK, lds, s>>>(d1, rcap1);                          \
    } while (0)
#define VNM_FXN1_S(NV_) do { if (q) { if (pv) VNM_FXN1(NV_, true, true); else VNM_FXN1(NV_, true, false); } else { if (pv) VNM_FXN1(NV_, false, true); else VNM_FXN1(NV_, false, false); } } while (0)
        if (NV == 2) VNM_FXN1_S(2); else VNM_FXN1_S(3);
#undef VNM_FXN1_S
#undef VNM_FXN1
        VNM_HIP(hipGetLastError());
    }
    const fxn_u4* fin_e = e1; const uint32_t* fin_n = n1;
    int64_t fin_cap = cap1;
    int fin_regions = grid1;
    if (levels == 2) {
        const int64_t per_pg = (int64_t)grid1 * rows_per_wg / np1 / split2;
        int64_t cap2 = ((per_pg / np2 + per_pg / np2 / 4 + 256) + 15) & ~15LL;
        if (((cap2 / 16) & 1) == 0) cap2 += 16;
        fxn_u4* e2 = (fxn_u4*)pool.take((size_t)np1 * np2 * split2 * cap2 * 16);
        uint32_t* n2 = (uint32_t*)pool.take((size_t)np1 * np2 * split2 * 4);
        if (!e2 || !n2) return 1;
        FxnArgs d2{};
        d2.map = mp;
        d2.in_ent = e1; d2.in_counts = n1; d2.in_cap = cap1; d2.in_regions = grid1; d2.in_split = split2; d2.in_bits = mp.bits - p1;
        d2.out_ent = e2; d2.out_counts = n2; d2.out_cap = cap2;
        d2.nparts = np2; d2.out_bits = tb;
        d2.flags = flags; d2.ready_list = ((int)env_i64("VNM_FXN_READY_LIST", 1) >> 1) & 1;
        {
            KernelTimer timer("agg_part_scatter2", s);
            const size_t lds = (size_t)np2 * rcap2 * 16;
            if (NV == 2) {
                VNM_HIP(hipFuncSetAttribute((const void*)fxn_scatter_kernel<false, 2, 2, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                fxn_scatter_kernel<false, 2, 2, false, false><<<np1 * split2, FXN_BLOCK, lds, s>>>(d2, rcap2);
            } else {
                VNM_HIP(hipFuncSetAttribute((const void*)fxn_scatter_kernel<false, 3, 2, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                fxn_scatter_kernel<false, 3, 2, false, false><<<np1 * split2, FXN_BLOCK, lds, s>>>(d2, rcap2);
            }
            VNM_HIP(hipGetLastError());
        }
        fin_e = e2; fin_n = n2; fin_cap = cap2; fin_regions = split2;
    }
    // the scatter passes have to be known good before anything is written for the handle
    unsigned long long fl[8];
    VNM_HIP(hipMemcpyAsync(fl, flags, 64, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (fl[0] || fl[7]) {
        h->fxn_state = -1;
        route_note("dense:fixed_point_columns_failed", "%s: the batch takes the per-column route", fl[7] ? "a value that is not a 31-bit multiple of its column's quantum" : "a key outside the code range or an overflowing ring / region");
        return 2;
    }
    const int64_t dstride = std::min<int64_t>(h->dense_span, nrows) + 2;
    uint64_t* rk = (uint64_t*)pool.take((size_t)dstride * 8 * 2);
    uint64_t* ra = (uint64_t*)pool.take((size_t)dstride * 8 * pl.n_words);
    if (!rk || !ra) return 1;
    fa.map = mp;
    fa.ent = fin_e; fa.counts = fin_n; fa.cap = fin_cap; fa.regions = fin_regions; fa.nfinal = (int64_t)1 << pbits;
    for (int c = 0; c < FXN_MAXV; c++) fa.q[c] = std::ldexp(1.0, h->fxn_qe[c < NV ? c : 0]);
    fa.dkey = rk; fa.dacc = ra; fa.dstride = dstride; fa.flags = flags;
    {
        KernelTimer timer("agg_part_final", s);
#define VNM_FXNF(NV_, TB_)                                                                                             \
    do {                                                                                                              \
        const int blk = TB_ >= 12 ? 1024 : 512;                                                                       \
        int occ = 0;                                                                                                  \
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)fxn_final_kernel<NV_, TB_>, blk, 0) != hipSuccess || occ < 1) occ = 1; \
        const int g3 = (int)std::min<int64_t>(fa.nfinal, (int64_t)cus * std::min(occ, 8));                            \
        fxn_final_kernel<NV_, TB_><<<g3, blk, 0, s>>>(fa);                                                            \
    } while (0)
        if (NV == 2) { if (tb == 10) VNM_FXNF(2, 10); else if (tb == 11) VNM_FXNF(2, 11); else VNM_FXNF(2, 12); }
        else { if (tb == 10) VNM_FXNF(3, 10); else if (tb == 11) VNM_FXNF(3, 11); else VNM_FXNF(3, 12); }
#undef VNM_FXNF
        VNM_HIP(hipGetLastError());
    }
    VNM_HIP(hipMemcpyAsync(fl, flags, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (fl[0]) return set_error("aggregate: fixed-point final pass overflowed its output (internal error)");
    route_note("dense:fixed_point_columns", "%d columns in 16-byte entries (quanta 2^%d, 2^%d, 2^%d), 2^%d codes, 2^%d-slot tables, %d level(s)%s", NV, h->fxn_qe[0], h->fxn_qe[1],
               NV > 2 ? h->fxn_qe[2] : 0, mp.bits, tb, levels, q ? ", stream segments" : "");
    pool.keep(rk); pool.keep(ra);
    adopt_run(h, rk, ra, dstride, (int64_t)fl[1]);
    return 0;
}
