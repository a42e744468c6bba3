// Sort / top-K for gfx950.
//
// Replaces Sort::Sorted (vinum_cpp/src/operators/sort/sort.cpp:15-63): arrow::compute::SortIndices over
// SortOptions{(column, Ascending|Descending)...} followed by compute::Take.  Semantics pinned by the golden
// vectors generated through the real reference (tests/golden/sort_*.arrow): stable; per key, values first,
// then NaN, then NULL -- for BOTH directions.
//
//   * every key column is turned into an order-preserving unsigned 64-bit code (DESC = complemented code)
//     plus a 2-bit class (0 value, 1 NaN, 2 NULL);
//   * full sort: stable LSD radix sort of (code, row id), 8 bits per pass, key columns from last to first: the encode kernel
//     also produces all eight digit histograms, each pass is ONE kernel (chained scan over the tiles, "onesweep"), passes
//     whose digit is identical for every row are skipped, the first pass makes up the identity row ids and the last one
//     writes int64 row ids straight into the caller's buffer;
//   * LIMIT K on a single key: a threshold taken from a sorted sample selects ~K..4K candidates in one scan
//     of the column (8 B/row), only the candidates are sorted -- identical first K rows (ties keep row
//     order) as the reference's full sort + SliceOperator (vinum/core/algebra.py:229-247).
// Roofline: HBM.  top-K: 8*N read; full sort: 8 B/row read + 8 written by the encode, 12 B/row read + 12 B/row written per
// executed pass (8 + 12 for the first, 12 + 8 for the last).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "vnm_common.hpp"

namespace vnm {


// ---- key encoding ---------------------------------------------------------------------------------------
// negzero (optional): set when the row holds -0.0 (its code is that of +0.0, so the value cannot be rebuilt from the code)
__device__ __forceinline__ void encode_key(const vnm_dcol& c, int64_t row, int desc, uint64_t* code, uint32_t* cls, bool* negzero = nullptr) {
    if (!col_valid(c, row)) { *code = 0; *cls = 2; return; }
    uint64_t e;
    if (type_is_float(c.type)) {
        double d = col_f64(c, row);
        if (d != d) { *code = 0; *cls = 1; return; }
        if (negzero && d == 0.0 && __double_as_longlong(d) != 0) *negzero = true;
        if (d == 0.0) d = 0.0;  // -0.0 and +0.0 compare equal in Arrow's sort: ties keep row order
        e = enc_f64(d);
    } else if (type_is_unsigned(c.type)) {
        e = (uint64_t)col_i64(c, row);
    } else {
        e = enc_i64(col_i64(c, row));
    }
    *code = desc ? ~e : e;
    *cls = 0;
}

// Digit histograms of one wave's codes into the workgroup's LDS table h[8][256] (all 64 lanes hold an element).
// The upper bytes of real keys are often identical across a wave: one add of 64 instead of 64 same-address adds.
__device__ __forceinline__ void hist8_wave(uint32_t* h, uint64_t c, int lane) {
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const uint32_t dg = (uint32_t)(c >> (8 * b)) & 255u;
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg);
        if (__ballot(dg != first) == 0) { if (lane == 0) atomicAdd(&h[b * 256 + first], 64u); }
        else atomicAdd(&h[b * 256 + dg], 1u);
    }
}

// code[i] (and cls[i] when cls != NULL) for row idx[i] (idx == NULL: identity); class_codes: code[i] = the row's class
// (0 value, 1 NaN, 2 NULL) instead -- the input of the class pass
// any_cls (optional): bit 0 set when some row is NaN or NULL (class != 0) -- lets the caller skip the class pass; bit 1 when some
// row is -0.0
// ghist (optional): the eight digit histograms of the codes are accumulated on the way (radix_sort_codes then needs no
// histogram pass of its own: one read of the codes less)
__global__ __launch_bounds__(256) void sort_encode_kernel(vnm_dcol c, int desc, const uint32_t* idx, int64_t n, uint64_t* code, uint8_t* cls,
                                                          unsigned long long* any_cls, unsigned long long* ghist, int class_codes) {
    __shared__ uint32_t h[8 * 256];
    if (ghist) {
        for (int i = threadIdx.x; i < 8 * 256; i += 256) h[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t nfull = n & ~63LL;
    bool special = false, negz = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t e; uint32_t k;
        encode_key(c, idx ? (int64_t)idx[i] : i, desc, &e, &k, &negz);
        if (class_codes) e = k;
        code[i] = e;
        if (cls) cls[i] = (uint8_t)k;
        special = special || k != 0;
        if (ghist) {
            if (i < nfull) hist8_wave(h, e, lane);   // i < nfull is uniform across the wave (64-aligned chunks)
            else {
#pragma unroll
                for (int b = 0; b < 8; b++) atomicAdd(&h[b * 256 + ((uint32_t)(e >> (8 * b)) & 255u)], 1u);
            }
        }
    }
    if (any_cls && __ballot(special) && lane == 0) atomicOr(any_cls, 1ULL);
    if (any_cls && __ballot(negz) && lane == 0) atomicOr(any_cls, 2ULL);   // bit 1: a -0.0 (the codes do not carry its sign)
    if (ghist) {
        __syncthreads();
        for (int i = threadIdx.x; i < 8 * 256; i += 256)
            if (h[i]) atomicAdd(&ghist[i], (unsigned long long)h[i]);
    }
}

__global__ void sort_iota_kernel(uint32_t* idx, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) idx[i] = (uint32_t)i;
}
// a 4-byte sort key as the 8-byte key of the same order: float32 -> float64 (exact), int32 / uint32 sign- / zero-extended
__global__ __launch_bounds__(256) void sort_widen_key_kernel(const void* src, int type, int64_t first, int64_t n, uint64_t* dst) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t k = first + i;
        uint64_t v;
        if (type == VNM_F32) v = (uint64_t)__double_as_longlong((double)((const float*)src)[k]);
        else if (type == VNM_I32) v = (uint64_t)(int64_t)((const int32_t*)src)[k];
        else v = ((const uint32_t*)src)[k];
        dst[i] = v;
    }
}
__global__ void sort_widen_kernel(const uint32_t* idx, int64_t n, int64_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int64_t)idx[i];
}

// ---- onesweep: one histogram pre-pass for all eight digits, then ONE kernel per executed pass ------------------------
// r01 ran three kernels per pass (per-block histogram: a full extra read of the codes, scan, scatter): 8 x 2.2 ms of the
// 83 ms went into re-reading the keys for histograms.  The digit histograms of the WHOLE array do not depend on the order
// of the elements, so a single pre-pass computes all eight (radix_hist_all_kernel), a 256-thread kernel turns them into
// exclusive digit bases, and each scatter pass finds its tile's offset inside every digit with a chained scan over the
// tiles that ran before it (decoupled look-back, one status word per tile and digit: tag | prefix-flag | count).  Tiles are
// handed out by an atomic ticket, so tile t - 1 is always resident or finished when tile t looks back.
constexpr int OS_BLOCK = 512;                    // 8 waves; two workgroups per CU (74 KB of LDS each)
constexpr int OS_SUB = 16;                       // elements per lane and tile
constexpr int OS_WAVES = OS_BLOCK / 64;
constexpr int OS_TILE = OS_BLOCK * OS_SUB;       // 8192 elements: ~32 per digit -> 256-B code runs, 128-B row-id runs
constexpr unsigned long long OS_PREFIX = 1ULL << 59;
constexpr unsigned long long OS_VAL_MASK = OS_PREFIX - 1;
constexpr unsigned long long OS_TAG_MASK = 0xFULL << 60;
constexpr size_t OS_LDS_BYTES = (size_t)OS_TILE * 8 + (size_t)OS_WAVES * 256 * 4 + 2 * 256 * 4;

__global__ __launch_bounds__(256) void radix_hist_all_kernel(const uint64_t* code, int64_t n, unsigned long long* ghist) {
    __shared__ uint32_t h[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += 256) h[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t nfull = n & ~63LL;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nfull; i += stride) hist8_wave(h, code[i], lane);   // whole waves only
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - nfull)) {
        const uint64_t c = code[nfull + threadIdx.x];
#pragma unroll
        for (int b = 0; b < 8; b++) atomicAdd(&h[b * 256 + ((uint32_t)(c >> (8 * b)) & 255u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += 256)
        if (h[i]) atomicAdd(&ghist[i], (unsigned long long)h[i]);
}

// ghist[8][256] -> exclusive scan per digit position (the first output slot of every digit value)
__global__ __launch_bounds__(256) void radix_bases_kernel(const unsigned long long* ghist, unsigned long long* bases) {
    __shared__ unsigned long long wt[4];
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    for (int b = 0; b < 8; b++) {
        const unsigned long long x = ghist[b * 256 + d];
        unsigned long long inc = x;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) { const unsigned long long o = __shfl_up(inc, k); if (lane >= k) inc += o; }
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        unsigned long long add = 0;
        for (int w = 0; w < wave; w++) add += wt[w];
        bases[b * 256 + d] = add + inc - x;
        __syncthreads();
    }
}

struct OsArgs {
    const uint64_t* code;
    const uint32_t* val;
    int64_t n, ntiles;
    int shift;
    const unsigned long long* base;   // [256] exclusive digit bases of this pass
    unsigned long long* status;       // [ntiles][256]
    unsigned int* ticket;
    unsigned long long tag;           // (pass + 1) << 60: status words of other passes read as "not published yet"
    uint64_t* code_out;
    uint32_t* val_out;
    int64_t* idx_out;                 // last pass of the last key: row ids widened to int64 straight into the caller's buffer
    uint64_t* key_out;                // ... and (optional) the sorted values of key 0 rebuilt from their codes: saves the caller a gather
    int key_type, key_desc;
};

// Tile shapes tried on 1e9 fp64 keys (ms per pass): 512 x 16 (this one) 6.1; 1024 threads x 8 9.4 (spills at 64 VGPRs);
// 512 x 8 = 4096-element tiles, three workgroups per CU 8.0 (runs half as long).
__global__ __launch_bounds__(OS_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void onesweep_kernel(OsArgs a) {
    extern __shared__ uint64_t os_lds[];
    uint64_t* stage = os_lds;                                  // [OS_TILE] codes by digit; reused for the row ids
    uint32_t* stage32 = (uint32_t*)os_lds;
    uint32_t* wcnt = (uint32_t*)(os_lds + OS_TILE);            // [OS_WAVES][256] per-wave digit counts -> bases
    uint32_t* off = wcnt + OS_WAVES * 256;                     // [256] start of each digit inside the staged tile
    uint32_t* tot = off + 256;                                 // [256] elements of each digit in this tile
    __shared__ unsigned long long run[256];                    // global output position of the tile's first element of each digit
    __shared__ uint32_t wtot[4];
    __shared__ uint32_t s_tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* mycnt = wcnt + wave * 256;
    for (;;) {
        if (tid == 0) s_tile = atomicAdd(a.ticket, 1u);
        for (int i = tid; i < OS_WAVES * 256; i += OS_BLOCK) wcnt[i] = 0;
        __syncthreads();
        const int64_t t = (int64_t)s_tile;
        if (t >= a.ntiles) break;
        const int64_t base = t * OS_TILE;
        const int64_t hi = base + OS_TILE < a.n ? base + OS_TILE : a.n;
        // ---- load + rank inside the wave (wave w owns elements [w * 1024, (w + 1) * 1024) of the tile)
        uint64_t c[OS_SUB];
        uint32_t v[OS_SUB], lp[OS_SUB / 2];   // lp: two 16-bit positions per register
        const int64_t wbase = base + (int64_t)wave * (64 * OS_SUB) + lane;
#pragma unroll
        for (int k = 0; k < OS_SUB; k++) {
            const int64_t i = wbase + k * 64;
            c[k] = i < hi ? a.code[i] : 0;
            v[k] = i < hi ? (a.val ? a.val[i] : (uint32_t)i) : 0;   // val == NULL: the rows are still in their original order
        }
#pragma unroll
        for (int k = 0; k < OS_SUB; k++) {
            const bool in = wbase + k * 64 < hi;
            const uint32_t dg = (uint32_t)(c[k] >> a.shift) & 255u;
            uint64_t m = __ballot(in);
#pragma unroll
            for (int bit = 0; bit < 8; bit++) {
                const uint64_t bb = __ballot((dg >> bit) & 1u);
                m &= ((dg >> bit) & 1u) ? bb : ~bb;
            }
            const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            uint32_t lpos = 0;
            if (in) {
                lpos = mycnt[dg] + before;                    // LDS ops of one wave execute in order
                if (before == 0) mycnt[dg] += (uint32_t)__popcll(m);
            }
            if ((k & 1) == 0) lp[k >> 1] = lpos; else lp[k >> 1] |= lpos << 16;
        }
        __syncthreads();
        // ---- per digit: wave counts -> exclusive bases over the waves, tile total (published at once), digit offsets
        if (tid < 256) {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < OS_WAVES; w++) { const uint32_t x = wcnt[w * 256 + tid]; wcnt[w * 256 + tid] = s; s += x; }
            tot[tid] = s;
            __hip_atomic_store(&a.status[t * 256 + tid], a.tag | (t == 0 ? OS_PREFIX : 0ULL) | (unsigned long long)s, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            uint32_t inc = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            off[tid] = inc - s;
            if (lane == 63) wtot[wave] = inc;
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t add = 0;
            for (int w = 0; w < wave; w++) add += wtot[w];
            off[tid] += add;
        }
        __syncthreads();
        // ---- stage the codes by digit
#pragma unroll
        for (int k = 0; k < OS_SUB; k++) {
            if (wbase + k * 64 < hi) {
                const uint32_t dg = (uint32_t)(c[k] >> a.shift) & 255u;
                const uint32_t pos = ((lp[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) + off[dg] + mycnt[dg];
                lp[k >> 1] = (lp[k >> 1] & (0xFFFFu << (16 * ((k & 1) ^ 1)))) | (pos << (16 * (k & 1)));
                stage[pos] = c[k];
            }
        }
        // ---- chained scan over the earlier tiles (one thread per digit value)
        if (tid < 256) {
            unsigned long long excl = 0;
            if (t > 0) {
                int64_t look = t - 1;
                for (;;) {
                    const unsigned long long sv = __hip_atomic_load(&a.status[look * 256 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((sv & OS_TAG_MASK) != a.tag) { __builtin_amdgcn_s_sleep(1); continue; }
                    excl += sv & OS_VAL_MASK;
                    if (sv & OS_PREFIX) break;
                    look--;
                }
                __hip_atomic_store(&a.status[t * 256 + tid], a.tag | OS_PREFIX | (excl + tot[tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            run[tid] = a.base[tid] + excl;
        }
        __syncthreads();
        // ---- copy the codes out in runs; remember each element's digit for the row-id round
        const uint32_t total = (uint32_t)(hi - base);
        uint32_t dgs[OS_SUB / 4];
#pragma unroll
        for (int j = 0; j < OS_SUB; j++) {
            const uint32_t i = (uint32_t)tid + (uint32_t)j * OS_BLOCK;
            uint32_t dg = 0;
            if (i < total) {
                const uint64_t cc = stage[i];
                dg = (uint32_t)(cc >> a.shift) & 255u;
                if (a.code_out) a.code_out[run[dg] + (i - off[dg])] = cc;
                if (a.key_out) {
                    const uint64_t e = a.key_desc ? ~cc : cc;
                    a.key_out[run[dg] + (i - off[dg])] = a.key_type == VNM_F64 ? (uint64_t)__double_as_longlong(dec_f64(e))
                                                       : (a.key_type == VNM_I64 ? (uint64_t)dec_i64(e) : e);
                }
            }
            if ((j & 3) == 0) dgs[j >> 2] = dg; else dgs[j >> 2] |= dg << (8 * (j & 3));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < OS_SUB; k++)
            if (wbase + k * 64 < hi) stage32[(lp[k >> 1] >> (16 * (k & 1))) & 0xFFFFu] = v[k];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < OS_SUB; j++) {
            const uint32_t i = (uint32_t)tid + (uint32_t)j * OS_BLOCK;
            if (i < total) {
                const uint32_t dg = (dgs[j >> 2] >> (8 * (j & 3))) & 255u;
                const unsigned long long pos = run[dg] + (i - off[dg]);
                if (a.idx_out) a.idx_out[pos] = (int64_t)stage32[i];
                else a.val_out[pos] = stage32[i];
            }
        }
        __syncthreads();
    }
}

struct RadixBufs {
    PoolScope pool;                   // owns the blocks below: they go back when the RadixBufs' scope ends (early returns included)
    uint64_t* code[2];
    uint32_t* val[2];
    unsigned long long* red;          // [0..1] unused, [4] caller's flag word, [8..15] tickets (as uint32 pairs)
    unsigned long long* ghist;        // [8][256] digit histograms of the whole array, then [8][256] exclusive bases
    unsigned long long* status;       // [ntiles][256] chained-scan status words
    int cur = 0;
    int64_t ntiles = 0;
};

static int radix_alloc(RadixBufs* r, int64_t n) {
    r->ntiles = (n + OS_TILE - 1) / OS_TILE;
    for (int k = 0; k < 2; k++) {
        r->code[k] = (uint64_t*)r->pool.take((size_t)(n ? n : 1) * 8);
        r->val[k] = (uint32_t*)r->pool.take((size_t)(n ? n : 1) * 4);
        if (!r->code[k] || !r->val[k]) return 1;
    }
    r->red = (unsigned long long*)r->pool.take(128);
    r->ghist = (unsigned long long*)r->pool.take((size_t)2 * 8 * 256 * 8);
    r->status = (unsigned long long*)r->pool.take((size_t)(r->ntiles ? r->ntiles : 1) * 256 * 8);
    return (r->red && r->ghist && r->status) ? 0 : 1;
}

// raises a kernel's dynamic-LDS limit; every kernel family does it once, in front of its first launch
template <class Kernel>
static int allow_dynamic_lds(Kernel kernel, size_t bytes) {
    VNM_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// sort (code[cur], val[cur]) stably by the bytes of code that are not constant
// extra (optional): receives r->red[4], a flag word the caller's previous kernel may have set (read back with the
// same synchronisation as the digit histograms)
// hist_ready: r->ghist already holds the digit histograms of the codes (sort_encode_kernel accumulated them)
// ident (optional, in/out): the row ids r->val[r->cur] are the identity and NOT materialised; the first executed pass makes them up
// last (optional): what the LAST pass of the whole sort may write on its way, see RadixLastPass
struct RadixLastPass {
    int64_t* idx_out;     // the caller's int64 row-id buffer.  When this call runs the last pass of the whole sort (no class pass will
    bool* wrote_idx;      // follow: !cls_possible or the flag word is 0) that pass writes the widened row ids straight into it and skips
                          // the code output; *wrote_idx tells the caller
    uint64_t* key_out;    // see OsArgs::key_out; only when the flag word says the key holds no NaN / NULL / -0.0: *wrote_key
    int key_type, key_desc;
    bool* wrote_key;
};
static int radix_sort_codes(RadixBufs* r, int64_t n, hipStream_t s, unsigned long long* extra = nullptr, bool cls_possible = false,
                            bool hist_ready = false, bool* ident = nullptr, const RadixLastPass* last = nullptr) {
    if (last && last->wrote_key) *last->wrote_key = false;
    if (last && last->wrote_idx) *last->wrote_idx = false;
    if (n <= 1) { if (extra) { VNM_HIP(hipMemcpyAsync(extra, r->red + 4, 8, hipMemcpyDeviceToHost, s)); VNM_HIP(hipStreamSynchronize(s)); } return 0; }
    static bool attr_set = false;   // (the one place: onesweep_kernel is launched from this function alone)
    if (!attr_set) {
        VNM_TRY(allow_dynamic_lds(onesweep_kernel, OS_LDS_BYTES));
        attr_set = true;
    }
    const int cus = device_info().num_cus;
    // ---- histograms of all eight digits in one read of the codes; status words and tickets cleared meanwhile
    unsigned long long hist[8 * 256 + 1];
    if (!hist_ready) VNM_HIP(hipMemsetAsync(r->ghist, 0, (size_t)8 * 256 * 8, s));
    VNM_HIP(hipMemsetAsync(r->red + 8, 0, 64, s));
    const int64_t ntiles = (n + OS_TILE - 1) / OS_TILE;   // <= r->ntiles: callers may sort fewer elements than they allocated for
    VNM_HIP(hipMemsetAsync(r->status, 0, (size_t)ntiles * 256 * 8, s));
    {
        KernelTimer timer("radix_hist", s);
        int g = cus * 8;
        const int64_t need = (n + 255) / 256;
        if (g > need) g = (int)need;
        if (!hist_ready) radix_hist_all_kernel<<<g, 256, 0, s>>>(r->code[r->cur], n, r->ghist);
        radix_bases_kernel<<<1, 256, 0, s>>>(r->ghist, r->ghist + 8 * 256);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(hist, r->ghist, (size_t)8 * 256 * 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(hist + 8 * 256, r->red + 4, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (extra) *extra = hist[8 * 256];
    const bool cls_follows = cls_possible && (hist[8 * 256] & 1ULL) != 0;
    int live[8], n_live = 0;
    for (int byte = 0; byte < 8; byte++) {
        bool constant = false;      // one digit value holds every element: nothing to reorder
        for (int d = 0; d < 256 && !constant; d++) constant = hist[byte * 256 + d] == (unsigned long long)n;
        if (!constant) live[n_live++] = byte;
    }
    int g = (int)std::min<int64_t>(ntiles, (int64_t)cus * 2);
    for (int k = 0; k < n_live; k++) {
        const int byte = live[k];
        KernelTimer timer("radix_pass", s);
        OsArgs a{};
        a.code = r->code[r->cur]; a.val = (ident && *ident) ? nullptr : r->val[r->cur]; a.n = n; a.ntiles = ntiles; a.shift = 8 * byte;
        a.base = r->ghist + 8 * 256 + byte * 256;
        a.status = r->status;
        a.ticket = (unsigned int*)(r->red + 8) + byte;
        a.tag = (unsigned long long)(byte + 1) << 60;
        a.code_out = r->code[r->cur ^ 1]; a.val_out = r->val[r->cur ^ 1];
        if (last && last->idx_out && !cls_follows && k == n_live - 1) {
            a.idx_out = last->idx_out; a.code_out = nullptr;
            if (last->wrote_idx) *last->wrote_idx = true;
            if (last->key_out && hist[8 * 256] == 0) {
                a.key_out = last->key_out; a.key_type = last->key_type; a.key_desc = last->key_desc;
                if (last->wrote_key) *last->wrote_key = true;
            }
        }
onesweep_kernel<<<g, OS_BLOCK, OS_LDS_BYTES, s>>>(a);
        r->cur ^= 1;
        if (ident) *ident = false;
    }
    VNM_HIP(hipGetLastError());
    return 0;
}


// ---- LIMIT K without the launch-bound tail ------------------------------------------------------------------------------
// r01's top-K query spent 1.35 ms in the selection scan and 1.5 ms in ~130 tiny radix launches (sorting the 2^18-key
// sample to read ONE threshold off it, then sorting a few hundred candidates three times).  Both small problems fit one
// workgroup each:
//   * topk_blockbest_kernel + one workgroup sort: the threshold is the r-th best of 4096 block winners of a 2^22-key sample
//     (a single-workgroup radix SELECT over the whole sample was tried first: 0.8 ms at 2^18 keys -- its LDS histogram
//     atomics all hit the few bins the keys' top bytes share);
//   * topk_small_sort_kernel: bitonic sort of up to 8192 candidates in LDS on the composite key (class, code, row id) --
//     the row id makes it the stable order of the full sort -- and the first K row ids go straight to the output.
// Block-best sampling: the m-key strided sample is cut into TB_BLOCKS blocks and only the BEST key of every block is kept.
// The r-th best of those block winners is a threshold with AT LEAST r rows at or above it (the r winners themselves) and
// about r * n / m in expectation while r << TB_BLOCKS -- the same statistic as the r-th order statistic of the sample,
// found by sorting 4096 keys in one workgroup instead of the whole sample.
constexpr int TB_BLOCKS = 4096;
__global__ __launch_bounds__(256) void topk_blockbest_kernel(vnm_dcol c, int desc, int64_t n, int64_t m, uint64_t* best_code, uint8_t* best_cls) {
    const int64_t per = (m + TB_BLOCKS - 1) / TB_BLOCKS;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    uint64_t bc = ~0ULL;
    uint32_t bk = 255;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const int64_t row = (int64_t)(((__int128)i * n) / m);
        uint64_t e; uint32_t k;
        encode_key(c, row, desc, &e, &k);
        if (k < bk || (k == bk && e < bc)) { bk = k; bc = e; }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t oc = __shfl_xor(bc, d);
        const uint32_t ok = __shfl_xor(bk, d);
        if (ok < bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; }
    }
    __shared__ uint64_t sc[4];
    __shared__ uint32_t sk[4];
    if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = bc; sk[threadIdx.x >> 6] = bk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) if (sk[w] < bk || (sk[w] == bk && sc[w] < bc)) { bk = sk[w]; bc = sc[w]; }
        best_code[blockIdx.x] = bc;
        best_cls[blockIdx.x] = (uint8_t)bk;
    }
}

constexpr int TS_MAX = 8192;
// thr (optional): instead of row ids, write the (class, code) of the element at sorted position `limit` to thr[0], thr[1]
__global__ __launch_bounds__(1024) void topk_small_sort_kernel(const uint64_t* code, const uint8_t* cls, const uint32_t* rows, int n, int np2,
                                                              int64_t limit, int64_t* out, unsigned long long* thr) {
    extern __shared__ uint64_t ts_lds[];
    uint64_t* k_code = ts_lds;                         // [np2]
    uint32_t* k_row = (uint32_t*)(ts_lds + np2);       // [np2]
    uint8_t* k_cls = (uint8_t*)(k_row + np2);          // [np2]
    const int tid = threadIdx.x;
    for (int i = tid; i < np2; i += 1024) {
        const bool in = i < n;
        k_code[i] = in ? code[i] : ~0ULL;
        k_row[i] = in ? (rows ? rows[i] : (uint32_t)i) : 0xFFFFFFFFu;
        k_cls[i] = in ? cls[i] : (uint8_t)255;         // padding sorts last
    }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < np2 / 2; t += 1024) {
                const int lo = 2 * t - (t & (stride - 1));   // index with bit `stride` clear
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint8_t ca = k_cls[lo], cb = k_cls[hi];
                const uint64_t xa = k_code[lo], xb = k_code[hi];
                const uint32_t ra = k_row[lo], rb = k_row[hi];
                const bool a_gt_b = ca != cb ? ca > cb : (xa != xb ? xa > xb : ra > rb);
                if (a_gt_b == up) {
                    k_cls[lo] = cb; k_cls[hi] = ca;
                    k_code[lo] = xb; k_code[hi] = xa;
                    k_row[lo] = rb; k_row[hi] = ra;
                }
            }
            __syncthreads();
        }
    }
    if (thr) {
        if (tid == 0) { thr[0] = k_cls[limit]; thr[1] = k_code[limit]; }
        return;
    }
    for (int64_t i = tid; i < limit; i += 1024) out[i] = (int64_t)k_row[i];
}

// ---- top-K candidate selection ----------------------------------------------------------------------------
__global__ void topk_sample_kernel(vnm_dcol c, int desc, int64_t n, int64_t m, uint64_t* code, uint8_t* cls) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        int64_t row = (int64_t)(((__int128)i * n) / m);
        uint64_t e; uint32_t k;
        encode_key(c, row, desc, &e, &k);
        code[i] = e;
        cls[i] = (uint8_t)k;
    }
}

// keep rows whose (class, code) <= (t_cls, t_code); unordered append of (code, class, row).
// Candidates are collected in a per-wave LDS buffer and appended with ONE atomic per 256 candidates: a
// returning atomic per wave-with-survivors saturates the shared counter (~90/us) once K reaches ~1e6.
// Four independent rows per lane keep the column reads in flight.
constexpr int TK_U = 4;
constexpr int TK_BUF = 256;
__global__ __launch_bounds__(256) void topk_select_kernel(vnm_dcol c, int desc, int64_t n, uint32_t t_cls, uint64_t t_code, int64_t cap,
                                                          unsigned long long* count, uint64_t* code, uint8_t* cls, uint32_t* rows) {
    __shared__ uint64_t b_code[4][TK_BUF];
    __shared__ uint32_t b_row[4][TK_BUF];
    __shared__ uint8_t b_cls[4][TK_BUF];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ULL : (~0ULL >> (64 - lane));
    uint32_t fill = 0;  // wave-uniform
    auto flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned long long)fill);
        base = __shfl(base, 0);
        for (uint32_t j = lane; j < fill; j += 64) {
            int64_t pos = (int64_t)base + j;
            if (pos < cap) { code[pos] = b_code[wave][j]; cls[pos] = b_cls[wave][j]; rows[pos] = b_row[wave][j]; }
        }
        __builtin_amdgcn_wave_barrier();
        fill = 0;
    };
    const int64_t tile_rows = 256 * TK_U;
    const int64_t ntiles = (n + tile_rows - 1) / tile_rows;
    const bool fast = c.type == VNM_F64 && !c.validity && (c.offset & 1) == 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint64_t e[TK_U];
        uint32_t k[TK_U];
        bool keep[TK_U];
        int64_t rowi[TK_U];
        if (fast && (t + 1) * tile_rows <= n) {
            // float64 without NULLs: a lane owns pairs of adjacent rows, 16 bytes per request
            const double* p = (const double*)c.values + c.offset + t * tile_rows + 2 * threadIdx.x;
#pragma unroll
            for (int u = 0; u < TK_U / 2; u++) {
                const double2 d = *(const double2*)(p + u * 512);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    double x = h ? d.y : d.x;
                    const int q = 2 * u + h;
                    rowi[q] = t * tile_rows + u * 512 + 2 * threadIdx.x + h;
                    if (x != x) { e[q] = 0; k[q] = 1; }
                    else {
                        if (x == 0.0) x = 0.0;  // -0.0 and +0.0 tie (see encode_key)
                        const uint64_t enc = enc_f64(x);
                        e[q] = desc ? ~enc : enc;
                        k[q] = 0;
                    }
                    keep[q] = k[q] < t_cls || (k[q] == t_cls && e[q] <= t_code);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < TK_U; u++) {
                int64_t i = t * tile_rows + u * 256 + threadIdx.x;
                rowi[u] = i;
                e[u] = 0; k[u] = 0; keep[u] = false;
                if (i < n) {
                    encode_key(c, i, desc, &e[u], &k[u]);
                    keep[u] = k[u] < t_cls || (k[u] == t_cls && e[u] <= t_code);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TK_U; u++) {
            uint64_t b = __ballot(keep[u]);
            if (!b) continue;
            uint32_t cnt = (uint32_t)__popcll(b);
            if (fill + cnt > TK_BUF) flush();
            if (keep[u]) {
                uint32_t slot = fill + (uint32_t)__popcll(b & lt);
                b_code[wave][slot] = e[u];
                b_cls[wave][slot] = (uint8_t)k[u];
                b_row[wave][slot] = (uint32_t)rowi[u];
            }
            fill += cnt;
        }
    }
    if (fill) flush();
}

__global__ void gather_u8_kernel(const uint8_t* src, const uint32_t* idx, int64_t n, uint64_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[idx[i]];
}
__global__ void gather_u64_kernel(const uint64_t* src, const uint32_t* idx, int64_t n, uint64_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[idx[i]];
}
__global__ void gather_i64_kernel(const int64_t* src, const int64_t* idx, int64_t n, int64_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[idx[i]];
}
__global__ void gather_u32_kernel(const uint32_t* src, const uint32_t* idx, int64_t n, uint32_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[idx[i]];
}
__global__ void u32_to_code_kernel(const uint32_t* src, int64_t n, uint64_t* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = src[i];
}

__global__ void take_kernel(vnm_dcol c, const int64_t* idx, int64_t n, void* out, uint8_t* out_valid) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int w = type_width(c.type);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int64_t r = idx[i];
        uint64_t bits = col_raw_bits(c, r);
        switch (w) {
            case 8: ((uint64_t*)out)[i] = bits; break;
            case 4: ((uint32_t*)out)[i] = (uint32_t)bits; break;
            case 2: ((uint16_t*)out)[i] = (uint16_t)bits; break;
            default: ((uint8_t*)out)[i] = (uint8_t)bits; break;
        }
        if (out_valid) out_valid[i] = col_valid(c, r);
    }
}

static int64_t env_sort_i64(const char* name, int64_t dflt) {
    const char* v = getenv(name);
    return v ? atoll(v) : dflt;
}

static int grid_for(int64_t n, int per_cu = 8) {
    int g = device_info().num_cus * per_cu;
    int64_t need = (n + 255) / 256;
    if (need < 1) need = 1;
    return g > need ? (int)need : g;
}

#include "vnm_ring.inc"
#include "vnm_sort_sample.inc"
#include "vnm_sort_apx.inc"

// A column that arrives clustered is often simply SORTED already (a time series ordered by its timestamp).  One pass counts the rows
// whose code is below their predecessor's; none: the order asked for is the row order (stable: equal keys keep it), the indices are 0 .. n - 1.
// (out[0]: rows below their predecessor, out[1]: rows above or EQUAL to it -- none of the latter: the column is strictly in the opposite order,
//  and without ties the stable answer is the row numbers backwards)
__global__ __launch_bounds__(256) void sort_inversions_kernel(vnm_dcol key, int desc, int64_t n, unsigned long long* out) {
    unsigned special = 0;
    unsigned int below = 0, not_below = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += stride) {
        const bool b = ss_code_of(key, i, desc, &special) < ss_code_of(key, i - 1, desc, &special);
        below += b ? 1u : 0u; not_below += b ? 0u : 1u;
    }
    for (int o = 32; o > 0; o >>= 1) { below += __shfl_xor(below, o); not_below += __shfl_xor(not_below, o); }
    if ((threadIdx.x & 63) == 0) { if (below) atomicAdd(out, (unsigned long long)below); if (not_below) atomicAdd(out + 1, (unsigned long long)not_below); }
}
__global__ void sort_iota64_kernel(int64_t* idx, int64_t n, int backwards) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) idx[i] = backwards ? n - 1 - i : i;
}

// ---- the splitter sample sort of one 8-byte key (kernels: vnm_sort_sample.inc), stage by stage -----------------------------------------
// What the stages hand to each other.  `pool` and `side` own every block named here: they go back when sample_sort returns.
constexpr size_t SS_SCATTER_LDS = (size_t)SS_B * SS_CAP * 12;
struct SsRun {
    vnm_dcol key; int desc; int64_t n; hipStream_t s;
    int has_null;                               // the key has a validity bitmap
    int l2; int64_t nb, m;                      // 512 x l2 buckets, m sampled keys
    PoolScope pool;
    uint64_t *split, *heavy; unsigned long long *flags, *lb, *hstart; unsigned int *hb, *nheavy_d;
    int nheavy; int64_t sample_nulls, total_nulls; unsigned long long eq_pairs;   // what the sample said
    RadixBufs side; int64_t side_cap, side_len;                                   // rows of heavy codes and NULL rows bypass the buckets
    Level1Geometry g; int64_t cap1, cap2;
    uint64_t *c1, *c2; uint32_t *r1, *n1, *r2, *n2; unsigned long long* offs;     // the regions of the two levels, the bucket offsets
    unsigned long long special;                                                   // flags[1] after the scatters: a NaN / -0.0 key
};

// buckets and sample size
static void ssort_plan(SsRun* st) {
    const int64_t n = st->n;
    // 512 x l2 buckets of ~2100-4200 rows: 2^18 at 1e9 rows, fewer below (2^18 buckets whatever n cost ~4.5 ms of fixed time:
    // the 2^23-key sample and 2^18 nearly empty local-sort workgroups; 1.7e7 rows 5.2 ms against 1.4 with the LSD passes)
    int l2 = 8;
    while (l2 < SS_B && n / ((int64_t)SS_B * l2) > 4200) l2 *= 2;
    st->l2 = (int)std::min<int64_t>(SS_B, std::max<int64_t>(8, env_sort_i64("VNM_SSORT_L2", l2)));
    st->nb = (int64_t)SS_B * st->l2;
    // Samples per bucket: a bucket's share of the rows is ~Gamma(k) / k for k samples per bucket, and a bucket beyond the local
    // sort's room (r times the mean) fails the whole attempt -- P ~ exp(-k (r - 1 - ln r)) per bucket.  At 1e9 rows r = 8192 / 3815
    // = 2.15: with k = 32 about one data set in ten lost a bucket among its 2^18 (and paid the LSD sort on top of the wasted
    // passes: 119 ms); k is chosen for P * buckets < 1e-7.
    const double mean = (double)n / (double)st->nb;
    const double r = std::min<double>((double)SS_LOCAL, 2.5 * mean + 128.0) / mean;
    const double need = (std::log((double)st->nb) + 16.0) / std::max(0.05, r - 1.0 - std::log(r));
    const int64_t k = std::min<int64_t>(128, std::max<int64_t>(32, (int64_t)std::ceil(need)));
    st->m = std::min<int64_t>(n, st->nb * env_sort_i64("VNM_SSORT_SAMPLES_PER_BUCKET", k));
}

static int ssort_allow_lds() {
    static bool attr_set = false;
    if (attr_set) return 0;
    VNM_TRY(allow_dynamic_lds(ssort_scatter_kernel<true, 1>, SS_SCATTER_LDS));
    VNM_TRY(allow_dynamic_lds(ssort_scatter_kernel<false, 1>, SS_SCATTER_LDS));
    VNM_TRY(allow_dynamic_lds(ssort_scatter_kernel<true, 2>, SS_SCATTER_LDS));
    VNM_TRY(allow_dynamic_lds(ssort_scatter_kernel<false, 2>, SS_SCATTER_LDS));
    VNM_TRY(allow_dynamic_lds(ssort_local_kernel<512, 10, 4096, false>, (size_t)SS_SMALL * 12 + 4096 * 4));
    VNM_TRY(allow_dynamic_lds(ssort_local_kernel<1024, 8, 8192, true>, (size_t)SS_LOCAL * 12 + 8192 * 4));
    attr_set = true;
    return 0;
}

// Stage 1: splitters from a sorted sample; heavy codes = runs of equal splitters.  2 = declined: too many NULLs or heavy values, or the
// rows arrive clustered (*clustered).  The sample itself goes back to the pool on return.
static int ssort_splitters(SsRun* st, bool* clustered) {
    hipStream_t s = st->s;
    const int64_t m = st->m, nb = st->nb;
    st->split = (uint64_t*)st->pool.take((size_t)nb * 8);
    st->flags = (unsigned long long*)st->pool.take(64);
    st->heavy = (uint64_t*)st->pool.take((size_t)SS_MAX_HEAVY * 8);
    st->lb = (unsigned long long*)st->pool.take((size_t)(SS_MAX_HEAVY + 2) * 8 * 2);   // lb[66], then hstart[65] (+ the NULL class)
    st->hb = (unsigned int*)st->pool.take((size_t)(SS_MAX_HEAVY + 2) * 4);             // hb[64], then the heavy counter
    if (!st->split || !st->flags || !st->heavy || !st->lb || !st->hb) return 1;
    st->hstart = st->lb + SS_MAX_HEAVY + 2;
    st->nheavy_d = st->hb + SS_MAX_HEAVY;
    unsigned long long* flags = st->flags;
    VNM_HIP(hipMemsetAsync(flags, 0, 64, s));
    VNM_HIP(hipMemsetAsync(st->nheavy_d, 0, 4, s));
    RadixBufs sr{};
    VNM_TRY(sorted_sample(st->key, st->desc, st->n, m, flags + 5, &sr, s));
    int64_t m_valid = m;     // NULL rows of the sample stand at the end of its sorted order: the splitters come from the rest
    if (st->has_null) {
        unsigned long long sn = 0, tn = 0;
        ssort_count_nulls_kernel<<<grid_for((st->n + 7) / 8), 256, 0, s>>>(st->key.validity, st->key.offset, st->n, flags + 6);
        VNM_HIP(hipMemcpyAsync(&sn, flags + 5, 8, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipMemcpyAsync(&tn, flags + 6, 8, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        st->sample_nulls = (int64_t)sn;
        st->total_nulls = (int64_t)tn;
        m_valid = m - st->sample_nulls;
        if (m_valid < nb * 4) {
            if (getenv("VNM_SORT_TRACE")) fprintf(stderr, "[sort] sample sort declined: %lld of %lld sampled rows are NULL\n", (long long)st->sample_nulls, (long long)m);
            return 2;
        }
    }
    ssort_splitters_kernel<<<(int)((nb + 255) / 256), 256, 0, s>>>(sr.code[sr.cur], m_valid, nb, st->split, flags, st->heavy, st->nheavy_d);
    VNM_HIP(hipGetLastError());
    unsigned long long min_span = ~0ULL, too_many = 0;
    VNM_TRY(sample_cluster_span(st->key, st->desc, st->n, sr.code[sr.cur], m_valid, flags + 7, &min_span, s));
    unsigned int nh = 0;
    uint64_t hcodes[SS_MAX_HEAVY];
    VNM_HIP(hipMemcpyAsync(&st->eq_pairs, flags + 3, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(&too_many, flags, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(&nh, st->nheavy_d, 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(hcodes, st->heavy, sizeof(hcodes), hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (rows_arrive_clustered(min_span, m_valid)) {
        *clustered = true;
        if (getenv("VNM_SORT_TRACE")) fprintf(stderr, "[sort] sample sort declined: the rows arrive clustered (a tile of 4096 consecutive rows spans %llu of %lld samples)\n", min_span, (long long)m_valid);
        return 2;
    }
    if (too_many || nh > (unsigned int)SS_MAX_HEAVY || getenv("VNM_SSORT_NO_HEAVY") != nullptr && nh) {
        if (getenv("VNM_SORT_TRACE")) fprintf(stderr, "[sort] sample sort declined: %u heavily duplicated values\n", nh);
        return 2;
    }
    st->nheavy = (int)nh;
    if (st->nheavy) {
        std::sort(hcodes, hcodes + st->nheavy);
        VNM_HIP(hipMemcpyAsync(st->heavy, hcodes, (size_t)st->nheavy * 8, hipMemcpyHostToDevice, s));
    }
    return 0;
}

// Stage 2: level 1, rows -> 512 buckets per workgroup region
static int ssort_level1(SsRun* st) {
    const int64_t n = st->n;
    const bool bypass = st->nheavy || st->has_null;
    // rows of heavy codes bypass the buckets: (heavy index << 32 | row id) entries in a side list, sorted below
    // (room: every run of r equal splitters stands for at most (r + 1) buckets' worth of rows)
    // (+ the NULL rows, counted)
    st->side_cap = bypass ? std::min<int64_t>(n, (int64_t)((double)(st->eq_pairs + 2 * (unsigned long long)st->nheavy) * (double)n / (double)st->nb * 1.3 + (double)st->total_nulls) + 65536) : 0;
    if (bypass) VNM_TRY(radix_alloc(&st->side, st->side_cap));
    st->g = level1_geometry(n, env_sort_i64("VNM_SSORT_PAIRS1", 1), env_sort_i64("VNM_SSORT_GRID1_PER_CU", 1), env_sort_i64("VNM_SSORT_SPLIT2", 1));
    const int grid1 = st->g.grid1;
    st->cap1 = ((st->g.rows_per_wg / SS_B + st->g.rows_per_wg / SS_B / 4 + 96) + 7) & ~7LL;
    st->c1 = (uint64_t*)st->pool.take((size_t)SS_B * grid1 * st->cap1 * 8);
    st->r1 = (uint32_t*)st->pool.take((size_t)SS_B * grid1 * st->cap1 * 4);
    st->n1 = (uint32_t*)st->pool.take((size_t)SS_B * grid1 * 4);
    if (!st->c1 || !st->r1 || !st->n1) return 1;
    SsArgs a1{};
    a1.key = st->key; a1.desc = st->desc; a1.nrows = n; a1.split = st->split; a1.l2 = st->l2;
    a1.out_code = st->c1; a1.out_row = st->r1; a1.out_counts = st->n1; a1.out_cap = st->cap1; a1.flags = st->flags;
    a1.heavy = st->heavy; a1.nheavy = st->nheavy; a1.has_null = st->has_null;
    a1.side = bypass ? (unsigned long long*)st->side.code[0] : nullptr; a1.side_cap = st->side_cap;
    {
        KernelTimer timer("sort_scatter1", st->s);
        if (st->g.pairs1 == 2) ssort_scatter_kernel<true, 2><<<grid1, SS_BLOCK, SS_SCATTER_LDS, st->s>>>(a1);
        else ssort_scatter_kernel<true, 1><<<grid1, SS_BLOCK, SS_SCATTER_LDS, st->s>>>(a1);
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

// Stage 3: level 2, every level-1 bucket -> l2 buckets.  2 = a region of either level overflowed.
static int ssort_level2(SsRun* st) {
    hipStream_t s = st->s;
    const int64_t nb = st->nb;
    const int split2 = st->g.split2;
    const int64_t avg_bucket = st->n / nb + 1;
    st->cap2 = ((std::min<int64_t>(SS_LOCAL, avg_bucket * 2 / split2 + avg_bucket / 2 + 128)) + 7) & ~7LL;
    st->c2 = (uint64_t*)st->pool.take((size_t)nb * split2 * st->cap2 * 8);
    st->r2 = (uint32_t*)st->pool.take((size_t)nb * split2 * st->cap2 * 4);
    st->n2 = (uint32_t*)st->pool.take((size_t)nb * split2 * 4);
    st->offs = (unsigned long long*)st->pool.take((size_t)(nb + 1) * 8);
    if (!st->c2 || !st->r2 || !st->n2 || !st->offs) return 1;
    SsArgs a2{};
    a2.split = st->split; a2.l2 = st->l2; a2.in_code = st->c1; a2.in_row = st->r1; a2.in_counts = st->n1; a2.in_cap = st->cap1; a2.in_regions = st->g.grid1; a2.in_split = split2;
    a2.out_code = st->c2; a2.out_row = st->r2; a2.out_counts = st->n2; a2.out_cap = st->cap2; a2.flags = st->flags;
    {
        KernelTimer timer("sort_scatter2", s);
        if (env_sort_i64("VNM_SSORT_PAIRS2", 1) >= 2) ssort_scatter_kernel<false, 2><<<SS_B * split2, SS_BLOCK, SS_SCATTER_LDS, s>>>(a2);
        else ssort_scatter_kernel<false, 1><<<SS_B * split2, SS_BLOCK, SS_SCATTER_LDS, s>>>(a2);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long fl[3] = {0, 0, 0};
    VNM_HIP(hipMemcpyAsync(fl, st->flags, 24, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    st->special = fl[1];
    st->side_len = (int64_t)fl[2];
    if (fl[0]) {
        if (getenv("VNM_SORT_TRACE")) fprintf(stderr, "[sort] sample sort: a region overflowed (side list %llu of %lld, %lld NULL rows, %lld of %lld samples NULL, %d heavy values), LSD sort instead\n",
                                              fl[2], (long long)st->side_cap, (long long)st->total_nulls, (long long)st->sample_nulls, (long long)st->m, st->nheavy);
        return 2;
    }
    return 0;
}

// Stage 4: where every bucket starts in the output.  The heavy rows: their side list sorted by (heavy index, row id) is their part of
// the output.  2 = a bucket outgrew the local sort's room.
static int ssort_offsets(SsRun* st) {
    hipStream_t s = st->s;
    if (st->nheavy || st->has_null) {
        st->side.cur = 0;
        if (st->side_len > 1) VNM_TRY(radix_sort_codes(&st->side, st->side_len, s));
        ssort_heavy_bounds_kernel<<<1, 128, 0, s>>>((const unsigned long long*)st->side.code[st->side.cur], st->side_len, st->heavy, st->nheavy, st->split, st->nb, st->lb, st->hb, st->has_null);
    }
    ssort_offsets_kernel<<<1, 1024, 0, s>>>(st->n2, st->g.split2, st->nb, st->offs, st->flags, st->nheavy, st->hb, st->lb, st->hstart, st->has_null);
    VNM_HIP(hipGetLastError());
    unsigned long long fail = 0;
    VNM_HIP(hipMemcpyAsync(&fail, st->flags, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (getenv("VNM_SORT_TRACE")) fprintf(stderr, "[sort] sample sort: n %lld grid1 %d cap1 %lld split2 %d cap2 %lld heavy %d (%lld rows) -> fail %llu special %llu\n",
                                          (long long)st->n, st->g.grid1, (long long)st->cap1, st->g.split2, (long long)st->cap2, st->nheavy, (long long)st->side_len, fail, st->special);
    return fail ? 2 : 0;
}

// VNM_SSORT_DEBUG = 7 / 8 (after the scatters): is every row in exactly one region of level 2 / 1?  6 (after the local sort): its counters
static int ssort_debug(SsRun* st, bool after_local_sort) {
    const int dbg = (int)env_sort_i64("VNM_SSORT_DEBUG", 0);
    hipStream_t s = st->s;
    const int64_t n = st->n;
    if (after_local_sort && dbg == 6) {
        unsigned long long f6[8];
        VNM_HIP(hipMemcpy(f6, st->flags, 64, hipMemcpyDeviceToHost));
        fprintf(stderr, "[sort] debug: %llu positions beyond the end (max %llu), %llu in the long path\n", f6[2], f6[3], f6[4]);
    }
    if (after_local_sort || (dbg != 7 && dbg != 8)) return 0;
    uint32_t* seen = (uint32_t*)st->pool.take((size_t)n * 4);
    if (!seen) return 1;
    VNM_HIP(hipMemsetAsync(seen, 0, (size_t)n * 4, s));
    VNM_HIP(hipMemsetAsync(st->flags + 4, 0, 8, s));
    if (dbg == 7) ssort_check_kernel<<<4096, 256, 0, s>>>(st->r2, st->n2, st->cap2, st->nb * st->g.split2, seen, n, st->flags + 4);
    else ssort_check_kernel<<<4096, 256, 0, s>>>(st->r1, st->n1, st->cap1, (int64_t)SS_B * st->g.grid1, seen, n, st->flags + 4);
    std::vector<uint32_t> hs((size_t)n);
    unsigned long long badv = 0;
    VNM_HIP(hipMemcpy(hs.data(), seen, (size_t)n * 4, hipMemcpyDeviceToHost));
    VNM_HIP(hipMemcpy(&badv, st->flags + 4, 8, hipMemcpyDeviceToHost));
    int64_t miss = 0, dup = 0, firstmiss = -1;
    for (int64_t i = 0; i < n; i++) { if (hs[i] == 0) { if (firstmiss < 0) firstmiss = i; miss++; } else if (hs[i] > 1) dup++; }
    fprintf(stderr, "[sort] debug level %d regions: %lld rows missing (first %lld), %lld duplicated, %llu out of range\n", dbg == 7 ? 2 : 1,
            (long long)miss, (long long)firstmiss, (long long)dup, badv);
    return 0;
}

// Stage 5: per-bucket LDS sort, straight into the caller's buffers
static int ssort_local(SsRun* st, int64_t* idx_out, uint64_t* key_out, bool* wrote_key) {
    hipStream_t s = st->s;
    const int cus = device_info().num_cus;
    const int64_t nb = st->nb;
    SsLocalArgs la{};
    la.code = st->c2; la.row = st->r2; la.counts = st->n2; la.cap = st->cap2; la.split = st->g.split2; la.offs = st->offs; la.nbuckets = nb;
    la.idx_out = idx_out;
    const bool keyed = key_out != nullptr && st->special == 0 && !st->has_null;   // (a sorted key column with NULLs in it: the caller gathers)
    la.key_out = keyed ? key_out : nullptr; la.key_type = st->key.type; la.key_desc = st->desc; la.flags = st->flags;
    la.debug = (int)env_sort_i64("VNM_SSORT_DEBUG", 0);
    la.crowded = (uint32_t*)st->pool.take((size_t)nb * 4);
    if (!la.crowded) return 1;
    VNM_HIP(hipMemsetAsync(la.crowded, 0, (size_t)nb * 4, s));
    {
        KernelTimer timer("sort_local", s);
        ssort_local_kernel<512, 10, 4096, false><<<(int)std::min<int64_t>(nb, (int64_t)cus * 64), 512, (size_t)SS_SMALL * 12 + 4096 * 4, s>>>(la);
        ssort_local_kernel<1024, 8, 8192, true><<<(int)std::min<int64_t>(nb, (int64_t)cus * 16), 1024, (size_t)SS_LOCAL * 12 + 8192 * 4, s>>>(la);
        if ((st->nheavy || st->has_null) && st->side_len > 0)
            ssort_heavy_write_kernel<<<grid_for(st->side_len), 256, 0, s>>>((const unsigned long long*)st->side.code[st->side.cur], st->side_len, st->heavy, st->lb, st->hstart, idx_out,
                                                                            keyed ? key_out : nullptr, st->key.type, st->desc, st->nheavy);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    VNM_TRY(ssort_debug(st, true));
    if (wrote_key) *wrote_key = keyed;
    return 0;
}

// Sample sort of one 8-byte key (see vnm_sort_sample.inc).  0 = done (idx_out written, *wrote_key), 1 = error, 2 = not applicable / a
// bucket outgrew its room (the caller sorts with the LSD passes); *clustered: declined because the rows arrive clustered.
static int sample_sort(const vnm_dcol& key, int desc, int64_t n, int64_t* idx_out, uint64_t* key_out, bool* wrote_key, bool* clustered, hipStream_t s) {
    if (wrote_key) *wrote_key = false;
    SsRun st{};
    st.key = key; st.desc = desc; st.n = n; st.s = s; st.has_null = key.validity != nullptr;
    ssort_plan(&st);
    VNM_TRY(ssort_allow_lds());
    VNM_TRY(ssort_splitters(&st, clustered));
    VNM_TRY(ssort_level1(&st));
    VNM_TRY(ssort_level2(&st));
    VNM_TRY(ssort_offsets(&st));
    VNM_TRY(ssort_debug(&st, false));
    return ssort_local(&st, idx_out, key_out, wrote_key);
}

// full stable multi-key sort; result: row ids (uint32) in r->val[r->cur]
// idx_out (optional): int64 output buffer; *wrote_idx = the last radix pass wrote it (else the caller widens r->val[r->cur])
// key_out (optional, with idx_out): the sorted values of key 0 (8-byte types, no NaN / NULL / -0.0 in it): *wrote_key
static int full_sort(int n_keys, const vnm_dcol* keys, const int* orders, int64_t n, RadixBufs* r, hipStream_t s,
                     int64_t* idx_out = nullptr, bool* wrote_idx = nullptr, uint64_t* key_out = nullptr, bool* wrote_key = nullptr) {
    if (wrote_idx) *wrote_idx = false;
    if (wrote_key) *wrote_key = false;
    const int kt0 = keys[0].type;
    if (!(kt0 == VNM_F64 || kt0 == VNM_I64 || kt0 == VNM_U64)) key_out = nullptr;
    bool ident = true;   // no pass has run yet: the row ids are the identity and are not materialised (the first pass makes them up)
    for (int k = n_keys - 1; k >= 0; k--) {
        // codes of key k in the current row order; their eight digit histograms come out of the same kernel
        VNM_HIP(hipMemsetAsync(r->red + 4, 0, 8, s));
        VNM_HIP(hipMemsetAsync(r->ghist, 0, (size_t)8 * 256 * 8, s));
        {
            KernelTimer timer("sort_encode", s);
            sort_encode_kernel<<<grid_for(n, 64), 256, 0, s>>>(keys[k], orders[k] == VNM_DESC, ident ? nullptr : r->val[r->cur], n, r->code[r->cur],
                                                               nullptr, r->red + 4, r->ghist, 0);   // 64 workgroups per CU: 3.3 ms per 1e9 keys (8: 3.55)
        }
        unsigned long long any_special = 0;
        const bool cls_possible = keys[k].validity != nullptr || type_is_float(keys[k].type);
        const RadixLastPass last{k == 0 ? idx_out : nullptr, wrote_idx, k == 0 ? key_out : nullptr, kt0, orders[0] == VNM_DESC, wrote_key};
        VNM_TRY(radix_sort_codes(r, n, s, &any_special, cls_possible, true, &ident, &last));
        // class pass (values < NaN < NULL), more significant than the code, over the classes in the CURRENT order
        if (cls_possible && (any_special & 1ULL) != 0) {   // no NaN / NULL at all: nothing to do
            VNM_HIP(hipMemsetAsync(r->ghist, 0, (size_t)8 * 256 * 8, s));
            {
                KernelTimer timer("sort_encode", s);
                sort_encode_kernel<<<grid_for(n, 64), 256, 0, s>>>(keys[k], orders[k] == VNM_DESC, ident ? nullptr : r->val[r->cur], n,
                                                                   r->code[r->cur], nullptr, nullptr, r->ghist, 1);
            }
            const RadixLastPass ids{k == 0 ? idx_out : nullptr, wrote_idx, nullptr, 0, 0, nullptr};
            VNM_TRY(radix_sort_codes(r, n, s, nullptr, false, true, &ident, &ids));
        }
    }
    VNM_HIP(hipGetLastError());
    if (ident && !(wrote_idx && *wrote_idx)) sort_iota_kernel<<<grid_for(n), 256, 0, s>>>(r->val[r->cur], n);   // every key constant
    return 0;
}

// ---- the routes of vnm_sort_indices_keyed, in the order it tries them ----------------------------------------------------------------------
// Every route answers 0 = done (out_indices and *wrote_key0 written, the stream synchronised), 1 = error (set_error has the message),
// 2 = not applicable or declined: the next route.  What a route allocates goes back to the pool when it returns.

struct TopkThreshold { uint32_t cls; uint64_t code; };   // rows at or below it in (class, code) order are candidates

// Threshold for small ranks: the rnk-th best of the 4096 block winners (one scan of the sample, one workgroup sort)
static int topk_threshold_of_block_winners(const vnm_dcol& key, int desc, int64_t n, int64_t m, int64_t rnk, TopkThreshold* t, hipStream_t s) {
    PoolScope pool;
    uint64_t* bcode = (uint64_t*)pool.take(TB_BLOCKS * 8);
    uint8_t* bcls = (uint8_t*)pool.take(TB_BLOCKS);
    unsigned long long* thr = (unsigned long long*)pool.take(64);
    if (!bcode || !bcls || !thr) return 1;
    {
        KernelTimer timer("topk_sample", s);
        topk_blockbest_kernel<<<TB_BLOCKS, 256, 0, s>>>(key, desc, n, m, bcode, bcls);
        topk_small_sort_kernel<<<1, 1024, (size_t)TB_BLOCKS * 13, s>>>(bcode, bcls, nullptr, TB_BLOCKS, TB_BLOCKS, rnk, nullptr, thr);
    }
    unsigned long long th[2] = {0, 0};
    VNM_HIP(hipMemcpyAsync(th, thr, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    t->cls = (uint32_t)th[0];
    t->code = th[1];
    return 0;
}

// Threshold for larger ranks: the r01 route -- sort a 2^18-key sample by (class, code) with the grid-wide radix sort and read the
// threshold off it (its ~130 small launches cost ~1.5 ms, which only matters for small K).  2 = the rank lies beyond the sample.
static int topk_threshold_of_sorted_sample(const vnm_dcol& key, int desc, int64_t n, int64_t limit, TopkThreshold* t, hipStream_t s) {
    const int64_t m = std::min<int64_t>(n, 1 << 18);
    const int64_t rnk = (int64_t)((double)limit / (double)n * (double)m * 1.5) + 64 + (int64_t)(6.0 * sqrt((double)limit / (double)n * (double)m + 1.0));
    if (rnk >= m - 1) return 2;
    RadixBufs sr{};
    VNM_TRY(radix_alloc(&sr, m));
    PoolScope pool;
    uint8_t* scls = (uint8_t*)pool.take((size_t)m);
    if (!scls) return 1;
    topk_sample_kernel<<<grid_for(m), 256, 0, s>>>(key, desc, n, m, sr.code[0], scls);
    sort_iota_kernel<<<grid_for(m), 256, 0, s>>>(sr.val[0], m);
    VNM_TRY(radix_sort_codes(&sr, m, s));
    uint64_t* scode_sorted = (uint64_t*)pool.take((size_t)m * 8);
    if (!scode_sorted) return 1;
    VNM_HIP(hipMemcpyAsync(scode_sorted, sr.code[sr.cur], (size_t)m * 8, hipMemcpyDeviceToDevice, s));
    gather_u8_kernel<<<grid_for(m), 256, 0, s>>>(scls, sr.val[sr.cur], m, sr.code[sr.cur]);
    sort_iota_kernel<<<grid_for(m), 256, 0, s>>>(sr.val[sr.cur], m);   // stable secondary key: position in the code order
    VNM_TRY(radix_sort_codes(&sr, m, s));
    uint32_t pos_in_code_sorted = 0;
    uint64_t cls64 = 0;
    VNM_HIP(hipMemcpyAsync(&pos_in_code_sorted, sr.val[sr.cur] + rnk, 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(&cls64, sr.code[sr.cur] + rnk, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    VNM_HIP(hipMemcpyAsync(&t->code, scode_sorted + pos_in_code_sorted, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    t->cls = (uint32_t)cls64;
    return 0;
}

// The candidates: (code, class, row id) of every row at or below the threshold, unordered; they live as long as this struct.
struct TopkCandidates {
    RadixBufs cr;                 // cr.code[0]: the codes; the finishers sort in it
    PoolScope pool;
    uint8_t* cls; uint32_t* rows;
    int64_t cap, found;           // found > cap: the list is cut short and of no use
};
static int topk_select(const vnm_dcol& key, int desc, int64_t n, int64_t limit, const TopkThreshold& t, TopkCandidates* c, hipStream_t s) {
    c->cap = std::max<int64_t>(limit * 4 + 65536, 1 << 20);
    VNM_TRY(radix_alloc(&c->cr, c->cap));
    c->cls = (uint8_t*)c->pool.take((size_t)c->cap);
    c->rows = (uint32_t*)c->pool.take((size_t)c->cap * 4);
    unsigned long long* cnt = (unsigned long long*)c->pool.take(64);
    if (!c->cls || !c->rows || !cnt) return 1;
    VNM_HIP(hipMemsetAsync(cnt, 0, 8, s));
    {
        KernelTimer timer("topk_select", s);
        topk_select_kernel<<<device_info().num_cus * 8, 256, 0, s>>>(key, desc, n, t.cls, t.code, c->cap, cnt, c->cr.code[0], c->cls, c->rows);
    }
    unsigned long long found = 0;
    VNM_HIP(hipMemcpyAsync(&found, cnt, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    c->found = (int64_t)found;
    return 0;
}

// Finisher for several keys: the candidates' key columns gathered, the full multi-key sort over them, the first `limit` row ids gathered
static int topk_finish_multi_key(int n_keys, const vnm_dcol* keys, const int* orders, int64_t limit, TopkCandidates* cd, int64_t* out_indices, hipStream_t s) {
    const int64_t c = cd->found;
    RadixBufs& cr = cd->cr;
    PoolScope pool;
    // the candidates in ROW order (the multi-key sort below is stable over it)
    u32_to_code_kernel<<<grid_for(c), 256, 0, s>>>(cd->rows, c, cr.code[0]);
    sort_iota_kernel<<<grid_for(c), 256, 0, s>>>(cr.val[0], c);
    cr.cur = 0;
    VNM_TRY(radix_sort_codes(&cr, c, s));
    int64_t* rows64 = (int64_t*)pool.take((size_t)c * 8);
    int64_t* perm = (int64_t*)pool.take((size_t)c * 8);
    if (!rows64 || !perm) return 1;
    VNM_HIP(hipMemcpyAsync(rows64, cr.code[cr.cur], (size_t)c * 8, hipMemcpyDeviceToDevice, s));   // the codes ARE the row ids
    // their key columns, gathered
    std::vector<vnm_dcol> sub((size_t)n_keys);
    for (int j = 0; j < n_keys; j++) {
        const int w = type_width(keys[j].type);
        void* dv = pool.take((size_t)c * w);
        uint8_t* db = keys[j].validity ? (uint8_t*)pool.take((size_t)c) : nullptr;
        uint8_t* bm = keys[j].validity ? (uint8_t*)pool.take((size_t)(c + 7) / 8 + 8) : nullptr;
        if (!dv || (keys[j].validity && (!db || !bm))) return 1;
        take_kernel<<<grid_for(c), 256, 0, s>>>(keys[j], rows64, c, dv, db);
        if (bm) VNM_TRY(vnm_pack_validity(db, c, bm, (void*)s));
        sub[j] = keys[j];
        sub[j].values = dv; sub[j].validity = bm; sub[j].offset = 0; sub[j].length = c;
    }
    RadixBufs r2{};
    VNM_TRY(radix_alloc(&r2, c));
    bool wrote = false;
    VNM_TRY(full_sort(n_keys, sub.data(), orders, c, &r2, s, perm, &wrote));
    if (!wrote) sort_widen_kernel<<<grid_for(c), 256, 0, s>>>(r2.val[r2.cur], c, perm);
    gather_i64_kernel<<<grid_for(limit), 256, 0, s>>>(rows64, perm, limit, out_indices);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

// Finisher for few candidates (<= TS_MAX): one workgroup sorts them in LDS and writes the first K row ids
static int topk_finish_in_lds(int64_t limit, TopkCandidates* cd, int64_t* out_indices, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        VNM_TRY(allow_dynamic_lds(topk_small_sort_kernel, (size_t)TS_MAX * 13));
        attr_set = true;
    }
    const int c = (int)cd->found;
    int np2 = 64;
    while (np2 < c) np2 <<= 1;
    {
        KernelTimer timer("topk_small_sort", s);
        topk_small_sort_kernel<<<1, 1024, (size_t)np2 * 13, s>>>(cd->cr.code[0], cd->cls, cd->rows, c, np2, limit, out_indices, nullptr);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

// Finisher for many candidates, three radix pass groups -- the canonical order: by row id, then (stable) by code, then by class
static int topk_finish_radix(int64_t limit, TopkCandidates* cd, int64_t* out_indices, hipStream_t s) {
    const int64_t c = cd->found;
    RadixBufs& cr = cd->cr;
    uint64_t* code_keep = (uint64_t*)cd->pool.take((size_t)c * 8);
    if (!code_keep) return 1;
    VNM_HIP(hipMemcpyAsync(code_keep, cr.code[0], (size_t)c * 8, hipMemcpyDeviceToDevice, s));
    // pass group 1: key = row id, value = candidate slot
    u32_to_code_kernel<<<grid_for(c), 256, 0, s>>>(cd->rows, c, cr.code[0]);
    sort_iota_kernel<<<grid_for(c), 256, 0, s>>>(cr.val[0], c);
    cr.cur = 0;
    VNM_TRY(radix_sort_codes(&cr, c, s));
    // pass group 2: key = code of the slot
    gather_u64_kernel<<<grid_for(c), 256, 0, s>>>(code_keep, cr.val[cr.cur], c, cr.code[cr.cur]);
    VNM_TRY(radix_sort_codes(&cr, c, s));
    // pass group 3: key = class of the slot
    gather_u8_kernel<<<grid_for(c), 256, 0, s>>>(cd->cls, cr.val[cr.cur], c, cr.code[cr.cur]);
    VNM_TRY(radix_sort_codes(&cr, c, s));
    // slots -> row ids -> int64 output (first `limit` entries)
    gather_u32_kernel<<<grid_for(limit), 256, 0, s>>>(cd->rows, cr.val[cr.cur], limit, cr.val[cr.cur ^ 1]);
    sort_widen_kernel<<<grid_for(limit), 256, 0, s>>>(cr.val[cr.cur ^ 1], limit, out_indices);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

// Route 1, LIMIT K: one scan selects the candidates, only they are sorted.
// Several sort keys: the same selection on the FIRST key -- every row that beats the threshold on key 0, ties included, is a
// candidate (a row that loses on key 0 loses whatever its other keys are) -- and the candidates alone go through the full
// multi-key sort.  2 also when the threshold kept fewer than K rows or more than the candidates' room (ties / NaN / NULL heavy
// data, or an unlucky sample): the full sort answers.
static int try_topk(int n_keys, const vnm_dcol* keys, const int* orders, int64_t n, int64_t limit, int64_t* out_indices, int* wrote_key0, hipStream_t s) {
    if (!(limit > 0 && limit * 8 < n && n >= (1 << 16) && getenv("VNM_SORT_NO_TOPK") == nullptr && (n_keys == 1 || getenv("VNM_SORT_NO_TOPK_MULTI") == nullptr))) return 2;
    route_note("sort:topk_threshold", "LIMIT %lld of %lld rows, %d keys: sampled threshold, candidates through the full sort", (long long)limit, (long long)n, n_keys);
    const int desc = orders[0] == VNM_DESC;
    const int64_t m = std::min<int64_t>(n, 1 << 22);
    // threshold = the sample element at the expected rank of the K-th row + a safety margin, in (class, code) order
    const double frac = (double)limit / (double)n;
    const int64_t rnk = (int64_t)(frac * (double)m * 1.5) + 8 + (int64_t)(6.0 * sqrt(frac * (double)m + 1.0));
    if (rnk >= m - 1) return 2;
    TopkThreshold t{};
    if (rnk < TB_BLOCKS / 4 && m >= TB_BLOCKS * 64) VNM_TRY(topk_threshold_of_block_winners(keys[0], desc, n, m, rnk, &t, s));
    else VNM_TRY(topk_threshold_of_sorted_sample(keys[0], desc, n, limit, &t, s));
    TopkCandidates cd{};
    VNM_TRY(topk_select(keys[0], desc, n, limit, t, &cd, s));
    if (cd.found < limit || cd.found > cd.cap) return 2;
    if (n_keys > 1) VNM_TRY(topk_finish_multi_key(n_keys, keys, orders, limit, &cd, out_indices, s));
    else if (cd.found <= TS_MAX && getenv("VNM_SORT_NO_SMALL") == nullptr) VNM_TRY(topk_finish_in_lds(limit, &cd, out_indices, s));
    else VNM_TRY(topk_finish_radix(limit, &cd, out_indices, s));
    if (wrote_key0) *wrote_key0 = 0;
    return 0;
}

// Route 2 (and, over a widened copy, route 3), the two sample sorts of one 8-byte key, many rows.  Only the order is asked for: first the
// entry-word sort (8-byte words, an equalising map of the code + row id -- the sample decides; duplicated keys, lumpy distributions keep
// the splitters).  Then the splitter sort (two bucket scatters + a sort in LDS instead of eight LSD passes), which can hand back the
// sorted key as well.  *clustered: declined because the rows arrive clustered -- the splitter sort would decline what the entry-word
// sort declined for that, so it is not tried then.
static int try_sample_sorts(const vnm_dcol& key8, const char* what, int desc, int64_t n, int64_t* out_indices, uint64_t* out_sorted_key0, int* wrote_key0,
                            bool* clustered, hipStream_t s) {
    *clustered = false;
    if (!out_sorted_key0 && env_sort_i64("VNM_SORT_APX", 1)) {
        const int rx = sample_sort_apx(key8, desc, n, out_indices, clustered, s);
        if (rx == 0) {
            route_note("sort:sample_sort_words", "%lld rows, %s, order only: an equalising map from a sample, two scatters of 8-byte entry words, per-bucket LDS sort", (long long)n, what);
            if (wrote_key0) *wrote_key0 = 0;
        }
        if (rx != 2) return rx;
    }
    if (*clustered) return 2;
    route_note("sort:sample_sort", "%lld rows, %s: splitters from a sample, two bucket scatters, per-bucket LDS sort", (long long)n, what);
    bool wrote_key = false;
    const int rc = sample_sort(key8, desc, n, out_indices, out_sorted_key0, &wrote_key, clustered, s);
    if (rc == 0 && wrote_key0) *wrote_key0 = wrote_key ? 1 : 0;
    return rc;
}

static bool sample_sorts_wanted(int n_keys, int64_t n) {
    return n_keys == 1 && n >= env_sort_i64("VNM_SSORT_MIN_ROWS", (int64_t)1 << 25) && getenv("VNM_SORT_NO_SAMPLE") == nullptr;
}

// ... one 4-byte key (float32 / int32 / uint32) the same way (round 5): widened to 8 bytes -- float32 -> float64 is exact and keeps the
// order, NaNs and signed zeros -- the sample sorts order the copy; 5e8 float32 keys through the LSD passes: 27.9 ms, float64: 15.7.
// (2: the sample sorts declined -- heavy values, an overflowing bucket: the LSD passes over the original column)
static int try_widened_sample_sorts(const vnm_dcol& key, int desc, int64_t n, int64_t* out_indices, int* wrote_key0, hipStream_t s) {
    if (key.validity || !(key.type == VNM_F32 || key.type == VNM_I32 || key.type == VNM_U32) || getenv("VNM_SORT_NO_WIDEN") != nullptr) return 2;
    PoolScope pool;
    uint64_t* wide = (uint64_t*)pool.take((size_t)n * 8);
    if (!wide) return 1;
    struct IdleStreamAtExit { hipStream_t s; ~IdleStreamAtExit() { (void)hipStreamSynchronize(s); } } idle{s};   // declared after `pool`: no kernel reads `wide` any more when it goes back, whichever way out
    sort_widen_key_kernel<<<grid_for(n), 256, 0, s>>>(key.values, key.type, key.offset, n, wide);
    VNM_HIP(hipGetLastError());
    vnm_dcol key8{};
    key8.values = wide; key8.length = n;
    key8.type = key.type == VNM_F32 ? VNM_F64 : (key.type == VNM_I32 ? VNM_I64 : VNM_U64);
    bool clustered = false;   // (of no use to the caller: the already-sorted check reads 8-byte keys)
    return try_sample_sorts(key8, "one 4-byte key widened to 8 bytes", desc, n, out_indices, nullptr, wrote_key0, &clustered, s);
}

// Route 4.  A column that arrives clustered is often simply SORTED already (a time series ordered by its timestamp): see sort_inversions_kernel.
static int try_already_sorted(const vnm_dcol& key, int desc, int64_t n, int64_t* out_indices, int* wrote_key0, hipStream_t s) {
    if (key.validity || type_width(key.type) != 8 || getenv("VNM_SORT_NO_SORTED_CHECK") != nullptr) return 2;
    PoolScope pool;
    unsigned long long* inv = (unsigned long long*)pool.take(64);
    if (!inv) return 1;
    unsigned long long ninv[2] = {1, 1};
    VNM_HIP(hipMemsetAsync(inv, 0, 16, s));
    sort_inversions_kernel<<<grid_for(n, 16), 256, 0, s>>>(key, desc, n, inv);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(ninv, inv, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (ninv[0] != 0 && ninv[1] != 0) return 2;
    const int backwards = ninv[0] != 0;
    route_note("sort:already_sorted", "%lld rows, one 8-byte key: the rows arrive %s: the indices are the row numbers%s", (long long)n,
               backwards ? "strictly in the opposite order (every row below its predecessor, no ties)" : "in the order asked for (no row below its predecessor)", backwards ? " backwards" : "");
    sort_iota64_kernel<<<grid_for(n, 16), 256, 0, s>>>(out_indices, n, backwards);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    if (wrote_key0) *wrote_key0 = 0;
    return 0;
}

// Route 5, always applicable: the LSD passes
static int lsd_sort(int n_keys, const vnm_dcol* keys, const int* orders, int64_t n, int64_t* out_indices, uint64_t* out_sorted_key0, int* wrote_key0, hipStream_t s) {
    RadixBufs r{};
    VNM_TRY(radix_alloc(&r, n));
    bool wrote = false, wrote_key = false;
    route_note("sort:lsd_radix", "%lld rows, %d keys: stable LSD passes over order-preserving codes, last key first", (long long)n, n_keys);
    VNM_TRY(full_sort(n_keys, keys, orders, n, &r, s, out_indices, &wrote, out_sorted_key0, &wrote_key));
    if (wrote_key0) *wrote_key0 = wrote_key ? 1 : 0;
    if (!wrote) sort_widen_kernel<<<grid_for(n), 256, 0, s>>>(r.val[r.cur], n, out_indices);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace vnm

using namespace vnm;

extern "C" {

int vnm_sort_indices(int n_keys, const vnm_dcol* keys, const int* orders, int64_t length, int64_t limit,
                     int64_t* out_indices, void* stream) {
    return vnm_sort_indices_keyed(n_keys, keys, orders, length, limit, out_indices, nullptr, nullptr, stream);
}

int vnm_sort_indices_keyed(int n_keys, const vnm_dcol* keys, const int* orders, int64_t length, int64_t limit,
                           int64_t* out_indices, void* out_sorted_key0, int* wrote_key0, void* stream) {
    if (wrote_key0) *wrote_key0 = 0;
    VNM_TRY(ensure_init());
    if (n_keys < 1 || n_keys > 16) return set_error("vnm_sort_indices: 1..16 sort keys");
    if (length >= (1LL << 32)) return set_error("vnm_sort_indices: at most 2^32 - 1 rows per sort");
    for (int k = 0; k < n_keys; k++)
        if (keys[k].length != length) return set_error("vnm_sort_indices: key %d length mismatch", k);
    if (length == 0) return 0;
    hipStream_t s = as_stream(stream);
    const int64_t n = length;
    const vnm_dcol& key = keys[0];
    const int desc = orders[0] == VNM_DESC;
    uint64_t* key_out = (uint64_t*)out_sorted_key0;
    // the routes in order; the first that does not answer 2 (not applicable / declined) is the answer
    bool clustered = false;   // the sample sorts saw rows that arrive clustered: worth the already-sorted check
    int rc = try_topk(n_keys, keys, orders, n, limit, out_indices, wrote_key0, s);
    if (rc == 2 && sample_sorts_wanted(n_keys, n)) {
        if (key.type == VNM_F64 || key.type == VNM_I64 || key.type == VNM_U64) {
            if (!key.validity || getenv("VNM_SSORT_NO_NULLS") == nullptr) rc = try_sample_sorts(key, "one 8-byte key", desc, n, out_indices, key_out, wrote_key0, &clustered, s);
        } else rc = try_widened_sample_sorts(key, desc, n, out_indices, wrote_key0, s);
    }
    if (rc == 2 && clustered && !key_out) rc = try_already_sorted(key, desc, n, out_indices, wrote_key0, s);
    if (rc == 2) rc = lsd_sort(n_keys, keys, orders, n, out_indices, key_out, wrote_key0, s);
    return rc;
}

int vnm_take(const vnm_dcol* col, const int64_t* indices, int64_t n, void* out_values, uint8_t* out_valid, void* stream) {
    VNM_TRY(ensure_init());
    if (!col || (n > 0 && (!indices || !out_values))) return set_error("vnm_take: null argument");
    if (col->validity && !out_valid) return set_error("vnm_take: column has nulls but no out_valid buffer");
    if (n <= 0) return 0;
    take_kernel<<<grid_for(n), 256, 0, as_stream(stream)>>>(*col, indices, n, out_values, out_valid);
    VNM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
