// String dictionary on the device: value -> int32 code for the non-numeric GROUP BY keys of GenericHashAggregate.
//
// The reference keys its generic map on vectors of arrow::Scalar -- one hash + Equals per row on the host
// (vinum_cpp/src/operators/aggregate/generic_hash_aggregate.h:10-45).  Round 2 dictionary-encoded such columns with Arrow's
// dictionary_encode + NumPy on the host: 7-17 M rows/s, 1.5 M rows/s at 5e6 distinct values -- three orders of magnitude
// behind the numeric operators the codes then go through.  Here the column's offsets and bytes cross PCIe once and ONE kernel
// maps every row to its code:
//   * hash of the bytes (8-byte steps), find-or-insert in a table of 32-byte slots [tag, id + 1, where, length];
//     a candidate with the same tag and length is compared byte for byte -- nothing rests on the 63-bit tag;
//   * a value first seen in this batch is represented by the ROW that claimed the slot (`where` = NEW | row); after the
//     kernel the new values are copied, in table order, to the end of the dictionary's byte heap (`where` = heap offset):
//     no allocation inside the claim, the heap is dense and sized exactly;
//   * ids come from per-workgroup chunks of a global counter (an LDS atomic inside the claim; holes < 2x);
//   * the table grows by rehash between launches (workgroups resume from progress[]); ids and heap offsets survive.
// The host side keeps the dictionary's values (it receives only the NEW values of each batch: ids, lengths, bytes) and maps
// the result's codes back (vinum_amd/keydict.py::KeyDictionary).
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vnm_common.hpp"
#include "vnm_strcase.hpp"

namespace vnm {

constexpr uint64_t SD_EMPTY = ~0ULL, SD_LOCKED = ~0ULL - 1, SD_NEW = 1ULL << 63;
constexpr int SD_TILE = 2048;      // rows per workgroup and room check
constexpr int SD_PER = 8;          // slots per thread in the compaction passes

struct SDict {
    uint64_t* slot;                // [cap][4]: tag, id + 1, heap offset or SD_NEW | row, length
    uint64_t cap;
    unsigned long long* ctl;       // [1] a workgroup ran out of room  [2] fill  [3] values new in this batch
};

struct SdArgs {
    const void* offs;              // Arrow offsets (int32 / int64), element `first` belongs to row 0
    const int32_t* lens;           // SPANS (null for Arrow offsets): row r is the lens[r] bytes at offs[r] (int64) -- fields of a CSV block in place
    int wide;
    int64_t first;
    const uint8_t* valid;          // bitmap, bit `vfirst` belongs to row 0 (or null)
    int64_t vfirst;
    const uint8_t* data;           // byte `data_base` of the Arrow data buffer
    int64_t data_base;
    int64_t nrows, ntiles, margin, fill_limit;
    SDict d;
    const uint8_t* heap;
    unsigned int* progress;
    int32_t* out;
    unsigned long long* gnext;
};

__device__ __forceinline__ uint64_t sd_ld(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sd_st(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int64_t sd_off(const SdArgs& a, int64_t row) {
    return a.wide ? ((const int64_t*)a.offs)[a.first + row] : (int64_t)((const int32_t*)a.offs)[a.first + row];
}

__device__ __forceinline__ uint64_t sd_mix(uint64_t h) {
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 32;
    return h;
}
__device__ __forceinline__ uint64_t sd_hash(const uint8_t* p, int64_t len) {
    uint64_t h = 0x9E3779B97F4A7C15ULL ^ ((uint64_t)len * 0xc4ceb9fe1a85ec53ULL);
    int64_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t x;
        __builtin_memcpy(&x, p + i, 8);
        h = sd_mix(h ^ x);
    }
    uint64_t x = 0;
    for (int k = 0; i + k < len; k++) x |= (uint64_t)p[i + k] << (8 * k);
    h = sd_mix(h ^ x ^ 0x5bd1e9955bd1e995ULL);
    return sd_mix(h) & 0x7FFFFFFFFFFFFFFFULL;
}
__device__ __forceinline__ bool sd_equal(const uint8_t* a, const uint8_t* b, int64_t len) {
    int64_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < len; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void sd_encode_kernel(SdArgs a) {
    __shared__ int s_go;
    __shared__ unsigned s_new;
    __shared__ unsigned long long s_gnext, s_gend;
    const int tid = threadIdx.x;
    if (tid == 0) { s_new = 0; s_gnext = 0; s_gend = 0; }
    __syncthreads();
    const uint64_t mask = a.d.cap - 1;
    unsigned it = a.progress[blockIdx.x];
    for (;; it++) {
        const int64_t tile = (int64_t)blockIdx.x + (int64_t)it * gridDim.x;
        if (tile >= a.ntiles) break;
        __syncthreads();
        if (tid == 0) {
            const unsigned v = atomicExch(&s_new, 0u);
            if (v) { atomicAdd(&a.d.ctl[2], (unsigned long long)v); atomicAdd(&a.d.ctl[3], (unsigned long long)v); }
            const unsigned long long fill = __hip_atomic_load(&a.d.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool room = (int64_t)fill + a.margin <= a.fill_limit;
            if (!room) __hip_atomic_store(&a.d.ctl[1], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (room && s_gend - s_gnext < (unsigned long long)SD_TILE) {   // every row of a tile may bring a new value
                const unsigned long long base = atomicAdd(a.gnext, 2ULL * SD_TILE);
                s_gnext = base; s_gend = base + 2ULL * SD_TILE;
            }
            s_go = room ? 1 : 0;
        }
        __syncthreads();
        if (!s_go) break;
        for (int r = 0; r < SD_TILE / 256; r++) {
            const int64_t row = tile * SD_TILE + (int64_t)r * 256 + tid;
            if (row >= a.nrows) continue;
            if (a.valid && !((a.valid[(a.vfirst + row) >> 3] >> ((a.vfirst + row) & 7)) & 1)) { a.out[row] = -1; continue; }
            const int64_t o0 = sd_off(a, row), len = a.lens ? (int64_t)a.lens[row] : sd_off(a, row + 1) - o0;
            const uint8_t* p = a.data + (o0 - a.data_base);
            const uint64_t tagv = sd_hash(p, len);
            uint64_t h = (tagv ^ (tagv >> 29)) & mask;
            int64_t id;
            for (;;) {
                uint64_t* s = a.d.slot + h * 4;
                const uint64_t t = sd_ld(s);
                if (t == tagv) {   // (the words behind a published tag are in place: the claimer drained them first)
                    const uint64_t id1 = sd_ld(s + 1), where = sd_ld(s + 2), l = sd_ld(s + 3);
                    if ((int64_t)l == len) {
                        const uint8_t* q = (where & SD_NEW) ? a.data + (sd_off(a, (int64_t)(where & ~SD_NEW)) - a.data_base) : a.heap + where;
                        if (sd_equal(p, q, len)) { id = (int64_t)id1 - 1; break; }
                    }
                    h = (h + 1) & mask;
                    continue;
                }
                if (t == SD_EMPTY) {
                    uint64_t expected = SD_EMPTY;
                    if (__hip_atomic_compare_exchange_strong(s, &expected, SD_LOCKED, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        id = (int64_t)atomicAdd(&s_gnext, 1ULL);
                        sd_st(s + 1, (uint64_t)id + 1);
                        sd_st(s + 2, SD_NEW | (uint64_t)row);
                        sd_st(s + 3, (uint64_t)len);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        sd_st(s, tagv);
                        atomicAdd(&s_new, 1u);
                        break;
                    }
                    continue;   // someone else is claiming this slot: look at it again
                }
                if (t == SD_LOCKED) continue;
                h = (h + 1) & mask;
            }
            a.out[row] = (int32_t)id;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned v = atomicExch(&s_new, 0u);
        if (v) { atomicAdd(&a.d.ctl[2], (unsigned long long)v); atomicAdd(&a.d.ctl[3], (unsigned long long)v); }
        a.progress[blockIdx.x] = it;
    }
}

// a bigger table: every slot moves as it is (the values are distinct: the first free slot of its probe sequence)
__global__ void sd_rehash_kernel(SDict from, SDict to) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t mask = to.cap - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)from.cap; i += stride) {
        const uint64_t* src = from.slot + (uint64_t)i * 4;
        const uint64_t t = src[0];
        if (t == SD_EMPTY || t == SD_LOCKED) continue;
        uint64_t h = (t ^ (t >> 29)) & mask;
        for (;;) {
            uint64_t* dst = to.slot + h * 4;
            uint64_t expected = SD_EMPTY;
            if (__hip_atomic_compare_exchange_strong(dst, &expected, t, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
                break;
            }
            h = (h + 1) & mask;
        }
    }
}

// ---- the batch's new values -> the heap, in table order ------------------------------------------------------------------
// pass A: per thread (SD_PER consecutive slots) the new values and their bytes; exclusive prefixes inside the workgroup
struct SdCompact {
    SDict d;
    uint32_t* pre_cnt;             // [cap / SD_PER] exclusive prefix inside the workgroup
    unsigned long long* pre_bytes;
    unsigned long long* blk;       // [2 * nblocks]: per workgroup (count, bytes) -> exclusive prefixes after pass B; [2 * nblocks ..]: totals
    int nblocks;
    // pass C
    SdArgs in;
    uint8_t* heap;
    unsigned long long heap_used;
    int32_t* new_ids;
    int32_t* new_lens;
    int64_t* id_off;               // id -> heap offset / length of its value (the LIKE matcher's view of the dictionary)
    int32_t* id_len;
};

__global__ __launch_bounds__(256) void sd_compact_count_kernel(SdCompact c) {
    __shared__ unsigned long long sc[256], sb[256];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    unsigned long long cnt = 0, bytes = 0;
    for (int k = 0; k < SD_PER; k++) {
        const int64_t h = t * SD_PER + k;
        if (h >= (int64_t)c.d.cap) break;
        const uint64_t* s = c.d.slot + (uint64_t)h * 4;
        const uint64_t tag = s[0];
        if (tag == SD_EMPTY || tag == SD_LOCKED || !(s[2] & SD_NEW)) continue;
        cnt++; bytes += s[3];
    }
    sc[tid] = cnt; sb[tid] = bytes;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan
        const unsigned long long x = tid >= d ? sc[tid - d] : 0, y = tid >= d ? sb[tid - d] : 0;
        __syncthreads();
        sc[tid] += x; sb[tid] += y;
        __syncthreads();
    }
    if (t * SD_PER < (int64_t)c.d.cap) { c.pre_cnt[t] = (uint32_t)(sc[tid] - cnt); c.pre_bytes[t] = sb[tid] - bytes; }
    if (tid == 255) { c.blk[2 * blockIdx.x] = sc[255]; c.blk[2 * blockIdx.x + 1] = sb[255]; }
}

// pass B: exclusive prefix of the workgroup totals (one workgroup)
__global__ __launch_bounds__(1024) void sd_compact_scan_kernel(unsigned long long* blk, int nblocks) {
    __shared__ unsigned long long sc[1024], sb[1024];
    const int tid = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int lo = tid * per, hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long c = 0, b = 0;
    for (int i = lo; i < hi; i++) { c += blk[2 * i]; b += blk[2 * i + 1]; }
    sc[tid] = c; sb[tid] = b;
    __syncthreads();
    if (tid == 0) {
        unsigned long long rc = 0, rb = 0;
        for (int i = 0; i < 1024; i++) { const unsigned long long x = sc[i], y = sb[i]; sc[i] = rc; sb[i] = rb; rc += x; rb += y; }
        blk[2 * nblocks] = rc; blk[2 * nblocks + 1] = rb;
    }
    __syncthreads();
    unsigned long long rc = sc[tid], rb = sb[tid];
    for (int i = lo; i < hi; i++) {
        const unsigned long long x = blk[2 * i], y = blk[2 * i + 1];
        blk[2 * i] = rc; blk[2 * i + 1] = rb;
        rc += x; rb += y;
    }
}

// pass C: bytes to the heap, the slot learns its heap offset, (id, length) of the new values in heap order
__global__ __launch_bounds__(256) void sd_compact_move_kernel(SdCompact c) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t * SD_PER >= (int64_t)c.d.cap) return;
    unsigned long long k = c.blk[2 * blockIdx.x] + c.pre_cnt[t];
    unsigned long long at = c.blk[2 * blockIdx.x + 1] + c.pre_bytes[t];
    for (int j = 0; j < SD_PER; j++) {
        const int64_t h = t * SD_PER + j;
        if (h >= (int64_t)c.d.cap) break;
        uint64_t* s = c.d.slot + (uint64_t)h * 4;
        const uint64_t tag = s[0];
        if (tag == SD_EMPTY || tag == SD_LOCKED || !(s[2] & SD_NEW)) continue;
        const int64_t row = (int64_t)(s[2] & ~SD_NEW), len = (int64_t)s[3];
        const uint8_t* p = c.in.data + (sd_off(c.in, row) - c.in.data_base);
        uint8_t* q = c.heap + c.heap_used + at;
        for (int64_t i = 0; i < len; i++) q[i] = p[i];
        s[2] = c.heap_used + at;
        const int32_t id = (int32_t)(s[1] - 1);
        c.new_ids[k] = id;
        c.new_lens[k] = (int32_t)len;
        c.id_off[id] = (int64_t)(c.heap_used + at);
        c.id_len[id] = (int32_t)len;
        k++; at += (unsigned long long)len;
    }
}

int sdict_alloc(SDict* d, uint64_t cap, hipStream_t s) {
    memset(d, 0, sizeof(*d));
    d->cap = cap;
    d->slot = (uint64_t*)pool_alloc((size_t)cap * 32);
    d->ctl = (unsigned long long*)pool_alloc(64);
    if (!d->slot || !d->ctl || hipMemsetAsync(d->slot, 0xFF, (size_t)cap * 32, s) != hipSuccess || hipMemsetAsync(d->ctl, 0, 64, s) != hipSuccess) {
        pool_free(d->slot); pool_free(d->ctl);   // (nothing half-allocated is left behind)
        memset(d, 0, sizeof(*d));
        return set_error("vnm_strdict: table allocation failed");
    }
    return 0;
}
void sdict_free(SDict* d) {
    pool_free(d->slot);
    pool_free(d->ctl);
    memset(d, 0, sizeof(*d));
}
int sdict_grow(SDict* d, uint64_t new_cap, hipStream_t s) {
    SDict nd;
    VNM_TRY(sdict_alloc(&nd, new_cap, s));
    VNM_HIP(hipMemcpyAsync(nd.ctl + 2, d->ctl + 2, 16, hipMemcpyDeviceToDevice, s));   // fill and the batch's new count carry over
    sd_rehash_kernel<<<(int)std::min<int64_t>(((int64_t)d->cap + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(*d, nd);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    sdict_free(d);
    *d = nd;
    return 0;
}

// ---- order-preserving ranks of the dictionary's values (round 5: string / binary ORDER BY keys on the device) -----------------
// Arrow's SortIndices compares utf8 / binary values byte-wise (sort.cpp:22-37).  The dictionary's values are DISTINCT, so their sort
// order is a rank per id; a row's sort key then is rank[code] -- an ordinary int32 column of the numeric sort (equal strings share
// a rank, so the stable sort keeps their row order).  The values are sorted by the existing multi-key radix sort over 8-byte
// BIG-ENDIAN chunks of their bytes (zero padded) with the length as the least significant key (a value that is a prefix of another
// sorts first, "a" before "a\0"): up to 15 chunks + the length per sort call, longer values in several stable rounds from the last
// chunks to the first (an LSD sort over the chunk columns; a round's keys are read through the permutation of the rounds before).
struct SdRankArgs {
    SDict d;
    const uint8_t* heap;
    uint64_t* voff;     // [D] heap offset (+ base: the joint ranking of two dictionaries lists addresses, its heap is null)
    uint64_t base;
    uint32_t* vlen;     // [D]
    int32_t* vid;       // [D]
    unsigned long long* ctl;   // [0] next list position  [1] longest value
};

__global__ __launch_bounds__(256) void sd_list_kernel(SdRankArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long maxlen = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)a.d.cap; i += stride) {
        const uint64_t* s = a.d.slot + (uint64_t)i * 4;
        const uint64_t tag = s[0];
        if (tag == SD_EMPTY || tag == SD_LOCKED) continue;
        const unsigned long long k = atomicAdd(&a.ctl[0], 1ULL);
        a.voff[k] = a.base + s[2]; a.vlen[k] = (uint32_t)s[3]; a.vid[k] = (int32_t)(s[1] - 1);
        if (s[3] > maxlen) maxlen = s[3];
    }
    if (maxlen) atomicMax(&a.ctl[1], maxlen);
}

// key columns of one round: out[c][i] = chunk (j0 + c) of value perm[i] (perm = null: value i); out[nchunks][i] = its length (with_len)
__global__ __launch_bounds__(256) void sd_chunk_kernel(const uint8_t* heap, const uint64_t* voff, const uint32_t* vlen, const int64_t* perm, int64_t n,
                                                       int j0, int nchunks, int with_len, uint64_t* out /* [nchunks + with_len][n] */) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t v = perm ? perm[i] : i;
        const uint8_t* p = (const uint8_t*)((uint64_t)heap + voff[v]);
        const int64_t len = vlen[v];
        for (int c = 0; c < nchunks; c++) {
            const int64_t at = (int64_t)(j0 + c) * 8;
            uint64_t x = 0;
            for (int b = 0; b < 8; b++) x = (x << 8) | (at + b < len ? (uint64_t)p[at + b] : 0ULL);
            out[(int64_t)c * n + i] = x;
        }
        if (with_len) out[(int64_t)nchunks * n + i] = (uint64_t)len;
    }
}

__global__ __launch_bounds__(256) void sd_rank_scatter_kernel(const int64_t* perm, const int32_t* vid, int64_t n, int32_t* rank_of_id) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) rank_of_id[vid[perm[i]]] = (int32_t)i;
}

// rows' codes -> rows' ranks (a NULL row -- code -1 -- gets 0; its validity bit says NULL)
__global__ __launch_bounds__(256) void sd_code_rank_kernel(const int32_t* codes, const int32_t* rank_of_id, int64_t n, int32_t* out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) { const int32_t c = codes[i]; out[i] = c < 0 ? 0 : rank_of_id[c]; }
}

// ---- two dictionaries against each other (a string column compared with a string column) ------------------------------------------
// vnm_strdict_translate: one lane per id of `src`, the encode kernel's probe of `dst`'s table without the insert (dst is only
// read: between two encodes no slot is locked and every `where` is a heap offset).  -2: dst does not hold the value, or the id was
// never handed out (-1 stays the NULL code).
struct SdTransArgs {
    const uint8_t* sheap;
    const int64_t* s_off;
    const int32_t* s_len;      // -1: an id never handed out
    SDict d;                   // dst (slot = null: no value yet)
    const uint8_t* dheap;
    int64_t id_begin, id_end;
    int32_t* out;
};

__global__ __launch_bounds__(256) void sd_translate_kernel(SdTransArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const uint64_t mask = a.d.cap - 1;
    for (int64_t id = a.id_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; id < a.id_end; id += stride) {
        const int64_t len = a.s_len[id];
        int32_t code = -2;
        if (len >= 0 && a.d.slot) {
            const uint8_t* p = a.sheap + a.s_off[id];
            const uint64_t tagv = sd_hash(p, len);
            uint64_t h = (tagv ^ (tagv >> 29)) & mask;
            for (uint64_t probes = 0; probes < a.d.cap; probes++) {   // (the table is at most 70 % full: an empty slot ends the walk)
                const uint64_t* s = a.d.slot + h * 4;
                const uint64_t t = s[0];
                if (t == SD_EMPTY) break;
                if (t == tagv && (int64_t)s[3] == len && sd_equal(p, a.dheap + s[2], len)) { code = (int32_t)(s[1] - 1); break; }
                h = (h + 1) & mask;
            }
        }
        a.out[id] = code;
    }
}

// vnm_strdict_ranks_joint: the values of both dictionaries in one list, sorted as vnm_strdict_ranks_device sorts one dictionary's;
// equal bytes end up next to each other (at most two: each dictionary's values are distinct), so a "differs from its predecessor"
// flag per sorted position and its inclusive prefix sum are the dense ranks.  Pass A: SD_PER positions per thread, the flags and
// their exclusive prefix inside the workgroup; pass B: sd_compact_scan_kernel over the workgroup totals; pass C: ranks -> ids.
struct SdJointArgs {
    const int64_t* perm;       // sorted position -> index in the value list
    const uint64_t* vaddr;     // [D] address of the value's bytes
    const uint32_t* vlen;
    const int32_t* vid;
    int64_t n, n_a;            // values; the first n_a belong to dictionary a
    uint8_t* flag;             // [n]
    uint32_t* pre;             // [threads]
    unsigned long long* blk;   // [2 * nblocks + 2] (count, unused) pairs, the layout sd_compact_scan_kernel scans
    int32_t* rank_a;
    int32_t* rank_b;
    int both;                  // one handle given twice: every rank goes to both outputs
};

__global__ __launch_bounds__(256) void sd_joint_flag_kernel(SdJointArgs a) {
    __shared__ unsigned sc[256];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    unsigned cnt = 0;
    for (int k = 0; k < SD_PER; k++) {
        const int64_t i = t * SD_PER + k;
        if (i >= a.n) break;
        uint8_t f = 0;
        if (i > 0) {
            const int64_t v = a.perm[i], u = a.perm[i - 1];
            f = (a.vlen[v] != a.vlen[u] || !sd_equal((const uint8_t*)a.vaddr[v], (const uint8_t*)a.vaddr[u], (int64_t)a.vlen[v])) ? 1 : 0;
        }
        a.flag[i] = f;
        cnt += f;
    }
    sc[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan
        const unsigned x = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += x;
        __syncthreads();
    }
    if (t * SD_PER < a.n) a.pre[t] = sc[tid] - cnt;
    if (tid == 255) { a.blk[2 * blockIdx.x] = sc[255]; a.blk[2 * blockIdx.x + 1] = 0; }
}

__global__ __launch_bounds__(256) void sd_joint_rank_kernel(SdJointArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t * SD_PER >= a.n) return;
    unsigned long long r = a.blk[2 * blockIdx.x] + a.pre[t];
    for (int k = 0; k < SD_PER; k++) {
        const int64_t i = t * SD_PER + k;
        if (i >= a.n) break;
        r += a.flag[i];
        const int64_t v = a.perm[i];
        (v < a.n_a ? a.rank_a : a.rank_b)[a.vid[v]] = (int32_t)r;
        if (a.both) a.rank_b[a.vid[v]] = (int32_t)r;
    }
}

// ---- LIKE against the dictionary's values (LikeFunction, vinum/core/functions.py:301-344) -----------------------------------------
// One lane per dictionary id, the classic wildcard walk: literal runs and single code points advance pattern and value together, a
// mismatch goes back to the last `%` and lets it take one more code point.  O(value x pattern) at worst, never exponential.  Neither
// `%` nor `_` matches '\n', so a '\n' of the value is consumed by a literal '\n' of the pattern or the match fails: a `%` that would
// have to take one ends the walk, and a literal run holding a '\n' fixes the position of everything before it (no `%` before it can
// move), so it clears the restart point.
struct LikeArgs {
    const uint8_t* heap;
    const int64_t* id_off;
    const int32_t* id_len;     // -1: an id never handed out
    const int32_t* tok;        // [ntok][3]: kind (LK_LIT_NL = a literal run with a '\n'), byte start, byte length
    const uint8_t* pat;
    int ntok;
    int flags;
    int64_t id_begin, id_end;
    uint8_t* out;
};
constexpr int LK_LIT_NL = 3;

__device__ __forceinline__ int64_t lk_cp_len(uint8_t b) { return b < 0xC0 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4; }

__device__ bool lk_match(const LikeArgs& a, const uint8_t* v, int64_t n) {
    int p = 0, star = -1;
    int64_t t = 0, mark = 0;
    while (t < n) {
        if (p < a.ntok) {
            const int kind = a.tok[3 * p];
            if (kind == VNM_LIKE_TOK_ANY) {
                if (v[t] != '\n') { t = min(t + lk_cp_len(v[t]), n); p++; continue; }
            } else if (kind == VNM_LIKE_TOK_STAR) {
                star = p++; mark = t;
                continue;
            } else {
                const int len = a.tok[3 * p + 2];
                const uint8_t* q = a.pat + a.tok[3 * p + 1];
                if (t + len <= n && v[t] == q[0]) {
                    int k = 1;
                    while (k < len && v[t + k] == q[k]) k++;
                    if (k == len) {
                        t += len; p++;
                        if (kind == LK_LIT_NL) star = -1;
                        continue;
                    }
                }
            }
        }
        if (star < 0 || v[mark] == '\n') return false;   // (`%` takes no newline)
        mark = min(mark + lk_cp_len(v[mark]), n);
        t = mark;
        p = star + 1;
    }
    while (p < a.ntok && a.tok[3 * p] == VNM_LIKE_TOK_STAR) p++;
    return p == a.ntok;
}

__global__ __launch_bounds__(256) void sd_like_kernel(LikeArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t id = a.id_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; id < a.id_end; id += stride) {
        const int32_t len = a.id_len[id];
        bool m = false;
        if (len >= 0) {
            const uint8_t* v = a.heap + a.id_off[id];
            int64_t n = len;
            if (a.flags & VNM_LIKE_STRIP_NUL)
                while (n > 0 && v[n - 1] == 0) n--;
            m = lk_match(a, v, n) || (n > 0 && v[n - 1] == '\n' && lk_match(a, v, n - 1));   // '$' before a final newline
        }
        a.out[id] = m ? 1 : 0;
    }
}

// ---- a dictionary-typed Arrow column: the batch dictionary's indices -> the running dictionary's codes ---------------------------
// The batch's distinct VALUES went through the encode kernel above (n_values rows, not n): `table[j]` is the running code of value
// j (-1: a NULL value).  A row is table[index[row]], or -1 when the row is NULL, its value is NULL or its index lies outside
// [0, n_values) -- the bounds test comes before the load, so such an index is never an address.  One lane takes RM_ROWS = 8
// consecutive rows: their indices in 16-byte loads (one 8-byte load for 1-byte indices) when the first one is aligned, element by
// element otherwise and in the last, partial group; 8 codes = two 16-byte stores; 8 validity bits = ONE byte of the output bitmap,
// which no other lane touches (no atomics, no byte shared between lanes, let alone waves).  HBM-bound: 1-8 index bytes in, 4 code
// bytes out per row; the table is read through L2, or from a copy in LDS when it is small against the rows (see the launch).
constexpr int RM_ROWS = 8;
constexpr int RM_TILE = 256 * RM_ROWS;     // rows per workgroup and step
constexpr int RM_LDS_VALUES = 8192;        // the LDS form: a table of up to this many codes is copied into LDS (32 KB) per workgroup

struct RemapArgs {
    const void* idx;           // element `first` belongs to row 0
    const uint8_t* valid;      // bitmap, bit `first` belongs to row 0 (or null)
    int64_t first, n, n_values, ntiles;
    const int32_t* table;
    int32_t* out;
    uint8_t* out_valid;        // bitmap at bit offset 0 (or null)
    unsigned long long* bad;   // valid rows with an index outside the table (null: not counted)
    int vec_in, vec_out;       // the first index / out[0] is aligned for the wide loads / stores
};

template <typename T, bool LDS>
__global__ __launch_bounds__(256) void sd_remap_kernel(RemapArgs a) {
    __shared__ unsigned s_bad;
    __shared__ int32_t s_table[LDS ? RM_LDS_VALUES : 1];
    if (threadIdx.x == 0) s_bad = 0;
    if constexpr (LDS)
        for (int64_t i = threadIdx.x; i < a.n_values; i += 256) s_table[i] = a.table[i];
    __syncthreads();
    unsigned nbad = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * RM_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < RM_ROWS ? (int)(a.n - row0) : RM_ROWS;
        const T* p = (const T*)a.idx + a.first + row0;
        T v[RM_ROWS];
        if (a.vec_in && cnt == RM_ROWS) {
            asm volatile("" ::: "memory");   // (compiler fences around the wide accesses: p[0] / o[0] of the element path merged into them splits a 16-byte access)
            if constexpr (sizeof(T) == 1) {
                const uint2 q = *(const uint2*)p;
                __builtin_memcpy(v, &q, sizeof(v));
            } else {
                uint4 q[sizeof(T) / 2];
#pragma unroll
                for (int j = 0; j < (int)(sizeof(T) / 2); j++) q[j] = ((const uint4*)p)[j];
                __builtin_memcpy(v, q, sizeof(v));
            }
            asm volatile("" ::: "memory");
        } else {
#pragma unroll
            for (int k = 0; k < RM_ROWS; k++) v[k] = k < cnt ? p[k] : (T)0;
        }
        unsigned vbits = 0xFFu;
        if (a.valid) {   // bits first + row0 ... + 7: at most two bytes of the bitmap, the second only if it exists
            const int64_t bit = a.first + row0, last_byte = (a.first + a.n - 1) >> 3;
            const int sh = (int)(bit & 7);
            vbits = (unsigned)a.valid[bit >> 3] >> sh;
            if (sh && (bit >> 3) + 1 <= last_byte) vbits |= (unsigned)a.valid[(bit >> 3) + 1] << (8 - sh);
        }
        vbits &= (1u << cnt) - 1;
        int32_t c[RM_ROWS];
        unsigned obits = 0;
#pragma unroll
        for (int k = 0; k < RM_ROWS; k++) {
            int32_t code = -1;
            if ((vbits >> k) & 1) {
                const uint64_t u = (uint64_t)v[k];            // (a negative index: sign-extended, far outside)
                if (u < (uint64_t)a.n_values) code = LDS ? s_table[u] : a.table[u];
                else nbad++;
            }
            c[k] = code;
            obits |= (code >= 0 ? 1u : 0u) << k;
        }
        int32_t* o = a.out + row0;
        if (a.vec_out && cnt == RM_ROWS) {
            asm volatile("" ::: "memory");
            ((int4*)o)[0] = make_int4(c[0], c[1], c[2], c[3]);
            ((int4*)o)[1] = make_int4(c[4], c[5], c[6], c[7]);
            asm volatile("" ::: "memory");
        } else {
#pragma unroll
            for (int k = 0; k < RM_ROWS; k++)
                if (k < cnt) o[k] = c[k];
        }
        if (a.out_valid) a.out_valid[row0 >> 3] = (uint8_t)obits;   // (bits past n stay 0: vbits was cut to cnt)
    }
    if (a.bad) {
        if (nbad) atomicAdd(&s_bad, nbad);
        __syncthreads();
        if (threadIdx.x == 0 && s_bad) atomicAdd(a.bad, (unsigned long long)s_bad);
    }
}

// ---- upper() / lower() over the dictionary's values (UpperStringFunction / LowerStringFunction, vinum/core/functions.py:279-298) -----
// pc.utf8_upper / utf8_lower map code point -> code point without context, so a function of the VALUE alone: one lane per id of
// `src` decodes its value, substitutes every code point found in a sorted table (map_from -> map_to, ~1500 pairs, a copy in LDS per
// workgroup), encodes the image into a scratch buffer and the (start, length) spans go through the encode kernel above into `dst`.
// No scan: a code point's image is at most twice as long as the code point (the host refuses a map where it is not), so value `id`
// owns the 2 * length bytes at twice its heap offset relative to the first heap byte of this call's ids.
//   * 8 source bytes per step while they are all < 0x80 and the map keeps ASCII inside ASCII: eight lookups in a 128-byte LDS
//     table, one 8-byte store -- the code point table is not touched;
//   * any other code point: lead byte -> length, the length is held against the END OF THE VALUE before a continuation byte is
//     read (a lead byte at the end of a value never pulls in its neighbour's bytes), continuation bytes must be 10xxxxxx; a stray
//     continuation byte and 0xF8..0xFF are no lead bytes.  Such a value is counted, gets no span (validity bit 0) and is not inserted;
//   * the search is a branch-free lower bound over the LDS copy (one compare + select per power of two);
//   * every store is held against the value's room first, whatever the table says.
// A wave takes 64 consecutive ids, so its ballot IS the 8 bytes of the validity bitmap the encode kernel reads for them.
constexpr int MC_MAX_MAP = 2048;   // pairs a workgroup holds in LDS (16 KB); the two Unicode case maps have ~1500

struct SdMapArgs {
    const uint8_t* sheap;
    const int64_t* s_off;
    const int32_t* s_len;          // -1: an id never handed out
    const int32_t* map;            // [n_map] from (ascending), [n_map] to, then 128 bytes: the image of every ASCII byte
    int n_map, top_step;           // top_step: the largest power of two <= n_map (0: an empty map)
    int ascii_closed;              // every ASCII code point maps inside ASCII: the 8-byte step may be taken
    int64_t id_begin, id_end;
    int64_t heap_base;             // no id >= id_begin lies below this heap offset
    uint8_t* scratch;
    int64_t scratch_bytes;
    int64_t* starts;               // [id_end - id_begin] spans of the images in `scratch`
    int32_t* lens;
    unsigned long long* valid;     // bitmap, bit id - id_begin: the value exists and is well-formed
    unsigned long long* counts;    // [0] malformed values  [1] values whose room lay outside the scratch buffer (internal error)
};

__global__ __launch_bounds__(256) void sd_map_kernel(SdMapArgs a) {
    __shared__ int32_t s_from[MC_MAX_MAP], s_to[MC_MAX_MAP];
    __shared__ uint8_t s_ascii[128];
    const int tid = threadIdx.x;
    for (int i = tid; i < a.n_map; i += 256) { s_from[i] = a.map[i]; s_to[i] = a.map[a.n_map + i]; }
    if (tid < 128) s_ascii[tid] = ((const uint8_t*)(a.map + 2 * (int64_t)a.n_map))[tid];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t id0 = a.id_begin + (int64_t)blockIdx.x * 256; id0 < a.id_end; id0 += stride) {   // (uniform trips: every lane reaches the ballots)
        const int64_t id = id0 + tid;
        const int64_t len = id < a.id_end ? (int64_t)a.s_len[id] : -1;
        const bool live = len >= 0;
        bool ok = live, outside = false;
        int64_t start = 0, o = 0;
        if (live) {
            const int64_t off = a.s_off[id];
            const int64_t room = 2 * len;
            start = 2 * (off - a.heap_base);
            if (off < a.heap_base || start + room > a.scratch_bytes) { ok = false; outside = true; }
            if (ok) {
                o = mc_map_value(a.sheap + off, len, a.scratch + start, room, s_from, s_to, a.n_map, a.top_step, s_ascii, a.ascii_closed != 0);
                ok = o >= 0;
            }
        }
        if (id < a.id_end) { a.starts[id - a.id_begin] = ok ? start : 0; a.lens[id - a.id_begin] = ok ? (int32_t)o : 0; }
        const unsigned long long good = __ballot(ok), bad = __ballot(live && !ok && !outside), out = __ballot(outside);
        if ((tid & 63) == 0) {
            const int64_t first = id0 + (tid & ~63);                        // the wave's first id
            if (first < a.id_end) a.valid[(first - a.id_begin) >> 6] = good;
            if (bad) atomicAdd(&a.counts[0], (unsigned long long)__popcll(bad));
            if (out) atomicAdd(&a.counts[1], (unsigned long long)__popcll(out));
        }
    }
}

// after the encode: a row without a span came back as the NULL code -1; in a table indexed by id it is "no code", -2
__global__ __launch_bounds__(256) void sd_map_absent_kernel(int32_t* codes, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        if (codes[i] < 0) codes[i] = -2;
}

}  // namespace vnm

using namespace vnm;

struct vnm_strdict {
    SDict d{};
    uint8_t* heap = nullptr;
    int64_t heap_cap = 0, heap_used = 0;
    unsigned long long* gnext = nullptr;     // device: first id not handed out yet
    int64_t ids = 0;                         // its host copy after the last encode
    std::vector<int32_t> new_ids, new_lens;  // the values the last encode added, in heap order
    std::vector<uint8_t> new_bytes;
    // An encode that fails between the encode kernel and the compaction leaves slots published as `NEW | row of a batch that is gone`:
    // the next encode would resolve them through ITS batch's offsets (wrong matches, reads out of range).  Such a handle refuses
    // further use.
    bool failed = false;
    // id -> heap offset / length (written by the compaction; -1 length: never handed out), for vnm_strdict_like
    int64_t* id_off = nullptr;
    int32_t* id_len = nullptr;
    int64_t id_cap = 0;
    std::map<std::string, std::pair<int32_t*, int>> like_patterns;   // pattern -> its tokens + bytes on the device, token count
    // (ids, heap_used) after every encode that added values: an id >= marks[k].first lies at or above heap offset marks[k].second
    // (ids are never handed out again and the heap only grows) -- where vnm_strdict_map_codepoints' scratch for [id_begin, ids) starts
    std::vector<std::pair<int64_t, int64_t>> marks;
    // as the DESTINATION of vnm_strdict_map_codepoints: the code point map this dictionary was derived with, uploaded once
    int32_t* map_dev = nullptr;              // [n] from, [n] to, 128 bytes ASCII image
    std::vector<int32_t> map_host;           // from + to, to recognise the map on the next call
    int map_ascii_closed = 0;
    // as the DESTINATION of vnm_strdict_concat_affix: prefix | suffix this dictionary was derived with, uploaded once
    uint8_t* affix_dev = nullptr;
    std::string affix_host;
    int64_t affix_pre = -1;
};

// the id-indexed arrays cover every id handed out so far (ids come in chunks, so they grow even when no value is new)
static int strdict_ensure_ids(vnm_strdict* h, int64_t ids, hipStream_t s) {
    if (ids <= h->id_cap) return 0;
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(ids, 2 * h->id_cap), 1 << 16);
    int64_t* off = (int64_t*)pool_alloc((size_t)cap * 8);
    int32_t* len = (int32_t*)pool_alloc((size_t)cap * 4);
    if (!off || !len) { pool_free(off); pool_free(len); return set_error("vnm_strdict: id table allocation failed"); }
    if (h->id_cap) {
        VNM_HIP(hipMemcpyAsync(off, h->id_off, (size_t)h->id_cap * 8, hipMemcpyDeviceToDevice, s));
        VNM_HIP(hipMemcpyAsync(len, h->id_len, (size_t)h->id_cap * 4, hipMemcpyDeviceToDevice, s));
    }
    VNM_HIP(hipMemsetAsync(len + h->id_cap, 0xFF, (size_t)(cap - h->id_cap) * 4, s));
    pool_free_after(h->id_off, s);
    pool_free_after(h->id_len, s);
    h->id_off = off; h->id_len = len; h->id_cap = cap;
    return 0;
}

extern "C" {

vnm_strdict* vnm_strdict_create(void) {
    if (ensure_init()) return nullptr;
    return new vnm_strdict();
}

void vnm_strdict_destroy(vnm_strdict* h) {
    if (!h) return;
    if (h->d.slot) sdict_free(&h->d);
    pool_free(h->heap);
    pool_free(h->gnext);
    pool_free(h->id_off);
    pool_free(h->id_len);
    for (auto& kv : h->like_patterns) pool_free(kv.second.first);
    pool_free(h->map_dev);
    pool_free(h->affix_dev);
    delete h;
}

int64_t vnm_strdict_ids(vnm_strdict* h) { return h ? h->ids : 0; }

static int strdict_encode_device_impl(vnm_strdict* h, const vnm_dcol* offsets, const int32_t* span_lens, const uint8_t* validity, int64_t validity_offset,
                                      const uint8_t* data, int64_t data_base, int32_t* out_codes, int64_t* n_new, int64_t* new_bytes, void* stream);

int vnm_strdict_encode_device(vnm_strdict* h, const vnm_dcol* offsets, const uint8_t* validity, int64_t validity_offset,
                              const uint8_t* data, int64_t data_base, int32_t* out_codes, int64_t* n_new, int64_t* new_bytes, void* stream) {
    if (h && h->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    const int rc = strdict_encode_device_impl(h, offsets, nullptr, validity, validity_offset, data, data_base, out_codes, n_new, new_bytes, stream);
    if (rc && h && h->d.slot) {
        (void)hipStreamSynchronize(as_stream(stream));   // (scratch of the failed call goes back to the pool: nothing may still be running on it)
        h->failed = true;
    }
    return rc;
}

// The same over SPANS of one device byte buffer: row r is the lens[r] bytes at data[starts[r]] (no NULLs).  How vnm_csv_parse_block_ex
// encodes the string columns of a CSV block where they lie in the staged text.
int vnm_strdict_encode_spans(vnm_strdict* h, const int64_t* starts, const int32_t* lens, int64_t n, const uint8_t* data, int32_t* out_codes,
                             int64_t* n_new, int64_t* new_bytes, void* stream) {
    if (h && h->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (n > 0 && (!starts || !lens || !data)) return set_error("vnm_strdict_encode_spans: null argument");
    vnm_dcol offs{};
    offs.values = (void*)starts; offs.type = VNM_I64; offs.offset = 0; offs.length = n + 1;
    const int rc = strdict_encode_device_impl(h, &offs, lens, nullptr, 0, data, 0, out_codes, n_new, new_bytes, stream);
    if (rc && h && h->d.slot) {
        (void)hipStreamSynchronize(as_stream(stream));
        h->failed = true;
    }
    return rc;
}

int vnm_strdict_last_new(vnm_strdict* h, int64_t* n_new, int64_t* new_bytes) {
    if (!h) return set_error("vnm_strdict_last_new: null handle");
    if (n_new) *n_new = (int64_t)h->new_ids.size();
    if (new_bytes) *new_bytes = (int64_t)h->new_bytes.size();
    return 0;
}

static int strdict_encode_device_impl(vnm_strdict* h, const vnm_dcol* offsets, const int32_t* span_lens, const uint8_t* validity, int64_t validity_offset,
                                      const uint8_t* data, int64_t data_base, int32_t* out_codes, int64_t* n_new, int64_t* new_bytes, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !offsets || !out_codes) return set_error("vnm_strdict_encode_device: null argument");
    if (offsets->type != VNM_I32 && offsets->type != VNM_I64) return set_error("vnm_strdict_encode_device: offsets must be int32 or int64");
    hipStream_t s = as_stream(stream);
    const int64_t nrows = offsets->length - 1;   // n + 1 offsets
    h->new_ids.clear(); h->new_lens.clear(); h->new_bytes.clear();
    if (n_new) *n_new = 0;
    if (new_bytes) *new_bytes = 0;
    if (nrows <= 0) return 0;
    if (!h->d.slot) {
        VNM_TRY(sdict_alloc(&h->d, 1 << 16, s));
        h->gnext = (unsigned long long*)pool_alloc(64);
        if (!h->gnext) return 1;
        VNM_HIP(hipMemsetAsync(h->gnext, 0, 8, s));
    }
    PoolScope pool;
    SdArgs a{};
    a.offs = offsets->values; a.wide = offsets->type == VNM_I64; a.first = offsets->offset;
    a.lens = span_lens;
    a.valid = validity; a.vfirst = validity_offset;
    a.data = data; a.data_base = data_base;
    a.nrows = nrows;
    a.ntiles = (nrows + SD_TILE - 1) / SD_TILE;
    a.out = out_codes;
    a.gnext = h->gnext;
    a.heap = h->heap;
    int grid = device_info().num_cus * 4;
    if (grid > a.ntiles) grid = (int)a.ntiles;
    a.margin = (int64_t)grid * SD_TILE;
    a.progress = (unsigned int*)pool.take((size_t)grid * 4);
    if (!a.progress) return 1;
    VNM_HIP(hipMemsetAsync(a.progress, 0, (size_t)grid * 4, s));
    VNM_HIP(hipMemsetAsync(h->d.ctl + 3, 0, 8, s));   // values new in this batch
    for (int round = 0;; round++) {
        while ((int64_t)(h->d.cap * 7 / 10) < a.margin + 1) VNM_TRY(sdict_grow(&h->d, h->d.cap * 4, s));
        VNM_HIP(hipMemsetAsync(h->d.ctl, 0, 16, s));   // [1] the flag; [2], [3] persist
        a.d = h->d;
        a.fill_limit = (int64_t)(h->d.cap * 7 / 10);
        {
            KernelTimer timer("strdict_encode", s);
            sd_encode_kernel<<<grid, 256, 0, s>>>(a);
        }
        VNM_HIP(hipGetLastError());
        unsigned long long ctl[4];
        VNM_HIP(hipMemcpyAsync(ctl, h->d.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (!ctl[1]) break;
        VNM_TRY(sdict_grow(&h->d, h->d.cap * (round >= 1 ? 16 : 4), s));   // the workgroups resume from progress[]
    }
    unsigned long long fresh = 0, gn = 0;
    VNM_HIP(hipMemcpyAsync(&fresh, h->d.ctl + 3, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(&gn, h->gnext, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    h->ids = (int64_t)gn;
    if (gn >= (1ULL << 31)) return set_error("vnm_strdict: more than 2^31 dictionary ids");
    VNM_TRY(strdict_ensure_ids(h, (int64_t)gn, s));
    if (!fresh) return 0;
    // ---- the new values -> the heap
    SdCompact c{};
    c.d = h->d;
    const int64_t threads = ((int64_t)h->d.cap + SD_PER - 1) / SD_PER;
    c.nblocks = (int)((threads + 255) / 256);
    c.pre_cnt = (uint32_t*)pool.take((size_t)c.nblocks * 256 * 4);
    c.pre_bytes = (unsigned long long*)pool.take((size_t)c.nblocks * 256 * 8);
    c.blk = (unsigned long long*)pool.take(((size_t)c.nblocks + 1) * 16);
    c.new_ids = (int32_t*)pool.take((size_t)fresh * 4);
    c.new_lens = (int32_t*)pool.take((size_t)fresh * 4);
    if (!c.pre_cnt || !c.pre_bytes || !c.blk || !c.new_ids || !c.new_lens) return 1;
    unsigned long long tot[2] = {0, 0};
    {
        KernelTimer timer("strdict_compact", s);
        sd_compact_count_kernel<<<c.nblocks, 256, 0, s>>>(c);
        sd_compact_scan_kernel<<<1, 1024, 0, s>>>(c.blk, c.nblocks);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(tot, c.blk + 2 * (size_t)c.nblocks, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (tot[0] != fresh) return set_error("vnm_strdict: %llu new values counted, %llu claimed (internal error)", tot[0], fresh);
    if (h->heap_used + (int64_t)tot[1] > h->heap_cap) {
        const int64_t want = std::max<int64_t>((h->heap_used + (int64_t)tot[1]) * 2, 1 << 20);
        uint8_t* nh = (uint8_t*)pool_alloc((size_t)want);
        if (!nh) return 1;
        if (h->heap_used) VNM_HIP(hipMemcpyAsync(nh, h->heap, (size_t)h->heap_used, hipMemcpyDeviceToDevice, s));
        VNM_HIP(hipStreamSynchronize(s));
        pool_free(h->heap);
        h->heap = nh;
        h->heap_cap = want;
    }
    c.in = a;
    c.id_off = h->id_off;
    c.id_len = h->id_len;
    c.heap = h->heap;
    c.heap_used = (unsigned long long)h->heap_used;
    {
        KernelTimer timer("strdict_compact", s);
        sd_compact_move_kernel<<<c.nblocks, 256, 0, s>>>(c);
    }
    VNM_HIP(hipGetLastError());
    h->new_ids.resize((size_t)fresh); h->new_lens.resize((size_t)fresh); h->new_bytes.resize((size_t)tot[1]);
    VNM_HIP(hipMemcpyAsync(h->new_ids.data(), c.new_ids, (size_t)fresh * 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(h->new_lens.data(), c.new_lens, (size_t)fresh * 4, hipMemcpyDeviceToHost, s));
    if (tot[1]) VNM_HIP(hipMemcpyAsync(h->new_bytes.data(), h->heap + h->heap_used, (size_t)tot[1], hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    h->heap_used += (int64_t)tot[1];
    h->marks.emplace_back(h->ids, h->heap_used);
    if (n_new) *n_new = (int64_t)fresh;
    if (new_bytes) *new_bytes = (int64_t)tot[1];
    return 0;
}

int vnm_strdict_encode(vnm_strdict* h, const void* offsets_host, int offsets_are_64, const uint8_t* data_host, const uint8_t* validity_host,
                       int64_t offset, int64_t length, int32_t* out_codes_host, int64_t* n_new, int64_t* new_bytes, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || (length > 0 && (!offsets_host || !out_codes_host))) return set_error("vnm_strdict_encode: null argument");
    if (n_new) *n_new = 0;
    if (new_bytes) *new_bytes = 0;
    h->new_ids.clear(); h->new_lens.clear(); h->new_bytes.clear();
    if (length <= 0) return 0;
    hipStream_t s = as_stream(stream);
    int64_t b0, b1;
    if (offsets_are_64) { b0 = ((const int64_t*)offsets_host)[offset]; b1 = ((const int64_t*)offsets_host)[offset + length]; }
    else { b0 = ((const int32_t*)offsets_host)[offset]; b1 = ((const int32_t*)offsets_host)[offset + length]; }
    if (b1 < b0) return set_error("vnm_strdict_encode: offsets decrease");
    if (b1 > b0 && !data_host) return set_error("vnm_strdict_encode: null data buffer");
    // the column crosses PCIe once: n + 1 offsets, the bytes of the validity bitmap that cover the rows, the bytes the rows refer to
    struct Cols { vnm_dcol offs{}, data{}, bits{}; ~Cols() { vnm_free_column(&offs); vnm_free_column(&data); vnm_free_column(&bits); } } st;
    VNM_TRY(vnm_stage_column(offsets_host, nullptr, offset, length + 1, offsets_are_64 ? VNM_I64 : VNM_I32, &st.offs, stream));
    if (validity_host) VNM_TRY(vnm_stage_column(validity_host, nullptr, offset >> 3, ((offset + length + 7) >> 3) - (offset >> 3), VNM_U8, &st.bits, stream));
    if (b1 > b0) VNM_TRY(vnm_stage_column(data_host, nullptr, b0, b1 - b0, VNM_U8, &st.data, stream));
    int32_t* codes = (int32_t*)pool_alloc((size_t)length * 4);
    if (!codes) return 1;
    int rc = vnm_strdict_encode_device(h, &st.offs, validity_host ? (const uint8_t*)st.bits.values : nullptr, offset & 7,
                                       (const uint8_t*)st.data.values, b0, codes, n_new, new_bytes, stream);
    if (!rc && (hipMemcpyAsync(out_codes_host, codes, (size_t)length * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
        rc = set_error("vnm_strdict_encode: copying the codes back failed");
    pool_free(codes);
    return rc;
}

int vnm_strdict_fetch_new(vnm_strdict* h, int32_t* ids_host, int32_t* lens_host, uint8_t* bytes_host) {
    if (!h) return set_error("vnm_strdict_fetch_new: null handle");
    if (!h->new_ids.empty()) {
        memcpy(ids_host, h->new_ids.data(), h->new_ids.size() * 4);
        memcpy(lens_host, h->new_lens.data(), h->new_lens.size() * 4);
    }
    if (!h->new_bytes.empty()) memcpy(bytes_host, h->new_bytes.data(), h->new_bytes.size());
    h->new_ids.clear(); h->new_lens.clear(); h->new_bytes.clear();   // (handed over once: a second fetch without an encode in between brings nothing)
    return 0;
}

// The value list (heap + voff[i], vlen[i]; D values, the longest `maxlen` bytes) sorted byte-wise: *perm_out[i] = the index of the value
// at sorted position i.  Scratch comes from `pool`.
static int sd_sort_value_list(const uint8_t* heap, const uint64_t* voff, const uint32_t* vlen, int64_t D, unsigned long long maxlen,
                              const char* route, PoolScope& pool, int64_t** perm_out, void* stream) {
    hipStream_t s = as_stream(stream);
    int64_t* perm = (int64_t*)pool.take((size_t)D * 8);
    int64_t* perm2 = (int64_t*)pool.take((size_t)D * 8);
    int64_t* perm3 = (int64_t*)pool.take((size_t)D * 8);
    if (!perm || !perm2 || !perm3) return 1;
    const int m = (int)((maxlen + 7) / 8);                    // chunks of the longest value
    route_note(route, "%lld distinct values, longest %llu bytes: %d round(s) of up to 15 chunk keys + the length", (long long)D, maxlen, m == 0 ? 1 : (m + 14) / 15);
    constexpr int PER = 15;                                   // chunk keys per sort call (+ the length: 16 keys)
    const int rounds = m == 0 ? 1 : (m + PER - 1) / PER;
    uint64_t* keys = (uint64_t*)pool.take((size_t)D * 8 * (size_t)(std::min(m, PER) + 1));
    if (!keys) return 1;
    const int g2 = (int)std::min<int64_t>((D + 255) / 256, (int64_t)device_info().num_cus * 8);
    bool have_perm = false;
    for (int r = 0; r < rounds; r++) {                        // least significant round first: the last chunks and the length
        const int hi = m - r * PER, lo = std::max(0, hi - PER), nc = hi - lo;
        const int with_len = r == 0 ? 1 : 0;
        sd_chunk_kernel<<<g2, 256, 0, s>>>(heap, voff, vlen, have_perm ? perm : nullptr, D, lo, nc, with_len, keys);
        VNM_HIP(hipGetLastError());
        vnm_dcol kc[16];
        int orders[16];
        const int nk = nc + with_len;
        for (int k = 0; k < nk; k++) {
            memset(&kc[k], 0, sizeof(vnm_dcol));
            kc[k].values = keys + (size_t)k * D; kc[k].type = VNM_U64; kc[k].length = D;
            orders[k] = VNM_ASC;
        }
        VNM_TRY(vnm_sort_indices(nk, kc, orders, D, 0, perm2, stream));
        if (!have_perm) std::swap(perm, perm2);
        else {                                                // positions in this round's order -> value indices
            vnm_dcol pc{};
            pc.values = perm; pc.type = VNM_I64; pc.length = D;
            VNM_TRY(vnm_take(&pc, perm2, D, perm3, nullptr, stream));
            std::swap(perm, perm3);
        }
        have_perm = true;
    }
    *perm_out = perm;
    return 0;
}

// Order-preserving ranks of every value in the dictionary: out_rank_of_id[id] = position of the value in ascending byte-wise order
// (device array of vnm_strdict_ids(h) int32s; ids that were never handed out are left untouched).
int vnm_strdict_ranks_device(vnm_strdict* h, int32_t* out_rank_of_id, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !out_rank_of_id) return set_error("vnm_strdict_ranks_device: null argument");
    if (h->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (!h->d.slot) return 0;
    hipStream_t s = as_stream(stream);
    unsigned long long fill = 0;
    VNM_HIP(hipMemcpyAsync(&fill, h->d.ctl + 2, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    const int64_t D = (int64_t)fill;
    if (D == 0) return 0;
    PoolScope pool;
    SdRankArgs a{};
    a.d = h->d; a.heap = h->heap;
    a.voff = (uint64_t*)pool.take((size_t)D * 8);
    a.vlen = (uint32_t*)pool.take((size_t)D * 4);
    a.vid = (int32_t*)pool.take((size_t)D * 4);
    a.ctl = (unsigned long long*)pool.take(64);
    if (!a.voff || !a.vlen || !a.vid || !a.ctl) return 1;
    VNM_HIP(hipMemsetAsync(a.ctl, 0, 64, s));
    const int grid = (int)std::min<int64_t>(((int64_t)h->d.cap + 255) / 256, (int64_t)device_info().num_cus * 8);
    sd_list_kernel<<<grid, 256, 0, s>>>(a);
    VNM_HIP(hipGetLastError());
    unsigned long long ctl[2];
    VNM_HIP(hipMemcpyAsync(ctl, a.ctl, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if ((int64_t)ctl[0] != D) return set_error("vnm_strdict_ranks_device: %llu values listed, %lld in the table (internal error)", ctl[0], (long long)D);
    int64_t* perm = nullptr;
    VNM_TRY(sd_sort_value_list(h->heap, a.voff, a.vlen, D, ctl[1], "sort:string_key_ranks", pool, &perm, stream));
    const int g2 = (int)std::min<int64_t>((D + 255) / 256, (int64_t)device_info().num_cus * 8);
    sd_rank_scatter_kernel<<<g2, 256, 0, s>>>(perm, a.vid, D, out_rank_of_id);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    return 0;
}

// codes (vnm_strdict_encode*) -> the rows' ranks under rank_of_id (vnm_strdict_ranks_device); all device buffers
int vnm_strdict_codes_to_ranks(const int32_t* codes, const int32_t* rank_of_id, int64_t n, int32_t* out_ranks, void* stream) {
    VNM_TRY(ensure_init());
    if (n <= 0) return 0;
    if (!codes || !rank_of_id || !out_ranks) return set_error("vnm_strdict_codes_to_ranks: null argument");
    sd_code_rank_kernel<<<(int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, as_stream(stream)>>>(codes, rank_of_id, n, out_ranks);
    VNM_HIP(hipGetLastError());
    return 0;
}

// out_dst_code_of_src_id[id] = the code `dst` holds for the bytes of src's value `id`, for id in [id_begin, vnm_strdict_ids(src));
// -2: dst does not hold them, or the id was never handed out.  One kernel on `stream`, launched asynchronously; dst is only read.
int vnm_strdict_translate(vnm_strdict* src, vnm_strdict* dst, int64_t id_begin, int32_t* out_dst_code_of_src_id, void* stream) {
    VNM_TRY(ensure_init());
    if (!src || !dst || !out_dst_code_of_src_id) return set_error("vnm_strdict_translate: null argument");
    if (src->failed || dst->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (id_begin < 0) return set_error("vnm_strdict_translate: id_begin < 0");
    if (id_begin >= src->ids) return 0;
    SdTransArgs a{};
    a.sheap = src->heap; a.s_off = src->id_off; a.s_len = src->id_len;
    a.d = dst->d; a.dheap = dst->heap;
    a.id_begin = id_begin; a.id_end = src->ids;
    a.out = out_dst_code_of_src_id;
    hipStream_t s = as_stream(stream);
    const int grid = (int)std::min<int64_t>((src->ids - id_begin + 255) / 256, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("strdict_translate", s);
        sd_translate_kernel<<<grid, 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

static int utf8_width(int64_t cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }

// Every value of `src` with an id in [id_begin, vnm_strdict_ids(src)) mapped code point by code point (map_from -> map_to) and
// found or inserted in `dst`: out_dst_code_of_src_id[id] = dst's code of the image, -2 for an id never handed out and for a
// malformed value.  sd_map_kernel writes the images, strdict_encode_device_impl (the spans form) inserts them: afterwards dst's
// new values are fetched as after any encode.  The encode reads counts back, so the call returns when the table is written.
int vnm_strdict_map_codepoints(vnm_strdict* src, vnm_strdict* dst, const int32_t* map_from, const int32_t* map_to, int64_t n_map,
                               int64_t id_begin, int32_t* out_dst_code_of_src_id, int64_t* out_invalid, void* stream) {
    VNM_TRY(ensure_init());
    if (out_invalid) *out_invalid = 0;
    if (!src || !dst || !out_dst_code_of_src_id || (n_map > 0 && (!map_from || !map_to))) return set_error("vnm_strdict_map_codepoints: null argument");
    if (src == dst) return set_error("vnm_strdict_map_codepoints: src and dst are one dictionary (src is only read, dst grows)");
    if (src->failed || dst->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (id_begin < 0) return set_error("vnm_strdict_map_codepoints: id_begin < 0");
    if (n_map < 0 || n_map > MC_MAX_MAP) return set_error("vnm_strdict_map_codepoints: a map of %lld pairs (0..%d are held)", (long long)n_map, MC_MAX_MAP);
    // ---- the map: checked on the host, uploaded once per dst handle
    if (!dst->map_dev) {
        int closed = 1;
        for (int64_t i = 0; i < n_map; i++) {
            const int64_t f = map_from[i], t = map_to[i];
            if (f < 0 || f > 0x10FFFF || t < 0 || t > 0x10FFFF) return set_error("vnm_strdict_map_codepoints: pair %lld (U+%04llX -> U+%04llX) is no code point", (long long)i, (long long)f, (long long)t);
            if (i > 0 && map_from[i - 1] >= f) return set_error("vnm_strdict_map_codepoints: map_from must be strictly ascending (entry %lld: U+%04llX after U+%04llX)", (long long)i, (long long)f, (long long)map_from[i - 1]);
            if (utf8_width(t) > 2 * utf8_width(f))
                return set_error("vnm_strdict_map_codepoints: U+%04llX (%d byte) -> U+%04llX (%d bytes): an image may be at most twice as long as its source, the room a value has",
                                 (long long)f, utf8_width(f), (long long)t, utf8_width(t));
            if (f < 0x80 && t >= 0x80) closed = 0;
        }
        std::vector<int32_t> blob((size_t)n_map * 2 + 32, 0);
        if (n_map) { memcpy(blob.data(), map_from, (size_t)n_map * 4); memcpy(blob.data() + n_map, map_to, (size_t)n_map * 4); }
        uint8_t* ascii = (uint8_t*)(blob.data() + 2 * n_map);
        for (int b = 0; b < 128; b++) ascii[b] = (uint8_t)b;
        if (closed)
            for (int64_t i = 0; i < n_map && map_from[i] < 0x80; i++) ascii[map_from[i]] = (uint8_t)map_to[i];
        int32_t* dev = (int32_t*)pool_alloc(blob.size() * 4);
        if (!dev) return 1;
        if (hipMemcpy(dev, blob.data(), blob.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { pool_free(dev); return set_error("vnm_strdict_map_codepoints: map upload failed"); }
        dst->map_dev = dev;
        dst->map_host.assign(blob.begin(), blob.begin() + 2 * n_map);
        dst->map_ascii_closed = closed;
    } else if ((int64_t)dst->map_host.size() != 2 * n_map || (n_map && (memcmp(dst->map_host.data(), map_from, (size_t)n_map * 4) ||
                                                                        memcmp(dst->map_host.data() + n_map, map_to, (size_t)n_map * 4)))) {
        return set_error("vnm_strdict_map_codepoints: dst was derived with another map");
    }
    dst->new_ids.clear(); dst->new_lens.clear(); dst->new_bytes.clear();
    const int64_t n = src->ids - id_begin;
    if (n <= 0) return 0;
    hipStream_t s = as_stream(stream);
    int64_t heap_base = 0;
    for (const auto& m : src->marks)
        if (m.first <= id_begin) heap_base = m.second;
    PoolScope pool;
    SdMapArgs a{};
    a.sheap = src->heap; a.s_off = src->id_off; a.s_len = src->id_len;
    a.map = dst->map_dev; a.n_map = (int)n_map; a.ascii_closed = dst->map_ascii_closed;
    for (int p = 1; p <= a.n_map; p <<= 1) a.top_step = p;
    a.id_begin = id_begin; a.id_end = src->ids;
    a.heap_base = heap_base;
    a.scratch_bytes = 2 * (src->heap_used - heap_base);
    const int64_t words = (n + 63) / 64;
    a.scratch = (uint8_t*)pool.take((size_t)std::max<int64_t>(a.scratch_bytes, 8));
    a.starts = (int64_t*)pool.take((size_t)n * 8);
    a.lens = (int32_t*)pool.take((size_t)n * 4);
    a.valid = (unsigned long long*)pool.take((size_t)words * 8);
    a.counts = (unsigned long long*)pool.take(16);
    if (!a.scratch || !a.starts || !a.lens || !a.valid || !a.counts) return 1;
    VNM_HIP(hipMemsetAsync(a.counts, 0, 16, s));
    const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8);
    {
        KernelTimer timer("strdict_map_codepoints", s);
        sd_map_kernel<<<grid, 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    vnm_dcol offs{};
    offs.values = (void*)a.starts; offs.type = VNM_I64; offs.offset = 0; offs.length = n + 1;
    int32_t* out = out_dst_code_of_src_id + id_begin;
    const int rc = strdict_encode_device_impl(dst, &offs, a.lens, (const uint8_t*)a.valid, 0, a.scratch, 0, out, nullptr, nullptr, stream);
    if (rc) {
        (void)hipStreamSynchronize(s);
        if (dst->d.slot) dst->failed = true;
        return rc;
    }
    sd_map_absent_kernel<<<(int)std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8), 256, 0, s>>>(out, n);
    VNM_HIP(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    VNM_HIP(hipMemcpyAsync(counts, a.counts, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));     // (the scratch goes back to the pool with this scope)
    if (counts[1]) return set_error("vnm_strdict_map_codepoints: %llu value(s) lay outside the scratch buffer (internal error)", counts[1]);
    if (out_invalid) {
        *out_invalid = (int64_t)counts[0];
        if (counts[0]) return set_error("Invalid UTF8 sequence in input (%llu of %lld dictionary value(s))", counts[0], (long long)n);
    }
    return 0;
}

// Dense ranks of the values of BOTH dictionaries in the ascending byte order of their union (the order of vnm_strdict_ranks_device);
// equal bytes in a and b share a rank.  Entries of ids never handed out are left untouched.
int vnm_strdict_ranks_joint(vnm_strdict* a, vnm_strdict* b, int32_t* out_rank_of_id_a, int32_t* out_rank_of_id_b, void* stream) {
    VNM_TRY(ensure_init());
    if (!a || !b || !out_rank_of_id_a || !out_rank_of_id_b) return set_error("vnm_strdict_ranks_joint: null argument");
    if (a->failed || b->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    hipStream_t s = as_stream(stream);
    vnm_strdict* hs[2] = {a, a == b ? nullptr : b};     // (one handle twice: its values once, both outputs get its ranks)
    unsigned long long fill[2] = {0, 0};
    for (int k = 0; k < 2; k++)
        if (hs[k] && hs[k]->d.slot) VNM_HIP(hipMemcpyAsync(&fill[k], hs[k]->d.ctl + 2, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    const int64_t Da = (int64_t)fill[0], D = Da + (int64_t)fill[1];
    if (D == 0) return 0;
    if (D >= (1LL << 31)) return set_error("vnm_strdict_ranks_joint: more than 2^31 values");
    PoolScope pool;
    uint64_t* vaddr = (uint64_t*)pool.take((size_t)D * 8);
    uint32_t* vlen = (uint32_t*)pool.take((size_t)D * 4);
    int32_t* vid = (int32_t*)pool.take((size_t)D * 4);
    unsigned long long* lctl = (unsigned long long*)pool.take(128);
    if (!vaddr || !vlen || !vid || !lctl) return 1;
    VNM_HIP(hipMemsetAsync(lctl, 0, 128, s));
    for (int k = 0; k < 2; k++) {
        if (!fill[k]) continue;
        const int64_t at = k ? Da : 0;
        SdRankArgs l{};
        l.d = hs[k]->d; l.heap = hs[k]->heap; l.base = (uint64_t)hs[k]->heap;
        l.voff = vaddr + at; l.vlen = vlen + at; l.vid = vid + at;
        l.ctl = lctl + 8 * k;
        const int grid = (int)std::min<int64_t>(((int64_t)hs[k]->d.cap + 255) / 256, (int64_t)device_info().num_cus * 8);
        sd_list_kernel<<<grid, 256, 0, s>>>(l);
        VNM_HIP(hipGetLastError());
    }
    unsigned long long ctl[16];
    VNM_HIP(hipMemcpyAsync(ctl, lctl, 128, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (ctl[0] != fill[0] || ctl[8] != fill[1])
        return set_error("vnm_strdict_ranks_joint: %llu + %llu values listed, %llu + %llu in the tables (internal error)", ctl[0], ctl[8], fill[0], fill[1]);
    int64_t* perm = nullptr;
    VNM_TRY(sd_sort_value_list(nullptr, vaddr, vlen, D, std::max(ctl[1], ctl[9]), "project:string_joint_ranks", pool, &perm, stream));
    SdJointArgs j{};
    j.perm = perm; j.vaddr = vaddr; j.vlen = vlen; j.vid = vid;
    j.n = D; j.n_a = Da;
    const int64_t threads = (D + SD_PER - 1) / SD_PER;
    const int nblocks = (int)((threads + 255) / 256);
    j.flag = (uint8_t*)pool.take((size_t)D);
    j.pre = (uint32_t*)pool.take((size_t)nblocks * 256 * 4);
    j.blk = (unsigned long long*)pool.take(((size_t)nblocks + 1) * 16);
    if (!j.flag || !j.pre || !j.blk) return 1;
    j.rank_a = out_rank_of_id_a;
    j.rank_b = out_rank_of_id_b;
    j.both = a == b;
    {
        KernelTimer timer("strdict_joint_dense_ranks", s);   // (the flag / scan / rank step alone: the list and chunk kernels are untimed, the sort has its own timers)
        sd_joint_flag_kernel<<<nblocks, 256, 0, s>>>(j);
        sd_compact_scan_kernel<<<1, 1024, 0, s>>>(j.blk, nblocks);
        sd_joint_rank_kernel<<<nblocks, 256, 0, s>>>(j);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));     // (the scratch goes back to the pool with this scope)
    return 0;
}

int vnm_like_compile(const uint8_t* pattern, int64_t pattern_len, int32_t* out_tokens, int64_t* n_tokens) {
    if (pattern_len < 0 || (pattern_len > 0 && !pattern) || !out_tokens || !n_tokens) return set_error("vnm_like_compile: null argument");
    if (pattern_len >= (1LL << 31)) return set_error("vnm_like_compile: pattern too long");
    int64_t nt = 0;
    for (int64_t i = 0; i < pattern_len;) {
        const uint8_t b = pattern[i];
        if (strchr("\\^$*+?{}[]|()", b) && b)
            return set_error("no GPU lowering for the LIKE pattern: '%c' has a regex meaning in the reference that LIKE does not restate", b);
        if (b == '%') {
            if (nt == 0 || out_tokens[3 * (nt - 1)] != VNM_LIKE_TOK_STAR) { out_tokens[3 * nt] = VNM_LIKE_TOK_STAR; out_tokens[3 * nt + 1] = (int32_t)i; out_tokens[3 * nt + 2] = 1; nt++; }
            i++;
        } else if (b == '_' || b == '.') {
            out_tokens[3 * nt] = VNM_LIKE_TOK_ANY; out_tokens[3 * nt + 1] = (int32_t)i; out_tokens[3 * nt + 2] = 1; nt++;
            i++;
        } else {   // a literal run: up to the next wildcard or metacharacter
            int64_t j = i;
            while (j < pattern_len && pattern[j] != '%' && pattern[j] != '_' && pattern[j] != '.' && !(pattern[j] && strchr("\\^$*+?{}[]|()", pattern[j]))) j++;
            out_tokens[3 * nt] = VNM_LIKE_TOK_LIT; out_tokens[3 * nt + 1] = (int32_t)i; out_tokens[3 * nt + 2] = (int32_t)(j - i); nt++;
            i = j;
        }
    }
    *n_tokens = nt;
    return 0;
}

int vnm_strdict_like(vnm_strdict* h, const uint8_t* pattern, int64_t pattern_len, int flags, int64_t id_begin,
                     uint8_t* out_match_of_id, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !out_match_of_id || pattern_len < 0 || (pattern_len > 0 && !pattern)) return set_error("vnm_strdict_like: null argument");
    if (h->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (flags & ~VNM_LIKE_STRIP_NUL) return set_error("vnm_strdict_like: unknown flags %d", flags);
    if (id_begin < 0) return set_error("vnm_strdict_like: id_begin < 0");
    const std::string key(pattern_len ? (const char*)pattern : "", (size_t)pattern_len);
    auto it = h->like_patterns.find(key);
    if (it == h->like_patterns.end()) {
        std::vector<int32_t> tok((size_t)std::max<int64_t>(pattern_len, 1) * 3);
        int64_t nt = 0;
        VNM_TRY(vnm_like_compile(pattern, pattern_len, tok.data(), &nt));
        for (int64_t k = 0; k < nt; k++)   // a literal run holding a newline fixes where everything before it matched
            if (tok[3 * k] == VNM_LIKE_TOK_LIT && memchr(pattern + tok[3 * k + 1], '\n', (size_t)tok[3 * k + 2])) tok[3 * k] = LK_LIT_NL;
        const size_t tb = (size_t)std::max<int64_t>(nt, 1) * 12;
        int32_t* dev = (int32_t*)pool_alloc(tb + (size_t)pattern_len + 1);
        if (!dev) return 1;
        std::vector<uint8_t> blob(tb + (size_t)pattern_len + 1, 0);
        memcpy(blob.data(), tok.data(), (size_t)nt * 12);
        if (pattern_len) memcpy(blob.data() + tb, pattern, (size_t)pattern_len);
        if (hipMemcpy(dev, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) { pool_free(dev); return set_error("vnm_strdict_like: pattern upload failed"); }
        it = h->like_patterns.emplace(key, std::make_pair(dev, (int)nt)).first;
    }
    if (id_begin >= h->ids) return 0;
    LikeArgs a{};
    a.heap = h->heap; a.id_off = h->id_off; a.id_len = h->id_len;
    a.tok = it->second.first;
    a.ntok = it->second.second;
    a.pat = (const uint8_t*)it->second.first + (size_t)std::max(a.ntok, 1) * 12;
    a.flags = flags;
    a.id_begin = id_begin; a.id_end = h->ids;
    a.out = out_match_of_id;
    hipStream_t s = as_stream(stream);
    const int grid = (int)std::min<int64_t>((h->ids - id_begin + 255) / 256, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("strdict_like", s);
        sd_like_kernel<<<grid, 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

static_assert(RM_TILE == VNM_STRDICT_REMAP_TILE, "the header documents the kernel's rows per workgroup");

int vnm_strdict_remap_indices(const vnm_dcol* indices, const int32_t* code_of_index, int64_t n_values, int32_t* out_codes,
                              uint8_t* out_validity, int64_t* out_bad, void* stream) {
    VNM_TRY(ensure_init());
    if (out_bad) *out_bad = 0;
    if (!indices) return set_error("vnm_strdict_remap_indices: null argument");
    const int64_t n = indices->length;
    if (n <= 0) return 0;
    if (!indices->values || !out_codes || (n_values > 0 && !code_of_index)) return set_error("vnm_strdict_remap_indices: null argument");
    if (n_values < 0 || indices->offset < 0) return set_error("vnm_strdict_remap_indices: negative n_values or offset");
    if (indices->type < VNM_I8 || indices->type > VNM_U64) return set_error("vnm_strdict_remap_indices: the indices must be of an integer type");
    static const int width[8] = {1, 2, 4, 8, 1, 2, 4, 8};   // VNM_I8 ... VNM_U64
    const int w = width[indices->type];
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    RemapArgs a{};
    a.idx = indices->values; a.valid = (const uint8_t*)indices->validity;
    a.first = indices->offset; a.n = n; a.n_values = n_values;
    a.table = code_of_index;
    a.out = out_codes; a.out_valid = out_validity;
    a.vec_in = (((uintptr_t)indices->values + (uintptr_t)indices->offset * (uintptr_t)w) & (w == 1 ? 7 : 15)) == 0;
    a.vec_out = ((uintptr_t)out_codes & 15) == 0;
    if (out_bad) {
        a.bad = (unsigned long long*)pool.take(8);
        if (!a.bad) return 1;
        VNM_HIP(hipMemsetAsync(a.bad, 0, 8, s));
    }
    const int64_t tiles = (n + RM_TILE - 1) / RM_TILE;
    if (tiles > 0x7FFFFFFFLL) return set_error("vnm_strdict_remap_indices: too many rows for one launch");
    a.ntiles = tiles;
    // the global form: one tile per workgroup, the table through L2.  The LDS form: a persistent grid, every workgroup copies the table
    // (up to 32 KB) into LDS once and takes several tiles -- taken when a workgroup's rows are at least 4x the values it copies
    // (VNM_REMAP_LDS=0 / 1: never / whenever the table fits, the A / B switch of tools/dictcol_bench.py)
    const char* sw = getenv("VNM_REMAP_LDS");
    const int64_t lds_grid = std::min<int64_t>(tiles, (int64_t)device_info().num_cus * 8);
    const int64_t rows_per_wg = (tiles + lds_grid - 1) / lds_grid * RM_TILE;
    const bool lds = n_values > 0 && n_values <= RM_LDS_VALUES && (sw ? sw[0] == '1' : rows_per_wg >= 4 * n_values);
    const dim3 grid((unsigned)(lds ? lds_grid : tiles));
#define VNM_REMAP_LAUNCH(T)                                      \
    do {                                                         \
        if (lds) sd_remap_kernel<T, true><<<grid, 256, 0, s>>>(a); \
        else sd_remap_kernel<T, false><<<grid, 256, 0, s>>>(a);    \
    } while (0)
    {
        KernelTimer timer("strdict_remap_indices", s);
        switch (indices->type) {
            case VNM_I8: VNM_REMAP_LAUNCH(int8_t); break;
            case VNM_I16: VNM_REMAP_LAUNCH(int16_t); break;
            case VNM_I32: VNM_REMAP_LAUNCH(int32_t); break;
            case VNM_I64: VNM_REMAP_LAUNCH(int64_t); break;
            case VNM_U8: VNM_REMAP_LAUNCH(uint8_t); break;
            case VNM_U16: VNM_REMAP_LAUNCH(uint16_t); break;
            case VNM_U32: VNM_REMAP_LAUNCH(uint32_t); break;
            default: VNM_REMAP_LAUNCH(uint64_t); break;
        }
    }
#undef VNM_REMAP_LAUNCH
    VNM_HIP(hipGetLastError());
    if (!out_bad) return 0;
    unsigned long long bad = 0;
    VNM_HIP(hipMemcpyAsync(&bad, a.bad, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    *out_bad = (int64_t)bad;
    if (bad) return set_error("vnm_strdict_remap_indices: dictionary index out of bounds (%llu row(s) of %lld, %lld value(s))", bad, (long long)n, (long long)n_values);
    return 0;
}

}  // extern "C"

#include "vnm_strconcat.inc"
#include "vnm_datetime.inc"
