// concat() / || over dictionary-coded string columns (ConcatFunction, vinum/core/functions.py:250-276).  Included at the end of
// vnm_strdict.hip: it reads the dictionaries' id tables and inserts through strdict_encode_device_impl, the one insert path.
//
// ONE column and literals -- concat('#', c, '!') -- is a function of the VALUE: vnm_strdict_concat_affix writes prefix +
// rstrip_nul(value) + suffix for every id of `src` (and for NULL: "None") into scratch spans and the spans go through dst's encode.
// TWO columns -- concat(a, sep, b) -- is a function of the row's PAIR of codes: vnm_strpair keeps an open-addressing table
// (code_a + 1) << 32 | (code_b + 1) -> code in dst across batches.  Per call:
//   find    one lane per 4 rows: both code columns in 16-byte loads, probe, CAS(EMPTY -> key).  A lane never waits for another lane
//           (no LOCKED state: the key IS the whole claim, the pair's code is filled in by a later kernel); the probe walk is bounded
//           (SP_WALK slots, never more than the capacity).  The winner of a CAS appends its slot to the new-pairs list (one atomic per wave); the row's SLOT goes to
//           out_codes.  Past the fill limit or the bound: the overflow flag -- raised at once, every wave
//           that sees it stops, since the pass is run again anyway --, the host grows the table x4 (sp_rehash_kernel re-inserts
//           key and code, pairs still without a code are listed again) and the find pass runs again -- inserts are idempotent.
//   concat  one lane per NEW pair: the image's exact length first (a reservation in the scratch buffer), then the bytes, every store
//           held against that room (vnm_strconcat.hpp); the spans go through dst's encode, the codes into the new slots.
//   gather  out_codes[i] = code_of_slot[out_codes[i]] in place, 16-byte accesses.
// String bytes are touched once per distinct pair; a row costs two 4-byte loads, one probe (an 8-byte load, L2) and one 4-byte gather.
#include "vnm_strconcat.hpp"

namespace vnm {

constexpr uint64_t SP_EMPTY = ~0ULL;
constexpr int SP_ROWS = 4;                 // rows per lane: one 16-byte load per code column, one 16-byte store
constexpr int SP_TILE = 256 * SP_ROWS;     // rows per workgroup and step
constexpr uint64_t SP_WALK = 1024;         // the longest probe walk (and never longer than the capacity): at 70 % fill a walk of linear probing
                                           // stays far below it; a longer one means the table is crowded, which is an overflow

struct SPair {
    uint64_t* keys;                // [cap] (code_a + 1) << 32 | (code_b + 1); SP_EMPTY
    int32_t* codes;                // [cap] the pair's code in dst; -1 until its image is inserted
    uint64_t cap;
};

__device__ __forceinline__ uint64_t sp_home(uint64_t key, uint64_t mask) {
    uint64_t h = key * 0x9E3779B97F4A7C15ULL;
    h ^= h >> 32;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 29;
    return h & mask;
}

__device__ __forceinline__ bool sp_bit(const uint8_t* bits, int64_t i) { return (bits[i >> 3] >> (i & 7)) & 1; }

struct SpFindArgs {
    SPair t;
    const int32_t* ca;             // row 0's code (the Arrow offset is applied); validity bit oa + row
    const uint8_t* va;
    int64_t oa;
    const int32_t* cb;
    const uint8_t* vb;
    int64_t ob;
    int64_t n, ntiles;
    int64_t ids_a, ids_b;          // codes lie in [-1, ids)
    int64_t fill_before, fill_limit;
    int32_t* out;                  // the row's slot; -1: not placed (overflow) or a code outside its dictionary
    uint32_t* list;                // slots claimed in this call
    int64_t list_cap;
    unsigned int* ctl;             // [0] 1: overflow, 2: the list is full (internal error)  [1] slots listed  [2] rows with a code outside its dictionary
                                   // [3] slots claimed (counted at the CAS itself: what the fill limit is held against)
    int vec;                       // ca, cb and out are 16-byte aligned
};

__global__ __launch_bounds__(256) void sp_find_kernel(SpFindArgs a) {
    const uint64_t mask = a.t.cap - 1, walk = a.t.cap < SP_WALK ? a.t.cap : SP_WALK;
    const int lane = threadIdx.x & 63;
    unsigned flag = 0, nbad = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {      // (trips uniform in a wave: every lane reaches the ballots)
        // once any lane has raised the overflow flag the host runs the whole pass again over a bigger table: nothing more to do here
        if (__any(__hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
        const int64_t row0 = (tile * 256 + threadIdx.x) * SP_ROWS;
        const int cnt = row0 >= a.n ? 0 : (a.n - row0 < SP_ROWS ? (int)(a.n - row0) : SP_ROWS);
        int32_t xa[SP_ROWS], xb[SP_ROWS], o[SP_ROWS];
        if (a.vec && cnt == SP_ROWS) {
            const int4 qa = *(const int4*)(a.ca + row0), qb = *(const int4*)(a.cb + row0);
            xa[0] = qa.x; xa[1] = qa.y; xa[2] = qa.z; xa[3] = qa.w;
            xb[0] = qb.x; xb[1] = qb.y; xb[2] = qb.z; xb[3] = qb.w;
        } else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) { xa[k] = k < cnt ? a.ca[row0 + k] : -1; xb[k] = k < cnt ? a.cb[row0 + k] : -1; }
        }
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const bool live = k < cnt;
            int64_t ia = xa[k], ib = xb[k];
            if (live && a.va && !sp_bit(a.va, a.oa + row0 + k)) ia = -1;
            if (live && a.vb && !sp_bit(a.vb, a.ob + row0 + k)) ib = -1;
            const bool bad = live && (ia < -1 || ia >= a.ids_a || ib < -1 || ib >= a.ids_b);
            if (bad) nbad++;
            int32_t slot = -1;
            bool won = false;
            if (live && !bad) {
                const uint64_t key = ((uint64_t)(uint32_t)(ia + 1) << 32) | (uint64_t)(uint32_t)(ib + 1);
                uint64_t h = sp_home(key, mask);
                for (uint64_t probes = 0; probes < walk; probes++) {
                    if ((probes & 15) == 15 && __hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                    uint64_t cur = sd_ld(a.t.keys + h);
                    if (cur == SP_EMPTY) {
                        const unsigned claimed = __hip_atomic_load(&a.ctl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (a.fill_before + (int64_t)claimed >= a.fill_limit) break;
                        if (__hip_atomic_compare_exchange_strong(a.t.keys + h, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            won = true;                    // the slot is this pair's, and this lane lists it
                            slot = (int32_t)h;
                            atomicAdd(&a.ctl[3], 1u);      // (no return value: the compiler folds a wave's adds into one)
                            break;
                        }                                  // (cur now holds what the slot had: this pair's key, or another's)
                    }
                    if (cur == key) { slot = (int32_t)h; break; }
                    h = (h + 1) & mask;
                }
                if (slot < 0 && !(flag & 1u)) {            // said at once, so that every other lane stops walking a crowded table
                    flag |= 1u;
                    atomicOr(&a.ctl[0], 1u);
                }
            }
            const unsigned long long winners = __ballot(won);
            if (winners) {                                  // one atomic per wave: the leader reserves, every winner stores
                const int leader = __ffsll((long long)winners) - 1;
                unsigned base = 0;
                if (lane == leader) base = atomicAdd(&a.ctl[1], (unsigned)__popcll(winners));
                base = __shfl(base, leader);
                if (won) {
                    const int64_t at = (int64_t)base + __popcll(winners & ((1ULL << lane) - 1));
                    if (at < a.list_cap) a.list[at] = (uint32_t)slot;
                    else flag |= 2u;
                }
            }
            o[k] = slot;
        }
        if (a.vec && cnt == SP_ROWS) *(int4*)(a.out + row0) = make_int4(o[0], o[1], o[2], o[3]);
        else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (k < cnt) a.out[row0 + k] = o[k];
        }
    }
    if (flag & 2u) atomicOr(&a.ctl[0], 2u);
    if (nbad) atomicAdd(&a.ctl[2], nbad);
}

// a bigger table: key and code move as they are (the keys are distinct: the first free slot of the probe walk); a pair whose image
// is not inserted yet (code -1: claimed by the find pass that overflowed) is listed again at its new slot
__global__ __launch_bounds__(256) void sp_rehash_kernel(SPair from, SPair to, uint32_t* list, int64_t list_cap, unsigned int* ctl) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const uint64_t mask = to.cap - 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)from.cap; i += stride) {
        const uint64_t key = from.keys[i];
        if (key == SP_EMPTY) continue;
        const int32_t code = from.codes[i];
        uint64_t h = sp_home(key, mask);
        for (uint64_t probes = 0; probes < to.cap; probes++) {
            uint64_t expected = SP_EMPTY;
            if (__hip_atomic_compare_exchange_strong(to.keys + h, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                to.codes[h] = code;
                if (code < 0) {
                    atomicAdd(&ctl[3], 1u);
                    const int64_t at = (int64_t)atomicAdd(&ctl[1], 1u);
                    if (at < list_cap) list[at] = (uint32_t)h;
                    else atomicOr(&ctl[0], 2u);
                }
                break;
            }
            h = (h + 1) & mask;
        }
    }
}

__global__ __launch_bounds__(256) void sp_store_codes_kernel(SPair t, const uint32_t* list, const int32_t* codes, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) t.codes[list[i]] = codes[i];
}

// out[i] = code_of_slot[out[i]] in place (-1 stays: only rows the call already refused hold it)
__global__ __launch_bounds__(256) void sp_gather_kernel(const int32_t* code_of_slot, int32_t* out, int64_t n, int64_t ntiles, int vec) {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * SP_ROWS;
        if (row0 >= n) break;
        if (vec && n - row0 >= SP_ROWS) {
            int4 q = *(const int4*)(out + row0);
            q.x = q.x < 0 ? -1 : code_of_slot[q.x]; q.y = q.y < 0 ? -1 : code_of_slot[q.y];
            q.z = q.z < 0 ? -1 : code_of_slot[q.z]; q.w = q.w < 0 ? -1 : code_of_slot[q.w];
            *(int4*)(out + row0) = q;
        } else {
            for (int k = 0; k < SP_ROWS && row0 + k < n; k++) { const int32_t sl = out[row0 + k]; out[row0 + k] = sl < 0 ? -1 : code_of_slot[sl]; }
        }
    }
}

// [0] occupied slots  [1] occupied slots without a code
__global__ __launch_bounds__(256) void sp_check_kernel(SPair t, unsigned long long* counts) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long occ = 0, half = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)t.cap; i += stride)
        if (t.keys[i] != SP_EMPTY) { occ++; if (t.codes[i] < 0) half++; }
    if (occ) atomicAdd(&counts[0], occ);
    if (half) atomicAdd(&counts[1], half);
}

// ---- the images: prefix + value(a) [+ sep + value(b)] + suffix as spans of a scratch buffer ------------------------------------------
struct ScSide {
    const uint8_t* heap;
    const int64_t* off;
    const int32_t* len;            // -1: an id never handed out
    int64_t ids;
};

struct ScArgs {
    ScSide a, b;
    int has_b;
    const uint8_t* lits;           // prefix | sep | suffix
    int64_t pre_len, sep_len, suf_len;
    int64_t n;                     // items
    int64_t id_begin;              // the affix form (list == null): item i is id id_begin + i of `a`, the LAST item is NULL
    const uint32_t* list;          // the pair form: item i is the pair in slot list[i] of `keys`
    const uint64_t* keys;
    int64_t* starts;               // [n] the spans of the images in `scratch`
    int32_t* lens;
    unsigned long long* valid;     // bitmap, bit i: item i has an image
    unsigned long long* ctl;       // [0] scratch bytes reserved  [1] items that are no value of their dictionary, images that left their room (internal errors)
    uint8_t* scratch;
    int64_t scratch_bytes;
    int pass;                      // 0: lengths and reservations  1: the bytes
};

// the operand of item `i` on one side: false = no image (an id never handed out); *len < 0 = NULL
__device__ __forceinline__ bool sc_side(const ScSide& s, int64_t id, const uint8_t** p, int64_t* len, bool* broken) {
    *p = nullptr; *len = -1;
    if (id < 0) return true;
    if (id >= s.ids) { *broken = true; return false; }
    const int64_t l = s.len[id];
    if (l < 0) return false;
    *p = s.heap + s.off[id];
    *len = l;
    return true;
}

__global__ __launch_bounds__(256) void sc_image_kernel(ScArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int tid = threadIdx.x;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < a.n; i0 += stride) {       // (uniform trips: every lane reaches the ballot)
        const int64_t i = i0 + tid;
        bool live = i < a.n, broken = false;
        const uint8_t *pa = nullptr, *pb = nullptr;
        int64_t la = -1, lb = -1;
        if (live) {
            if (a.list) {
                const uint64_t key = a.keys[a.list[i]];
                live = sc_side(a.a, (int64_t)(key >> 32) - 1, &pa, &la, &broken) && sc_side(a.b, (int64_t)(uint32_t)key - 1, &pb, &lb, &broken);
                if (!live) broken = true;               // (a row's code without a value: the caller's codes are not this dictionary's)
            } else if (i + 1 < a.n) {
                live = sc_side(a.a, a.id_begin + i, &pa, &la, &broken);
            }
        }
        if (a.pass == 0) {
            int64_t room = 0, start = 0;
            if (live) {
                room = sc_concat_room(a.pre_len, pa, la, a.sep_len, a.has_b != 0, pb, lb, a.suf_len);
                if (room > 0x7FFFFFFFLL) { live = false; broken = true; }
                else start = (int64_t)atomicAdd(&a.ctl[0], (unsigned long long)room);
            }
            if (i < a.n) { a.starts[i] = live ? start : 0; a.lens[i] = live ? (int32_t)room : 0; }
            const unsigned long long good = __ballot(live);
            if ((tid & 63) == 0 && i < a.n) a.valid[i >> 6] = good;
        } else if (live) {
            const int64_t start = a.starts[i], room = a.lens[i];
            if (start < 0 || start + room > a.scratch_bytes) broken = true;
            else if (sc_concat_write(a.scratch + start, room, a.lits, a.pre_len, pa, la, a.sep_len, a.has_b != 0, pb, lb, a.suf_len) != room) broken = true;
        }
        if (broken) atomicAdd(&a.ctl[1], 1ULL);
    }
}

// the affix table: codes of ids [id_begin, id_begin + n) from the encode's output (-1: no span -> -2, "no code")
__global__ __launch_bounds__(256) void sc_affix_table_kernel(const int32_t* codes, int64_t n, int32_t* table) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) table[i] = codes[i] < 0 ? -2 : codes[i];
}

// the row pass of the one-column form: out[i] = table[code[i]], and `null_code` -- the code of the NULL image -- where the row is
// NULL by its validity bit or by code -1.  No validity comes out: concat() is never NULL.  4 rows per lane, 16-byte accesses.
struct ScGatherArgs {
    const int32_t* codes;          // row 0's code
    const uint8_t* valid;          // bit `vfirst` belongs to row 0 (or null)
    int64_t vfirst, n, ntiles;
    const int32_t* table;          // [n_ids]; a code at or past n_ids is never an address: the row gets -2
    int64_t n_ids;
    int32_t null_code;
    int32_t* out;
    int vec;
};

__global__ __launch_bounds__(256) void sc_gather_kernel(ScGatherArgs a) {
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * SP_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < SP_ROWS ? (int)(a.n - row0) : SP_ROWS;
        int32_t c[SP_ROWS];
        if (a.vec && cnt == SP_ROWS) {
            const int4 q = *(const int4*)(a.codes + row0);
            c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) c[k] = k < cnt ? a.codes[row0 + k] : -1;
        }
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const bool null = c[k] < 0 || (k < cnt && a.valid && !sp_bit(a.valid, a.vfirst + row0 + k));
            c[k] = null ? a.null_code : (c[k] < a.n_ids ? a.table[c[k]] : -2);
        }
        if (a.vec && cnt == SP_ROWS) *(int4*)(a.out + row0) = make_int4(c[0], c[1], c[2], c[3]);
        else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (k < cnt) a.out[row0 + k] = c[k];
        }
    }
}

}  // namespace vnm

struct vnm_strpair {
    SPair t{};
    int64_t fill = 0;                          // slots whose code is in place
    unsigned int* ctl = nullptr;               // device, see SpFindArgs
    uint8_t* lits_dev = nullptr;               // prefix | sep | suffix, uploaded with the first call
    std::string prefix, suffix, lits;
    bool have_sep = false;
    int64_t sep_len = 0;
    int64_t pair_launches = 0, pairs_concatenated = 0, rehashes = 0;
    bool failed = false;
};

static ScSide sc_side_of(const vnm_strdict* d) {
    ScSide s{};
    s.heap = d->heap; s.off = d->id_off; s.len = d->id_len; s.ids = d->ids;
    return s;
}

static int sc_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)device_info().num_cus * 8)); }

// the images of `a`'s n items found or inserted in dst: out_codes[i] (device, n int32s) = dst's code, -1 for an item without an image
static int sc_images_into(vnm_strdict* dst, ScArgs& a, int32_t* out_codes, const char* what, PoolScope& pool, hipStream_t s) {
    const int64_t n = a.n;
    a.starts = (int64_t*)pool.take((size_t)n * 8);
    a.lens = (int32_t*)pool.take((size_t)n * 4);
    a.valid = (unsigned long long*)pool.take((size_t)((n + 63) / 64) * 8);
    a.ctl = (unsigned long long*)pool.take(16);
    if (!a.starts || !a.lens || !a.valid || !a.ctl) return 1;
    VNM_HIP(hipMemsetAsync(a.ctl, 0, 16, s));
    unsigned long long ctl[2] = {0, 0};
    {
        KernelTimer timer(what, s);
        a.pass = 0;
        sc_image_kernel<<<sc_grid(n), 256, 0, s>>>(a);
        VNM_HIP(hipGetLastError());
        VNM_HIP(hipMemcpyAsync(ctl, a.ctl, 16, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (ctl[1]) return set_error("%s: %llu item(s) hold a code that is no value of its dictionary", what, ctl[1]);
        a.scratch_bytes = (int64_t)ctl[0];
        a.scratch = (uint8_t*)pool.take((size_t)std::max<int64_t>(a.scratch_bytes, 8));
        if (!a.scratch) return 1;
        a.pass = 1;
        sc_image_kernel<<<sc_grid(n), 256, 0, s>>>(a);
        VNM_HIP(hipGetLastError());
    }
    vnm_dcol offs{};
    offs.values = (void*)a.starts; offs.type = VNM_I64; offs.offset = 0; offs.length = n + 1;
    const int rc = strdict_encode_device_impl(dst, &offs, a.lens, (const uint8_t*)a.valid, 0, a.scratch, 0, out_codes, nullptr, nullptr, (void*)s);
    if (rc) {
        (void)hipStreamSynchronize(s);
        if (dst->d.slot) dst->failed = true;
        return rc;
    }
    VNM_HIP(hipMemcpyAsync(ctl, a.ctl, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));         // (the scratch goes back to the pool with the caller's scope)
    if (ctl[1]) return set_error("%s: %llu image(s) left their room (internal error)", what, ctl[1]);
    return 0;
}

static int sc_upload_lits(const std::string& lits, uint8_t** dev) {
    uint8_t* p = (uint8_t*)pool_alloc(std::max<size_t>(lits.size(), 8));
    if (!p) return 1;
    if (!lits.empty() && hipMemcpy(p, lits.data(), lits.size(), hipMemcpyHostToDevice) != hipSuccess) {
        pool_free(p);
        return set_error("concat: literal upload failed");
    }
    *dev = p;
    return 0;
}

extern "C" {

int vnm_strdict_concat_affix(vnm_strdict* src, vnm_strdict* dst, const uint8_t* prefix, int64_t prefix_len, const uint8_t* suffix, int64_t suffix_len,
                             int64_t id_begin, int32_t* out_dst_code_of_src_id, int32_t* out_null_code, void* stream) {
    VNM_TRY(ensure_init());
    if (out_null_code) *out_null_code = -2;
    if (!src || !dst || prefix_len < 0 || suffix_len < 0 || (prefix_len > 0 && !prefix) || (suffix_len > 0 && !suffix))
        return set_error("vnm_strdict_concat_affix: null argument");
    if (src == dst) return set_error("vnm_strdict_concat_affix: src and dst are one dictionary (src is only read, dst grows)");
    if (src->failed || dst->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (id_begin < 0) return set_error("vnm_strdict_concat_affix: id_begin < 0");
    const int64_t n_ids = std::max<int64_t>(src->ids - id_begin, 0);
    if (n_ids > 0 && !out_dst_code_of_src_id) return set_error("vnm_strdict_concat_affix: null table");
    std::string lits((const char*)prefix, (size_t)prefix_len);
    lits.append((const char*)suffix, (size_t)suffix_len);
    if (!dst->affix_dev) {
        VNM_TRY(sc_upload_lits(lits, &dst->affix_dev));
        dst->affix_host = lits;
        dst->affix_pre = prefix_len;
    } else if (dst->affix_host != lits || dst->affix_pre != prefix_len) {
        return set_error("vnm_strdict_concat_affix: dst was derived with another prefix / suffix");
    }
    dst->new_ids.clear(); dst->new_lens.clear(); dst->new_bytes.clear();
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    ScArgs a{};
    a.a = sc_side_of(src);
    a.lits = dst->affix_dev; a.pre_len = prefix_len; a.suf_len = suffix_len;
    a.n = n_ids + 1;                                      // (+ the image of NULL)
    a.id_begin = id_begin;
    int32_t* codes = (int32_t*)pool.take((size_t)a.n * 4);
    if (!codes) return 1;
    VNM_TRY(sc_images_into(dst, a, codes, "strdict_concat_affix", pool, s));
    if (n_ids) {
        sc_affix_table_kernel<<<sc_grid(n_ids), 256, 0, s>>>(codes, n_ids, out_dst_code_of_src_id + id_begin);
        VNM_HIP(hipGetLastError());
    }
    int32_t null_code = -2;
    VNM_HIP(hipMemcpyAsync(&null_code, codes + n_ids, 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (null_code < 0) return set_error("vnm_strdict_concat_affix: the image of NULL got no code (internal error)");
    if (out_null_code) *out_null_code = null_code;
    return 0;
}

int vnm_strdict_gather_codes(const int32_t* codes, const uint8_t* validity, int64_t validity_offset, const int32_t* table, int64_t n_ids, int64_t n,
                             int32_t null_code, int32_t* out_codes, void* stream) {
    VNM_TRY(ensure_init());
    if (n <= 0) return 0;
    if (!codes || !out_codes || n_ids < 0 || (n_ids > 0 && !table) || validity_offset < 0) return set_error("vnm_strdict_gather_codes: null argument");
    ScGatherArgs a{};
    a.codes = codes; a.valid = validity; a.vfirst = validity_offset; a.n = n;
    a.ntiles = (n + SP_TILE - 1) / SP_TILE;
    a.table = table; a.n_ids = n_ids; a.null_code = null_code; a.out = out_codes;
    a.vec = ((((uintptr_t)codes) | ((uintptr_t)out_codes)) & 15) == 0;
    hipStream_t s = as_stream(stream);
    {
        KernelTimer timer("strdict_gather_codes", s);
        sc_gather_kernel<<<(int)std::min<int64_t>(a.ntiles, (int64_t)device_info().num_cus * 16), 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

vnm_strpair* vnm_strpair_create(const uint8_t* prefix, int64_t prefix_len, const uint8_t* suffix, int64_t suffix_len) {
    if (ensure_init()) return nullptr;
    if (prefix_len < 0 || suffix_len < 0 || (prefix_len > 0 && !prefix) || (suffix_len > 0 && !suffix)) { set_error("vnm_strpair_create: null argument"); return nullptr; }
    vnm_strpair* h = new vnm_strpair();
    h->prefix.assign((const char*)prefix, (size_t)prefix_len);
    h->suffix.assign((const char*)suffix, (size_t)suffix_len);
    return h;
}

void vnm_strpair_destroy(vnm_strpair* h) {
    if (!h) return;
    pool_free(h->t.keys);
    pool_free(h->t.codes);
    pool_free(h->ctl);
    pool_free(h->lits_dev);
    delete h;
}

static int strpair_alloc(SPair* t, uint64_t cap, hipStream_t s) {
    t->cap = cap;
    t->keys = (uint64_t*)pool_alloc((size_t)cap * 8);
    t->codes = (int32_t*)pool_alloc((size_t)cap * 4);
    if (!t->keys || !t->codes || hipMemsetAsync(t->keys, 0xFF, (size_t)cap * 8, s) != hipSuccess || hipMemsetAsync(t->codes, 0xFF, (size_t)cap * 4, s) != hipSuccess) {
        pool_free(t->keys); pool_free(t->codes);
        t->keys = nullptr; t->codes = nullptr; t->cap = 0;
        return set_error("vnm_strpair: table allocation failed");
    }
    return 0;
}

static uint64_t strpair_initial_slots() {
    uint64_t want = 1 << 16;
    if (const char* e = getenv("VNM_STRPAIR_SLOTS")) {
        const long long v = atoll(e);
        if (v > 0) want = (uint64_t)std::min<long long>(v, 1LL << 30);
    }
    uint64_t cap = 16;
    while (cap < want) cap <<= 1;
    return cap;
}

int vnm_strpair_concat(vnm_strpair* h, vnm_strdict* a, vnm_strdict* b, vnm_strdict* dst, const uint8_t* sep, int64_t sep_len, const vnm_dcol* codes_a,
                       const vnm_dcol* codes_b, int64_t length, int32_t* out_codes, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !a || !b || !dst || !codes_a || !codes_b || sep_len < 0 || (sep_len > 0 && !sep)) return set_error("vnm_strpair_concat: null argument");
    if (h->failed) return set_error("vnm_strpair: an earlier call failed half-way; the table cannot be used any more (create a new one)");
    if (dst == a || dst == b) return set_error("vnm_strpair_concat: dst is one of the operands' dictionaries (they are only read, dst grows)");
    if (a->failed || b->failed || dst->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (codes_a->type != VNM_I32 || codes_b->type != VNM_I32) return set_error("vnm_strpair_concat: the code columns must be int32");
    if (length < 0 || codes_a->length != length || codes_b->length != length || codes_a->offset < 0 || codes_b->offset < 0)
        return set_error("vnm_strpair_concat: the code columns' lengths and `length` differ, or a negative offset");
    if (!h->have_sep) {
        h->lits = h->prefix;
        h->lits.append((const char*)sep, (size_t)sep_len);
        h->lits += h->suffix;
        VNM_TRY(sc_upload_lits(h->lits, &h->lits_dev));
        h->sep_len = sep_len;
        h->have_sep = true;
    } else if (h->sep_len != sep_len || (sep_len && memcmp(h->lits.data() + h->prefix.size(), sep, (size_t)sep_len))) {
        return set_error("vnm_strpair_concat: the table was built with another separator");
    }
    if (length == 0) return 0;
    if (!codes_a->values || !codes_b->values || !out_codes) return set_error("vnm_strpair_concat: null argument");
    hipStream_t s = as_stream(stream);
    if (!h->t.keys) {
        VNM_TRY(strpair_alloc(&h->t, strpair_initial_slots(), s));
        h->ctl = (unsigned int*)pool_alloc(64);
        if (!h->ctl) return 1;
    }
    h->pair_launches++;
    PoolScope pool;
    SpFindArgs f{};
    f.ca = (const int32_t*)codes_a->values + codes_a->offset; f.va = codes_a->validity; f.oa = codes_a->offset;
    f.cb = (const int32_t*)codes_b->values + codes_b->offset; f.vb = codes_b->validity; f.ob = codes_b->offset;
    f.n = length;
    f.ntiles = (length + SP_TILE - 1) / SP_TILE;
    f.ids_a = a->ids; f.ids_b = b->ids;
    f.out = out_codes;
    f.list_cap = length;                                   // (a batch brings at most one new pair per row)
    f.list = (uint32_t*)pool.take((size_t)length * 4);
    if (!f.list) return 1;
    f.ctl = h->ctl;
    f.vec = ((((uintptr_t)f.ca) | ((uintptr_t)f.cb) | ((uintptr_t)out_codes)) & 15) == 0;
    const int grid = (int)std::min<int64_t>(f.ntiles, (int64_t)device_info().num_cus * 16);
    VNM_HIP(hipMemsetAsync(h->ctl, 0, 16, s));
    unsigned int ctl[4] = {0, 0, 0, 0};
    for (;;) {
        f.t = h->t;
        f.fill_before = h->fill;
        f.fill_limit = (int64_t)(h->t.cap * 7 / 10);
        {
            KernelTimer timer("strpair_find", s);
            sp_find_kernel<<<grid, 256, 0, s>>>(f);
        }
        VNM_HIP(hipGetLastError());
        VNM_HIP(hipMemcpyAsync(ctl, h->ctl, 16, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (ctl[2]) { h->failed = ctl[1] != 0; return set_error("vnm_strpair_concat: %u row(s) hold a code outside their dictionary", ctl[2]); }
        if (ctl[0] & 2u) { h->failed = true; return set_error("vnm_strpair_concat: more new pairs than rows (internal error)"); }
        if (!ctl[0]) break;
        // ---- overflow: a table four times the size, every key and code re-inserted, the batch's find pass again
        SPair grown{};
        h->failed = true;                                  // (until the pairs claimed so far have their codes)
        VNM_TRY(strpair_alloc(&grown, h->t.cap * 4, s));
        VNM_HIP(hipMemsetAsync(h->ctl, 0, 16, s));
        {
            KernelTimer timer("strpair_rehash", s);
            sp_rehash_kernel<<<sc_grid((int64_t)h->t.cap), 256, 0, s>>>(h->t, grown, f.list, f.list_cap, h->ctl);
        }
        VNM_HIP(hipGetLastError());
        VNM_HIP(hipStreamSynchronize(s));
        pool_free(h->t.keys); pool_free(h->t.codes);
        h->t = grown;
        h->rehashes++;
    }
    const int64_t fresh = (int64_t)ctl[1];
    if (fresh) {
        // ---- concat: the new pairs' images into dst, their codes into the slots
        h->failed = true;
        ScArgs c{};
        c.a = sc_side_of(a); c.b = sc_side_of(b); c.has_b = 1;
        c.lits = h->lits_dev; c.pre_len = (int64_t)h->prefix.size(); c.sep_len = h->sep_len; c.suf_len = (int64_t)h->suffix.size();
        c.n = fresh;
        c.list = f.list; c.keys = h->t.keys;
        int32_t* codes = (int32_t*)pool.take((size_t)fresh * 4);
        if (!codes) return 1;
        dst->new_ids.clear(); dst->new_lens.clear(); dst->new_bytes.clear();
        VNM_TRY(sc_images_into(dst, c, codes, "strpair_concat", pool, s));
        sp_store_codes_kernel<<<sc_grid(fresh), 256, 0, s>>>(h->t, f.list, codes, fresh);
        VNM_HIP(hipGetLastError());
        h->fill += fresh;
        h->pairs_concatenated += fresh;
    } else {
        dst->new_ids.clear(); dst->new_lens.clear(); dst->new_bytes.clear();
    }
    h->failed = false;
    {
        KernelTimer timer("strpair_gather", s);
        sp_gather_kernel<<<grid, 256, 0, s>>>(h->t.codes, out_codes, length, f.ntiles, ((uintptr_t)out_codes & 15) == 0);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));                      // (the new-pairs list goes back to the pool with this scope)
    return 0;
}

int vnm_strpair_stats(vnm_strpair* h, int64_t* out6, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !out6) return set_error("vnm_strpair_stats: null argument");
    out6[0] = h->pair_launches; out6[1] = h->pairs_concatenated; out6[2] = h->rehashes; out6[3] = (int64_t)h->t.cap; out6[4] = 0; out6[5] = 0;
    if (!h->t.keys) return 0;
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    unsigned long long* counts = (unsigned long long*)pool.take(16);
    if (!counts) return 1;
    VNM_HIP(hipMemsetAsync(counts, 0, 16, s));
    sp_check_kernel<<<sc_grid((int64_t)h->t.cap), 256, 0, s>>>(h->t, counts);
    VNM_HIP(hipGetLastError());
    unsigned long long c[2] = {0, 0};
    VNM_HIP(hipMemcpyAsync(c, counts, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    out6[4] = (int64_t)c[0]; out6[5] = (int64_t)c[1];
    return 0;
}

}  // extern "C"
