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
//
// to_str(v) over an integer, date32 or timestamp column (StringCastFunction, functions.py:189-193) is the SAME table keyed by the row's
// VALUE: vnm_strval.  The find pass is generic over how a row's key is formed (SpPairRows: two codes; SpValueRows: a value loaded at
// width 1 / 2 / 4 / 8 and widened); rehash, store-codes, gather, check, the growth policy and the host passes (sp_find_all, sp_finish,
// sp_stats) are one code for both.  What a value key adds: it can BE the empty marker (-1, UINT64_MAX), and a row can be NULL -- those
// two live in side slots `cap` and `cap + 1` outside the probed range, claimed by one CAS on a flag word and listed like any new slot,
// so the gather needs no special case.  The image of a new slot is formatted from the slot's key (vnm_tostr.hpp), once per distinct value.
#include "vnm_strconcat.hpp"
#include "vnm_tostr.hpp"

namespace vnm {

constexpr uint64_t SP_EMPTY = ~0ULL;
constexpr int SP_ROWS = 4;                 // rows per lane: one 16-byte load per code column, one 16-byte store
constexpr int SP_TILE = 256 * SP_ROWS;     // rows per workgroup and step
constexpr uint64_t SP_WALK = 1024;         // the longest probe walk (and never longer than the capacity): at 70 % fill a walk of linear probing
                                           // stays far below it; a longer one means the table is crowded, which is an overflow

struct SPair {
    uint64_t* keys;                // [cap] the row's key (SpPairRows / SpValueRows); SP_EMPTY
    int32_t* codes;                // [cap + 2] the key's code in dst; -1 until its image is inserted.  [cap], [cap + 1]: the side slots
    uint64_t cap;
    unsigned int* side;            // [2] 1: side slot cap + j is claimed (null: a table whose keys never need one).  Outside the probed
                                   // range: a key that IS the empty marker, and NULL; the flags outlive a rehash, the codes move with it
};

__device__ __forceinline__ uint64_t sp_home(uint64_t key, uint64_t mask) {
    uint64_t h = key * 0x9E3779B97F4A7C15ULL;
    h ^= h >> 32;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 29;
    return h & mask;
}

__device__ __forceinline__ bool sp_bit(const uint8_t* bits, int64_t i) { return (bits[i >> 3] >> (i & 7)) & 1; }

// How a row's key is formed -- the one thing the find pass does not know.  A row source loads a lane's SP_ROWS rows (`vec`: in one
// access per column, the caller has checked the alignment) and says what row k is: SP_KEY with its key, SP_BAD (counted, the row
// gets -1), or SP_SIDE0 / SP_SIDE1 (the row lives in side slot cap / cap + 1).
enum { SP_KEY = 0, SP_BAD, SP_SIDE0, SP_SIDE1 };

// concat(a, sep, b): (code_a + 1) << 32 | (code_b + 1), NULL is code -1 or a cleared validity bit.  Never SP_EMPTY: no side slots
struct SpPairRows {
    const int32_t* ca;             // row 0's code (the Arrow offset is applied); validity bit oa + row
    const uint8_t* va;
    int64_t oa;
    const int32_t* cb;
    const uint8_t* vb;
    int64_t ob;
    int64_t ids_a, ids_b;          // codes lie in [-1, ids)
    struct Regs { int32_t xa[SP_ROWS], xb[SP_ROWS]; };
    __device__ __forceinline__ void load(Regs& r, int64_t row0, int cnt, bool vec) const {
        if (vec) {
            const int4 qa = *(const int4*)(ca + row0), qb = *(const int4*)(cb + row0);
            r.xa[0] = qa.x; r.xa[1] = qa.y; r.xa[2] = qa.z; r.xa[3] = qa.w;
            r.xb[0] = qb.x; r.xb[1] = qb.y; r.xb[2] = qb.z; r.xb[3] = qb.w;
        } else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) { r.xa[k] = k < cnt ? ca[row0 + k] : -1; r.xb[k] = k < cnt ? cb[row0 + k] : -1; }
        }
    }
    __device__ __forceinline__ int key(const Regs& r, int k, int64_t row, uint64_t* key) const {
        int64_t ia = r.xa[k], ib = r.xb[k];
        if (va && !sp_bit(va, oa + row)) ia = -1;
        if (vb && !sp_bit(vb, ob + row)) ib = -1;
        if (ia < -1 || ia >= ids_a || ib < -1 || ib >= ids_b) return SP_BAD;
        *key = ((uint64_t)(uint32_t)(ia + 1) << 32) | (uint64_t)(uint32_t)(ib + 1);
        return SP_KEY;
    }
};

// to_str(v): the key is the VALUE widened to 64 bits (by sign, or by zero extension), so the slot's key gives the value back
// exactly.  The all-ones pattern (-1, UINT64_MAX) is the empty marker: side slot 0; a NULL row: side slot 1
struct SpValueRows {
    const uint8_t* p;              // row 0's value (the Arrow offset is applied); validity bit off + row
    const uint8_t* valid;
    int64_t off;
    int width;                     // 1, 2, 4, 8 bytes
    int is_signed;
    struct Regs { uint64_t x[SP_ROWS]; };
    __device__ __forceinline__ uint64_t widen(uint64_t raw) const {
        const int sh = 64 - 8 * width;
        return is_signed ? (uint64_t)(((int64_t)(raw << sh)) >> sh) : raw;
    }
    __device__ __forceinline__ void load(Regs& r, int64_t row0, int cnt, bool vec) const {
        if (vec) {                 // SP_ROWS rows in one 4 / 8 / 16 / 32-byte access
            if (width == 1) {
                const uint32_t q = *(const uint32_t*)(p + row0);
                r.x[0] = q & 0xFF; r.x[1] = (q >> 8) & 0xFF; r.x[2] = (q >> 16) & 0xFF; r.x[3] = q >> 24;
            } else if (width == 2) {
                const uint2 q = *(const uint2*)(p + row0 * 2);
                r.x[0] = q.x & 0xFFFF; r.x[1] = q.x >> 16; r.x[2] = q.y & 0xFFFF; r.x[3] = q.y >> 16;
            } else if (width == 4) {
                const uint4 q = *(const uint4*)(p + row0 * 4);
                r.x[0] = q.x; r.x[1] = q.y; r.x[2] = q.z; r.x[3] = q.w;
            } else {
                const ulonglong2 q0 = *(const ulonglong2*)(p + row0 * 8), q1 = *(const ulonglong2*)(p + row0 * 8 + 16);
                r.x[0] = q0.x; r.x[1] = q0.y; r.x[2] = q1.x; r.x[3] = q1.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) {
                uint64_t v = 0;
                if (k < cnt) {
                    const uint8_t* q = p + (row0 + k) * width;
                    v = width == 1 ? *q : width == 2 ? *(const uint16_t*)q : width == 4 ? *(const uint32_t*)q : *(const uint64_t*)q;
                }
                r.x[k] = v;
            }
        }
    }
    __device__ __forceinline__ int key(const Regs& r, int k, int64_t row, uint64_t* key) const {
        if (valid && !sp_bit(valid, off + row)) return SP_SIDE1;
        *key = widen(r.x[k]);
        return *key == SP_EMPTY ? SP_SIDE0 : SP_KEY;
    }
};

template <class Rows>
struct SpFindArgs {
    SPair t;
    Rows rows;
    int64_t n, ntiles;
    int64_t fill_before, fill_limit;
    int32_t* out;                  // the row's slot; -1: not placed (overflow) or a bad row
    uint32_t* list;                // slots claimed in this call
    int64_t list_cap;
    unsigned int* ctl;             // [0] 1: overflow, 2: the list is full (internal error)  [1] slots listed  [2] bad rows (a code outside its dictionary)
                                   // [3] slots of the probed range claimed (counted at the CAS itself: what the fill limit is held against)
    int vec;                       // the rows' columns and out are aligned for one access per lane
};

template <class Rows>
__global__ __launch_bounds__(256) void sp_find_kernel(SpFindArgs<Rows> a) {
    const uint64_t mask = a.t.cap - 1, walk = a.t.cap < SP_WALK ? a.t.cap : SP_WALK;
    const int lane = threadIdx.x & 63;
    unsigned flag = 0, nbad = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {      // (trips uniform in a wave: every lane reaches the ballots)
        // once any lane has raised the overflow flag the host runs the whole pass again over a bigger table: nothing more to do here
        if (__any(__hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
        const int64_t row0 = (tile * 256 + threadIdx.x) * SP_ROWS;
        const int cnt = row0 >= a.n ? 0 : (a.n - row0 < SP_ROWS ? (int)(a.n - row0) : SP_ROWS);
        typename Rows::Regs regs;
        int32_t o[SP_ROWS];
        a.rows.load(regs, row0, cnt, a.vec && cnt == SP_ROWS);
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const bool live = k < cnt;
            uint64_t key = 0;
            const int what = live ? a.rows.key(regs, k, row0 + k, &key) : SP_BAD;
            if (live && what == SP_BAD) nbad++;
            int32_t slot = -1;
            bool won = false;
            if (live && what == SP_KEY) {
                uint64_t h = sp_home(key, mask);
                for (uint64_t probes = 0; probes < walk; probes++) {
                    if ((probes & 15) == 15 && __hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                    uint64_t cur = sd_ld(a.t.keys + h);
                    if (cur == SP_EMPTY) {
                        const unsigned claimed = __hip_atomic_load(&a.ctl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (a.fill_before + (int64_t)claimed >= a.fill_limit) break;
                        if (__hip_atomic_compare_exchange_strong(a.t.keys + h, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            won = true;                    // the slot is this key's, and this lane lists it
                            slot = (int32_t)h;
                            atomicAdd(&a.ctl[3], 1u);      // (no return value: the compiler folds a wave's adds into one)
                            break;
                        }                                  // (cur now holds what the slot had: this key, or another)
                    }
                    if (cur == key) { slot = (int32_t)h; break; }
                    h = (h + 1) & mask;
                }
                if (slot < 0 && !(flag & 1u)) {            // said at once, so that every other lane stops walking a crowded table
                    flag |= 1u;
                    atomicOr(&a.ctl[0], 1u);
                }
            } else if (live && what != SP_BAD && a.t.side) {
                // a side slot: one flag word outside the probed range, claimed by one CAS; its winner is listed like any other
                unsigned int* f = a.t.side + (what - SP_SIDE0);
                slot = (int32_t)(a.t.cap + (uint64_t)(what - SP_SIDE0));
                if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) won = atomicCAS(f, 0u, 1u) == 0u;
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
    // the side slots: the flags stay where they are, the codes move to the new table's end; a claimed one without a code is listed again
    if (from.side && blockIdx.x == 0 && threadIdx.x < 2 && from.side[threadIdx.x]) {
        const int32_t code = from.codes[from.cap + threadIdx.x];
        to.codes[to.cap + threadIdx.x] = code;
        if (code < 0) {
            const int64_t at = (int64_t)atomicAdd(&ctl[1], 1u);
            if (at < list_cap) list[at] = (uint32_t)(to.cap + threadIdx.x);
            else atomicOr(&ctl[0], 2u);
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
    if (t.side && blockIdx.x == 0 && threadIdx.x < 2 && t.side[threadIdx.x]) { occ++; if (t.codes[t.cap + threadIdx.x] < 0) half++; }
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
    int value_form, ts_kind;       // the value form (to_str, one of vnm_tostr.hpp's kinds): item i is the VALUE that is the key of slot
    uint64_t cap;                  // list[i] of `keys`; slot cap is the value SP_EMPTY itself, slot cap + 1 is NULL
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
        int64_t la = -1, lb = -1, value = 0;
        int kind = a.ts_kind;
        if (live) {
            if (a.value_form) {
                const uint64_t slot = a.list[i];
                if (slot > a.cap + 1) { live = false; broken = true; }
                else if (slot == a.cap + 1) kind = TS_NONE;
                else value = (int64_t)(slot == a.cap ? SP_EMPTY : a.keys[slot]);
            } else if (a.list) {
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
                room = a.value_form ? ts_room(kind, value) : sc_concat_room(a.pre_len, pa, la, a.sep_len, a.has_b != 0, pb, lb, a.suf_len);
                if (room > 0x7FFFFFFFLL || (a.value_form && (room <= 0 || room > TS_MAX_BYTES))) { live = false; broken = true; }
                else start = (int64_t)atomicAdd(&a.ctl[0], (unsigned long long)room);
            }
            if (i < a.n) { a.starts[i] = live ? start : 0; a.lens[i] = live ? (int32_t)room : 0; }
            const unsigned long long good = __ballot(live);
            if ((tid & 63) == 0 && i < a.n) a.valid[i >> 6] = good;
        } else if (live) {
            const int64_t start = a.starts[i], room = a.lens[i];
            if (start < 0 || start + room > a.scratch_bytes) broken = true;
            else if ((a.value_form ? ts_write(a.scratch + start, room, kind, value)
                                   : sc_concat_write(a.scratch + start, room, a.lits, a.pre_len, pa, la, a.sep_len, a.has_b != 0, pb, lb, a.suf_len)) != room) broken = true;
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

// the table both handles keep across calls, and what the shared passes (sp_find_all, sp_finish, sp_stats) work on
struct SpTable {
    SPair t{};
    int64_t fill = 0;                          // slots of the probed range whose code is in place
    unsigned int* ctl = nullptr;               // device, see SpFindArgs
    int64_t launches = 0, images = 0, rehashes = 0;    // calls with length > 0, keys whose image was written (= distinct keys seen)
    bool failed = false;
};

struct vnm_strpair : SpTable {
    uint8_t* lits_dev = nullptr;               // prefix | sep | suffix, uploaded with the first call
    std::string prefix, suffix, lits;
    bool have_sep = false;
    int64_t sep_len = 0;
};

struct vnm_strval : SpTable {
    int kind = 0;                              // enum vnm_tostr_kind
    int type = -1;                             // the vnm_type of the first call's column: the keys are its values
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

// ---- the passes vnm_strpair and vnm_strval share: allocate / find (+ grow) / images + codes + gather / stats ---------------------------
static int sp_alloc(SPair* t, uint64_t cap, unsigned int* side, hipStream_t s) {
    t->cap = cap;
    t->side = side;
    t->keys = (uint64_t*)pool_alloc((size_t)cap * 8);
    t->codes = (int32_t*)pool_alloc((size_t)(cap + 2) * 4);
    if (!t->keys || !t->codes || hipMemsetAsync(t->keys, 0xFF, (size_t)cap * 8, s) != hipSuccess || hipMemsetAsync(t->codes, 0xFF, (size_t)(cap + 2) * 4, s) != hipSuccess) {
        pool_free(t->keys); pool_free(t->codes);
        t->keys = nullptr; t->codes = nullptr; t->cap = 0;
        return set_error("vnm_strpair: table allocation failed");
    }
    return 0;
}

static uint64_t sp_initial_slots() {
    uint64_t want = 1 << 16;
    if (const char* e = getenv("VNM_STRPAIR_SLOTS")) {
        const long long v = atoll(e);
        if (v > 0) want = (uint64_t)std::min<long long>(v, 1LL << 30);
    }
    uint64_t cap = 16;
    while (cap < want) cap <<= 1;
    return cap;
}

// the table of the first call with rows: ctl is [0..3] the find pass's words, [4..5] the side slots' flags
static int sp_table_ready(SpTable* h, bool with_side, hipStream_t s) {
    if (!h->t.keys) {
        if (!h->ctl) {
            h->ctl = (unsigned int*)pool_alloc(64);
            if (!h->ctl) return 1;
            VNM_HIP(hipMemsetAsync(h->ctl, 0, 64, s));
        }
        VNM_TRY(sp_alloc(&h->t, sp_initial_slots(), with_side ? h->ctl + 4 : nullptr, s));
    }
    h->launches++;
    return 0;
}

static void sp_table_free(SpTable* h) {
    pool_free(h->t.keys);
    pool_free(h->t.codes);
    pool_free(h->ctl);
}

// the find pass over f's rows, the table grown x4 and the pass run again as often as it overflows: afterwards f.out holds every row's
// slot, f.list the `*fresh` slots that still need an image and a code
template <class Rows>
static int sp_find_all(SpTable* h, SpFindArgs<Rows>& f, const char* what, int64_t* fresh, PoolScope& pool, hipStream_t s) {
    f.ntiles = (f.n + SP_TILE - 1) / SP_TILE;
    f.list_cap = f.n;                                      // (a batch brings at most one new key per row)
    f.list = (uint32_t*)pool.take((size_t)f.n * 4);
    if (!f.list) return 1;
    f.ctl = h->ctl;
    const int grid = (int)std::min<int64_t>(f.ntiles, (int64_t)device_info().num_cus * 16);
    VNM_HIP(hipMemsetAsync(h->ctl, 0, 16, s));
    unsigned int ctl[4] = {0, 0, 0, 0};
    for (;;) {
        f.t = h->t;
        f.fill_before = h->fill;
        f.fill_limit = (int64_t)(h->t.cap * 7 / 10);
        {
            KernelTimer timer("strpair_find", s);
            sp_find_kernel<Rows><<<grid, 256, 0, s>>>(f);
        }
        VNM_HIP(hipGetLastError());
        VNM_HIP(hipMemcpyAsync(ctl, h->ctl, 16, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (ctl[2]) { h->failed = ctl[1] != 0; return set_error("%s: %u row(s) hold a code outside their dictionary", what, ctl[2]); }
        if (ctl[0] & 2u) { h->failed = true; return set_error("%s: more new keys than rows (internal error)", what); }
        if (!ctl[0]) break;
        // ---- overflow: a table four times the size, every key and code re-inserted, the batch's find pass again
        SPair grown{};
        h->failed = true;                                  // (until the keys claimed so far have their codes)
        VNM_TRY(sp_alloc(&grown, h->t.cap * 4, h->t.side, s));
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
    *fresh = (int64_t)ctl[1];
    h->fill += (int64_t)ctl[3];                            // (the side slots are listed, not counted: they lie outside the probed range)
    if (*fresh) h->failed = true;                          // (until sp_finish has given the new slots their codes)
    return 0;
}

// the images of the `fresh` listed slots through dst's encode (`c` says which form: sc_image_kernel), their codes into the slots, and
// out[i] = code_of_slot[out[i]] over the rows
static int sp_finish(SpTable* h, vnm_strdict* dst, ScArgs& c, const uint32_t* list, int64_t fresh, int32_t* out, int64_t length, const char* what,
                     PoolScope& pool, hipStream_t s) {
    dst->new_ids.clear(); dst->new_lens.clear(); dst->new_bytes.clear();
    if (fresh) {
        c.n = fresh;
        c.list = list; c.keys = h->t.keys;
        int32_t* codes = (int32_t*)pool.take((size_t)fresh * 4);
        if (!codes) return 1;
        VNM_TRY(sc_images_into(dst, c, codes, what, pool, s));
        sp_store_codes_kernel<<<sc_grid(fresh), 256, 0, s>>>(h->t, list, codes, fresh);
        VNM_HIP(hipGetLastError());
        h->images += fresh;
    }
    h->failed = false;
    const int64_t ntiles = (length + SP_TILE - 1) / SP_TILE;
    {
        KernelTimer timer("strpair_gather", s);
        sp_gather_kernel<<<(int)std::min<int64_t>(ntiles, (int64_t)device_info().num_cus * 16), 256, 0, s>>>(h->t.codes, out, length, ntiles, ((uintptr_t)out & 15) == 0);
    }
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));                      // (the new-keys list goes back to the pool with the caller's scope)
    return 0;
}

static int sp_stats(SpTable* h, int64_t* out6, hipStream_t s) {
    out6[0] = h->launches; out6[1] = h->images; out6[2] = h->rehashes; out6[3] = (int64_t)h->t.cap; out6[4] = 0; out6[5] = 0;
    if (!h->t.keys) return 0;
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
    sp_table_free(h);
    pool_free(h->lits_dev);
    delete h;
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
    VNM_TRY(sp_table_ready(h, false, s));
    PoolScope pool;
    SpFindArgs<SpPairRows> f{};
    f.rows.ca = (const int32_t*)codes_a->values + codes_a->offset; f.rows.va = codes_a->validity; f.rows.oa = codes_a->offset;
    f.rows.cb = (const int32_t*)codes_b->values + codes_b->offset; f.rows.vb = codes_b->validity; f.rows.ob = codes_b->offset;
    f.rows.ids_a = a->ids; f.rows.ids_b = b->ids;
    f.n = length;
    f.out = out_codes;
    f.vec = ((((uintptr_t)f.rows.ca) | ((uintptr_t)f.rows.cb) | ((uintptr_t)out_codes)) & 15) == 0;
    int64_t fresh = 0;
    VNM_TRY(sp_find_all(h, f, "vnm_strpair_concat", &fresh, pool, s));
    // ---- concat: the new pairs' images into dst, their codes into the new slots; then the rows' slots become codes
    ScArgs c{};
    c.a = sc_side_of(a); c.b = sc_side_of(b); c.has_b = 1;
    c.lits = h->lits_dev; c.pre_len = (int64_t)h->prefix.size(); c.sep_len = h->sep_len; c.suf_len = (int64_t)h->suffix.size();
    return sp_finish(h, dst, c, f.list, fresh, out_codes, length, "strpair_concat", pool, s);
}

int vnm_strpair_stats(vnm_strpair* h, int64_t* out6, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !out6) return set_error("vnm_strpair_stats: null argument");
    return sp_stats(h, out6, as_stream(stream));
}

vnm_strval* vnm_strval_create(int kind) {
    if (ensure_init()) return nullptr;
    if (kind < VNM_TOSTR_INT || kind > VNM_TOSTR_TIMESTAMP_NS) { set_error("vnm_strval_create: kind %d is no vnm_tostr_kind", kind); return nullptr; }
    vnm_strval* h = new vnm_strval();
    h->kind = kind;
    return h;
}

void vnm_strval_destroy(vnm_strval* h) {
    if (!h) return;
    sp_table_free(h);
    delete h;
}

int vnm_strval_to_str(vnm_strval* h, vnm_strdict* dst, const vnm_dcol* values, int64_t length, int32_t* out_codes, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !dst || !values) return set_error("vnm_strval_to_str: null argument");
    if (h->failed) return set_error("vnm_strval: an earlier call failed half-way; the table cannot be used any more (create a new one)");
    if (dst->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    const int t = values->type;
    const bool is_signed = t >= VNM_I8 && t <= VNM_I64, is_unsigned = t >= VNM_U8 && t <= VNM_U64;
    const bool fits = h->kind == VNM_TOSTR_INT ? is_signed : h->kind == VNM_TOSTR_UINT ? is_unsigned : h->kind == VNM_TOSTR_DATE32 ? t == VNM_I32 : t == VNM_I64;
    if (!fits) return set_error("vnm_strval_to_str: a column of vnm_type %d does not fit kind %d (signed integers, unsigned integers, date32 = int32, timestamps = int64)", t, h->kind);
    if (h->type >= 0 && h->type != t) return set_error("vnm_strval_to_str: the table was built over vnm_type %d, this column is %d", h->type, t);
    if (length < 0 || values->length != length || values->offset < 0) return set_error("vnm_strval_to_str: the column's length and `length` differ, or a negative offset");
    h->type = t;
    if (length == 0) return 0;
    if (!values->values || !out_codes) return set_error("vnm_strval_to_str: null argument");
    hipStream_t s = as_stream(stream);
    VNM_TRY(sp_table_ready(h, true, s));
    PoolScope pool;
    SpFindArgs<SpValueRows> f{};
    f.rows.width = type_width(t);
    f.rows.is_signed = is_signed ? 1 : 0;
    f.rows.p = (const uint8_t*)values->values + values->offset * f.rows.width; f.rows.valid = values->validity; f.rows.off = values->offset;
    f.n = length;
    f.out = out_codes;
    f.vec = (((uintptr_t)f.rows.p) & (uintptr_t)(SP_ROWS * f.rows.width - 1)) == 0 && (((uintptr_t)out_codes) & 15) == 0;
    int64_t fresh = 0;
    VNM_TRY(sp_find_all(h, f, "vnm_strval_to_str", &fresh, pool, s));
    route_note("to_str:value_table", "%lld rows of vnm_type %d, kind %d: %lld new value(s) to format, %lld slots, %s loads", (long long)length, t, h->kind, (long long)fresh,
               (long long)h->t.cap, f.vec ? "vector" : "scalar");
    // ---- format: the new values' images into dst, their codes into the new slots; then the rows' slots become codes
    ScArgs c{};
    c.value_form = 1; c.ts_kind = h->kind; c.cap = h->t.cap;
    return sp_finish(h, dst, c, f.list, fresh, out_codes, length, "strval_to_str", pool, s);
}

int vnm_strval_stats(vnm_strval* h, int64_t* out6, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !out6) return set_error("vnm_strval_stats: null argument");
    return sp_stats(h, out6, as_stream(stream));
}

}  // extern "C"
