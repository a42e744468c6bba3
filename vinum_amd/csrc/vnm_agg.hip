// Hash group-by aggregate for gfx950.
//
// Replaces BaseAggregate::Next's scalar row loop (vinum_cpp/src/operators/aggregate/base_aggregate.cpp:
// 23-45), the robin_hood maps of Single/MultiNumericalHashAggregate (single_numerical_hash_aggregate.cpp:
// 15-46, multi_numerical_hash_aggregate.cpp:17-43) and OneGroupAggregate (one_group_aggregate.cpp:9-26).
//
// Design facts measured on MI355X (tools/microbench.hip, profiles/microbench_r01.txt):
//   * device-scope atomics top out at ~24 G/s regardless of table size  -> never one per row;
//   * LDS atomics sustain > 1 T row-updates/s chip-wide                  -> every row lands in LDS;
//   * a grid of 8 x 256 CUs grid-striding 16 B/lane streams 6.3 TB/s.
// So rows are pre-aggregated in a per-workgroup LDS hash table (keys + 64-bit accumulator words that
// merge commutatively); only table flushes touch the HBM-resident table, with agent-scope atomics.
// The fused WHERE predicate is evaluated in the scan, so no filtered batch is ever materialised.  Host side: this file keeps the handle, the C-ABI entry points, the queue of a stream (queueable, flush_queue) and the widening helpers; vnm_agg_next.inc takes a batch to its kernels (next_device_impl: one stage function per family of routes).
#include <memory>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "vnm_agg.hpp"

namespace vnm {

constexpr uint64_t EMPTY = ~0ULL;
constexpr uint64_t LOCKED = ~0ULL - 1;
constexpr int AGG_BLOCK = 1024;        // LDS kernel: 16 waves, one workgroup per CU
#ifndef VNM_AGG_R
#define VNM_AGG_R 8
#endif
constexpr int AGG_ROWS_PER_THREAD = VNM_AGG_R;
constexpr int AGG_TILE = AGG_BLOCK * AGG_ROWS_PER_THREAD;
constexpr int AGG_LDS_BUDGET = 128 * 1024;
constexpr int AGG_MAX_PROBES = 48;
constexpr int OG_BLOCK = 256;

// HBM-resident table: tag[] (the key itself on the single-key path), optional wide key words, and
// SoA accumulator words.  Arrays have cap + 2 entries: [cap] = the group whose key equals the EMPTY
// sentinel, [cap + 1] = the NULL-key group (single_numerical_hash_aggregate.cpp:24-32).
struct GTable {
    uint64_t* tag;
    uint64_t* keyw;  // kwt * stride (wide keys only)
    uint64_t* acc;   // n_words * stride
    uint64_t cap;    // power of two
    uint64_t stride; // cap + 2
    unsigned long long* ctl;  // [0] ticket  [1] overflow flag  [2] fill (groups in table)  [3] dense count
    int kwt;         // wide key words (0 on the single-key path)
    int n_words;
};

// ---- expressions inside aggregates, evaluated in registers -------------------------------------------------------------
// `SELECT k, sum((1 - total) * (2 + tax) * (1 - tip)) ... GROUP BY k` (vinum/tests/test_query_results.py:436-443): the
// reference's planner projects the expression into a temporary column first (planner.py:384-417, one NumPy pass and one
// n-row temporary per AST node) and the aggregate re-reads it.  Here the input of the hot-shape aggregate may BE an
// expression: a postfix program over up to four float64 columns without NULLs, evaluated per row pair where the scan /
// partition kernels used to load the value column -- no materialised column, no extra pass.  float64 +, -, *, /, negation
// one IEEE operation per AST node (the interpreter's dispatch keeps the compiler from contracting a*b+c into an FMA), so the
// values are bit-identical to the projection kernel's and to NumPy's.  Anything else (other types, NULLs, more columns,
// deeper stacks, other aggregate shapes) is materialised by vnm_project first (vnm_agg_next_device_expr).
constexpr int EXR_MAX_INS = 16, EXR_MAX_COLS = 4, EXR_MAX_DEPTH = 4;
struct ExprIns { int op; int arg; double imm; };
struct ExprProg {
    int n;
    const double* cols[EXR_MAX_COLS];
    ExprIns ins[EXR_MAX_INS];
};
// the stack lives in four named registers (a dynamically indexed array would go to scratch memory)
template <typename V, typename LOADER>
__device__ __forceinline__ V expr_eval(const ExprProg& e, LOADER&& load_col, V splat_zero) {
    V s0 = splat_zero, s1 = splat_zero, s2 = splat_zero, s3 = splat_zero;
    for (int i = 0; i < e.n; i++) {
        const int op = e.ins[i].op;
        if (op == VNM_EX_COL || op == VNM_EX_CONST_F) {
            s3 = s2; s2 = s1; s1 = s0;
            s0 = op == VNM_EX_COL ? load_col(e.ins[i].arg) : splat_zero + e.ins[i].imm;
        } else if (op == VNM_EX_NEG) {
            s0 = -s0;
        } else {
            const V b = s0, a = s1;
            s1 = s2; s2 = s3;
            switch (op) {
                case VNM_EX_ADD: s0 = a + b; break;
                case VNM_EX_SUB: s0 = a - b; break;
                case VNM_EX_MUL: s0 = a * b; break;
                default: s0 = a / b; break;
            }
        }
    }
    return s0;
}
typedef double expr_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 expr_eval2(const ExprProg& e, int64_t r) {   // rows r, r + 1 (r even: 16-byte loads)
    const expr_v2 z = {0.0, 0.0};
    const expr_v2 v = expr_eval<expr_v2>(e, [&](int c) { return *(const expr_v2*)(e.cols[c] + r); }, z);
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ double expr_eval1(const ExprProg& e, int64_t r) {
    return expr_eval<double>(e, [&](int c) { return e.cols[c][r]; }, 0.0);
}

// One record batch of a STREAM handed to a kernel as part of one logical batch (vnm_agg_set_async: batches wait in the operator and
// go to the device together -- a launch per 2^24-row batch costs more in launch gaps, LDS table start-up and partial flushes than
// its rows).  The hot shape only: 8-byte key, one plain float64 input column, float64 predicate column or none.  A segment owns
// the tiles [first_tile, first_tile + ceil(nrows / tile)) of the launch; tiles never span segments.
struct VSeg {
    const uint64_t* kp;      // key values (Arrow offset applied; 16-byte aligned)
    const uint64_t* vp;      // input column values
    const double* pp;        // predicate column values (the input column itself when the predicate reads it)
    const uint8_t* vvalid;   // validity bitmap of the input column or null (dense path over a nullable value column)
    int64_t voff;
    int64_t nrows;
    int64_t first_tile;
};

// The segment table is read through the CONSTANT address space (nobody writes it while the kernel runs): uniform loads from it are
// scalar loads (s_load: the scalar cache, results in scalar registers, no wait on the wave's outstanding vector loads).  Through a
// plain global pointer the same reads are vector loads -- the compiler cannot scalarise loads from memory the kernel also stores
// to -- whose latency, behind a saturated memory system, sat on every tile's critical path and whose results occupied vector
// registers (58 segments, G = 7: 4.1 ms against 2.7 for the same rows as one batch).
typedef const VSeg __attribute__((address_space(4)))* VSegConst;
__device__ __forceinline__ VSegConst seg_table(const VSeg* p) { return (VSegConst)(uintptr_t)p; }
// A value every lane of the wave holds alike, moved into scalar registers.  Loads through a.segs are uniform, but the compiler
// cannot scalarise loads from memory the kernel also stores to: the segment pointers then sit in vector registers -- two sets of
// them, this tile's and the next one's -- and the scan kernel spilled 46-116 VGPRs (58 segments, G = 7: 4.1 ms against 2.7 for
// the same rows as one batch).
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <typename T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) { return (const T*)uniform_u64((uint64_t)p); }

struct AggArgs {
    AggPlan plan;
    const VSeg* segs;  // agg_hot_kernel, nseg > 0: the rows are these segments (keys[0] / cols[0] / pred describe the first one)
    int nseg;
    int has_expr;      // the (only) input column of this hot-shape plan is `expr`, not a.cols[0]
    ExprProg expr;
    vnm_dcol keys[AGG_MAX_KEYS];
    vnm_dcol cols[AGG_MAX_COLS];
    vnm_dcol pred;
    Predicate p;
    GTable g;
    int64_t nrows;
    int64_t ntiles;
    int64_t fill_limit;   // take a new tile only while fill + margin <= fill_limit
    int64_t margin;
    int lds_slots;
    unsigned int* progress;  // per-block loop index to resume from
    // hot-shape kernel (single 8-byte key, one float64 input column, no validity bitmaps)
    int hot_w_rows, hot_w_valid, hot_w_sum;
    int hot_comp;      // float64 sums are compensated (hi, lo) pairs: M_ADD_F64C
    int hot_pred_is_v;
    // extended hot shape: every accumulator kind over ONE 8-byte input column without NULLs (or no input at all)
    int hot_w[9];      // word of each AccKind, -1 = absent
    int hot_w2[9];     // ... for a second input column (agg_hot_kernel<TWO>)
    int hot_vtype2;
    unsigned long long hot_wpack, hot_wpack2;  // the same tables, 6 bits per kind (63 = absent, COUNT(*) excluded): scalar registers
    int hot_vtype;     // VNM_F64 / VNM_I64 / VNM_U64
    int hot_has_val;
    const ulonglong2* ent;  // agg_hot_kernel<FROM_ENT>: (key, value bits) entries spilled by the partitioned path
    int part_generic;  // partitioned path with a generic accumulator program over one 8-byte column (or none)
    int part_vtype;
    int part_vtypes[6];  // wide entries: type of each input column
    int part_wide;       // wide entries (several input columns, NULLs, narrow types, any predicate column)
    int part_vmask;      // ... with a validity word
    int debug;  // timing experiments (VNM_AGG_DEBUG): 1 = no accumulator ops, 2 = no probes either, 4 = no room check
    // agg_hotn_kernel: {COUNT(*), COUNT, SUM, AVG} over THREE to SIX plain float64 columns
    int hn_w_sum[6];    // word of each column's sum (-1: the column is only counted)
    int hn_w_base;      // the count word the kernel maintains; the others are copies of it before a flush (no NULLs: every count is the row count)
    int hn_n_copy;
    int hn_w_copy[7];
    int hn_pred_col;    // the predicate column is this input column (-1: a column of its own, a.pred)
    int hn_ctype[6];    // VNM_F64 / VNM_I64 / VNM_U64
    int hn_iw[6][4];    // integer sums of the column: word of A_SUM_I64 / A_SUM_LO32 / A_SUM_HI32S / A_SUM_HI32U (-1: absent)
    int hn_any_int;
    int hn_wmm[6][2];   // MIN / MAX words of the column (-1: absent)
    int hn_any_mm;
};

// ---- global table primitives ------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exact rounding error of s = fl(a + b) (Knuth's TwoSum: a + b == s + e in real arithmetic).  Zero when the sum
// overflowed or an operand was not finite, so that inf / NaN results are what a plain sum gives.
__device__ __forceinline__ double two_sum_err(double a, double b, double s) {
    const double bb = s - a;
    const double e = (a - (s - bb)) + (b - bb);
    return (s - s == 0.0) ? e : 0.0;
}
// Compensated add into the (hi, lo) word pair of an M_ADD_F64C accumulator: hi = fl(hi + x) with a RETURNING atomic,
// the exact error of that add goes to lo (the word `ws` elements further on).  Exact adds (the benchmark's quantised
// data) never touch lo.
__device__ __forceinline__ void g_add_f64c(uint64_t* p, int64_t ws, double x) {
    const double old = __hip_atomic_fetch_add((double*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double e = two_sum_err(old, x, old + x);
    if (e != 0.0) __hip_atomic_fetch_add((double*)(p + ws), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void l_add_f64c(uint64_t* p, int ws, double x) {
    const double old = __hip_atomic_fetch_add((double*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const double e = two_sum_err(old, x, old + x);
    if (e != 0.0) __hip_atomic_fetch_add((double*)(p + ws), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ws: distance (in elements) between consecutive accumulator words of one group (M_ADD_F64C updates word + 1 too)
__device__ __forceinline__ void g_merge(uint64_t* p, int mk, uint64_t v, int64_t ws) {
    switch (mk) {
        case M_ADD_U64: __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;
        case M_ADD_F64: __hip_atomic_fetch_add((double*)p, __longlong_as_double((long long)v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;
        case M_ADD_F64C: g_add_f64c(p, ws, __longlong_as_double((long long)v)); break;
        case M_MIN_U64: __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;
        default: __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break;
    }
}
__device__ __forceinline__ void l_merge(uint64_t* p, int mk, uint64_t v, int ws) {
    switch (mk) {
        case M_ADD_U64: __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break;
        case M_ADD_F64: __hip_atomic_fetch_add((double*)p, __longlong_as_double((long long)v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break;
        case M_ADD_F64C: l_add_f64c(p, ws, __longlong_as_double((long long)v)); break;
        case M_MIN_U64: __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break;
        default: __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break;
    }
}

// single 64-bit key: the tag word IS the key; claim by CAS from EMPTY
// New groups are counted into a block-local LDS counter (*newc) and folded into the table's fill word once per
// tile: one agent-scope atomic per NEW GROUP on a single word capped merges at ~1 group/ns (122 ms per 1e8).
__device__ __forceinline__ uint64_t gt_find_single(const GTable& g, uint64_t key, unsigned* newc) {
    const uint64_t mask = g.cap - 1;
    uint64_t h = hash_u64(key) & mask;
    for (uint64_t probes = 0;; probes++) {
        if (probes > mask) {  // table full: cannot happen while the room checks hold; never spin forever
            __hip_atomic_store(&g.ctl[1], 2ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return g.cap;
        }
        uint64_t k = ld_agent(&g.tag[h]);
        if (k == key) return h;
        if (k == EMPTY) {
            uint64_t expected = EMPTY;
            if (__hip_atomic_compare_exchange_strong(&g.tag[h], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                atomicAdd(newc, 1u);
                return h;
            }
            if (expected == key) return h;
        }
        h = (h + 1) & mask;
    }
}

__device__ __forceinline__ uint64_t wide_tag(const uint64_t* kw, int n) {
    uint64_t h = 0x9E3779B97F4A7C15ULL * (uint64_t)n;
    for (int i = 0; i < n; i++) {
        uint64_t x = kw[i];
        h ^= (uint64_t)hash_u64(x) * 0x9E3779B1ULL + ((uint64_t)hash_u64(x ^ 0x5bd1e995) << 32) + (h << 6) + (h >> 2);
    }
    return h & 0x7FFFFFFFFFFFFFFFULL;
}

// wide keys: tag = 63-bit hash; EMPTY -> LOCKED -> tag.  The claimer publishes the key words with
// write-through agent-scope stores, drains them, then publishes the tag (no lane ever waits inside the
// critical section, so same-wave spinners cannot deadlock).
__device__ __forceinline__ uint64_t gt_find_wide(const GTable& g, const uint64_t* kw, uint64_t tagv, unsigned* newc) {
    const uint64_t mask = g.cap - 1;
    uint64_t h = (tagv ^ (tagv >> 29)) & mask;
    for (;;) {
        uint64_t t = ld_agent(&g.tag[h]);
        if (t == tagv) {
            bool eq = true;
            for (int i = 0; i < g.kwt; i++) eq = eq && (ld_agent(&g.keyw[(uint64_t)i * g.stride + h]) == kw[i]);
            if (eq) return h;
            h = (h + 1) & mask;
            continue;
        }
        if (t == EMPTY) {
            uint64_t expected = EMPTY;
            if (__hip_atomic_compare_exchange_strong(&g.tag[h], &expected, LOCKED, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                for (int i = 0; i < g.kwt; i++) st_agent(&g.keyw[(uint64_t)i * g.stride + h], kw[i]);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_agent(&g.tag[h], tagv);
                atomicAdd(newc, 1u);
                return h;
            }
            continue;  // someone else is claiming this slot: look at it again
        }
        if (t == LOCKED) continue;
        h = (h + 1) & mask;
    }
}

// one thread per block folds the block's new-group count into the table's fill word
__device__ __forceinline__ void fold_new(const GTable& g, unsigned* s_new) {
    unsigned v = atomicExch(s_new, 0u);
    if (v) atomicAdd(&g.ctl[2], (unsigned long long)v);
}

// ---- per-row accumulator contributions ----------------------------------------------------------------
// Returns false when the op contributes nothing for this row (NULL input); otherwise the value to merge.
__device__ __forceinline__ bool op_value(const AccOp& op, const vnm_dcol* cols, int64_t row, uint64_t* out) {
    if (op.kind == A_COUNT_ROWS) { *out = 1; return true; }
    const vnm_dcol& c = cols[op.col];
    if (!col_valid(c, row)) return false;
    switch (op.kind) {
        case A_COUNT_VALID: *out = 1; return true;
        case A_SUM_F64: *out = (uint64_t)__double_as_longlong(col_f64(c, row)); return true;
        case A_SUM_I64: *out = (uint64_t)col_i64(c, row); return true;
        case A_SUM_LO32: *out = (uint64_t)col_i64(c, row) & 0xFFFFFFFFULL; return true;
        case A_SUM_HI32S: *out = (uint64_t)(col_i64(c, row) >> 32); return true;
        case A_SUM_HI32U: *out = (uint64_t)col_i64(c, row) >> 32; return true;
        default:  // A_MIN / A_MAX on the order-preserving encoding
            if (type_is_float(c.type)) *out = enc_f64(col_f64(c, row));
            else if (type_is_unsigned(c.type)) *out = (uint64_t)col_i64(c, row);
            else *out = enc_i64(col_i64(c, row));
            return true;
    }
}

// Tiles are statically strided over the grid (tile = block + i * grid): no shared ticket word, so the
// scan never serialises on one atomic (a CAS ticket per 2048-row tile cost 1.3 s per 1e9 rows).  Before
// each tile the block checks that the HBM table has room for everything that can be in flight; if not it
// raises the overflow flag, parks its loop index in progress[block] and exits so the host can grow the
// table and relaunch the same grid from where every block stopped.
__device__ __forceinline__ bool table_has_room(const AggArgs& a, unsigned* s_new) {
    fold_new(a.g, s_new);
    unsigned long long fill = __hip_atomic_load(&a.g.ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int64_t)fill + a.margin > a.fill_limit) {
        __hip_atomic_store(&a.g.ctl[1], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
    }
    return true;
}

#include "vnm_agg_scan.inc"

#include "vnm_agg_tuple.inc"

#include "vnm_agg_onegroup.inc"

#include "vnm_agg_table.inc"

#include "vnm_ring.inc"

#include "vnm_agg_part.inc"

#include "vnm_agg_pack.inc"

#include "vnm_agg_dense.inc"

#include "vnm_agg_finalize.inc"

}  // namespace vnm

// ==========================================================================================================
// host side
// ==========================================================================================================
using namespace vnm;

struct DensePending {
    DFinalArgs df;         // what every batch shares: the code map, the words of the plan, the flags block
    int tb = 0, levels = 0, p1 = 0, fsplits = 1;
    int64_t nfinal = 0;
    int64_t dstride = 0;   // bound of the groups the pass can produce
    int64_t rows = 0;      // rows behind the sets: below 2^32, the slots of the final pass count a group's rows in 32 bits
    // exact-add statistics over the batches of the pass (exact_track): known only while every batch came through a scatter that keeps them
    bool x_known = true;
    uint32_t x_inv = 0, x_exp = 0;
    bool exact_ok() const { return x_known && exact_adds_proved(((unsigned long long)x_exp << 32) | x_inv, rows); }
    std::vector<DSet> sets;      // one per batch whose scatter passes are done
    std::vector<void*> blocks;   // pool blocks the entries live in
    DSet* dsets = nullptr;       // device copy of `sets` (refreshed by complete_pending)
    DTabSlot* table = nullptr;   // DF_TABLE result (kept until the handle goes: the exchange reads it)
    ~DensePending() { for (void* b : blocks) pool_free(b); pool_free(table); pool_free(dsets); }
};
constexpr size_t DP_MAX_SETS = 512;   // batches a deferred pass may span (then it runs, as a run, and a new one starts)
// the table a stream of small-range batches accumulates in (dscan_accumulate_kernel); groups are written by flush_scan_pending
struct DScanPending {
    DFinalArgs df{};   // code map + the words of the plan
    DScanTable t{};
    int slots = 0;
    uint64_t* part_sum = nullptr;   // the current batch's per-workgroup tables [cus][slots] (kept: no allocation per batch)
    float* part_lo = nullptr;
    uint32_t* part_cnt = nullptr;
    unsigned long long* flags = nullptr;
    ~DScanPending() { pool_free(t.sum); pool_free(t.lo); pool_free(t.cnt); pool_free(part_sum); pool_free(part_lo); pool_free(part_cnt); pool_free(flags); }
};

struct vnm_agg {
    AggPlan plan;
    FuncOut outs[AGG_MAX_FUNCS];
    int n_funcs = 0;
    int func_col[AGG_MAX_FUNCS];   // distinct column index per func (-1 for COUNT(*))
    int col_first_func[AGG_MAX_COLS];
    bool single = false;           // single 64-bit key path
    Predicate pred{};
    bool pred_set = false;
    int pred_op = 0, pred_is_float = 0;
    double pred_dval = 0;
    int64_t pred_ival = 0;
    int64_t hint = 0;
    GTable g{};
    bool have_table = false;
    int64_t rows_seen = 0;
    // dense result (device + host mirror)
    uint64_t* dkey = nullptr;
    uint64_t* dacc = nullptr;
    int64_t dstride = 0;
    int64_t n_groups = -1;
    std::vector<uint64_t> h_key, h_acc;
    bool host_ready = false;
    // dense run produced by the partitioned path (not yet merged into the HBM table)
    uint64_t* run_key = nullptr;
    uint64_t* run_acc = nullptr;
    int64_t run_stride = 0, run_n = 0;
    bool have_run = false;
    bool result_is_run = false;
    bool estimated = false;  // hint came from estimate_groups()
    int64_t merge_stride = 0;  // set by vnm_agg_merge_rows around vnm_agg_merge_device
    unsigned long long* run_dir = nullptr;  // partition directory of the run (partitioned path, one workgroup per partition)
    int64_t run_nfin = 0;
    // packed composite keys (multi-column GROUP BY through the single-key machinery)
    vnm_agg* inner = nullptr;
    bool pack_tried = false;
    bool key_only_failed = false;  // COUNT(*)-only programs: 8-byte entries overflowed a region once (skewed keys)
    // dense-key partitioned path (vnm_agg_dense.inc): 0 = range not sampled yet, 1 = code map valid, -1 = not applicable
    int dense_state = 0;
    DenseMap dmap{};
    int64_t dense_span = 0;  // 2^bits: upper bound of the groups a dense run can hold
    uint64_t dense_rlo = 0, dense_rhi = 0;  // the sampled (widened) range itself, as order-preserving unsigned images
    bool rank_aligned = false;  // vnm_agg_set_exchange_mode: only run layouts every rank derives identically
    // dense path, final pass DEFERRED (round 3): the scatter passes of the last batch are done, the direct-addressed final pass
    // has not run yet -- what it writes depends on who asks: another batch / finish() -> the dense partial state (a run),
    // vnm_agg_result_device_alloc -> the result columns themselves, vnm_agg_dense_table -> the tables for the multi-GPU exchange
    struct DensePending* pending = nullptr;
    double heavy_share = 0.0;   // share of the rows held by heavy keys in the estimator's sample (0: none seen, or never sampled)
    // A single narrow integer key (int8 .. uint32) is WIDENED to int64 / uint64 on arrival (round 5): every specialised path reads plain
    // 8-byte keys, and such keys took the interpreted scan and the generic entries at 1.5-2.9 x the time for fewer bytes.  The plan then
    // says int64 / uint64 (the key WORD of a narrow key is its sign- / zero-extended value anyway: array_iterators.h:215-217), the result
    // columns keep the type the caller declared.  The widened buffers live until no recorded batch needs them (sequence numbers).
    int key_out_type = -1;
    std::vector<std::pair<int64_t, void*>> widened;
    // ... and float32 INPUT columns under SUM / AVG / COUNT only (the reference sums float32 in double anyway: SumFunc<float, double>,
    // AvgFunc<float, double, double>, agg_func_factory.cpp:126-131, 206-211): widened to float64 on arrival, so that `sum(v), avg(v) WHERE v > x`
    // over a float32 column takes the float64 kernels.  A predicate over such a column compares in float32 in the reference (NumPy:
    // float32 array against a Python scalar) -- the same as comparing the widened values with the literal ROUNDED to float32.
    bool widen_in[AGG_MAX_FUNCS] = {};
    bool any_widen_in = false;
    bool pred_lit_rounded = false;   // pred_dval holds the literal rounded to float32 (the caller's literal: pred_user_*)
    int pred_user_is_float = 0;
    double pred_user_dval = 0.0;
    int64_t pred_user_ival = 0;
    // fixed-point entries on the dense path (round 6, DPartArgs::fx_q): 0 = the value column has not been sampled yet, 1 = on (every value of
    // the sample is m * 2^fx_qe with |m| < 2^31 and room to spare), -1 = off (the sample or a later row does not fit)
    int fx_state = 0, fx_qe = 0;
    bool pack_null_seen = false;     // packed composite keys: some batch brought a key column with a validity bitmap (NULL codes may be in the words)
    bool pring_off = false;          // the ring form of the hash-partition scatter failed once (a heavy key, a full region): the tile-sorting scatter from then on
    bool fx_narrow = false;          // ... with |m| < 2^18: the words of the last scatter level are 32 bits (dring_scatter_kernel<..., W32>)
    int fx_L = 0, fx_E = 0;          // ... what the sample saw: lowest set bit 2^fx_L, |v| < 2^fx_E, smallest and largest value
    double fx_vmin = 0.0, fx_vmax = 0.0;
    bool fx_narrow1_off = false;     // a row fell outside the window of the first level's 32-bit words once (plan_narrow_first_level): 8-byte words there from then on
    int fxn_state = 0, fxn_qe[3] = {0, 0, 0};   // ... and of the entries of two or three values (vnm_agg_fxn.inc)
    bool null_inputs_seen = false;   // some batch brought an input column with a validity bitmap: the HBM table may hold groups whose COUNT(v) differs
                                     // from COUNT(*) (or whose SUM is NULL) -- the side-table fold of the fused result columns assumes they do not
    bool count8_off = false;    // the counters of COUNT(*)-only programs overflowed once (dcount8_final_kernel): not again
    int count_cb = 0;           // ... their width once the bytes overflowed: 16
    struct DScanPending* scan_pending = nullptr;   // a stream of small-range batches: their table (see dense_scan_stream)
    bool dense_by_bound = false;   // the first batch went dense on the sample's LOWER bound of the group count (no estimate exists)
    bool range_given = false;   // vnm_agg_set_dense_range: the code range is the caller's (agreed by all ranks), not a sample's
    // expression input (vnm_agg_set_input_expr): the functions reading plan column expr_col get an expression's value
    int expr_col = -1;
    std::vector<vnm_expr_ins> expr_prog;
    int expr_ncols = 0;
    bool expr_fusable = false;   // the program fits the in-register evaluator (float64 + - * / neg, <= 16 ins, depth <= 4)
    bool expr_active = false;    // set around one vnm_agg_next_device call: evaluate expr_dev in the scan instead of a column
    ExprProg expr_dev{};
    PackParams pack{};
    int c_funcs[AGG_MAX_FUNCS], c_in_types[AGG_MAX_FUNCS], c_in_flags[AGG_MAX_FUNCS], c_in_col_ids[AGG_MAX_FUNCS];
    bool c_has_ids = false;
    // program split (round 3): more input columns than one partition entry carries (key + six words) used to mean the LDS
    // scan with its flush storms at large G.  The function list is cut into sub-operators over a few columns each, all over
    // the same key; every batch goes through each of them and their results are joined by key when the state is needed
    // (collapse_parts: a run in ascending key order).
    // tuple dictionary (round 3, tuple_gid_kernel): key sets that do not pack into one word.  tdict maps tuple -> group id;
    // `inner` aggregates by that id
    TDict tdict{};
    int64_t widest_est = 0;                // plan_packing: the largest distinct-count estimate of a single key column
    unsigned long long* tnext = nullptr;   // device: first group id not handed out yet
    bool tuple_mode = false;
    std::vector<vnm_agg*> parts;
    std::vector<std::vector<int>> part_funcs;   // [part][function of the part] -> function index here
    bool split_tried = false;
    // Asynchronous streams (round 4, vnm_agg_set_async): hot-shape batches WAIT here (the caller keeps their buffers alive) and go
    // to the device together as the segments of one logical batch -- at vnm_agg_sync / finish / result, when 2^30 rows or 256
    // batches are waiting, or when a batch of another shape arrives.  No host read-back, allocation or launch per next().
    bool async = false;
    struct QBatch { int64_t nrows; vnm_dcol key, col, pred; std::vector<vnm_dcol> ins; int64_t seq; };   // ins: one column per function (several input columns); seq: see cur_seq
    bool q_multi = false;                  // the waiting batches carry several input columns (they are cut into parts when they go to the device)
    std::vector<QBatch> q;
    int64_t q_rows = 0;
    bool q_pred_is_v = false;
    const std::vector<QBatch>* segs_active = nullptr;   // set around the one vnm_agg_next_device call that processes the queue
    // a NULLABLE single key through the dense path (round 4): set around one next_device_impl call whose keys[0] had its validity
    // stripped -- pass 1 reads it (dring_scatter_kernel<..., KN>) and sums the NULL-key rows into the HBM table's NULL slot
    const uint8_t* kn_valid = nullptr;
    int64_t kn_off = 0;
    bool kn_failed = false;      // the dense path did not take such a batch once: later ones go straight to the packed route
    std::vector<VSeg> seg_host;                         // the segment table of the last launch (kept until the next one: H2D source)
    // reference-exact float MIN / MAX under NaNs and mixed-sign zeros (round 5, vnm_agg_exact.inc): top-level handles only
    struct vnm_agg_exact* ex = nullptr;
    // Which batches a stream still needs the buffers of (vnm_agg_waiting): every vnm_agg_next_device call on a TOP-LEVEL handle takes the
    // next sequence number; a recorded batch keeps the number of the call that brought it, also when it is handed on to the operators
    // the handle runs for itself (parts, the suffix operator of an ordered MIN / MAX stream), which record under the caller's number.
    bool child = false;
    int64_t seq = 0;        // calls so far (top-level handles)
    int64_t cur_seq = -1;   // number of the batch being handed in
};

namespace {

int table_alloc(vnm_agg* h, GTable* g, uint64_t cap, hipStream_t s) {
    memset(g, 0, sizeof(*g));
    g->cap = cap;
    g->stride = cap + 2;
    g->kwt = h->single || h->plan.n_keys == 0 ? 0 : h->plan.n_keys + 1;
    g->n_words = h->plan.n_words;
    g->tag = (uint64_t*)pool_alloc(g->stride * 8);
    g->acc = (uint64_t*)pool_alloc(g->stride * 8 * (size_t)g->n_words);
    g->ctl = (unsigned long long*)pool_alloc(64);
    if (g->kwt) g->keyw = (uint64_t*)pool_alloc(g->stride * 8 * (size_t)g->kwt);
    if (!g->tag || !g->acc || !g->ctl || (g->kwt && !g->keyw)) return 1;
    VNM_HIP(hipMemsetAsync(g->tag, 0xFF, g->stride * 8, s));
    VNM_HIP(hipMemsetAsync(g->ctl, 0, 64, s));
    for (int w = 0; w < g->n_words; w++) {
        const uint64_t init = merge_init(h->plan.merge[w]);
        if (init == 0 || init == ~0ULL) VNM_HIP(hipMemsetAsync(g->acc + (size_t)w * g->stride, init ? 0xFF : 0, g->stride * 8, s));
        else {   // (float sums start at -0.0: not a byte pattern)
            fill_u64_kernel<<<(int)std::min<uint64_t>((g->stride + 255) / 256, (uint64_t)device_info().num_cus * 8), 256, 0, s>>>(g->acc + (size_t)w * g->stride, init, (int64_t)g->stride);
            VNM_HIP(hipGetLastError());
        }
    }
    return 0;
}

void table_free(GTable* g) {
    pool_free(g->tag);
    pool_free(g->acc);
    pool_free(g->keyw);
    pool_free(g->ctl);
    memset(g, 0, sizeof(*g));
}

uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

int lds_slots_for(const AggPlan& p, int budget = AGG_LDS_BUDGET) {
    int per_slot = 8 * (1 + p.n_words);
    int s = 1;
    while ((s * 2 + 2) * per_slot <= budget) s *= 2;
    if (s > 8192) s = 8192;
    return s;
}

// grow the table by rehashing every occupied slot into a larger one
int table_grow(vnm_agg* h, uint64_t new_cap, hipStream_t s) {
    GTable old = h->g, ng;
    VNM_TRY(table_alloc(h, &ng, new_cap, s));
    MergeArgs m{};
    m.plan = h->plan;
    m.g = ng;
    m.n = (int64_t)old.stride;
    m.src_is_table = 1;
    m.src_stride = 1;
    m.src_tag = old.tag;
    m.src_cap = (int64_t)old.cap;
    for (int j = 0; j < old.kwt; j++) m.src_key[j] = old.keyw + (size_t)j * old.stride;
    for (int w = 0; w < old.n_words; w++) m.src_acc[w] = old.acc + (size_t)w * old.stride;
    int grid = device_info().num_cus * 8;
    agg_merge_kernel<<<grid, 256, 0, s>>>(m);
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipStreamSynchronize(s));
    table_free(&old);
    h->g = ng;
    return 0;
}

// rows_only: the rows are what a partitioned pass spilled (the groups of the batch live in its run) -- the table is sized by them,
// not by the group count hint (a handful of spilled entries under a hint of 1e8 groups used to get a 2^28-slot table: its memset,
// and the walk over its slots at finish, cost 2-4 ms)
int ensure_table(vnm_agg* h, int64_t nrows, hipStream_t s, bool rows_only = false) {
    if (h->have_table) return 0;
    uint64_t cap;
    if (h->plan.n_keys == 0) cap = 2;
    else {
        uint64_t want = h->hint > 0 ? (uint64_t)h->hint * 2 : (uint64_t)1 << 22;
        if ((h->hint <= 0 || rows_only) && (uint64_t)nrows * 2 < want) want = (uint64_t)(nrows > 512 ? nrows : 512) * 2;
        // (spilled rows are mostly FEW keys -- a heavy key's 3e7 entries got a 2^26-slot table: its memset and the walks over its
        // slots at finish, run_patch_append_kernel 2.9 ms; the scan grows the table when the keys are many after all)
        if (rows_only && want > (1ULL << 20)) want = 1ULL << 20;
        cap = pow2_at_least(want < 1024 ? 1024 : want);
    }
    VNM_TRY(table_alloc(h, &h->g, cap, s));
    h->have_table = true;
    return 0;
}

void invalidate_result(vnm_agg* h) {
    if (!h->result_is_run) {
        pool_free(h->dkey);
        pool_free(h->dacc);
    }
    h->result_is_run = false;
    h->dkey = h->dacc = nullptr;
    h->n_groups = -1;
    h->host_ready = false;
}

// ---- partitioned path orchestration -------------------------------------------------------------------
int64_t env_i64(const char* name, int64_t dflt) {
    const char* v = getenv(name);
    return v ? (int64_t)atoll(v) : dflt;
}

void drop_run(vnm_agg* h) {
    pool_free(h->run_key);
    pool_free(h->run_acc);
    pool_free(h->run_dir);
    h->run_dir = nullptr;
    h->run_nfin = 0;
    h->run_key = h->run_acc = nullptr;
    h->have_run = false;
    h->run_n = h->run_stride = 0;
}
// The run belongs to the handle from here on (the caller has keep()-ed its blocks); dir / nfin: the hash partitions' partition directory.
void adopt_run(vnm_agg* h, uint64_t* key, uint64_t* acc, int64_t stride, int64_t n, unsigned long long* dir = nullptr, int64_t nfin = 0) {
    h->run_key = key; h->run_acc = acc; h->run_stride = stride; h->run_n = n;
    h->run_dir = dir; h->run_nfin = nfin;
    h->have_run = true;
}

// distinct-key estimate from a strided sample (tiered: a small sample settles small G cheaply)
// tier0_lb (optional): when the small sample cannot settle G (most sampled keys distinct) return right there with
// *est = 0 and a LOWER bound of G from the uniform model -- the dense-key path only needs to know that G is large.
int estimate_groups(vnm_agg* h, const vnm_dcol& key, int64_t nrows, int64_t* est, hipStream_t s, int64_t* tier0_lb = nullptr) {
    const uint64_t* kp = (const uint64_t*)key.values + key.offset;
    int64_t sizes[2] = {std::min<int64_t>(nrows, 1 << 18), std::min<int64_t>(nrows, 1 << 24)};
    *est = 0;
    double heavy_share = 0.0;   // share of the rows held by heavy keys, and how many of those there are (from tier 0's sample)
    int64_t heavy_keys = 0;
    // tier 0: small sample into a scratch table (exact distinct count of the sample, ~50 us)
    {
        const int64_t m = sizes[0];
        GTable t{};
        t.cap = pow2_at_least((uint64_t)m * 2);
        t.stride = t.cap + 2;
        t.tag = (uint64_t*)pool_alloc(t.stride * 8);
        t.ctl = (unsigned long long*)pool_alloc(64);
        unsigned int* cnt = (unsigned int*)pool_alloc(t.cap * 4);
        if (!t.tag || !t.ctl || !cnt) return 1;
        VNM_HIP(hipMemsetAsync(t.tag, 0xFF, t.stride * 8, s));
        VNM_HIP(hipMemsetAsync(t.ctl, 0, 64, s));
        VNM_HIP(hipMemsetAsync(cnt, 0, t.cap * 4, s));
        int grid = (int)std::min<int64_t>((m + 255) / 256, (int64_t)device_info().num_cus * 8);
        agg_sample_kernel<<<grid, 256, 0, s>>>(kp, nrows, m, t, cnt, h->kn_valid, h->kn_off);
        agg_sample_heavy_kernel<<<grid, 256, 0, s>>>(cnt, (int64_t)t.cap, (unsigned int)std::max<int64_t>(64, m / 256), t.ctl);
        VNM_HIP(hipGetLastError());
        unsigned long long got[6] = {0, 0, 0, 0, 0, 0};
        VNM_HIP(hipMemcpyAsync(got, t.ctl, 48, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        pool_free(t.tag);
        pool_free(t.ctl);
        pool_free(cnt);
        unsigned long long d = got[2];
        if (d == 0) d = 1;
        // Heavy keys (each with > 0.4 % of the sample: NULLs, a default value) break the uniform model below -- half of the
        // rows in one key halves d / m and G came out 2.2x too small.  They are taken out: the model sees the remaining keys
        // over the remaining rows, and the heavy keys are added back as what they are, a handful of groups.
        h->heavy_share = got[5] ? (double)got[4] / (double)m : 0.0;   // (any key above 0.4 % of the sample: pass 2 of the dense path splits finer)
        if ((double)got[4] >= 0.02 * (double)m && got[5] < d) {
            heavy_share = std::min(0.999, (double)got[4] / (double)m);
            heavy_keys = (int64_t)got[5];
        }
        const double m0 = (double)m * (1.0 - heavy_share);
        const double d0 = (double)d - (double)heavy_keys;
        if (d0 / m0 < 0.125 || m == nrows) {  // the sample saw (nearly) every group
            *est = (int64_t)((double)d * (m == nrows ? 1.0 : 1.15)) + 1;
            return 0;
        }
        if (tier0_lb) {
            const double frac = std::min(0.97, d0 / m0);  // beyond 0.97 the sample has no resolution: G >= ~16 m
            double lo = 1e-9, hi = 64.0;
            for (int it = 0; it < 80; it++) {
                const double x = 0.5 * (lo + hi);
                if ((1.0 - exp(-x)) / x > frac) lo = x; else hi = x;
            }
            *tier0_lb = (int64_t)(m0 / (0.5 * (lo + hi)));
            return 0;
        }
    }
    // tier 1: HyperLogLog over a 16 M-key sample, then the uniform model d = G (1 - exp(-m / G)) solved for G
    {
        const int64_t m = sizes[1];
        unsigned int* regs = (unsigned int*)pool_alloc(HLL_M * 4);
        if (!regs) return 1;
        VNM_HIP(hipMemsetAsync(regs, 0, HLL_M * 4, s));
        int grid = (int)std::min<int64_t>((m + 1023) / 1024, (int64_t)device_info().num_cus);
        agg_hll_kernel<<<grid, 1024, 0, s>>>(kp, nrows, m, regs, h->kn_valid, h->kn_off);
        VNM_HIP(hipGetLastError());
        std::vector<unsigned int> hr(HLL_M);
        VNM_HIP(hipMemcpyAsync(hr.data(), regs, HLL_M * 4, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        pool_free(regs);
        double sum = 0;
        int zeros = 0;
        for (int i = 0; i < HLL_M; i++) { sum += ldexp(1.0, -(int)hr[i]); zeros += hr[i] == 0; }
        const double alpha = 0.7213 / (1.0 + 1.079 / HLL_M);
        double d = alpha * (double)HLL_M * (double)HLL_M / sum;
        if (d <= 2.5 * HLL_M && zeros) d = (double)HLL_M * log((double)HLL_M / zeros);  // linear counting
        if (d > (double)m) d = (double)m;
        d -= (double)heavy_keys;
        if (d < 1) d = 1;
        const double mm = (double)m * (1.0 - heavy_share);   // the rows of the sample that are not a heavy key's
        const double frac = std::min(1.0, d / mm);
        // solve d/m = (1 - exp(-x)) / x for x = m / G by bisection (x -> 1 / frac when the sample saw every group many times:
        // the upper bound must cover m / d, a bound of 64 turned G = 1e5 into an estimate of 3.1e5 and a second partition level)
        double lo = 1e-9, hi = 2.0 / frac + 64.0;
        for (int it = 0; it < 80; it++) {
            double x = 0.5 * (lo + hi);
            double f = (1.0 - exp(-x)) / x;
            if (f > frac) lo = x; else hi = x;
        }
        double G = mm / (0.5 * (lo + hi));
        if (frac > 0.97) G = mm * 30.0;  // beyond the resolution of the sample: at least this many
        G += (double)heavy_keys;
        if (G > (double)nrows) G = (double)nrows;
        *est = (int64_t)(G * 1.2) + 1;
    }
    return 0;
}

// Spilled wide entries [n][E] -> plain columns (key, the input columns at their own widths, validity bitmaps for the
// nullable ones), so that the general scan takes them like any batch.
struct UnzipArgs {
    const uint64_t* ent;
    int64_t n;
    int E, nval, has_vmask;
    uint64_t* key;
    void* vals[6];
    int widths[6];
    unsigned long long* valid[6];   // nullptr: the column had no bitmap
};
// The two spill lists of the dense path over a nullable value column -> columns: rows [0, n_ent) are the (key, value) entries,
// rows [n_ent, n_ent + n_null) the keys whose value is NULL; `valid` = the value column's validity bitmap (64 rows per word).
__global__ __launch_bounds__(256) void dense_vn_unzip_kernel(const ulonglong2* ent, int64_t n_ent, const uint64_t* nkeys, int64_t n_null,
                                                             uint64_t* key, uint64_t* val, unsigned long long* valid) {
    const int64_t n = n_ent + n_null;
    const int64_t n64 = (n + 63) & ~63LL;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n64; i += (int64_t)gridDim.x * 256) {
        bool ok = false;
        if (i < n_ent) { const ulonglong2 e = ent[i]; key[i] = e.x; val[i] = e.y; ok = true; }
        else if (i < n) { key[i] = nkeys[i - n_ent]; val[i] = 0; }
        const unsigned long long b = __ballot(ok);
        if ((threadIdx.x & 63) == 0) valid[i >> 6] = b;
    }
}

__global__ __launch_bounds__(256) void spill_unzip_kernel(UnzipArgs u) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t n64 = (u.n + 63) / 64 * 64;   // whole waves: the ballots below cover 64 consecutive entries
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n64; i += stride) {
        const bool in = i < u.n;
        const uint64_t* e = u.ent + (in ? i : u.n - 1) * u.E;
        if (in) u.key[i] = e[0];
        const uint64_t vmask = u.has_vmask ? e[u.E - 1] : ~0ULL;
        for (int c = 0; c < u.nval; c++) {
            const uint64_t raw = e[1 + c];
            if (in) {
                switch (u.widths[c]) {
                    case 1: ((uint8_t*)u.vals[c])[i] = (uint8_t)raw; break;
                    case 2: ((uint16_t*)u.vals[c])[i] = (uint16_t)raw; break;
                    case 4: ((uint32_t*)u.vals[c])[i] = (uint32_t)raw; break;
                    default: ((uint64_t*)u.vals[c])[i] = raw; break;
                }
            }
            if (u.valid[c]) {
                const unsigned long long b = __ballot(in && ((vmask >> c) & 1ULL));
                if ((threadIdx.x & 63) == 0) u.valid[c][i >> 6] = b;
            }
        }
    }
}

}  // namespace
static int merge_run_into_table(vnm_agg* h, hipStream_t s);
static int flush_scan_pending(vnm_agg* h, hipStream_t s);
#include "vnm_agg_routes.inc"

// fold a pending run into the HBM table (needed as soon as a second source of groups shows up)
static int merge_run_into_table(vnm_agg* h, hipStream_t s) {
    if (!h->have_run) return 0;
    uint64_t* kw[2] = {h->run_key, h->run_key + h->run_stride};
    uint64_t* aw[AGG_MAX_WORDS];
    for (int w = 0; w < h->plan.n_words; w++) aw[w] = h->run_acc + (size_t)w * h->run_stride;
    const int64_t n = h->run_n;
    h->have_run = false;  // vnm_agg_merge_device must not recurse into us
    int rc = vnm_agg_merge_device(h, n, kw, aw, (void*)s);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_error("merge_run_into_table: stream sync failed");
    h->have_run = true;
    drop_run(h);
    return rc;
}


// The table of a stream of small-range batches (DScanPending) -> a run.  Whatever the handle holds as a run already goes to the HBM
// table first (one run at a time).
static int flush_scan_pending(vnm_agg* h, hipStream_t s) {
    DScanPending* sp = h->scan_pending;
    if (!sp) return 0;
    h->scan_pending = nullptr;
    std::unique_ptr<DScanPending> own(sp);
    if (h->pending) VNM_TRY(complete_pending(h, s, DF_RUN, nullptr, nullptr));
    if (h->have_run) VNM_TRY(merge_run_into_table(h, s));
    const int64_t dstride = sp->slots + 2;
    PoolScope pool;
    uint64_t* rk = (uint64_t*)pool.take((size_t)dstride * 8 * 2);
    uint64_t* ra = (uint64_t*)pool.take((size_t)dstride * 8 * std::max(1, h->plan.n_words));
    if (!rk || !ra) return 1;
    VNM_HIP(hipMemsetAsync(sp->flags, 0, 64, s));
    DFinalArgs df = sp->df;
    df.dkey = rk; df.dacc = ra; df.dstride = dstride; df.flags = sp->flags;
    dscan_emit_kernel<<<sp->slots / 512, 512, 0, s>>>(df, sp->slots, sp->t);
    VNM_HIP(hipGetLastError());
    unsigned long long fl[2];
    VNM_HIP(hipMemcpyAsync(fl, sp->flags, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (fl[0]) return set_error("aggregate: the stream table holds more groups than slots (internal error)");
    pool.keep(rk); pool.keep(ra);
    adopt_run(h, rk, ra, dstride, (int64_t)fl[1]);
    return 0;
}

// see run_patch_kernel; *done = false leaves everything as it was (the caller merges the run into the table instead)
static int merge_table_into_run(vnm_agg* h, hipStream_t s, bool* done) {
    *done = false;
    if (!h->have_run || !h->have_table || !h->single || h->plan.n_keys != 1 || h->g.kwt != 0 || getenv("VNM_AGG_NO_RUN_PATCH") != nullptr) return 0;
    unsigned long long fill = 0;
    VNM_HIP(hipMemcpyAsync(&fill, h->g.ctl + 2, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    const int64_t tmax = (int64_t)fill + 2;   // + the two special groups
    if (tmax * env_i64("VNM_RUN_PATCH_RATIO", 8) > h->run_n || h->run_n + tmax > h->run_stride - 2) return 0;
    PoolScope pool;
    const size_t fbytes = ((size_t)h->g.cap + 2 + 15) / 8 * 8;
    uint8_t* found = (uint8_t*)pool.take(fbytes + 8);
    if (!found) return 1;
    VNM_HIP(hipMemsetAsync(found, 0, fbytes + 8, s));
    PatchArgs a{};
    a.plan = h->plan; a.g = h->g;
    a.rkey = h->run_key; a.racc = h->run_acc; a.rn = h->run_n; a.rstride = h->run_stride;
    a.found = found;
    a.appended = (unsigned long long*)(found + fbytes);
    a.bloom = (uint32_t*)pool.take(PATCH_BLOOM_BITS / 8);
    if (!a.bloom) return 1;
    VNM_HIP(hipMemsetAsync(a.bloom, 0, PATCH_BLOOM_BITS / 8, s));
    const int cus = device_info().num_cus;
    run_patch_bloom_kernel<<<(int)std::min<int64_t>(((int64_t)h->g.cap + 255) / 256, (int64_t)cus * 8), 256, 0, s>>>(a);
    run_patch_kernel<<<(int)std::min<int64_t>((h->run_n + 1023) / 1024, (int64_t)cus * 2), 1024, 0, s>>>(a);
    run_patch_append_kernel<<<(int)std::min<int64_t>(((int64_t)h->g.cap + 2 + 255) / 256, (int64_t)cus * 8), 256, 0, s>>>(a);
    VNM_HIP(hipGetLastError());
    unsigned long long appended = 0;
    VNM_HIP(hipMemcpyAsync(&appended, a.appended, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if ((int64_t)appended > tmax) return set_error("aggregate: more table groups than the table's fill count (internal error)");
    h->run_n += (int64_t)appended;
    if (appended) {   // the partition directory no longer describes the whole run
        pool_free(h->run_dir);
        h->run_dir = nullptr;
        h->run_nfin = 0;
    }
    table_free(&h->g);
    h->have_table = false;
    *done = true;
    return 0;
}

#include "vnm_agg_fxn.inc"
#include "vnm_agg_multikey.inc"

#include "vnm_agg_exact.inc"

extern "C" {

vnm_agg* vnm_agg_create(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                        const int* in_types, const int* in_flags, const int* in_col_ids) {
    int wide_type = -1;
    if (kind == VNM_SINGLE_NUMERICAL && n_keys == 1 && key_types && getenv("VNM_AGG_NO_WIDEN_KEYS") == nullptr) {
        const int t = key_types[0];
        if (t == VNM_I8 || t == VNM_I16 || t == VNM_I32) wide_type = VNM_I64;
        else if (t == VNM_U8 || t == VNM_U16 || t == VNM_U32) wide_type = VNM_U64;
    }
    // float32 input columns whose every function is a SUM / AVG / COUNT: declared float64 to the plan, widened on arrival
    std::vector<int> types2;
    bool widen_in[AGG_MAX_FUNCS] = {};
    bool any_widen = false;
    if (funcs && in_types && n_funcs > 0 && n_funcs <= AGG_MAX_FUNCS && getenv("VNM_AGG_NO_WIDEN_INPUTS") == nullptr) {
        types2.assign(in_types, in_types + n_funcs);
        for (int i = 0; i < n_funcs; i++) {
            if (in_types[i] != VNM_F32 || funcs[i] == VNM_COUNT_STAR) continue;
            bool ok = true;      // every function over the same column (same id; without ids: this function alone) must allow it
            bool sums = false;   // ... and one of them must be a SUM / AVG: a column that is only COUNTed is read for its validity alone
            for (int j = 0; j < n_funcs && ok; j++) {
                const bool same_col = in_col_ids ? (in_col_ids[j] >= 0 && in_col_ids[j] == in_col_ids[i]) : j == i;
                if (same_col && funcs[j] != VNM_SUM && funcs[j] != VNM_AVG && funcs[j] != VNM_COUNT) ok = false;
                if (same_col && in_types[j] != VNM_F32) ok = false;
                if (same_col && (funcs[j] == VNM_SUM || funcs[j] == VNM_AVG)) sums = true;
            }
            if (ok && sums) { widen_in[i] = true; types2[(size_t)i] = VNM_F64; any_widen = true; }
        }
    }
    vnm_agg* h = agg_create(kind, n_keys, wide_type >= 0 ? &wide_type : key_types, n_funcs, funcs, any_widen ? types2.data() : in_types, in_flags, in_col_ids);
    if (h && wide_type >= 0) h->key_out_type = key_types[0];
    if (h && any_widen) { memcpy(h->widen_in, widen_in, sizeof(widen_in)); h->any_widen_in = true; }
    if (h) exact_attach(h);
    return h;
}

namespace vnm {
// narrow integer key values -> 64-bit words, sign- or zero-extended; dst[i] belongs to row i (src index first + i)
__global__ __launch_bounds__(256) void widen_key_kernel(const void* src, int type, int64_t first, int64_t n, uint64_t* dst) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t k = first + i;
        uint64_t v;
        switch (type) {
            case VNM_I8: v = (uint64_t)(int64_t)((const int8_t*)src)[k]; break;
            case VNM_I16: v = (uint64_t)(int64_t)((const int16_t*)src)[k]; break;
            case VNM_I32: v = (uint64_t)(int64_t)((const int32_t*)src)[k]; break;
            case VNM_U8: v = ((const uint8_t*)src)[k]; break;
            case VNM_U16: v = ((const uint16_t*)src)[k]; break;
            default: v = ((const uint32_t*)src)[k]; break;
        }
        dst[i] = v;
    }
}
// float32 values -> float64 (exact); dst[i] belongs to row i (src index first + i)
__global__ __launch_bounds__(256) void widen_f32_kernel(const float* src, int64_t first, int64_t n, double* dst) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = (double)src[first + i];
}
}  // namespace vnm

// the float32 input columns of this call that the plan took as float64 (vnm_agg_create): `win` = the inputs with those columns replaced
// by widened copies (one per distinct column); a predicate column that IS one of them follows, and the literal is rounded to float32 once
static int widen_inputs(vnm_agg* h, int64_t nrows, const vnm_dcol** inputs, vnm_dcol* win, const vnm_dcol** pred, vnm_dcol* wpred, hipStream_t s) {
    if (!h->any_widen_in || !*inputs) return 0;
    const vnm_dcol* in = *inputs;
    for (int i = 0; i < h->n_funcs; i++) win[i] = in[i];
    for (int i = 0; i < h->n_funcs; i++) {
        if (!h->widen_in[i]) continue;
        if (in[i].type != VNM_F32) return set_error("vnm_agg_next_device: input %d was declared float32, the batch brings type %d", i, in[i].type);
        int prev = -1;
        for (int j = 0; j < i && prev < 0; j++)
            if (h->widen_in[j] && in[j].values == in[i].values && in[j].offset == in[i].offset && in[j].validity == in[i].validity) prev = j;
        if (prev >= 0) { win[i] = win[prev]; continue; }
        win[i].type = VNM_F64;
        if (nrows > 0) {
            const int64_t off = in[i].validity ? (in[i].offset & 7) : 0;
            double* buf = (double*)pool_alloc((size_t)(off + nrows) * 8);
            if (!buf) return 1;
            h->widened.push_back({h->cur_seq, buf});
            if (off) VNM_HIP(hipMemsetAsync(buf, 0, (size_t)off * 8, s));
            const int grid = (int)std::min<int64_t>((nrows + 255) / 256, (int64_t)device_info().num_cus * 16);
            widen_f32_kernel<<<grid, 256, 0, s>>>((const float*)in[i].values, in[i].offset, nrows, buf + off);
            VNM_HIP(hipGetLastError());
            win[i].values = buf;
            win[i].validity = in[i].validity ? in[i].validity + (in[i].offset >> 3) : nullptr;
            win[i].offset = off;
            win[i].length = nrows;
        }
    }
    bool pred_widened = false;
    if (*pred && (*pred)->type == VNM_F32) {
        for (int i = 0; i < h->n_funcs; i++) {
            if (!h->widen_in[i] || in[i].values != (*pred)->values || in[i].offset != (*pred)->offset || in[i].validity != (*pred)->validity) continue;
            *wpred = win[i];
            *pred = wpred;
            pred_widened = true;
            break;
        }
    }
    // The EFFECTIVE literal of this batch: the caller's literal rounded to float32 when the predicate column is a float32 column
    // that travels widened (NumPy compares float32 against the literal in float32), the caller's own literal otherwise -- a later batch
    // whose predicate column is not widened gets it back -- and the suffix operator of an ordered MIN / MAX stream (fed the widened
    // column) compares with the same number as this handle.
    if (h->pred_set) {
        if (pred_widened) {
            const double lit = h->pred_user_is_float ? h->pred_user_dval : (double)h->pred_user_ival;
            h->pred_dval = (double)(float)lit;
            h->pred_is_float = 1;
            h->pred_lit_rounded = true;
        } else if (h->pred_lit_rounded) {
            h->pred_dval = h->pred_user_dval; h->pred_is_float = h->pred_user_is_float; h->pred_ival = h->pred_user_ival;
            h->pred_lit_rounded = false;
        }
        if (h->ex && h->ex->post) { h->ex->post->pred_dval = h->pred_dval; h->ex->post->pred_is_float = h->pred_is_float; h->ex->post->pred_ival = h->pred_ival; }
    }
    *inputs = win;
    return 0;
}

// the key column of this call as the operator's kernels want it: *keys stays, or becomes `wide` (values in a pool block the handle keeps
// until no recorded batch needs it)
static int widen_key(vnm_agg* h, int64_t nrows, const vnm_dcol** keys, vnm_dcol* wide, hipStream_t s) {
    if (h->key_out_type < 0 || !*keys) return 0;
    const vnm_dcol& k = (*keys)[0];
    if (k.type != h->key_out_type) return set_error("vnm_agg_next_device: key 0 changed type between batches");
    *wide = k;
    wide->type = h->plan.key_types[0];
    if (nrows > 0) {
        // the validity bitmap keeps its bit offset modulo 8 (the column's offset addresses values and validity alike)
        const int64_t off = k.validity ? (k.offset & 7) : 0;
        uint64_t* buf = (uint64_t*)pool_alloc((size_t)(off + nrows) * 8);
        if (!buf) return 1;
        h->widened.push_back({h->cur_seq, buf});
        if (off) VNM_HIP(hipMemsetAsync(buf, 0, (size_t)off * 8, s));
        const int grid = (int)std::min<int64_t>((nrows + 255) / 256, (int64_t)device_info().num_cus * 16);
        widen_key_kernel<<<grid, 256, 0, s>>>(k.values, k.type, k.offset, nrows, buf + off);
        VNM_HIP(hipGetLastError());
        wide->values = buf;
        wide->validity = k.validity ? k.validity + (k.offset >> 3) : nullptr;
        wide->offset = off;
        wide->length = nrows;
    }
    *keys = wide;
    return 0;
}
static void waiting_of(const vnm_agg* h, int64_t* batches, int64_t* rows, int64_t* oldest);
// widened key buffers no recorded batch needs any more go back to the pool -- behind an event on the stream whose kernels read them
// (pool_free_after: the pool is shared with other streams and threads; `synced`: the stream has just been synchronised)
static void release_widened(vnm_agg* h, void* stream, bool synced = false) {
    if (h->widened.empty()) return;
    int64_t b = 0, r = 0, o = -1;
    waiting_of(h, &b, &r, &o);
    size_t keep = 0;
    for (size_t i = 0; i < h->widened.size(); i++) {
        if (b > 0 && o >= 0 && h->widened[i].first >= o) h->widened[keep++] = h->widened[i];
        else if (synced) pool_free(h->widened[i].second);
        else pool_free_after(h->widened[i].second, as_stream(stream));
    }
    h->widened.resize(keep);
}

void vnm_agg_destroy(vnm_agg* h) {
    if (!h) return;
    if (h->ex) { exact_drop_result(h); exact_destroy(h->ex); h->ex = nullptr; }   // (a merged result's arrays go with their owner)
    if (h->inner) { vnm_agg_destroy(h->inner); h->inner = nullptr; }
    drop_parts(h);
    leave_tuple_mode(h);
    free_pack_tables(h);
    if (h->have_table) table_free(&h->g);
    invalidate_result(h);
    drop_run(h);
    delete h->pending;
    delete h->scan_pending;
    for (auto& w : h->widened) pool_free(w.second);
    delete h;
}

int vnm_agg_set_predicate(vnm_agg* h, int enabled, int op, int scalar_is_float, double dval, int64_t ival) {
    if (!h) return set_error("vnm_agg_set_predicate: null handle");
    if (enabled && (op < VNM_EQ || op > VNM_LE)) return set_error("vnm_agg_set_predicate: bad comparison op %d", op);
    // (a literal that was rounded to float32 for a widened float32 predicate column: the caller's own values are compared)
    const int cur_is_float = h->pred_lit_rounded ? h->pred_user_is_float : h->pred_is_float;
    const double cur_dval = h->pred_lit_rounded ? h->pred_user_dval : h->pred_dval;
    const int64_t cur_ival = h->pred_lit_rounded ? h->pred_user_ival : h->pred_ival;
    const bool same = h->pred_set == (enabled != 0) && (!enabled || (h->pred_op == op && cur_is_float == scalar_is_float && cur_ival == ival &&
                                                                     memcmp(&cur_dval, &dval, 8) == 0));
    if (same) return 0;
    // the waiting batches of an asynchronous stream were recorded under the OLD predicate (and without a predicate column when none was set)
    if (!h->q.empty()) return set_error("vnm_agg_set_predicate: batches are waiting (call vnm_agg_sync first)");
    for (vnm_agg* c : h->parts) if (!c->q.empty()) return set_error("vnm_agg_set_predicate: batches are waiting (call vnm_agg_sync first)");
    h->pred_set = enabled != 0;
    h->pred_op = op;
    h->pred_is_float = scalar_is_float;
    h->pred_dval = dval;
    h->pred_ival = ival;
    h->pred_lit_rounded = false;
    h->pred_user_is_float = scalar_is_float; h->pred_user_dval = dval; h->pred_user_ival = ival;
    if (h->ex && h->ex->post) VNM_TRY(vnm_agg_set_predicate(h->ex->post, enabled, op, scalar_is_float, dval, ival));
    return 0;
}

int vnm_agg_set_exchange_mode(vnm_agg* h, int rank_aligned) {
    if (!h) return set_error("vnm_agg_set_exchange_mode: null handle");
    h->rank_aligned = rank_aligned != 0;
    return 0;
}

int vnm_agg_set_hint(vnm_agg* h, int64_t expected_groups) {
    if (!h) return set_error("vnm_agg_set_hint: null handle");
    h->hint = expected_groups;
    if (h->ex && h->ex->post) h->ex->post->hint = expected_groups;
    return 0;
}

int vnm_agg_estimate_groups(vnm_agg* h, int64_t nrows, const vnm_dcol* key, int64_t* estimate, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !key || !estimate) return set_error("vnm_agg_estimate_groups: null argument");
    *estimate = 0;
    if (nrows <= 0 || type_width(key->type) != 8 || key->validity || (key->offset & 1)) return 0;   // the estimator reads plain 8-byte keys
    int64_t est = 0;
    VNM_TRY(estimate_groups(h, *key, nrows, &est, as_stream(stream)));
    *estimate = est;
    return 0;
}

}  // extern "C"
// the batch router: Batch / BatchShape / SpillState, the stage functions and next_device_impl, the driver over them
#include "vnm_agg_next.inc"
extern "C" {

// The waiting batches of an asynchronous stream (vnm_agg_set_async) -> the device: as the segments of ONE logical batch where the
// path's kernels take segments (the dense-key path's ring scatter, the hot-shape LDS scan), one by one otherwise.
static int flush_queue(vnm_agg* h, void* stream) {
    if (h->q.empty()) return 0;
    std::vector<vnm_agg::QBatch> q;
    q.swap(h->q);
    const int64_t total = h->q_rows;
    h->q_rows = 0;
    int rc = VNM_RC_SINGLY;
    auto one = [&](const vnm_agg::QBatch& b, int64_t n) {
        vnm_dcol in[AGG_MAX_FUNCS];
        for (int i = 0; i < h->n_funcs; i++) {
            memset(&in[i], 0, sizeof(vnm_dcol));
            if (!b.ins.empty()) in[i] = b.ins[i];
            else if (h->func_col[i] >= 0) in[i] = b.col;
        }
        const int64_t save = h->cur_seq;
        h->cur_seq = b.seq;     // (whoever records the batch again -- the parts of a split program -- keeps its number)
        const int rc1 = next_device_impl(h, n, &b.key, in, h->pred_set ? &b.pred : nullptr, stream);
        h->cur_seq = save;
        return rc1;
    };
    if (q.size() > 1 && getenv("VNM_AGG_NO_SEGMENTS") == nullptr) {
        h->segs_active = &q;
        rc = one(q[0], total);
        h->segs_active = nullptr;
        if (rc != VNM_RC_SINGLY) route_note("stream:segments_of_one_launch", "%zu recorded batches, %lld rows", q.size(), (long long)total);
    }
    if (rc == VNM_RC_SINGLY) {
        if (q.size() > 1) route_note("stream:batches_singly", "%zu recorded batches (the path's kernels read one batch)", q.size());
        rc = 0;
        for (size_t i = 0; i < q.size() && !rc; i++) rc = one(q[i], q[i].nrows);
    }
    return rc;
}

// does this batch have the shape whose kernels take stream segments (VSeg)?  The hot shape: one plain 8-byte key, {COUNT(*), COUNT,
// SUM, AVG} of ONE plain float64 column, a plain float64 predicate column or none.
static bool queueable(const vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, bool* pred_is_v, bool* multi) {
    *multi = false;
    if (!h->single || h->plan.n_keys != 1 || h->plan.n_cols < 1 || h->inner || h->tuple_mode || h->expr_col >= 0) return false;
    if (nrows <= 0 || nrows >= (1LL << 30)) return false;
    if (h->plan.n_cols > 1) {
        // SEVERAL plain 8-byte input columns over a plain int64 / uint64 key (round 4): the batches wait so that the path is chosen from
        // the stream's total row count (a 2^24-row batch alone is too short for a 2^27-code range: three columns, G = 1e8, 30 batches:
        // 315 ms through the hash partitions); when they go to the device the program is cut into parts (next_parts), which record
        // the batches in turn and launch once each -- or they go one by one, as before, where no part rule applies
        if (h->rank_aligned || !plain8_aligned(keys[0]) || keys[0].type != h->plan.key_types[0] || (keys[0].type != VNM_I64 && keys[0].type != VNM_U64)) return false;
        for (int i = 0; i < h->n_funcs; i++)
            if (h->func_col[i] >= 0 && (!plain8_aligned(inputs[i]) || !is_8byte_numeric(inputs[i].type))) return false;
        if (h->pred_set && (!pred || !plain8_aligned(*pred) || pred->type != VNM_F64)) return false;
        *pred_is_v = false;
        *multi = true;
        return true;
    }
    if (!h->parts.empty()) return false;
    const vnm_dcol& col = inputs[h->col_first_func[0]];
    if (!plain8_aligned(keys[0]) || keys[0].type != h->plan.key_types[0] || !plain8_aligned(col) || col.type != VNM_F64) return false;
    for (int o = 0; o < h->plan.n_ops; o++) {
        const int k = h->plan.ops[o].kind;
        if (k != A_COUNT_ROWS && k != A_COUNT_VALID && k != A_SUM_F64) return false;
    }
    for (int i = 0; i < h->n_funcs; i++)   // every function reads that one column (COUNT(*): none)
        if (h->func_col[i] >= 0 && (!same_values(inputs[i], col) || inputs[i].validity)) return false;
    *pred_is_v = false;
    if (h->pred_set) {
        if (!pred || !plain8_aligned(*pred) || pred->type != VNM_F64) return false;
        *pred_is_v = same_values(*pred, col);
    }
    return true;
}

static int next_device_body(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, void* stream);

int vnm_agg_next_device(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs,
                        const vnm_dcol* pred, void* stream) {
    if (!h) return set_error("vnm_agg_next_device: null handle");
    if (!h->child) h->cur_seq = h->seq++;
    vnm_dcol wide, wpred;
    vnm_dcol win[AGG_MAX_FUNCS];
    if (h->key_out_type >= 0) { VNM_TRY(ensure_init()); VNM_TRY(widen_key(h, nrows, &keys, &wide, as_stream(stream))); }
    if (h->any_widen_in) { VNM_TRY(ensure_init()); VNM_TRY(widen_inputs(h, nrows, &inputs, win, &pred, &wpred, as_stream(stream))); }
    const int rc = next_device_body(h, nrows, keys, inputs, pred, stream);
    if (h->key_out_type >= 0 || h->any_widen_in) release_widened(h, stream);
    return rc;
}

static int next_device_body(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred, void* stream) {
    if (h->ex && inputs && (keys || h->plan.n_keys == 0)) {   // float MIN / MAX: the flag pass, and the ordered mode once the stream is unclean
        bool handled = false;
        VNM_TRY(exact_next(h, nrows, keys, inputs, pred, stream, &handled));
        if (handled) return 0;
    }
    if (h->async && keys && inputs) {
        bool piv = false, multi = false;
        if (queueable(h, nrows, keys, inputs, pred, &piv, &multi) && (h->q.empty() || (piv == h->q_pred_is_v && multi == h->q_multi))) {
            // (the first batch waits like any other: the estimates and the code range of the path are taken from the first SEGMENT
            // when the waiting batches are processed)
            if (h->q_rows + nrows > (1LL << 30) || h->q.size() >= 256) VNM_TRY(flush_queue(h, stream));
            vnm_agg::QBatch b{};
            b.seq = h->cur_seq;
            b.nrows = nrows; b.key = keys[0]; b.col = inputs[h->col_first_func[0]];
            if (multi) b.ins.assign(inputs, inputs + h->n_funcs);
            h->q_multi = multi;
            if (h->pred_set) b.pred = *pred;
            h->q.push_back(b);
            h->q_rows += nrows;
            h->q_pred_is_v = piv;
            invalidate_result(h);
            return 0;
        }
    }
    VNM_TRY(flush_queue(h, stream));
    return next_device_impl(h, nrows, keys, inputs, pred, stream);
}

int vnm_agg_set_async(vnm_agg* h, int enabled) {
    if (!h) return set_error("vnm_agg_set_async: null handle");
    if (!enabled && !h->q.empty()) return set_error("vnm_agg_set_async: batches are waiting (call vnm_agg_sync first)");
    for (vnm_agg* c : h->parts) VNM_TRY(vnm_agg_set_async(c, enabled));
    if (h->ex && h->ex->post) VNM_TRY(vnm_agg_set_async(h->ex->post, enabled));
    h->async = enabled != 0;
    return 0;
}

int vnm_agg_sync(vnm_agg* h, void* stream) {
    if (!h) return set_error("vnm_agg_sync: null handle");
    VNM_TRY(flush_queue(h, stream));
    for (vnm_agg* c : h->parts) VNM_TRY(flush_queue(c, stream));   // (the parts of a split program record their batches themselves)
    if (h->ex && h->ex->post) VNM_TRY(vnm_agg_sync(h->ex->post, stream));
    VNM_HIP(hipStreamSynchronize(as_stream(stream)));
    release_widened(h, stream, true);
    return 0;
}

// the recorded batches the handle (its parts, the suffix operator of an ordered MIN / MAX stream) still needs the buffers of
static void waiting_of(const vnm_agg* h, int64_t* batches, int64_t* rows, int64_t* oldest) {
    *batches += (int64_t)h->q.size();
    *rows += h->q_rows;
    for (const auto& b : h->q) if (*oldest < 0 || b.seq < *oldest) *oldest = b.seq;
    for (const vnm_agg* c : h->parts) waiting_of(c, batches, rows, oldest);
    if (h->ex && h->ex->post) waiting_of(h->ex->post, batches, rows, oldest);
}

int vnm_agg_waiting(vnm_agg* h, int64_t* batches, int64_t* rows, int64_t* oldest_seq, int64_t* last_seq) {
    if (!h) return set_error("vnm_agg_waiting: null handle");
    int64_t b = 0, r = 0, o = -1;
    waiting_of(h, &b, &r, &o);
    if (batches) *batches = b;     // (a batch the parts of a split program hold is counted once per part)
    if (rows) *rows = r;
    if (oldest_seq) *oldest_seq = o;
    if (last_seq) *last_seq = h->seq - 1;
    return 0;
}

// ---- expressions inside aggregates ---------------------------------------------------------------------------------------
int vnm_agg_set_input_expr(vnm_agg* h, int func_idx, int n_ins, const vnm_expr_ins* program, int n_cols) {
    if (!h || !program) return set_error("vnm_agg_set_input_expr: null argument");
    if (func_idx < 0 || func_idx >= h->n_funcs || h->func_col[func_idx] < 0) return set_error("vnm_agg_set_input_expr: function %d has no input column", func_idx);
    if (h->expr_col >= 0 && h->expr_col != h->func_col[func_idx]) return set_error("vnm_agg_set_input_expr: one expression input per operator (project the others first)");
    if (n_ins < 1 || n_ins > VNM_PROJECT_MAX_INS || n_cols < 1 || n_cols > VNM_PROJECT_MAX_COLS) return set_error("vnm_agg_set_input_expr: bad program size");
    if (h->c_in_types[func_idx] != VNM_F64 || h->widen_in[func_idx]) return set_error("vnm_agg_set_input_expr: declare the function's input type as float64 (the expression's result type)");
    h->expr_col = h->func_col[func_idx];
    h->expr_prog.assign(program, program + n_ins);
    h->expr_ncols = n_cols;
    // does it fit the in-register evaluator?
    bool ok = n_ins <= EXR_MAX_INS && n_cols <= EXR_MAX_COLS;
    int sp = 0;
    for (int i = 0; ok && i < n_ins; i++) {
        switch (program[i].op) {
            case VNM_EX_COL: ok = program[i].arg >= 0 && program[i].arg < n_cols && ++sp <= EXR_MAX_DEPTH; break;
            case VNM_EX_CONST_F: case VNM_EX_CONST_I: ok = ++sp <= EXR_MAX_DEPTH; break;
            case VNM_EX_NEG: ok = sp >= 1; break;
            case VNM_EX_ADD: case VNM_EX_SUB: case VNM_EX_MUL: case VNM_EX_DIV: ok = sp >= 2; sp--; break;
            default: ok = false; break;
        }
    }
    h->expr_fusable = ok && sp == 1;
    return 0;
}

int vnm_agg_next_device_expr(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred,
                             int n_expr_cols, const vnm_dcol* expr_cols, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || !expr_cols) return set_error("vnm_agg_next_device_expr: null argument");
    if (h->expr_col < 0) return set_error("vnm_agg_next_device_expr: call vnm_agg_set_input_expr first");
    if (n_expr_cols != h->expr_ncols) return set_error("vnm_agg_next_device_expr: the expression reads %d columns, %d given", h->expr_ncols, n_expr_cols);
    hipStream_t s = as_stream(stream);
    std::vector<vnm_dcol> in(inputs, inputs + h->n_funcs);
    // fused: the hot shape -- {COUNT(*), COUNT, SUM, AVG} of the expression alone, a plain 8-byte key (or no GROUP BY),
    // float64 columns without NULLs at even offsets, float64 predicate column or none
    bool fuse = h->expr_fusable && h->plan.n_cols == 1 && getenv("VNM_AGG_NO_HOT") == nullptr && getenv("VNM_AGG_NO_EXPR_FUSION") == nullptr &&
                nrows > 0 && (h->plan.n_keys == 0 || (h->single && h->plan.n_keys == 1 && type_width(keys[0].type) == 8 && !keys[0].validity && (keys[0].offset & 1) == 0));
    for (int o = 0; fuse && o < h->plan.n_ops; o++) {
        const int k = h->plan.ops[o].kind;
        fuse = k == A_COUNT_ROWS || k == A_COUNT_VALID || k == A_SUM_F64;
    }
    for (int c = 0; fuse && c < n_expr_cols; c++)
        fuse = expr_cols[c].type == VNM_F64 && !expr_cols[c].validity && (expr_cols[c].offset & 1) == 0 && expr_cols[c].length >= nrows;
    if (fuse && h->pred_set) fuse = pred && pred->type == VNM_F64 && !pred->validity && (pred->offset & 1) == 0;
    if (fuse) {
        ExprProg& e = h->expr_dev;
        e.n = (int)h->expr_prog.size();
        for (int c = 0; c < EXR_MAX_COLS; c++) e.cols[c] = c < n_expr_cols ? (const double*)expr_cols[c].values + expr_cols[c].offset : nullptr;
        for (int i = 0; i < e.n; i++) {
            const vnm_expr_ins& pi = h->expr_prog[i];
            e.ins[i].op = pi.op == VNM_EX_CONST_I ? VNM_EX_CONST_F : pi.op;
            e.ins[i].arg = pi.arg;
            e.ins[i].imm = pi.op == VNM_EX_CONST_I ? (double)pi.imm_i : pi.imm_f;
        }
        // a stand-in column view for the functions that read the expression: float64, no NULLs; its address is never
        // dereferenced (and equals no real column, so `predicate column == value column` cannot match by accident)
        vnm_dcol stand{};
        stand.values = (const void*)h; stand.type = VNM_F64; stand.length = nrows;
        for (int i = 0; i < h->n_funcs; i++) if (h->func_col[i] == h->expr_col) in[i] = stand;
        h->expr_active = true;
        const int rc = vnm_agg_next_device(h, nrows, keys, in.data(), pred, stream);
        h->expr_active = false;
        return rc;
    }
    // general case: one fused projection pass materialises the expression, the aggregate reads it like any column
    double* tmp = (double*)pool_alloc((size_t)(nrows > 0 ? nrows : 1) * 8);
    if (!tmp) return 1;
    int out_type = 0;
    int rc = vnm_project((int)h->expr_prog.size(), h->expr_prog.data(), n_expr_cols, expr_cols, nrows, tmp, &out_type, stream);
    if (!rc && out_type != VNM_F64) rc = set_error("vnm_agg_next_device_expr: the expression's result type is %d, float64 expected (cast in the projection)", out_type);
    if (!rc) {
        vnm_dcol col{};
        col.values = tmp; col.type = VNM_F64; col.length = nrows;
        for (int i = 0; i < h->n_funcs; i++) if (h->func_col[i] == h->expr_col) in[i] = col;
        rc = vnm_agg_next_device(h, nrows, keys, in.data(), pred, stream);
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = set_error("vnm_agg_next_device_expr: stream synchronisation failed");
    pool_free(tmp);
    return rc;
}

static int merge_device_impl(vnm_agg* h, int64_t n, uint64_t* const* key_words, uint64_t* const* acc_words, void* stream, int64_t blk_rows, const uint64_t* blk_base);

int vnm_agg_merge_device(vnm_agg* h, int64_t n, uint64_t* const* key_words, uint64_t* const* acc_words, void* stream) {
    return merge_device_impl(h, n, key_words, acc_words, stream, 0, nullptr);
}

static int merge_device_impl(vnm_agg* h, int64_t n, uint64_t* const* key_words, uint64_t* const* acc_words, void* stream, int64_t blk_rows, const uint64_t* blk_base) {
    VNM_TRY(ensure_init());
    if (!h) return set_error("vnm_agg_merge_device: null handle");
    hipStream_t s = as_stream(stream);
    VNM_TRY(flush_queue(h, stream));
    if (h->inner) VNM_TRY(demote_packed(h, s));
    VNM_TRY(collapse_parts(h, s));
    invalidate_result(h);
    VNM_TRY(ensure_table(h, n, s));
    if (n <= 0) return 0;
    if (h->plan.n_keys) {
        unsigned long long fill = 0;
        VNM_HIP(hipMemcpyAsync(&fill, h->g.ctl + 2, 8, hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        uint64_t need = pow2_at_least((uint64_t)((fill + (uint64_t)n) * 10 / 7 + 16));
        if (need > h->g.cap) VNM_TRY(table_grow(h, need, s));
    }
    MergeArgs m{};
    m.plan = h->plan;
    m.g = h->g;
    m.n = n;
    m.src_stride = h->merge_stride > 0 ? h->merge_stride : 1;
    m.blk_rows = blk_rows; m.blk_base = blk_base;
    for (int j = 0; j < h->plan.kw; j++) m.src_key[j] = key_words[j];
    for (int w = 0; w < h->plan.n_words; w++) m.src_acc[w] = acc_words[w];
    int grid = device_info().num_cus * 8;
    int64_t need_blocks = (n + 255) / 256;
    if (grid > need_blocks) grid = (int)need_blocks;
    agg_merge_kernel<<<grid, 256, 0, s>>>(m);
    VNM_HIP(hipGetLastError());
    return 0;
}

// merge row-major partial groups [n][n_key_words + n_acc_words] (what vnm_agg_bucket_by_owner produces and the
// all_to_all delivers) into this handle
int vnm_agg_merge_rows(vnm_agg* h, int64_t n, const uint64_t* rows, void* stream) {
    if (!h) return set_error("vnm_agg_merge_rows: null handle");
    const int nw = h->plan.kw + h->plan.n_words;
    uint64_t* kw[AGG_MAX_KEYS + 1];
    uint64_t* aw[AGG_MAX_WORDS];
    for (int j = 0; j < h->plan.kw; j++) kw[j] = const_cast<uint64_t*>(rows) + j;
    for (int w = 0; w < h->plan.n_words; w++) aw[w] = const_cast<uint64_t*>(rows) + h->plan.kw + w;
    h->merge_stride = nw;
    int rc = vnm_agg_merge_device(h, n, kw, aw, stream);
    h->merge_stride = 0;
    return rc;
}

// `nblocks` blocks of (block_rows + 1) row-major rows [n_key_words + n_acc_words]; row 0 of a block is its header (word 0 = the number of
// partial groups in rows 1 ..): the receive buffer of distributed.exchange_small_fixed, merged without a host look at the counts
int vnm_agg_merge_row_blocks(vnm_agg* h, int nblocks, int64_t block_rows, const uint64_t* blocks, void* stream) {
    if (!h || nblocks < 1 || block_rows < 1 || !blocks) return set_error("vnm_agg_merge_row_blocks: bad argument");
    const int nw = h->plan.kw + h->plan.n_words;
    uint64_t* kw[AGG_MAX_KEYS + 1];
    uint64_t* aw[AGG_MAX_WORDS];
    for (int j = 0; j < h->plan.kw; j++) kw[j] = const_cast<uint64_t*>(blocks) + j;
    for (int w = 0; w < h->plan.n_words; w++) aw[w] = const_cast<uint64_t*>(blocks) + h->plan.kw + w;
    h->merge_stride = nw;
    const int rc = merge_device_impl(h, (int64_t)nblocks * block_rows, kw, aw, stream, block_rows, blocks);
    h->merge_stride = 0;
    return rc;
}

int vnm_agg_finish(vnm_agg* h, int64_t* n_groups, void* stream) {
    VNM_TRY(ensure_init());
    if (!h) return set_error("vnm_agg_finish: null handle");
    const int rc = h->ex && h->ex->switched ? exact_finish(h, n_groups, stream)   // prefix + suffix merged, float MIN / MAX composed in row order
                                            : agg_finish_core(h, n_groups, stream);
    release_widened(h, stream);
    return rc;
}

static int agg_finish_core(vnm_agg* h, int64_t* n_groups, void* stream) {
    hipStream_t s = as_stream(stream);
    VNM_TRY(flush_queue(h, stream));   // (the waiting batches of an asynchronous stream)
    if (h->n_groups >= 0) {
        if (n_groups) *n_groups = h->n_groups;
        return 0;
    }
    if (h->inner) {  // packed composite keys: finish the single-key operator, unpack its keys into the wide layout
        int64_t n = 0;
        VNM_TRY(vnm_agg_finish(h->inner, &n, stream));
        h->dstride = n + 2;
        h->dkey = (uint64_t*)pool_alloc((size_t)h->dstride * 8 * h->plan.kw);
        h->dacc = (uint64_t*)pool_alloc((size_t)h->dstride * 8 * h->plan.n_words);
        if (!h->dkey || !h->dacc) return 1;
        if (n > 0) {
            VNM_TRY(inner_keys(h, h->inner, n, h->dkey, h->dstride, s));
            for (int w = 0; w < h->plan.n_words; w++)
                VNM_HIP(hipMemcpyAsync(h->dacc + (size_t)w * h->dstride, h->inner->dacc + (size_t)w * h->inner->dstride, (size_t)n * 8,
                                       hipMemcpyDeviceToDevice, s));
            VNM_HIP(hipGetLastError());
            VNM_HIP(hipStreamSynchronize(s));
        }
        h->n_groups = n;
        if (n_groups) *n_groups = n;
        return 0;
    }
    VNM_TRY(flush_scan_pending(h, s));                 // a stream of small-range batches: its table, as a run
    VNM_TRY(collapse_parts(h, s));                     // a split program: its parts joined by key, as a run
    if (h->pending) VNM_TRY(complete_pending(h, s));   // the deferred final pass of the dense path, as a run
    if (h->have_run && h->have_table) {   // a big run + a few spilled groups in the table: fold the table into the run
        bool patched = false;
        VNM_TRY(merge_table_into_run(h, s, &patched));
    }
    if (h->have_run && !h->have_table) {  // the partitioned path already produced the dense result
        h->dkey = h->run_key; h->dacc = h->run_acc; h->dstride = h->run_stride; h->n_groups = h->run_n;
        h->result_is_run = true;
        if (n_groups) *n_groups = h->n_groups;
        return 0;
    }
    if (h->have_run) VNM_TRY(merge_run_into_table(h, s));
    if (!h->have_table) {
        if (h->plan.n_keys == 0) VNM_TRY(ensure_table(h, 0, s));  // OneGroup over no batches still yields one row
        else {
            h->n_groups = 0;
            if (n_groups) *n_groups = 0;
            return 0;
        }
    }
    unsigned long long fill = 0;
    VNM_HIP(hipMemcpyAsync(&fill, h->g.ctl + 2, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    h->dstride = (int64_t)fill + 2;
    h->dkey = (uint64_t*)pool_alloc((size_t)h->dstride * 8 * (h->plan.kw ? h->plan.kw : 1));
    h->dacc = (uint64_t*)pool_alloc((size_t)h->dstride * 8 * h->plan.n_words);
    if (!h->dkey || !h->dacc) return 1;
    VNM_HIP(hipMemsetAsync(h->g.ctl + 3, 0, 8, s));
    CompactArgs c{};
    c.plan = h->plan;
    c.g = h->g;
    c.dkey = h->dkey;
    c.dacc = h->dacc;
    c.dstride = h->dstride;
    if (h->plan.n_keys) {
        int grid = device_info().num_cus * 8;
        int64_t need_blocks = ((int64_t)h->g.cap + 255) / 256;
        if (grid > need_blocks) grid = (int)need_blocks;
        agg_compact_kernel<<<grid, 256, 0, s>>>(c);
    }
    agg_compact_special_kernel<<<1, 64, 0, s>>>(c);
    VNM_HIP(hipGetLastError());
    unsigned long long cnt = 0;
    VNM_HIP(hipMemcpyAsync(&cnt, h->g.ctl + 3, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    h->n_groups = (int64_t)cnt;
    if (n_groups) *n_groups = h->n_groups;
    return 0;
}

// Multi-GPU exchange helper: writes the finished dense run as rows of (key words, accumulator words) grouped
// by owner rank (vinum_amd/distributed.py::owner_of) into out_rows [n_groups][n_key_words + n_acc_words] and
// the per-owner row counts into counts_host[world].
int vnm_agg_bucket_by_owner(vnm_agg* h, int world, uint64_t* out_rows, int64_t* counts_host, void* stream) {
    VNM_TRY(ensure_init());
    if (!h || world < 1 || world > 64 || !counts_host) return set_error("vnm_agg_bucket_by_owner: bad argument");
    hipStream_t s = as_stream(stream);
    int64_t n = 0;
    VNM_TRY(vnm_agg_finish(h, &n, stream));
    for (int o = 0; o < world; o++) counts_host[o] = 0;
    if (n == 0) return 0;
    BucketArgs b{};
    b.nkw = h->plan.kw;
    b.nw = h->plan.kw + h->plan.n_words;
    for (int j = 0; j < h->plan.kw; j++) b.words[j] = h->dkey + (size_t)j * h->dstride;
    for (int w = 0; w < h->plan.n_words; w++) b.words[h->plan.kw + w] = h->dacc + (size_t)w * h->dstride;
    b.n = n;
    b.world = world;
    b.out = out_rows;
    if (h->plan.kw == 0) {  // ONE_GROUP: a single row, owner 0
        for (int w = 0; w < h->plan.n_words; w++)
            VNM_HIP(hipMemcpyAsync(out_rows + w, h->dacc + (size_t)w * h->dstride, 8, hipMemcpyDeviceToDevice, s));
        VNM_HIP(hipStreamSynchronize(s));
        counts_host[0] = n;
        return 0;
    }
    b.nb = (int)std::min<int64_t>((n + 4095) / 4096, (int64_t)device_info().num_cus * 8);
    b.per = ((n + b.nb - 1) / b.nb + 255) / 256 * 256;
    unsigned long long* ctr = (unsigned long long*)pool_alloc(((size_t)world * b.nb + BK_MAX_WORLD) * 8);
    if (!ctr) return 1;
    b.blk = ctr;
    b.totals = ctr + (size_t)world * b.nb;
    agg_bucket_count_kernel<<<b.nb, 256, 0, s>>>(b);
    agg_bucket_scan_kernel<<<1, BK_MAX_WORLD, 0, s>>>(b);
    agg_bucket_scatter_kernel<<<b.nb, 256, 0, s>>>(b);
    VNM_HIP(hipGetLastError());
    unsigned long long tot[BK_MAX_WORLD];
    VNM_HIP(hipMemcpyAsync(tot, b.totals, sizeof(unsigned long long) * world, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    for (int o = 0; o < world; o++) counts_host[o] = (int64_t)tot[o];
    pool_free(ctr);
    return 0;
}

#include "vnm_agg_exchange.inc"

#include "vnm_agg_result.inc"

#include "vnm_agg_exchange2.inc"

}  // extern "C"
