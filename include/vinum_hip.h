/*
 * vinum_hip.h -- C ABI of libvinum_hip.so, the MI355X (gfx950) operator library behind Vinum's
 * native operator boundary.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / Arrow C Data Interface structs
 * and returns a status code (0 = ok; vnm_last_error() holds the message).  Nothing throws or aborts
 * across the ABI (the reference aborts on a bad handle, vinum/core/vinum_lib.cpp:62-63).
 * One handle = one HIP stream; handles are not thread-safe, distinct handles may be used from distinct
 * threads.  Device pointers are plain `void*` (hipMalloc / torch .data_ptr()).
 *
 * Each block cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef VINUM_HIP_H
#define VINUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Arrow C Data Interface (https://arrow.apache.org/docs/format/CDataInterface.html) ---------- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char* format;
    const char* name;
    const char* metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema** children;
    struct ArrowSchema* dictionary;
    void (*release)(struct ArrowSchema*);
    void* private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void** buffers;
    struct ArrowArray** children;
    struct ArrowArray* dictionary;
    void (*release)(struct ArrowArray*);
    void* private_data;
};
#endif

/* ---- Arrow C Stream Interface (https://arrow.apache.org/docs/format/CStreamInterface.html) ------ */
#ifndef ARROW_C_STREAM_INTERFACE
#define ARROW_C_STREAM_INTERFACE
struct ArrowArrayStream {
    int (*get_schema)(struct ArrowArrayStream*, struct ArrowSchema* out);
    int (*get_next)(struct ArrowArrayStream*, struct ArrowArray* out);
    const char* (*get_last_error)(struct ArrowArrayStream*);
    void (*release)(struct ArrowArrayStream*);
    void* private_data;
};
#endif

/* ---- enums ---------------------------------------------------------------------------------- */
/* physical column types; temporal Arrow types map to their storage integers */
enum vnm_type { VNM_I8 = 0, VNM_I16, VNM_I32, VNM_I64, VNM_U8, VNM_U16, VNM_U32, VNM_U64, VNM_F32, VNM_F64 };
/* replaces py::enum_<AggFuncType>  vinum/core/vinum_lib.cpp:25-32 (same order) */
enum vnm_agg_func { VNM_COUNT_STAR = 0, VNM_COUNT, VNM_MIN, VNM_MAX, VNM_SUM, VNM_AVG };
/* which operator class: vinum/core/aggregate.py:96-104 */
enum vnm_agg_kind { VNM_ONE_GROUP = 0, VNM_SINGLE_NUMERICAL = 1, VNM_MULTI_NUMERICAL = 2 };
/* replaces py::enum_<SortOrder>  vinum/core/vinum_lib.cpp:34-37 */
enum vnm_sort_order { VNM_ASC = 0, VNM_DESC = 1 };
/* comparison predicates: vinum/core/expressions.py:30-36 */
enum vnm_cmp_op { VNM_EQ = 0, VNM_NE, VNM_GT, VNM_GE, VNM_LT, VNM_LE };
/* arithmetic / bitwise expression opcodes: vinum/core/expressions.py:13-24 */
enum vnm_expr_op {
    VNM_EX_COL = 0,   /* push input column  (arg = column index)            */
    VNM_EX_CONST_F,   /* push float literal (imm_f)                          */
    VNM_EX_CONST_I,   /* push int literal   (imm_i)                          */
    VNM_EX_ADD, VNM_EX_SUB, VNM_EX_MUL, VNM_EX_DIV, VNM_EX_MOD,   /* np.add .. np.mod         */
    VNM_EX_NEG,                                                    /* np.negative              */
    VNM_EX_BAND, VNM_EX_BOR, VNM_EX_BXOR, VNM_EX_BNOT,             /* np.bitwise_* and ~x      */
    /* predicates (vinum/core/expressions.py:27-48): the result is a boolean mask */
    VNM_EX_EQ, VNM_EX_NE, VNM_EX_GT, VNM_EX_GE, VNM_EX_LT, VNM_EX_LE, /* NumPy comparison lambdas :30-36 */
    VNM_EX_AND, VNM_EX_OR, VNM_EX_NOT,                             /* pc.and_ / pc.or_ / pc.invert :27-29 */
    VNM_EX_IS_NULL, VNM_EX_IS_NOT_NULL,                            /* pc.is_null / pc.is_valid :37-38 (arg = column) */
    VNM_EX_STORE,     /* pop the top of the stack into output `arg` (vnm_project_multi: one SELECT list, one pass) */
    /* built-in scalar functions: _default_functions_registry, vinum/core/functions.py:353-387.  NumPy 2 ufunc typing:
     * sqrt and the transcendentals give float16 for (u)int8, float32 for (u)int16 and float32, float64 otherwise */
    VNM_EX_ABS,       /* 'abs': np.absolute  functions.py:362 (integers wrap: abs(int8 -128) == -128)          */
    VNM_EX_SQRT,      /* 'sqrt': np.sqrt     functions.py:363 (correctly rounded)                              */
    VNM_EX_SIN,       /* 'sin': np.sin       functions.py:365                                                  */
    VNM_EX_COS,       /* 'cos': np.cos       functions.py:364                                                  */
    VNM_EX_TAN,       /* 'tan': np.tan       functions.py:366                                                  */
    VNM_EX_LOG,       /* 'log': np.log       functions.py:368                                                  */
    VNM_EX_LOG2,      /* 'log2': np.log2     functions.py:369                                                  */
    VNM_EX_LOG10,     /* 'log10': np.log10   functions.py:370                                                  */
    VNM_EX_POW,       /* 'power': np.power   functions.py:367 (binary; integer ** negative integer: ValueError) */
    VNM_EX_TO_F64,    /* 'to_float': FloatCastFunction, np.array(x, dtype='float')  functions.py:172-176,355    */
    VNM_EX_TO_I64,    /* 'to_int': IntCastFunction, np.array(x, dtype='int')  functions.py:179-183,356 (NaN, inf and
                       * out-of-range floats give INT64_MIN, as on x86-64)                                           */
    VNM_EX_TO_BOOL,   /* 'to_bool': BoolCastFunction, np.array(x, dtype='bool') = x != 0  functions.py:165-169,354 */
    /* LIKE / NOT LIKE over a dictionary-coded string column: LikeFunction, functions.py:301-344.  Pushes table[code] as a
     * predicate value: arg = the int32 code column, imm_i = the index in `cols` of the table -- a VNM_U8 column of one byte
     * per dictionary id (vnm_strdict_like) whose length is the id count, not the batch length; it is read by this opcode only.
     * A NULL code, a negative code and a code past the table push 0 (NOT LIKE = NOT of it: true on NULL rows, as `!=`). */
    VNM_EX_LOOKUP_U8,
    /* A dictionary-coded string / binary column compared with ANOTHER such column (expressions.py:30-36 on the two value arrays).
     * Same operands as VNM_EX_LOOKUP_U8, the table a VNM_I32 column without NULLs (vnm_strdict_translate: the other dictionary's
     * code of each id; vnm_strdict_ranks_joint: the rank of each id in the union of both dictionaries).  Pushes table[code] as an
     * integer VALUE, NULL when the code is NULL, negative or past the table: a comparison with it is False on such rows, `!=`
     * True, like every comparison with a NULL operand.  Value 38; no earlier value moves. */
    VNM_EX_LOOKUP_I32
};
/* out_type of vnm_project when the expression is a predicate: out_values is a byte mask (1 byte per row) */
#define VNM_MASK_U8 100
/* out_type of vnm_project for a float16 result (sqrt / sin / ... of an 8-bit integer): 2 bytes per row.  float16 is a
 * result type only, never an input column type */
#define VNM_OUT_F16 101
/* column flags */
#define VNM_FLAG_SUM32 1 /* time32: SUM accumulates and wraps in int32 (agg_func_factory.cpp:132-137) */

/* ---- device column view ------------------------------------------------------------------------
 * The GPU counterpart of the reference's ArrayIter family (vinum_cpp/src/common/array_iterators.h:
 * 13-255): raw values buffer + optional validity bitmap + Arrow offset.  `values`/`validity` are
 * DEVICE pointers to the start of the Arrow buffers (not offset-adjusted). */
typedef struct vnm_dcol {
    const void* values;
    const uint8_t* validity; /* NULL = no nulls */
    int64_t offset;
    int64_t length;
    int32_t type;  /* enum vnm_type */
    int32_t flags; /* VNM_FLAG_* */
} vnm_dcol;

/* ---- library ------------------------------------------------------------------------------------ */
/* replaces vinum_lib.import_pyarrow() (vinum/core/vinum_lib.cpp:22-23): one-time init; selects the
 * HIP device.  Fails (non-zero) when no gfx950 device / HIP runtime is usable -- there is no CPU
 * fallback anywhere in this library. */
int vnm_init(int device_id);
const char* vnm_last_error(void);
int vnm_device_count(void);
/* host-side statistics of the last operator call (kernel launches, bytes staged, ...); debugging aid */
int vnm_device_synchronize(void);

/* kernel timing with HIP events on the launch stream (bench.py roofline leg): spans are named after the
 * kernel they bracket ("filter_kernel", "agg_scan", ...) */
int vnm_set_profiling(int on);
int vnm_profile_query(const char* name, double* total_ms, int64_t* count);
/* Which route of DESIGN.md section 4 the operators took, and why (round 5).  Every operator call that commits a batch to a path leaves
 * a note: a route name and the reason in numbers (estimates, ranges, thresholds).  vnm_route_counts: "route=count" lines for every
 * route taken since the library was loaded (or vnm_route_reset) into buf (cap bytes, zero terminated); returns the bytes the full
 * text needs.  vnm_route_last: the calling thread's last note, "route: reason".  VNM_AGG_TRACE=1 prints every note to stderr. */
int64_t vnm_route_counts(char* buf, int64_t cap);
int64_t vnm_route_last(char* buf, int64_t cap);
void vnm_route_reset(void);

/* ---- filter: FilterOperator._kernel + RecordBatch.filter -----------------------------------------
 * replaces vinum/core/algebra.py:119-123, vinum/arrow/record_batch.py:85-90 and the NumPy comparison
 * lambdas vinum/core/expressions.py:30-36 for the `column <op> literal` predicate shape, fused:
 * compare -> wave-ballot rank -> single-pass (decoupled look-back) compaction of every payload column.
 * NULL predicate inputs compare False (they reach NumPy as NaN, record_batch.py:112-118), `!=` True.
 *
 * pred:      predicate column;  scalar_is_float selects dval (Python float literal) or ival (int).
 * n_payload: columns to compact (the predicate column itself may be listed).
 * out_values[i]: device buffer of >= length * width(type_i) bytes.
 * out_valid[i]:  device byte-per-row validity (>= length bytes) or NULL when payload i has no validity.
 * out_count: host int64, rows kept.  stream: hipStream_t or NULL (default stream). */
int vnm_filter_cmp(const vnm_dcol* pred, int op, int scalar_is_float, double dval, int64_t ival,
                   int n_payload, const vnm_dcol* payload, void** out_values, uint8_t** out_valid,
                   int64_t* out_count, void* stream);
/* generic boolean mask (1 byte / row, optional byte validity -> emit_null) -> compaction */
int vnm_filter_mask(const uint8_t* mask, const uint8_t* mask_valid, int64_t length, int n_payload,
                    const vnm_dcol* payload, void** out_values, uint8_t** out_valid, int64_t* out_count,
                    void* stream);
/* byte-per-row validity (as written by the filter) -> Arrow validity bitmap of (n + 7) / 8 bytes */
int vnm_pack_validity(const uint8_t* valid_bytes, int64_t n, uint8_t* bitmap, void* stream);
/* bytes needed for the look-back scratch of a filter over `length` rows */
int64_t vnm_filter_scratch_bytes(int64_t length);

/* ---- hash aggregate ------------------------------------------------------------------------------
 * replaces  SingleNumericalHashAggregate / MultiNumericalHashAggregate / OneGroupAggregate
 *           (vinum/core/vinum_lib.cpp:54-124; vinum_cpp/src/operators/aggregate/).
 * Device level: keys / inputs are vnm_dcol views of HBM-resident columns. */
typedef struct vnm_agg vnm_agg;
struct vnm_expr_ins;   /* defined with the projection below */

/* in_col_ids (may be NULL): functions with equal NON-NEGATIVE ids read the same input column (they then share loads
 * and accumulators, e.g. SUM(v) and AVG(v)); a negative id means "a column of its own" (never shared); ignored for
 * COUNT(*).
 * Narrow columns (round 5): a SINGLE narrow integer key (int8 .. uint32) and float32 input columns whose functions are SUM / AVG / COUNT
 * only are widened to 64 bits inside vnm_agg_next_device (one extra pass, 12 B/row) and take the int64 / float64 kernels; the caller
 * declares and passes the columns as they are, result columns keep the declared key type (sums / averages of float32 are float64 in the
 * reference too: agg_func_factory.cpp:126-131, 206-211), and a predicate over a widened float32 column compares in float32 as NumPy does. */
vnm_agg* vnm_agg_create(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                        const int* in_types, const int* in_flags, const int* in_col_ids);
void vnm_agg_destroy(vnm_agg* h);
/* optional fused WHERE `pred <op> literal` evaluated inside the aggregate scan (no materialised
 * filtered batch): Filter -> Aggregate of vinum/planner/planner.py:373-378,463-469 in one pass. */
int vnm_agg_set_predicate(vnm_agg* h, int enabled, int op, int scalar_is_float, double dval, int64_t ival);
/* Multi-GPU: the finished result of this handle will be exchanged with other ranks.  rank_aligned = 1 restricts the
 * operator to run layouts that every rank derives identically from the keys alone (hash partitions: owner(f) = f * P / F,
 * vnm_agg_run_partitions / _reorder / vnm_agg_merge_partitioned); the dense-key paths, whose code range comes from a
 * per-rank sample, are only used while the group count stays small enough for the all-gather exchange, where nothing
 * needs aligning. */
int vnm_agg_set_exchange_mode(vnm_agg* h, int rank_aligned);
/* The operator's own group-count estimate for a batch (the sample it would take itself: exact for up to ~30 k groups,
 * HyperLogLog beyond), WITHOUT aggregating anything; 0 = not applicable (the key is not a plain 8-byte column).
 * Multi-GPU hosts call it on every rank, agree on the maximum and pass it to vnm_agg_set_hint, so that all ranks cut their
 * results into the same partitions (the partition count follows the hint). */
int vnm_agg_estimate_groups(vnm_agg* h, int64_t nrows, const vnm_dcol* key, int64_t* estimate, void* stream);
/* expected number of groups (0 = unknown): sizes the table and picks the kernel strategy */
int vnm_agg_set_hint(vnm_agg* h, int64_t expected_groups);
/* BaseAggregate::Next (base_aggregate.cpp:23-45).  inputs[i] is the input column of func i (ignored for
 * COUNT_STAR).  pred may be NULL when no predicate is set.  Asynchronous on `stream`. */
int vnm_agg_next_device(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs,
                        const vnm_dcol* pred, void* stream);
/* Asynchronous streams (round 4).  The reference feeds an aggregate one record batch per Next() call (base_aggregate.cpp:23-45;
 * TableReaderOperator / stream_reader.py:32-94 produce them) and its state does not depend on where the batches are cut.  With
 * vnm_agg_set_async(h, 1), vnm_agg_next_device only RECORDS a batch of the hot shape (one plain 8-byte key; COUNT(*) / COUNT /
 * SUM / AVG of one plain float64 column; a plain float64 predicate column or none): no launch, allocation or host read-back per
 * call.  The waiting batches go to the device together, as the segments of ONE logical batch (one launch of the path's kernels
 * over all of them), when vnm_agg_sync / vnm_agg_finish / any result call is made, when 2^30 rows or 256 batches are waiting, or
 * when a batch of another shape arrives (that one is processed as usual, after the waiting ones).  Group-count estimates and the
 * dense path's code range are sampled from the FIRST waiting batch; errors of a waiting batch surface in the call that processes it.
 * CONTRACT: the buffers of every batch passed while async is on must stay alive and unchanged until the next vnm_agg_sync /
 * vnm_agg_finish / vnm_agg_result_* / vnm_agg_dense_table call on the handle returns.  Results are identical to the synchronous
 * mode (same kernels, same merges).  Default: off.
 * Batches over SEVERAL plain 8-byte input columns (int64 / uint64 key) are recorded too: when they go to the device the path is chosen
 * from the stream's total row count, the program is cut into one part per input column where a rule applies (the parts record the
 * batches in turn and launch once each), and otherwise the batches are processed one by one as in the synchronous mode. */
int vnm_agg_set_async(vnm_agg* h, int enabled);
/* processes every waiting batch and waits for `stream` */
int vnm_agg_sync(vnm_agg* h, void* stream);
/* Which batches of an asynchronous stream the library still only holds RECORDED.  Every vnm_agg_next_device call on the handle
 * has a sequence number (0, 1, 2, ...; *last_seq = the latest call's); *oldest_seq = the number of the oldest call whose batch is
 * still waiting somewhere in the operator (-1: none is).  The caller may release the buffers of every batch with a smaller number
 * -- what keeps the memory of a long stream bounded (the reference streams inputs larger than memory batch by batch:
 * vinum/api/stream_reader.py:32-94, README.rst:43-45).  *batches / *rows (optional): how much is waiting (at most 256 batches /
 * 2^30 rows per queue; a batch the parts of a split program hold is counted once per part).  Any pointer may be NULL. */
int vnm_agg_waiting(vnm_agg* h, int64_t* batches, int64_t* rows, int64_t* oldest_seq, int64_t* last_seq);
/* Expressions inside aggregates -- `sum((1 - total) * (2 + tax) * (1 - tip))`, vinum/tests/test_query_results.py:436-443;
 * the reference's planner projects the expression into a temporary column first (vinum/planner/planner.py:384-417).
 * vnm_agg_set_input_expr: the input column of function `func_idx` (and of every function sharing its in_col_id; declare
 * their input type as VNM_F64) is the value of `program` (postfix, as vnm_project; result float64) over the n_cols
 * columns passed to vnm_agg_next_device_expr as expr_cols.  In the hot shape ({COUNT(*), COUNT, SUM, AVG} of the
 * expression, plain 8-byte key or no GROUP BY, float64 columns without NULLs, program of + - * / negation within 16
 * instructions / 4 columns / stack depth 4) the expression is evaluated IN REGISTERS inside the scan / partition
 * kernels -- no materialised column; otherwise one fused vnm_project pass materialises it first.  inputs[i] of the
 * functions reading the expression are ignored. */
int vnm_agg_set_input_expr(vnm_agg* h, int func_idx, int n_ins, const struct vnm_expr_ins* program, int n_cols);
int vnm_agg_next_device_expr(vnm_agg* h, int64_t nrows, const vnm_dcol* keys, const vnm_dcol* inputs, const vnm_dcol* pred,
                             int n_expr_cols, const vnm_dcol* expr_cols, void* stream);
/* BaseAggregate::Result part 1: compact the table into dense device arrays; returns group count. */
int vnm_agg_finish(vnm_agg* h, int64_t* n_groups, void* stream);
/* dense partial state (after finish), for the multi-GPU exchange: key words then accumulator words,
 * each a device array of n_groups uint64.  n_key_words / n_acc_words describe the layout. */
int vnm_agg_layout(vnm_agg* h, int* n_key_words, int* n_acc_words);
int vnm_agg_dense_ptrs(vnm_agg* h, uint64_t** key_words, uint64_t** acc_words);
/* multi-GPU exchange helper: the finished dense run as rows [n_groups][n_key_words + n_acc_words] (device,
 * row-major) grouped by owner rank, owner = mix(key words) mod world exactly as vinum_amd/distributed.py::owner_of;
 * counts_host[world] receives the rows per owner. */
int vnm_agg_bucket_by_owner(vnm_agg* h, int world, uint64_t* out_rows, int64_t* counts_host, void* stream);
/* merge dense partial states produced by another handle with the same spec (device pointers) */
int vnm_agg_merge_device(vnm_agg* h, int64_t n, uint64_t* const* key_words, uint64_t* const* acc_words,
                         void* stream);
/* Partition-aligned exchange for large G (single 8-byte key, add-merge words): the partitioned path leaves the
 * groups of hash partition f contiguous and every rank uses the same hash bits, so owner(f) = f * world / F and
 * the owner merges partition by partition in LDS (no HBM atomics).
 *   vnm_agg_run_partitions: F when the finished result is such a run, else 0 (all ranks must agree).
 *   vnm_agg_run_reorder:    rows in partition order [n][2 + n_acc_words], device uint32 row counts per partition,
 *                           host row counts per owner.
 *   vnm_agg_merge_partitioned: on an EMPTY handle: received rows grouped by source rank, row offsets of the
 *                           source blocks (host, world + 1), device uint32 counts [world][nlocal]. */
int64_t vnm_agg_run_partitions(vnm_agg* h);
int vnm_agg_run_reorder(vnm_agg* h, int world, uint64_t* out_rows, uint32_t* out_part_counts,
                        int64_t* owner_counts_host, void* stream);
int vnm_agg_merge_partitioned(vnm_agg* h, int world, int64_t nlocal, const uint64_t* rows,
                              const int64_t* src_row_offsets_host, const uint32_t* part_counts, void* stream);
/* merge row-major partial groups [n][n_key_words + n_acc_words] (layout of vnm_agg_bucket_by_owner) */
int vnm_agg_merge_rows(vnm_agg* h, int64_t n, const uint64_t* rows, void* stream);
/* The receive buffer of the one-collective small-result exchange (vinum_amd/distributed.py::exchange_small_fixed): `nblocks` blocks
 * of (block_rows + 1) such rows, row 0 of every block being its header (word 0 = how many of the following rows hold partial
 * groups).  Merged like vnm_agg_merge_rows, the counts are read on the device. */
int vnm_agg_merge_row_blocks(vnm_agg* h, int nblocks, int64_t block_rows, const uint64_t* blocks, void* stream);
/* BaseAggregate::Result part 2 (+ agg funcs' Summarize, agg_funcs.h:72-80,358-397,482-491,519-540):
 * D2H + host finalisation.  key j -> vals[n] raw 64-bit patterns + valid[n] bytes.
 * func i -> cells of 16 bytes (decimal128 uses all 16), valid bytes; returns the output kind. */
enum vnm_out_kind { VNM_OUT_U64 = 0, VNM_OUT_I64, VNM_OUT_F64, VNM_OUT_F32, VNM_OUT_DEC128, VNM_OUT_I32 };
int vnm_agg_result_key(vnm_agg* h, int key_idx, uint64_t* vals, uint8_t* valid);
int vnm_agg_result_func(vnm_agg* h, int func_idx, void* cells16, uint8_t* valid, int* out_kind);

/* BaseAggregate::Result part 2 ON THE DEVICE: the result column of group key `key_idx` / function `func_idx` as Arrow
 * buffers in HBM (what base_aggregate.cpp:47-68 assembles from the functions' Summarize methods, agg_funcs.h:72-80,
 * 482-491, 519-540 incl. the 128-bit AVG): out_values = n_groups values of the column's OUTPUT type (keys and MIN / MAX:
 * the input type; COUNT: uint64; SUM: int64 / uint64 / float64, int32 for time32; AVG: float64, float32 for 8 / 16-bit
 * integers -- *out_kind as in vnm_agg_result_func), out_bitmap = Arrow validity bitmap of ((n_groups + 63) / 64) * 8
 * bytes, *null_count = NULL results.  Returns 2 (and leaves the buffers undefined) when an int64 / uint64 SUM overflowed
 * 64 bits in some group: the reference then promotes the whole column to decimal128 (agg_funcs.h:366-389), which
 * vnm_agg_result_func does on the host. */
int vnm_agg_result_key_device(vnm_agg* h, int key_idx, void* out_values, uint8_t* out_bitmap, int64_t* null_count, void* stream);
/* The same for n_cols result columns in ONE kernel launch (the accumulator words of a group are read once and
 * the launch cost is paid once): which[c] >= 0 selects aggregate function which[c], which[c] < 0 selects key
 * column ~which[c].  out_kinds[c] = VNM_OUT_* of a function column, -1 for a key column (it keeps its input
 * type).  Returns 2 when any selected int64 / uint64 SUM overflowed (all other columns are still valid). */
int vnm_agg_result_device(vnm_agg* h, int n_cols, const int* which, void* const* out_values,
                          uint8_t* const* out_bitmaps, int* out_kinds, int64_t* null_counts, void* stream);
int vnm_agg_result_func_device(vnm_agg* h, int func_idx, void* out_values, uint8_t* out_bitmap, int* out_kind,
                               int64_t* null_count, void* stream);
/* BaseAggregate::Result (base_aggregate.cpp:47-68: Reserve(G) on every builder, Summarize every group, one RecordBatch)
 * with the output columns ALLOCATED BY THE LIBRARY -- the group count is only known once the last pass has run, exactly as
 * the reference's builders only learn it in SummarizeGroups (single_numerical_hash_aggregate.cpp:48-68).  When the last
 * batch went through the dense-key path, its direct-addressed final pass is still pending at this point and writes the
 * result columns ITSELF (key, SUM, AVG, COUNT of a float64 column: the Summarize expressions of agg_funcs.h:139-142,
 * 286-292, 519-522 evaluated where the accumulators live) -- no dense partial state, no second kernel re-reading it.
 * Every other state: vnm_agg_finish + vnm_agg_result_device.  *n_groups = rows; out_values[c] = vnm_malloc block of
 * >= *n_groups cells of the column's output type (as vnm_agg_result_device); out_bitmaps[c] = validity bitmap block or
 * NULL when the column has no NULL result.  The CALLER frees both with vnm_free.  Returns 2 like vnm_agg_result_device. */
int vnm_agg_result_device_alloc(vnm_agg* h, int n_cols, const int* which, void** out_values, uint8_t** out_bitmaps,
                                int* out_kinds, int64_t* null_counts, int64_t* n_groups, void* stream);

/* Multi-GPU, large results (legal because base_aggregate.cpp:23-45 only ever Init()s or Update()s a group's
 * state: partial states of disjoint row sets merge commutatively).  The dense-key path replaces a key by a code inside a
 * key RANGE; when all ranks use the SAME range, their direct-addressed final tables are slot-compatible: they add up
 * element by element, a key's owner is a range of codes, and nothing has to be bucketed, counted or re-ordered.
 *   vnm_agg_dense_range      this rank's sampled key range of a batch, as order-preserving unsigned images (*lo > *hi: the
 *                            key type has no dense path).  Ranks reduce lo by MIN, hi by MAX ...
 *   vnm_agg_set_dense_range  ... and give every operator the agreed range BEFORE its first batch (lo > hi: none).
 *   vnm_agg_dense_table      after ONE batch: *table = 2^*bits slots {double sum; float lo; uint32 count} (count 0 = no
 *                            group), slot = scrambled key code; NULL when the batch did not take that path (spilled keys,
 *                            another aggregate shape, several batches): the caller falls back to the owner-bucketed
 *                            exchange.  geometry[4] = {range start, bits, multiplier, sign}: must agree on all ranks.
 *                            The table belongs to the handle.
 *   vnm_agg_merge_dense_tables   owner side: slices [code0, code0 + n) of the nsrc ranks' tables (rank order) -> the
 *                            result of the EMPTY handle h (`like`: any handle that produced one of the tables).  Sums merge
 *                            with the library's compensated add, in rank order: the result does not depend on the owner. */
int vnm_agg_dense_range(vnm_agg* h, int64_t nrows, const vnm_dcol* key, uint64_t* lo, uint64_t* hi, void* stream);
int vnm_agg_set_dense_range(vnm_agg* h, int key_type, uint64_t lo, uint64_t hi);
int vnm_agg_dense_table(vnm_agg* h, void** table, int* bits, uint64_t* geometry, void* stream);
int vnm_agg_merge_dense_tables(vnm_agg* h, const vnm_agg* like, int nsrc, const void* const* slices, uint64_t code0,
                               int64_t n, void* stream);

/* Host-only helpers (no GPU touched): how (functions, input types) lower onto 64-bit accumulator words
 * with commutative merge kinds (0 add-u64, 1 add-f64, 2 min-u64, 3 max-u64, 4 compensated add-f64: the high
 * word of a (hi, lo) pair -- every add into it is a returning atomic whose exact rounding error (TwoSum) is
 * added to the NEXT word, an ordinary add-f64 word; the float64 SUM / AVG of a group is hi + lo, i.e. the
 * correctly rounded exact sum up to second-order terms, whatever order the rows arrived in), and the
 * finalisation of one result column from dense accumulator words in HOST memory.  Used by the multi-GPU merge
 * and unit-tested on CPU. */
int vnm_agg_plan_host(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                      const int* in_types, const int* in_flags, const int* in_col_ids, int* n_key_words,
                      int* n_acc_words, int* merge_kinds /* >= 40 ints */, int* n_ops,
                      int* op_kind_col_word /* >= 3 * 48 ints: per-row update kind, distinct input column, word;
                                               kinds: 0 count rows, 1 count valid, 2 sum f64, 3 sum i64 (wrap),
                                               4 sum low 32 bits, 5 sum high 32 (signed), 6 sum high 32 (unsigned),
                                               7 min, 8 max (on the order-preserving 64-bit encoding) */);
int vnm_agg_finalize_host(int kind, int n_keys, const int* key_types, int n_funcs, const int* funcs,
                          const int* in_types, const int* in_flags, const int* in_col_ids, int func_idx,
                          int64_t n, const uint64_t* const* acc_words, void* cells16, uint8_t* valid,
                          int* out_kind);

/* Arrow level (host RecordBatches through the C Data Interface; columns are staged to HBM with
 * pinned double-buffered DMA).  Same constructor arguments as the pybind classes. */
typedef struct vnm_agg_op vnm_agg_op;
vnm_agg_op* vnm_agg_op_create(int kind, int n_groupby, const char** groupby_cols, int n_aggcols,
                              const char** agg_cols, int n_funcs, const int* func_types,
                              const char** in_cols, const char** out_cols);
/* Consumes both.  The first batch fixes the layout: the columns the operator reads are found there by name, and every later
 * batch must hold each of them at the same position, with the same name and format (otherwise: "the batch schema changed").
 * Columns nobody reads may be of any type.
 * A child with a `dictionary` is never read as its indices.  dictionary<intN, utf8 | large_utf8 | binary | large_binary> is taken as
 * group key, under COUNT and under MIN / MAX: per batch the dictionary's VALUES go through the operator's device dictionary, the
 * native-width indices through vnm_strdict_remap_indices (route note keys:dictionary_child); a row is NULL when its index or its
 * value is (one NULL group; COUNT counts neither); result() hands key and MIN / MAX columns back in the dictionary type, ordered
 * flag kept, with a dictionary of exactly the values the groups use (vnm_dict_take_compact; more of them than the index type
 * names fails with Arrow's "These dictionaries cannot be combined. ...").  Later batches must repeat the value format too.  Any
 * other dictionary type as key, or any dictionary type under SUM / AVG, gets the error of an unsupported column type. */
int vnm_agg_op_next(vnm_agg_op* h, struct ArrowArray* batch, struct ArrowSchema* schema);
/* Every batch of an Arrow C stream, as one vnm_agg_op_next each (consumes and releases the stream).  The reference's pipeline
 * hands over 10 000-row batches (vinum/__init__.py:52, table_batch_reader.cpp:5-16); crossing the language boundary once per
 * few hundred of them instead of once each is what the caller saves -- the operator keeps small batches as they are (no
 * concatenation on the host) and stages them to the device together. */
int vnm_agg_op_next_stream(vnm_agg_op* h, struct ArrowArrayStream* stream);
int vnm_agg_op_result(vnm_agg_op* h, struct ArrowArray* out, struct ArrowSchema* out_schema);
void vnm_agg_op_destroy(vnm_agg_op* h);

/* ---- sort: Sort.next / Sort.sorted ------------------------------------------------------------------
 * replaces vinum/core/vinum_lib.cpp:126-142, vinum_cpp/src/operators/sort/sort.cpp:11-63
 * (arrow::compute::SortIndices + Take).  The order is total -- order-preserving key encodings, then the row id (stable) --
 * with NaN after all numbers and NULL after NaN for both ASC and DESC, whichever of the library's sorts produces it: the sample
 * sort over 8-byte entry words (one 8-byte key, order only, distinct keys: vnm_sort_apx.inc), the splitter sample sort (keyed
 * results, duplicated keys), the stable LSD radix sort (several keys, heavily duplicated keys, rows that arrive in key order),
 * top-K selection for limit > 0. */
int vnm_sort_indices(int n_keys, const vnm_dcol* keys, const int* orders, int64_t length,
                     int64_t limit /* <=0: full sort; >0: only the first `limit` rows are needed */,
                     int64_t* out_indices /* device, length entries (first `limit` valid) */, void* stream);
/* The same (Sort::Sorted = SortIndices + Take of EVERY column, sort.cpp:22-40), and -- for a full sort whose first key is
 * int64 / uint64 / float64 without NULL, NaN or -0.0 -- the sorted
 * values of that key straight from the sort (out_sorted_key0: device, length x 8 bytes; *wrote_key0 = 1), which saves
 * the caller the gather (vnm_take: 25 ms per 1e9 rows) for that column.  *wrote_key0 = 0: gather as usual. */
int vnm_sort_indices_keyed(int n_keys, const vnm_dcol* keys, const int* orders, int64_t length, int64_t limit,
                           int64_t* out_indices, void* out_sorted_key0, int* wrote_key0, void* stream);
int vnm_take(const vnm_dcol* col, const int64_t* indices, int64_t n, void* out_values, uint8_t* out_valid,
             void* stream);
/* Take for the column types vnm_take does not cover (Sort::Sorted takes EVERY column of the table, any Arrow type: sort.cpp:38-40).
 * All pointers are DEVICE pointers unless said otherwise.
 * vnm_take_varwidth: utf8 / binary values by row ids.  offsets: n_rows + 1 int64 offsets into `data` (int32 Arrow offsets are widened
 *   by the caller), validity: bitmap (bit i = row i) or NULL.  out_offsets: n + 1 int64s; *out_data: the gathered bytes, a block the
 *   CALLER frees with vnm_free (*out_bytes of them); out_valid: n bytes (1 = valid) or NULL.  A NULL row contributes no bytes.
 * vnm_take_bits: bits (bit_offset + indices[i]) of a bitmap -> n bytes of 0 / 1 (boolean values, validity bitmaps).
 * vnm_take_fixed16: 16-byte values (decimal128).
 * vnm_decimal128_sort_keys: decimal128 values -> (high word int64, low word uint64): two numeric sort keys, most significant first. */
int vnm_take_varwidth(const int64_t* offsets, const uint8_t* data, const uint8_t* validity, const int64_t* indices, int64_t n,
                      int64_t* out_offsets, uint8_t** out_data, int64_t* out_bytes, uint8_t* out_valid, void* stream);
int vnm_take_bits(const uint8_t* bits, int64_t bit_offset, const int64_t* indices, int64_t n, uint8_t* out_bytes, void* stream);
int vnm_take_fixed16(const void* values, const int64_t* indices, int64_t n, void* out_values, void* stream);
int vnm_decimal128_sort_keys(const void* values, int64_t n, int64_t* out_hi, uint64_t* out_lo, void* stream);
/* Distributed sample sort (Sort::Sorted over rows sharded by batch, sort.cpp:22-44): the per-rank partition step.
 * Stable partition of the rows 0 .. n-1 by OWNER = number of splitters <= codes[row] (ascending int64 splitters, at most 63 of them; a
 * code equal to a splitter goes to the upper owner).  out_order: n row numbers, the rows of owner 0 first, source order kept inside an
 * owner; out_counts: n_splitters + 1 rows-per-owner counts.  All DEVICE pointers; returns after the stream has been synchronised. */
int vnm_partition_by_owner(const int64_t* codes, int64_t n, const int64_t* splitters, int n_splitters, int64_t* out_order,
                           int64_t* out_counts, void* stream);
typedef struct vnm_sort_op vnm_sort_op;
vnm_sort_op* vnm_sort_op_create(int n, const char** cols, const int* orders);
int vnm_sort_op_next(vnm_sort_op* h, struct ArrowArray* batch, struct ArrowSchema* schema);
int vnm_sort_op_next_stream(vnm_sort_op* h, struct ArrowArrayStream* stream);   /* as vnm_agg_op_next_stream */
/* Column types: numeric / temporal, utf8 / large_utf8 / binary / large_binary, decimal128, boolean (payload only), and
 * dictionary<intN, utf8 | large_utf8 | binary | large_binary> as key or payload: the batch dictionaries' values go through one
 * device dictionary per column, the native-width indices through vnm_strdict_remap_indices, a key orders by the values' ranks (a
 * row that is NULL by index or by value last in both directions), and the column leaves in its own dictionary type -- indices of
 * the input's width, the ordered flag kept, a dictionary of exactly the values the produced rows use (vnm_dict_take_compact; more
 * of them than the index type holds fails with Arrow's "These dictionaries cannot be combined. ...").  A dictionary over any
 * other value type: "has a type the GPU path does not handle". */
int vnm_sort_op_sorted(vnm_sort_op* h, int64_t limit, struct ArrowArray* out, struct ArrowSchema* out_schema);
void vnm_sort_op_destroy(vnm_sort_op* h);

/* ---- projection: arithmetic expression evaluation ----------------------------------------------------
 * replaces the NumPy ufunc dispatch vinum/core/expressions.py:13-24 as evaluated by
 * VectorizedExpression.evaluate (vinum/core/base.py:105-125,145-151) and ProjectOperator._kernel
 * (vinum/core/algebra.py:52-64): one fused kernel per output expression, no temporaries.
 * Program = postfix opcode stream over columns of ANY numeric width (int8..uint64, float32, float64).  NumPy
 * promotion (2.x / NEP 50): floats win (float32 only survives 8 / 16-bit integers), same-signedness integers widen,
 * unsigned + signed -> the next wider signed type (uint64 + signed -> float64), integer results wrap in the result
 * width, `/` -> float64 (float32 for float32 with narrow integers), `%` = floor-mod (sign of the divisor); a literal
 * (VNM_EX_CONST_*) is "weak" and takes the column's type (arg = 1 makes it a strong int64 / float64 value, what an IN
 * list is); a column with NULLs is evaluated as float64 with NaN (float32 stays float32).  A program with an integer
 * power whose exponent is a signed column synchronises the stream and fails with NumPy's ValueError when an exponent is
 * negative; every other program is launched asynchronously. */
typedef struct vnm_expr_ins {
    int32_t op;  /* enum vnm_expr_op */
    int32_t arg; /* column index for VNM_EX_COL */
    double imm_f;
    int64_t imm_i;
} vnm_expr_ins;
/* what one program may hold (vnm_project counts its implied final STORE as an instruction; vnm_agg_set_input_expr takes the same) */
#define VNM_PROJECT_MAX_INS 64
#define VNM_PROJECT_MAX_COLS 16
#define VNM_PROJECT_MAX_OUT 16
/* out_type (returned): the vnm_type of the result, values stored with that type's width (a buffer of length*8 bytes
 * always suffices), or VNM_MASK_U8 (predicate) with out_values = length bytes (BETWEEN / IN are compiled to AND / OR
 * chains by the caller). */
int vnm_project(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                void* out_values, int* out_type, void* stream);
/* A whole SELECT list in one pass (ProjectOperator._kernel evaluates every expression of the list over the same
 * batch, vinum/core/algebra.py:52-64): the program holds n_out expressions, each terminated by
 * VNM_EX_STORE(arg = output index); every input column is read from HBM once.  out_values[k] must hold
 * length*8 bytes (length bytes suffice for a predicate output); out_types[k] is returned per output. */
int vnm_project_multi(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                      int n_out, void** out_values, int* out_types, void* stream);

/* ---- TableBatchReader -----------------------------------------------------------------------------
 * replaces vinum/core/vinum_lib.cpp:144-165 / vinum_cpp/src/operators/table_batch_reader.cpp:5-16.
 * Host-side zero-copy slicing lives in the Python shim (pyarrow Table.slice); this entry stages one
 * host column into HBM through the library's pinned double buffer and returns the device view. */
int vnm_stage_column(const void* host_values, const uint8_t* host_validity, int64_t offset, int64_t length,
                     int32_t type, vnm_dcol* out, void* stream);
int vnm_free_column(vnm_dcol* col);

/* ---- string dictionary: non-numeric GROUP BY keys -----------------------------------------------------------------------
 * replaces the scalar-vector keyed map of GenericHashAggregate (vinum_cpp/src/operators/aggregate/generic_hash_aggregate.h:10-45:
 * one hash + Equals of arrow::Scalar vectors per row) for utf8 / binary key columns: every row's value -> a running int32
 * dictionary code (equal bytes <=> equal code, across all batches given to one handle); the codes then are an ordinary
 * numeric key column of the aggregate operators.  NULL rows get code -1.  Codes are NOT dense (ids are handed out in chunks;
 * vnm_strdict_ids = their upper bound).
 * vnm_strdict_encode: one Arrow utf8 / large_utf8 / binary array as HOST buffers (offsets int32 or int64, data, validity bitmap
 * or NULL, logical offset / length); offsets + bytes cross PCIe once, the codes come back to out_codes_host (length int32s).
 * *n_new / *new_bytes: the values this call added to the dictionary; vnm_strdict_fetch_new copies their (id, length) pairs and
 * concatenated bytes (in that order) to host buffers of n_new / n_new / new_bytes entries -- the caller's copy of the
 * dictionary is the concatenation of these (how vinum_amd/vinum_lib.py decodes the result's key column).
 * vnm_strdict_encode_device: the same over DEVICE buffers (offsets->values / ->type (VNM_I32 | VNM_I64) / ->offset /
 * ->length = rows + 1; validity bitmap + bit offset or NULL; data = byte data_base of the Arrow data buffer). */
typedef struct vnm_strdict vnm_strdict;
vnm_strdict* vnm_strdict_create(void);
void vnm_strdict_destroy(vnm_strdict* h);
int64_t vnm_strdict_ids(vnm_strdict* h);
int vnm_strdict_encode(vnm_strdict* h, const void* offsets_host, int offsets_are_64, const uint8_t* data_host,
                       const uint8_t* validity_host, int64_t offset, int64_t length, int32_t* out_codes_host,
                       int64_t* n_new, int64_t* new_bytes, void* stream);
int vnm_strdict_encode_device(vnm_strdict* h, const vnm_dcol* offsets, const uint8_t* validity, int64_t validity_offset,
                              const uint8_t* data, int64_t data_base, int32_t* out_codes, int64_t* n_new, int64_t* new_bytes,
                              void* stream);
int vnm_strdict_fetch_new(vnm_strdict* h, int32_t* ids_host, int32_t* lens_host, uint8_t* bytes_host);
/* Order-preserving RANKS of the dictionary's values (round 5: utf8 / binary ORDER BY keys on the device -- Arrow's SortIndices compares
 * such values byte-wise, sort.cpp:22-37).  out_rank_of_id: DEVICE array of vnm_strdict_ids(h) int32s; entry id = the position of the
 * value with that id among all values in ascending byte order (ids never handed out are left untouched).  vnm_strdict_codes_to_ranks maps
 * a column of codes (device; -1 = NULL -> rank 0, the row's validity bit says NULL) to its ranks: an ordinary int32 sort key column. */
int vnm_strdict_ranks_device(vnm_strdict* h, int32_t* out_rank_of_id, void* stream);
int vnm_strdict_codes_to_ranks(const int32_t* codes, const int32_t* rank_of_id, int64_t n, int32_t* out_ranks, void* stream);
/* LIKE / NOT LIKE against the dictionary's values (LikeFunction, vinum/core/functions.py:301-344: the pattern becomes the regex
 * '^' + p.replace('_', '.').replace('%', '.*') + '$', matched per row).  Restated exactly: `_` and `.` match one code point other
 * than '\n', `%` zero or more such code points, every other byte is literal; a value also matches when it ends in '\n' and
 * matches without that byte ('$' matches before a final newline).  VNM_LIKE_STRIP_NUL: trailing NUL bytes are dropped first (a
 * utf8 column reaches the reference as a NumPy 'U' array, which strips them; large_utf8 stays an object array and keeps them).
 * A pattern with another regex metacharacter (\ ^ $ * + ? { } [ ] | ( )) is refused.
 * vnm_like_compile: the pattern -> tokens on the host (no device): 3 int32 per token (kind VNM_LIKE_TOK_*, byte start, byte
 * length in the pattern), consecutive `%` folded; out_tokens holds 3 * max(pattern_len, 1) entries.
 * vnm_strdict_like: out_match_of_id[id] = 1 / 0 for every id in [id_begin, vnm_strdict_ids(h)) -- 0 for an id never handed
 * out.  out_match_of_id is a DEVICE buffer of at least vnm_strdict_ids(h) bytes; only that range is written, so a table kept
 * across batches is extended with id_begin = the id count it covers.  One kernel on `stream`, launched asynchronously (a
 * pattern's tokens are uploaded once per handle and kept). */
#define VNM_LIKE_STRIP_NUL 1
#define VNM_LIKE_TOK_LIT 0
#define VNM_LIKE_TOK_ANY 1
#define VNM_LIKE_TOK_STAR 2
int vnm_like_compile(const uint8_t* pattern, int64_t pattern_len, int32_t* out_tokens, int64_t* n_tokens);
int vnm_strdict_like(vnm_strdict* h, const uint8_t* pattern, int64_t pattern_len, int flags, int64_t id_begin,
                     uint8_t* out_match_of_id, void* stream);
/* Two dictionaries against each other: what `city_from = city_to` / `city_from < city_to` need when the two columns keep separate
 * dictionaries.  Bytes are compared exactly (no trailing-NUL rule, as a literal is compared by vnm_strdict_* callers).
 * vnm_strdict_translate: out_dst_code_of_src_id[id] = the code dst holds for the bytes of src's value id, for every id in
 * [id_begin, vnm_strdict_ids(src)); -2 where dst does not hold the value or the id was never handed out (-1 stays the NULL code,
 * valid codes are >= 0).  The encode kernels' probe of dst's table without the insert: dst is only read.  One kernel on `stream`,
 * launched asynchronously.  A table kept across batches is extended with id_begin = the id count it covers only while dst has
 * not grown (an absent value can become present).
 * vnm_strdict_ranks_joint: dense ranks of the values of both dictionaries in the ascending byte order of their union -- the order of
 * vnm_strdict_ranks_device (a prefix first); equal bytes in a and b get the same rank.  out_rank_of_id_a / _b: DEVICE arrays of
 * vnm_strdict_ids(a) / (b) int32s; entries of ids never handed out are left untouched.  Enqueued on `stream`; like
 * vnm_strdict_ranks_device it reads counts back in between and returns when the ranks are written. */
int vnm_strdict_translate(vnm_strdict* src, vnm_strdict* dst, int64_t id_begin, int32_t* out_dst_code_of_src_id, void* stream);
int vnm_strdict_ranks_joint(vnm_strdict* a, vnm_strdict* b, int32_t* out_rank_of_id_a, int32_t* out_rank_of_id_b, void* stream);
/* upper() / lower() (UpperStringFunction / LowerStringFunction, vinum/core/functions.py:279-298: pc.utf8_upper / pc.utf8_lower, one
 * code point -> one code point, no context) as a function of the dictionary's VALUES: dst is the dictionary DERIVED from src under
 * the map, a row then costs one lookup of its code.
 * vnm_strdict_map_codepoints: for every id of src in [id_begin, vnm_strdict_ids(src)) the value's bytes are decoded as UTF-8, each
 * code point found in map_from (n_map entries, strictly ascending, at most 2048) is replaced by the map_to entry at the same
 * position, the result is encoded and found or inserted in dst; out_dst_code_of_src_id[id] = dst's code of it (a DEVICE array of
 * vnm_strdict_ids(src) int32s; only that range is written).  -2: the id was never handed out, or its value is malformed (-1 stays
 * the NULL code).  Two values with one image get one code.  src is only read; afterwards vnm_strdict_last_new / _fetch_new on dst
 * return the values it added, as after an encode.  A table kept across batches is extended with id_begin = the id count it covers;
 * growth of dst invalidates nothing as long as dst grows through this call alone.  The map is checked and uploaded on the first
 * call with a dst handle and kept; a later call with another map is refused, so is a map_from that is not strictly ascending and a
 * pair whose image needs more than twice the bytes of its source (a value's room in the scratch buffer is twice its length; the
 * Unicode case maps stay inside: ASCII maps into ASCII, the longest growth is 2 -> 3 bytes).
 * Malformed means structurally broken, what Arrow refuses: a continuation byte where a lead byte is due, a lead byte without all
 * its continuation bytes inside the value (the bytes of the NEXT value are never read), 0xF8..0xFF.  Overlong forms, surrogates and
 * values past U+10FFFF are not looked for (Arrow is lax about them too): a code point outside the map is copied as it stands.
 * Such a value is counted and not inserted.  out_invalid != NULL: the count is stored there and a non-zero count returns non-zero
 * with "Invalid UTF8 sequence in input" -- the well-formed values are in dst and in the table all the same.  out_invalid == NULL:
 * malformed values just get -2.  Either way the call goes through dst's encode, which reads counts back: it returns when the
 * table is written. */
int vnm_strdict_map_codepoints(vnm_strdict* src, vnm_strdict* dst, const int32_t* map_from, const int32_t* map_to, int64_t n_map,
                               int64_t id_begin, int32_t* out_dst_code_of_src_id, int64_t* out_invalid, void* stream);
/* concat() / || (ConcatFunction, vinum/core/functions.py:250-276: every operand through np.array(., dtype='U'), folded left with
 * np.char.add).  An operand contributes its bytes without TRAILING 0x00 bytes (leading and embedded ones stay); a NULL contributes
 * the four bytes "None"; the result is never NULL.  The work is on bytes: malformed UTF-8 is concatenated as it stands.
 *
 * vnm_strdict_concat_affix -- one column and literals, a function of the value: for every id of src in [id_begin,
 * vnm_strdict_ids(src)) the image prefix + rstrip_nul(value) + suffix is written into scratch spans and found or inserted in dst
 * through dst's span encode (the one insert path); out_dst_code_of_src_id[id] = dst's code of it (a DEVICE array of
 * vnm_strdict_ids(src) int32s, only that range is written; -2: the id was never handed out).  The image of NULL, prefix + "None" +
 * suffix, is inserted by the same call and its code stored in *out_null_code (host).  Two values with one image ("a\0" and "a") get
 * one code.  src is only read; afterwards vnm_strdict_last_new / _fetch_new on dst return the values it added.  A table kept across
 * batches is extended with id_begin = the id count it covers.  dst remembers the prefix and suffix of its first call and refuses
 * others.  The call goes through dst's encode, which reads counts back: it returns when the table is written.
 *
 * vnm_strdict_gather_codes -- the row pass of that form: out_codes[i] = table[codes[i]], and null_code where row i is NULL by its
 * validity bit (bit validity_offset + i; validity may be NULL) or by code -1.  A code at or past n_ids gets -2 and is never an
 * address.  No validity comes out.  codes points at row 0.  One kernel on `stream`, launched asynchronously. */
int vnm_strdict_concat_affix(vnm_strdict* src, vnm_strdict* dst, const uint8_t* prefix, int64_t prefix_len, const uint8_t* suffix, int64_t suffix_len,
                             int64_t id_begin, int32_t* out_dst_code_of_src_id, int32_t* out_null_code, void* stream);
int vnm_strdict_gather_codes(const int32_t* codes, const uint8_t* validity, int64_t validity_offset, const int32_t* table, int64_t n_ids, int64_t n,
                             int32_t null_code, int32_t* out_codes, void* stream);
/* vnm_strpair -- two columns, concat(a, sep, b): a persistent open-addressing table on the device, one per (pair of dictionaries,
 * prefix, sep, suffix), that lives across batches so a pair keeps its code.  A slot holds the 64-bit key (uint32)(code_a + 1) << 32 |
 * (uint32)(code_b + 1) -- NULL is code -1 or a cleared validity bit of the operand's column -- and the pair's int32 code in dst.
 * vnm_strpair_create takes the literal in front of a and the one behind b (either may be empty).
 * vnm_strpair_concat(h, a, b, dst, sep, sep_len, codes_a, codes_b, length, out_codes, stream): codes_a / codes_b are int32 DEVICE
 * columns of `length` rows (values, validity or NULL, Arrow offset) holding codes of a / b; out_codes[i] (DEVICE, `length` int32s) =
 * dst's code of prefix + value_a + sep + value_b + suffix of row i.  Passes: find (4 rows per lane, 16-byte loads where the three
 * pointers are aligned; probe, CAS(EMPTY -> key); no lane waits for another; the probe walk is bounded by 1024 slots and by the capacity; the
 * CAS winner appends its slot to a new-pairs list); on overflow -- past 70 % fill or the bound -- the table grows x4, a rehash kernel
 * re-inserts key and code, the find pass runs again (counted in `rehashes`); concat (one lane per NEW pair: exact length first,
 * every store held against it, the spans through dst's encode, the codes into the new slots); gather (in place).  String bytes are
 * touched once per distinct pair.  a and b may be one dictionary; dst must be neither.  a, b are only read and may have grown since
 * the last call.  A separator other than the first call's is refused; so is a code outside [-1, vnm_strdict_ids).  Returns when
 * out_codes is written; vnm_strdict_last_new / _fetch_new on dst return the values the call added.
 * The initial slot count is $VNM_STRPAIR_SLOTS rounded up to a power of two (default 65536, at least 16).
 * vnm_strpair_stats: out6 = {calls with length > 0, pairs concatenated (= distinct pairs seen), rehashes, slots, occupied slots,
 * occupied slots WITHOUT a code (0 after every call that returned 0)}. */
typedef struct vnm_strpair vnm_strpair;
vnm_strpair* vnm_strpair_create(const uint8_t* prefix, int64_t prefix_len, const uint8_t* suffix, int64_t suffix_len);
void vnm_strpair_destroy(vnm_strpair* h);
int vnm_strpair_concat(vnm_strpair* h, vnm_strdict* a, vnm_strdict* b, vnm_strdict* dst, const uint8_t* sep, int64_t sep_len, const vnm_dcol* codes_a,
                       const vnm_dcol* codes_b, int64_t length, int32_t* out_codes, void* stream);
int vnm_strpair_stats(vnm_strpair* h, int64_t* out6, void* stream);
/* to_str() (StringCastFunction, vinum/core/functions.py:189-193, an AbstractCastFunction, functions.py:148-193: np.array(column,
 * dtype='str'), NumPy's text of the value) over an integer, date32 or timestamp column: the table of vnm_strpair keyed by the VALUE.
 * A fixed-width value widened to 64 bits (by sign; by zero extension for the unsigned types) is itself the key, so the same find /
 * rehash / store-codes / gather passes serve, a formatter runs ONCE per distinct value (vnm_tostr.hpp: ts_room, then ts_write with
 * every store held against that room; the longest image is 29 bytes) and the spans go through dst's encode.  No string is built per
 * row: a row costs one load of its value, one probe and one 4-byte gather.
 *   VNM_TOSTR_INT / VNM_TOSTR_UINT   decimal digits, '-' in front of a negative one; the width and signedness are the column's vnm_type
 *                                    (VNM_I8 .. VNM_I64 for INT, VNM_U8 .. VNM_U64 for UINT)
 *   VNM_TOSTR_DATE32                 a VNM_I32 column of days: datetime64[D] text, YYYY-MM-DD, the year as C's %04d with the sign inside
 *                                    the width (0000-01-01, -001-12-31, 10000-01-01, -5877641-06-23)
 *   VNM_TOSTR_TIMESTAMP_S .. _NS     a VNM_I64 column: YYYY-MM-DDTHH:MM:SS and .fff / .ffffff / .fffffffff at full width; division floors
 *                                    (-1 ns is 1969-12-31T23:59:59.999999999); years of unit s reach 12 digits; INT64_MIN prints NaT.
 *                                    A zone-aware column prints its UTC instant (the stored value), as the reference does
 * A NULL row -- a cleared validity bit -- gives the four bytes "None", for every kind, and no validity comes out: the rule concat()
 * has for its operands.  This DEPARTS from the reference for integers (with a NULL in the batch it converts the column to float64
 * first and prints "1.0" / "nan", so one column prints differently from batch to batch) and for dates (it prints "NaT").
 * The empty marker of the table is the all-ones key, which is the value -1 / UINT64_MAX: that value and NULL live in two side slots
 * outside the probed range (slot indices `slots` and `slots + 1`), each claimed by one CAS on a flag word; both survive a rehash.
 * vnm_strval_to_str(h, dst, values, length, out_codes, stream): `values` is a DEVICE column of `length` rows (values, validity or
 * NULL, Arrow offset); out_codes[i] (DEVICE, `length` int32s) = dst's code of the text of row i.  4 rows per lane, one 4 / 8 / 16 /
 * 32-byte access where row 0's address is a multiple of 4 widths and out_codes of 16 bytes, scalar loads otherwise.  A column type
 * that does not fit the kind (a float column; a date kind over a VNM_I64 column) is refused, so is a type other than the first
 * call's.  Returns when out_codes is written; vnm_strdict_last_new / _fetch_new on dst return the values the call added.  dst may
 * hold values from other sources: a text it already has keeps its code.  Every call with rows leaves the route note
 * "to_str:value_table".  The initial slot count is $VNM_STRPAIR_SLOTS, as for vnm_strpair.
 * vnm_strval_stats: as vnm_strpair_stats: out6 = {calls with length > 0, values formatted (= distinct values seen, NULL and the
 * all-ones value included), rehashes, slots, occupied slots (the side slots included), occupied slots WITHOUT a code}. */
enum vnm_tostr_kind { VNM_TOSTR_INT = 0, VNM_TOSTR_UINT, VNM_TOSTR_DATE32, VNM_TOSTR_TIMESTAMP_S, VNM_TOSTR_TIMESTAMP_MS, VNM_TOSTR_TIMESTAMP_US,
                      VNM_TOSTR_TIMESTAMP_NS };
typedef struct vnm_strval vnm_strval;
vnm_strval* vnm_strval_create(int kind);
void vnm_strval_destroy(vnm_strval* h);
int vnm_strval_to_str(vnm_strval* h, vnm_strdict* dst, const vnm_dcol* values, int64_t length, int32_t* out_codes, void* stream);
int vnm_strval_stats(vnm_strval* h, int64_t* out6, void* stream);
/* date() / datetime() / from_timestamp() (DateFunction / DatetimeFunction / TimestampFunction, vinum/core/functions.py:25-137:
 * np.array(column, dtype='datetime64[unit]'), NumPy's ISO 8601 parser) -- the inverse of to_str().  Over a STRING column the function
 * depends on the value alone: each distinct value is parsed ONCE on the device into a per-id table (vnm_dtparse.hpp has the grammar,
 * the value rule and what is refused though NumPy takes it), and a row costs one code load and one 8-byte gather.
 * vnm_strdict_parse_datetime: for every id in [id_begin, vnm_strdict_ids(h)) out_value_of_id[id] = the int64 value (days for
 * VNM_UNIT_D, unit counts since 1970-01-01 otherwise; 0 unless the status is 0) and out_status_of_id[id] = 0 a value, 1 NULL (the
 * empty string, "NaT" in any letter case: NumPy's NaT), 2 refused; an id never handed out gets status 2.  Both are DEVICE arrays of
 * vnm_strdict_ids(h) entries and only that range is written, so a table kept across batches is extended with id_begin = the id count
 * it covers.  One lane per value over the dictionary's heap; h is only read.  *out_first_refused_id (host; may be NULL) = the lowest
 * id in the range that was HANDED OUT and refused, or -1: refused strings are data, the call itself succeeds, and whether a ROW
 * holds such a value is the row pass's to say (a dictionary derived by concat() always holds the image of NULL, "None...", which
 * no row may hold).  It reads that id back, so it returns when the tables are written.
 * vnm_strdict_gather_temporal: the row pass.  out_values[i] = value_of_id[codes[i]] as int32 for out_width == 4 (date32) and as
 * int64 for out_width == 8; row i is NULL in out_validity_bitmap (a DEVICE bitmap at bit offset 0, (n + 7) / 8 bytes, required) and
 * its value 0 when its validity bit is clear (bit validity_offset + i; validity may be NULL), its code is negative, its code is at or
 * past n_ids -- never an address -- or its id's status is 1.  A non-NULL row whose id's status is 2 keeps the table's 0 as a value
 * and is reported: *out_first_refused_id (host; may be NULL) = the lowest such id, or -1 -- the caller raises naming the value.  codes points at row 0.  A lane takes 8 rows and writes ONE whole byte of the bitmap, which no other lane
 * touches; the bits past n in the last byte and the bytes past (n + 7) / 8 are left as they were.  16-byte accesses where row 0 of
 * codes / out_values is 16-byte aligned, scalar ones otherwise.  out_null_count (host; may be NULL): the NULL rows.  With either
 * host pointer the call synchronises, without both it is one kernel on `stream`, launched asynchronously.
 * vnm_temporal_rescale: date(ts_col) / datetime(col, unit) over a date32 (VNM_I32) or timestamp (VNM_I64) column: a change of unit.
 * One of mul / div is 1.  div > 1 (to a coarser unit): the FLOOR of the division (-1 s is day -1), by NumPy's formula (v - (div - 1))
 * / div for a negative v, whose subtraction wraps within div - 1 of INT64_MIN as NumPy's does.  mul > 1 (to a finer unit): the
 * product, wrapping as NumPy's cast does (computed unsigned).  INT64_MIN in a VNM_I64 column with out_width 8 is NumPy's NaT and
 * stays INT64_MIN.  With mul == div == 1 it is from_timestamp() over an integer column narrower than VNM_U64: the values widened
 * to 64 bits (VNM_I8 .. VNM_U32 are taken; VNM_U64 and the float types are refused).  Rows [col->offset, col->offset + length) -> out_values[0 .. length) as int32 (out_width 4) or int64 (8); the
 * caller passes the validity through.  One kernel on `stream`, launched asynchronously. */
enum vnm_temporal_unit { VNM_UNIT_D = 0, VNM_UNIT_S, VNM_UNIT_MS, VNM_UNIT_US, VNM_UNIT_NS };
int vnm_strdict_parse_datetime(vnm_strdict* h, int unit, int64_t id_begin, int64_t* out_value_of_id, uint8_t* out_status_of_id,
                               int64_t* out_first_refused_id, void* stream);
int vnm_strdict_gather_temporal(const int32_t* codes, const uint8_t* validity, int64_t validity_offset, const int64_t* value_of_id,
                                const uint8_t* status_of_id, int64_t n_ids, int64_t n, int out_width, void* out_values, uint8_t* out_validity_bitmap,
                                int64_t* out_null_count, int64_t* out_first_refused_id, void* stream);
int vnm_temporal_rescale(const vnm_dcol* col, int64_t mul, int64_t div, int64_t length, int out_width, void* out_values, void* stream);
/* Arithmetic on temporal values: typed, exact int64 with validity, what NumPy's datetime64 / timedelta64
 * arithmetic computes.
 * vnm_temporal_affine: out_values[i] = a[i] * ka + b[i] * kb + c over rows [offset, offset + length) of one or two columns (b may
 * be NULL, a may not), each 4 bytes (date32, VNM_I32) or 8 bytes (timestamp / duration, VNM_I64) wide with its own validity and
 * Arrow offset; any other type is refused.  Products and sums wrap (computed unsigned) as NumPy's do.  Unit alignment is in the
 * factors (ka = 86400 for a date against seconds), subtraction is kb = -k, negation ka = -1, a constant operand c.  out_width 4
 * writes the low 32 bits of the result as int32, 8 the int64.  Row i is NULL in out_validity_bitmap (a DEVICE bitmap at bit offset
 * 0, (length + 7) / 8 bytes, required) and its value 0 when either input row is NULL, an 8-byte input holds INT64_MIN (NaT) or the
 * 64-bit result is INT64_MIN (whatever out_width is: NumPy computes dates in int64 too).  A lane takes 8 rows and writes ONE whole byte of the bitmap, which no other lane touches; the bits
 * past length in the last byte and the bytes past (length + 7) / 8 are left as they were.  16-byte accesses where row 0 of a
 * buffer is 16-byte aligned, scalar ones otherwise.  out_null_count (host; may be NULL): the NULL rows; with it the call
 * synchronises, without it it is one kernel on `stream`, launched asynchronously.
 * vnm_temporal_busday: np.is_busday over a date32 (VNM_I32) column as a byte mask (0 / 1, what a predicate program writes):
 * out_mask[i] = bit ((day + 3) floor-mod 7) of weekmask (bit 0 Monday; 1970-01-01 is a Thursday) AND day is not among `holidays`,
 * a sorted, distinct DEVICE array of n_holidays <= 8192 days (32 KB of LDS; more is refused with "ValueError: ...") that is staged
 * into LDS and probed with a branch-free binary search.  A NULL row gives 0.  One kernel on `stream`, launched asynchronously. */
int vnm_temporal_affine(const vnm_dcol* a, int64_t ka, const vnm_dcol* b, int64_t kb, int64_t c, int64_t length, int out_width,
                        void* out_values, uint8_t* out_validity_bitmap, int64_t* out_null_count, void* stream);
/* vnm_temporal_floordiv: duration // duration (np.floor_divide over timedelta64) -> int64: out_values[i] = floor(x / y), x = a[i] * ka
 * and y = b[i] * kb with the unit factors in ka / kb (wrapping); a NULL column pointer makes that side the constant ka / kb itself
 * (one side at least is a column).  Operands, validity, bitmap, lane shape and out_null_count as vnm_temporal_affine.  A NULL or NaT
 * (8-byte INT64_MIN) input row is NULL with value 0 (NumPy gives 0 there); a zero divisor gives 0, as NumPy does. */
int vnm_temporal_floordiv(const vnm_dcol* a, int64_t ka, const vnm_dcol* b, int64_t kb, int64_t length, int64_t* out_values,
                          uint8_t* out_validity_bitmap, int64_t* out_null_count, void* stream);
int vnm_temporal_busday(const vnm_dcol* days, int64_t length, int weekmask, const int32_t* holidays, int64_t n_holidays, uint8_t* out_mask,
                        void* stream);
/* A dictionary-typed Arrow column (dictionary<intN, utf8 | large_utf8 | binary | large_binary>): the batch dictionary's indices ->
 * codes of the running dictionary.  The caller runs the batch dictionary's VALUES through vnm_strdict_encode and uploads the result
 * as code_of_index (n_values int32s on the DEVICE; -1 = a NULL value), so only n_values strings are hashed, not one per row.
 * indices: the DEVICE view of the index buffer -- any of VNM_I8 ... VNM_U64, optional validity bitmap, Arrow offset, length.
 * out_codes[i] = code_of_index[index[i]], or -1 when row i is NULL or its value is NULL (length int32s on the device).
 * out_validity: NULL, or a device bitmap at bit offset 0, bit i = out_codes[i] >= 0, (length + 7) / 8 bytes, the bits past length
 * in the last byte 0; every byte is written by exactly one lane (no atomics).
 * The bounds test precedes the table load: an index outside [0, n_values) on a valid row is never used as an address; the row gets
 * -1 and is counted.  With out_bad the call synchronises, stores the count there and, if it is not 0, returns non-zero with
 * "dictionary index out of bounds" (what Arrow's validate(full=True) says of such an array).  out_bad == NULL: one kernel on
 * `stream`, launched asynchronously; the caller accepts -1 for such rows.
 * A lane takes 8 consecutive rows (one bitmap byte): 16-byte index loads when values + offset is 16-byte aligned (8-byte for the
 * 1-byte types), element loads otherwise and in the last partial group; 16-byte code stores when out_codes is 16-byte aligned.
 * The table is read through L2, one tile per workgroup, or -- up to 8192 values, when a workgroup's rows are at least 4 x the values --
 * from a copy in LDS by a persistent grid (VNM_REMAP_LDS=0 / 1 pins the form; DESIGN.md section 4.9c has both measured).
 * VNM_STRDICT_REMAP_TILE: rows per workgroup and step (a size the tests walk around). */
#define VNM_STRDICT_REMAP_TILE 2048
int vnm_strdict_remap_indices(const vnm_dcol* indices, const int32_t* code_of_index, int64_t n_values, int32_t* out_codes,
                              uint8_t* out_validity, int64_t* out_bad, void* stream);
/* The way back: running codes -> a compact dictionary column of the input's index type (what Sort hands out for a dictionary-typed
 * column).  Ids are handed out in chunks and a LIMIT uses only some of them, so the codes are not dense.
 * With c_i = codes[rows ? rows[i] : i] (codes: int32s on the DEVICE; rows: n int64 row numbers on the device, NULL = identity):
 *   an id is USED if some c_i equals it; out_used_ids (device, room for min(n, n_ids) int32s) receives the used ids in ascending
 *   order and *out_n_used their count;
 *   out_indices[i] (device, n values of index_type: VNM_I8 ... VNM_U64) = the position of c_i in out_used_ids, 0 where c_i < 0;
 *   out_validity: NULL, or a device bitmap at bit offset 0, bit i = c_i >= 0, (n + 7) / 8 bytes, the bits past n in the last byte
 *   0; every byte is written by exactly one lane (no atomics); *out_null_count (may be NULL) = the cleared bits among the n.
 * The two counts are HOST memory, written after the call's own synchronisation of `stream`.
 * n_ids bounds the codes (vnm_strdict_ids): the bounds test precedes every table access, so a code >= n_ids on a row that is read
 * is never used as an address; such rows are counted and the call returns non-zero with "code out of bounds (K row(s) ...)".
 * If *out_n_used exceeds the largest value of index_type the call returns non-zero with Arrow's own words for the same data
 * (pa.concat_arrays): "These dictionaries cannot be combined.  The unified dictionary requires a larger index type."; nothing is
 * promised about the output buffers then.
 * Three passes: mark (plain one-byte stores into a zeroed n_ids-byte table), scan (exclusive, over the table), gather (a lane takes
 * 8 consecutive rows = one bitmap byte; 16-byte code loads when rows == NULL and codes is 16-byte aligned; 8 / 16-byte index
 * stores when out_indices is 16-byte aligned (8 for the 1-byte types), element stores otherwise and in the last partial group).
 * The scan's table is read through L2, one tile per workgroup, or -- up to VNM_DICT_COMPACT_LDS_IDS ids, when a workgroup's rows are
 * at least 4 x n_ids -- from a copy in LDS by a persistent grid (VNM_DICT_COMPACT_LDS=0 / 1 pins the form).
 * VNM_DICT_COMPACT_TILE: rows per workgroup and step of the gather, ids per workgroup of the scan (sizes the tests walk around). */
#define VNM_DICT_COMPACT_TILE 2048
#define VNM_DICT_COMPACT_LDS_IDS 8192
int vnm_dict_take_compact(const int32_t* codes, const int64_t* rows, int64_t n, int64_t n_ids, int index_type, void* out_indices,
                          uint8_t* out_validity, int64_t* out_null_count, int32_t* out_used_ids, int64_t* out_n_used, void* stream);

/* ---- IN / NOT IN against a list of any length: the list as a device-resident set ---------------------------
 * replaces np.isin(x, values[, invert]) (vinum/core/expressions.py:39-40; the parser hands it ONE Literal holding the whole list,
 * vinum/parser/parser.py:151-160) for lists the projection interpreter's OR chain of `==` cannot hold.
 * vnm_in_set_create: the list as NumPy's array holds it -- n int64 values, or n float64 values as soon as one member is a float
 * (list_is_float = 1).  Needs no device; n == 0 fails with "ValueError: IN with an empty list".
 * vnm_in_set_probe: out_mask[i] = 1 / 0 for row i of `col` (invert: NOT IN), one byte per row, one kernel on `stream`, launched
 * asynchronously.  out_mask is a DEVICE buffer of `length` bytes, 4-byte aligned.  Column and list are compared in the domain the
 * chain of `==` compares them in, so both give the same mask:
 *   VNM_IN_DOM_I64  an integer column other than uint64 without validity, int64 list: exact; the column value is widened
 *   VNM_IN_DOM_U64  a uint64 column without validity, int64 list: exact; negative members and values >= 2^63 match nothing
 *   VNM_IN_DOM_F64  a float column, a float64 list, or a column with a validity bitmap (it reaches NumPy as float64 with NaN,
 *                   vinum/arrow/record_batch.py:112-118): members and values as float64, compared with == (-0.0 == 0.0, NaN and
 *                   NULL rows are in no list).
 * A domain's canonical table (sorted, distinct; NaN members dropped, -0.0 folded) is built and uploaded by the first probe that
 * needs it and kept by the handle.  Routes (vnm_route_last names the one taken): a bitmap where the members' range is at most
 * 64 bits per member (integer domains), else a branch-free binary search of the sorted table; either from LDS up to 32 KB, else
 * from global memory.
 * vnm_in_set_plan_host: what a probe of a column of `col_type` would use -- domain, route, the canonical table (out_table: room
 * for n 64-bit patterns of the domain's type, *out_members of them written) and the members' range hi - lo + 1 (integer domains;
 * 0 otherwise).  Host only, no device touched. */
typedef struct vnm_in_set vnm_in_set;
enum vnm_in_domain { VNM_IN_DOM_I64 = 0, VNM_IN_DOM_U64 = 1, VNM_IN_DOM_F64 = 2 };
enum vnm_in_route { VNM_IN_ROUTE_BITMAP_LDS = 0, VNM_IN_ROUTE_BITMAP_GLOBAL = 1, VNM_IN_ROUTE_SORTED_LDS = 2, VNM_IN_ROUTE_SORTED_GLOBAL = 3 };
int vnm_in_set_create(int list_is_float, const void* values_host, int64_t n, vnm_in_set** out);
void vnm_in_set_destroy(vnm_in_set* h);
int vnm_in_set_probe(vnm_in_set* h, const vnm_dcol* col, int64_t length, int invert, uint8_t* out_mask, void* stream);
int vnm_in_set_plan_host(int list_is_float, const void* values_host, int64_t n, int col_type, int col_has_validity, int* out_domain,
                         int* out_route, int64_t* out_members, uint64_t* out_table, uint64_t* out_range);

/* ---- CSV ingest ---------------------------------------------------------------------------------------
 * replaces, for numeric columns, the pyarrow.csv reader behind stream_csv() / read_csv() (vinum/io/arrow.py:58-61,106;
 * FileReaderOperator vinum/core/algebra.py:268-279): one block of CSV text (must end with '\n'; < 2 GiB) is staged once
 * and tokenised + parsed on the device.  n_fields = fields per row (from the header); field_idx[c] (ascending) / types[c]
 * (VNM_I64 | VNM_F64) select the columns; out_cols[c] receives an HBM column (values + validity bitmap; an empty field is
 * NULL; free with vnm_free_column).  Decimal -> float64 is exact integer arithmetic (correctly rounded, as strtod /
 * fast_float).  fallback[c] = 1: column c holds a field outside the device parser's domain (> 19 significant digits,
 * |decimal exponent| > 19, "nan" / "inf", stray characters): parse that column of this block on the host;
 * fallback[n_cols] = 1: a row ends inside a quoted field (a newline in a value; quoted fields themselves are tokenised: delimiters
 * inside quotes do not split, a quoted number is parsed from between its quotes); fallback[n_cols + 1] = 1: a row whose
 * field count differs from n_fields. */
int vnm_csv_parse_block(const char* host_text, int64_t nbytes, int skip_header, int delimiter, int n_fields, int n_cols,
                        const int* field_idx, const int* types, vnm_dcol* out_cols, int64_t* n_rows, int* fallback,
                        void* stream);
/* Round 5: the non-numeric columns pyarrow.csv infers for such files stay on the device too (the same reader, its `string`,
 * `date32[day]`, `timestamp[s]` and `timestamp[ns]` conversions: vinum/io/arrow.py:58-61,106).  types[c] may also be
 *   VNM_CSV_STRING        utf8: out_cols[c] = int32 codes of dicts[c] (a vnm_strdict the caller keeps for the column across blocks; never
 *                         NULL -- pyarrow reads an empty field of a string column as the empty string); the field bytes are encoded where
 *                         they lie in the staged text (vnm_strdict_encode_spans) and checked to be well-formed UTF-8 (fallback otherwise:
 *                         pyarrow raises on them); after the call vnm_strdict_last_new / vnm_strdict_fetch_new hand over the values
 *                         the block added, as after vnm_strdict_encode.  A field with an escaped quote ("" inside quotes): fallback.
 *   VNM_CSV_DATE32        YYYY-MM-DD -> int32 days since 1970-01-01
 *   VNM_CSV_TIMESTAMP_S   YYYY-MM-DD | YYYY-MM-DD[ T]hh:mm | ...:ss -> int64 seconds
 *   VNM_CSV_TIMESTAMP_NS  the same plus .f{1,9} -> int64 nanoseconds (years 1678 .. 2261)
 * Calendar-checked (month, day of month, leap years, hh < 24, mm / ss < 60); any other spelling Arrow's ISO 8601 parser knows (zone
 * offsets, hour-only times, "Z") raises the column's fallback flag.  dicts: n_cols entries (NULL where the column is no string) or NULL. */
#define VNM_CSV_STRING 200
#define VNM_CSV_DATE32 201
#define VNM_CSV_TIMESTAMP_S 202
#define VNM_CSV_TIMESTAMP_NS 203
/*   VNM_CSV_BOOL          true / True / TRUE / 1 and false / False / FALSE / 0 (pyarrow's true_values / false_values) -> int32 1 / 0: the
 *                         codes of a dictionary [false, true] (booleans travel dictionary-coded like every non-numeric column)
 *   VNM_CSV_TIME32_S      hh:mm | hh:mm:ss (hh < 24) -> int32 seconds since midnight */
#define VNM_CSV_BOOL 204
#define VNM_CSV_TIME32_S 205
int vnm_csv_parse_block_ex(const char* host_text, int64_t nbytes, int skip_header, int delimiter, int n_fields, int n_cols,
                           const int* field_idx, const int* types, vnm_strdict* const* dicts, vnm_dcol* out_cols, int64_t* n_rows,
                           int* fallback, void* stream);
/* vnm_strdict_encode_device over SPANS of one device buffer: row r = the lens[r] bytes at data[starts[r]] (no NULLs). */
int vnm_strdict_encode_spans(vnm_strdict* h, const int64_t* starts, const int32_t* lens, int64_t n, const uint8_t* data,
                             int32_t* out_codes, int64_t* n_new, int64_t* new_bytes, void* stream);
/* how many values (and bytes) the last encode of this handle added and vnm_strdict_fetch_new has not handed over yet: the sizes it
 * fills (a fetch hands them over ONCE) */
int vnm_strdict_last_new(vnm_strdict* h, int64_t* n_new, int64_t* new_bytes);

/* device memory helpers for hosts without a GPU allocator of their own (ctypes / cgo bindings).
 * vnm_malloc / vnm_free go through the library's caching allocator: a freed block is handed to the NEXT
 * request of a similar size at once, without waiting for the device.  That is safe while everything that
 * touches the block is enqueued on ONE stream (work is ordered on it; the entry points that return counts or
 * flags also synchronise it).  A host that spreads calls over several streams must synchronise the stream
 * that last used a block before vnm_free (as with hipFree, minus its implicit device synchronisation). */
void* vnm_malloc(int64_t bytes);
int vnm_free(void* p);
/* hand every block the caching allocator holds but nobody uses back to the device (hipFree); returns the
 * bytes released.  For long-lived hosts that want the HBM back between queries; live blocks are untouched. */
int64_t vnm_pool_trim(void);
/* The cache also gives itself back: once no allocation or release has gone through the allocator for `idle_ms` (default 2000;
 * VNM_POOL_IDLE_MS) a background thread releases the cached blocks beyond `keep_bytes` (default 256 MiB; VNM_POOL_KEEP_BYTES),
 * so a host that embeds the library (an unmodified Vinum process) does not sit on tens of GB of HBM after a large query, while a
 * query in flight is never trimmed under its feet.  idle_ms < 0: never; keep_bytes < 0: leave it unchanged.
 * vnm_pool_cached_bytes: what the cache holds right now. */
int vnm_pool_set_idle_trim(int64_t idle_ms, int64_t keep_bytes);
int64_t vnm_pool_cached_bytes(void);
/* Guard mode of the caching allocator: TEST INFRASTRUCTURE, off by default (VNM_POOL_GUARD=1|2 sets the initial mode), and while
 * it is off the allocator does exactly what the paragraphs above say.  mode 1: every block handed out from now on is laid out as
 * front zone | body (the bytes asked for) | back zone inside its raw block; the front zone is a multiple of 4096 bytes, the back
 * zone is everything up to the end of the raw block (rounding slack and reuse slack included, at least 4096 bytes); both hold a
 * canary that is checked on the device when the block is released.  mode 2: the body is also filled with the 64-bit word
 * 0x7FF8DEAD7FC0BEEF (NaN as float64 and as two float32, huge as an integer) before the caller sees it, and with another such
 * word once it is released.  The mode synchronises the device at every allocation and release; it never fails a call, it records.
 * A block remembers how it was allocated, so the mode may change while blocks are live.
 * vnm_pool_guard_report: checks the zones of every live guarded block too, then writes a summary line and one line per violation
 * since the last reset: "violation zone=front|back offset=<of the first damaged byte, from the body's end (back, >= 0) or start
 * (front, < 0)> bytes=<damaged> first=<up to 16 bytes from there, hex> requested=<bytes asked for> block=<raw block bytes> ptr=
 * mode= site=<library+offset(symbol+offset) of the pool_alloc call> span=<last timed kernel span> test=<$PYTEST_CURRENT_TEST>";
 * the same line goes to stderr when the violation is found.  Returns the bytes needed including the final 0; *violations and
 * *blocks_checked count since the last vnm_pool_guard_reset.
 * vnm_pool_guard_layout: what a fresh block for `bytes` looks like in the CURRENT mode (needs no device): the raw block's size,
 * the front zone and the smallest back zone (0 and 0 with the guard off, where the block is the rounded size of always). */
int vnm_pool_set_guard(int mode);
int64_t vnm_pool_guard_report(char* buf, int64_t cap, int64_t* violations, int64_t* blocks_checked);
void vnm_pool_guard_reset(void);
int vnm_pool_guard_layout(int64_t bytes, int64_t* block_bytes, int64_t* front_zone, int64_t* back_zone_min);
int vnm_memcpy_h2d(void* dst, const void* src, int64_t bytes);
int vnm_memcpy_d2h(void* dst, const void* src, int64_t bytes);
int vnm_memset(void* dst, int value, int64_t bytes);
/* device -> device copy on `stream` (asynchronous) */
int vnm_memcpy_d2d(void* dst, const void* src, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINUM_HIP_H */
