// Projection: fused arithmetic expression evaluation for gfx950.
//
// Replaces the NumPy ufunc dispatch of vinum/core/expressions.py:13-24 as driven by
// VectorizedExpression.evaluate (vinum/core/base.py:105-125; n-ary chains left-folded :145-151) and
// ProjectOperator._kernel (vinum/core/algebra.py:52-64).  The reference materialises one full temporary
// column per AST node; here one kernel reads each input column once and writes the result once.
// Roofline: HBM, 8 B per distinct input column + 8 B per output per row.
//
// NumPy semantics restated (the arithmetic lives in third-party NumPy, pinned >= 1.19 by the reference; the image and the
// golden vectors use 2.2, i.e. NEP 50 promotion: Python literals are "weak" and take the array's type):
//   * every numeric Arrow width: int8..int64, uint8..uint64, float32, float64.  result_type of two columns: floats win
//     (float32 only survives 8 / 16-bit integers), same-signedness integers widen, unsigned + signed go to the next wider
//     signed type (uint64 + signed -> float64); integer (+,-,*,%) wrap in the RESULT width; `/` is true division (float64,
//     float32 only for float32 with 8 / 16-bit integers); a Python int literal takes the column's type (out of range for
//     it: OverflowError, as NumPy 2), a Python float literal makes integers float64 and leaves float32 alone;
//   * `%` = floor-mod with the sign of the divisor (x % 0 = 0 for ints, NaN for floats);
//   * comparisons: integers exactly (int64 vs uint64 included), mixed int / float in float64, float32 column against a
//     Python literal in float32 (the literal is rounded first), against an IN list in float64 (np.isin makes an array);
//   * a column WITH nulls reaches NumPy as float64 with NaN -- float32 stays float32 -- (record_batch.py:112-118).
// Values travel through the interpreter as 64-bit words: integers sign / zero extended, floats as float64 bits (a
// float32 value as the float64 of that float32); after every operation whose result type is narrower the word is
// brought back into that type's range (wraparound / rounding to float32), which is bit-identical to narrow arithmetic.
//
// Built-in scalar functions (_default_functions_registry, vinum/core/functions.py:353-387): abs, sqrt, sin, cos, tan, log,
// log2, log10, power and the casts to_float / to_int / to_bool.  NumPy 2 ufunc typing: sqrt and the transcendentals of
// (u)int8 are float16 (NumPy's `e` loops: sqrt in float32, rounded to half), of (u)int16 and float32 float32, of wider
// integers and float64 float64; abs keeps the type (integers wrap); power promotes like the other binary operators.
// sqrt is correctly rounded in its width (bit-identical to NumPy); the transcendentals and float power run in float64
// (OCML) and are rounded to the result type.
// A float16 value is held as the float64 of that half and brought back into half range after every operation (float32
// first, then half, like NumPy's float16 loops).  Programs with any of these opcodes run a MATH instantiation of the
// kernel -- MATH = 1 for the exact ones (abs, sqrt, casts, float16 arithmetic), MATH = 2 when a transcendental or power is
// in the program, whose OCML code needs far more registers; every other program runs the same code as before (MATH = 0).
//
// VNM_EX_LOOKUP_U8 (LIKE / NOT LIKE over a dictionary-coded string column, vinum/core/functions.py:301-344) pushes
// table[code] as a predicate value: `arg` is the int32 code column, `imm_i` the index in `cols` of the TABLE -- a VNM_U8
// column of one byte per dictionary id (KeyDictionary.like_table, vnm_strdict_like), whose length is the dictionary's id
// count, not the batch length.  A table is read by this opcode only; a NULL code, a negative code and a code at or past the
// table's length push 0.  Programs with a lookup run an LK = 1 instantiation, so the push path of every other program keeps
// the registers it had.
//
// VNM_EX_LOOKUP_I32 (a dictionary-coded string column compared with ANOTHER such column: the codes of one dictionary translated into
// the other's, or both columns' ranks in the byte order of the union of their dictionaries -- vnm_strdict_translate,
// vnm_strdict_ranks_joint) pushes table[code] as a VALUE: same operands, the table a VNM_I32 column without NULLs.  The value is held
// like an int32 column with NULLs -- float64, NaN where the code is NULL, negative or past the table -- so the comparisons' NULL rule
// applies as it stands (compare False, `!=` True).  Programs with this opcode run the LK = 2 instantiation (both lookups); LK = 0 / 1
// programs run the code they ran before.
#include "vnm_common.hpp"
#include "vnm_project_type.hpp"   // the limits, PIns and the host's program typer

namespace vnm {

constexpr int PJ_BLOCK = 256;
#ifndef VNM_PJ_R
#define VNM_PJ_R 4
#endif
constexpr int PJ_R = VNM_PJ_R;                 // rows per lane per tile: one opcode decode serves PJ_R rows
constexpr int PJ_TILE = PJ_BLOCK * PJ_R;
static_assert(PJ_R % 2 == 0, "a lane owns pairs of adjacent rows");

struct ProjArgs {
    int n_ins;
    int n_cols;
    PIns ins[PJ_MAX_INS];
    vnm_dcol cols[PJ_MAX_COLS];
    int64_t length;
    void* out[PJ_MAX_OUT];
    uint8_t out_is_mask[PJ_MAX_OUT];  // predicate outputs are byte masks
    uint8_t out_type[PJ_MAX_OUT];     // vnm_type of a value output (its width decides the store), or VNM_OUT_F16
    int* neg_pow;                     // MATH: set when an integer power meets a negative exponent column (NumPy ValueError)
};

__device__ __forceinline__ uint64_t pj_dbits(double d) { return (uint64_t)__double_as_longlong(d); }
__device__ __forceinline__ double pj_bitsd(uint64_t x) { return __longlong_as_double((long long)x); }

// wraparound / rounding of a 64-bit interpreter word into the range of a narrower type
template <int MATH>
__device__ __forceinline__ uint64_t pj_narrow(int t, uint64_t x) {
    if (MATH > 0 && t == VNM_OUT_F16) return pj_dbits((double)(_Float16)(float)pj_bitsd(x));   // float32 first, then half
    switch (t) {
        case VNM_I8: return (uint64_t)(int64_t)(int8_t)x;
        case VNM_I16: return (uint64_t)(int64_t)(int16_t)x;
        case VNM_I32: return (uint64_t)(int64_t)(int32_t)x;
        case VNM_U8: return x & 0xFFULL;
        case VNM_U16: return x & 0xFFFFULL;
        case VNM_U32: return x & 0xFFFFFFFFULL;
        case VNM_F32: return (uint64_t)__double_as_longlong((double)(float)__longlong_as_double((long long)x));
        default: return x;
    }
}
__device__ __forceinline__ uint64_t np_umod(uint64_t a, uint64_t b) { return b == 0 ? 0 : a % b; }
__device__ __forceinline__ double np_fmod(double a, double b) {
    // npy_divmod: mod = fmod(a, b); if (mod) { if ((b < 0) != (mod < 0)) mod += b; } else mod = copysign(0, b)
    if (b == 0.0) return __builtin_nan("");
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0) != (m < 0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}
__device__ __forceinline__ int64_t np_imod(int64_t a, int64_t b) {
    if (b == 0) return 0;
    if (b == -1) return 0;  // avoids INT64_MIN % -1
    int64_t m = a % b;
    if (m != 0 && ((m < 0) != (b < 0))) m += b;
    return m;
}

// an operand word as a double: 0 float64 bits, 1 signed integer, 2 unsigned integer
__device__ __forceinline__ double pj_as_f64(int cvt, uint64_t x) {
    return cvt ? (cvt == 2 ? (double)x : (double)(int64_t)x) : pj_bitsd(x);
}

// the exact unary built-ins (abs, sqrt, casts) over one word.  cvt: how the operand is held; f32: compute in float32 (float32 / float16 results)
__device__ __forceinline__ uint64_t pj_math1(int op, int cvt, bool f32, uint64_t x) {
    switch (op) {
        case VNM_EX_ABS:   // floats: the sign bit cleared (NaN included); signed integers: wraps in the result width
            return cvt == 0 ? (x & 0x7FFFFFFFFFFFFFFFULL) : ((int64_t)x < 0 ? (uint64_t)0 - x : x);
        case VNM_EX_TO_BOOL: return (cvt == 0 ? pj_bitsd(x) != 0.0 : x != 0) ? 1ULL : 0ULL;
        case VNM_EX_TO_F64: return pj_dbits(pj_as_f64(cvt, x));
        case VNM_EX_TO_I64: {
            if (cvt != 0) return x;                               // integers: int64 bits (uint64 wraps)
            const double d = trunc(pj_bitsd(x));
            // NaN, +-inf and values outside [-2^63, 2^63): INT64_MIN, what cvttsd2si gives NumPy on x86-64
            if (!(d >= -9223372036854775808.0 && d < 9223372036854775808.0)) return 0x8000000000000000ULL;
            return (uint64_t)(int64_t)d;
        }
        default:           // VNM_EX_SQRT: correctly rounded in both widths
            return f32 ? pj_dbits((double)sqrtf((float)pj_as_f64(cvt, x))) : pj_dbits(sqrt(pj_as_f64(cvt, x)));
    }
}
// the transcendentals (OCML), kept apart from the cheap functions so only their own loop carries their registers.  They
// run in float64 for every result type: float32 / float16 results are the float64 value rounded (float32, then half),
// which is within 1 ULP where OCML's float32 functions measured up to 2.1 ULP (logf)
__device__ __forceinline__ uint64_t pj_math_t(int op, int cvt, bool f32, uint64_t x) {
    const double d = pj_as_f64(cvt, x);
    double r;
    switch (op) {
        case VNM_EX_SIN: r = sin(d); break;
        case VNM_EX_COS: r = cos(d); break;
        case VNM_EX_TAN: r = tan(d); break;
        case VNM_EX_LOG: r = log(d); break;
        case VNM_EX_LOG2: r = log2(d); break;
        default: r = log10(d); break;
    }
    return pj_dbits(f32 ? (double)(float)r : r);
}

// npy integer power (loops_autovec / `@TYPE@_power`): exponentiation by squaring, wrapping in 64 bits; the caller narrows
__device__ __forceinline__ uint64_t pj_ipow(uint64_t base, uint64_t e) {
    if (e == 0 || base == 1) return 1;
    uint64_t out = (e & 1) ? base : 1;
    e >>= 1;
    while (e > 0) {
        base *= base;
        if (e & 1) out *= base;
        e >>= 1;
    }
    return out;
}

// Postfix interpreter.  The program is uniform, so opcode fetch and dispatch are scalar; the top of the stack
// lives in registers (tos), deeper values in LDS (sized by the host to the program's real depth), and every
// decoded opcode is applied to PJ_R rows of the lane.
template <int MATH, int LK>
__global__ __launch_bounds__(PJ_BLOCK) void project_kernel(ProjArgs a) {
    extern __shared__ uint64_t stk[];  // [depth - 1][PJ_R][PJ_BLOCK]
    const int tid = threadIdx.x;
    const int64_t ntiles = (a.length + PJ_TILE - 1) / PJ_TILE;
#define STK(level, r) stk[((level) * PJ_R + (r)) * PJ_BLOCK + tid]
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // a lane owns PAIRS of adjacent rows (2 tid, 2 tid + 1) + k * 2 * PJ_BLOCK, so 8-byte columns move 16 bytes per
        // request whenever the Arrow offset is even
        const int64_t base = tile * PJ_TILE + 2 * tid;
        const bool full_tile = (tile + 1) * PJ_TILE <= a.length;
        uint64_t tos[PJ_R];
#pragma unroll
        for (int r = 0; r < PJ_R; r++) tos[r] = 0;
        int sp = 0;  // values on the stack, tos included
        for (int i = 0; i < a.n_ins; i++) {
            const PIns& in = a.ins[i];
            const int op = in.op;
            if (op == PJ_NOP) continue;
            if (op == VNM_EX_COL || op == VNM_EX_CONST_F || op == VNM_EX_CONST_I || op == VNM_EX_IS_NULL ||
                op == VNM_EX_IS_NOT_NULL || (LK && op == VNM_EX_LOOKUP_U8) || (LK == 2 && op == VNM_EX_LOOKUP_I32)) {
                // ---- push ----
                if (sp > 0) {
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) STK(sp - 1, r) = tos[r];
                }
                sp++;
                if (op == VNM_EX_COL && full_tile && !a.cols[in.arg].validity && (a.cols[in.arg].offset & 1) == 0 &&
                    (a.cols[in.arg].type == VNM_F64 || (!in.is_f && type_width(a.cols[in.arg].type) == 8 && a.cols[in.arg].type != VNM_F32))) {
                    // 8-byte column pushed with its own type: raw bits, 16 bytes per request
                    const uint64_t* p = (const uint64_t*)a.cols[in.arg].values + a.cols[in.arg].offset + base;
#pragma unroll
                    for (int k = 0; k < PJ_R / 2; k++) {
                        const ulonglong2 t = *(const ulonglong2*)(p + k * (2 * PJ_BLOCK));
                        tos[2 * k] = t.x;
                        tos[2 * k + 1] = t.y;
                    }
                } else if (op == VNM_EX_COL) {
                    const vnm_dcol& c = a.cols[in.arg];
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        uint64_t v = 0;
                        if (row < a.length) {
                            if (in.is_f) {   // float column, or an integer column with NULLs (-> float64 NaN)
                                double d = col_valid(c, row) ? col_f64(c, row) : __builtin_nan("");
                                v = (uint64_t)__double_as_longlong(d);
                            } else {
                                v = (uint64_t)col_i64(c, row);   // sign / zero extended
                            }
                        }
                        tos[r] = v;
                    }
                } else if (LK && op == VNM_EX_LOOKUP_U8) {
                    // table[code]: the table is a few bytes per distinct value and stays in cache
                    const vnm_dcol& c = a.cols[in.arg];
                    const vnm_dcol& t = a.cols[in.imm_i];
                    const int32_t* codes = (const int32_t*)c.values + c.offset;
                    const uint8_t* tab = (const uint8_t*)t.values + t.offset;
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        uint64_t v = 0;
                        if (row < a.length && col_valid(c, row)) {
                            const int32_t code = codes[row];
                            if (code >= 0 && (int64_t)code < t.length) v = tab[code] ? 1ULL : 0ULL;
                        }
                        tos[r] = v;
                    }
                } else if (LK == 2 && op == VNM_EX_LOOKUP_I32) {
                    // table[code] as a value: one dependent 4-byte gather per row (NaN = NULL: no code, or no entry for it)
                    const vnm_dcol& c = a.cols[in.arg];
                    const vnm_dcol& t = a.cols[in.imm_i];
                    const int32_t* codes = (const int32_t*)c.values + c.offset;
                    const int32_t* tab = (const int32_t*)t.values + t.offset;
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        double d = __builtin_nan("");
                        if (row < a.length && col_valid(c, row)) {
                            const int32_t code = codes[row];
                            if (code >= 0 && (int64_t)code < t.length) d = (double)tab[code];
                        }
                        tos[r] = pj_dbits(d);
                    }
                } else if (op == VNM_EX_CONST_F) {
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) tos[r] = (uint64_t)__double_as_longlong(in.imm_f);
                } else if (op == VNM_EX_CONST_I) {
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) tos[r] = (uint64_t)in.imm_i;
                } else {
                    const vnm_dcol& c = a.cols[in.arg];
                    const bool want_null = op == VNM_EX_IS_NULL;
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        bool valid = row < a.length ? col_valid(c, row) : true;
                        tos[r] = (valid != want_null) ? 1ULL : 0ULL;
                    }
                }
            } else if (op == VNM_EX_NEG || op == VNM_EX_BNOT || op == VNM_EX_NOT) {
                // ---- unary ----
#pragma unroll
                for (int r = 0; r < PJ_R; r++) {
                    uint64_t x = tos[r];
                    if (op == VNM_EX_NEG)
                        x = in.is_f ? (uint64_t)__double_as_longlong(-__longlong_as_double((long long)x)) : (uint64_t)0 - x;
                    else if (op == VNM_EX_BNOT) x = ~x;
                    else x ^= 1ULL;
                    if (in.nar >= 0) x = pj_narrow<MATH>(in.nar, x);
                    tos[r] = x;
                }
            } else if (MATH > 0 && op >= VNM_EX_ABS && op != VNM_EX_POW) {
                // ---- unary built-in function ----
                if (op == VNM_EX_ABS || op == VNM_EX_SQRT || op >= VNM_EX_TO_F64) {
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        uint64_t x = pj_math1(op, in.cvt_a, in.cmp == 1, tos[r]);
                        if (in.nar >= 0) x = pj_narrow<MATH>(in.nar, x);
                        tos[r] = x;
                    }
                } else if (MATH == 2) {
                    // transcendentals: one row at a time through the free LDS level sp - 1, so ONE copy of the OCML code
                    // holds registers (unrolled over the PJ_R rows, interleaved copies cut the occupancy of every MATH program)
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) STK(sp - 1, r) = tos[r];
#pragma unroll 1
                    for (int r = 0; r < PJ_R; r++) {
                        uint64_t x = pj_math_t(op, in.cvt_a, in.cmp == 1, STK(sp - 1, r));
                        if (in.nar >= 0) x = pj_narrow<MATH>(in.nar, x);
                        STK(sp - 1, r) = x;
                    }
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) tos[r] = STK(sp - 1, r);
                }
            } else if (op == VNM_EX_STORE) {
                // ---- pop into an output column ----
                if (MATH > 0 && a.out_type[in.arg] == VNM_OUT_F16) {
                    _Float16* o = (_Float16*)a.out[in.arg];
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        if (row < a.length) o[row] = (_Float16)pj_bitsd(tos[r]);   // exact: the word holds a half
                    }
                } else if (a.out_is_mask[in.arg]) {
                    uint8_t* o = (uint8_t*)a.out[in.arg];
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        if (row < a.length) o[row] = (uint8_t)tos[r];
                    }
                } else if (type_width(a.out_type[in.arg]) != 8) {
                    // narrow output types: typed scalar stores (float32 values are held as float64)
                    const int ot = a.out_type[in.arg];
                    void* o = a.out[in.arg];
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        if (row >= a.length) continue;
                        if (ot == VNM_F32) ((float*)o)[row] = (float)__longlong_as_double((long long)tos[r]);
                        else if (type_width(ot) == 4) ((uint32_t*)o)[row] = (uint32_t)tos[r];
                        else if (type_width(ot) == 2) ((uint16_t*)o)[row] = (uint16_t)tos[r];
                        else ((uint8_t*)o)[row] = (uint8_t)tos[r];
                    }
                } else if (full_tile) {
                    uint64_t* o = (uint64_t*)a.out[in.arg] + base;
#pragma unroll
                    for (int k = 0; k < PJ_R / 2; k++) {
                        ulonglong2 t;
                        t.x = tos[2 * k];
                        t.y = tos[2 * k + 1];
                        *(ulonglong2*)(o + k * (2 * PJ_BLOCK)) = t;
                    }
                } else {
                    uint64_t* o = (uint64_t*)a.out[in.arg];
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) {
                        const int64_t row = base + (r >> 1) * (2 * PJ_BLOCK) + (r & 1);
                        if (row < a.length) o[row] = tos[r];
                    }
                }
                sp--;
                if (sp > 0) {
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) tos[r] = STK(sp - 1, r);
                }
            } else {
                // ---- binary: a = value below the top (LDS), b = top (registers) ----
                sp--;
                const bool cmp = op >= VNM_EX_EQ && op <= VNM_EX_LE;
                const bool as_f = cmp ? (in.cvt_a || in.cvt_b || in.arg) : in.is_f != 0;
                if (MATH == 2 && op == VNM_EX_POW) {
                    // np.power, one row at a time like the transcendentals (b goes to the free LDS level sp)
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) STK(sp, r) = tos[r];
#pragma unroll 1
                    for (int r = 0; r < PJ_R; r++) {
                        const uint64_t xa = STK(sp - 1, r);
                        const uint64_t xb = STK(sp, r);
                        uint64_t res;
                        if (as_f) {
                            const double da = pj_as_f64(in.cvt_a, xa), db = pj_as_f64(in.cvt_b, xb);
                            res = pj_dbits(in.cmp == 1 ? (double)(float)pow(da, db) : pow(da, db));   // float64, rounded as above
                        } else if (in.arg == 1 && (int64_t)xb < 0) {
                            *a.neg_pow = 1;   // "Integers to negative integer powers are not allowed." (the host raises)
                            res = 0;
                        } else {
                            res = pj_ipow(xa, xb);
                        }
                        if (in.nar >= 0) res = pj_narrow<MATH>(in.nar, res);
                        STK(sp, r) = res;
                    }
#pragma unroll
                    for (int r = 0; r < PJ_R; r++) tos[r] = STK(sp, r);
                    continue;
                }
#pragma unroll
                for (int r = 0; r < PJ_R; r++) {
                    const uint64_t xa = STK(sp - 1, r);
                    const uint64_t xb = tos[r];
                    uint64_t res;
                    if (op == VNM_EX_AND) res = xa & xb;
                    else if (op == VNM_EX_OR) res = xa | xb;
                    else if (as_f) {
                        double da = in.cvt_a ? (in.cvt_a == 2 ? (double)xa : (double)(int64_t)xa) : __longlong_as_double((long long)xa);
                        double db = in.cvt_b ? (in.cvt_b == 2 ? (double)xb : (double)(int64_t)xb) : __longlong_as_double((long long)xb);
                        if (cmp) res = cmp_apply<double>(op - VNM_EX_EQ, da, db) ? 1ULL : 0ULL;  // same order as enum vnm_cmp_op
                        else {
                            double d;
                            switch (op) {
                                case VNM_EX_ADD: d = da + db; break;
                                case VNM_EX_SUB: d = da - db; break;
                                case VNM_EX_MUL: d = da * db; break;
                                case VNM_EX_DIV: d = da / db; break;
                                default: d = np_fmod(da, db); break;
                            }
                            res = (uint64_t)__double_as_longlong(d);
                        }
                    } else if (cmp) {
                        bool t;
                        switch (in.cmp) {
                            case 2: t = cmp_apply<uint64_t>(op - VNM_EX_EQ, xa, xb); break;
                            case 3:  // a uint64, b signed: a negative b is below every a
                                t = (int64_t)xb < 0 ? (op == VNM_EX_NE || op == VNM_EX_GT || op == VNM_EX_GE) : cmp_apply<uint64_t>(op - VNM_EX_EQ, xa, xb);
                                break;
                            case 4:
                                t = (int64_t)xa < 0 ? (op == VNM_EX_NE || op == VNM_EX_LT || op == VNM_EX_LE) : cmp_apply<uint64_t>(op - VNM_EX_EQ, xa, xb);
                                break;
                            default: t = cmp_apply<int64_t>(op - VNM_EX_EQ, (int64_t)xa, (int64_t)xb); break;
                        }
                        res = t ? 1ULL : 0ULL;
                    } else {
                        switch (op) {
                            case VNM_EX_ADD: res = xa + xb; break;
                            case VNM_EX_SUB: res = xa - xb; break;
                            case VNM_EX_MUL: res = xa * xb; break;
                            case VNM_EX_MOD: res = in.cmp == 2 ? np_umod(xa, xb) : (uint64_t)np_imod((int64_t)xa, (int64_t)xb); break;
                            case VNM_EX_BAND: res = xa & xb; break;
                            case VNM_EX_BOR: res = xa | xb; break;
                            default: res = xa ^ xb; break;
                        }
                    }
                    if (in.nar >= 0) res = pj_narrow<MATH>(in.nar, res);
                    tos[r] = res;
                }
            }
        }
    }
#undef STK
}

}  // namespace vnm

using namespace vnm;

// The nine instantiations, [lookup level][math level]: the entry's function is what gets the raised LDS limit AND what is launched;
// its name is what the profile shows (the lookup level names a program before its math level does).
using ProjectKernel = void (*)(ProjArgs);
struct ProjectKernelEntry {
    ProjectKernel fn;
    const char* timer;
};
// Not needed for correctness: the table below would instantiate the same nine kernels by naming them.  Spelled out only to keep them in
// the code object in the order they have always had (same code per kernel either way), so that its assembly compares equal line by
// line with the one before the host side was split.
template __global__ void vnm::project_kernel<2, 2>(ProjArgs); template __global__ void vnm::project_kernel<1, 2>(ProjArgs); template __global__ void vnm::project_kernel<0, 2>(ProjArgs);
template __global__ void vnm::project_kernel<2, 1>(ProjArgs); template __global__ void vnm::project_kernel<1, 1>(ProjArgs); template __global__ void vnm::project_kernel<0, 1>(ProjArgs);
template __global__ void vnm::project_kernel<2, 0>(ProjArgs); template __global__ void vnm::project_kernel<1, 0>(ProjArgs); template __global__ void vnm::project_kernel<0, 0>(ProjArgs);
static const ProjectKernelEntry PJ_KERNELS[3][3] = {
    {{project_kernel<0, 0>, "project_kernel"}, {project_kernel<1, 0>, "project_kernel_exact_fn"}, {project_kernel<2, 0>, "project_kernel_math"}},
    {{project_kernel<0, 1>, "project_kernel_lookup"}, {project_kernel<1, 1>, "project_kernel_lookup"}, {project_kernel<2, 1>, "project_kernel_lookup"}},
    {{project_kernel<0, 2>, "project_kernel_lookup_i32"}, {project_kernel<1, 2>, "project_kernel_lookup_i32"}, {project_kernel<2, 2>, "project_kernel_lookup_i32"}},
};

// ONE workgroup per tile: a workgroup loads, computes and stores with nothing of its own to overlap, so it is the
// dispatcher that keeps the memory system busy (three expressions over 1e9 rows: 8 workgroups per CU looping over tiles
// 11.15 ms, 32 per CU 10.2, 128 per CU 9.7, one per tile 9.27 = 5.2 TB/s)
static int project_grid(int64_t length) {
    const int64_t grid64 = getenv("VNM_PJ_GRID") ? (int64_t)device_info().num_cus * atoi(getenv("VNM_PJ_GRID")) : (int64_t)1 << 30;
    const int64_t need = (length + PJ_TILE - 1) / PJ_TILE;
    return (int)grid64 > need ? (int)need : (int)grid64;
}

static int project_launch(ProjArgs& a, const PjTyped& t, hipStream_t s) {
    const ProjectKernelEntry& k = PJ_KERNELS[t.lookup][t.math];
    // depth - 1 levels below the register top; MATH programs stage the top through one more level
    const size_t lds = (size_t)(t.math ? t.depth : (t.depth > 1 ? t.depth - 1 : 1)) * PJ_R * PJ_BLOCK * 8;
    const int grid = project_grid(a.length);
    if (lds > 64 * 1024)   // depth >= 10: beyond the default dynamic LDS limit
        VNM_HIP(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PoolScope scope;
    if (t.pow_check) {   // an integer power with a signed exponent column: the kernel reports a negative exponent
        a.neg_pow = (int*)scope.take(sizeof(int));
        if (!a.neg_pow) return 1;
        VNM_HIP(hipMemsetAsync(a.neg_pow, 0, sizeof(int), s));
    }
    {
        KernelTimer timer(k.timer, s);
        k.fn<<<grid, PJ_BLOCK, lds, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    if (t.pow_check) {
        int neg = 0;
        VNM_HIP(hipMemcpyAsync(&neg, a.neg_pow, sizeof(int), hipMemcpyDeviceToHost, s));
        VNM_HIP(hipStreamSynchronize(s));
        if (neg) return set_error("ValueError: Integers to negative integer powers are not allowed.");
    }
    return 0;
}

// Type the program (vnm_project_type.hpp), then launch the instantiation its lookup and math levels name.  `single`: the program is
// one expression without a STORE; out index 0 is implied.
static int project_impl(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                        int n_out, void** out_values, int* out_types, bool single, void* stream) {
    PjTyped typed;
    const std::string err = pj_type_program(n_ins, program, n_cols, cols, length, n_out, single, typed);
    if (!err.empty()) return set_error("%s", err.c_str());
    if (out_types) std::copy(typed.out_types, typed.out_types + n_out, out_types);
    // typing needs no device: a zero-length call type-checks a program (result types, NumPy's errors) on any host
    if (length <= 0) return 0;
    VNM_TRY(ensure_init());
    if (typed.pow_check && typed.math != 2) return set_error("vnm_project: internal error (power outside the MATH kernel)");
    ProjArgs a{};
    a.n_ins = typed.n_ins;
    a.n_cols = n_cols;
    a.length = length;
    std::copy(typed.ins, typed.ins + typed.n_ins, a.ins);
    std::copy(cols, cols + n_cols, a.cols);
    std::copy(out_values, out_values + n_out, a.out);
    memcpy(a.out_is_mask, typed.out_is_mask, sizeof(a.out_is_mask));
    memcpy(a.out_type, typed.out_type, sizeof(a.out_type));
    return project_launch(a, typed, as_stream(stream));
}

extern "C" {

int vnm_project(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                void* out_values, int* out_type, void* stream) {
    void* outs[1] = {out_values};
    return project_impl(n_ins, program, n_cols, cols, length, 1, outs, out_type, true, stream);
}

int vnm_project_multi(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                      int n_out, void** out_values, int* out_types, void* stream) {
    if (!out_values) return set_error("vnm_project_multi: null argument");
    return project_impl(n_ins, program, n_cols, cols, length, n_out, out_values, out_types, false, stream);
}

}  // extern "C"
