// The host half of the projection (vnm_project.hip): the abstract interpretation that gives every stack slot of a postfix program a
// type -- the ten numeric types with NumPy 2's promotion, "weak" Python literals, bool masks, float16 values -- and rewrites it into
// the typed program the kernel runs.  Nothing here touches the device or the library's error state: a step that can fail returns its
// message (empty: fine) and the caller reports it.  tests/project_type_main.cpp runs all of it under AddressSanitizer without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/vinum_hip.h"
#include "vnm_types.hpp"

namespace vnm {

constexpr int PJ_MAX_INS = VNM_PROJECT_MAX_INS;
constexpr int PJ_MAX_COLS = VNM_PROJECT_MAX_COLS;
constexpr int PJ_MAX_OUT = VNM_PROJECT_MAX_OUT;
constexpr int PJ_STACK = 12;
constexpr int PJ_NOP = -1;   // an instruction folded away by the host (unary operator on a literal)

struct PIns {
    int op;
    int arg;
    int is_f;    // result (or pushed value) is held as float64 bits
    int cvt_a;   // convert operand a (deeper) to float64 first: 1 from int64, 2 from uint64
    int cvt_b;   // ... operand b (top)
    int nar;     // bring the result back into this vnm_type's range (-1: it already is)
    int cmp;     // comparisons: 0 int64, 1 float64, 2 uint64, 3 a is uint64 / b signed, 4 a signed / b is uint64
    double imm_f;
    int64_t imm_i;
};

// a typed program and what the launch needs to know about it
struct PjTyped {
    PIns ins[PJ_MAX_INS];
    int n_ins = 0;                    // the implied STORE of a `single` program included
    int depth = 1;                    // the deepest the stack gets
    int math = 0;                     // the kernel instantiation: 1 exact built-ins / float16 values, 2 transcendentals or power
    int lookup = 0;                   // ... 1 a uint8 lookup, 2 an int32 lookup
    bool pow_check = false;           // an integer power with a signed exponent column: the kernel reports a negative exponent
    uint8_t out_is_mask[PJ_MAX_OUT];  // predicate outputs are byte masks
    uint8_t out_type[PJ_MAX_OUT];     // vnm_type of a value output (its width decides the store), or VNM_OUT_F16
    int out_types[PJ_MAX_OUT];        // what the ABI returns per output: a vnm_type, VNM_MASK_U8 or VNM_OUT_F16
};

__attribute__((format(printf, 1, 2))) inline std::string pj_msg(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// 0..9 = vnm_type; bool mask; weak Python int / float literal; float16 value
enum { PJ_T_B = 10, PJ_T_WI = 11, PJ_T_WF = 12, PJ_T_F16 = 13 };

// np.result_type of two column types (NumPy 2 / NEP 50; probed table in profiles/numpy_promotion_r02.txt)
inline int pj_promote(int a, int b) {
    if (a == b) return a;
    const bool fa = type_is_float(a), fb = type_is_float(b);
    if (fa && fb) return VNM_F64;
    if (fa || fb) {
        const int f = fa ? a : b, i = fa ? b : a;
        if (f == VNM_F64) return VNM_F64;
        return type_width(i) <= 2 ? VNM_F32 : VNM_F64;
    }
    const bool ua = type_is_unsigned(a), ub = type_is_unsigned(b);
    const int wa = type_width(a), wb = type_width(b);
    if (ua == ub) return wa >= wb ? a : b;
    const int u = ua ? a : b, sg = ua ? b : a;
    if (type_width(u) < type_width(sg)) return sg;
    switch (u) {
        case VNM_U8: return VNM_I16;
        case VNM_U16: return VNM_I32;
        case VNM_U32: return VNM_I64;
        default: return VNM_F64;   // uint64 with a signed type
    }
}
// the same with float16 values (results of sqrt / sin / ... over 8-bit integers): float16 survives 8-bit integers and
// float16, float32 16-bit integers and float32, everything else goes to float64
inline int pj_promote_h(int a, int b) {
    if (a != PJ_T_F16 && b != PJ_T_F16) return pj_promote(a, b);
    const int o = a == PJ_T_F16 ? b : a;
    if (o == PJ_T_F16) return PJ_T_F16;
    if (type_is_float(o)) return o;
    return type_width(o) == 1 ? (int)PJ_T_F16 : type_width(o) == 2 ? (int)VNM_F32 : (int)VNM_F64;
}
inline const char* pj_type_name(int t) {
    static const char* n[] = {"int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64"};
    return t >= 0 && t < 10 ? n[t] : "?";
}
inline bool pj_int_fits(int t, int64_t v) {
    switch (t) {
        case VNM_I8: return v >= -128 && v <= 127;
        case VNM_I16: return v >= -32768 && v <= 32767;
        case VNM_I32: return v >= INT32_MIN && v <= INT32_MAX;
        case VNM_U8: return v >= 0 && v <= 255;
        case VNM_U16: return v >= 0 && v <= 65535;
        case VNM_U32: return v >= 0 && v <= (int64_t)UINT32_MAX;
        case VNM_U64: return v >= 0;
        default: return true;
    }
}
// the float16 nearest to d (ties to even, beyond 65504 + half a step: infinity), as a double: npy_double_to_half, one rounding straight
// from double.  Spelled out because not every host compiler has a half type.
inline double pj_round_f16(double d) {
    if (std::isnan(d)) {   // quiet, the payload cut to what a half holds
        uint64_t b;
        memcpy(&b, &d, 8);
        b = (b & 0xFFFFFC0000000000ULL) | 0x0008000000000000ULL;
        memcpy(&d, &b, 8);
        return d;
    }
    if (std::isinf(d)) return d;
    int e;
    std::frexp(d, &e);   // |d| in [2^(e-1), 2^e)
    const double step = std::ldexp(1.0, std::max(e - 1, -14) - 10);   // the spacing of halves there (subnormals: 2^-24)
    const double r = std::nearbyint(d / step) * step;
    return std::fabs(r) > 65504.0 ? std::copysign(INFINITY, d) : r;
}
inline int pj_strong(int t) { return t == PJ_T_WI ? (int)VNM_I64 : t == PJ_T_WF ? (int)VNM_F64 : t; }   // what NumPy makes of a Python scalar on its own
inline bool pj_is_float(int t) { return t == PJ_T_F16 || (t < 10 && type_is_float(t)); }
inline bool pj_held_f(int t) { return t == PJ_T_WF || pj_is_float(t); }   // held as float64 bits
inline bool pj_is_weak(int t) { return t == PJ_T_WI || t == PJ_T_WF; }

// The lookup tables of VNM_EX_LOOKUP_U8 / _I32 are columns of their own length (one entry per dictionary id); every other column is
// a row column of the batch.  Finds the tables (is_table[n_cols]) and the lookup level, checks every column.
inline std::string pj_check_columns(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length,
                                    bool* is_table, int* lookup) {
    int table_type[PJ_MAX_COLS] = {};
    for (int i = 0; i < n_ins; i++) {
        if (program[i].op != VNM_EX_LOOKUP_U8 && program[i].op != VNM_EX_LOOKUP_I32) continue;
        const int64_t t = program[i].imm_i;
        const int want = program[i].op == VNM_EX_LOOKUP_U8 ? VNM_U8 : VNM_I32;
        if (t < 0 || t >= n_cols) return pj_msg("vnm_project: lookup table index %lld out of range", (long long)t);
        if (program[i].arg == t) return pj_msg("vnm_project: a lookup reads its codes from its own table");
        if (is_table[t] && table_type[t] != want) return pj_msg("vnm_project: lookup table %lld is read as uint8 and as int32", (long long)t);
        is_table[t] = true;
        table_type[t] = want;
        *lookup = std::max(*lookup, want == VNM_U8 ? 1 : 2);
    }
    for (int c = 0; c < n_cols; c++) {
        if (cols[c].type < VNM_I8 || cols[c].type > VNM_F64) return pj_msg("vnm_project: column %d: unsupported type %d", c, cols[c].type);
        if (is_table[c]) {
            if (cols[c].type != table_type[c] || cols[c].validity || cols[c].offset < 0 || cols[c].length < 0)
                return pj_msg("vnm_project: lookup table %d must be %s column without NULLs", c, table_type[c] == VNM_U8 ? "a uint8" : "an int32");
        } else if (cols[c].length != length) return pj_msg("Select expressions have unequal sizes. This is not permitted.");
    }
    return "";
}

// The interpreter: one member function per opcode class, each leaves the typed instruction in `o` and the stack as the kernel's will be.
struct PjTyper {
    struct Slot {
        int ty;    // 0..9 = vnm_type, or PJ_T_*
        int lit;   // the instruction that pushed a weak literal still unchanged on the stack (-1: none)
        int cst;   // the CONST instruction that pushed the slot's value, weak or strong, still unchanged (-1: none)
    };
    PjTyped& out;
    const vnm_dcol* cols;
    int n_cols, n_out;
    bool is_table[PJ_MAX_COLS] = {};
    bool stored[PJ_MAX_OUT] = {};
    Slot st[PJ_STACK];
    int sp = 0;

    PjTyper(PjTyped& typed, const vnm_dcol* columns, int n_columns, int n_outputs) : out(typed), cols(columns), n_cols(n_columns), n_out(n_outputs) {}

    Slot& top(int below = 0) { return st[sp - 1 - below]; }
    void replace_top(int t) { top() = Slot{t, -1, -1}; }
    static std::string underflow() { return "vnm_project: malformed program (stack underflow)"; }

    // the column operand of a push is a row column (`codes`: of int32 dictionary codes)
    std::string check_row_column(int col, bool codes) const {
        if (col < 0 || col >= n_cols) return pj_msg("vnm_project: column index %d out of range", col);
        if (is_table[col]) return pj_msg("vnm_project: column %d is a lookup table, not a row column", col);
        if (codes && cols[col].type != VNM_I32) return pj_msg("vnm_project: a lookup reads int32 dictionary codes (column %d)", col);
        return "";
    }
    std::string check_room() const { return sp >= PJ_STACK ? "vnm_project: expression too deep" : ""; }
    // a weak literal meets a float32 column or a float16 value: NumPy casts the scalar to that type first
    void round_lit(int slot, int t) {
        if (st[slot].lit < 0 || (t != VNM_F32 && t != PJ_T_F16)) return;
        PIns& p = out.ins[st[slot].lit];
        // (an integer goes to float32 in ONE rounding; on its way to float16 it passes through double, as it always has)
        if (t == VNM_F32) p.imm_f = p.op == VNM_EX_CONST_I ? (double)(float)p.imm_i : (double)(float)p.imm_f;
        else p.imm_f = pj_round_f16(p.op == VNM_EX_CONST_I ? (double)p.imm_i : p.imm_f);
        if (p.op == VNM_EX_CONST_I) { p.op = VNM_EX_CONST_F; p.is_f = 1; }
    }
    // how the kernel turns the word of slot `slot` into a double: 0 it holds float64 bits, 1 from int64, 2 from uint64
    int operand_cvt(int slot) const {
        // the literal may just have become a float constant: ask the instruction, not the type
        const bool f = pj_held_f(st[slot].ty) || (st[slot].lit >= 0 && out.ins[st[slot].lit].op == VNM_EX_CONST_F);
        return f ? 0 : cvt_of(st[slot].ty);
    }
    static int cvt_of(int t) { return pj_held_f(t) ? 0 : (t == VNM_U64 ? 2 : 1); }

    std::string push_column(const vnm_expr_ins& in, PIns& o) {
        std::string err = check_row_column(in.arg, false);
        if (err.empty()) err = check_room();
        if (!err.empty()) return err;
        int t = cols[in.arg].type;
        if (cols[in.arg].validity != nullptr && !type_is_float(t)) t = VNM_F64;   // NULL -> NaN needs a float (record_batch.py:112-118)
        o.is_f = type_is_float(t);
        st[sp++] = Slot{t, -1, -1};
        return "";
    }
    std::string push_constant(int i, const vnm_expr_ins& in, PIns& o) {
        const std::string err = check_room();
        if (!err.empty()) return err;
        o.is_f = in.op == VNM_EX_CONST_F;
        // arg = 1: a STRONG constant (an element of the array np.isin builds from an IN list): int64 / float64
        const int weak = o.is_f ? PJ_T_WF : PJ_T_WI;
        st[sp++] = Slot{in.arg == 1 ? pj_strong(weak) : weak, in.arg == 1 ? -1 : i, i};
        o.arg = 0;
        return "";
    }
    std::string push_lookup_or_null_test(const vnm_expr_ins& in, PIns& o) {
        const bool i32 = in.op == VNM_EX_LOOKUP_I32;
        std::string err = check_row_column(in.arg, i32 || in.op == VNM_EX_LOOKUP_U8);
        if (err.empty()) err = check_room();
        if (!err.empty()) return err;
        o.is_f = i32;                                             // an int32 value that can be NULL: float64, NaN
        st[sp++] = Slot{i32 ? (int)VNM_F64 : (int)PJ_T_B, -1, -1};
        return "";
    }
    std::string sign_or_invert(const vnm_expr_ins& in, PIns& o) {
        if (sp < 1) return underflow();
        const int t = top().ty;
        if (t == PJ_T_B) return "vnm_project: arithmetic on a boolean mask is not supported";
        if (in.op == VNM_EX_BNOT && pj_held_f(t)) return "ufunc 'invert' not supported for float inputs";
        if (t >= PJ_T_WI && top().lit >= 0) {
            // a Python literal: folded here.  `~5` stays a (weak) Python int; np.negative(5) RETURNS a NumPy scalar,
            // np.int64 / np.float64, which is a strong type from then on
            PIns& c = out.ins[top().lit];
            if (in.op == VNM_EX_BNOT) c.imm_i = ~c.imm_i;
            else {
                if (c.op == VNM_EX_CONST_I) c.imm_i = (int64_t)(0 - (uint64_t)c.imm_i);
                else c.imm_f = -c.imm_f;
                top().ty = c.op == VNM_EX_CONST_I ? VNM_I64 : VNM_F64;
                top().lit = -1;
            }
            o.op = PJ_NOP;
            return "";
        }
        o.is_f = pj_held_f(t);
        if (t < 10 && !type_is_float(t) && type_width(t) < 8) o.nar = t;
        replace_top(t);
        return "";
    }
    std::string builtin_or_cast(const vnm_expr_ins& in, PIns& o) {
        if (sp < 1) return underflow();
        const bool cast = in.op >= VNM_EX_TO_F64;
        const bool trans = !cast && in.op != VNM_EX_ABS && in.op != VNM_EX_SQRT;
        out.math = std::max(out.math, trans ? 2 : 1);
        if (top().ty == PJ_T_B && !cast) return "vnm_project: arithmetic on a boolean mask is not supported";
        const int t = pj_strong(top().ty);    // a NumPy ufunc / np.array over a Python scalar: int64 / float64
        o.cvt_a = t == PJ_T_B ? 1 : cvt_of(t);
        int rt;
        if (in.op == VNM_EX_ABS) {
            rt = t;
            if (type_is_unsigned(t)) o.op = PJ_NOP;                       // the identity
            else if (!pj_is_float(t) && type_width(t) < 8) o.nar = t;     // abs(int8 -128) == -128
        } else if (in.op == VNM_EX_TO_F64) rt = VNM_F64;
        else if (in.op == VNM_EX_TO_I64) rt = VNM_I64;
        else if (in.op == VNM_EX_TO_BOOL) rt = PJ_T_B;
        else {
            rt = pj_is_float(t) ? t : type_width(t) == 1 ? (int)PJ_T_F16 : type_width(t) == 2 ? (int)VNM_F32 : (int)VNM_F64;
            o.cmp = rt != VNM_F64 ? 1 : 0;                               // float32 arithmetic, NumPy's f / e loops
            if (rt == PJ_T_F16) o.nar = VNM_OUT_F16;
        }
        o.is_f = pj_held_f(rt);
        replace_top(rt);
        return "";
    }
    std::string logical(const vnm_expr_ins& in) {
        if (in.op == VNM_EX_NOT) {
            if (sp < 1) return underflow();
            return top().ty != PJ_T_B ? "NOT expects a boolean operand" : "";
        }
        if (sp < 2) return underflow();
        if (top().ty != PJ_T_B || top(1).ty != PJ_T_B) return "AND / OR expect boolean operands";
        sp--;
        return "";
    }
    std::string comparison(PIns& o) {
        if (sp < 2) return underflow();
        const int tb = top().ty, ta = top(1).ty;
        if (ta == PJ_T_B || tb == PJ_T_B) return "vnm_project: comparing boolean masks is not supported";
        // a float32 column against a Python literal compares in float32
        if (pj_is_weak(tb)) round_lit(sp - 1, ta);
        if (pj_is_weak(ta)) round_lit(sp - 2, tb);
        const bool anyf = pj_held_f(ta) || pj_held_f(tb);
        if (anyf) {  // NumPy compares in float64 as soon as one side is float (float32 values are exact float64s)
            o.cmp = 1;
            o.cvt_a = operand_cvt(sp - 2);
            o.cvt_b = operand_cvt(sp - 1);
        } else {     // integers compare exactly, int64 against uint64 included
            const bool ua = ta == VNM_U64, ub = tb == VNM_U64;
            const bool sa = ta == PJ_T_WI || (ta < 10 && !type_is_unsigned(ta)), sb = tb == PJ_T_WI || (tb < 10 && !type_is_unsigned(tb));
            o.cmp = (ua && ub) ? 2 : (ua && sb) ? 3 : (sa && ub) ? 4 : (ua || ub) ? 2 : 0;
        }
        o.arg = anyf ? 1 : 0;
        sp--;
        replace_top(PJ_T_B);
        return "";
    }
    // the result type of a binary arithmetic operator before `/` and the bitwise rule; a weak literal is range-checked and rounded
    std::string arithmetic_type(int op, int* rt) {
        const int tb = top().ty, ta = top(1).ty;
        const bool wa = pj_is_weak(ta), wb = pj_is_weak(tb);
        if (wa && wb) *rt = (ta == PJ_T_WF || tb == PJ_T_WF) ? VNM_F64 : VNM_I64;       // Python scalars: default int64 / float64
        else if (wa || wb) {
            const int w = wa ? ta : tb, t = wa ? tb : ta, wslot = wa ? sp - 2 : sp - 1;
            if (w == PJ_T_WI) {
                *rt = t;                                                              // the literal takes the column's type
                // true division runs in float64 whatever the integer width: NumPy converts the literal to double, no range check
                if (op != VNM_EX_DIV && !pj_is_float(t) && st[wslot].lit >= 0 && !pj_int_fits(t, out.ins[st[wslot].lit].imm_i))
                    return pj_msg("OverflowError: Python integer %lld out of bounds for %s", (long long)out.ins[st[wslot].lit].imm_i, pj_type_name(t));
            } else *rt = (t == VNM_F32 || t == PJ_T_F16) ? t : (int)VNM_F64;
            round_lit(wslot, t);
        } else *rt = pj_promote_h(ta, tb);
        return "";
    }
    std::string arithmetic(const vnm_expr_ins& in, PIns& o) {
        if (sp < 2) return underflow();
        const int tb = top().ty, ta = top(1).ty;
        if (ta == PJ_T_B || tb == PJ_T_B) return "vnm_project: arithmetic on a boolean mask is not supported";
        int rt;
        const std::string err = arithmetic_type(in.op, &rt);
        if (!err.empty()) return err;
        const bool bitop = in.op >= VNM_EX_BAND && in.op <= VNM_EX_BXOR;
        if (bitop && (pj_is_float(rt) || pj_held_f(ta) || pj_held_f(tb))) return "ufunc 'bitwise' not supported for float inputs";
        if (in.op == VNM_EX_DIV && !pj_is_float(rt)) rt = VNM_F64;
        const bool rf = pj_is_float(rt);
        if (in.op == VNM_EX_POW) {
            out.math = 2;
            if (!rf) {
                // integer ** negative integer: NumPy's ValueError -- a constant exponent here, a column in the kernel
                const int c = top().cst;
                if (c >= 0 && out.ins[c].op == VNM_EX_CONST_I && out.ins[c].imm_i < 0)
                    return "ValueError: Integers to negative integer powers are not allowed.";
                if (c < 0 && !type_is_unsigned(tb)) { o.arg = 1; out.pow_check = true; }
            } else if (rt != VNM_F64) o.cmp = 1;   // float32 arithmetic (float32 and float16 results)
        }
        o.is_f = rf;
        if (rf) {
            o.cvt_a = operand_cvt(sp - 2);
            o.cvt_b = operand_cvt(sp - 1);
        }
        if (rt == VNM_F32 || (!rf && type_width(rt) < 8)) o.nar = rt;
        if (rt == PJ_T_F16) { o.nar = VNM_OUT_F16; out.math = std::max(out.math, 1); }
        if (rt == VNM_U64 && in.op == VNM_EX_MOD) o.cmp = 2;   // unsigned modulo
        sp--;
        replace_top(rt);
        return "";
    }
    std::string store(const vnm_expr_ins& in, bool foreign) {
        if (foreign) return "vnm_project: VNM_EX_STORE belongs to vnm_project_multi programs";
        if (sp < 1) return underflow();
        if (in.arg < 0 || in.arg >= n_out) return pj_msg("vnm_project: output index %d out of range", in.arg);
        if (stored[in.arg]) return pj_msg("vnm_project: output %d stored twice", in.arg);
        stored[in.arg] = true;
        int t = pj_strong(top().ty);           // np.repeat(5, n) -> int64, np.repeat(5.0, n) -> float64 (algebra.py:77-87)
        if (t == PJ_T_F16) t = VNM_OUT_F16;
        out.out_is_mask[in.arg] = t == PJ_T_B;
        out.out_type[in.arg] = t == PJ_T_B ? (int)VNM_U8 : t;
        out.out_types[in.arg] = t == PJ_T_B ? VNM_MASK_U8 : t;
        sp--;
        return "";
    }
    // instruction i: `foreign_store`, a STORE written into a program whose only STORE is implied
    std::string step(int i, const vnm_expr_ins& in, bool foreign_store) {
        PIns& o = out.ins[i];
        o = PIns{in.op, in.arg, 0, 0, 0, -1, 0, in.imm_f, in.imm_i};
        switch (in.op) {
            case VNM_EX_COL: return push_column(in, o);
            case VNM_EX_CONST_F: case VNM_EX_CONST_I: return push_constant(i, in, o);
            case VNM_EX_LOOKUP_U8: case VNM_EX_LOOKUP_I32: case VNM_EX_IS_NULL: case VNM_EX_IS_NOT_NULL: return push_lookup_or_null_test(in, o);
            case VNM_EX_NEG: case VNM_EX_BNOT: return sign_or_invert(in, o);
            case VNM_EX_ABS: case VNM_EX_SQRT: case VNM_EX_SIN: case VNM_EX_COS: case VNM_EX_TAN: case VNM_EX_LOG:
            case VNM_EX_LOG2: case VNM_EX_LOG10: case VNM_EX_TO_F64: case VNM_EX_TO_I64: case VNM_EX_TO_BOOL: return builtin_or_cast(in, o);
            case VNM_EX_NOT: case VNM_EX_AND: case VNM_EX_OR: return logical(in);
            case VNM_EX_EQ: case VNM_EX_NE: case VNM_EX_GT: case VNM_EX_GE: case VNM_EX_LT: case VNM_EX_LE: return comparison(o);
            case VNM_EX_ADD: case VNM_EX_SUB: case VNM_EX_MUL: case VNM_EX_DIV: case VNM_EX_MOD:
            case VNM_EX_BAND: case VNM_EX_BOR: case VNM_EX_BXOR: case VNM_EX_POW: return arithmetic(in, o);
            case VNM_EX_STORE: return store(in, foreign_store);
            default: return pj_msg("vnm_project: unknown opcode %d", in.op);
        }
    }
};

// Types `program` over `cols` into `out`.  `single`: the program is one expression without a STORE; out index 0 is implied.  Needs no
// device, so a zero-length call type-checks a program (result types, NumPy's errors) on any host.  Returns the message of the first
// fault, empty when the program is fine; `out` is complete only then.
inline std::string pj_type_program(int n_ins, const vnm_expr_ins* program, int n_cols, const vnm_dcol* cols, int64_t length, int n_out,
                                   bool single, PjTyped& out) {
    if (n_ins <= 0 || n_ins + (single ? 1 : 0) > PJ_MAX_INS)
        return pj_msg("vnm_project: program must have 1..%d instructions", PJ_MAX_INS - (single ? 1 : 0));
    if (n_cols < 0 || n_cols > PJ_MAX_COLS) return pj_msg("vnm_project: at most %d input columns", PJ_MAX_COLS);
    if (n_out < 1 || n_out > PJ_MAX_OUT) return pj_msg("vnm_project: 1..%d outputs per call", PJ_MAX_OUT);
    out = PjTyped{};
    PjTyper ty(out, cols, n_cols, n_out);
    std::string err = pj_check_columns(n_ins, program, n_cols, cols, length, ty.is_table, &out.lookup);
    if (!err.empty()) return err;
    out.n_ins = n_ins + (single ? 1 : 0);
    for (int i = 0; i < out.n_ins; i++) {
        vnm_expr_ins implied{};
        implied.op = VNM_EX_STORE;
        err = ty.step(i, i < n_ins ? program[i] : implied, single && i < n_ins);
        if (!err.empty()) return err;
        out.depth = std::max(out.depth, ty.sp);
    }
    if (ty.sp != 0) return pj_msg("vnm_project: malformed program (final stack depth %d)", ty.sp + (single ? 1 : 0));
    for (int k = 0; k < n_out; k++)
        if (!ty.stored[k]) return pj_msg("vnm_project: output %d is never stored", k);
    return "";
}

}  // namespace vnm
