// The projection's program typer (vinum_amd/csrc/vnm_project_type.hpp) on its own: built with AddressSanitizer and UBSan by
// tests/test_project_type_cpu.py and run as a child process, no GPU and no library.  Types a fixed corpus of programs and prints one
// line per program: every field of every typed instruction, then depth, math, lookup, pow_check and the out types -- or the message
// of a refused program.  The test compares the lines with what the typer printed before it was split out of vnm_project.hip.
#include "../vinum_amd/csrc/vnm_project_type.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace vnm;

static const int64_t ROWS = 5;
static const uint8_t VALIDITY[1] = {0x15};

struct Prog {
    std::vector<vnm_expr_ins> ins;   // exactly as long as the program: a read past it is a heap overflow
    std::vector<vnm_dcol> cols;
    int64_t length = ROWS;
    int n_out = 1;
    bool single = true;
};

static vnm_expr_ins I(int op, int arg = 0, double f = 0.0, int64_t k = 0) {
    vnm_expr_ins in{};
    in.op = op; in.arg = arg; in.imm_f = f; in.imm_i = k;
    return in;
}
static vnm_dcol column(int type, bool nullable, int64_t length = ROWS) {
    vnm_dcol c{};
    c.validity = nullable ? VALIDITY : nullptr;
    c.length = length;
    c.type = type;
    return c;
}

static const int ALL_COLS = -1000;
static void emit(const std::string& label, const Prog& p, int n_cols = ALL_COLS) {
    PjTyped t;
    const std::string err = pj_type_program((int)p.ins.size(), p.ins.data(), n_cols == ALL_COLS ? (int)p.cols.size() : n_cols, p.cols.data(), p.length,
                                            p.n_out, p.single, t);
    if (!err.empty()) { printf("%s|ERR %s\n", label.c_str(), err.c_str()); return; }
    printf("%s|", label.c_str());
    for (int i = 0; i < t.n_ins; i++) {
        const PIns& o = t.ins[i];
        uint64_t bits;
        memcpy(&bits, &o.imm_f, 8);
        printf("%d,%d,%d,%d,%d,%d,%d,%016llx,%lld;", o.op, o.arg, o.is_f, o.cvt_a, o.cvt_b, o.nar, o.cmp, (unsigned long long)bits, (long long)o.imm_i);
    }
    printf("|d=%d m=%d l=%d p=%d|", t.depth, t.math, t.lookup, (int)t.pow_check);
    for (int k = 0; k < p.n_out; k++) printf("%d:%d:%d,", t.out_is_mask[k], t.out_type[k], t.out_types[k]);
    printf("\n");
}

static const int BINARY[] = {VNM_EX_ADD, VNM_EX_SUB, VNM_EX_MUL, VNM_EX_DIV, VNM_EX_MOD, VNM_EX_BAND, VNM_EX_BOR, VNM_EX_BXOR, VNM_EX_EQ,
                             VNM_EX_NE, VNM_EX_GT, VNM_EX_GE, VNM_EX_LT, VNM_EX_LE, VNM_EX_AND, VNM_EX_OR, VNM_EX_POW};
static const int UNARY[] = {VNM_EX_NEG, VNM_EX_BNOT, VNM_EX_NOT, VNM_EX_ABS, VNM_EX_SQRT, VNM_EX_SIN, VNM_EX_COS, VNM_EX_TAN, VNM_EX_LOG,
                            VNM_EX_LOG2, VNM_EX_LOG10, VNM_EX_TO_F64, VNM_EX_TO_I64, VNM_EX_TO_BOOL};
// literals that cross each narrow type's range: 3, -3, 300, 70000, 2^40 as Python ints and floats, 2.5; then integers beyond 2^53
static std::vector<vnm_expr_ins> literals(int strong) {
    std::vector<vnm_expr_ins> v;
    for (int64_t k : {(int64_t)3, (int64_t)-3, (int64_t)300, (int64_t)70000, (int64_t)1 << 40}) {
        v.push_back(I(VNM_EX_CONST_I, strong, 0.0, k));
        v.push_back(I(VNM_EX_CONST_F, strong, (double)k, 0));
    }
    v.push_back(I(VNM_EX_CONST_F, strong, 2.5, 0));
    // integers no double holds: what they become beside a float32 column or a float16 value depends on how often they are rounded
    for (int64_t k : {((int64_t)1 << 60) + ((int64_t)1 << 36) + 1, ((int64_t)1 << 53) + 1, -(((int64_t)1 << 60) + ((int64_t)1 << 36) + 1), INT64_MAX, INT64_MIN})
        v.push_back(I(VNM_EX_CONST_I, strong, 0.0, k));
    return v;
}
static std::string name(const char* cls, std::initializer_list<long long> ids) {
    std::string s = cls;
    for (long long x : ids) s += "/" + std::to_string(x);
    return s;
}

static void two_columns() {
    for (int ta = 0; ta < 10; ta++) for (int na = 0; na < 2; na++) for (int tb = 0; tb < 10; tb++) for (int nb = 0; nb < 2; nb++) for (int op : BINARY) {
        Prog p;
        p.cols = {column(ta, na), column(tb, nb)};
        p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_COL, 1), I(op)};
        emit(name("bin", {ta, na, tb, nb, op}), p);
    }
}
static void one_column() {
    for (int t = 0; t < 10; t++) for (int n = 0; n < 2; n++) for (int op : UNARY) {
        Prog p;
        p.cols = {column(t, n)};
        p.ins = {I(VNM_EX_COL, 0), I(op)};
        emit(name("un", {t, n, op}), p);
    }
}
// a weak (strong = 0) or strong literal on either side of a column; then the literal under a folded NEG / BNOT, and under two
static void column_and_literal() {
    for (int strong = 0; strong < 2; strong++) {
        const std::vector<vnm_expr_ins> lits = literals(strong);
        for (int t = 0; t < 10; t++) for (int n = 0; n < 2; n++) for (size_t l = 0; l < lits.size(); l++) for (int op : BINARY) {
            Prog p;
            p.cols = {column(t, n)};
            p.ins = {I(VNM_EX_COL, 0), lits[l], I(op)};
            emit(name("lit_right", {strong, t, n, (long long)l, op}), p);
            p.ins = {lits[l], I(VNM_EX_COL, 0), I(op)};
            emit(name("lit_left", {strong, t, n, (long long)l, op}), p);
        }
    }
    const vnm_expr_ins few[] = {I(VNM_EX_CONST_I, 0, 0.0, 3), I(VNM_EX_CONST_I, 0, 0.0, -300), I(VNM_EX_CONST_F, 0, 2.5, 0)};
    for (int t = 0; t < 10; t++) for (int n = 0; n < 2; n++) for (int l = 0; l < 3; l++) for (int fold : {VNM_EX_NEG, VNM_EX_BNOT}) for (int op : BINARY) {
        Prog p;
        p.cols = {column(t, n)};
        p.ins = {I(VNM_EX_COL, 0), few[l], I(fold), I(op)};
        emit(name("fold_right", {t, n, l, fold, op}), p);
        p.ins = {few[l], I(fold), I(VNM_EX_COL, 0), I(op)};
        emit(name("fold_left", {t, n, l, fold, op}), p);
        p.ins = {I(VNM_EX_COL, 0), few[l], I(fold), I(fold), I(op)};
        emit(name("fold_twice", {t, n, l, fold, op}), p);
    }
    for (int l = 0; l < 3; l++) for (int m = 0; m < 3; m++) for (int op : BINARY) {   // two literals, and one alone
        Prog p;
        p.ins = {few[l], few[m], I(op)};
        emit(name("lit_lit", {l, m, op}), p);
    }
    for (int l = 0; l < 3; l++) for (int op : UNARY) {
        Prog p;
        p.ins = {few[l], I(op)};
        emit(name("lit_un", {l, op}), p);
    }
}
// float16 values: sqrt / sin of an 8-bit column against a column, a literal, another float16 value, and under every unary opcode
static void float16_values() {
    for (int src : {VNM_U8, VNM_I8}) for (int fn : {VNM_EX_SQRT, VNM_EX_SIN}) {
        for (int t = 0; t < 10; t++) for (int n = 0; n < 2; n++) for (int op : BINARY) {
            Prog p;
            p.cols = {column(src, false), column(t, n)};
            p.ins = {I(VNM_EX_COL, 0), I(fn), I(VNM_EX_COL, 1), I(op)};
            emit(name("f16_col", {src, fn, t, n, op}), p);
            p.ins = {I(VNM_EX_COL, 1), I(VNM_EX_COL, 0), I(fn), I(op)};
            emit(name("col_f16", {src, fn, t, n, op}), p);
        }
        const std::vector<vnm_expr_ins> lits = literals(0);
        for (size_t l = 0; l < lits.size(); l++) for (int op : BINARY) {
            Prog p;
            p.cols = {column(src, false)};
            p.ins = {I(VNM_EX_COL, 0), I(fn), lits[l], I(op)};
            emit(name("f16_lit", {src, fn, (long long)l, op}), p);
            p.ins = {lits[l], I(VNM_EX_COL, 0), I(fn), I(op)};
            emit(name("lit_f16", {src, fn, (long long)l, op}), p);
        }
        for (int op : BINARY) {
            Prog p;
            p.cols = {column(src, false)};
            p.ins = {I(VNM_EX_COL, 0), I(fn), I(VNM_EX_COL, 0), I(VNM_EX_SQRT), I(op)};
            emit(name("f16_f16", {src, fn, op}), p);
        }
        for (int op : UNARY) {
            Prog p;
            p.cols = {column(src, false)};
            p.ins = {I(VNM_EX_COL, 0), I(fn), I(op)};
            emit(name("f16_un", {src, fn, op}), p);
        }
    }
}
// both lookups alone, under NOT, next to the other, and with no / an exact / a transcendental built-in: the nine (lookup, math) cells
static void lookups() {
    for (int lk = 0; lk < 4; lk++) for (int math = 0; math < 3; math++) for (int neg = 0; neg < 2; neg++) for (int nullable = 0; nullable < 2; nullable++) {
        Prog p;
        // (a table has its own length; a column no lookup names is a row column like any other)
        p.cols = {column(VNM_I32, nullable), column(VNM_U8, false, lk & 1 ? 7 : ROWS), column(VNM_I32, false, lk & 2 ? 9 : ROWS), column(VNM_F64, false)};
        if (lk & 1) {
            p.ins.push_back(I(VNM_EX_LOOKUP_U8, 0, 0.0, 1));
            if (neg) p.ins.push_back(I(VNM_EX_NOT));
        }
        if (lk & 2) {
            p.ins.insert(p.ins.end(), {I(VNM_EX_LOOKUP_I32, 0, 0.0, 2), I(VNM_EX_LOOKUP_I32, 0, 0.0, 2), I(neg ? VNM_EX_NE : VNM_EX_LT)});
            if (lk & 1) p.ins.push_back(I(VNM_EX_AND));
        }
        p.ins.push_back(I(VNM_EX_COL, 3));
        if (math) p.ins.push_back(I(math == 1 ? VNM_EX_ABS : VNM_EX_SIN));
        p.ins.insert(p.ins.end(), {I(VNM_EX_CONST_F, 0, 0.5, 0), I(VNM_EX_GT)});
        if (lk) p.ins.push_back(I(VNM_EX_OR));
        emit(name("lookup", {lk, math, neg, nullable}), p);
    }
    Prog p;
    p.cols = {column(VNM_I32, true), column(VNM_U8, false, 0)};
    p.ins = {I(VNM_EX_LOOKUP_U8, 0, 0.0, 1)};
    emit("lookup/alone_u8", p);
    p.cols = {column(VNM_I32, true), column(VNM_I32, false, 3)};
    p.ins = {I(VNM_EX_LOOKUP_I32, 0, 0.0, 1)};
    emit("lookup/alone_i32", p);
    p.cols = {column(VNM_I32, true), column(VNM_U8, false, 0), column(VNM_I32, false, 3)};
    p.ins = {I(VNM_EX_LOOKUP_I32, 0, 0.0, 2), I(VNM_EX_SQRT), I(VNM_EX_LOOKUP_U8, 0, 0.0, 1), I(VNM_EX_TO_I64), I(VNM_EX_ADD)};
    emit("lookup/as_values", p);
}
static void many_outputs() {
    const int orders[][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
    for (int o = 0; o < 3; o++) for (int t = 0; t < 10; t++) {
        Prog p;
        p.single = false;
        p.n_out = 4;
        p.cols = {column(t, false), column(VNM_U8, false), column(VNM_I16, true)};
        p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_COL, 1), I(VNM_EX_MUL), I(VNM_EX_STORE, orders[o][0]),
                 I(VNM_EX_COL, 0), I(VNM_EX_CONST_I, 0, 0.0, 7), I(VNM_EX_LE), I(VNM_EX_IS_NULL, 2), I(VNM_EX_OR), I(VNM_EX_STORE, orders[o][1]),
                 I(VNM_EX_COL, 1), I(VNM_EX_SQRT), I(VNM_EX_STORE, orders[o][2]),
                 I(VNM_EX_CONST_F, 0, 1.5, 0), I(VNM_EX_STORE, orders[o][3])};
        emit(name("multi", {o, t}), p);
    }
    // two values on the stack when the first STORE comes: the second pops what is below
    Prog p;
    p.single = false;
    p.n_out = 2;
    p.cols = {column(VNM_I8, false), column(VNM_F32, false)};
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_COL, 1), I(VNM_EX_STORE, 1), I(VNM_EX_STORE, 0)};
    emit("multi/nested", p);
}
// the limits: depth 12 and 13 (with and without a built-in), 63 / 64 / 65 instructions with and without the implied STORE
static void limits() {
    for (int depth : {9, 10, 12, 13}) for (int fn : {0, (int)VNM_EX_ABS, (int)VNM_EX_SIN}) for (int single = 0; single < 2; single++) {
        Prog p;
        p.single = single;
        p.cols = {column(VNM_F64, false), column(VNM_I32, false)};
        for (int k = 0; k < depth; k++) p.ins.push_back(I(VNM_EX_COL, k & 1));
        if (fn) p.ins.push_back(I(fn));
        for (int k = 1; k < depth; k++) p.ins.push_back(I(VNM_EX_ADD));
        if (!single) p.ins.push_back(I(VNM_EX_STORE, 0));
        emit(name("depth", {depth, fn, single}), p);
    }
    for (int n_ins : {63, 64, 65}) for (int single = 0; single < 2; single++) {
        Prog p;
        p.single = single;
        p.cols = {column(VNM_I64, false)};
        p.ins = {I(VNM_EX_COL, 0)};
        while ((int)p.ins.size() + 2 < n_ins) p.ins.insert(p.ins.end(), {I(VNM_EX_CONST_I, 0, 0.0, (int64_t)p.ins.size()), I(VNM_EX_ADD)});
        while ((int)p.ins.size() + (single ? 0 : 1) < n_ins) p.ins.push_back(I(VNM_EX_NEG));
        if (!single) p.ins.push_back(I(VNM_EX_STORE, 0));
        emit(name("length", {n_ins, single}), p);
    }
}
static void malformed() {
    const int classes[] = {VNM_EX_NEG, VNM_EX_BNOT, VNM_EX_ABS, VNM_EX_TO_BOOL, VNM_EX_NOT, VNM_EX_AND, VNM_EX_EQ, VNM_EX_ADD, VNM_EX_POW};
    for (int op : classes) for (int have = 0; have < 2; have++) {   // nothing on the stack; one value where two are needed
        Prog p;
        p.cols = {column(VNM_I32, false)};
        if (have) p.ins.push_back(I(VNM_EX_COL, 0));
        p.ins.push_back(I(op));
        emit(name("underflow", {op, have}), p);
    }
    Prog p;
    p.cols = {column(VNM_I32, false), column(VNM_F64, true)};
    p.single = false;
    p.ins = {I(VNM_EX_STORE, 0)};
    emit("bad/store_underflow", p);
    // (tables as long as the batch, so that one no lookup names passes for a row column)
    p.cols = {column(VNM_I32, false), column(VNM_U8, false), column(VNM_I32, false), column(VNM_I64, false), column(VNM_U8, false)};
    for (int op : {VNM_EX_COL, VNM_EX_IS_NULL, VNM_EX_IS_NOT_NULL, VNM_EX_LOOKUP_U8, VNM_EX_LOOKUP_I32}) for (int idx : {-1, 5}) {
        p.ins = {I(op, idx, 0.0, op == VNM_EX_LOOKUP_I32 ? 2 : 1), I(VNM_EX_STORE, 0)};
        emit(name("bad/column_index", {op, idx}), p);
    }
    for (int op : {VNM_EX_LOOKUP_U8, VNM_EX_LOOKUP_I32}) for (int64_t table : {(int64_t)-1, (int64_t)5, (int64_t)1 << 32}) {
        p.ins = {I(op, 0, 0.0, table), I(VNM_EX_STORE, 0)};
        emit(name("bad/table_index", {op, (long long)table}), p);
    }
    p.ins = {I(VNM_EX_LOOKUP_U8, 0, 0.0, 1), I(VNM_EX_LOOKUP_I32, 0, 0.0, 1), I(VNM_EX_STORE, 0)};
    emit("bad/table_both_kinds", p);
    p.ins = {I(VNM_EX_LOOKUP_U8, 1, 0.0, 1), I(VNM_EX_STORE, 0)};
    emit("bad/own_table", p);
    for (int op : {VNM_EX_COL, VNM_EX_IS_NULL, VNM_EX_LOOKUP_U8}) {
        p.ins = {I(VNM_EX_LOOKUP_U8, 0, 0.0, 1), I(op, 1, 0.0, 4), I(VNM_EX_AND), I(VNM_EX_STORE, 0)};
        emit(name("bad/table_as_row_column", {op}), p);
    }
    for (int op : {VNM_EX_LOOKUP_U8, VNM_EX_LOOKUP_I32}) {
        p.ins = {I(op, 3, 0.0, op == VNM_EX_LOOKUP_U8 ? 1 : 2), I(VNM_EX_STORE, 0)};
        emit(name("bad/codes_not_int32", {op}), p);
        p.ins = {I(op, 0, 0.0, op == VNM_EX_LOOKUP_U8 ? 2 : 1), I(VNM_EX_STORE, 0)};
        emit(name("bad/table_type", {op}), p);
    }
    p.ins = {I(VNM_EX_LOOKUP_U8, 0, 0.0, 1), I(VNM_EX_STORE, 0)};
    p.cols[1].validity = VALIDITY;
    emit("bad/table_with_validity", p);
    p.cols[1] = column(VNM_U8, false, -1);
    emit("bad/table_negative_length", p);
    p.cols[1] = column(VNM_U8, false);
    p.cols[1].offset = -1;
    emit("bad/table_negative_offset", p);
    p.cols = {column(VNM_I32, false), column(VNM_F64, false, ROWS + 1)};
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, 0)};
    emit("bad/unequal_lengths", p);
    p.cols = {column(VNM_I32, false), column(10, false)};
    emit("bad/column_type_10", p);
    p.cols[1].type = -1;
    emit("bad/column_type_minus_1", p);
    p.cols = {column(VNM_I32, false), column(VNM_F64, true)};
    p.n_out = 2;
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, 0), I(VNM_EX_COL, 1), I(VNM_EX_STORE, 0)};
    emit("bad/store_twice", p);
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, 1)};
    emit("bad/store_never", p);
    for (int idx : {-1, 2}) {
        p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, idx)};
        emit(name("bad/store_index", {idx}), p);
    }
    p.n_out = 1;
    p.single = true;
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, 0)};
    emit("bad/store_in_single", p);
    for (int op : {-1, -2, 39, 1000}) {
        p.ins = {I(VNM_EX_COL, 0), I(op)};
        emit(name("bad/opcode", {op}), p);
    }
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_COL, 1)};
    emit("bad/two_left_single", p);
    p.single = false;
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_COL, 1), I(VNM_EX_STORE, 0)};
    emit("bad/one_left_multi", p);
    p.ins = {I(VNM_EX_IS_NULL, 1), I(VNM_EX_COL, 0), I(VNM_EX_GT), I(VNM_EX_STORE, 0)};
    emit("bad/compare_mask", p);
    p.ins = {I(VNM_EX_IS_NULL, 1), I(VNM_EX_NEG), I(VNM_EX_STORE, 0)};
    emit("bad/negate_mask", p);
    p.ins.clear();
    emit("bad/no_instructions", p);
    p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_STORE, 0)};
    for (int n_out : {0, 17, -1}) {
        p.n_out = n_out;
        emit(name("bad/n_out", {n_out}), p);
    }
    p.n_out = 1;
    p.cols.assign(17, column(VNM_I32, false));
    emit("bad/n_cols_17", p);
    emit("bad/n_cols_minus_1", p, -1);
    p.cols.resize(16);
    emit("ok/n_cols_16", p);
    p.n_out = 16;
    p.ins.clear();
    for (int k = 0; k < 16; k++) p.ins.insert(p.ins.end(), {I(VNM_EX_COL, k), I(VNM_EX_STORE, 15 - k)});
    emit("ok/n_out_16", p);
}
// the literal's rounding to float16, on its own: ties, the subnormal range, the overflow threshold, both signs
static void half_rounding() {
    uint32_t seed = 2024;
    std::vector<double> v = {0.0, -0.0, 65504.0, 65519.999, 65520.0, 65536.0, 1e300, -1e300, 1e-300, 5.9604644775390625e-8, 2.98023223876953125e-8,
                             2.9802322387695316e-8, 6.103515625e-5, 6.0975551605224609375e-5, 2049.0, 2051.0, 1.0009765625, 1.00048828125, 1.000488281250001,
                             INFINITY, -INFINITY, 1.0 / 3.0, (double)NAN, -(double)NAN};
    const uint64_t low_payload = 0x7FF0000000000123ULL;   // a NaN whose payload a half cannot hold (and whose quiet bit is clear)
    double nan_low;
    memcpy(&nan_low, &low_payload, 8);
    v.push_back(nan_low);
    for (int k = 0; k < 2000; k++) {
        seed = seed * 1664525u + 1013904223u;
        const int e = (int)((seed >> 8) % 48) - 30;
        seed = seed * 1664525u + 1013904223u;
        const double m = 1.0 + (double)(seed >> 8) / 16777216.0;       // 24 mantissa bits: ties among them
        seed = seed * 1664525u + 1013904223u;
        const double fine = (seed >> 31) ? 0.0 : (double)((seed >> 8) & 0xFF) / 1099511627776.0;   // and values just beside a tie
        v.push_back(((seed >> 30) & 1 ? -1.0 : 1.0) * std::ldexp(m + fine, e));
    }
    for (int k = 7; k < 2048; k += 7) v.push_back((k + 0.5) * 5.9604644775390625e-8);   // halfway between subnormal halves
    for (double d : v) {
        Prog p;
        p.cols = {column(VNM_U8, false)};
        p.ins = {I(VNM_EX_COL, 0), I(VNM_EX_SQRT), I(VNM_EX_CONST_F, 0, d, 0), I(VNM_EX_ADD)};
        uint64_t bits;
        memcpy(&bits, &d, 8);
        char label[64];
        snprintf(label, sizeof label, "half/%016llx", (unsigned long long)bits);
        emit(label, p);
    }
}

int main() {
    two_columns();
    one_column();
    column_and_literal();
    float16_values();
    lookups();
    many_outputs();
    limits();
    malformed();
    half_rounding();
    return 0;
}
