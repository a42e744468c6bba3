// The host half of the Arrow-level operators (vnm_arrow.cpp, vnm_agg_op.cpp, vnm_sort_op.cpp): what an Arrow C Data schema child
// is, validity bits, freshly allocated Arrow arrays and schemas, and the host copy of a device dictionary's values.  Nothing here
// touches the device or the library's error state: a helper that can fail returns its message (empty: fine) and the caller
// reports it.  tests/arrow_host_main.cpp runs all of it under AddressSanitizer without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vinum_hip.h"

namespace vnm {

// ---- what a schema child is ---------------------------------------------------------------------------------------------------------
struct ColType {
    int type = -1;   // vnm_type or -1 (unsupported)
    int flags = 0;
    std::string format;
};

inline ColType parse_format(const char* f) {
    ColType c;
    c.format = f ? f : "";
    const std::string& s = c.format;
    if (s == "c") c.type = VNM_I8;
    else if (s == "C") c.type = VNM_U8;
    else if (s == "s") c.type = VNM_I16;
    else if (s == "S") c.type = VNM_U16;
    else if (s == "i") c.type = VNM_I32;
    else if (s == "I") c.type = VNM_U32;
    else if (s == "l") c.type = VNM_I64;
    else if (s == "L") c.type = VNM_U64;
    else if (s == "f") c.type = VNM_F32;
    else if (s == "g") c.type = VNM_F64;
    else if (s == "tdD") c.type = VNM_I32;                              // date32
    else if (s == "tdm") c.type = VNM_I64;                              // date64
    else if (s == "tts" || s == "ttm") { c.type = VNM_I32; c.flags = VNM_FLAG_SUM32; }  // time32
    else if (s == "ttu" || s == "ttn") c.type = VNM_I64;                // time64
    else if (s.rfind("ts", 0) == 0 && s.size() >= 4 && s[3] == ':') c.type = VNM_I64;  // timestamp
    else if (s == "tDs" || s == "tDm" || s == "tDu" || s == "tDn") c.type = VNM_I64;   // duration
    return c;
}

// How a column travels.  COL_NONE: not taken (a dictionary over anything but strings / binaries among them: a child with a dictionary
// is judged by its SCHEMA and never read as its indices).  Each operator keeps its own policy on top (Sort refuses a boolean key, the
// aggregates SUM / AVG over anything but COL_NUM).
enum ColKind { COL_NONE = -1, COL_NUM = 0, COL_STR, COL_BOOL, COL_DEC, COL_DICT };
// The two operators have never agreed on decimals, and Arrow can emit a format that shows it: scale is any int32, so decimal256(76,
// 128) is "d:76,128,256", which the aggregates' rule takes for 16-byte values.  Each keeps its rule until that is decided.
enum DecimalRule {
    DECIMAL_128_ONLY,        // Sort: d:p,s and d:p,s,128
    DECIMAL_ANY_COMMA_128    // aggregates: d:p,s and any format that contains ",128"
};
struct ColDesc {
    ColKind kind = COL_NONE;
    ColType t;                  // the child's own format; its numeric type (COL_NUM) or index type (COL_DICT), else -1
    bool wide = false;          // 64-bit offsets: large_utf8 / large_binary (COL_DICT: of the values)
    bool has_dictionary = false;
    std::string value_format;   // of the dictionary (COL_DICT: u / U / z / Z)
    bool ordered = false;       // ARROW_FLAG_DICTIONARY_ORDERED
    // what a later batch's child must repeat: the format, and under a dictionary its value format and the ordered flag.  ('|' is in no
    // integer format, the only ones a dictionary's indices can have.)
    std::string signature() const {
        return has_dictionary ? t.format + "|" + value_format + (ordered ? "|ordered" : "") : t.format;
    }
};

inline ColDesc describe_column(const struct ArrowSchema* s, DecimalRule rule) {
    ColDesc c;
    c.t = parse_format(s->format);
    const std::string& f = c.t.format;
    auto string_like = [](const std::string& x) { return x == "u" || x == "U" || x == "z" || x == "Z"; };
    if (s->dictionary) {
        c.has_dictionary = true;
        c.value_format = s->dictionary->format ? s->dictionary->format : "";
        c.ordered = (s->flags & 1) != 0;
        if (f.size() == 1 && strchr("cCsSiIlL", f[0]) && string_like(c.value_format)) {
            c.kind = COL_DICT;
            c.wide = c.value_format == "U" || c.value_format == "Z";
        } else c.t.type = -1;
        return c;
    }
    if (c.t.type >= 0) c.kind = COL_NUM;
    else if (string_like(f)) { c.kind = COL_STR; c.wide = f == "U" || f == "Z"; }
    else if (f == "b") c.kind = COL_BOOL;
    else if (f.rfind("d:", 0) == 0) {   // d:precision,scale[,bit width]: 128 bits unless said otherwise
        const size_t c1 = f.find(','), c2 = c1 == std::string::npos ? std::string::npos : f.find(',', c1 + 1);
        const bool only128 = c1 != std::string::npos && (c2 == std::string::npos || f.substr(c2 + 1) == "128");
        const bool any128 = f.find(",128") != std::string::npos || std::count(f.begin(), f.end(), ',') == 1;
        if (rule == DECIMAL_128_ONLY ? only128 : any128) c.kind = COL_DEC;
    }
    return c;
}

// ---- validity bits ------------------------------------------------------------------------------------------------------------------
// n bits of src (from bit src_off) to dst (from bit dst_off); dst's bits in that range are zero on entry.  Byte-wise with a shift:
// ~1 ns per byte instead of a branch per bit (5e7 nullable rows per column: 100+ ms of the small-batch route).
inline void copy_bits(uint8_t* dst, int64_t dst_off, const uint8_t* src, int64_t src_off, int64_t n) {
    auto bit = [&](int64_t i) { if ((src[(src_off + i) >> 3] >> ((src_off + i) & 7)) & 1) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7)); };
    int64_t i = 0;
    for (; i < n && ((dst_off + i) & 7); i++) bit(i);   // head: up to the next byte boundary of dst
    const int64_t body = (n - i) / 8;
    if (body > 0) {
        uint8_t* d = dst + ((dst_off + i) >> 3);
        const int64_t so = src_off + i;
        const uint8_t* sp = src + (so >> 3);
        const int sh = (int)(so & 7);
        if (sh == 0) memcpy(d, sp, (size_t)body);
        else for (int64_t k = 0; k < body; k++) d[k] = (uint8_t)((sp[k] >> sh) | (sp[k + 1] << (8 - sh)));
        i += body * 8;
    }
    for (; i < n; i++) bit(i);
}
inline void set_bits(uint8_t* dst, int64_t dst_off, int64_t n) {
    int64_t i = 0;
    for (; i < n && ((dst_off + i) & 7); i++) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
    const int64_t body = (n - i) / 8;
    if (body > 0) { memset(dst + ((dst_off + i) >> 3), 0xFF, (size_t)body); i += body * 8; }
    for (; i < n; i++) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
}
// The validity of several runs of rows laid end to end: (total + 7) / 8 bytes and 8 of padding, or EMPTY when no run has a bitmap
// (no NULL anywhere) or there are no rows.
struct BitRun { const uint8_t* bits; int64_t off, len; };   // rows [off, off + len) of a bitmap; bits null: all valid
inline std::vector<uint8_t> join_validity(const std::vector<BitRun>& runs, int64_t total) {
    std::vector<uint8_t> bits;
    bool any = false;
    for (auto& r : runs) any = any || r.bits != nullptr;
    if (!any || total == 0) return bits;
    bits.assign((size_t)(total + 7) / 8 + 8, 0);
    int64_t pos = 0;
    for (auto& r : runs) {
        if (r.bits) copy_bits(bits.data(), pos, r.bits, r.off, r.len); else set_bits(bits.data(), pos, r.len);
        pos += r.len;
    }
    return bits;
}
// one byte per row -> a calloc'ed bitmap; *zeros: the rows whose byte is 0
inline uint8_t* pack_bits(const uint8_t* bytes, int64_t n, int64_t* zeros) {
    uint8_t* bm = (uint8_t*)calloc((size_t)((n + 7) / 8 + 1), 1);
    int64_t z = 0;
    for (int64_t i = 0; i < n; i++) { if (bytes[i]) bm[i >> 3] |= (uint8_t)(1u << (i & 7)); else z++; }
    if (zeros) *zeros = z;
    return bm;
}

// ---- freshly allocated Arrow schemas and arrays (malloc'ed, released by their own release) -------------------------------------------
inline void release_schema(struct ArrowSchema* s) {
    if (!s || !s->release) return;
    for (int64_t i = 0; i < s->n_children; i++) {
        if (s->children[i]) {
            if (s->children[i]->release) s->children[i]->release(s->children[i]);
            free(s->children[i]);
        }
    }
    free(s->children);
    if (s->dictionary) {
        if (s->dictionary->release) s->dictionary->release(s->dictionary);
        free(s->dictionary);
    }
    free((void*)s->format);
    free((void*)s->name);
    s->release = nullptr;
}

inline void release_array(struct ArrowArray* a) {
    if (!a || !a->release) return;
    for (int64_t i = 0; i < a->n_children; i++) {
        if (a->children[i]) {
            if (a->children[i]->release) a->children[i]->release(a->children[i]);
            free(a->children[i]);
        }
    }
    free(a->children);
    if (a->dictionary) {
        if (a->dictionary->release) a->dictionary->release(a->dictionary);
        free(a->dictionary);
    }
    for (int64_t i = 0; i < a->n_buffers; i++) free((void*)a->buffers[i]);
    free(a->buffers);
    a->release = nullptr;
}

inline void make_schema(struct ArrowSchema* s, const std::string& format, const std::string& name, int64_t n_children) {
    memset(s, 0, sizeof(*s));
    s->format = strdup(format.c_str());
    s->name = strdup(name.c_str());
    s->flags = 2;  // ARROW_FLAG_NULLABLE
    s->n_children = n_children;
    s->children = n_children ? (struct ArrowSchema**)calloc((size_t)n_children, sizeof(void*)) : nullptr;
    for (int64_t i = 0; i < n_children; i++) s->children[i] = (struct ArrowSchema*)calloc(1, sizeof(struct ArrowSchema));
    s->release = release_schema;
}
// the schema a column leaves with: its own format, and under COL_DICT the dictionary child and the ordered flag it came in with
inline void make_dict_schema(struct ArrowSchema* s, const ColDesc& d, const std::string& name) {
    make_schema(s, d.t.format, name, 0);
    if (d.kind != COL_DICT) return;
    s->dictionary = (struct ArrowSchema*)calloc(1, sizeof(struct ArrowSchema));
    make_schema(s->dictionary, d.value_format, "", 0);
    if (d.ordered) s->flags |= 1;   // ARROW_FLAG_DICTIONARY_ORDERED
}

// an array of n rows and n_buffers null buffers
inline void make_array(struct ArrowArray* a, int64_t n, int n_buffers) {
    memset(a, 0, sizeof(*a));
    a->length = n;
    a->n_buffers = n_buffers;
    a->buffers = (const void**)calloc((size_t)n_buffers, sizeof(void*));
    a->release = release_array;
}
// primitive array with malloc'ed buffers; valid_bytes (one byte per row) may be NULL (no nulls)
inline void make_primitive(struct ArrowArray* a, int64_t n, int width, const void* values, const uint8_t* valid_bytes) {
    make_array(a, n, 2);
    if (valid_bytes) {
        uint8_t* bm = pack_bits(valid_bytes, n, &a->null_count);
        if (a->null_count) a->buffers[0] = bm; else free(bm);
    }
    void* data = malloc((size_t)(n ? n : 1) * width);
    if (n) memcpy(data, values, (size_t)n * width);
    a->buffers[1] = data;
}

inline void make_struct(struct ArrowArray* a, int64_t n, int64_t n_children) {
    make_array(a, n, 1);
    a->n_children = n_children;
    a->children = n_children ? (struct ArrowArray**)calloc((size_t)n_children, sizeof(void*)) : nullptr;
    for (int64_t i = 0; i < n_children; i++) a->children[i] = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
}

// ---- the host copy of a device dictionary's values -----------------------------------------------------------------------------------
// The values the encodes of one vnm_strdict added, laid end to end in the order they came back (value k: ids[k], bytes [off[k],
// off[k + 1])).  Nothing is indexed by id until a result asks for the ids it uses: an id-indexed table of strings is one cache miss
// per value.  Ids are handed out in chunks (not dense, not in order).
struct DictValues {
    std::vector<int32_t> ids;
    std::vector<int64_t> off{0};
    std::vector<uint8_t> bytes;
    int32_t top = 0;   // every id < top

    // n_new more values of new_bytes bytes together; fetch(ids, lens, bytes) writes them in place (vnm_strdict_fetch_new's
    // signature: the caller binds the dictionary) and returns 0, or a status that is handed on with nothing appended
    template <class Fetch>
    int append_new(int64_t n_new, int64_t new_bytes, Fetch fetch) {
        if (n_new <= 0) return 0;
        const size_t k0 = ids.size(), b0 = bytes.size();
        std::vector<int32_t> lens((size_t)n_new);
        ids.resize(k0 + (size_t)n_new);
        bytes.resize(b0 + (size_t)new_bytes + 1);     // (+ 1: never a null pointer for the fetch; cut below)
        const int rc = fetch(ids.data() + k0, lens.data(), bytes.data() + b0);
        ids.resize(rc ? k0 : k0 + (size_t)n_new);
        bytes.resize(rc ? b0 : b0 + (size_t)new_bytes);
        if (rc) return rc;
        for (int64_t i = 0; i < n_new; i++) {
            off.push_back(off.back() + lens[(size_t)i]);
            top = std::max(top, ids[k0 + (size_t)i] + 1);
        }
        return 0;
    }

    // The values of want[0 .. n) -> a utf8 / binary (wide: large_) array.  Row i is NULL where want[i] < 0 or valid_bytes (one byte
    // per row, may be null) says so: a result dictionary passes ascending ids and no NULLs, a plain key column or a string MIN / MAX
    // passes whatever its groups hold.  One pass over the list fills a position-by-id table (4 bytes per id), then one gather.
    // `what` names the array in the messages ("a result dictionary").
    std::string make_string_array(struct ArrowArray* a, bool wide, const int32_t* want, const uint8_t* valid_bytes, int64_t n, const char* what) const {
        char msg[200];
        std::vector<int32_t> at_of_id((size_t)(top > 0 ? top : 1), -1);
        for (size_t k = 0; k < ids.size(); k++) if (ids[k] >= 0) at_of_id[(size_t)ids[k]] = (int32_t)k;
        std::vector<uint8_t> valid((size_t)(n ? n : 1), 1);
        size_t total = 0;
        for (int64_t i = 0; i < n; i++) {
            if (want[i] < 0 || (valid_bytes && !valid_bytes[i])) { valid[(size_t)i] = 0; continue; }
            if (want[i] >= top || at_of_id[(size_t)want[i]] < 0) {
                snprintf(msg, sizeof(msg), "%s names id %d, which no encode handed over (internal error)", what, want[i]);
                return msg;
            }
            const size_t k = (size_t)at_of_id[(size_t)want[i]];
            total += (size_t)(off[k + 1] - off[k]);
        }
        if (!wide && total > 0x7FFFFFFFULL) {
            snprintf(msg, sizeof(msg), "%s holds more than 2 GiB of bytes (use the large type)", what);
            return msg;
        }
        make_array(a, n, 3);
        uint8_t* bm = pack_bits(valid.data(), n, &a->null_count);
        if (a->null_count) a->buffers[0] = bm; else free(bm);
        uint8_t* data = (uint8_t*)malloc(total ? total : 1);
        int32_t* o32 = wide ? nullptr : (int32_t*)malloc((size_t)(n + 1) * 4);
        int64_t* o64 = wide ? (int64_t*)malloc((size_t)(n + 1) * 8) : nullptr;
        size_t at = 0;
        for (int64_t i = 0; i <= n; i++) {
            if (wide) o64[i] = (int64_t)at; else o32[i] = (int32_t)at;
            if (i == n || !valid[(size_t)i]) continue;
            const size_t k = (size_t)at_of_id[(size_t)want[i]];
            const size_t len = (size_t)(off[k + 1] - off[k]);
            if (len) memcpy(data + at, bytes.data() + off[k], len);
            at += len;
        }
        a->buffers[1] = wide ? (void*)o64 : (void*)o32;
        a->buffers[2] = data;
        return std::string();
    }
};

}  // namespace vnm
