// One concat() image: the per-lane byte writer of sc_image_kernel (vnm_strconcat.inc), kept free of anything a host compiler does
// not know so that the same code runs under a host sanitizer against exactly-sized buffers (as vnm_strcase.hpp).
//
// ConcatFunction (vinum/core/functions.py:250-276) turns every operand into a NumPy 'U' array and folds them with np.char.add.  A 'U'
// array drops TRAILING NUL code points of an element (leading and embedded ones stay) and holds str(None) = "None" for a NULL row.
// On UTF-8 bytes a NUL code point is the byte 0x00 and no other code point contains that byte, so the rule is one on bytes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VNM_HD __host__ __device__ __forceinline__
#else
#define VNM_HD inline
#endif

namespace vnm {

// the length of p[0 .. len) without its trailing 0x00 bytes
VNM_HD int64_t sc_rstrip_nul(const uint8_t* p, int64_t len) {
    while (len > 0 && p[len - 1] == 0) len--;
    return len;
}

// what an operand contributes: len < 0 is NULL, the four bytes "None"
VNM_HD int64_t sc_value_room(const uint8_t* p, int64_t len) { return len < 0 ? 4 : sc_rstrip_nul(p, len); }

// n bytes of p to q + o, held against the room first: the new write position, -1 once anything did not fit (and from then on)
VNM_HD int64_t sc_put(uint8_t* q, int64_t o, int64_t room, const uint8_t* p, int64_t n) {
    if (o < 0 || n < 0 || o + n > room) return -1;
    for (int64_t i = 0; i < n; i++) q[o + i] = p[i];
    return o + n;
}

VNM_HD int64_t sc_put_value(uint8_t* q, int64_t o, int64_t room, const uint8_t* p, int64_t len) {
    const uint8_t none[4] = {'N', 'o', 'n', 'e'};
    return len < 0 ? sc_put(q, o, room, none, 4) : sc_put(q, o, room, p, sc_rstrip_nul(p, len));
}

// prefix + value(a) [+ sep + value(b)] + suffix.  lits = prefix | sep | suffix back to back (already without trailing NULs where the
// host merged them).  sc_concat_room is the exact length of the image; sc_concat_write returns the bytes written (== the room it
// was given when that came from sc_concat_room) or -1 when a store would have left q[0 .. room).
VNM_HD int64_t sc_concat_room(int64_t pre_len, const uint8_t* a, int64_t a_len, int64_t sep_len, bool has_b, const uint8_t* b, int64_t b_len,
                              int64_t suf_len) {
    return pre_len + sc_value_room(a, a_len) + (has_b ? sep_len + sc_value_room(b, b_len) : 0) + suf_len;
}

VNM_HD int64_t sc_concat_write(uint8_t* q, int64_t room, const uint8_t* lits, int64_t pre_len, const uint8_t* a, int64_t a_len, int64_t sep_len,
                               bool has_b, const uint8_t* b, int64_t b_len, int64_t suf_len) {
    int64_t o = sc_put(q, 0, room, lits, pre_len);
    o = sc_put_value(q, o, room, a, a_len);
    if (has_b) {
        o = sc_put(q, o, room, lits + pre_len, sep_len);
        o = sc_put_value(q, o, room, b, b_len);
    }
    return sc_put(q, o, room, lits + pre_len + sep_len, suf_len);
}

}  // namespace vnm
