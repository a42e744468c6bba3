// One value through a code point map: the per-lane body of sd_map_kernel (vnm_strdict.hip), kept free of anything a host compiler
// does not know so that the same code runs under a host sanitizer against exactly-sized buffers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VNM_HD __host__ __device__ __forceinline__
#else
#define VNM_HD inline
#endif

namespace vnm {

// The `len` bytes at `p` decoded as UTF-8, every code point found in from[0 .. n_map) (ascending) replaced by its `to` entry, encoded
// into q[0 .. room).  Returns the bytes written, -1 for a malformed value: a continuation byte or 0xF8..0xFF where a lead byte is
// due, a lead byte whose sequence does not end inside the value (the length is checked BEFORE a continuation byte is read: nothing
// at or past p + len is touched), a continuation position holding another kind of byte.  Also -1 where an image would not fit the
// room -- every store is checked, whatever the map says; the entry point refuses maps under which that can happen.
//   * ascii_closed (the map keeps ASCII inside ASCII): 8 source bytes per step while none has its top bit set, eight lookups in the
//     128-byte table `ascii`, one 8-byte store; a single ASCII byte takes the same table.
//   * any other code point: a branch-free lower bound over `from` (top_step = the largest power of two <= n_map; one compare and
//     one select per halving).  A code point outside the map is copied as it stands.
VNM_HD int64_t mc_map_value(const uint8_t* p, int64_t len, uint8_t* q, int64_t room, const int32_t* from, const int32_t* to, int n_map,
                            int top_step, const uint8_t* ascii, bool ascii_closed) {
    int64_t i = 0, o = 0;
    while (i < len) {
        if (ascii_closed && i + 8 <= len) {
            uint64_t x;
            __builtin_memcpy(&x, p + i, 8);
            if (!(x & 0x8080808080808080ULL)) {
                uint64_t y = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) y |= (uint64_t)ascii[(x >> (8 * k)) & 0x7F] << (8 * k);
                if (o + 8 > room) return -1;
                __builtin_memcpy(q + o, &y, 8);
                i += 8; o += 8;
                continue;
            }
        }
        const uint32_t b = p[i];
        const int n = b < 0x80 ? 1 : b < 0xC0 ? 0 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : b < 0xF8 ? 4 : 0;
        if (n == 0 || i + n > len) return -1;                      // no lead byte, or the value ends inside the sequence
        uint32_t cp = n == 1 ? b : (b & (0xFFu >> (n + 1)));
        bool cont = true;
        for (int k = 1; k < n; k++) {
            const uint32_t c = p[i + k];
            cont = cont && (c & 0xC0) == 0x80;
            cp = (cp << 6) | (c & 0x3F);
        }
        if (!cont) return -1;
        uint32_t m = cp;
        bool hit = false;
        if (n == 1 && ascii_closed) {
            m = ascii[b]; hit = true;
        } else if (n_map > 0) {
            int lo = 0;                                             // entries <= cp
            for (int step = top_step; step; step >>= 1) {
                const int j = lo + step, at = (j <= n_map ? j : n_map) - 1;
                lo = (j <= n_map && from[at] <= (int32_t)cp) ? j : lo;
            }
            const int at = lo > 0 ? lo - 1 : 0;
            hit = lo > 0 && from[at] == (int32_t)cp;
            if (hit) m = (uint32_t)to[at];
        }
        if (!hit) {                                                 // not in the map: the sequence as it stands
            if (o + n > room) return -1;
            for (int k = 0; k < n; k++) q[o + k] = p[i + k];
            o += n;
        } else {
            const int e = m < 0x80 ? 1 : m < 0x800 ? 2 : m < 0x10000 ? 3 : 4;
            if (o + e > room) return -1;
            if (e == 1) q[o] = (uint8_t)m;
            else if (e == 2) { q[o] = (uint8_t)(0xC0 | (m >> 6)); q[o + 1] = (uint8_t)(0x80 | (m & 0x3F)); }
            else if (e == 3) { q[o] = (uint8_t)(0xE0 | (m >> 12)); q[o + 1] = (uint8_t)(0x80 | ((m >> 6) & 0x3F)); q[o + 2] = (uint8_t)(0x80 | (m & 0x3F)); }
            else { q[o] = (uint8_t)(0xF0 | ((m >> 18) & 0x07)); q[o + 1] = (uint8_t)(0x80 | ((m >> 12) & 0x3F)); q[o + 2] = (uint8_t)(0x80 | ((m >> 6) & 0x3F)); q[o + 3] = (uint8_t)(0x80 | (m & 0x3F)); }
            o += e;
        }
        i += n;
    }
    return o;
}

}  // namespace vnm
