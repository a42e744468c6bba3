// One to_str() image: the per-lane formatter of the value form of sc_image_kernel (vnm_strconcat.inc), kept free of anything a host
// compiler does not know so that the same code runs under a host sanitizer against exactly-sized buffers (as vnm_strconcat.hpp).
//
// StringCastFunction (vinum/core/functions.py:189-193, AbstractCastFunction :148-162) computes np.array(column, dtype='str'): NumPy's
// text of the value.
//   integers      decimal digits, '-' in front of a negative one
//   date32        datetime64[D]: YYYY-MM-DD.  The year is C's %04d with the sign INSIDE the width: 0000, -001, 10000, -5877641
//   timestamp     datetime64[s | ms | us | ns]: YYYY-MM-DDTHH:MM:SS and .fff / .ffffff / .fffffffff, always at full width.  Division
//                 floors (-1 ns is 1969-12-31T23:59:59.999999999); the year of unit s reaches 12 digits, so the calendar is int64;
//                 the stored value INT64_MIN is NaT and prints "NaT"
//   NULL          the four bytes "None" (TS_NONE) -- one rule for every type, the rule concat() has for its operands.  The reference
//                 prints a NULL integer column through float64 ("1.0" / "nan", batch by batch) and a NULL date as "NaT": not restated.
// The caller widens the value to 64 bits, by sign (signed integers, date32, timestamps) or by zero extension (TS_UINT).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VNM_HD __host__ __device__ __forceinline__
#else
#define VNM_HD inline
#endif

namespace vnm {

// (the first seven are enum vnm_tostr_kind of include/vinum_hip.h, in its order)
enum { TS_INT = 0, TS_UINT, TS_DATE32, TS_TIMESTAMP_S, TS_TIMESTAMP_MS, TS_TIMESTAMP_US, TS_TIMESTAMP_NS, TS_NONE };

constexpr int TS_MAX_BYTES = 29;   // the longest image: 2262-04-11T23:47:16.854775807 (ns), -290308-12-21T19:59:05.224192 (us),
                                   // -292275055-05-16T16:47:04.192 (ms); -292277022657-01-27T08:29:53 (s) is 28, an integer at most 20

// floor division and modulus by a positive divisor (C's truncate towards zero)
VNM_HD int64_t ts_floor_div(int64_t a, int64_t b) { return a / b - ((a % b) < 0 ? 1 : 0); }
VNM_HD int64_t ts_floor_mod(int64_t a, int64_t b) { const int64_t r = a % b; return r < 0 ? r + b : r; }

// one byte to q + o, held against the room first; q == nullptr only counts.  The new write position, -1 once anything did not fit
VNM_HD int64_t ts_put(uint8_t* q, int64_t o, int64_t room, uint8_t c) {
    if (o < 0) return -1;
    if (!q) return o + 1;
    if (o + 1 > room) return -1;
    q[o] = c;
    return o + 1;
}

// the decimal digits of v, at least `width` of them (zero padded)
VNM_HD int64_t ts_put_digits(uint8_t* q, int64_t o, int64_t room, uint64_t v, int width) {
    uint8_t d[20];
    int n = 0;
    do { d[n++] = (uint8_t)('0' + v % 10); v /= 10; } while (v);
    for (int k = width; k > n; k--) o = ts_put(q, o, room, '0');
    while (n > 0) o = ts_put(q, o, room, d[--n]);
    return o;
}

// a signed number as %0<width>d: the sign counts towards the width.  The magnitude comes from unsigned arithmetic (INT64_MIN)
VNM_HD int64_t ts_put_signed(uint8_t* q, int64_t o, int64_t room, int64_t v, int width) {
    if (v >= 0) return ts_put_digits(q, o, room, (uint64_t)v, width);
    o = ts_put(q, o, room, '-');
    return ts_put_digits(q, o, room, 0ULL - (uint64_t)v, width - 1);
}

// days since 1970-01-01 -> YYYY-MM-DD in the proleptic Gregorian calendar (the inverse of vnm_csv.hip's days_from_civil): eras of
// 400 years = 146097 days, the year beginning on March 1st
VNM_HD int64_t ts_put_date(uint8_t* q, int64_t o, int64_t room, int64_t days) {
    const int64_t z = days + 719468;
    const int64_t era = ts_floor_div(z, 146097), doe = z - era * 146097;                    // [0, 146096]
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;              // [0, 399]
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                            // [0, 365]
    const int64_t mp = (5 * doy + 2) / 153;                                                 // [0, 11]: March = 0
    const int64_t d = doy - (153 * mp + 2) / 5 + 1, m = mp < 10 ? mp + 3 : mp - 9;
    const int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
    o = ts_put_signed(q, o, room, y, 4);
    o = ts_put(q, o, room, '-');
    o = ts_put_digits(q, o, room, (uint64_t)m, 2);
    o = ts_put(q, o, room, '-');
    return ts_put_digits(q, o, room, (uint64_t)d, 2);
}

// the image of `value` under `kind` into q[0 .. room): its length, -1 when a store would have left the room.  q == nullptr: the length alone
VNM_HD int64_t ts_image(uint8_t* q, int64_t room, int kind, int64_t value) {
    int64_t o = 0;
    if (kind == TS_NONE) {
        const uint8_t none[4] = {'N', 'o', 'n', 'e'};
        for (int k = 0; k < 4; k++) o = ts_put(q, o, room, none[k]);
        return o;
    }
    if (kind == TS_INT) return ts_put_signed(q, o, room, value, 1);
    if (kind == TS_UINT) return ts_put_digits(q, o, room, (uint64_t)value, 1);
    if (kind == TS_DATE32) return ts_put_date(q, o, room, value);
    if (kind < TS_TIMESTAMP_S || kind > TS_TIMESTAMP_NS) return -1;
    if (value == INT64_MIN) {                                                               // NumPy's NaT
        const uint8_t nat[3] = {'N', 'a', 'T'};
        for (int k = 0; k < 3; k++) o = ts_put(q, o, room, nat[k]);
        return o;
    }
    const int64_t per_s = kind == TS_TIMESTAMP_S ? 1 : kind == TS_TIMESTAMP_MS ? 1000 : kind == TS_TIMESTAMP_US ? 1000000 : 1000000000;
    const int frac_width = kind == TS_TIMESTAMP_S ? 0 : kind == TS_TIMESTAMP_MS ? 3 : kind == TS_TIMESTAMP_US ? 6 : 9;
    const int64_t secs = ts_floor_div(value, per_s), frac = ts_floor_mod(value, per_s);
    const int64_t days = ts_floor_div(secs, 86400), sod = ts_floor_mod(secs, 86400);
    o = ts_put_date(q, o, room, days);
    o = ts_put(q, o, room, 'T');
    o = ts_put_digits(q, o, room, (uint64_t)(sod / 3600), 2);
    o = ts_put(q, o, room, ':');
    o = ts_put_digits(q, o, room, (uint64_t)(sod / 60 % 60), 2);
    o = ts_put(q, o, room, ':');
    o = ts_put_digits(q, o, room, (uint64_t)(sod % 60), 2);
    if (frac_width) {
        o = ts_put(q, o, room, '.');
        o = ts_put_digits(q, o, room, (uint64_t)frac, frac_width);
    }
    return o;
}

// ts_room: the exact byte length of the image.  ts_write: the bytes written (== the room it was given when that came from ts_room)
// or -1 when a store would have left q[0 .. room) -- every store is held against the room first, as sc_put does
VNM_HD int64_t ts_room(int kind, int64_t value) { return ts_image(nullptr, 0, kind, value); }
VNM_HD int64_t ts_write(uint8_t* q, int64_t room, int kind, int64_t value) { return q ? ts_image(q, room, kind, value) : -1; }

}  // namespace vnm
