// One date() / datetime() value: the per-lane parser of dt_parse_kernel (vnm_datetime.hip), kept free of anything a host compiler does
// not know so that the same code runs under a host sanitizer against exactly-sized buffers (as vnm_tostr.hpp, whose inverse this is).
//
// DatetimeFunction / DateFunction (vinum/core/functions.py:25-128) compute np.array(column, dtype='datetime64[unit]'): NumPy's ISO 8601
// parser.  dt_parse takes one value's bytes and a target unit and gives an int64 -- days (DT_D) or unit counts since 1970-01-01 --
// and a status: DT_VALUE, DT_NULL (NumPy's NaT) or DT_REFUSED.  It reads no byte outside [p, p + len).
//
// Accepted, after trailing 0x00 bytes are dropped (a utf8 column without NULLs loses them on its way into the reference), are exactly
// the full matches of
//     \d{4}(-\d{2}(-\d{2}([T ]\d{2}(:\d{2}(:\d{2}(\.\d{0,9})?)?)?)?)?)?          (\d: the ten ASCII digits)
// whose fields are in range: month 01-12, day 01 to the month's end in the proleptic Gregorian calendar (year 0000 is a leap year),
// hour 00-23, minute and second 00-59.  Missing fields are 01 / 00.  The empty string and "NaT" in any letter case are DT_NULL.  The
// value is NumPy's: a coarser target FLOORS (1969-12-31T23:59:59.9 is -1 in s and in D; the time of day is never negative, so the
// floor is a truncation of the fraction).
// Refused though NumPy takes them: white space around the value, zone designators (Z, +01:00: NumPy itself deprecates them), "now" /
// "today", a year that is not exactly four digits or carries a sign, more than nine fraction digits, and for DT_NS an instant whose
// count does not fit int64 (NumPy wraps silently: 0000-01-01 prints as 1753-08-29).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VNM_HD __host__ __device__ __forceinline__
#else
#define VNM_HD inline
#endif

namespace vnm {

// (enum vnm_temporal_unit of include/vinum_hip.h, in its order)
enum { DT_D = 0, DT_S, DT_MS, DT_US, DT_NS };
enum { DT_VALUE = 0, DT_NULL = 1, DT_REFUSED = 2 };

// the two ASCII digits at p[at], p[at + 1] as a number; -1 when either is no digit or lies at or past len
VNM_HD int dt_two(const uint8_t* p, int64_t len, int64_t at) {
    if (at + 2 > len) return -1;
    const unsigned a = (unsigned)p[at] - '0', b = (unsigned)p[at + 1] - '0';
    return (a > 9 || b > 9) ? -1 : (int)(a * 10 + b);
}

// days since 1970-01-01 of y-m-d in the proleptic Gregorian calendar (vnm_csv.hip's days_from_civil; y >= 0 here)
VNM_HD int64_t dt_days_from_civil(int64_t y, int m, int d) {
    y -= m <= 2 ? 1 : 0;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;                                          // [0, 399]
    const int64_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;        // [0, 365]
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;                  // [0, 146096]
    return era * 146097 + doe - 719468;
}

VNM_HD int dt_days_in_month(int y, int m) {
    if (m == 2) return (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 29 : 28;
    return (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
}

// the value of p[0 .. len) under `unit` into *out (0 unless DT_VALUE); the status
VNM_HD int dt_parse(const uint8_t* p, int64_t len, int unit, int64_t* out) {
    *out = 0;
    if (unit < DT_D || unit > DT_NS || len < 0 || (len > 0 && !p)) return DT_REFUSED;
    while (len > 0 && p[len - 1] == 0) len--;
    if (len == 0) return DT_NULL;
    if (len == 3 && (p[0] | 0x20) == 'n' && (p[1] | 0x20) == 'a' && (p[2] | 0x20) == 't') return DT_NULL;
    if (len > 29) return DT_REFUSED;                                            // YYYY-MM-DDTHH:MM:SS.fffffffff
    const int hi = dt_two(p, len, 0), lo = dt_two(p, len, 2);
    if (hi < 0 || lo < 0) return DT_REFUSED;
    const int y = hi * 100 + lo;
    int mo = 1, d = 1, h = 0, mi = 0, s = 0;
    int64_t frac = 0;                                                           // nanoseconds
    int64_t at = 4;
    if (at < len) {                                                             // -MM
        if (p[at] != '-' || (mo = dt_two(p, len, at + 1)) < 0) return DT_REFUSED;
        at += 3;
        if (at < len) {                                                         // -DD
            if (p[at] != '-' || (d = dt_two(p, len, at + 1)) < 0) return DT_REFUSED;
            at += 3;
            if (at < len) {                                                     // [T ]HH
                if ((p[at] != 'T' && p[at] != ' ') || (h = dt_two(p, len, at + 1)) < 0) return DT_REFUSED;
                at += 3;
                if (at < len) {                                                 // :MM
                    if (p[at] != ':' || (mi = dt_two(p, len, at + 1)) < 0) return DT_REFUSED;
                    at += 3;
                    if (at < len) {                                             // :SS
                        if (p[at] != ':' || (s = dt_two(p, len, at + 1)) < 0) return DT_REFUSED;
                        at += 3;
                        if (at < len) {                                         // .f{0,9}
                            if (p[at] != '.' || len - (at + 1) > 9) return DT_REFUSED;
                            at++;
                            int64_t scale = 100000000;
                            for (; at < len; at++, scale /= 10) {
                                const unsigned c = (unsigned)p[at] - '0';
                                if (c > 9) return DT_REFUSED;
                                frac += (int64_t)c * scale;
                            }
                        }
                    }
                }
            }
        }
    }
    if (mo < 1 || mo > 12 || d < 1 || d > dt_days_in_month(y, mo) || h > 23 || mi > 59 || s > 59) return DT_REFUSED;
    const int64_t days = dt_days_from_civil(y, mo, d);
    const int64_t secs = days * 86400 + h * 3600 + mi * 60 + s;                 // [-62167219200, 253402300799]
    if (unit == DT_D) *out = days;
    else if (unit == DT_S) *out = secs;
    else if (unit == DT_MS) *out = secs * 1000 + frac / 1000000;
    else if (unit == DT_US) *out = secs * 1000000 + frac / 1000;
    else {
        // INT64_MIN = -9223372037 s + 145224192 ns, INT64_MAX = 9223372036 s + 854775807 ns
        if (secs < -9223372037LL || (secs == -9223372037LL && frac < 145224192)) return DT_REFUSED;
        if (secs > 9223372036LL || (secs == 9223372036LL && frac > 854775807)) return DT_REFUSED;
        // (the sum fits, the product alone need not: -9223372037 s is below INT64_MIN until the fraction is added)
        *out = secs < 0 ? (secs + 1) * 1000000000 + (frac - 1000000000) : secs * 1000000000 + frac;
    }
    return DT_VALUE;
}

}  // namespace vnm
