// date() / datetime() / from_timestamp() (DateFunction / DatetimeFunction / TimestampFunction, vinum/core/functions.py:25-137).
// Included at the end of vnm_strdict.hip: the parse pass reads a dictionary's heap and id tables.
//
// Over a STRING column the function depends on the value alone, so it is the inverse of to_str(): vnm_strdict_parse_datetime parses each
// distinct value ONCE (one lane per id over the heap, vnm_dtparse.hpp) into a per-id table of int64 values and status bytes, and
// vnm_strdict_gather_temporal is the row pass: one code load, one 8-byte gather through L2, one validity bit.  Over a date32 /
// timestamp column the function is a change of unit: vnm_temporal_rescale.
#include <type_traits>

#include "vnm_dtparse.hpp"

namespace vnm {

struct DtParseArgs {
    const uint8_t* heap;
    const int64_t* id_off;
    const int32_t* id_len;
    int64_t id_begin, id_end;
    int unit;
    int64_t* value;                // [id_end]
    uint8_t* status;               // [id_end]
    unsigned long long* refused;   // the lowest refused id handed out; ~0 while there is none
};

__global__ __launch_bounds__(256) void dt_parse_kernel(DtParseArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long lowest = ~0ULL;
    for (int64_t id = a.id_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; id < a.id_end; id += stride) {
        const int32_t len = a.id_len[id];
        int64_t v = 0;
        int st = DT_REFUSED;                                   // (an id never handed out: no row holds it)
        if (len >= 0) {
            st = dt_parse(a.heap + a.id_off[id], len, a.unit, &v);
            if (st == DT_REFUSED && (unsigned long long)id < lowest) lowest = (unsigned long long)id;
        }
        a.value[id] = v;
        a.status[id] = (uint8_t)st;
    }
    if (lowest != ~0ULL) atomicMin(a.refused, lowest);
}

// The row pass.  One lane takes DT_ROWS = 8 consecutive rows: their codes in two 16-byte loads, their values in four (int64) or two
// (int32) 16-byte stores when row 0 of both is aligned, element by element otherwise and in the last, partial group; 8 validity bits
// = ONE byte of the output bitmap, which no other lane touches.  The last byte keeps its bits past n (the one lane that owns it reads
// it first).  A code outside [0, n_ids) is never an address.  A non-NULL row whose id was refused keeps the table's 0 and is reported:
// the lowest such id goes back to the host, which raises naming the value.
constexpr int DT_ROWS = 8;
constexpr int DT_TILE = 256 * DT_ROWS;

struct DtGatherArgs {
    const int32_t* codes;          // row 0's code
    const uint8_t* valid;          // bit `vfirst` belongs to row 0 (or null)
    int64_t vfirst, n, ntiles, n_ids;
    const int64_t* value;          // [n_ids]
    const uint8_t* status;         // [n_ids]
    void* out;
    uint8_t* out_valid;            // bitmap at bit offset 0
    unsigned long long* nulls;     // (or null: not counted)
    unsigned long long* refused;   // the lowest refused id a non-NULL row holds; ~0 while there is none (or null: not looked for)
    int vec_in, vec_out;
};

template <typename OUT>
__global__ __launch_bounds__(256) void dt_gather_kernel(DtGatherArgs a) {
    __shared__ unsigned s_nulls;
    if (threadIdx.x == 0) s_nulls = 0;
    __syncthreads();
    unsigned nnull = 0;
    unsigned long long lowest = ~0ULL;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * DT_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < DT_ROWS ? (int)(a.n - row0) : DT_ROWS;
        const bool full = cnt == DT_ROWS;
        int32_t c[DT_ROWS];
        if (a.vec_in && full) {
            const int4 q0 = ((const int4*)(a.codes + row0))[0], q1 = ((const int4*)(a.codes + row0))[1];
            c[0] = q0.x; c[1] = q0.y; c[2] = q0.z; c[3] = q0.w; c[4] = q1.x; c[5] = q1.y; c[6] = q1.z; c[7] = q1.w;
        } else {
#pragma unroll
            for (int k = 0; k < DT_ROWS; k++) c[k] = k < cnt ? a.codes[row0 + k] : -1;
        }
        unsigned vbits = 0xFFu;
        if (a.valid) {   // bits vfirst + row0 ... + 7: at most two bytes of the bitmap, the second only if it exists
            const int64_t bit = a.vfirst + row0, last_byte = (a.vfirst + a.n - 1) >> 3;
            const int sh = (int)(bit & 7);
            vbits = (unsigned)a.valid[bit >> 3] >> sh;
            if (sh && (bit >> 3) + 1 <= last_byte) vbits |= (unsigned)a.valid[(bit >> 3) + 1] << (8 - sh);
        }
        const unsigned mask = (1u << cnt) - 1;
        vbits &= mask;
        OUT v[DT_ROWS];
        unsigned obits = 0;
#pragma unroll
        for (int k = 0; k < DT_ROWS; k++) {
            int64_t x = 0;
            if (((vbits >> k) & 1) && c[k] >= 0 && (int64_t)c[k] < a.n_ids) {
                const uint8_t st = a.status[c[k]];
                if (st != DT_NULL) {
                    x = a.value[c[k]];
                    obits |= 1u << k;
                    if (st == DT_REFUSED && (unsigned long long)c[k] < lowest) lowest = (unsigned long long)c[k];
                }
            }
            v[k] = (OUT)x;
        }
        nnull += (unsigned)__popc(mask & ~obits);
        OUT* o = (OUT*)a.out + row0;
        if (a.vec_out && full) {
            uint4 q[sizeof(OUT) / 2];
            __builtin_memcpy(q, v, sizeof(v));
#pragma unroll
            for (int j = 0; j < (int)(sizeof(OUT) / 2); j++) ((uint4*)o)[j] = q[j];
        } else {
#pragma unroll
            for (int k = 0; k < DT_ROWS; k++)
                if (k < cnt) o[k] = v[k];
        }
        uint8_t* ob = a.out_valid + (row0 >> 3);
        *ob = full ? (uint8_t)obits : (uint8_t)((*ob & ~mask) | obits);
    }
    if (a.nulls) {
        if (nnull) atomicAdd(&s_nulls, nnull);
        __syncthreads();
        if (threadIdx.x == 0 && s_nulls) atomicAdd(a.nulls, (unsigned long long)s_nulls);
    }
    if (a.refused && lowest != ~0ULL) atomicMin(a.refused, lowest);
}

// a change of unit: floor division to a coarser one, a wrapping multiplication (unsigned) to a finer one.  The floor of a negative
// value is NumPy's own formula, (v - (div - 1)) / div truncated, the subtraction wrapping (unsigned) as NumPy's does: within div - 1 of
// INT64_MIN its result is the wrapped one, everywhere else the floor.  INT64_MIN in an 8-byte input is NumPy's NaT and stays INT64_MIN
// in an 8-byte output, as NumPy's cast keeps it
template <typename IN, typename OUT>
__global__ __launch_bounds__(256) void dt_rescale_kernel(const IN* in, int64_t n, int64_t mul, int64_t div, OUT* out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t v = (int64_t)in[i];
        int64_t r;
        if (sizeof(IN) == 8 && sizeof(OUT) == 8 && v == INT64_MIN) r = v;
        else if (div > 1) r = v >= 0 ? v / div : (int64_t)((uint64_t)v - (uint64_t)(div - 1)) / div;
        else r = (int64_t)((uint64_t)v * (uint64_t)mul);
        out[i] = (OUT)r;
    }
}

// Arithmetic on temporal values: out[i] = a[i] * ka + b[i] * kb + c over up to two date32 (4-byte) / timestamp / duration (8-byte)
// columns, exact in int64 and wrapping (unsigned) as NumPy's does.  The shape is dt_gather_kernel's: a lane takes DT_ROWS rows --
// 16-byte loads and stores where row 0 of a buffer is aligned, element by element otherwise and in the last, partial group --, reads
// at most two bytes of each operand's validity and writes ONE whole byte of the output bitmap.  NumPy's NaT rule: a row is NULL when
// either input row is NULL, an 8-byte input holds INT64_MIN or the 64-bit result is INT64_MIN; a NULL row's value is 0.
struct DtAffineArgs {
    const void* a;                 // row 0's value
    const void* b;                 // (or null: one operand)
    const uint8_t* a_valid;        // bit `a_vfirst` belongs to row 0 (or null)
    const uint8_t* b_valid;
    int64_t a_vfirst, b_vfirst, n, ntiles;
    int64_t ka, kb, c;
    void* out;
    uint8_t* out_valid;            // bitmap at bit offset 0
    unsigned long long* nulls;     // (or null: not counted)
    int vec_a, vec_b, vec_out;
};

// 8 validity bits of rows row0 ... row0 + 7: at most two bytes of the bitmap, the second only if it exists
__device__ __forceinline__ unsigned dt_valid_bits(const uint8_t* valid, int64_t vfirst, int64_t row0, int64_t n) {
    if (!valid) return 0xFFu;
    const int64_t bit = vfirst + row0, last_byte = (vfirst + n - 1) >> 3;
    const int sh = (int)(bit & 7);
    unsigned v = (unsigned)valid[bit >> 3] >> sh;
    if (sh && (bit >> 3) + 1 <= last_byte) v |= (unsigned)valid[(bit >> 3) + 1] << (8 - sh);
    return v & 0xFFu;
}

// DT_ROWS values of type T from p: whole 16-byte loads (`vec`: p is 16-byte aligned and the group is full), else the first cnt one by one
template <typename T>
__device__ __forceinline__ void dt_load_rows(const T* p, bool vec, int cnt, T (&v)[DT_ROWS]) {
    if (vec) {
        uint4 q[sizeof(T) / 2];
#pragma unroll
        for (int j = 0; j < (int)(sizeof(T) / 2); j++) q[j] = ((const uint4*)p)[j];
        __builtin_memcpy(v, q, sizeof(v));
    } else {
#pragma unroll
        for (int k = 0; k < DT_ROWS; k++) v[k] = k < cnt ? p[k] : (T)0;
    }
}

struct DtNoColumn {};              // the absent second operand

template <typename A, typename B, typename OUT>
__global__ __launch_bounds__(256) void dt_affine_kernel(DtAffineArgs a) {
    constexpr bool TWO = !std::is_same<B, DtNoColumn>::value;
    using BT = typename std::conditional<TWO, B, int32_t>::type;
    __shared__ unsigned s_nulls;
    if (threadIdx.x == 0) s_nulls = 0;
    __syncthreads();
    unsigned nnull = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * DT_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < DT_ROWS ? (int)(a.n - row0) : DT_ROWS;
        const bool full = cnt == DT_ROWS;
        const unsigned mask = (1u << cnt) - 1;
        A x[DT_ROWS];
        BT y[DT_ROWS];
        dt_load_rows((const A*)a.a + row0, a.vec_a && full, cnt, x);
        unsigned vbits = dt_valid_bits(a.a_valid, a.a_vfirst, row0, a.n) & mask;
        if (TWO) {
            dt_load_rows((const BT*)a.b + row0, a.vec_b && full, cnt, y);
            vbits &= dt_valid_bits(a.b_valid, a.b_vfirst, row0, a.n);
        }
        OUT v[DT_ROWS];
        unsigned obits = 0;
#pragma unroll
        for (int k = 0; k < DT_ROWS; k++) {
            bool ok = (vbits >> k) & 1;
            if (sizeof(A) == 8) ok = ok && (int64_t)x[k] != INT64_MIN;
            uint64_t r = (uint64_t)(int64_t)x[k] * (uint64_t)a.ka + (uint64_t)a.c;
            if (TWO) {
                if (sizeof(BT) == 8) ok = ok && (int64_t)y[k] != INT64_MIN;
                r += (uint64_t)(int64_t)y[k] * (uint64_t)a.kb;
            }
            ok = ok && (int64_t)r != INT64_MIN;              // (the 64-bit result, whatever the output's width: NumPy computes in int64)
            v[k] = ok ? (OUT)(int64_t)r : (OUT)0;
            obits |= (unsigned)ok << k;
        }
        nnull += (unsigned)__popc(mask & ~obits);
        OUT* o = (OUT*)a.out + row0;
        if (a.vec_out && full) {
            uint4 q[sizeof(OUT) / 2];
            __builtin_memcpy(q, v, sizeof(v));
#pragma unroll
            for (int j = 0; j < (int)(sizeof(OUT) / 2); j++) ((uint4*)o)[j] = q[j];
        } else {
#pragma unroll
            for (int k = 0; k < DT_ROWS; k++)
                if (k < cnt) o[k] = v[k];
        }
        uint8_t* ob = a.out_valid + (row0 >> 3);
        *ob = full ? (uint8_t)obits : (uint8_t)((*ob & ~mask) | obits);
    }
    if (a.nulls) {
        if (nnull) atomicAdd(&s_nulls, nnull);
        __syncthreads();
        if (threadIdx.x == 0 && s_nulls) atomicAdd(a.nulls, (unsigned long long)s_nulls);
    }
}

// duration // duration (np.floor_divide over timedelta64): out[i] = floor(x / y) as int64, x = a[i] * ka and y = b[i] * kb with the unit
// factors in ka / kb (wrapping as above); an absent column (DtNoColumn) makes its side the constant ka / kb itself.  The same lane
// shape and DtAffineArgs.  A NULL or NaT input row is NULL (value 0); a zero divisor gives 0, as NumPy does.
template <typename A, typename B>
__global__ __launch_bounds__(256) void dt_floordiv_kernel(DtAffineArgs a) {
    constexpr bool HAS_A = !std::is_same<A, DtNoColumn>::value, HAS_B = !std::is_same<B, DtNoColumn>::value;
    using AT = typename std::conditional<HAS_A, A, int32_t>::type;
    using BT = typename std::conditional<HAS_B, B, int32_t>::type;
    __shared__ unsigned s_nulls;
    if (threadIdx.x == 0) s_nulls = 0;
    __syncthreads();
    unsigned nnull = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * DT_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < DT_ROWS ? (int)(a.n - row0) : DT_ROWS;
        const bool full = cnt == DT_ROWS;
        const unsigned mask = (1u << cnt) - 1;
        AT x[DT_ROWS];
        BT y[DT_ROWS];
        unsigned vbits = mask;
        if (HAS_A) {
            dt_load_rows((const AT*)a.a + row0, a.vec_a && full, cnt, x);
            vbits &= dt_valid_bits(a.a_valid, a.a_vfirst, row0, a.n);
        }
        if (HAS_B) {
            dt_load_rows((const BT*)a.b + row0, a.vec_b && full, cnt, y);
            vbits &= dt_valid_bits(a.b_valid, a.b_vfirst, row0, a.n);
        }
        int64_t v[DT_ROWS];
        unsigned obits = 0;
#pragma unroll
        for (int k = 0; k < DT_ROWS; k++) {
            bool ok = (vbits >> k) & 1;
            int64_t p = a.ka, q = a.kb;
            if (HAS_A) {
                if (sizeof(AT) == 8) ok = ok && (int64_t)x[k] != INT64_MIN;
                p = (int64_t)((uint64_t)(int64_t)x[k] * (uint64_t)a.ka);
            }
            if (HAS_B) {
                if (sizeof(BT) == 8) ok = ok && (int64_t)y[k] != INT64_MIN;
                q = (int64_t)((uint64_t)(int64_t)y[k] * (uint64_t)a.kb);
            }
            int64_t r = 0;
            if (ok && q != 0) {
                if (q == -1) r = (int64_t)(0 - (uint64_t)p);           // (INT64_MIN / -1 has no quotient: it wraps)
                else {
                    r = p / q;
                    if ((p % q != 0) && ((p < 0) != (q < 0))) r -= 1;    // truncation -> floor
                }
            }
            v[k] = r;
            obits |= (unsigned)ok << k;
        }
        nnull += (unsigned)__popc(mask & ~obits);
        int64_t* o = (int64_t*)a.out + row0;
        if (a.vec_out && full) {
            uint4 w[4];
            __builtin_memcpy(w, v, sizeof(v));
#pragma unroll
            for (int j = 0; j < 4; j++) ((uint4*)o)[j] = w[j];
        } else {
#pragma unroll
            for (int k = 0; k < DT_ROWS; k++)
                if (k < cnt) o[k] = v[k];
        }
        uint8_t* ob = a.out_valid + (row0 >> 3);
        *ob = full ? (uint8_t)obits : (uint8_t)((*ob & ~mask) | obits);
    }
    if (a.nulls) {
        if (nnull) atomicAdd(&s_nulls, nnull);
        __syncthreads();
        if (threadIdx.x == 0 && s_nulls) atomicAdd(a.nulls, (unsigned long long)s_nulls);
    }
}

// is_busday(date32 column): mask[i] = the weekmask's bit of the day's weekday (bit 0 Monday; day 0, 1970-01-01, is a Thursday) AND the
// day is in no holiday.  The weekday is branch-free for negative days: DT_WEEK_BIAS = 3 + a multiple of 7 that is >= 2^31 makes the sum
// non-negative in 64 bits before the unsigned % 7.  The holidays -- sorted, distinct, at most DT_MAX_HOLIDAYS -- are staged into LDS
// and probed with the branch-free lower bound of the IN probe (vnm_inset.hip).  A NULL row gives 0 (np.is_busday(NaT) is False).
constexpr int DT_MAX_HOLIDAYS = 8192;                          // 32 KB of LDS
constexpr uint64_t DT_WEEK_BIAS = 3ull + 7ull * 306783379ull;  // 7 * 306783379 = 2^31 + 5

struct DtBusdayArgs {
    const int32_t* days;           // row 0's day
    const uint8_t* valid;          // bit `vfirst` belongs to row 0 (or null)
    int64_t vfirst, n, ntiles;
    const int32_t* holidays;
    int n_holidays;
    unsigned weekmask;
    uint8_t* out;
    int vec_in, vec_out;
};

__global__ __launch_bounds__(256) void dt_busday_kernel(DtBusdayArgs a) {
    __shared__ int32_t s_hol[DT_MAX_HOLIDAYS];
    for (int k = threadIdx.x; k < a.n_holidays; k += 256) s_hol[k] = a.holidays[k];
    if (a.n_holidays == 0 && threadIdx.x == 0) s_hol[0] = 0;
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * DT_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < DT_ROWS ? (int)(a.n - row0) : DT_ROWS;
        const bool full = cnt == DT_ROWS;
        int32_t d[DT_ROWS];
        dt_load_rows(a.days + row0, a.vec_in && full, cnt, d);
        const unsigned vbits = dt_valid_bits(a.valid, a.vfirst, row0, a.n) & ((1u << cnt) - 1);
        uint8_t m[DT_ROWS];
#pragma unroll
        for (int k = 0; k < DT_ROWS; k++) {
            const unsigned wd = (unsigned)(((uint64_t)((int64_t)d[k]) + DT_WEEK_BIAS) % 7u);
            uint32_t base = 0, len = (uint32_t)a.n_holidays;
            while (len > 1) {      // `len` is uniform: every lane takes the same ceil(log2 n) steps
                const uint32_t half = len >> 1;
                base += s_hol[base + half - 1] < d[k] ? half : 0;
                len -= half;
            }
            const unsigned holiday = (a.n_holidays > 0) & (s_hol[base] == d[k]);
            m[k] = (uint8_t)(((vbits >> k) & 1) & ((a.weekmask >> wd) & 1) & (holiday ^ 1u));
        }
        uint8_t* o = a.out + row0;
        if (a.vec_out && full) {
            uint2 q;
            __builtin_memcpy(&q, m, 8);
            *(uint2*)o = q;
        } else {
#pragma unroll
            for (int k = 0; k < DT_ROWS; k++)
                if (k < cnt) o[k] = m[k];
        }
    }
}

// 4 for a date32 (VNM_I32) column, 8 for a timestamp / duration (VNM_I64) one, 0 for every other type
inline int temporal_width(const vnm_dcol* col) { return col->type == VNM_I32 ? 4 : col->type == VNM_I64 ? 8 : 0; }

template <typename A, typename B>
void affine_launch(int out_width, int grid, hipStream_t s, const DtAffineArgs& a) {
    if (out_width == 4) dt_affine_kernel<A, B, int32_t><<<grid, 256, 0, s>>>(a);
    else dt_affine_kernel<A, B, int64_t><<<grid, 256, 0, s>>>(a);
}

template <typename A>
void affine_launch_b(int b_width, int out_width, int grid, hipStream_t s, const DtAffineArgs& a) {
    if (b_width == 0) affine_launch<A, DtNoColumn>(out_width, grid, s, a);
    else if (b_width == 4) affine_launch<A, int32_t>(out_width, grid, s, a);
    else affine_launch<A, int64_t>(out_width, grid, s, a);
}

template <typename A>
void floordiv_launch_b(int b_width, int grid, hipStream_t s, const DtAffineArgs& a) {
    if (b_width == 0) dt_floordiv_kernel<A, DtNoColumn><<<grid, 256, 0, s>>>(a);
    else if (b_width == 4) dt_floordiv_kernel<A, int32_t><<<grid, 256, 0, s>>>(a);
    else dt_floordiv_kernel<A, int64_t><<<grid, 256, 0, s>>>(a);
}

}  // namespace vnm

extern "C" {

int vnm_strdict_parse_datetime(vnm_strdict* h, int unit, int64_t id_begin, int64_t* out_value_of_id, uint8_t* out_status_of_id,
                               int64_t* out_first_refused_id, void* stream) {
    VNM_TRY(ensure_init());
    if (out_first_refused_id) *out_first_refused_id = -1;
    if (!h || !out_value_of_id || !out_status_of_id) return set_error("vnm_strdict_parse_datetime: null argument");
    if (h->failed) return set_error("vnm_strdict: an earlier encode failed half-way; the dictionary cannot be used any more (create a new one)");
    if (unit < VNM_UNIT_D || unit > VNM_UNIT_NS) return set_error("vnm_strdict_parse_datetime: unknown unit %d", unit);
    if (id_begin < 0) return set_error("vnm_strdict_parse_datetime: id_begin < 0");
    if (id_begin >= h->ids) return 0;
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    DtParseArgs a{};
    a.heap = h->heap; a.id_off = h->id_off; a.id_len = h->id_len;
    a.id_begin = id_begin; a.id_end = h->ids; a.unit = unit;
    a.value = out_value_of_id; a.status = out_status_of_id;
    a.refused = (unsigned long long*)pool.take(8);
    if (!a.refused) return 1;
    VNM_HIP(hipMemsetAsync(a.refused, 0xFF, 8, s));
    const int grid = (int)std::min<int64_t>((h->ids - id_begin + 255) / 256, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("strdict_parse_datetime", s);
        dt_parse_kernel<<<grid, 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long refused = ~0ULL;
    VNM_HIP(hipMemcpyAsync(&refused, a.refused, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (out_first_refused_id) *out_first_refused_id = refused == ~0ULL ? -1 : (int64_t)refused;
    return 0;
}

int vnm_strdict_gather_temporal(const int32_t* codes, const uint8_t* validity, int64_t validity_offset, const int64_t* value_of_id,
                                const uint8_t* status_of_id, int64_t n_ids, int64_t n, int out_width, void* out_values, uint8_t* out_validity_bitmap,
                                int64_t* out_null_count, int64_t* out_first_refused_id, void* stream) {
    VNM_TRY(ensure_init());
    if (out_null_count) *out_null_count = 0;
    if (out_first_refused_id) *out_first_refused_id = -1;
    if (out_width != 4 && out_width != 8) return set_error("vnm_strdict_gather_temporal: out_width must be 4 or 8, not %d", out_width);
    if (n <= 0) return 0;
    if (!codes || !out_values || !out_validity_bitmap || n_ids < 0 || (n_ids > 0 && (!value_of_id || !status_of_id)) || validity_offset < 0)
        return set_error("vnm_strdict_gather_temporal: null argument");
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    DtGatherArgs a{};
    a.codes = codes; a.valid = validity; a.vfirst = validity_offset; a.n = n; a.n_ids = n_ids;
    a.value = value_of_id; a.status = status_of_id; a.out = out_values; a.out_valid = out_validity_bitmap;
    a.vec_in = ((uintptr_t)codes & 15) == 0;
    a.vec_out = ((uintptr_t)out_values & 15) == 0;
    const int64_t tiles = (n + DT_TILE - 1) / DT_TILE;
    a.ntiles = tiles;
    if (out_null_count) {
        a.nulls = (unsigned long long*)pool.take(8);
        if (!a.nulls) return 1;
        VNM_HIP(hipMemsetAsync(a.nulls, 0, 8, s));
    }
    if (out_first_refused_id) {
        a.refused = (unsigned long long*)pool.take(8);
        if (!a.refused) return 1;
        VNM_HIP(hipMemsetAsync(a.refused, 0xFF, 8, s));
    }
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("strdict_gather_temporal", s);
        if (out_width == 4) dt_gather_kernel<int32_t><<<grid, 256, 0, s>>>(a);
        else dt_gather_kernel<int64_t><<<grid, 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    if (!out_null_count && !out_first_refused_id) return 0;
    unsigned long long nulls = 0, refused = ~0ULL;
    if (out_null_count) VNM_HIP(hipMemcpyAsync(&nulls, a.nulls, 8, hipMemcpyDeviceToHost, s));
    if (out_first_refused_id) VNM_HIP(hipMemcpyAsync(&refused, a.refused, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (out_null_count) *out_null_count = (int64_t)nulls;
    if (out_first_refused_id) *out_first_refused_id = refused == ~0ULL ? -1 : (int64_t)refused;
    return 0;
}

int vnm_temporal_rescale(const vnm_dcol* col, int64_t mul, int64_t div, int64_t length, int out_width, void* out_values, void* stream) {
    VNM_TRY(ensure_init());
    if (!col) return set_error("vnm_temporal_rescale: null argument");
    if (out_width != 4 && out_width != 8) return set_error("vnm_temporal_rescale: out_width must be 4 or 8, not %d", out_width);
    if (col->type < VNM_I8 || col->type > VNM_U32)
        return set_error("vnm_temporal_rescale: the column must be a date32 (VNM_I32), timestamp (VNM_I64) or integer column narrower than VNM_U64");
    if (mul < 1 || div < 1 || (mul > 1 && div > 1)) return set_error("vnm_temporal_rescale: one of mul / div is 1, the other >= 1 (got %lld / %lld)", (long long)mul, (long long)div);
    if (length < 0 || col->offset < 0 || length > col->length) return set_error("vnm_temporal_rescale: length outside the column");
    if (length == 0) return 0;
    if (!col->values || !out_values) return set_error("vnm_temporal_rescale: null argument");
    hipStream_t s = as_stream(stream);
    const int grid = (int)std::min<int64_t>((length + 255) / 256, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("temporal_rescale", s);
#define VNM_RESCALE_LAUNCH(T)                                                                                        \
    do {                                                                                                             \
        const T* in = (const T*)col->values + col->offset;                                                           \
        if (out_width == 4) dt_rescale_kernel<<<grid, 256, 0, s>>>(in, length, mul, div, (int32_t*)out_values);       \
        else dt_rescale_kernel<<<grid, 256, 0, s>>>(in, length, mul, div, (int64_t*)out_values);                      \
    } while (0)
        switch (col->type) {
            case VNM_I8: VNM_RESCALE_LAUNCH(int8_t); break;
            case VNM_I16: VNM_RESCALE_LAUNCH(int16_t); break;
            case VNM_I32: VNM_RESCALE_LAUNCH(int32_t); break;
            case VNM_I64: VNM_RESCALE_LAUNCH(int64_t); break;
            case VNM_U8: VNM_RESCALE_LAUNCH(uint8_t); break;
            case VNM_U16: VNM_RESCALE_LAUNCH(uint16_t); break;
            default: VNM_RESCALE_LAUNCH(uint32_t); break;
        }
#undef VNM_RESCALE_LAUNCH
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

int vnm_temporal_affine(const vnm_dcol* a, int64_t ka, const vnm_dcol* b, int64_t kb, int64_t c, int64_t length, int out_width,
                        void* out_values, uint8_t* out_validity_bitmap, int64_t* out_null_count, void* stream) {
    VNM_TRY(ensure_init());
    if (out_null_count) *out_null_count = 0;
    if (!a) return set_error("vnm_temporal_affine: null argument");
    if (out_width != 4 && out_width != 8) return set_error("vnm_temporal_affine: out_width must be 4 or 8, not %d", out_width);
    const int wa = temporal_width(a), wb = b ? temporal_width(b) : 0;
    if (!wa || (b && !wb))
        return set_error("vnm_temporal_affine: an operand must be 4 bytes (date32, VNM_I32) or 8 bytes (timestamp / duration, VNM_I64) wide");
    if (length < 0 || a->offset < 0 || length > a->length || (b && (b->offset < 0 || length > b->length)))
        return set_error("vnm_temporal_affine: length outside the column");
    if (length == 0) return 0;
    if (!a->values || (b && !b->values) || !out_values || !out_validity_bitmap) return set_error("vnm_temporal_affine: null argument");
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    DtAffineArgs k{};
    k.a = (const uint8_t*)a->values + a->offset * wa;
    k.a_valid = (const uint8_t*)a->validity; k.a_vfirst = a->offset;
    if (b) {
        k.b = (const uint8_t*)b->values + b->offset * wb;
        k.b_valid = (const uint8_t*)b->validity; k.b_vfirst = b->offset;
    }
    k.ka = ka; k.kb = b ? kb : 0; k.c = c; k.n = length;
    k.out = out_values; k.out_valid = out_validity_bitmap;
    k.vec_a = ((uintptr_t)k.a & 15) == 0;
    k.vec_b = ((uintptr_t)k.b & 15) == 0;
    k.vec_out = ((uintptr_t)out_values & 15) == 0;
    const int64_t tiles = (length + DT_TILE - 1) / DT_TILE;
    k.ntiles = tiles;
    if (out_null_count) {
        k.nulls = (unsigned long long*)pool.take(8);
        if (!k.nulls) return 1;
        VNM_HIP(hipMemsetAsync(k.nulls, 0, 8, s));
    }
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("temporal_affine", s);
        if (wa == 4) affine_launch_b<int32_t>(wb, out_width, grid, s, k);
        else affine_launch_b<int64_t>(wb, out_width, grid, s, k);
    }
    VNM_HIP(hipGetLastError());
    if (!out_null_count) return 0;
    unsigned long long nulls = 0;
    VNM_HIP(hipMemcpyAsync(&nulls, k.nulls, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    *out_null_count = (int64_t)nulls;
    return 0;
}

int vnm_temporal_floordiv(const vnm_dcol* a, int64_t ka, const vnm_dcol* b, int64_t kb, int64_t length, int64_t* out_values,
                          uint8_t* out_validity_bitmap, int64_t* out_null_count, void* stream) {
    VNM_TRY(ensure_init());
    if (out_null_count) *out_null_count = 0;
    if (!a && !b) return set_error("vnm_temporal_floordiv: null argument (one side at least is a column)");
    const int wa = a ? temporal_width(a) : 0, wb = b ? temporal_width(b) : 0;
    if ((a && !wa) || (b && !wb))
        return set_error("vnm_temporal_floordiv: an operand must be 4 bytes (VNM_I32) or 8 bytes (duration, VNM_I64) wide");
    if (length < 0 || (a && (a->offset < 0 || length > a->length)) || (b && (b->offset < 0 || length > b->length)))
        return set_error("vnm_temporal_floordiv: length outside the column");
    if (length == 0) return 0;
    if ((a && !a->values) || (b && !b->values) || !out_values || !out_validity_bitmap) return set_error("vnm_temporal_floordiv: null argument");
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    DtAffineArgs k{};
    if (a) {
        k.a = (const uint8_t*)a->values + a->offset * wa;
        k.a_valid = (const uint8_t*)a->validity; k.a_vfirst = a->offset;
    }
    if (b) {
        k.b = (const uint8_t*)b->values + b->offset * wb;
        k.b_valid = (const uint8_t*)b->validity; k.b_vfirst = b->offset;
    }
    k.ka = ka; k.kb = kb; k.n = length;
    k.out = out_values; k.out_valid = out_validity_bitmap;
    k.vec_a = ((uintptr_t)k.a & 15) == 0;
    k.vec_b = ((uintptr_t)k.b & 15) == 0;
    k.vec_out = ((uintptr_t)out_values & 15) == 0;
    const int64_t tiles = (length + DT_TILE - 1) / DT_TILE;
    k.ntiles = tiles;
    if (out_null_count) {
        k.nulls = (unsigned long long*)pool.take(8);
        if (!k.nulls) return 1;
        VNM_HIP(hipMemsetAsync(k.nulls, 0, 8, s));
    }
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("temporal_floordiv", s);
        if (wa == 4) floordiv_launch_b<int32_t>(wb, grid, s, k);
        else if (wa == 8) floordiv_launch_b<int64_t>(wb, grid, s, k);
        else if (wb == 4) dt_floordiv_kernel<DtNoColumn, int32_t><<<grid, 256, 0, s>>>(k);
        else dt_floordiv_kernel<DtNoColumn, int64_t><<<grid, 256, 0, s>>>(k);
    }
    VNM_HIP(hipGetLastError());
    if (!out_null_count) return 0;
    unsigned long long nulls = 0;
    VNM_HIP(hipMemcpyAsync(&nulls, k.nulls, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    *out_null_count = (int64_t)nulls;
    return 0;
}

int vnm_temporal_busday(const vnm_dcol* days, int64_t length, int weekmask, const int32_t* holidays, int64_t n_holidays, uint8_t* out_mask,
                        void* stream) {
    VNM_TRY(ensure_init());
    if (!days) return set_error("vnm_temporal_busday: null argument");
    if (temporal_width(days) != 4) return set_error("vnm_temporal_busday: the column must be 4 bytes wide (date32, VNM_I32)");
    if (weekmask < 0 || weekmask > 127) return set_error("vnm_temporal_busday: the weekmask has 7 bits (bit 0 Monday), not %d", weekmask);
    if (n_holidays < 0 || n_holidays > DT_MAX_HOLIDAYS)
        return set_error("ValueError: is_busday() takes at most %d holidays (32 KB of LDS), not %lld", DT_MAX_HOLIDAYS, (long long)n_holidays);
    if (length < 0 || days->offset < 0 || length > days->length) return set_error("vnm_temporal_busday: length outside the column");
    if (length == 0) return 0;
    if (!days->values || !out_mask || (n_holidays > 0 && !holidays)) return set_error("vnm_temporal_busday: null argument");
    hipStream_t s = as_stream(stream);
    DtBusdayArgs k{};
    k.days = (const int32_t*)days->values + days->offset;
    k.valid = (const uint8_t*)days->validity; k.vfirst = days->offset; k.n = length;
    k.holidays = holidays; k.n_holidays = (int)n_holidays; k.weekmask = (unsigned)weekmask;
    k.out = out_mask;
    k.vec_in = ((uintptr_t)k.days & 15) == 0;
    k.vec_out = ((uintptr_t)out_mask & 7) == 0;
    const int64_t tiles = (length + DT_TILE - 1) / DT_TILE;
    k.ntiles = tiles;
    const int grid = (int)std::min<int64_t>(tiles, (int64_t)device_info().num_cus * 16);
    {
        KernelTimer timer("temporal_busday", s);
        dt_busday_kernel<<<grid, 256, 0, s>>>(k);
    }
    VNM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
