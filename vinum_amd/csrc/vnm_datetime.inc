// date() / datetime() / from_timestamp() (DateFunction / DatetimeFunction / TimestampFunction, vinum/core/functions.py:25-137).
// Included at the end of vnm_strdict.hip: the parse pass reads a dictionary's heap and id tables.
//
// Over a STRING column the function depends on the value alone, so it is the inverse of to_str(): vnm_strdict_parse_datetime parses each
// distinct value ONCE (one lane per id over the heap, vnm_dtparse.hpp) into a per-id table of int64 values and status bytes, and
// vnm_strdict_gather_temporal is the row pass: one code load, one 8-byte gather through L2, one validity bit.  Over a date32 /
// timestamp column the function is a change of unit: vnm_temporal_rescale.
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

}  // extern "C"
