// Running codes of a device string dictionary -> a compact, typed dictionary column (vnm_dict_take_compact).
//
// A vnm_strdict hands its ids out in chunks, and a LIMIT or an aggregate's result uses only some of them: the Arrow column that
// leaves needs indices of the INPUT's index width into a dictionary without holes.  Three passes over c_i = codes[rows ? rows[i] : i]:
//   mark    used[c_i] = 1 -- plain one-byte stores of the same value into a zeroed n_ids-byte table, no atomics; a code outside
//           [0, n_ids) is held against n_ids BEFORE it is an address, counted, and fails the call;
//   scan    an exclusive scan over the table: dense_of_code[id] = how many used ids lie below id, used_ids[dense] = id
//           (per-workgroup counts, one workgroup over the counts, then the emit);
//   gather  out_indices[i] = (T)dense_of_code[c_i]: one lane takes DC_ROWS = 8 consecutive rows, as the remap kernel does -- 16-byte
//           code loads without `rows`, 8 / 16-byte index stores when out_indices is aligned, element by element otherwise and in the
//           last partial group; the 8 validity bits are ONE byte of the bitmap that no other lane touches.  dense_of_code is read
//           through L2, or from a copy in LDS (up to DC_LDS_IDS ids, 32 KB) by a persistent grid when the rows per workgroup pay
//           for the copy (VNM_DICT_COMPACT_LDS=0 / 1 pins the form).
#include <algorithm>

#include "vnm_common.hpp"

using namespace vnm;

namespace {

constexpr int DC_ROWS = 8;
constexpr int DC_TILE = 256 * DC_ROWS;      // rows per workgroup and step of the gather; ids per workgroup of the scan
constexpr int DC_LDS_IDS = 8192;            // the LDS form: dense_of_code of up to this many ids is copied into LDS (32 KB) per workgroup
static_assert(DC_TILE == VNM_DICT_COMPACT_TILE, "the header documents the kernel's rows per workgroup");
static_assert(DC_LDS_IDS == VNM_DICT_COMPACT_LDS_IDS, "the header documents the largest table of the LDS form");

struct DcArgs {
    const int32_t* codes;
    const int64_t* rows;            // null: identity
    int64_t n, n_ids, ntiles;
    uint8_t* used;                  // [n_ids rounded up to DC_TILE], zeroed
    unsigned long long* counters;   // [0] rows with a code >= n_ids, [1] NULL rows
    uint32_t* blk;                  // [nblocks] used ids per scan workgroup -> their exclusive prefix; [nblocks]: the total
    int nblocks;
    int32_t* dense;                 // [n_ids rounded up to DC_TILE]
    int32_t* used_ids;
    void* out;
    uint8_t* out_valid;             // bitmap at bit offset 0 (or null)
    int vec_in, vec_out;            // codes / out_indices are aligned for the wide loads / stores
};

__global__ __launch_bounds__(256) void dc_mark_kernel(DcArgs a) {
    __shared__ unsigned s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    unsigned nbad = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        const int32_t c = a.codes[a.rows ? a.rows[i] : i];
        if (c < 0) continue;
        if ((int64_t)c < a.n_ids) a.used[c] = 1;      // (every lane that hits this byte stores the same value)
        else nbad++;
    }
    if (nbad) atomicAdd(&s_bad, nbad);
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(a.counters, (unsigned long long)s_bad);
}

// the used ids among the DC_ROWS ids of this lane (the table is padded to whole tiles: one 8-byte load)
__device__ inline unsigned dc_lane_flags(const DcArgs& a, int64_t t, unsigned* cnt) {
    const uint2 q = *(const uint2*)(a.used + t * DC_ROWS);
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < DC_ROWS; k++) bits |= ((((k < 4 ? q.x : q.y) >> (8 * (k & 3))) & 0xFFu) ? 1u : 0u) << k;
    *cnt = (unsigned)__popc(bits);
    return bits;
}

__global__ __launch_bounds__(256) void dc_count_kernel(DcArgs a) {
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    unsigned cnt;
    dc_lane_flags(a, (int64_t)blockIdx.x * 256 + threadIdx.x, &cnt);
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = s_cnt;
}

// exclusive prefix of the workgroup counts (one workgroup)
__global__ __launch_bounds__(1024) void dc_scan_kernel(uint32_t* blk, int nblocks) {
    __shared__ uint32_t sc[1024];
    const int tid = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int lo = tid * per < nblocks ? tid * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
    uint32_t c = 0;
    for (int i = lo; i < hi; i++) c += blk[i];
    sc[tid] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan
        const uint32_t x = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += x;
        __syncthreads();
    }
    uint32_t run = sc[tid] - c;
    if (tid == 1023) blk[nblocks] = sc[1023];
    for (int i = lo; i < hi; i++) { const uint32_t x = blk[i]; blk[i] = run; run += x; }
}

__global__ __launch_bounds__(256) void dc_emit_kernel(DcArgs a) {
    __shared__ uint32_t sc[256];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 256 + tid;
    unsigned cnt;
    const unsigned bits = dc_lane_flags(a, t, &cnt);
    sc[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan
        const uint32_t x = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += x;
        __syncthreads();
    }
    uint32_t run = a.blk[blockIdx.x] + sc[tid] - cnt;
#pragma unroll
    for (int k = 0; k < DC_ROWS; k++) {
        const int64_t id = t * DC_ROWS + k;
        a.dense[id] = (int32_t)run;                    // (padded to whole tiles like `used`)
        if ((bits >> k) & 1) a.used_ids[run++] = (int32_t)id;   // (a set byte lies below n_ids: run < n_used <= n_ids)
    }
}

template <typename T, bool LDS>
__global__ __launch_bounds__(256) void dc_gather_kernel(DcArgs a) {
    __shared__ unsigned s_null;
    __shared__ int32_t s_dense[LDS ? DC_LDS_IDS : 1];
    if (threadIdx.x == 0) s_null = 0;
    if constexpr (LDS)
        for (int64_t i = threadIdx.x; i < a.n_ids; i += 256) s_dense[i] = a.dense[i];
    __syncthreads();
    unsigned nnull = 0;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t row0 = (tile * 256 + threadIdx.x) * DC_ROWS;
        if (row0 >= a.n) break;
        const int cnt = a.n - row0 < DC_ROWS ? (int)(a.n - row0) : DC_ROWS;
        int32_t c[DC_ROWS];
        if (!a.rows && a.vec_in && cnt == DC_ROWS) {
            const int4 q0 = ((const int4*)(a.codes + row0))[0], q1 = ((const int4*)(a.codes + row0))[1];
            c[0] = q0.x; c[1] = q0.y; c[2] = q0.z; c[3] = q0.w; c[4] = q1.x; c[5] = q1.y; c[6] = q1.z; c[7] = q1.w;
        } else {
#pragma unroll
            for (int k = 0; k < DC_ROWS; k++) c[k] = k < cnt ? a.codes[a.rows ? a.rows[row0 + k] : row0 + k] : -1;
        }
        T v[DC_ROWS];
        unsigned obits = 0;
#pragma unroll
        for (int k = 0; k < DC_ROWS; k++) {
            int32_t dense = 0;
            if (c[k] >= 0) {
                obits |= 1u << k;
                if ((int64_t)c[k] < a.n_ids) dense = LDS ? s_dense[c[k]] : a.dense[c[k]];      // (the bounds test precedes the load)
            }
            v[k] = (T)dense;
        }
        nnull += (unsigned)(cnt - __popc(obits));
        T* o = (T*)a.out + row0;
        if (a.vec_out && cnt == DC_ROWS) {
            if constexpr (sizeof(T) == 1) {
                uint2 q;
                __builtin_memcpy(&q, v, sizeof(v));
                *(uint2*)o = q;
            } else {
                uint4 q[sizeof(T) / 2];
                __builtin_memcpy(q, v, sizeof(v));
#pragma unroll
                for (int j = 0; j < (int)(sizeof(T) / 2); j++) ((uint4*)o)[j] = q[j];
            }
        } else {
#pragma unroll
            for (int k = 0; k < DC_ROWS; k++)
                if (k < cnt) o[k] = v[k];
        }
        if (a.out_valid) a.out_valid[row0 >> 3] = (uint8_t)obits;   // (bits past n stay 0: rows past n read as -1)
    }
    if (nnull) atomicAdd(&s_null, nnull);
    __syncthreads();
    if (threadIdx.x == 0 && s_null) atomicAdd(a.counters + 1, (unsigned long long)s_null);
}

}  // namespace

extern "C" {

int vnm_dict_take_compact(const int32_t* codes, const int64_t* rows, int64_t n, int64_t n_ids, int index_type, void* out_indices,
                          uint8_t* out_validity, int64_t* out_null_count, int32_t* out_used_ids, int64_t* out_n_used, void* stream) {
    VNM_TRY(ensure_init());
    if (out_n_used) *out_n_used = 0;
    if (out_null_count) *out_null_count = 0;
    if (!codes || !out_indices || !out_used_ids || !out_n_used) return set_error("vnm_dict_take_compact: null argument");
    if (n < 0 || n_ids < 0) return set_error("vnm_dict_take_compact: negative n or n_ids");
    if (n_ids > 0x7FFFFFFFLL) return set_error("vnm_dict_take_compact: more ids than an int32 code can name");
    if (index_type < VNM_I8 || index_type > VNM_U64) return set_error("vnm_dict_take_compact: the indices must be of an integer type");
    if (n == 0) return 0;
    static const int width[8] = {1, 2, 4, 8, 1, 2, 4, 8};   // VNM_I8 ... VNM_U64
    static const uint64_t top[8] = {0x7F, 0x7FFF, 0x7FFFFFFF, 0x7FFFFFFFFFFFFFFFULL, 0xFF, 0xFFFF, 0xFFFFFFFFu, ~0ULL};
    const int w = width[index_type];
    hipStream_t s = as_stream(stream);
    PoolScope pool;
    DcArgs a{};
    a.codes = codes; a.rows = rows; a.n = n; a.n_ids = n_ids;
    a.out = out_indices; a.out_valid = out_validity; a.used_ids = out_used_ids;
    a.vec_in = ((uintptr_t)codes & 15) == 0;
    a.vec_out = ((uintptr_t)out_indices & (w == 1 ? 7 : 15)) == 0;
    const int64_t tiles = (n + DC_TILE - 1) / DC_TILE;
    if (tiles > 0x7FFFFFFFLL) return set_error("vnm_dict_take_compact: too many rows for one launch");
    a.ntiles = tiles;
    a.nblocks = (int)std::max<int64_t>((n_ids + DC_TILE - 1) / DC_TILE, 1);
    const size_t padded = (size_t)a.nblocks * DC_TILE;
    a.used = (uint8_t*)pool.take(padded);
    a.dense = (int32_t*)pool.take(padded * 4);
    a.blk = (uint32_t*)pool.take(((size_t)a.nblocks + 1) * 4);
    a.counters = (unsigned long long*)pool.take(16);
    if (!a.used || !a.dense || !a.blk || !a.counters) return 1;
    VNM_HIP(hipMemsetAsync(a.used, 0, padded, s));
    VNM_HIP(hipMemsetAsync(a.counters, 0, 16, s));
    const int64_t cus = device_info().num_cus;
    {
        KernelTimer timer("dict_compact_mark_scan", s);
        dc_mark_kernel<<<dim3((unsigned)std::min<int64_t>((n + 255) / 256, cus * 16)), 256, 0, s>>>(a);
        dc_count_kernel<<<dim3((unsigned)a.nblocks), 256, 0, s>>>(a);
        dc_scan_kernel<<<1, 1024, 0, s>>>(a.blk, a.nblocks);
        dc_emit_kernel<<<dim3((unsigned)a.nblocks), 256, 0, s>>>(a);
    }
    VNM_HIP(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    uint32_t n_used = 0;
    VNM_HIP(hipMemcpyAsync(&n_used, a.blk + a.nblocks, 4, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipMemcpyAsync(counts, a.counters, 8, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (counts[0]) return set_error("vnm_dict_take_compact: code out of bounds (%llu row(s) of %lld, %lld id(s))", counts[0], (long long)n, (long long)n_ids);
    *out_n_used = (int64_t)n_used;
    if ((uint64_t)n_used > top[index_type])
        return set_error("These dictionaries cannot be combined.  The unified dictionary requires a larger index type.");
    // the global form: one tile per workgroup, dense_of_code through L2.  The LDS form: a persistent grid, every workgroup copies the
    // table once and takes several tiles -- taken when a workgroup's rows are at least 4x the ids it copies
    const char* sw = getenv("VNM_DICT_COMPACT_LDS");
    const int64_t lds_grid = std::min<int64_t>(tiles, cus * 8);
    const int64_t rows_per_wg = (tiles + lds_grid - 1) / lds_grid * DC_TILE;
    const bool lds = n_ids > 0 && n_ids <= DC_LDS_IDS && (sw ? sw[0] == '1' : rows_per_wg >= 4 * n_ids);
    const dim3 grid((unsigned)(lds ? lds_grid : tiles));
#define VNM_DC_LAUNCH(T)                                           \
    do {                                                           \
        if (lds) dc_gather_kernel<T, true><<<grid, 256, 0, s>>>(a); \
        else dc_gather_kernel<T, false><<<grid, 256, 0, s>>>(a);    \
    } while (0)
    {
        KernelTimer timer("dict_compact_gather", s);
        switch (w) {       // (a dense index is below 2^31: the signed and the unsigned type of a width hold the same bytes)
            case 1: VNM_DC_LAUNCH(uint8_t); break;
            case 2: VNM_DC_LAUNCH(uint16_t); break;
            case 4: VNM_DC_LAUNCH(uint32_t); break;
            default: VNM_DC_LAUNCH(uint64_t); break;
        }
    }
#undef VNM_DC_LAUNCH
    VNM_HIP(hipGetLastError());
    VNM_HIP(hipMemcpyAsync(counts, a.counters, 16, hipMemcpyDeviceToHost, s));
    VNM_HIP(hipStreamSynchronize(s));
    if (out_null_count) *out_null_count = (int64_t)counts[1];
    return 0;
}

}  // extern "C"
