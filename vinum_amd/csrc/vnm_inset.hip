// IN / NOT IN against a long list: the list as a device-resident set, probed by a kernel of its own that writes a byte mask
// (np.isin(x, values[, invert]), vinum/core/expressions.py:39-40).  DESIGN.md section 4.9b.
//
// The set lives in one of three compare domains -- exactly what the projection interpreter's OR chain of `==` computes for
// the same column and list (vnm_project.hip, VNM_EX_EQ typing): exact int64, exact uint64, or float64 with NULL -> NaN.  A
// domain's canonical table (sorted, distinct) is prepared the first time a probe needs it.  Two representations:
//   bitmap  (integer domains, range <= 64 * n bits): one bit test at (uint64)(v - lo);
//   sorted  (everything else): a branch-free lower bound, ceil(log2 n) steps for every lane.
// Either is copied into LDS when it is at most 32 KB, read from global memory otherwise.
#include <algorithm>
#include <cmath>

#include "vnm_common.hpp"

using namespace vnm;

namespace {

constexpr int IS_BLOCK = 256;                        // 4 waves
constexpr int IS_RUN = 4;                            // adjacent rows per lane and run: their mask bytes leave as one 4-byte store
constexpr int IS_RUNS = 8;                           // runs per lane and tile
constexpr int IS_STRIDE = IS_BLOCK * IS_RUN;         // rows of one run over the workgroup
constexpr int IS_TILE = IS_STRIDE * IS_RUNS;         // 8192 rows per workgroup
constexpr int64_t IS_LDS_WORDS = 4096;               // 8-byte words of LDS per workgroup: 32 KB, four workgroups in a CU's 160 KB
constexpr uint64_t IS_LDS_BITS = IS_LDS_WORDS * 64;  // bitmap bits that fit

struct ProbeArgs {
    vnm_dcol col;
    int64_t length;
    const uint64_t* table;   // sorted members (bit patterns of the domain's type) or the bitmap's 64-bit words; >= 1 word
    int64_t n;               // sorted: members; bitmap: 64-bit words
    uint64_t lo;             // bitmap: the smallest member
    uint64_t range_m1;       // bitmap: largest - smallest member
    uint8_t* out;
    int invert;
    int vec;                 // 8-byte column, no validity, 16-byte aligned first row: full tiles come in as 16-byte loads
};

template <int DOM> struct DomType;
template <> struct DomType<VNM_IN_DOM_I64> { using T = int64_t; };
template <> struct DomType<VNM_IN_DOM_U64> { using T = uint64_t; };
template <> struct DomType<VNM_IN_DOM_F64> { using T = double; };

template <class T> __device__ __forceinline__ T from_bits(uint64_t b) {
    T v;
    memcpy(&v, &b, 8);
    return v;
}

// row i of the column as a value of the domain (NULL -> NaN in the float64 domain: record_batch.py:112-118)
template <int DOM> __device__ __forceinline__ typename DomType<DOM>::T row_value(const vnm_dcol& c, int64_t i) {
    if constexpr (DOM == VNM_IN_DOM_F64) return col_valid(c, i) ? col_f64(c, i) : __builtin_nan("");
    else return (typename DomType<DOM>::T)col_i64(c, i);
}

// the 8 raw bytes of an 8-byte column without validity as a value of the domain
template <int DOM> __device__ __forceinline__ typename DomType<DOM>::T raw_value(uint64_t bits, int type) {
    if constexpr (DOM == VNM_IN_DOM_F64) {
        if (type == VNM_F64) return from_bits<double>(bits);
        if (type == VNM_U64) return (double)bits;
        return (double)(int64_t)bits;
    } else return (typename DomType<DOM>::T)bits;
}

template <int DOM, bool BITMAP>
__device__ __forceinline__ uint32_t is_member(typename DomType<DOM>::T v, const uint64_t* tab, int64_t n, uint64_t lo, uint64_t range_m1) {
    using T = typename DomType<DOM>::T;
    if constexpr (BITMAP) {
        // the range check is the unsigned subtraction itself: INT64_MIN / INT64_MAX members cannot overflow it
        const uint64_t d = (uint64_t)v - lo;
        const uint64_t w = tab[d <= range_m1 ? (d >> 6) : 0];
        return (d <= range_m1) & (uint32_t)((w >> (d & 63)) & 1);
    } else {
        // branch-free lower bound: `len` is uniform, every lane takes the same ceil(log2 n) steps.  Doubles compare with < and
        // ==, never on bits: -0.0 finds 0.0, NaN finds nothing
        uint32_t base = 0, len = (uint32_t)n;
        while (len > 1) {
            const uint32_t half = len >> 1;
            base += from_bits<T>(tab[base + half - 1]) < v ? half : 0;
            len -= half;
        }
        return (n > 0) & (from_bits<T>(tab[base]) == v);
    }
}

template <int DOM, bool BITMAP, bool LDS>
__global__ __launch_bounds__(IS_BLOCK) void in_set_kernel(ProbeArgs a) {
    using T = typename DomType<DOM>::T;
    __shared__ uint64_t s_tab[LDS ? IS_LDS_WORDS : 1];
    if constexpr (LDS) {
        const int words = (int)(a.n > 0 ? a.n : 1);
        for (int k = threadIdx.x; k < words; k += IS_BLOCK) s_tab[k] = a.table[k];
        __syncthreads();
    }
    const uint64_t* tab = LDS ? s_tab : a.table;
    const uint32_t flip = a.invert ? 0x01010101u : 0u;
    const int64_t tile0 = (int64_t)blockIdx.x * IS_TILE;
    if (a.vec && tile0 + IS_TILE <= a.length) {
        const uint64_t* vals = (const uint64_t*)a.col.values + a.col.offset;
#pragma unroll
        for (int g = 0; g < IS_RUNS; g += 4) {
            ulonglong2 x[4][2];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const ulonglong2* p = (const ulonglong2*)(vals + tile0 + (int64_t)(g + j) * IS_STRIDE + (int64_t)threadIdx.x * IS_RUN);
                x[j][0] = p[0];
                x[j][1] = p[1];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t m = is_member<DOM, BITMAP>(raw_value<DOM>(x[j][0].x, a.col.type), tab, a.n, a.lo, a.range_m1)
                                 | is_member<DOM, BITMAP>(raw_value<DOM>(x[j][0].y, a.col.type), tab, a.n, a.lo, a.range_m1) << 8
                                 | is_member<DOM, BITMAP>(raw_value<DOM>(x[j][1].x, a.col.type), tab, a.n, a.lo, a.range_m1) << 16
                                 | is_member<DOM, BITMAP>(raw_value<DOM>(x[j][1].y, a.col.type), tab, a.n, a.lo, a.range_m1) << 24;
                *(uint32_t*)(a.out + tile0 + (int64_t)(g + j) * IS_STRIDE + (int64_t)threadIdx.x * IS_RUN) = m ^ flip;
            }
        }
        return;
    }
    // the ragged last tile, odd offsets, 1/2/4-byte columns, columns with validity: row by row
    for (int j = 0; j < IS_RUNS; j++) {
        const int64_t r = tile0 + (int64_t)j * IS_STRIDE + (int64_t)threadIdx.x * IS_RUN;
        if (r + IS_RUN <= a.length) {
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < IS_RUN; k++)
                m |= is_member<DOM, BITMAP>(row_value<DOM>(a.col, r + k), tab, a.n, a.lo, a.range_m1) << (8 * k);
            *(uint32_t*)(a.out + r) = m ^ flip;
        } else {
            for (int64_t i = r; i < a.length; i++)
                a.out[i] = (uint8_t)(is_member<DOM, BITMAP>(row_value<DOM>(a.col, i), tab, a.n, a.lo, a.range_m1) ^ (flip & 1));
        }
    }
}

// ---- host: domains, canonical tables, routes -------------------------------------------------------------------------
int domain_of(int col_type, bool has_validity, bool list_is_float) {
    if (list_is_float || has_validity || type_is_float(col_type)) return VNM_IN_DOM_F64;
    return col_type == VNM_U64 ? VNM_IN_DOM_U64 : VNM_IN_DOM_I64;
}

struct Plan {
    int domain = 0, route = 0;
    std::vector<uint64_t> table;   // sorted, distinct: the members' bit patterns in the domain's type
    uint64_t lo = 0, range_m1 = 0; // smallest member, largest - smallest (integer domains with members)
};

const char* const ROUTE_NAME[4] = {"in_set:bitmap_lds", "in_set:bitmap_global", "in_set:sorted_lds", "in_set:sorted_global"};
const char* const DOMAIN_NAME[3] = {"i64", "u64", "f64"};

void make_plan(bool list_is_float, const void* values, int64_t n, int domain, Plan& p) {
    p.domain = domain;
    const int64_t* iv = (const int64_t*)values;
    const double* dv = (const double*)values;
    if (domain == VNM_IN_DOM_F64) {
        std::vector<double> t;
        t.reserve(n);
        for (int64_t k = 0; k < n; k++) {
            double d = list_is_float ? dv[k] : (double)iv[k];
            if (std::isnan(d)) continue;   // NaN == anything is False: the member matches nothing
            if (d == 0.0) d = 0.0;         // -0.0 == 0.0: one member
            t.push_back(d);
        }
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        p.table.resize(t.size());
        if (!t.empty()) memcpy(p.table.data(), t.data(), t.size() * 8);
    } else if (domain == VNM_IN_DOM_U64) {
        for (int64_t k = 0; k < n; k++)
            if (iv[k] >= 0) p.table.push_back((uint64_t)iv[k]);   // a negative member equals no uint64
        std::sort(p.table.begin(), p.table.end());
        p.table.erase(std::unique(p.table.begin(), p.table.end()), p.table.end());
    } else {
        std::vector<int64_t> t(iv, iv + n);
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        p.table.resize(t.size());
        memcpy(p.table.data(), t.data(), t.size() * 8);
    }
    const uint64_t m = p.table.size();
    bool bitmap = false;
    if (domain != VNM_IN_DOM_F64 && m > 0) {
        p.lo = p.table.front();
        p.range_m1 = p.table.back() - p.table.front();   // unsigned: exact for INT64_MIN .. INT64_MAX too
        // the bitmap is no larger than the sorted table it replaces: range = range_m1 + 1 <= 64 * m
        bitmap = p.range_m1 < 64 * m;
    }
    if (bitmap) p.route = p.range_m1 < IS_LDS_BITS ? VNM_IN_ROUTE_BITMAP_LDS : VNM_IN_ROUTE_BITMAP_GLOBAL;
    else p.route = (int64_t)m <= IS_LDS_WORDS ? VNM_IN_ROUTE_SORTED_LDS : VNM_IN_ROUTE_SORTED_GLOBAL;
}

bool is_bitmap(int route) { return route == VNM_IN_ROUTE_BITMAP_LDS || route == VNM_IN_ROUTE_BITMAP_GLOBAL; }

struct Prepared {
    bool ready = false;
    int route = 0;
    int64_t members = 0;   // of the canonical table
    int64_t n = 0;         // what the kernel gets: members (sorted) or 64-bit words (bitmap)
    uint64_t lo = 0, range_m1 = 0;
    uint64_t* dev = nullptr;
};

}  // namespace

struct vnm_in_set {
    bool is_float = false;
    std::vector<uint64_t> values;   // the list as it came (int64 or float64 bit patterns)
    Prepared dom[3];
    hipStream_t last_stream = nullptr;
    std::mutex mu;
};

namespace {

int prepare(vnm_in_set* h, int domain) {
    Prepared& pr = h->dom[domain];
    if (pr.ready) return 0;
    Plan p;
    make_plan(h->is_float, h->values.data(), (int64_t)h->values.size(), domain, p);
    std::vector<uint64_t> bits;
    const std::vector<uint64_t>* up = &p.table;
    if (is_bitmap(p.route)) {
        bits.assign((size_t)(p.range_m1 >> 6) + 1, 0);
        for (uint64_t v : p.table) {
            const uint64_t d = v - p.lo;
            bits[d >> 6] |= 1ull << (d & 63);
        }
        up = &bits;
    }
    const size_t words = std::max<size_t>(up->size(), 1);
    uint64_t* dev = (uint64_t*)pool_alloc(words * 8);
    if (!dev) return 1;
    const uint64_t zero = 0;
    // a blocking copy: the host vector is gone when this returns, and every later launch is ordered after it
    hipError_t e = hipMemcpy(dev, up->empty() ? &zero : up->data(), words * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        pool_free(dev);
        return set_error("vnm_in_set: uploading the set failed: %s", hipGetErrorString(e));
    }
    pr.route = p.route;
    pr.members = (int64_t)p.table.size();
    pr.n = is_bitmap(p.route) ? (int64_t)bits.size() : pr.members;
    pr.lo = p.lo;
    pr.range_m1 = p.range_m1;
    pr.dev = dev;
    pr.ready = true;
    return 0;
}

template <int DOM, bool BITMAP>
void launch(int route, int grid, hipStream_t s, const ProbeArgs& a) {
    if (route == VNM_IN_ROUTE_BITMAP_LDS || route == VNM_IN_ROUTE_SORTED_LDS) in_set_kernel<DOM, BITMAP, true><<<grid, IS_BLOCK, 0, s>>>(a);
    else in_set_kernel<DOM, BITMAP, false><<<grid, IS_BLOCK, 0, s>>>(a);
}

}  // namespace

extern "C" {

int vnm_in_set_create(int list_is_float, const void* values_host, int64_t n, vnm_in_set** out) {
    if (!out) return set_error("vnm_in_set_create: null argument");
    *out = nullptr;
    if (n <= 0) return set_error("ValueError: IN with an empty list");
    if (!values_host) return set_error("vnm_in_set_create: null argument");
    vnm_in_set* h = new vnm_in_set();
    h->is_float = list_is_float != 0;
    h->values.assign((const uint64_t*)values_host, (const uint64_t*)values_host + n);
    *out = h;
    return 0;
}

void vnm_in_set_destroy(vnm_in_set* h) {
    if (!h) return;
    for (Prepared& p : h->dom)
        if (p.dev) pool_free_after(p.dev, h->last_stream);   // a probe may still be running
    delete h;
}

int vnm_in_set_probe(vnm_in_set* h, const vnm_dcol* col, int64_t length, int invert, uint8_t* out_mask, void* stream) {
    if (!h || !col) return set_error("vnm_in_set_probe: null argument");
    if (col->type < VNM_I8 || col->type > VNM_F64) return set_error("vnm_in_set_probe: unsupported column type %d", col->type);
    if (length < 0 || col->offset < 0 || col->length < length) return set_error("vnm_in_set_probe: %lld rows asked of a column of %lld",
                                                                                (long long)length, (long long)col->length);
    if (length == 0) return 0;
    if (!out_mask || !col->values) return set_error("vnm_in_set_probe: null argument");
    VNM_TRY(ensure_init());
    const int domain = domain_of(col->type, col->validity != nullptr, h->is_float);
    std::lock_guard<std::mutex> lock(h->mu);
    VNM_TRY(prepare(h, domain));
    const Prepared& pr = h->dom[domain];
    hipStream_t s = as_stream(stream);
    h->last_stream = s;
    ProbeArgs a{};
    a.col = *col;
    a.length = length;
    a.table = pr.dev;
    a.n = pr.n;
    a.lo = pr.lo;
    a.range_m1 = pr.range_m1;
    a.out = out_mask;
    a.invert = invert != 0;
    if (((uintptr_t)out_mask & 3) != 0) return set_error("vnm_in_set_probe: the mask must be 4-byte aligned");
    // (an even Arrow offset over a 16-byte aligned buffer)
    a.vec = type_width(col->type) == 8 && !col->validity && ((uintptr_t)((const uint64_t*)col->values + col->offset) & 15) == 0;
    route_note(ROUTE_NAME[pr.route], "n=%lld range=%llu domain=%s rows=%lld", (long long)pr.members,
               (unsigned long long)(pr.members && domain != VNM_IN_DOM_F64 ? pr.range_m1 + 1 : 0), DOMAIN_NAME[domain], (long long)length);
    const int grid = (int)((length + IS_TILE - 1) / IS_TILE);
    KernelTimer timer("in_set_kernel", s);
    if (is_bitmap(pr.route)) launch<VNM_IN_DOM_I64, true>(pr.route, grid, s, a);   // (one unsigned subtraction serves both integer domains)
    else if (domain == VNM_IN_DOM_I64) launch<VNM_IN_DOM_I64, false>(pr.route, grid, s, a);
    else if (domain == VNM_IN_DOM_U64) launch<VNM_IN_DOM_U64, false>(pr.route, grid, s, a);
    else launch<VNM_IN_DOM_F64, false>(pr.route, grid, s, a);
    VNM_HIP(hipGetLastError());
    return 0;
}

int vnm_in_set_plan_host(int list_is_float, const void* values_host, int64_t n, int col_type, int col_has_validity, int* out_domain,
                         int* out_route, int64_t* out_members, uint64_t* out_table, uint64_t* out_range) {
    if (n <= 0) return set_error("ValueError: IN with an empty list");
    if (!values_host) return set_error("vnm_in_set_plan_host: null argument");
    if (col_type < VNM_I8 || col_type > VNM_F64) return set_error("vnm_in_set_plan_host: unsupported column type %d", col_type);
    Plan p;
    make_plan(list_is_float != 0, values_host, n, domain_of(col_type, col_has_validity != 0, list_is_float != 0), p);
    if (out_domain) *out_domain = p.domain;
    if (out_route) *out_route = p.route;
    if (out_members) *out_members = (int64_t)p.table.size();
    if (out_table && !p.table.empty()) memcpy(out_table, p.table.data(), p.table.size() * 8);
    // the members' range hi - lo + 1 (integer domains; 0 = no members, or all 2^64 values)
    if (out_range) *out_range = p.domain != VNM_IN_DOM_F64 && !p.table.empty() ? p.range_m1 + 1 : 0;
    return 0;
}

}  // extern "C"
