// Arrow-level operator handles: the entry points a binding of the reference's native boundary calls
// (vinum/core/vinum_lib.cpp:54-142: next(batch) per RecordBatch, one result()/sorted()).
// Batches cross as Arrow C Data Interface structs (no libarrow dependency); columns are staged into HBM,
// the device-level operators run there, and results come back as freshly allocated Arrow arrays.
// This file: what the aggregate operator (vnm_agg_op.cpp) and the sort operator (vnm_sort_op.cpp) share and what needs the device.
#include "vnm_arrow.hpp"

#include <algorithm>

namespace vnm {

std::vector<ColChunk> chunks_of(const std::vector<const struct ArrowArray*>& batches, int ci) {
    std::vector<ColChunk> v;
    for (const struct ArrowArray* b : batches) v.push_back(ColChunk{b->children[ci], b->children[ci]->offset + b->offset, b->length});
    return v;
}

std::vector<uint8_t> chunks_validity(const std::vector<ColChunk>& chunks, int64_t total) {
    std::vector<BitRun> runs;
    for (auto& c : chunks) runs.push_back(BitRun{chunk_validity(c), c.off, c.len});
    return join_validity(runs, total);
}

int upload_validity(const std::vector<ColChunk>& chunks, int64_t total, uint8_t** out) {
    *out = nullptr;
    const std::vector<uint8_t> bits = chunks_validity(chunks, total);
    if (bits.empty()) return 0;
    uint8_t* db = (uint8_t*)pool_alloc(bits.size());
    if (!db) return 1;
    if (hipMemcpy(db, bits.data(), (size_t)(total + 7) / 8, hipMemcpyHostToDevice) != hipSuccess) { pool_free(db); return set_error("staging the validity bits failed"); }
    *out = db;
    return 0;
}

int stage_child(const ColChunk& c, const ColType& t, vnm_dcol* out, hipStream_t s) {
    const uint8_t* validity = (c.col->n_buffers > 0 && c.col->null_count != 0) ? (const uint8_t*)c.col->buffers[0] : nullptr;
    const void* values = c.col->n_buffers > 1 ? c.col->buffers[1] : nullptr;
    VNM_TRY(vnm_stage_column(values, validity, c.off, c.len, t.type, out, (void*)s));
    out->flags = t.flags;
    return 0;
}

// Table::FromRecordBatches, as Sort does (sort.cpp:16): the chunks' values go through the pinned ring as they are -- no joined copy
// on the host -- and the validity bits, where a chunk has NULLs, are laid end to end by byte-wise shifts and staged as one small buffer.
int stage_children(const std::vector<ColChunk>& chunks, const ColType& t, int64_t total, vnm_dcol* out) {
    const int w = type_width(t.type);
    std::vector<const void*> srcs;
    std::vector<size_t> sizes;
    for (auto& c : chunks) {
        if (!c.len) continue;
        srcs.push_back((const uint8_t*)c.col->buffers[1] + (size_t)c.off * w);
        sizes.push_back((size_t)c.len * w);
    }
    memset(out, 0, sizeof(*out));
    void* dv = pool_alloc((size_t)(total ? total : 1) * w);
    if (!dv) return 1;
    out->values = dv; out->type = t.type; out->length = total; out->flags = t.flags;
    int rc = stage_chunks(dv, srcs.data(), sizes.data(), srcs.size(), nullptr);
    uint8_t* db = nullptr;
    if (!rc) rc = upload_validity(chunks, total, &db);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = set_error("staging failed");
    if (rc) { pool_free(db); pool_free(dv); out->values = nullptr; } else out->validity = db;
    return rc;
}

int make_primitive_from_device(struct ArrowArray* a, int64_t n, int width, const void* dev_values, const uint8_t* dev_bitmap, int64_t null_count) {
    make_array(a, n, 2);
    a->null_count = null_count;
    void* data = malloc((size_t)(n ? n : 1) * width);
    a->buffers[1] = data;
    if (n && hipMemcpy(data, dev_values, (size_t)n * width, hipMemcpyDeviceToHost) != hipSuccess) return set_error("result: device to host copy failed");
    if (null_count) {
        uint8_t* bm = (uint8_t*)calloc((size_t)((n + 63) / 64) * 8, 1);
        a->buffers[0] = bm;
        if (hipMemcpy(bm, dev_bitmap, (size_t)((n + 7) / 8), hipMemcpyDeviceToHost) != hipSuccess) return set_error("result: device to host copy failed");
    }
    return 0;
}

int make_string_array(const DictValues& values, struct ArrowArray* a, bool wide, const int32_t* want, const uint8_t* valid_bytes, int64_t n, const char* what) {
    const std::string msg = values.make_string_array(a, wide, want, valid_bytes, n, what);
    return msg.empty() ? 0 : set_error("%s", msg.c_str());
}

// ---- dictionary-typed columns -------------------------------------------------------------------------------------------------------
int append_new_values(vnm_strdict* dict, DictValues* values, int64_t n_new, int64_t new_bytes) {
    return values->append_new(n_new, new_bytes, [&](int32_t* ids, int32_t* lens, uint8_t* bytes) { return vnm_strdict_fetch_new(dict, ids, lens, bytes); });
}

// bit i = codes[i] >= 0; one lane per byte of the bitmap (the bits past n in the last byte 0)
__global__ void codes_valid_bits_kernel(const int32_t* codes, int64_t n, uint8_t* bits) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b * 8 >= n) return;
    unsigned v = 0;
    for (int k = 0; k < 8; k++)
        if (b * 8 + k < n && codes[b * 8 + k] >= 0) v |= 1u << k;
    bits[b] = (uint8_t)v;
}

// A row is NULL by index or by value.  Per chunk the D VALUES of its dictionary are encoded from their host buffers (own offset,
// length, validity; a NULL value: table entry -1) unless the chunk repeats the previous chunk's dictionary buffers -- judged inside
// one call only, while every chunk is alive --, the code_of_index table is uploaded, and the native-width indices, joined through
// the pinned ring, are remapped on the device into the joined codes at the chunk's row offset.  No per-row host loop, no string
// bytes per row over PCIe.
int stage_dict_codes(vnm_strdict* dict, DictValues* values, const ColDesc& d, const std::vector<ColChunk>& chunks, int64_t total,
                     const char* malformed, int32_t** codes_out, uint8_t** validity_out, DictReadStats* stats) {
    const int w = type_width(d.t.type);
    const size_t t1 = (size_t)(total ? total : 1);
    PoolScope pool;
    void* didx = pool.take(t1 * w);
    int32_t* codes = (int32_t*)pool.take(t1 * 4);
    uint8_t* vbits = (uint8_t*)pool.take((size_t)(total + 7) / 8 + 8);
    if (!didx || !codes || !vbits) return 1;
    std::vector<const void*> srcs;
    std::vector<size_t> sizes;
    for (auto& c : chunks) {
        if (!c.len) continue;
        if (!c.col->dictionary || c.col->dictionary->n_buffers < 3 || c.col->n_buffers < 2 || !c.col->buffers[1]) return set_error("%s", malformed);
        srcs.push_back((const uint8_t*)c.col->buffers[1] + (size_t)c.off * w);
        sizes.push_back((size_t)c.len * w);
    }
    if (!srcs.empty()) VNM_TRY(stage_chunks(didx, srcs.data(), sizes.data(), srcs.size(), nullptr));
    uint8_t* dbits = nullptr;
    VNM_TRY(upload_validity(chunks, total, &dbits));
    PoolSlotGuard<uint8_t> dbits_guard(&dbits);
    VNM_HIP(hipStreamSynchronize(nullptr));
    int32_t* table = nullptr;
    int64_t table_cap = 0, row = 0;
    const struct ArrowArray* prev = nullptr;
    for (auto& c : chunks) {
        if (!c.len) continue;
        const struct ArrowArray* dv = c.col->dictionary;
        const int64_t D = dv->length;
        const bool same = prev && prev->buffers[0] == dv->buffers[0] && prev->buffers[1] == dv->buffers[1] && prev->buffers[2] == dv->buffers[2] &&
                          prev->offset == dv->offset && prev->length == dv->length;
        if (same) stats->dictionaries_skipped++;
        else {
            std::vector<int32_t> code_of((size_t)(D ? D : 1), -1);
            if (D > 0) {
                int64_t n_new = 0, new_bytes = 0;
                const uint8_t* valid = dv->null_count != 0 ? (const uint8_t*)dv->buffers[0] : nullptr;
                VNM_TRY(vnm_strdict_encode(dict, dv->buffers[1], d.wide ? 1 : 0, (const uint8_t*)dv->buffers[2], valid, dv->offset, D,
                                           code_of.data(), &n_new, &new_bytes, nullptr));
                VNM_TRY(append_new_values(dict, values, n_new, new_bytes));
            }
            if (D > table_cap) {
                pool.done(table);
                table_cap = std::max<int64_t>(D, 2 * table_cap);
                table = (int32_t*)pool.take((size_t)table_cap * 4);
                if (!table) return 1;
            }
            if (D > 0) VNM_HIP(hipMemcpy(table, code_of.data(), (size_t)D * 4, hipMemcpyHostToDevice));
            stats->values_encoded += D;
            prev = dv;
        }
        vnm_dcol view{};
        view.values = didx; view.validity = dbits; view.offset = row; view.length = c.len; view.type = d.t.type;
        int64_t bad = 0;
        VNM_TRY(vnm_strdict_remap_indices(&view, table, D, codes + row, nullptr, &bad, nullptr));
        row += c.len;
    }
    if (total > 0) {
        const int64_t nb = (total + 7) / 8;
        codes_valid_bits_kernel<<<dim3((unsigned)((nb + 255) / 256)), 256, 0, nullptr>>>(codes, total, vbits);
        VNM_HIP(hipGetLastError());
    }
    VNM_HIP(hipStreamSynchronize(nullptr));
    *codes_out = codes; *validity_out = vbits;
    pool.keep(codes); pool.keep(vbits);
    return 0;
}

int make_dict_array(const int32_t* codes, const int64_t* rows, int64_t n, const ColDesc& d, vnm_strdict* dict, const DictValues& values, struct ArrowArray* out) {
    const size_t n1 = (size_t)(n ? n : 1);
    const int w = type_width(d.t.type);
    const int64_t n_ids = vnm_strdict_ids(dict);
    PoolScope pool;
    void* dind = pool.take(n1 * w);
    uint8_t* dvalid = (uint8_t*)pool.take((size_t)(n + 7) / 8 + 8);
    int32_t* dused = (int32_t*)pool.take((size_t)std::max<int64_t>(std::min(n, n_ids), 1) * 4);
    if (!dind || !dvalid || !dused) return 1;
    int64_t nulls = 0, n_used = 0;
    VNM_TRY(vnm_dict_take_compact(codes, rows, n, n_ids, d.t.type, dind, dvalid, &nulls, dused, &n_used, nullptr));
    std::vector<int32_t> used((size_t)(n_used ? n_used : 1));
    if (n_used) VNM_HIP(hipMemcpy(used.data(), dused, (size_t)n_used * 4, hipMemcpyDeviceToHost));
    VNM_TRY(make_primitive_from_device(out, n, w, dind, dvalid, nulls));
    out->dictionary = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
    return make_string_array(values, out->dictionary, d.wide, used.data(), nullptr, n_used, "a result dictionary");
}

}  // namespace vnm
