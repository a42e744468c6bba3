// The sort operator below the C ABI: vnm_sort_op_* (Sort, vinum_cpp/src/operators/sort/sort.cpp).
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "vnm_arrow.hpp"

using namespace vnm;

// one column of the whole table in HBM, by the kind of its ColDesc
struct DevSortCol {
    vnm_dcol num{};              // COL_NUM
    int64_t* offs = nullptr;     // COL_STR: total + 1 offsets (rebased to one data buffer)
    uint8_t* data = nullptr;
    uint8_t* bits = nullptr;     // COL_BOOL: the values, bit i = row i
    void* fixed = nullptr;       // COL_DEC: 16-byte values
    uint8_t* validity = nullptr; // bitmap, bit i = row i (null: no NULLs); COL_NUM keeps its own in `num`
    // COL_DICT: the rows' codes in one dictionary that grows with the batches (-1: NULL by index or by value; `validity` = codes >= 0)
    int32_t* codes = nullptr;
    vnm_strdict* dict = nullptr;
    DictValues values;
    DictReadStats read;          // for the route note
    void free_all() {
        vnm_free_column(&num);
        pool_free(offs); pool_free(data); pool_free(bits); pool_free(fixed); pool_free(validity); pool_free(codes);
        offs = nullptr; data = nullptr; bits = nullptr; fixed = nullptr; validity = nullptr; codes = nullptr;
        if (dict) vnm_strdict_destroy(dict);
        dict = nullptr;
    }
};

static int stage_sort_col(const std::vector<ColChunk>& chunks, const ColDesc& info, int64_t total, DevSortCol* d) {
    if (info.kind == COL_NUM) return stage_children(chunks, info.t, total, &d->num);
    if (info.kind == COL_DICT) {
        if (!(d->dict = vnm_strdict_create())) return 1;
        return stage_dict_codes(d->dict, &d->values, info, chunks, total, "Sort: a dictionary-typed column without its dictionary", &d->codes, &d->validity, &d->read);
    }
    VNM_TRY(upload_validity(chunks, total, &d->validity));
    if (info.kind == COL_STR) {
        std::vector<int64_t> offs((size_t)total + 1, 0);
        std::vector<const void*> srcs;
        std::vector<size_t> sizes;
        int64_t row = 0, base = 0;
        for (auto& c : chunks) {
            const struct ArrowArray* ch = c.col;
            const int64_t off = c.off, len = c.len;
            if (!len) continue;
            if (ch->n_buffers < 3 || !ch->buffers[1]) return set_error("Sort: a string / binary column without an offsets buffer");
            int64_t first, last;
            if (info.wide) {
                const int64_t* o = (const int64_t*)ch->buffers[1] + off;
                first = o[0]; last = o[len];
                for (int64_t i = 0; i <= len; i++) offs[(size_t)(row + i)] = base + (o[i] - first);
            } else {
                const int32_t* o = (const int32_t*)ch->buffers[1] + off;
                first = o[0]; last = o[len];
                for (int64_t i = 0; i <= len; i++) offs[(size_t)(row + i)] = base + ((int64_t)o[i] - first);
            }
            if (last > first) {
                if (!ch->buffers[2]) return set_error("Sort: a string / binary column without a data buffer");
                srcs.push_back((const uint8_t*)ch->buffers[2] + first);
                sizes.push_back((size_t)(last - first));
            }
            row += len; base += last - first;
        }
        d->offs = (int64_t*)pool_alloc(((size_t)total + 1) * 8);
        d->data = (uint8_t*)pool_alloc((size_t)(base > 0 ? base : 1));
        if (!d->offs || !d->data) return 1;
        if (hipMemcpy(d->offs, offs.data(), ((size_t)total + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) return set_error("Sort: staging offsets failed");
        if (!srcs.empty()) VNM_TRY(stage_chunks(d->data, srcs.data(), sizes.data(), srcs.size(), nullptr));
        if (hipStreamSynchronize(nullptr) != hipSuccess) return set_error("staging failed");
        return 0;
    }
    if (info.kind == COL_BOOL) {
        std::vector<uint8_t> bits((size_t)(total + 7) / 8 + 8, 0);
        int64_t pos = 0;
        for (auto& c : chunks) {
            const struct ArrowArray* ch = c.col;
            const int64_t off = c.off, len = c.len;
            if (len && ch->buffers[1]) copy_bits(bits.data(), pos, (const uint8_t*)ch->buffers[1], off, len);
            pos += len;
        }
        d->bits = (uint8_t*)pool_alloc(bits.size());
        if (!d->bits) return 1;
        if (hipMemcpy(d->bits, bits.data(), bits.size(), hipMemcpyHostToDevice) != hipSuccess) return set_error("Sort: staging a boolean column failed");
        return 0;
    }
    // COL_DEC: 16-byte values
    std::vector<const void*> srcs;
    std::vector<size_t> sizes;
    for (auto& c : chunks) {
        if (!c.len) continue;
        srcs.push_back((const uint8_t*)c.col->buffers[1] + (size_t)c.off * 16);
        sizes.push_back((size_t)c.len * 16);
    }
    d->fixed = pool_alloc((size_t)(total ? total : 1) * 16);
    if (!d->fixed) return 1;
    if (!srcs.empty()) VNM_TRY(stage_chunks(d->fixed, srcs.data(), sizes.data(), srcs.size(), nullptr));
    if (hipStreamSynchronize(nullptr) != hipSuccess) return set_error("staging failed");
    return 0;
}

// rows `idx` of a staged column -> a freshly allocated Arrow array (host buffers)
static int take_sort_col(const DevSortCol& d, const ColDesc& info, const int64_t* idx, int64_t n, struct ArrowArray* out) {
    const size_t n1 = (size_t)(n ? n : 1);
    if (info.kind == COL_NUM) {
        const int w = type_width(info.t.type);
        std::vector<uint8_t> hv(n1 * w), hb(n1);
        if (n > 0) {
            PoolScope pool;
            void* dv = pool.take((size_t)n * w);
            uint8_t* db = d.num.validity ? (uint8_t*)pool.take((size_t)n) : nullptr;
            if (!dv || (d.num.validity && !db)) return 1;
            VNM_TRY(vnm_take(&d.num, idx, n, dv, db, nullptr));
            VNM_HIP(hipMemcpy(hv.data(), dv, (size_t)n * w, hipMemcpyDeviceToHost));
            if (db) VNM_HIP(hipMemcpy(hb.data(), db, (size_t)n, hipMemcpyDeviceToHost));
        }
        make_primitive(out, n, w, hv.data(), d.num.validity ? hb.data() : nullptr);
        return 0;
    }
    if (info.kind == COL_DICT) return make_dict_array(d.codes, idx, n, info, d.dict, d.values, out);
    PoolScope pool;
    std::vector<uint8_t> hvalid;
    uint8_t* dvalid = nullptr;
    if (d.validity && n > 0) {
        dvalid = (uint8_t*)pool.take((size_t)n);
        if (!dvalid) return 1;
        hvalid.resize((size_t)n);
    }
    memset(out, 0, sizeof(*out));
    out->length = n;
    out->release = release_array;
    if (info.kind == COL_STR) {
        std::vector<int64_t> ho(n1 + 1, 0);
        std::vector<uint8_t> hd;
        if (n > 0) {
            int64_t* doffs = (int64_t*)pool.take(((size_t)n + 1) * 8);
            if (!doffs) return 1;
            uint8_t* ddata = nullptr;
            int64_t nbytes = 0;
            VNM_TRY(vnm_take_varwidth(d.offs, d.data, d.validity, idx, n, doffs, &ddata, &nbytes, dvalid, nullptr));
            PoolSlotGuard<uint8_t> g(&ddata);
            hd.resize((size_t)(nbytes > 0 ? nbytes : 1));
            VNM_HIP(hipMemcpy(ho.data(), doffs, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
            if (nbytes > 0) VNM_HIP(hipMemcpy(hd.data(), ddata, (size_t)nbytes, hipMemcpyDeviceToHost));
            if (dvalid) VNM_HIP(hipMemcpy(hvalid.data(), dvalid, (size_t)n, hipMemcpyDeviceToHost));
            if (!info.wide && nbytes > 0x7FFFFFFFLL) return set_error("Sort: the sorted %s column holds more than 2 GiB of bytes (use the large type)", info.t.format.c_str());
        }
        out->n_buffers = 3;
        out->buffers = (const void**)calloc(3, sizeof(void*));
        if (dvalid) { int64_t z = 0; out->buffers[0] = pack_bits(hvalid.data(), n, &z); out->null_count = z; }
        if (info.wide) {
            int64_t* o = (int64_t*)malloc((n1 + 1) * 8);
            memcpy(o, ho.data(), ((size_t)n + 1) * 8);
            out->buffers[1] = o;
        } else {
            int32_t* o = (int32_t*)malloc((n1 + 1) * 4);
            for (int64_t i = 0; i <= n; i++) o[i] = (int32_t)ho[(size_t)i];
            out->buffers[1] = o;
        }
        const size_t nb = hd.empty() ? 1 : hd.size();
        uint8_t* dd = (uint8_t*)malloc(nb);
        if (!hd.empty()) memcpy(dd, hd.data(), hd.size());
        out->buffers[2] = dd;
        return 0;
    }
    if (dvalid) {
        VNM_TRY(vnm_take_bits(d.validity, 0, idx, n, dvalid, nullptr));
        VNM_HIP(hipMemcpy(hvalid.data(), dvalid, (size_t)n, hipMemcpyDeviceToHost));
    }
    out->n_buffers = 2;
    out->buffers = (const void**)calloc(2, sizeof(void*));
    if (dvalid) { int64_t z = 0; out->buffers[0] = pack_bits(hvalid.data(), n, &z); out->null_count = z; }
    if (info.kind == COL_BOOL) {
        std::vector<uint8_t> hv(n1, 0);
        if (n > 0) {
            uint8_t* dv = (uint8_t*)pool.take((size_t)n);
            if (!dv) return 1;
            VNM_TRY(vnm_take_bits(d.bits, 0, idx, n, dv, nullptr));
            VNM_HIP(hipMemcpy(hv.data(), dv, (size_t)n, hipMemcpyDeviceToHost));
        }
        out->buffers[1] = pack_bits(hv.data(), n, nullptr);
        return 0;
    }
    // COL_DEC
    void* hv = malloc(n1 * 16);
    out->buffers[1] = hv;
    if (n > 0) {
        void* dv = pool.take((size_t)n * 16);
        if (!dv) return 1;
        VNM_TRY(vnm_take_fixed16(d.fixed, idx, n, dv, nullptr));
        VNM_HIP(hipMemcpy(hv, dv, (size_t)n * 16, hipMemcpyDeviceToHost));
    }
    return 0;
}

struct vnm_sort_op {
    std::vector<std::string> cols;
    std::vector<int> orders;
    std::vector<std::unique_ptr<ImportedBatch>> batches;
};

extern "C" {

vnm_sort_op* vnm_sort_op_create(int n, const char** cols, const int* orders) {
    if (ensure_init()) return nullptr;
    if (n < 1) { set_error("Sort needs at least one column"); return nullptr; }
    vnm_sort_op* h = new vnm_sort_op();
    for (int i = 0; i < n; i++) { h->cols.push_back(cols[i]); h->orders.push_back(orders[i] ? VNM_DESC : VNM_ASC); }
    return h;
}

void vnm_sort_op_destroy(vnm_sort_op* h) {
    if (!h) return;
    for (auto& b : h->batches) b->drop();
    delete h;
}

// Sort::Next (sort.cpp:11-13): only buffers the batch
int vnm_sort_op_next(vnm_sort_op* h, struct ArrowArray* batch, struct ArrowSchema* schema) {
    if (!h || !batch || !schema) return set_error("vnm_sort_op_next: null argument");
    auto ib = std::make_unique<ImportedBatch>();
    ib->arr = *batch; ib->sch = *schema; ib->live = true;
    batch->release = nullptr; schema->release = nullptr;
    h->batches.push_back(std::move(ib));
    return 0;
}

int vnm_sort_op_next_stream(vnm_sort_op* h, struct ArrowArrayStream* stream) {
    if (!h || !stream || !stream->get_next) return set_error("vnm_sort_op_next_stream: null argument");
    return drain_stream(stream, "vnm_sort_op_next_stream", [&](struct ArrowArray* a, struct ArrowSchema* sc) { return vnm_sort_op_next(h, a, sc); });
}

// Sort::Sorted (sort.cpp:15-63).  limit > 0: only the first `limit` rows are produced (LIMIT pushed into the
// sort; the reference sorts everything and slices later, same rows).
// Column types (round 5: every type the reference's own tests sort or carry along crosses the ABI and is handled on the device):
//   numeric / temporal     keys through the radix / sample sort, payload through vnm_take
//   utf8 / large_utf8 / binary / large_binary
//                          KEY: the values' order-preserving ranks (string dictionary on the device + a sort of the distinct
//                          values, vnm_strdict_ranks_device) as an int32 key column -- NULL stays NULL (last in both directions),
//                          equal values share a rank, so the stable sort keeps them in row order like SortIndices;
//                          PAYLOAD: gathered on the device (lengths -> prefix sums -> bytes, vnm_take_varwidth)
//   dictionary<intN, one of the four above>
//                          the batch dictionaries' VALUES through one device dictionary, the indices remapped to its codes on the
//                          device (stage_dict_codes); KEY: the codes' ranks, as above; leaves in its own type, the dictionary compacted
//                          to the values the produced rows use (vnm_dict_take_compact) -- DESIGN.md section 4.9e
//   decimal128             KEY: (high int64, low uint64) as two keys; PAYLOAD: 16-byte gather
//   boolean                PAYLOAD: bit gather; as a KEY it raises like the reference (vinum/core/algebra.py:191-201)
int vnm_sort_op_sorted(vnm_sort_op* h, int64_t limit, struct ArrowArray* out, struct ArrowSchema* out_schema) {
    if (!h || !out || !out_schema) return set_error("vnm_sort_op_sorted: null argument");
    if (h->batches.empty()) return set_error("Failed to create table from record batches.");
    const struct ArrowSchema* sch = &h->batches[0]->sch;
    const int64_t ncols = sch->n_children;
    int64_t total = 0;
    std::vector<ColDesc> info((size_t)ncols);
    for (int64_t c = 0; c < ncols; c++) info[c] = describe_column(sch->children[c], DECIMAL_128_ONLY);
    std::vector<const struct ArrowArray*> arrays;
    for (auto& b : h->batches) {
        if (b->sch.n_children != ncols) return set_error("Failed to create table from record batches.");
        for (int64_t c = 0; c < ncols; c++)
            if (describe_column(b->sch.children[c], DECIMAL_128_ONLY).signature() != info[c].signature()) return set_error("Failed to create table from record batches.");
        total += b->arr.length;
        arrays.push_back(&b->arr);
    }
    for (int64_t c = 0; c < ncols; c++) {
        if (info[c].kind == COL_NONE && info[c].has_dictionary)
            return set_error("Sort: column '%s' has a type the GPU path does not handle (format dictionary<%s, %s>)",
                             sch->children[c]->name, sch->children[c]->format, sch->children[c]->dictionary->format);
        if (info[c].kind == COL_NONE) return set_error("Sort: column '%s' has a type the GPU path does not handle (format %s)",
                                                       sch->children[c]->name, sch->children[c]->format);
    }
    std::vector<int> key_col;
    for (auto& name : h->cols) {
        int i = find_child(sch, name);
        if (i < 0) return set_error("Failed to sort table.");
        if (info[i].kind == COL_BOOL) return set_error("Failed to sort table.");   // (Arrow 3.0 has no boolean sort; algebra.py:191-201 rejects it first)
        key_col.push_back(i);
    }
    // Table::FromRecordBatches: every column of all batches as ONE column in HBM
    std::vector<DevSortCol> dev((size_t)ncols);
    PoolScope scratch;              // key helper buffers (ranks, decimal words)
    struct DictGuard { std::vector<vnm_strdict*> d; ~DictGuard() { for (auto* x : d) vnm_strdict_destroy(x); } } dicts;
    int rc = 0;
    for (int64_t c = 0; c < ncols && !rc; c++) rc = stage_sort_col(chunks_of(arrays, (int)c), info[c], total, &dev[c]);
    const int64_t n_out = (limit > 0 && limit < total) ? limit : total;
    int64_t* idx = nullptr;
    if (!rc && total > 0) {
        std::vector<vnm_dcol> keys;
        std::vector<int> orders;
        for (size_t k = 0; k < key_col.size() && !rc; k++) {
            const int c = key_col[k];
            DevSortCol& d = dev[c];
            vnm_dcol kc{};
            kc.length = total; kc.validity = d.validity;
            if (info[c].kind == COL_NUM) { keys.push_back(d.num); orders.push_back(h->orders[k]); continue; }
            if (info[c].kind == COL_DICT) {   // the codes are there already: ranks over the dictionary as COL_STR takes them after its encode
                int32_t* ranks = (int32_t*)scratch.take((size_t)total * 4);
                int32_t* rank_of = (int32_t*)scratch.take((size_t)std::max<int64_t>(vnm_strdict_ids(d.dict), 1) * 4);
                if (!ranks || !rank_of) { rc = 1; break; }
                rc = vnm_strdict_ranks_device(d.dict, rank_of, nullptr);
                if (!rc) rc = vnm_strdict_codes_to_ranks(d.codes, rank_of, total, ranks, nullptr);
                kc.values = ranks; kc.type = VNM_I32;
                keys.push_back(kc); orders.push_back(h->orders[k]);
                continue;
            }
            if (info[c].kind == COL_STR) {
                vnm_strdict* sd = vnm_strdict_create();
                if (!sd) { rc = 1; break; }
                dicts.d.push_back(sd);
                int32_t* codes = (int32_t*)scratch.take((size_t)total * 4);
                int32_t* ranks = (int32_t*)scratch.take((size_t)total * 4);
                if (!codes || !ranks) { rc = 1; break; }
                vnm_dcol oc{};
                oc.values = d.offs; oc.type = VNM_I64; oc.length = total + 1;
                rc = vnm_strdict_encode_device(sd, &oc, d.validity, 0, d.data, 0, codes, nullptr, nullptr, nullptr);
                int32_t* rank_of = nullptr;
                if (!rc) { rank_of = (int32_t*)scratch.take((size_t)std::max<int64_t>(vnm_strdict_ids(sd), 1) * 4); if (!rank_of) rc = 1; }
                if (!rc) rc = vnm_strdict_ranks_device(sd, rank_of, nullptr);
                if (!rc) rc = vnm_strdict_codes_to_ranks(codes, rank_of, total, ranks, nullptr);
                kc.values = ranks; kc.type = VNM_I32;
                keys.push_back(kc); orders.push_back(h->orders[k]);
            } else {   // COL_DEC
                int64_t* hi = (int64_t*)scratch.take((size_t)total * 8);
                uint64_t* lo = (uint64_t*)scratch.take((size_t)total * 8);
                if (!hi || !lo) { rc = 1; break; }
                rc = vnm_decimal128_sort_keys(d.fixed, total, hi, lo, nullptr);
                kc.values = hi; kc.type = VNM_I64;
                keys.push_back(kc); orders.push_back(h->orders[k]);
                kc.values = lo; kc.type = VNM_U64;
                keys.push_back(kc); orders.push_back(h->orders[k]);
            }
        }
        if (!rc && keys.size() > 16) rc = set_error("Sort: more than 16 sort key words");
        if (!rc) { idx = (int64_t*)pool_alloc((size_t)total * 8); if (!idx) rc = 1; }
        if (!rc) rc = vnm_sort_indices((int)keys.size(), keys.data(), orders.data(), total, n_out < total ? n_out : 0, idx, nullptr);
    }
    if (!rc) {
        make_struct(out, n_out, ncols);
        make_schema(out_schema, "+s", "", ncols);
        for (int64_t c = 0; c < ncols && !rc; c++) {
            rc = take_sort_col(dev[c], info[c], idx, n_out, out->children[c]);
            if (!rc) make_dict_schema(out_schema->children[c], info[c], sch->children[c]->name ? sch->children[c]->name : "");
        }
        if (rc) { release_array(out); release_schema(out_schema); }
    }
    if (!rc) {
        int64_t cols = 0, values = 0, skipped = 0;
        for (int64_t c = 0; c < ncols; c++)
            if (info[c].kind == COL_DICT) { cols++; values += dev[c].read.values_encoded; skipped += dev[c].read.dictionaries_skipped; }
        if (cols) route_note("sort:dictionary_key_ranks", "rows=%lld columns=%lld values_encoded=%lld dictionaries_skipped=%lld",
                             (long long)total, (long long)cols, (long long)values, (long long)skipped);
    }
    pool_free(idx);
    for (auto& d : dev) d.free_all();
    for (auto& b : h->batches) b->drop();
    h->batches.clear();
    return rc;
}

}  // extern "C"
