// The aggregate operator below the C ABI: vnm_agg_op_* (BaseAggregate::Next / Result, vinum_cpp/src/operators/aggregate/
// base_aggregate.cpp:23-68), its non-numeric keys and its MIN / MAX over strings.
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "vnm_agg.hpp"
#include "vnm_arrow.hpp"

using namespace vnm;

// ---- non-numeric GROUP BY keys and COUNT inputs below the C ABI (round 6) ------------------------------------------------------------
// GenericHashAggregate (vinum_cpp/src/operators/aggregate/generic_hash_aggregate.h:10-45, bound at vinum/core/vinum_lib.cpp:92-109) keys
// its map on arrow::Scalar vectors of ANY type.  Here a utf8 / large_utf8 / binary / large_binary key column becomes the int32 codes of a
// per-operator device string dictionary (vnm_strdict: the bytes cross PCIe once, equal bytes <=> equal code across all batches), a boolean
// key its 0 / 1, a decimal128 key the index of its 16-byte value in a host map; the codes are an ordinary int32 key column of the numeric
// operators (NULL stays NULL through the column's own validity bitmap), and result() turns the groups' codes back into values of the
// column's type.  COUNT over a non-numeric column counts through an int8 stand-in with the column's validity (CountFunc, agg_funcs.h:
// 129-161, reads nothing but the validity).  A dictionary-typed string column travels as the codes stage_dict_codes (vnm_arrow.cpp)
// makes of it.  MIN / MAX of strings: strmm_* below.
struct GenKey {
    ColDesc d;                     // what the column is (COL_NUM: travels as it is)
    vnm_strdict* dict = nullptr;   // COL_STR, COL_DICT
    DictValues values;             // ... and the host copy of its values
    std::map<std::pair<uint64_t, uint64_t>, int32_t> dec_id;      // COL_DEC: (low, high) words -> code
    std::vector<std::pair<uint64_t, uint64_t>> dec_val;
    ~GenKey() { if (dict) vnm_strdict_destroy(dict); }
};
// a non-numeric key column -> int32 codes in HBM
static int stage_generic_key(GenKey& g, const std::vector<ColChunk>& chunks, int64_t total, vnm_dcol* out) {
    if (g.d.kind == COL_DICT) {
        int32_t* codes = nullptr;
        uint8_t* valid = nullptr;
        DictReadStats read;
        VNM_TRY(stage_dict_codes(g.dict, &g.values, g.d, chunks, total, "a dictionary-typed column without its dictionary or indices", &codes, &valid, &read));
        route_note("keys:dictionary_child", "rows=%lld values_encoded=%lld dictionaries_skipped=%lld", (long long)total, (long long)read.values_encoded, (long long)read.dictionaries_skipped);
        memset(out, 0, sizeof(*out));
        out->values = codes; out->validity = valid; out->type = VNM_I32; out->length = total;
        return 0;
    }
    std::vector<int32_t> codes((size_t)(total ? total : 1), -1);
    int64_t pos = 0;
    for (auto& c : chunks) {
        if (!c.len) continue;
        const uint8_t* valid = chunk_validity(c);
        auto is_valid = [&](int64_t i) { return !valid || ((valid[(c.off + i) >> 3] >> ((c.off + i) & 7)) & 1); };
        if (g.d.kind == COL_STR) {
            int64_t n_new = 0, new_bytes = 0;
            VNM_TRY(vnm_strdict_encode(g.dict, c.col->buffers[1], g.d.wide ? 1 : 0, (const uint8_t*)c.col->buffers[2], valid, c.off, c.len, codes.data() + pos, &n_new, &new_bytes, nullptr));
            VNM_TRY(append_new_values(g.dict, &g.values, n_new, new_bytes));
        } else if (g.d.kind == COL_BOOL) {
            const uint8_t* v = (const uint8_t*)c.col->buffers[1];
            for (int64_t i = 0; i < c.len; i++) if (is_valid(i)) codes[(size_t)(pos + i)] = (v[(c.off + i) >> 3] >> ((c.off + i) & 7)) & 1;
        } else {
            const uint64_t* v = (const uint64_t*)c.col->buffers[1];
            for (int64_t i = 0; i < c.len; i++) {
                if (!is_valid(i)) continue;
                const std::pair<uint64_t, uint64_t> key(v[2 * (c.off + i)], v[2 * (c.off + i) + 1]);
                auto it = g.dec_id.find(key);
                if (it == g.dec_id.end()) { it = g.dec_id.emplace(key, (int32_t)g.dec_val.size()).first; g.dec_val.push_back(key); }
                codes[(size_t)(pos + i)] = it->second;
            }
        }
        pos += c.len;
    }
    const std::vector<uint8_t> bits = chunks_validity(chunks, total);
    VNM_TRY(vnm_stage_column(codes.data(), bits.empty() ? nullptr : bits.data(), 0, total, VNM_I32, out, nullptr));
    if (hipStreamSynchronize(nullptr) != hipSuccess) return set_error("staging a key column's codes failed");   // (codes / bits are locals)
    return 0;
}
// COUNT over a non-numeric column: zeros with the column's validity
static int stage_count_standin(const std::vector<ColChunk>& chunks, int64_t total, vnm_dcol* out) {
    const std::vector<uint8_t> zeros((size_t)(total ? total : 1), 0);
    const std::vector<uint8_t> bits = chunks_validity(chunks, total);
    VNM_TRY(vnm_stage_column(zeros.data(), bits.empty() ? nullptr : bits.data(), 0, total, VNM_I8, out, nullptr));
    if (hipStreamSynchronize(nullptr) != hipSuccess) return set_error("staging a COUNT stand-in failed");
    return 0;
}
// A non-numeric result column (group key, string MIN / MAX) of the type it came in with, from the groups' codes (host: int32 values +
// validity bytes).  A dictionary-typed column: the codes go back to the device and leave through make_dict_array (rows = NULL); the
// NULL group stays NULL.
static int make_key_column(struct ArrowArray* a, const GenKey& g, int64_t n, const int32_t* codes, const uint8_t* valid_bytes) {
    if (g.d.kind == COL_STR) return make_string_array(g.values, a, g.d.wide, codes, valid_bytes, n, "a result column");
    if (g.d.kind == COL_DICT) {
        const size_t n1 = (size_t)(n ? n : 1);
        std::vector<int32_t> hc(n1, -1);
        for (int64_t i = 0; i < n; i++) if (valid_bytes[i]) hc[(size_t)i] = codes[i];
        PoolScope pool;
        int32_t* dcodes = (int32_t*)pool.take(n1 * 4);
        if (!dcodes) return 1;
        VNM_HIP(hipMemcpy(dcodes, hc.data(), n1 * 4, hipMemcpyHostToDevice));
        return make_dict_array(dcodes, nullptr, n, g.d, g.dict, g.values, a);
    }
    make_array(a, n, 2);
    uint8_t* bm = pack_bits(valid_bytes, n, &a->null_count);
    if (a->null_count) a->buffers[0] = bm; else free(bm);
    if (g.d.kind == COL_BOOL) {
        uint8_t* v = (uint8_t*)calloc((size_t)((n + 7) / 8 + 1), 1);
        for (int64_t i = 0; i < n; i++) if (valid_bytes[i] && codes[i] == 1) v[i >> 3] |= (uint8_t)(1u << (i & 7));
        a->buffers[1] = v;
        return 0;
    }
    uint64_t* v = (uint64_t*)calloc((size_t)(n ? n : 1) * 2, 8);
    for (int64_t i = 0; i < n; i++)
        if (valid_bytes[i] && codes[i] >= 0 && (size_t)codes[i] < g.dec_val.size()) { v[2 * i] = g.dec_val[(size_t)codes[i]].first; v[2 * i + 1] = g.dec_val[(size_t)codes[i]].second; }
    a->buffers[1] = v;
    return 0;
}

// ---- MIN / MAX over utf8 / large_utf8 / binary / large_binary columns below the C ABI -------------------------------------------------
// StringMinMaxFunc (agg_funcs.h:219-261): NULLs skipped, a group of NULLs only gives NULL, values compared byte-wise.  The device
// aggregates order-preserving RANKS: a column's values go through ONE dictionary that grows with the operator (vnm_strdict: the bytes of
// a value cross PCIe once), and for every device-sized batch a throw-away operator of the caller's kind takes MIN / MAX of
// rank(value) per group, ranks taken over the dictionary as it stands (vnm_strdict_ranks_device).  What it leaves is one CANDIDATE per
// group and function -- the id of the winning value, which does not depend on later growth -- kept in HBM as a chunk (group keys +
// ids).  Chunks are folded (the same operator over the chunks, ids ranked against the dictionary of that moment) whenever they
// hold more than twice the groups of the last fold: nothing accumulates per batch.  result() folds once more and lines the
// candidates up with the numeric operator's groups by key.
struct StrCol { int child = -1; GenKey dict; };
struct StrFn { int func = 0; int op_idx = 0; int col = 0; };          // VNM_MIN / VNM_MAX, index among the operator's functions, index into strcols
struct CandChunk {
    int64_t n = 0;
    std::vector<void*> kv; std::vector<uint8_t*> kb; std::vector<int64_t> knull;      // per key column: values of the key's width, bitmap, NULL count
    std::vector<int32_t*> ids; std::vector<uint8_t*> idb; std::vector<int64_t> idnull;  // per string function: candidate ids (-1 = NULL), bitmap
    void drop() {
        for (void* p : kv) pool_free(p);
        for (uint8_t* p : kb) pool_free(p);
        for (int32_t* p : ids) pool_free(p);
        for (uint8_t* p : idb) pool_free(p);
        kv.clear(); kb.clear(); ids.clear(); idb.clear(); knull.clear(); idnull.clear(); n = 0;
    }
};
__global__ void strmm_invert_kernel(const int32_t* rank_of_id, int64_t top, int32_t* id_of_rank) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < top && rank_of_id[id] >= 0) id_of_rank[rank_of_id[id]] = (int32_t)id;
}
__global__ void strmm_rank_to_id_kernel(const int32_t* ranks, const uint8_t* bitmap, int64_t n, const int32_t* id_of_rank, int32_t* ids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool valid = !bitmap || ((bitmap[i >> 3] >> (i & 7)) & 1);
    ids[i] = valid ? id_of_rank[ranks[i]] : -1;
}

static bool has_strdict(const ColDesc& d) { return d.kind == COL_STR || d.kind == COL_DICT; }   // its values go through a vnm_strdict

struct vnm_agg_op {
    int kind;
    std::vector<std::unique_ptr<GenKey>> gkeys;   // per group-by column: how a non-numeric key travels (COL_NUM: as it is)
    std::vector<char> standin;                    // per function: COUNT over a non-numeric column (int8 stand-in with its validity)
    // per function: COUNT over a dictionary-typed string column counts its CODES (valid by index and by value); the dictionary is
    // the key's when the column is a key too, one of count_dicts otherwise
    std::vector<GenKey*> count_gk;
    std::vector<std::unique_ptr<GenKey>> count_dicts;
    std::vector<std::string> groupby, agg_cols, in_cols, out_cols;
    std::vector<int> funcs;
    vnm_agg* dev = nullptr;
    bool inited = false;
    std::vector<int> key_idx, in_idx, aggcol_key;  // child indices; agg_col -> position in groupby
    std::vector<ColType> key_t, in_t;
    // small batches wait here until they add up to a device-sized one (vnm_agg_op_next)
    std::vector<std::unique_ptr<ImportedBatch>> pending;
    int64_t pending_rows = 0;
    std::vector<std::string> formats, names;   // children of the first batch: later batches must match on the columns used
    // MIN / MAX over utf8 / binary columns (StringMinMaxFunc, agg_funcs.h:219-261), see strmm_* below
    std::vector<std::unique_ptr<StrCol>> strcols;   // one device dictionary per such column
    std::vector<StrFn> strfns;
    std::vector<int> dev_of;                        // operator function -> function of the device operator (-1: a string function)
    std::vector<CandChunk> cands;
    int64_t cand_rows = 0, cand_floor = 0;
    int n_dev = 0;                                  // functions of the device operator
};

static int agg_op_init(vnm_agg_op* h, const struct ArrowSchema* sch) {
    // a failed earlier attempt (unknown column, unsupported type) must not leave half-filled index vectors behind
    h->key_idx.clear(); h->key_t.clear(); h->in_idx.clear(); h->in_t.clear(); h->aggcol_key.clear(); h->gkeys.clear(); h->standin.clear();
    h->strcols.clear(); h->strfns.clear(); h->dev_of.clear(); h->count_gk.clear(); h->count_dicts.clear();
    for (auto& c : h->cands) c.drop();
    h->cands.clear(); h->cand_rows = 0; h->cand_floor = 0;
    if (h->dev) { vnm_agg_destroy(h->dev); h->dev = nullptr; }
    // lookup_col_indices base_aggregate.cpp:121-131
    for (auto& c : h->groupby) {
        int i = find_child(sch, c);
        if (i < 0) return set_error("Column not found: %s", c.c_str());
        h->key_idx.push_back(i);
        std::unique_ptr<GenKey> g(new GenKey());
        g->d = describe_column(sch->children[i], DECIMAL_ANY_COMMA_128);
        h->key_t.push_back(g->d.t);
        if (g->d.kind != COL_NUM) {   // a non-numeric key: its codes travel (the column keeps its format for the result)
            if (g->d.kind == COL_NONE || h->kind == VNM_ONE_GROUP) return set_error("Unsupported data type for aggregation column.");
            if (has_strdict(g->d) && !(g->dict = vnm_strdict_create())) return 1;
            h->key_t.back().type = VNM_I32;
        }
        h->gkeys.push_back(std::move(g));
    }
    for (auto& c : h->agg_cols) {
        int pos = -1;
        for (size_t j = 0; j < h->groupby.size(); j++) if (h->groupby[j] == c) pos = (int)j;
        if (find_child(sch, c) < 0) return set_error("Column not found: %s", c.c_str());
        if (pos < 0) return set_error("aggregate column %s is not a group-by column", c.c_str());
        h->aggcol_key.push_back(pos);
    }
    std::vector<int> ktypes, itypes, iflags, ids, dfuncs;
    for (auto& t : h->key_t) ktypes.push_back(t.type);
    for (size_t i = 0; i < h->funcs.size(); i++) {
        h->standin.push_back(0);
        h->count_gk.push_back(nullptr);
        h->dev_of.push_back((int)dfuncs.size());
        if (h->funcs[i] == VNM_COUNT_STAR || h->in_cols[i].empty()) {
            h->in_idx.push_back(-1);
            h->in_t.push_back(ColType());
            dfuncs.push_back(h->funcs[i]); itypes.push_back(VNM_U64); iflags.push_back(0); ids.push_back(-1);
            continue;
        }
        int ci = find_child(sch, h->in_cols[i]);
        if (ci < 0) return set_error("Column not found: %s", h->in_cols[i].c_str());
        const ColDesc how = describe_column(sch->children[ci], DECIMAL_ANY_COMMA_128);
        ColType t = how.t;
        if (how.kind != COL_NUM) t.type = -1;   // (a dictionary-typed child is judged by its values, never read as its indices)
        h->in_idx.push_back(ci);
        h->in_t.push_back(t);
        if (t.type < 0 && (h->funcs[i] == VNM_MIN || h->funcs[i] == VNM_MAX) && has_strdict(how)) {
            // MIN / MAX of strings / binaries: not a function of the device operator (strmm_* below)
            int col = -1;
            for (size_t q = 0; q < h->strcols.size(); q++) if (h->strcols[q]->child == ci) col = (int)q;
            if (col < 0) {
                std::unique_ptr<StrCol> sc(new StrCol());
                sc->child = ci;
                sc->dict.d = how;
                if (!(sc->dict.dict = vnm_strdict_create())) return 1;
                col = (int)h->strcols.size();
                h->strcols.push_back(std::move(sc));
            }
            StrFn sf; sf.func = h->funcs[i]; sf.op_idx = (int)i; sf.col = col;
            h->strfns.push_back(sf);
            h->dev_of.back() = -1;
            continue;
        }
        if (t.type < 0 && h->funcs[i] != VNM_COUNT) {
            switch (h->funcs[i]) {
                case VNM_MIN: case VNM_MAX: return set_error("Column data type is not supported by min()/max().");
                case VNM_SUM: return set_error("Column data type is not supported by sum().");
                default: return set_error("Column data type is not supported by avg().");
            }
        }
        if (t.type < 0 && how.kind == COL_DICT) {   // COUNT over a dictionary-typed string column: its codes, NULL where the row OR its value is
            GenKey* g = nullptr;
            for (size_t j = 0; j < h->key_idx.size(); j++) if (h->key_idx[j] == ci) g = h->gkeys[j].get();
            for (size_t q = 0; !g && q < i; q++) if (h->count_gk[q] && h->in_idx[q] == ci) g = h->count_gk[q];
            if (!g) {
                std::unique_ptr<GenKey> own(new GenKey());
                own->d = how;
                if (!(own->dict = vnm_strdict_create())) return 1;
                g = own.get();
                h->count_dicts.push_back(std::move(own));
            }
            h->count_gk.back() = g;
            h->in_t.back().type = VNM_I32;
            dfuncs.push_back(h->funcs[i]); itypes.push_back(VNM_I32); iflags.push_back(0); ids.push_back(1000000 + ci);
            continue;
        }
        if (t.type < 0) {   // COUNT over a non-numeric column: an int8 stand-in with the column's validity (its own column id: the same
                            // column may also be a key, which travels as codes)
            h->standin.back() = 1;
            h->in_t.back().type = VNM_I8;
            dfuncs.push_back(h->funcs[i]); itypes.push_back(VNM_I8); iflags.push_back(0); ids.push_back(1000000 + ci);
            continue;
        }
        dfuncs.push_back(h->funcs[i]); itypes.push_back(t.type); iflags.push_back(t.flags); ids.push_back(ci);
    }
    if (dfuncs.empty() && !h->strfns.empty()) {   // string functions only: the device operator still lists the groups (a COUNT(*) nobody reads)
        dfuncs.push_back(VNM_COUNT_STAR); itypes.push_back(VNM_U64); iflags.push_back(0); ids.push_back(-1);
    }
    h->n_dev = (int)dfuncs.size();
    h->dev = vnm_agg_create(h->kind, (int)ktypes.size(), ktypes.data(), (int)dfuncs.size(), dfuncs.data(),
                            itypes.data(), iflags.data(), ids.data());
    if (!h->dev) return 1;
    h->inited = true;
    return 0;
}

extern "C" {

vnm_agg_op* vnm_agg_op_create(int kind, int n_groupby, const char** groupby_cols, int n_aggcols, const char** agg_cols,
                              int n_funcs, const int* func_types, const char** in_cols, const char** out_cols) {
    if (ensure_init()) return nullptr;
    if (kind < VNM_ONE_GROUP || kind > VNM_MULTI_NUMERICAL) { set_error("vnm_agg_op_create: bad operator kind %d", kind); return nullptr; }
    vnm_agg_op* h = new vnm_agg_op();
    h->kind = kind;
    for (int i = 0; i < n_groupby; i++) h->groupby.push_back(groupby_cols[i]);
    for (int i = 0; i < n_aggcols; i++) h->agg_cols.push_back(agg_cols[i]);
    for (int i = 0; i < n_funcs; i++) {
        if (func_types[i] < VNM_COUNT_STAR || func_types[i] > VNM_AVG) { set_error("Unrecognized Aggregate function type."); delete h; return nullptr; }
        h->funcs.push_back(func_types[i]);
        h->in_cols.push_back(in_cols[i] ? in_cols[i] : "");
        h->out_cols.push_back(out_cols[i] ? out_cols[i] : "");
    }
    return h;
}

void vnm_agg_op_destroy(vnm_agg_op* h) {
    if (!h) return;
    for (auto& b : h->pending) b->drop();
    if (h->dev) vnm_agg_destroy(h->dev);
    for (auto& c : h->cands) c.drop();
    delete h;
}

}  // extern "C"

// ---- string MIN / MAX: one throw-away operator over (keys, ranks) -> a chunk of candidates --------------------------------------------
struct StrmmBatch { int64_t n; std::vector<vnm_dcol> keys; std::vector<vnm_dcol> ids; };   // ids: per string FUNCTION, int32 dictionary ids with validity
static int strmm_run(vnm_agg_op* h, const std::vector<StrmmBatch>& batches, CandChunk* out) {
    const int nk = (int)h->key_idx.size(), nf = (int)h->strfns.size(), nc = (int)h->strcols.size();
    std::vector<int> ktypes, funcs, itypes, iflags, ids;
    for (auto& t : h->key_t) ktypes.push_back(t.type);
    for (int f = 0; f < nf; f++) { funcs.push_back(h->strfns[f].func); itypes.push_back(VNM_I32); iflags.push_back(0); ids.push_back(f); }
    vnm_agg* tmp = vnm_agg_create(h->kind, nk, ktypes.data(), nf, funcs.data(), itypes.data(), iflags.data(), ids.data());
    if (!tmp) return 1;
    PoolScope pool;
    int rc = 0;
    // ranks of every dictionary as it stands now, and their inverse
    std::vector<int32_t*> rank_of(nc, nullptr), id_of(nc, nullptr);
    for (int c = 0; !rc && c < nc; c++) {
        const int64_t top = std::max<int64_t>(1, vnm_strdict_ids(h->strcols[c]->dict.dict));
        rank_of[c] = (int32_t*)pool.take((size_t)top * 4);
        id_of[c] = (int32_t*)pool.take((size_t)top * 4);
        if (!rank_of[c] || !id_of[c]) { rc = 1; break; }
        if (hipMemsetAsync(rank_of[c], 0xFF, (size_t)top * 4, nullptr) != hipSuccess || hipMemsetAsync(id_of[c], 0xFF, (size_t)top * 4, nullptr) != hipSuccess) { rc = set_error("string min / max: memset failed"); break; }
        rc = vnm_strdict_ranks_device(h->strcols[c]->dict.dict, rank_of[c], nullptr);
        if (!rc) {
            strmm_invert_kernel<<<(int)((top + 255) / 256), 256, 0, nullptr>>>(rank_of[c], top, id_of[c]);
            if (hipGetLastError() != hipSuccess) rc = set_error("string min / max: kernel launch failed");
        }
    }
    for (size_t b = 0; !rc && b < batches.size(); b++) {
        const StrmmBatch& sb = batches[b];
        if (sb.n <= 0) continue;
        PoolScope bp;
        std::vector<vnm_dcol> inputs((size_t)nf);
        for (int f = 0; !rc && f < nf; f++) {
            int same = -1;   // (two functions over one column of a data batch share the rank column)
            for (int g = 0; g < f; g++) if (sb.ids[g].values == sb.ids[f].values && sb.ids[g].offset == sb.ids[f].offset) same = g;
            if (same >= 0) { inputs[f] = inputs[same]; continue; }
            int32_t* r = (int32_t*)bp.take((size_t)sb.n * 4);
            if (!r) { rc = 1; break; }
            rc = vnm_strdict_codes_to_ranks((const int32_t*)sb.ids[f].values + sb.ids[f].offset, rank_of[h->strfns[f].col], sb.n, r, nullptr);
            inputs[f] = sb.ids[f];
            inputs[f].values = r - sb.ids[f].offset;      // (the validity bitmap keeps the column's own offset)
        }
        if (!rc) rc = vnm_agg_next_device(tmp, sb.n, sb.keys.data(), inputs.data(), nullptr, nullptr);
        if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) rc = set_error("string min / max: stream synchronisation failed");
    }
    int64_t n = 0;
    if (!rc) rc = vnm_agg_finish(tmp, &n, nullptr);
    if (!rc) {
        out->n = n;
        const size_t bm_bytes = (size_t)((n + 63) / 64 + 1) * 8;
        for (int j = 0; !rc && j < nk; j++) {
            void* v = pool_alloc((size_t)(n ? n : 1) * 8);
            uint8_t* bm = (uint8_t*)pool_alloc(bm_bytes);
            int64_t nulls = 0;
            out->kv.push_back(v); out->kb.push_back(bm); out->knull.push_back(0);
            if (!v || !bm) { rc = 1; break; }
            rc = vnm_agg_result_key_device(tmp, j, v, bm, &nulls, nullptr);
            out->knull.back() = nulls;
        }
        for (int f = 0; !rc && f < nf; f++) {
            int32_t* rv = (int32_t*)pool.take((size_t)(n ? n : 1) * 8);
            int32_t* idv = (int32_t*)pool_alloc((size_t)(n ? n : 1) * 4);
            uint8_t* bm = (uint8_t*)pool_alloc(bm_bytes);
            int kind = 0;
            int64_t nulls = 0;
            out->ids.push_back(idv); out->idb.push_back(bm); out->idnull.push_back(0);
            if (!rv || !idv || !bm) { rc = 1; break; }
            rc = vnm_agg_result_func_device(tmp, f, rv, bm, &kind, &nulls, nullptr);
            out->idnull.back() = nulls;
            if (!rc && n) {
                strmm_rank_to_id_kernel<<<(int)((n + 255) / 256), 256, 0, nullptr>>>(rv, nulls ? bm : nullptr, n, id_of[h->strfns[f].col], idv);
                if (hipGetLastError() != hipSuccess) rc = set_error("string min / max: kernel launch failed");
            }
        }
        if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) rc = set_error("string min / max: stream synchronisation failed");
    }
    vnm_agg_destroy(tmp);
    if (rc) out->drop();
    return rc;
}
// all chunks -> one (the candidates of every chunk ranked against the dictionary of this moment)
static int strmm_fold(vnm_agg_op* h) {
    if (h->cands.size() <= 1) return 0;
    const int nk = (int)h->key_idx.size(), nf = (int)h->strfns.size();
    std::vector<StrmmBatch> bs;
    for (auto& ch : h->cands) {
        StrmmBatch sb; sb.n = ch.n;
        for (int j = 0; j < nk; j++) {
            vnm_dcol d; memset(&d, 0, sizeof(d));
            d.values = ch.kv[j]; d.validity = ch.knull[j] ? ch.kb[j] : nullptr; d.length = ch.n; d.type = h->key_t[j].type; d.flags = h->key_t[j].flags;
            sb.keys.push_back(d);
        }
        for (int f = 0; f < nf; f++) {
            vnm_dcol d; memset(&d, 0, sizeof(d));
            d.values = ch.ids[f]; d.validity = ch.idnull[f] ? ch.idb[f] : nullptr; d.length = ch.n; d.type = VNM_I32;
            sb.ids.push_back(d);
        }
        bs.push_back(std::move(sb));
    }
    CandChunk folded;
    VNM_TRY(strmm_run(h, bs, &folded));
    for (auto& ch : h->cands) ch.drop();
    h->cands.clear();
    h->cand_rows = folded.n;
    h->cand_floor = folded.n;
    h->cands.push_back(std::move(folded));
    return 0;
}
// the string columns of one device batch (chunks_of(child) = where its rows lie) -> one more chunk of candidates
template <class ChunksOf>
static int strmm_batch(vnm_agg_op* h, int64_t total, const std::vector<vnm_dcol>& keys, ChunksOf chunks_of) {
    if (h->strfns.empty() || total <= 0) return 0;
    const int nc = (int)h->strcols.size();
    std::vector<vnm_dcol> idcols((size_t)nc);
    int rc = 0, staged = 0;
    for (int c = 0; !rc && c < nc; c++, staged += !rc) rc = stage_generic_key(h->strcols[c]->dict, chunks_of(h->strcols[c]->child), total, &idcols[c]);
    if (!rc) {
        StrmmBatch sb; sb.n = total; sb.keys = keys;
        for (auto& f : h->strfns) sb.ids.push_back(idcols[f.col]);
        CandChunk ch;
        rc = strmm_run(h, std::vector<StrmmBatch>{sb}, &ch);
        if (!rc) { h->cand_rows += ch.n; h->cands.push_back(std::move(ch)); }
    }
    for (int c = 0; c < staged; c++) vnm_free_column(&idcols[c]);
    if (!rc && h->cands.size() > 1 && h->cand_rows > 2 * std::max<int64_t>(h->cand_floor, (int64_t)1 << 16)) rc = strmm_fold(h);
    return rc;
}

// result(): the folded candidates lined up with the numeric operator's groups by key -> per string function, the winning id of every group
static int strmm_join(vnm_agg_op* h, int64_t n, std::vector<std::vector<int32_t>>* ids_of_fn) {
    const int nk = (int)h->key_idx.size(), nf = (int)h->strfns.size();
    ids_of_fn->assign((size_t)nf, std::vector<int32_t>((size_t)(n ? n : 1), -1));
    if (h->cands.empty() || n == 0) return 0;
    const CandChunk& ch = h->cands[0];
    const int64_t m = ch.n;
    std::vector<int> width((size_t)nk);
    size_t klen = 0;
    for (int j = 0; j < nk; j++) { width[j] = type_width(h->key_t[j].type); klen += 1 + (size_t)width[j]; }
    // candidates: key bytes -> row
    std::vector<std::vector<uint8_t>> cv((size_t)nk), cb((size_t)nk);
    for (int j = 0; j < nk; j++) {
        cv[j].resize((size_t)(m ? m : 1) * width[j]);
        if (m && hipMemcpy(cv[j].data(), ch.kv[j], (size_t)m * width[j], hipMemcpyDeviceToHost) != hipSuccess) return set_error("string min / max: device to host copy failed");
        if (ch.knull[j]) {
            cb[j].resize((size_t)(m + 7) / 8);
            if (hipMemcpy(cb[j].data(), ch.kb[j], cb[j].size(), hipMemcpyDeviceToHost) != hipSuccess) return set_error("string min / max: device to host copy failed");
        }
    }
    auto key_of = [&](std::string& k, int64_t r, const std::vector<const uint8_t*>& vals, const std::vector<int>& stride, const std::vector<std::function<bool(int64_t)>>& valid) {
        k.assign(klen, '\0');
        size_t at = 0;
        for (int j = 0; j < nk; j++) {
            const bool v = valid[j](r);
            k[at++] = v ? 1 : 0;
            if (v) memcpy(&k[at], vals[j] + (size_t)r * stride[j], (size_t)width[j]);
            at += (size_t)width[j];
        }
    };
    std::unordered_map<std::string, int64_t> row_of;
    row_of.reserve((size_t)m * 2 + 16);
    {
        std::vector<const uint8_t*> vals; std::vector<int> stride; std::vector<std::function<bool(int64_t)>> valid;
        for (int j = 0; j < nk; j++) {
            vals.push_back(cv[j].data()); stride.push_back(width[j]);
            const uint8_t* bm = ch.knull[j] ? cb[j].data() : nullptr;
            valid.push_back([bm](int64_t r) { return !bm || ((bm[r >> 3] >> (r & 7)) & 1); });
        }
        std::string k;
        for (int64_t r = 0; r < m; r++) { key_of(k, r, vals, stride, valid); row_of.emplace(k, r); }
    }
    std::vector<std::vector<int32_t>> cid((size_t)nf);
    for (int f = 0; f < nf; f++) {
        cid[f].resize((size_t)(m ? m : 1));
        if (m && hipMemcpy(cid[f].data(), ch.ids[f], (size_t)m * 4, hipMemcpyDeviceToHost) != hipSuccess) return set_error("string min / max: device to host copy failed");
    }
    // the numeric operator's groups
    std::vector<std::vector<uint64_t>> mv((size_t)nk);
    std::vector<std::vector<uint8_t>> mb((size_t)nk);
    for (int j = 0; j < nk; j++) {
        mv[j].resize((size_t)n); mb[j].resize((size_t)n);
        VNM_TRY(vnm_agg_result_key(h->dev, j, mv[j].data(), mb[j].data()));
    }
    std::vector<const uint8_t*> vals; std::vector<int> stride; std::vector<std::function<bool(int64_t)>> valid;
    for (int j = 0; j < nk; j++) {
        vals.push_back((const uint8_t*)mv[j].data()); stride.push_back(8);
        const uint8_t* vb = mb[j].data();
        valid.push_back([vb](int64_t r) { return vb[r] != 0; });
    }
    std::string k;
    for (int64_t r = 0; r < n; r++) {
        key_of(k, r, vals, stride, valid);
        auto it = row_of.find(k);
        if (it == row_of.end()) continue;
        for (int f = 0; f < nf; f++) (*ids_of_fn)[f][(size_t)r] = cid[f][(size_t)it->second];
    }
    return 0;
}
// string function f of the result: the winning ids as values of the column's type, and the column's schema
static int strmm_column(vnm_agg_op* h, int f, int64_t n, const std::vector<int32_t>& ids, const std::string& name, struct ArrowArray* out, struct ArrowSchema* out_schema) {
    const GenKey& g = h->strcols[(size_t)h->strfns[(size_t)f].col]->dict;
    make_dict_schema(out_schema, g.d, name);
    std::vector<uint8_t> vb((size_t)(n ? n : 1));
    for (int64_t r = 0; r < n; r++) vb[(size_t)r] = ids[(size_t)r] >= 0;
    return make_key_column(out, g, n, ids.data(), vb.data());
}

// One device batch: the `total` rows of `batches` (struct arrays; child ci of each is one chunk of column ci).  Every column the
// operator reads is staged once per form, the device operator takes the batch, the string MIN / MAX columns follow.  A numeric column
// that is a single chunk -- a large batch on its own -- goes straight from its own buffers (stage_child); several chunks are joined.
static int agg_op_run_batch(vnm_agg_op* h, const std::vector<const struct ArrowArray*>& batches, int64_t total) {
    std::vector<vnm_dcol> keys(h->key_idx.size()), inputs((size_t)std::max(h->n_dev, 1));
    for (auto& d : inputs) { memset(&d, 0, sizeof(vnm_dcol)); d.length = total; }
    std::map<std::pair<int, int>, vnm_dcol> staged;   // (child, form: 0 as it is / 1 key codes / 2 COUNT stand-in)
    int rc = 0;
    auto get = [&](int ci, const ColType& t, vnm_dcol* out, GenKey* g = nullptr, bool standin = false) -> int {
        const int form = g && g->d.kind != COL_NUM ? 1 : (standin ? 2 : 0);
        auto it = staged.find({ci, form});
        if (it == staged.end()) {
            vnm_dcol d;
            const std::vector<ColChunk> chunks = chunks_of(batches, ci);
            if (form == 1) VNM_TRY(stage_generic_key(*g, chunks, total, &d));
            else if (form == 2) VNM_TRY(stage_count_standin(chunks, total, &d));
            else if (chunks.size() == 1) VNM_TRY(stage_child(chunks[0], t, &d, nullptr));
            else VNM_TRY(stage_children(chunks, t, total, &d));
            it = staged.emplace(std::make_pair(ci, form), d).first;
        }
        *out = it->second;
        return 0;
    };
    for (size_t j = 0; !rc && j < h->key_idx.size(); j++) rc = get(h->key_idx[j], h->key_t[j], &keys[j], h->gkeys[j].get());
    for (size_t i = 0; !rc && i < h->funcs.size(); i++)
        if (h->dev_of[i] >= 0 && h->in_idx[i] >= 0) rc = get(h->in_idx[i], h->in_t[i], &inputs[(size_t)h->dev_of[i]], h->count_gk[i], h->standin[i] != 0);
    if (!rc && total > 0) rc = vnm_agg_next_device(h->dev, total, keys.data(), inputs.data(), nullptr, nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) rc = set_error("vnm_agg_op_next: stream synchronisation failed");
    if (!rc) rc = strmm_batch(h, total, keys, [&](int ci) { return chunks_of(batches, ci); });
    for (auto& kv : staged) vnm_free_column(&kv.second);
    return rc;
}

// one device batch out of everything that is pending
static int agg_op_flush(vnm_agg_op* h) {
    if (h->pending.empty()) return 0;
    std::vector<const struct ArrowArray*> batches;
    for (auto& b : h->pending) batches.push_back(&b->arr);
    const int rc = agg_op_run_batch(h, batches, h->pending_rows);
    for (auto& b : h->pending) b->drop();
    h->pending.clear();
    h->pending_rows = 0;
    return rc;
}

// (function, the device operator's output kind, the input's type) -> the result column's Arrow format and the width of its values
static std::pair<std::string, int> result_format(int f, int kind, const ColType& t) {
    if (f == VNM_MIN || f == VNM_MAX) return {t.format, type_width(t.type)};   // type preserving (agg_func_factory.cpp:35-107)
    switch (kind) {
        case VNM_OUT_U64: return {"L", 8};
        case VNM_OUT_I64: return {f == VNM_SUM && (t.format == "ttu" || t.format == "ttn" || t.format.rfind("tD", 0) == 0) ? t.format : "l", 8};
        case VNM_OUT_I32: return {t.format, 4};
        case VNM_OUT_F64: return {"g", 8};
        case VNM_OUT_F32: return {"f", 4};
        default: return {"d:38,0", 16};   // an int64 / uint64 SUM past 64 bits (host finaliser only)
    }
}

extern "C" {

// The reference streams 10 000-row batches by default (vinum/__init__.py:52, table_batch_reader.cpp:5-16); a launch per such
// batch would cost more than its rows.  Batches below 2^20 rows are therefore kept (the operator owns them: Arrow C Data
// move semantics) until 2^22 rows are waiting -- or result() is called -- and then go to the device as ONE batch; a large batch
// is staged straight from its own buffers as before.  Aggregates do not depend on where batches are cut (every accumulator
// merges commutatively, float sums are compensated), so the result is the same.
int vnm_agg_op_next(vnm_agg_op* h, struct ArrowArray* batch, struct ArrowSchema* schema) {
    if (!h || !batch || !schema) return set_error("vnm_agg_op_next: null argument");
    std::unique_ptr<ImportedBatch> ibp(new ImportedBatch());
    ImportedBatch& ib = *ibp;
    ib.arr = *batch; ib.sch = *schema; ib.live = true;
    batch->release = nullptr; schema->release = nullptr;  // ownership moved (Arrow C Data Interface move semantics)
    int rc = 0;
    auto signature = [&](int64_t c) { return describe_column(ib.sch.children[c], DECIMAL_ANY_COMMA_128).signature(); };
    if (!h->inited) {
        rc = agg_op_init(h, &ib.sch);
        if (!rc) {
            h->formats.clear(); h->names.clear();
            for (int64_t c = 0; c < ib.sch.n_children; c++) {
                h->formats.push_back(signature(c));
                h->names.push_back(ib.sch.children[c]->name ? ib.sch.children[c]->name : "");
            }
        }
    } else {
        // the columns the operator reads must be where -- and what, under the same name -- they were in the first batch (a
        // column of the same type in another layout would otherwise be read in their place)
        auto same = [&](int ci) { return ci < (int)ib.sch.n_children && ci < (int)h->formats.size() && ib.sch.children[ci]->format &&
                                         h->formats[(size_t)ci] == signature(ci) && ib.sch.children[ci]->name &&
                                         h->names[(size_t)ci] == ib.sch.children[ci]->name; };
        for (size_t j = 0; !rc && j < h->key_idx.size(); j++) if (!same(h->key_idx[j])) rc = set_error("vnm_agg_op_next: the batch schema changed");
        for (size_t i = 0; !rc && i < h->funcs.size(); i++) if (h->in_idx[i] >= 0 && !same(h->in_idx[i])) rc = set_error("vnm_agg_op_next: the batch schema changed");
    }
    if (rc) { ib.drop(); return rc; }
    static const int64_t small_rows = getenv("VNM_AGG_COALESCE_BELOW") ? atoll(getenv("VNM_AGG_COALESCE_BELOW")) : (1 << 20);
    static const int64_t flush_rows = getenv("VNM_AGG_COALESCE_ROWS") ? atoll(getenv("VNM_AGG_COALESCE_ROWS")) : (1 << 22);
    if (ib.arr.length < small_rows) {
        h->pending_rows += ib.arr.length;
        h->pending.push_back(std::move(ibp));
        return h->pending_rows >= flush_rows ? agg_op_flush(h) : 0;
    }
    rc = agg_op_flush(h);   // (rows that arrived earlier go first; the order does not matter to the result)
    if (!rc) rc = agg_op_run_batch(h, {&ib.arr}, ib.arr.length);
    ib.drop();
    return rc;
}

int vnm_agg_op_next_stream(vnm_agg_op* h, struct ArrowArrayStream* stream) {
    if (!h || !stream || !stream->get_next) return set_error("vnm_agg_op_next_stream: null argument");
    return drain_stream(stream, "vnm_agg_op_next_stream", [&](struct ArrowArray* a, struct ArrowSchema* sc) { return vnm_agg_op_next(h, a, sc); });
}

int vnm_agg_op_result(vnm_agg_op* h, struct ArrowArray* out, struct ArrowSchema* out_schema) {
    if (!h || !out || !out_schema) return set_error("vnm_agg_op_result: null argument");
    if (!h->inited) return set_error("vnm_agg_op_result: no batch was ever passed to next()");
    VNM_TRY(agg_op_flush(h));
    int64_t n = 0;
    VNM_TRY(vnm_agg_finish(h->dev, &n, nullptr));
    std::vector<std::vector<int32_t>> str_ids;      // per string function: the winning dictionary id of every group (-1 = NULL)
    std::vector<int> strfn_of(h->funcs.size(), -1);
    if (!h->strfns.empty()) {
        VNM_TRY(strmm_fold(h));
        VNM_TRY(strmm_join(h, n, &str_ids));
        for (size_t f = 0; f < h->strfns.size(); f++) strfn_of[(size_t)h->strfns[f].op_idx] = (int)f;
    }
    const int64_t ncols = (int64_t)h->agg_cols.size() + (int64_t)h->funcs.size();
    make_struct(out, n, ncols);
    make_schema(out_schema, "+s", "", ncols);
    // BaseAggregate::Result on the DEVICE: every column is finalised by a kernel into Arrow-layout buffers and only those
    // cross PCIe (8 bytes per group and column instead of all accumulator words + a serial host loop).  The one case that
    // changes a column's TYPE -- an int64 / uint64 SUM overflowing 64 bits (-> decimal128, agg_funcs.h:366-389) -- makes
    // the kernel return 2 and the whole result falls back to the host finaliser below.
    if (getenv("VNM_AGG_HOST_FINALIZE") == nullptr) {
        void* dv = pool_alloc((size_t)(n ? n : 1) * 8);
        uint8_t* db = (uint8_t*)pool_alloc((size_t)((n + 63) / 64 + 1) * 8);
        if (!dv || !db) return 1;
        int rc = 0, col = 0;
        for (size_t a = 0; !rc && a < h->agg_cols.size(); a++, col++) {
            const int j = h->aggcol_key[a];
            const ColType& t = h->key_t[j];
            int64_t nulls = 0;
            rc = vnm_agg_result_key_device(h->dev, j, dv, db, &nulls, nullptr);
            if (!rc && h->gkeys[j]->d.kind != COL_NUM) {   // the groups' codes -> values of the key column's type
                std::vector<int32_t> codes((size_t)(n ? n : 1));
                std::vector<uint8_t> bm((size_t)((n + 7) / 8 + 8), 0xFF), vb((size_t)(n ? n : 1), 1);
                if (n && hipMemcpy(codes.data(), dv, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = set_error("result: device to host copy failed");
                if (!rc && nulls && hipMemcpy(bm.data(), db, (size_t)((n + 7) / 8), hipMemcpyDeviceToHost) != hipSuccess) rc = set_error("result: device to host copy failed");
                if (!rc) {
                    if (nulls) for (int64_t r = 0; r < n; r++) vb[(size_t)r] = (bm[(size_t)(r >> 3)] >> (r & 7)) & 1;
                    rc = make_key_column(out->children[col], *h->gkeys[j], n, codes.data(), vb.data());
                }
            } else if (!rc) rc = make_primitive_from_device(out->children[col], n, type_width(t.type), dv, db, nulls);
            make_dict_schema(out_schema->children[col], h->gkeys[j]->d, h->agg_cols[a]);
        }
        for (size_t i = 0; !rc && i < h->funcs.size(); i++, col++) {
            int kind = 0;
            int64_t nulls = 0;
            if (strfn_of[i] >= 0) {
                rc = strmm_column(h, strfn_of[i], n, str_ids[(size_t)strfn_of[i]], h->out_cols[i], out->children[col], out_schema->children[col]);
                continue;
            }
            rc = vnm_agg_result_func_device(h->dev, h->dev_of[i], dv, db, &kind, &nulls, nullptr);
            if (rc) break;
            const std::pair<std::string, int> fw = result_format(h->funcs[i], kind, h->in_t[i]);
            rc = make_primitive_from_device(out->children[col], n, fw.second, dv, db, nulls);
            make_schema(out_schema->children[col], fw.first, h->out_cols[i], 0);
        }
        pool_free(dv); pool_free(db);
        if (rc == 0) return 0;
        release_array(out); release_schema(out_schema);       // rebuilt below
        if (rc != 2) return rc;
        make_struct(out, n, ncols);
        make_schema(out_schema, "+s", "", ncols);
    }
    std::vector<uint64_t> vals((size_t)(n ? n : 1));
    std::vector<uint8_t> valid((size_t)(n ? n : 1));
    std::vector<uint8_t> cells((size_t)(n ? n : 1) * 16);
    int col = 0;
    // group keys that are selected, in agg_cols order (base_aggregate.cpp:99-118, GroupBuilder agg_funcs.h:544-578)
    for (size_t a = 0; a < h->agg_cols.size(); a++, col++) {
        int j = h->aggcol_key[a];
        VNM_TRY(vnm_agg_result_key(h->dev, j, vals.data(), valid.data()));
        const ColType& t = h->key_t[j];
        int w = type_width(t.type);
        if (h->gkeys[j]->d.kind != COL_NUM) {
            std::vector<int32_t> codes((size_t)(n ? n : 1));
            for (int64_t r = 0; r < n; r++) codes[(size_t)r] = (int32_t)vals[(size_t)r];
            VNM_TRY(make_key_column(out->children[col], *h->gkeys[j], n, codes.data(), valid.data()));
            make_dict_schema(out_schema->children[col], h->gkeys[j]->d, h->agg_cols[a]);
            continue;
        }
        std::vector<uint8_t> narrow((size_t)(n ? n : 1) * w);
        for (int64_t r = 0; r < n; r++) memcpy(&narrow[(size_t)r * w], &vals[r], (size_t)w);  // little endian truncation
        make_primitive(out->children[col], n, w, narrow.data(), valid.data());
        make_schema(out_schema->children[col], t.format, h->agg_cols[a], 0);
    }
    for (size_t i = 0; i < h->funcs.size(); i++, col++) {
        int kind = 0;
        if (strfn_of[i] >= 0) {
            VNM_TRY(strmm_column(h, strfn_of[i], n, str_ids[(size_t)strfn_of[i]], h->out_cols[i], out->children[col], out_schema->children[col]));
            continue;
        }
        VNM_TRY(vnm_agg_result_func(h->dev, h->dev_of[i], cells.data(), valid.data(), &kind));
        const ColType& t = h->in_t[i];
        const std::pair<std::string, int> fw = result_format(h->funcs[i], kind, t);
        const int w = fw.second;
        std::vector<uint8_t> buf((size_t)(n ? n : 1) * 16);
        for (int64_t r = 0; r < n; r++) {   // cells hold the value in 16 bytes (MIN / MAX: widened to 64 bits)
            if ((h->funcs[i] == VNM_MIN || h->funcs[i] == VNM_MAX) && t.type == VNM_F32) { double d; memcpy(&d, &cells[(size_t)r * 16], 8); float fl = (float)d; memcpy(&buf[(size_t)r * 4], &fl, 4); }
            else memcpy(&buf[(size_t)r * w], &cells[(size_t)r * 16], (size_t)w);
        }
        make_primitive(out->children[col], n, w, buf.data(), valid.data());
        make_schema(out_schema->children[col], fw.first, h->out_cols[i], 0);
    }
    return 0;
}

}  // extern "C"
