// What the Arrow-level operators (vnm_agg_op.cpp, vnm_sort_op.cpp) share and what needs the device: imported batches, the chunks of
// a column, staging into HBM, and the one reader and the one writer of dictionary-typed columns.  The host-only half is
// vnm_arrow_host.hpp.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "vnm_arrow_host.hpp"
#include "vnm_common.hpp"

namespace vnm {

struct ImportedBatch {
    struct ArrowArray arr;
    struct ArrowSchema sch;
    bool live = false;
    void drop() {
        if (!live) return;
        if (arr.release) arr.release(&arr);
        if (sch.release) sch.release(&sch);
        live = false;
    }
};

inline int find_child(const struct ArrowSchema* s, const std::string& name) {
    for (int64_t i = 0; i < s->n_children; i++)
        if (s->children[i]->name && name == s->children[i]->name) return (int)i;
    return -1;
}

struct ColChunk { const struct ArrowArray* col; int64_t off, len; };   // rows [off, off + len) of a child array
inline const uint8_t* chunk_validity(const ColChunk& c) { return (c.col->null_count != 0 && c.col->n_buffers > 0) ? (const uint8_t*)c.col->buffers[0] : nullptr; }
// child `ci` of struct batches, one chunk per batch
std::vector<ColChunk> chunks_of(const std::vector<const struct ArrowArray*>& batches, int ci);
// the chunks' validity laid end to end on the host (empty: no NULL anywhere) and in HBM (*out null: no NULL anywhere)
std::vector<uint8_t> chunks_validity(const std::vector<ColChunk>& chunks, int64_t total);
int upload_validity(const std::vector<ColChunk>& chunks, int64_t total, uint8_t** out);

// one chunk of a numeric column into HBM, straight from its own buffers (vnm_stage_column)
int stage_child(const ColChunk& c, const ColType& t, vnm_dcol* out, hipStream_t s);
// several chunks of a numeric column -> ONE column in HBM
int stage_children(const std::vector<ColChunk>& chunks, const ColType& t, int64_t total, vnm_dcol* out);

// primitive array whose buffers are filled by D2H copies of device-finalised Arrow buffers (values of `width` bytes + bitmap)
int make_primitive_from_device(struct ArrowArray* a, int64_t n, int width, const void* dev_values, const uint8_t* dev_bitmap, int64_t null_count);

// ---- dictionary-typed columns (dictionary<intN, utf8 / large_utf8 / binary / large_binary>, ColDesc COL_DICT) ------------------------
struct DictReadStats { int64_t values_encoded = 0, dictionaries_skipped = 0; };   // for the callers' route notes
// the values the last vnm_strdict_encode of `dict` added -> values
int append_new_values(vnm_strdict* dict, DictValues* values, int64_t n_new, int64_t new_bytes);
// The column's chunks -> int32 codes of `dict` in HBM (-1: NULL by index or by value) and their validity bitmap (bit i = codes[i]
// >= 0), both pool blocks the caller owns.  `malformed`: the caller's message for a chunk without its dictionary or indices.
int stage_dict_codes(vnm_strdict* dict, DictValues* values, const ColDesc& d, const std::vector<ColChunk>& chunks, int64_t total,
                     const char* malformed, int32_t** codes, uint8_t** validity, DictReadStats* stats);
// codes[rows[i]] (rows null: codes[i]) of n rows -> a dictionary-typed array: indices of the input's width into a dictionary of
// exactly the values these rows use, in id order
int make_dict_array(const int32_t* codes, const int64_t* rows, int64_t n, const ColDesc& d, vnm_strdict* dict, const DictValues& values, struct ArrowArray* out);
// DictValues::make_string_array with its message as the library's error
int make_string_array(const DictValues& values, struct ArrowArray* a, bool wide, const int32_t* want, const uint8_t* valid_bytes, int64_t n, const char* what);

// pulls every batch of an Arrow C stream through `take` (which consumes array and schema); releases the stream
template <class F>
int drain_stream(struct ArrowArrayStream* stream, const char* who, F take) {
    int rc = 0;
    for (;;) {
        struct ArrowArray arr;
        memset(&arr, 0, sizeof(arr));
        if (stream->get_next(stream, &arr) != 0) {
            const char* msg = stream->get_last_error ? stream->get_last_error(stream) : nullptr;
            rc = set_error("%s: the stream failed: %s", who, msg ? msg : "(no message)");
            break;
        }
        if (!arr.release) break;   // end of the stream
        struct ArrowSchema sch;
        memset(&sch, 0, sizeof(sch));
        if (stream->get_schema(stream, &sch) != 0) {
            arr.release(&arr);
            rc = set_error("%s: the stream has no schema", who);
            break;
        }
        rc = take(&arr, &sch);
        if (arr.release) arr.release(&arr);     // (not taken: an error on the way)
        if (sch.release) sch.release(&sch);
        if (rc) break;
    }
    if (stream->release) stream->release(stream);
    return rc;
}

}  // namespace vnm
