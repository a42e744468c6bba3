// The host helpers of the Arrow-level operators (vinum_amd/csrc/vnm_arrow_host.hpp) on their own: built with AddressSanitizer and
// UBSan by tests/test_arrow_host_cpu.py and run as a child process, no GPU and no library.  Exits non-zero at the first mismatch.
#include "../vinum_amd/csrc/vnm_arrow_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace vnm;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);      \
            fprintf(stderr, __VA_ARGS__);                                   \
            fprintf(stderr, "\n");                                          \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static bool bit(const uint8_t* p, int64_t i) { return (p[i >> 3] >> (i & 7)) & 1; }
static const int64_t LENGTHS[] = {0, 1, 7, 8, 9, 63, 64, 65, 200};

// copy_bits / set_bits at every pair of offsets: the source holds exactly the bytes the bits need, so one byte read past them is
// reported; the destination is sized as the callers size theirs ((total + 7) / 8 + 8, zeroed)
static void check_copy_and_set_bits() {
    for (int64_t so = 0; so < 16; so++) for (int64_t dof = 0; dof < 16; dof++) for (int64_t n : LENGTHS) {
        const size_t src_bytes = (size_t)(so + n + 7) / 8, dst_bytes = (size_t)(dof + n + 7) / 8 + 8;
        uint8_t* src = (uint8_t*)malloc(src_bytes);
        for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)rnd();
        uint8_t* dst = (uint8_t*)calloc(dst_bytes, 1);
        copy_bits(dst, dof, src, so, n);
        for (int64_t i = 0; i < (int64_t)dst_bytes * 8; i++) {
            const bool want = i >= dof && i < dof + n && bit(src, so + (i - dof));
            CHECK(bit(dst, i) == want, "copy_bits src_off=%lld dst_off=%lld n=%lld bit %lld", (long long)so, (long long)dof, (long long)n, (long long)i);
        }
        memset(dst, 0, dst_bytes);
        set_bits(dst, dof, n);
        for (int64_t i = 0; i < (int64_t)dst_bytes * 8; i++)
            CHECK(bit(dst, i) == (i >= dof && i < dof + n), "set_bits dst_off=%lld n=%lld bit %lld", (long long)dof, (long long)n, (long long)i);
        free(src); free(dst);
    }
}

static void check_join_validity() {
    // four chunks of 0, 13, 8 and 1 rows: a bitmap nobody reads, a bitmap from bit 3, no bitmap (all valid), a bitmap from bit 9
    const int64_t lens[4] = {0, 13, 8, 1}, offs[4] = {5, 3, 2, 9};
    uint8_t b0[1] = {0xA5}, b1[2] = {0x5B, 0xC6}, b3[2] = {0xFF, 0xFD};   // (b3: bit 9 is clear -> the last row is NULL)
    const uint8_t* maps[4] = {b0, b1, nullptr, b3};
    std::vector<BitRun> runs;
    std::vector<bool> want;
    for (int c = 0; c < 4; c++) {
        runs.push_back(BitRun{maps[c], offs[c], lens[c]});
        for (int64_t i = 0; i < lens[c]; i++) want.push_back(!maps[c] || bit(maps[c], offs[c] + i));
    }
    const std::vector<uint8_t> got = join_validity(runs, 22);
    CHECK(got.size() == (22 + 7) / 8 + 8, "join_validity: %zu bytes", got.size());
    for (int64_t i = 0; i < (int64_t)got.size() * 8; i++) CHECK(bit(got.data(), i) == (i < 22 && want[(size_t)i]), "join_validity bit %lld", (long long)i);
    CHECK(!want[21] && want[13], "the table above lost its NULL");
    for (auto& r : runs) r.bits = nullptr;
    CHECK(join_validity(runs, 22).empty(), "join_validity: no chunk has a bitmap, yet NULLs are reported");
    CHECK(join_validity({}, 0).empty(), "join_validity: no rows");
}

struct Want { const char* format; const char* dict; bool ordered; ColKind kind; int type; bool wide; const char* signature; };
static void check_describe_column() {
    const Want table[] = {
        {"c", nullptr, false, COL_NUM, VNM_I8, false, "c"},         {"C", nullptr, false, COL_NUM, VNM_U8, false, "C"},
        {"s", nullptr, false, COL_NUM, VNM_I16, false, "s"},        {"S", nullptr, false, COL_NUM, VNM_U16, false, "S"},
        {"i", nullptr, false, COL_NUM, VNM_I32, false, "i"},        {"I", nullptr, false, COL_NUM, VNM_U32, false, "I"},
        {"l", nullptr, false, COL_NUM, VNM_I64, false, "l"},        {"L", nullptr, false, COL_NUM, VNM_U64, false, "L"},
        {"f", nullptr, false, COL_NUM, VNM_F32, false, "f"},        {"g", nullptr, false, COL_NUM, VNM_F64, false, "g"},
        {"tdD", nullptr, false, COL_NUM, VNM_I32, false, "tdD"},    {"tdm", nullptr, false, COL_NUM, VNM_I64, false, "tdm"},
        {"tts", nullptr, false, COL_NUM, VNM_I32, false, "tts"},    {"ttu", nullptr, false, COL_NUM, VNM_I64, false, "ttu"},
        {"tsu:UTC", nullptr, false, COL_NUM, VNM_I64, false, "tsu:UTC"}, {"tDn", nullptr, false, COL_NUM, VNM_I64, false, "tDn"},
        {"u", nullptr, false, COL_STR, -1, false, "u"},             {"U", nullptr, false, COL_STR, -1, true, "U"},
        {"z", nullptr, false, COL_STR, -1, false, "z"},             {"Z", nullptr, false, COL_STR, -1, true, "Z"},
        {"b", nullptr, false, COL_BOOL, -1, false, "b"},
        {"d:10,2", nullptr, false, COL_DEC, -1, false, "d:10,2"},   {"d:10,2,128", nullptr, false, COL_DEC, -1, false, "d:10,2,128"},
        {"d:10,2,256", nullptr, false, COL_NONE, -1, false, "d:10,2,256"}, {"+s", nullptr, false, COL_NONE, -1, false, "+s"},
        // dictionary children: index format -> value format
        {"i", "u", false, COL_DICT, VNM_I32, false, "i|u"},         {"i", "u", true, COL_DICT, VNM_I32, false, "i|u|ordered"},
        {"c", "Z", false, COL_DICT, VNM_I8, true, "c|Z"},           {"c", "Z", true, COL_DICT, VNM_I8, true, "c|Z|ordered"},
        {"l", "l", false, COL_NONE, -1, false, "l|l"},              {"l", "l", true, COL_NONE, -1, false, "l|l|ordered"},
        {"u", "u", false, COL_NONE, -1, false, "u|u"},              {"u", "u", true, COL_NONE, -1, false, "u|u|ordered"},
    };
    for (const Want& w : table) for (DecimalRule rule : {DECIMAL_128_ONLY, DECIMAL_ANY_COMMA_128}) {
        struct ArrowSchema s, d;
        make_schema(&s, w.format, "x", 0);
        if (w.dict) { make_schema(&d, w.dict, "", 0); s.dictionary = &d; }
        if (w.ordered) s.flags |= 1;
        const ColDesc c = describe_column(&s, rule);
        CHECK(c.kind == w.kind && c.t.type == w.type && c.wide == w.wide && c.signature() == w.signature && c.t.format == w.format &&
              c.has_dictionary == (w.dict != nullptr) && c.ordered == (w.dict && w.ordered) && c.value_format == (w.dict ? w.dict : ""),
              "describe_column(%s -> %s%s): kind %d type %d wide %d signature %s", w.format, w.dict ? w.dict : "-", w.ordered ? ", ordered" : "",
              (int)c.kind, c.t.type, (int)c.wide, c.signature().c_str());
        s.dictionary = nullptr;      // (d is a local, not the calloc'ed child release_schema frees)
        if (w.dict) d.release(&d);
        s.release(&s);
    }
    // the one format on which the operators' decimal rules part: decimal256 with scale 128
    struct ArrowSchema s;
    make_schema(&s, "d:76,128,256", "x", 0);
    CHECK(describe_column(&s, DECIMAL_128_ONLY).kind == COL_NONE && describe_column(&s, DECIMAL_ANY_COMMA_128).kind == COL_DEC, "the decimal rules");
    s.release(&s);
    // what a later batch must not turn into
    std::vector<std::string> sigs;
    const char* pairs[4][2] = {{"i", "u"}, {"i", "U"}, {"i", "u"}, {"i", nullptr}};
    for (int k = 0; k < 4; k++) {
        struct ArrowSchema a;
        make_schema(&a, pairs[k][0], "x", 0);
        if (pairs[k][1]) { a.dictionary = (struct ArrowSchema*)calloc(1, sizeof(struct ArrowSchema)); make_schema(a.dictionary, pairs[k][1], "", 0); }
        if (k == 2) a.flags |= 1;
        sigs.push_back(describe_column(&a, DECIMAL_128_ONLY).signature());
        a.release(&a);
    }
    for (int x = 0; x < 4; x++) for (int y = x + 1; y < 4; y++) CHECK(sigs[x] != sigs[y], "signatures %d and %d are both %s", x, y, sigs[x].c_str());
}

static void append(DictValues* v, const std::vector<int32_t>& ids, const std::vector<std::string>& words) {
    std::string all;
    for (auto& w : words) all += w;
    const int rc = v->append_new((int64_t)ids.size(), (int64_t)all.size(), [&](int32_t* out_ids, int32_t* lens, uint8_t* bytes) {
        for (size_t i = 0; i < ids.size(); i++) { out_ids[i] = ids[i]; lens[i] = (int32_t)words[i].size(); }
        if (!all.empty()) memcpy(bytes, all.data(), all.size());
        return 0;
    });
    CHECK(rc == 0, "append_new");
}
template <class Off>
static void expect_strings(const struct ArrowArray& a, const std::vector<const char*>& want, const char* what) {   // nullptr: NULL
    CHECK(a.length == (int64_t)want.size() && a.n_buffers == 3 && a.buffers[1] && a.buffers[2], "%s: shape", what);
    const Off* off = (const Off*)a.buffers[1];
    const char* data = (const char*)a.buffers[2];
    int64_t nulls = 0;
    CHECK(off[0] == 0, "%s: first offset", what);
    for (size_t i = 0; i < want.size(); i++) {
        const bool valid = !a.buffers[0] || bit((const uint8_t*)a.buffers[0], (int64_t)i);
        CHECK(valid == (want[i] != nullptr), "%s: row %zu validity", what, i);
        const std::string got(data + off[i], (size_t)(off[i + 1] - off[i]));
        CHECK(got == (want[i] ? want[i] : ""), "%s: row %zu is '%s'", what, i, got.c_str());
        nulls += !valid;
    }
    CHECK(a.null_count == nulls && (nulls > 0) == (a.buffers[0] != nullptr), "%s: null_count %lld", what, (long long)a.null_count);
}
static void check_dict_values() {
    DictValues v;
    int failed = v.append_new(2, 3, [](int32_t*, int32_t*, uint8_t*) { return 7; });     // a fetch that fails appends nothing
    CHECK(failed == 7 && v.ids.empty() && v.bytes.empty() && v.off.size() == 1, "append_new after a failed fetch");
    append(&v, {5, 2}, {"ab", ""});        // ids come in chunks: out of order, with gaps
    append(&v, {9}, {"xyz"});
    append(&v, {}, {});
    append(&v, {0, 7}, {"q", "rs"});
    CHECK(v.top == 10 && v.ids.size() == 5 && v.off.back() == 8, "the store after three rounds");
    struct ArrowArray a;
    const int32_t ascending[] = {0, 2, 5, 7, 9};
    std::string msg = v.make_string_array(&a, false, ascending, nullptr, 5, "a result dictionary");
    CHECK(msg.empty(), "%s", msg.c_str());
    expect_strings<int32_t>(a, {"q", "", "ab", "rs", "xyz"}, "ascending ids, 32-bit offsets");
    a.release(&a);
    msg = v.make_string_array(&a, true, ascending, nullptr, 5, "a result dictionary");
    CHECK(msg.empty(), "%s", msg.c_str());
    expect_strings<int64_t>(a, {"q", "", "ab", "rs", "xyz"}, "ascending ids, 64-bit offsets");
    a.release(&a);
    const int32_t repeating[] = {5, -1, 5, 2, 9, 0};
    const uint8_t valid[] = {1, 1, 0, 1, 1, 1};
    msg = v.make_string_array(&a, false, repeating, valid, 6, "a result column");
    CHECK(msg.empty(), "%s", msg.c_str());
    expect_strings<int32_t>(a, {"ab", nullptr, nullptr, "", "xyz", "q"}, "repeating ids with NULLs");
    CHECK(a.null_count == 2 && ((const uint8_t*)a.buffers[0])[0] == 0x39, "repeating ids with NULLs: the bitmap");
    a.release(&a);
    for (int32_t never : {3, 10, 1 << 30}) {
        memset(&a, 0, sizeof(a));
        msg = v.make_string_array(&a, false, &never, nullptr, 1, "a result dictionary");
        CHECK(!msg.empty() && msg.find("a result dictionary names id") == 0 && !a.release, "id %d was never appended: '%s'", never, msg.c_str());
    }
    msg = v.make_string_array(&a, false, nullptr, nullptr, 0, "a result dictionary");
    CHECK(msg.empty(), "%s", msg.c_str());
    expect_strings<int32_t>(a, {}, "n = 0");
    a.release(&a);
    msg = DictValues().make_string_array(&a, true, nullptr, nullptr, 0, "a result dictionary");
    CHECK(msg.empty(), "%s", msg.c_str());
    expect_strings<int64_t>(a, {}, "n = 0 of an empty store");
    a.release(&a);
}

static void check_primitive_and_pack_bits() {
    for (int64_t n : {0, 1, 8, 9}) {
        std::vector<int32_t> values((size_t)(n ? n : 1));
        std::vector<uint8_t> valid((size_t)(n ? n : 1));
        int64_t want_nulls = 0;
        for (int64_t i = 0; i < n; i++) { values[(size_t)i] = (int32_t)(100 + i); valid[(size_t)i] = i % 3 != 0; want_nulls += !valid[(size_t)i]; }
        int64_t zeros = -1;
        uint8_t* bm = pack_bits(valid.data(), n, &zeros);
        CHECK(zeros == want_nulls, "pack_bits n=%lld: %lld zeros", (long long)n, (long long)zeros);
        for (int64_t i = 0; i < ((n + 7) / 8) * 8; i++) CHECK(bit(bm, i) == (i < n && valid[(size_t)i]), "pack_bits n=%lld bit %lld", (long long)n, (long long)i);
        free(bm);
        struct ArrowArray a;
        make_primitive(&a, n, 4, values.data(), valid.data());
        CHECK(a.length == n && a.null_count == want_nulls && (a.buffers[0] != nullptr) == (want_nulls > 0), "make_primitive n=%lld: null_count %lld", (long long)n, (long long)a.null_count);
        for (int64_t i = 0; i < n; i++) CHECK(((const int32_t*)a.buffers[1])[i] == 100 + i && bit((const uint8_t*)a.buffers[0], i) == (valid[(size_t)i] != 0), "make_primitive n=%lld row %lld", (long long)n, (long long)i);
        a.release(&a);
        make_primitive(&a, n, 4, values.data(), nullptr);
        CHECK(a.null_count == 0 && !a.buffers[0], "make_primitive without validity");
        a.release(&a);
    }
    // a struct over a dictionary-typed child leaves through one release
    struct ArrowArray st;
    struct ArrowSchema ss;
    make_struct(&st, 3, 2);
    make_schema(&ss, "+s", "", 2);
    const int32_t idx[3] = {0, 1, 0};
    for (int c = 0; c < 2; c++) make_primitive(st.children[c], 3, 4, idx, nullptr);
    DictValues v;
    append(&v, {1, 0}, {"no", "yes"});
    st.children[1]->dictionary = (struct ArrowArray*)calloc(1, sizeof(struct ArrowArray));
    const int32_t both[2] = {0, 1};
    CHECK(v.make_string_array(st.children[1]->dictionary, false, both, nullptr, 2, "a result dictionary").empty(), "the dictionary of a struct child");
    ColDesc d;
    d.kind = COL_DICT; d.t = parse_format("i"); d.has_dictionary = true; d.value_format = "u"; d.ordered = true;
    make_schema(ss.children[0], "i", "k", 0);
    make_dict_schema(ss.children[1], d, "c");
    CHECK(ss.children[1]->dictionary && std::string(ss.children[1]->dictionary->format) == "u" && (ss.children[1]->flags & 1) && std::string(ss.children[1]->format) == "i", "make_dict_schema");
    CHECK(describe_column(ss.children[1], DECIMAL_128_ONLY).signature() == d.signature(), "make_dict_schema and describe_column disagree");
    st.release(&st);
    ss.release(&ss);
    CHECK(!st.release && !ss.release, "release leaves its mark");
}

int main() {
    check_copy_and_set_bits();
    check_join_validity();
    check_describe_column();
    check_dict_values();
    check_primitive_and_pack_bits();
    printf("arrow_host: ok\n");
    return 0;
}
