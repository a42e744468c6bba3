// The to_str() formatter (vinum_amd/csrc/vnm_tostr.hpp) on the host, under AddressSanitizer and UBSan: this program includes nothing
// but that header.  argv[1] names a file of lines "<kind> <value>" (the value in decimal: unsigned for TS_UINT, signed otherwise);
// for every line the image is written into a HEAP buffer of exactly ts_room bytes and printed on a line of its own.  The same
// value then goes into a buffer ONE byte short, where ts_write must say -1 and leave the byte behind its room alone (the sanitizer
// sees a store past either buffer).  tests/test_to_str_host_cpu.py holds the output against NumPy's text byte for byte.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../vinum_amd/csrc/vnm_tostr.hpp"

static int fail(const char* what, int kind, long long value) {
    std::fprintf(stderr, "tostr_host: %s (kind %d, value %lld)\n", what, kind, value);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: tostr_host <file of \"kind value\" lines>", -1, 0);
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the input", -1, 0);
    char line[128];
    long long n = 0;
    while (std::fgets(line, sizeof line, f)) {
        char* rest = nullptr;
        const int kind = (int)std::strtol(line, &rest, 10);
        const int64_t value = kind == vnm::TS_UINT ? (int64_t)std::strtoull(rest, nullptr, 10) : (int64_t)std::strtoll(rest, nullptr, 10);
        const int64_t room = vnm::ts_room(kind, value);
        if (room <= 0 || room > vnm::TS_MAX_BYTES) { std::fclose(f); return fail("ts_room outside (0, TS_MAX_BYTES]", kind, value); }
        uint8_t* exact = (uint8_t*)std::malloc((size_t)room);
        if (vnm::ts_write(exact, room, kind, value) != room) { std::fclose(f); return fail("ts_write != ts_room", kind, value); }
        std::fwrite(exact, 1, (size_t)room, stdout);
        std::fputc('\n', stdout);
        // one byte short: -1, what fits is the image's beginning, and the room is the heap block itself
        uint8_t* tight = (uint8_t*)std::malloc((size_t)room - 1 + (room == 1));
        if (vnm::ts_write(tight, room - 1, kind, value) != -1) { std::fclose(f); return fail("a room one byte short was accepted", kind, value); }
        if (room > 1 && std::memcmp(tight, exact, (size_t)room - 1)) { std::fclose(f); return fail("the short room holds other bytes", kind, value); }
        std::free(tight);
        std::free(exact);
        n++;
    }
    std::fclose(f);
    if (vnm::ts_write(nullptr, 4, vnm::TS_NONE, 0) != -1) return fail("a null buffer was accepted", vnm::TS_NONE, 0);
    if (vnm::ts_room(99, 0) != -1) return fail("an unknown kind has a room", 99, 0);
    std::fprintf(stderr, "tostr_host: ok %lld\n", n);
    return 0;
}
