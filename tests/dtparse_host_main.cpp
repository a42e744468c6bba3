// The date() / datetime() parser (vinum_amd/csrc/vnm_dtparse.hpp) on the host, under AddressSanitizer and UBSan: this program includes
// nothing but that header.  argv[1] names a file of lines "<unit> <the value's bytes as hex digits, or - for none>"; every value is
// copied into a HEAP buffer of exactly its length before the call (the sanitizer sees a read past either end), and a line
// "<status> <value>" is printed for it.  tests/test_dtparse_host_cpu.py holds the output against NumPy's own parser.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../vinum_amd/csrc/vnm_dtparse.hpp"

static int fail(const char* what, long long line) {
    std::fprintf(stderr, "dtparse_host: %s (line %lld)\n", what, line);
    return 1;
}

static int nibble(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: dtparse_host <file of \"unit hex\" lines>", 0);
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the input", 0);
    char line[512];
    long long n = 0;
    while (std::fgets(line, sizeof line, f)) {
        n++;
        char* rest = nullptr;
        const int unit = (int)std::strtol(line, &rest, 10);
        while (*rest == ' ') rest++;
        size_t hex = 0;
        while (nibble(rest[hex]) >= 0) hex++;
        if (rest[0] == '-') hex = 0;
        else if (hex == 0 || hex % 2) { std::fclose(f); return fail("malformed hex", n); }
        const size_t len = hex / 2;
        uint8_t* exact = (uint8_t*)std::malloc(len ? len : 1);      // (a value of no bytes: the one byte is never the parser's to read)
        if (!exact) { std::fclose(f); return fail("out of memory", n); }
        for (size_t k = 0; k < len; k++) exact[k] = (uint8_t)(nibble(rest[2 * k]) * 16 + nibble(rest[2 * k + 1]));
        int64_t value = 77;
        const int status = vnm::dt_parse(len ? exact : exact + 1, (int64_t)len, unit, &value);
        if (status != vnm::DT_VALUE && value != 0) { std::fclose(f); return fail("a value came out without DT_VALUE", n); }
        std::printf("%d %" PRId64 "\n", status, value);
        std::free(exact);
    }
    std::fclose(f);
    int64_t v = 5;
    if (vnm::dt_parse(nullptr, 4, vnm::DT_S, &v) != vnm::DT_REFUSED) return fail("a null buffer was accepted", 0);
    if (vnm::dt_parse((const uint8_t*)"2020", 4, 9, &v) != vnm::DT_REFUSED) return fail("an unknown unit was accepted", 0);
    if (vnm::dt_parse((const uint8_t*)"2020", -1, vnm::DT_S, &v) != vnm::DT_REFUSED) return fail("a negative length was accepted", 0);
    std::fprintf(stderr, "dtparse_host: ok %lld\n", n);
    return 0;
}
