// inflate_hostcheck.cpp -- the decoder of csrc/tip_inflate_core.h as plain host C++ under AddressSanitizer and UBSan.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tissue_image_processing_amd/csrc \
//       tools/inflate_hostcheck.cpp -o inflate_hostcheck && ./inflate_hostcheck cases.bin
//
// cases.bin is what tests/inflate_cases.py's dump() writes.  Every case is decoded from a heap copy of its stream of the exact
// length (a read one byte past it trips the sanitizer) into a destination with 64 guard bytes on either side; a valid case
// must give its bytes and status 0, an invalid one its named status.  Then 6000 fixed-seed mutations of the valid streams --
// one byte changed, or the stream cut short -- must each return (any status) with the guards intact.  tests/test_inflate_host.py
// builds and runs this; it never runs on a GPU and loads nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tip_inflate_core.h"

namespace {

constexpr int GUARD = 64;

struct Case {
    int wrapper, status, valid;
    std::vector<uint8_t> stream, expected;
    int64_t dst_len;
};

uint8_t guard_byte(int64_t i) { return (uint8_t)(i * 37 + 11); }

// decodes `stream` (copied to an exactly-sized heap block) and checks the guards; the output is left in `out`
int run_one(const std::vector<uint8_t> &stream, int wrapper, int64_t dst_len, tip_inflate::Tables &T, std::vector<uint8_t> &out, bool *guards_ok)
{
    uint8_t *src = (uint8_t *)malloc(stream.size() ? stream.size() : 1);      // (a 0-byte stream: a 1-byte block that is never read -- src_len 0)
    if (!stream.empty()) memcpy(src, stream.data(), stream.size());
    uint8_t *dst = (uint8_t *)malloc((size_t)dst_len + 2 * GUARD);
    for (int64_t i = 0; i < dst_len + 2 * GUARD; ++i) dst[i] = guard_byte(i);
    const int64_t strip[4] = {0, (int64_t)stream.size(), GUARD, dst_len};
    const int st = tip_inflate::inflate_strip_serial(src, strip, wrapper, dst, T);
    *guards_ok = true;
    for (int64_t i = 0; i < GUARD; ++i)
        if (dst[i] != guard_byte(i) || dst[GUARD + dst_len + i] != guard_byte(GUARD + dst_len + i)) *guards_ok = false;
    out.assign(dst + GUARD, dst + GUARD + dst_len);
    free(dst);
    free(src);
    return st;
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t n = 0;
    if (!read_exact(f, &n, 4) || n < 0 || n > 100000) return 2;
    std::vector<Case> cases((size_t)n);
    for (Case &c : cases) {
        int32_t head[3];
        int64_t lens[2];
        if (!read_exact(f, head, 12) || !read_exact(f, lens, 16) || lens[0] < 0 || lens[1] < 0) return 2;
        c.wrapper = head[0], c.status = head[1], c.valid = head[2], c.dst_len = lens[1];
        c.stream.resize((size_t)lens[0]);
        if (!read_exact(f, c.stream.data(), c.stream.size())) return 2;
        if (c.valid) {
            c.expected.resize((size_t)lens[1]);
            if (!read_exact(f, c.expected.data(), c.expected.size())) return 2;
        }
    }
    fclose(f);

    tip_inflate::Tables T;
    memset(&T, 0, sizeof T);
    std::vector<uint8_t> out;
    int failures = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
        const Case &c = cases[k];
        bool guards = false;
        const int st = run_one(c.stream, c.wrapper, c.dst_len, T, out, &guards);
        const bool ok = guards && st == c.status && (!c.valid || out == c.expected);
        if (!ok) {
            printf("case %zu: status %d (want %d), guards %s%s\n", k, st, c.status, guards ? "intact" : "BROKEN",
                   c.valid && out != c.expected ? ", bytes differ" : "");
            ++failures;
        }
    }
    if (failures) return 1;
    printf("cases %zu ok\n", cases.size());

    // mutations: xorshift64*, fixed seed
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() {
        rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
        return rng * 0x2545F4914F6CDD1Dull;
    };
    std::vector<size_t> valid;
    for (size_t k = 0; k < cases.size(); ++k)
        if (cases[k].valid && !cases[k].stream.empty()) valid.push_back(k);
    if (valid.empty()) return 2;
    const int mutations = 6000;
    int histogram[16] = {0};
    for (int m = 0; m < mutations; ++m) {
        const Case &c = cases[valid[next() % valid.size()]];
        std::vector<uint8_t> s = c.stream;
        // the interesting bytes are the headers and tables at a block's start: half of the mutations land in the first 96 bytes
        const size_t span = (next() & 1) && s.size() > 96 ? 96 : s.size();
        const size_t at = next() % span;
        if (next() % 3 == 0) s.resize(at);                      // cut short
        else s[at] ^= (uint8_t)(1u + next() % 255u);           // one byte changed
        bool guards = false;
        const int st = run_one(s, c.wrapper, c.dst_len, T, out, &guards);
        if (!guards || st < 0 || st > 10) {
            printf("mutation %d: status %d, guards %s\n", m, st, guards ? "intact" : "BROKEN");
            return 1;
        }
        ++histogram[st];
    }
    printf("mutations %d ok; by status:", mutations);
    for (int s = 0; s <= 10; ++s) printf(" %d:%d", s, histogram[s]);
    printf("\n");
    return 0;
}
