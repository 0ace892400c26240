// fuzz_vcf.cpp — pgenhip_vcf_index_lines against a naive walk, built by tests/test_parse_gt.py with g++ -fsanitize=address,undefined
// together with pgen_rs_amd/csrc/host_pure.cpp (the same source libpgen_hip.so is built from).  The function indexes bytes that come
// straight from a file: on random soups of tabs, newlines, carriage returns and digits, in allocations of exactly the text's and the
// arrays' size (ASan sees any access outside them), it must report what a byte-by-byte walk reports.
//   usage: fuzz_vcf <iterations> <rng seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/pgen_hip.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = rng_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Line {
    uint64_t start, format, field, end;
};

// byte by byte: columns counted as the tabs go by
static std::vector<Line> naive(const std::vector<uint8_t> &t, uint32_t format_col, uint64_t max_lines, bool last_block, uint64_t &consumed)
{
    std::vector<Line> out;
    uint64_t pos = 0;
    consumed = 0;
    while (out.size() < max_lines && pos < t.size()) {
        uint64_t stop = pos;
        while (stop < t.size() && t[stop] != '\n') stop++;
        if (stop == t.size() && !last_block) break;
        const uint64_t end = stop < t.size() && stop > pos && t[stop - 1] == '\r' ? stop - 1 : stop;
        Line l{pos, UINT64_MAX, UINT64_MAX, end};
        uint32_t col = 0;
        if (format_col == 0) l.format = pos;
        for (uint64_t i = pos; i < end; i++) {
            if (t[i] != '\t') continue;
            if (col == format_col) {
                l.field = i;
                break;
            }
            col++;
            if (col == format_col) l.format = i + 1;
        }
        if (l.format != UINT64_MAX && l.field == UINT64_MAX) l.field = end;
        out.push_back(l);
        pos = stop < t.size() ? stop + 1 : t.size();
        consumed = pos;
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long iters = std::atol(argv[1]);
    rng_state = std::strtoull(argv[2], nullptr, 10);
    static const uint8_t kAlphabet[] = {'\t', '\t', '\t', '\n', '\n', '\r', '0', '1', '/', '.'};
    long lines = 0, short_lines = 0;
    for (long it = 0; it < iters; it++) {
        const size_t len = (size_t)(rnd() % 97);
        std::vector<uint8_t> text(len);   // own allocation of exactly len bytes
        for (auto &b : text) b = kAlphabet[rnd() % sizeof(kAlphabet)];
        const uint32_t format_col = (uint32_t)(rnd() % 11);
        const bool last_block = rnd() & 1;
        const uint64_t max_lines = rnd() % 4 == 0 ? rnd() % 5 : len + 1;
        std::vector<uint64_t> a(max_lines), b(max_lines), c(max_lines), d(max_lines);
        uint64_t n = ~0ull, consumed = ~0ull;
        const int rc = pgenhip_vcf_index_lines(len ? text.data() : nullptr, len, format_col, max_lines, last_block ? PGENHIP_VCF_LAST_BLOCK : 0u,
                                               a.data(), b.data(), c.data(), d.data(), &n, &consumed);
        if (rc != PGENHIP_OK && !(max_lines == 0)) {
            std::fprintf(stderr, "iteration %ld: status %d\n", it, rc);
            return 1;
        }
        if (rc != PGENHIP_OK) continue;
        uint64_t want_consumed;
        const std::vector<Line> want = naive(text, format_col, max_lines, last_block, want_consumed);
        bool same = n == want.size() && consumed == want_consumed;
        for (size_t i = 0; same && i < want.size(); i++)
            same = a[i] == want[i].start && b[i] == want[i].format && c[i] == want[i].field && d[i] == want[i].end;
        if (!same) {
            std::fprintf(stderr, "iteration %ld: differs from the naive walk (len %zu, format_col %u, last_block %d, max_lines %llu)\n", it, len, format_col,
                         (int)last_block, (unsigned long long)max_lines);
            return 1;
        }
        lines += (long)n;
        for (size_t i = 0; i < want.size(); i++) short_lines += want[i].field == UINT64_MAX;
    }
    std::printf("fuzz_vcf: %ld iterations: %ld lines indexed, %ld with too few columns\n", iters, lines, short_lines);
    return 0;
}
