// prune_check.cpp — host/prune_plan.cpp alone behind a small text protocol, for tests/test_prune_host.py: built from this file and
// prune_plan.cpp only (the proof that it needs no device and no other host source) under ASan + UBSan, and held against
// tests/prune_ref.py.  Reads one case from stdin, prints one value per line.
//   keys <with_pos> <n>, then n lines "<chrom> <pos>"                      -> n keys
//   window <max_span> <cap> <n>, then n keys                                 -> W
//   priority <n>, then n lines "<c0> <c1> <c2>"                            -> n priorities
//   pos <n>, then n tokens (a '-' stands for the empty string)              -> n lines "<ok> <value>"
//   masks <n_rows> <window> <free_bytes>                                     -> mask_bytes, fits
//   resolve <n> <m> <with_priority>, m lines "<a> <b>", [n priorities], n states -> n states
#include <iostream>
#include <string>

#include "../pgen_rs_amd/host/prune_plan.h"

namespace P = pgenhost::prune_plan;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const std::string mode = argv[1];
    if (mode == "keys") {
        int with_pos;
        size_t n;
        std::cin >> with_pos >> n;
        std::vector<std::string> chrom(n);
        std::vector<uint64_t> pos(n);
        for (size_t i = 0; i < n; i++) std::cin >> chrom[i] >> pos[i];
        for (const uint64_t k : P::keys(chrom, with_pos ? &pos : nullptr)) std::cout << k << "\n";
    } else if (mode == "window") {
        uint64_t span;
        uint32_t cap;
        size_t n;
        std::cin >> span >> cap >> n;
        std::vector<uint64_t> key(n);
        for (auto &k : key) std::cin >> k;
        std::cout << P::window_for_span(key, span, cap) << "\n";
    } else if (mode == "priority") {
        size_t n;
        std::cin >> n;
        for (size_t i = 0; i < n; i++) {
            uint32_t c0, c1, c2;
            std::cin >> c0 >> c1 >> c2;
            std::cout << P::priority(c0, c1, c2) << "\n";
        }
    } else if (mode == "pos") {
        size_t n;
        std::cin >> n;
        for (size_t i = 0; i < n; i++) {
            std::string t;
            std::cin >> t;
            uint64_t v = 0;
            const bool ok = P::parse_pos(t == "-" ? std::string() : t, v);
            std::cout << (ok ? 1 : 0) << " " << v << "\n";
        }
    } else if (mode == "masks") {
        uint64_t n, free_bytes;
        uint32_t w;
        std::cin >> n >> w >> free_bytes;
        std::cout << P::mask_bytes(n, w) << "\n" << (P::masks_fit(n, w, free_bytes) ? 1 : 0) << "\n";
    } else if (mode == "resolve") {
        uint64_t n, m;
        int with_priority;
        std::cin >> n >> m >> with_priority;
        std::vector<std::pair<uint64_t, uint64_t>> edges(m);
        for (auto &e : edges) std::cin >> e.first >> e.second;
        std::vector<uint32_t> prio(with_priority ? n : 0);
        for (auto &p : prio) std::cin >> p;
        std::vector<uint8_t> state(n);
        for (auto &s : state) {
            int v;
            std::cin >> v;
            s = (uint8_t)v;
        }
        for (const uint8_t s : P::resolve(n, edges, prio, state)) std::cout << (int)s << "\n";
    } else {
        return 2;
    }
    return std::cin.fail() ? 3 : 0;
}
