// prune_plan.cpp — `prune` without a device (prune_plan.h)
#include "prune_plan.h"

#include <algorithm>
#include <numeric>
#include <unordered_map>

namespace pgenhost::prune_plan {

bool parse_pos(const std::string &text, uint64_t &pos)
{
    if (text.empty() || text.size() > 10) return false;
    uint64_t v = 0;
    for (const char c : text) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (uint64_t)(c - '0');
    }
    if (v > 0xFFFFFFFFull) return false;
    pos = v;
    return true;
}

std::vector<uint64_t> keys(const std::vector<std::string> &chrom, const std::vector<uint64_t> *pos)
{
    std::unordered_map<std::string, uint64_t> rank;
    std::vector<uint64_t> out(chrom.size());
    for (size_t r = 0; r < chrom.size(); r++) {
        const uint64_t c = rank.emplace(chrom[r], (uint64_t)rank.size()).first->second;
        out[r] = (c << 32) | (pos ? (*pos)[r] : 0u);
    }
    return out;
}

uint32_t window_for_span(const std::vector<uint64_t> &key, uint64_t max_span, uint32_t cap)
{
    uint64_t w = 1;
    const size_t n = key.size();
    for (size_t i = 0; i < n; i++) {
        for (size_t j = i + 1; j < n && (cap == 0 || j - i <= cap); j++) {
            if ((key[j] >> 32) != (key[i] >> 32)) break;
            if (key[j] - key[i] <= max_span)
                w = std::max<uint64_t>(w, j - i);
            else if (key[j] > key[i])
                break;   // past the span in ascending order (a row that lies before row i is skipped: it is never an edge)
        }
    }
    return (uint32_t)std::min<uint64_t>(w, 0xFFFFFFFFull);
}

uint32_t priority(uint32_t c0, uint32_t c1, uint32_t c2)
{
    const uint64_t called = (uint64_t)c0 + c1 + c2;
    if (called == 0) return 0u;
    const uint64_t alt = (uint64_t)c1 + 2ull * c2;
    const double maf = (double)std::min(alt, 2 * called - alt) / (double)(2 * called);
    return (uint32_t)(maf * 4294967294.0);
}

uint64_t mask_bytes(uint64_t n_rows, uint32_t window) { return 2ull * n_rows * (((uint64_t)window + 31u) / 32u) * 4ull; }

bool masks_fit(uint64_t n_rows, uint32_t window, uint64_t free_bytes) { return mask_bytes(n_rows, window) <= free_bytes / 2u; }

std::vector<uint8_t> resolve(uint64_t n_rows, const std::vector<std::pair<uint64_t, uint64_t>> &edges, const std::vector<uint32_t> &priority,
                             std::vector<uint8_t> state)
{
    state.resize((size_t)n_rows, 0u);
    std::vector<std::vector<uint64_t>> adj((size_t)n_rows);
    for (const auto &e : edges) {
        if (e.first >= n_rows || e.second >= n_rows) continue;
        adj[(size_t)e.first].push_back(e.second);
        adj[(size_t)e.second].push_back(e.first);
    }
    std::vector<uint64_t> order((size_t)n_rows);
    std::iota(order.begin(), order.end(), 0ull);
    if (!priority.empty())
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return priority[(size_t)a] > priority[(size_t)b]; });
    std::vector<uint64_t> rank((size_t)n_rows);
    for (size_t k = 0; k < order.size(); k++) rank[(size_t)order[k]] = k;
    for (const uint64_t v : order) {
        if (state[(size_t)v] == 1u || state[(size_t)v] == 2u) continue;
        bool beaten = false;
        for (const uint64_t u : adj[(size_t)v]) beaten = beaten || (rank[(size_t)u] < rank[(size_t)v] && state[(size_t)u] == 1u);
        state[(size_t)v] = beaten ? 2u : 1u;
    }
    return state;
}

}  // namespace pgenhost::prune_plan
