// prune_plan.h — everything of `prune` that needs no device (standard headers only, like merge_match.h): the keys, the window that
// --window-kb implies, the priority, the mask-memory check, and a plain sequential restatement of the greedy set for the tests'
// stand-alone checker (tests/prune_check.cpp, built alone under ASan + UBSan and held against tests/prune_ref.py).
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

namespace pgenhost::prune_plan {

// a POS field: decimal digits only, below 2^32
bool parse_pos(const std::string &text, uint64_t &pos);

// (CHROM rank by first appearance << 32) | POS, one per row; pos == nullptr: POS left out (0)
std::vector<uint64_t> keys(const std::vector<std::string> &chrom, const std::vector<uint64_t> *pos);

// The largest d for which some row i has key[i + d] - key[i] (mod 2^64) <= max_span with rows i .. i + d on one chromosome: the W a
// window in base pairs needs.  The scan behind row i stops at the first row of another chromosome, at the first row of the same
// chromosome that lies past the span in ascending order, or after `cap` rows (0: no cap).  At least 1.
uint32_t window_for_span(const std::vector<uint64_t> &key, uint64_t max_span, uint32_t cap);

// minor-allele frequency among called alleles, mapped monotonically to u32; 0 when nothing is called
uint32_t priority(uint32_t c0, uint32_t c1, uint32_t c2);

// bytes of the two masks of V rows and window W, and whether they take at most half of `free_bytes` (the device's free memory)
uint64_t mask_bytes(uint64_t n_rows, uint32_t window);
bool masks_fit(uint64_t n_rows, uint32_t window, uint64_t free_bytes);

// S from a list of undirected edges (a, b): rows in beating order (higher priority, then lower index); a row with state 1 or 2 keeps
// it; any other is 1 (kept) iff none of its neighbours that beat it is kept, else 2.  priority empty: all equal.
std::vector<uint8_t> resolve(uint64_t n_rows, const std::vector<std::pair<uint64_t, uint64_t>> &edges, const std::vector<uint32_t> &priority,
                             std::vector<uint8_t> state);

}  // namespace pgenhost::prune_plan
