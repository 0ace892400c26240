// merge_match.h — the matching rules of `merge`, pure: which rows of the inputs' .pvar files are one variant, which output rows they
// make and in what order, which parts are flipped or absent there; and the check of the joined .psam rows.  Standard headers only: no
// device, no file, no other project header (tests/merge_check.cpp builds this file alone, under the sanitizers).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace pgenhost::merge {

// every rule's violation; what() names the files and lines
struct MatchError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

constexpr int64_t kAbsent = -1;

// one input's .pvar or .psam: its column-header line and its rows, verbatim without their line ends
struct Table {
    std::string name;                // the file, for messages
    std::string column_line;
    std::vector<std::string> rows;
    std::vector<uint64_t> line_no;   // 1-based line of each row in the file
};

struct Match {
    // per output row: the input and row whose .pvar line is written (the first input, in argument order, that holds the variant)
    std::vector<uint32_t> from_input;
    std::vector<uint64_t> from_row;
    // [input][output row]: the input's row, or kAbsent; whether the input's REF and ALT are exchanged against the output row's
    std::vector<std::vector<int64_t>> src;
    std::vector<std::vector<uint8_t>> flip;
    // per input: output rows flipped, output rows it lacks, rows of it in no output row
    std::vector<uint64_t> flipped, absent, dropped;
    uint64_t id_conflicts = 0;       // (output row, later input that holds it) pairs whose ID differs from the row written
};

// A variant's key is (CHROM, POS, {REF, ALT}): strings compared verbatim, the allele pair unordered.  Default: the intersection, in
// the first input's order.  with_union: every variant of any input, stably sorted by (rank of CHROM by first appearance scanning the
// inputs in argument order and rows in file order, POS as an unsigned integer, first-seen order).  Throws MatchError for column
// lines that differ, a column line without CHROM / POS / ID / REF / ALT, a row with too few fields, two rows of one input with one
// key, and (union) a POS that is not an unsigned integer.  Strand flips (A/G against T/C) are not detected.
Match match_variants(const std::vector<Table> &pvars, bool with_union);

// The .psam column lines must be byte-identical; the first column named IID (a leading '#' on the line dropped) must not hold one
// value twice over all inputs.  Throws MatchError naming the IID and both files.
void check_samples(const std::vector<Table> &psams);

// the fields of a tab-separated line
std::vector<std::string> split_tabs(const std::string &line);

}  // namespace pgenhost::merge
