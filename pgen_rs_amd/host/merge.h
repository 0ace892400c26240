// merge.h — `merge`: two to eight filesets' samples side by side in one fileset.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pfile.h"

namespace pgenhost {

struct MergeOptions {
    bool with_union = false;   // --union: every variant of any input (a part that lacks a row is missing there) instead of the intersection
    bool dry_run = false;      // --dry-run: the whole selection and matching, no device, no file
};

struct MergeStats {
    uint64_t inputs = 0, samples = 0, variants = 0, id_conflicts = 0, file_bytes = 0;
    std::vector<uint64_t> flipped, absent, dropped;   // per input: output rows flipped, output rows it lacks, rows of it in no output row
    double seconds_filter = 0, seconds_body = 0, seconds_setup = 0, seconds_kernel = 0;
    // `"inputs": 2, "samples": .., "variants": .., "flipped": [..], "absent": [..], "dropped": [..], "id_conflicts": ..`
    std::string json_counts() const;
};

// The inputs (each fixed-width, or variable-width with plain records) joined into OUT_PREFIX.pgen (fixed-width, storage mode 0x02),
// .pvar (the first input's header lines, then per output row the verbatim row of the first input, in argument order, that holds the
// variant) and .psam (the first input's bytes up to and including its column line, then every input's rows in argument order).
// Samples: the .psam column lines must be byte-identical and no IID may occur twice.  Variants: merge_match.h's rules (key (CHROM,
// POS, {REF, ALT}); intersection in the first input's order, or the sorted union; an input whose REF and ALT are exchanged is flipped,
// codes 0 and 2 exchanged; strand flips are not detected).  Per block of output rows each input's records are staged with one pread
// per run of neighbouring records, pgenhip_join_records joins them on device 0 and the rows are written with pwrite at 12 + j*R.
// OUT_PREFIX naming an input's own .pgen is refused before anything is opened for writing; any error leaves no output file; no
// device is an error before any file exists.  Uses block_text_bytes (record bytes per block, inputs and output) and read_threads.
MergeStats merge_pfiles(const std::vector<std::string> &prefixes, const std::string &out_prefix, const MergeOptions &mopt, const OutputOptions &opt = OutputOptions());

}  // namespace pgenhost
