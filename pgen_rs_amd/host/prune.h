// prune.h — what `prune` (prune.cpp) shares with `export` (commands.cpp): export's body in two halves that take a selection, so
// that `prune --export` writes the variants it kept through export's own path.
#pragma once
#include <string>

#include "host_internal.h"

namespace pgenhost {

// the .pvar / .psam (or .bim / .fam) texts of a selection's kept rows
void export_texts(const Pfile &pf, const Pfile::Selection &sel, const ExportOptions &eopt, std::string &var_text, std::string &sam_text);
// the records of `vars` packed to the kept samples on the device(s) (pgenhip_pack_records) and written as OUT.pgen / .bed, then the texts
void export_records(const Pfile &pf, const Pfile::IdxRecords &vars, const KeptSamples &kept, const std::string &out_prefix, const ExportOptions &eopt,
                    const OutputOptions &opt, OutputStats &st, const std::string &var_text, const std::string &sam_text);
// throws when out_main names the input's own .pgen
void refuse_export_over_input(const Pfile &pf, const std::string &out_main);

}  // namespace pgenhost
