// merge_match.cpp — the matching rules of `merge` (merge_match.h): pure, standard headers only.
#include "merge_match.h"

#include <algorithm>
#include <unordered_map>

namespace pgenhost::merge {

std::vector<std::string> split_tabs(const std::string &line)
{
    std::vector<std::string> out;
    for (size_t b = 0;;) {
        const size_t e = line.find('\t', b);
        out.push_back(line.substr(b, e == std::string::npos ? e : e - b));
        if (e == std::string::npos) break;
        b = e + 1;
    }
    return out;
}

namespace {

// index of the first column named `name` (a leading '#' on the line does not count), or throws
size_t column_of(const std::vector<std::string> &names, const char *name, const std::string &file)
{
    for (size_t c = 0; c < names.size(); c++)
        if (names[c] == name) return c;
    throw MatchError(std::string(name) + " not among the headers of " + file);
}

std::vector<std::string> column_names(const std::string &column_line)
{
    return split_tabs(!column_line.empty() && column_line[0] == '#' ? column_line.substr(1) : column_line);
}

void same_column_lines(const std::vector<Table> &tables, const char *kind)
{
    for (size_t p = 1; p < tables.size(); p++)
        if (tables[p].column_line != tables[0].column_line)
            throw MatchError(std::string("the ") + kind + " column lines of " + tables[0].name + " and " + tables[p].name +
                             " differ (harmonising columns is not built)");
}

bool parse_u64(const std::string &s, uint64_t &v)
{
    if (s.empty()) return false;
    v = 0;
    for (const char c : s) {
        if (c < '0' || c > '9') return false;
        const uint64_t d = (uint64_t)(c - '0');
        if (v > (UINT64_MAX - d) / 10u) return false;
        v = v * 10u + d;
    }
    return true;
}

struct Variant {
    uint32_t first_input;
    uint64_t first_row;
    std::string ref, id;
    uint64_t chrom_rank = 0, pos = 0;
    uint32_t holders = 0;
    std::vector<int64_t> row;     // per input
    std::vector<uint8_t> flip;
};

}  // namespace

Match match_variants(const std::vector<Table> &pvars, bool with_union)
{
    const size_t P = pvars.size();
    Match m;
    m.src.resize(P), m.flip.resize(P);
    m.flipped.assign(P, 0), m.absent.assign(P, 0), m.dropped.assign(P, 0);
    if (P == 0) return m;
    same_column_lines(pvars, ".pvar");
    const std::vector<std::string> names = column_names(pvars[0].column_line);
    const std::string &f0 = pvars[0].name;
    const size_t c_chrom = column_of(names, "CHROM", f0), c_pos = column_of(names, "POS", f0), c_id = column_of(names, "ID", f0),
                 c_ref = column_of(names, "REF", f0), c_alt = column_of(names, "ALT", f0);
    const size_t need = std::max({c_chrom, c_pos, c_id, c_ref, c_alt}) + 1;

    std::vector<Variant> variants;   // in first-seen order
    std::unordered_map<std::string, size_t> by_key;
    std::unordered_map<std::string, uint64_t> chrom_rank;
    for (size_t p = 0; p < P; p++) {
        const Table &t = pvars[p];
        std::unordered_map<size_t, uint64_t> seen_here;   // variant -> the row of this input that holds it
        for (size_t r = 0; r < t.rows.size(); r++) {
            const std::vector<std::string> f = split_tabs(t.rows[r]);
            const uint64_t line = r < t.line_no.size() ? t.line_no[r] : r + 1;
            if (f.size() < need) throw MatchError(t.name + ": line " + std::to_string(line) + ": fewer fields than the column line names");
            const std::string &ref = f[c_ref], &alt = f[c_alt];
            const std::string key = f[c_chrom] + '\t' + f[c_pos] + '\t' + std::min(ref, alt) + '\t' + std::max(ref, alt);
            uint64_t pos = 0;
            if (with_union && !parse_u64(f[c_pos], pos))
                throw MatchError(t.name + ": line " + std::to_string(line) + ": POS '" + f[c_pos] + "' is not an unsigned integer");
            const uint64_t rank = chrom_rank.emplace(f[c_chrom], chrom_rank.size()).first->second;
            auto it = by_key.find(key);
            if (it == by_key.end()) {
                it = by_key.emplace(key, variants.size()).first;
                Variant v;
                v.first_input = (uint32_t)p, v.first_row = r, v.ref = ref, v.id = f[c_id], v.chrom_rank = rank, v.pos = pos;
                v.row.assign(P, kAbsent), v.flip.assign(P, 0);
                variants.push_back(std::move(v));
            }
            Variant &v = variants[it->second];
            const auto dup = seen_here.emplace(it->second, r);
            if (!dup.second) {
                const uint64_t other = dup.first->second < t.line_no.size() ? t.line_no[dup.first->second] : dup.first->second + 1;
                throw MatchError(t.name + ": lines " + std::to_string(other) + " and " + std::to_string(line) + " hold the same variant (" + f[c_chrom] +
                                 ":" + f[c_pos] + " " + ref + "/" + alt + ")");
            }
            v.row[p] = (int64_t)r;
            v.flip[p] = ref != v.ref;   // the key matched: then REF is the row's ALT
            v.holders++;
        }
    }

    // the output rows
    std::vector<size_t> order;
    if (with_union) {
        order.resize(variants.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            const Variant &x = variants[a], &y = variants[b];
            return x.chrom_rank != y.chrom_rank ? x.chrom_rank < y.chrom_rank : x.pos < y.pos;
        });
    } else {
        // variants of the first input are first seen in its order
        for (size_t i = 0; i < variants.size(); i++)
            if (variants[i].first_input == 0 && variants[i].holders == P) order.push_back(i);
    }
    const size_t V = order.size();
    m.from_input.resize(V), m.from_row.resize(V);
    for (size_t p = 0; p < P; p++) m.src[p].resize(V), m.flip[p].resize(V);
    for (size_t j = 0; j < V; j++) {
        const Variant &v = variants[order[j]];
        m.from_input[j] = v.first_input, m.from_row[j] = v.first_row;
        for (size_t p = 0; p < P; p++) {
            m.src[p][j] = v.row[p];
            m.flip[p][j] = v.row[p] != kAbsent && v.flip[p];
            m.flipped[p] += m.flip[p][j];
            m.absent[p] += v.row[p] == kAbsent;
            if (v.row[p] != kAbsent && p != v.first_input && split_tabs(pvars[p].rows[(size_t)v.row[p]])[c_id] != v.id) m.id_conflicts++;
        }
    }
    for (size_t p = 0; p < P; p++) m.dropped[p] = pvars[p].rows.size() - (V - m.absent[p]);
    return m;
}

void check_samples(const std::vector<Table> &psams)
{
    if (psams.empty()) return;
    same_column_lines(psams, ".psam");
    const size_t c_iid = column_of(column_names(psams[0].column_line), "IID", psams[0].name);
    std::unordered_map<std::string, size_t> seen;   // IID -> input
    for (size_t p = 0; p < psams.size(); p++)
        for (size_t r = 0; r < psams[p].rows.size(); r++) {
            const std::vector<std::string> f = split_tabs(psams[p].rows[r]);
            const uint64_t line = r < psams[p].line_no.size() ? psams[p].line_no[r] : r + 1;
            if (f.size() <= c_iid) throw MatchError(psams[p].name + ": line " + std::to_string(line) + ": fewer fields than the column line names");
            const auto ins = seen.emplace(f[c_iid], p);
            if (!ins.second)
                throw MatchError("sample IID '" + f[c_iid] + "' occurs twice: in " + psams[ins.first->second].name + " and in " + psams[p].name +
                                 " (sample overlap between inputs is not built)");
        }
}

}  // namespace pgenhost::merge
