// merge_check.cpp — pgen_rs_amd/host/merge_match.cpp on files, as a stand-alone program (tests/test_host_merge.py builds it from that
// source alone under ASan + UBSan and compares its lines with tests/merge_ref.py).
//   merge_check variants|union A.pvar B.pvar ...   "row <from_input> <from_row> <src_0> <flip_0> <src_1> <flip_1> ..." per output row,
//                                                  then "flipped ..", "absent ..", "dropped ..", "id_conflicts n"
//   merge_check samples A.psam B.psam ...          "ok"
// A MatchError prints "error <what>"; the exit status is 0 either way.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../pgen_rs_amd/host/merge_match.h"

using namespace pgenhost::merge;

// the column line is the last leading '#' line; the rows follow
static Table read_table(const char *path)
{
    Table t;
    t.name = path;
    std::ifstream f(path);
    std::string line;
    uint64_t n = 0;
    bool head = true;
    while (std::getline(f, line)) {
        n++;
        if (head && !line.empty() && line[0] == '#') {
            t.column_line = line;
            continue;
        }
        head = false;
        if (line.empty()) continue;
        t.rows.push_back(line);
        t.line_no.push_back(n);
    }
    return t;
}

static void print(const char *what, const std::vector<uint64_t> &v)
{
    std::printf("%s", what);
    for (const uint64_t x : v) std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    std::vector<Table> tables;
    for (int i = 2; i < argc; i++) tables.push_back(read_table(argv[i]));
    try {
        if (mode == "samples") {
            check_samples(tables);
            std::printf("ok\n");
            return 0;
        }
        const Match m = match_variants(tables, mode == "union");
        for (size_t j = 0; j < m.from_input.size(); j++) {
            std::printf("row %u %llu", m.from_input[j], (unsigned long long)m.from_row[j]);
            for (size_t p = 0; p < tables.size(); p++) std::printf(" %lld %u", (long long)m.src[p][j], (unsigned)m.flip[p][j]);
            std::printf("\n");
        }
        print("flipped", m.flipped);
        print("absent", m.absent);
        print("dropped", m.dropped);
        std::printf("id_conflicts %llu\n", (unsigned long long)m.id_conflicts);
    } catch (const MatchError &e) {
        std::printf("error %s\n", e.what());
    }
    return 0;
}
