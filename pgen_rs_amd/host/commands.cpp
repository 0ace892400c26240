// commands.cpp — the commands of pfile.h that the reference does not have: freq, sample-counts, score, matrix, ld, export,
// kinship, grm and pca (assoc: assoc.cpp; prune: prune.cpp; import: import.cpp; merge: merge.cpp).  Each selects, runs its counter
// through the block loop (block_loop.h), calls the arithmetic (stats.h, linalg.h) and prints.
#include <fcntl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <map>
#include <mutex>

#include "block_loop.h"
#include "prune.h"
#include "linalg.h"
#include "stats.h"

namespace pgenhost {

namespace {

// freq's counter: 16 bytes per variant, copied back block by block
struct VariantCounter : Counter {
    std::vector<uint32_t> &counts;   // 4 per kept variant
    uint32_t *d_counts, *h_counts;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const { genotype_counts(b, nv, d_counts); }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, nv * 16), "D2H counts"); }
    void collect(size_t b0, size_t nv) const { std::memcpy(counts.data() + 4 * b0, h_counts, nv * 16); }
};

// sample-counts' counter: every block of the shard accumulates into one device buffer of 16 bytes per kept sample (the first
// overwrites it), copied back once; the host sums the shards in u64
struct SampleCounter : Counter {
    size_t K;
    std::vector<uint64_t> &totals;   // 4 per kept sample
    std::mutex &mu;
    uint32_t *d_counts, *h_counts;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool first) const { sample_counts(b, nv, d_counts, !first); }
    void finish(pgenhip_ctx *ctx) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, K * 16), "D2H counts");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < 4 * K; i++) totals[i] += h_counts[i];
    }
};

// score's counter: per block the matched rows' weights go up, the rows' mean dosages are computed from their genotype counts
// (mean imputation) and go up as the miss values, and the score kernel adds the block into the shard's K x C doubles, eight
// columns per launch; the sample counts of the same rows accumulate beside them (the per-sample missing count).  Both come back
// once per shard and the host sums the shards in FP64 / u64.
struct ScoreCounter : Counter {
    size_t K, C;                      // kept samples, score columns
    bool impute;
    const std::vector<float> &w;      // matched rows x C, the sign of REF-effect rows flipped
    std::vector<double> &sums;        // K x C
    std::vector<uint64_t> &missing;   // K
    std::mutex &mu;
    float *d_w, *d_miss, *h_miss;
    uint32_t *d_gc, *h_gc, *d_counts, *h_counts;
    double *d_scores, *h_scores;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t, bool first) const
    {
        pgenhip_ctx *ctx = b.ctx;
        if (impute) {
            genotype_counts_now(b, nv, d_gc, h_gc);
            for (uint32_t j = 0; j < nv; j++) h_miss[j] = (float)stats::mean_dosage(h_gc + 4 * j);
            check(pgenhip_memcpy_h2d(ctx, d_miss, h_miss, (size_t)nv * sizeof(float)), "H2D mean dosages");
        }
        check(pgenhip_memcpy_h2d(ctx, d_w, w.data() + b0 * C, (size_t)nv * C * sizeof(float)), "H2D weights");
        const uint32_t acc = first ? 0u : PGENHIP_SCORE_ACCUMULATE;
        column_groups(C, PGENHIP_SCORE_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            double *dst = d_scores + K * c0;   // group g's K x cg block behind the blocks of the groups before it
            launch_rows(b, NAMED(pgenhip_sample_scores), NAMED(pgenhip_sample_scores_at), nv, d_w + c0, C, (uint32_t)cg, impute ? d_miss : nullptr, dst,
                        PGENHIP_SCORE_AUTO | acc);
        });
        sample_counts(b, nv, d_counts, !first);
    }
    void finish(pgenhip_ctx *ctx) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_scores, d_scores, K * C * sizeof(double)), "D2H scores");
        check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, K * 16), "D2H counts");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        std::lock_guard<std::mutex> lk(mu);
        column_groups(C, PGENHIP_SCORE_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            for (size_t k = 0; k < K; k++)
                for (size_t c = 0; c < cg; c++) sums[k * C + c0 + c] += h_scores[K * c0 + k * cg + c];
        });
        for (size_t k = 0; k < K; k++) missing[k] += h_counts[4 * k + 3];
    }
};

// matrix's "counter": every block is decoded into one device buffer, copied back and written to its place in the .npy file.
// Variant-major: a block is nv consecutive rows of the file, one pwrite.  Sample-major: a block is a column band, K pieces of
// nv elements, written from a few threads.
constexpr unsigned kMatrixWriteThreads = 4;   // a constant like the BGZF pool's cap, never the machine's CPU count
struct MatrixWriter : Counter {
    size_t K, V;
    const MatrixOptions &m;
    uint64_t pitch;   // sample-major: bytes between the device buffer's rows (a multiple of 128)
    uint8_t *d_out, *h_out;
    int fd;
    const std::string &path;
    uint64_t data_off;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const
    {
        const uint32_t flags = PGENHIP_MATRIX_AUTO | (m.sample_major ? PGENHIP_MATRIX_SAMPLE_MAJOR : 0u);
        const uint64_t stride = m.sample_major ? pitch : (uint64_t)K * m.elem_bytes;
        launch_rows(b, NAMED(pgenhip_decode_matrix), NAMED(pgenhip_decode_matrix_at), nv, d_out, stride, m.elem_bytes, m.values, flags);
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const
    {
        const size_t bytes = m.sample_major ? (size_t)((K - 1) * pitch) + nv * m.elem_bytes : nv * K * m.elem_bytes;
        check(pgenhip_memcpy_d2h(ctx, h_out, d_out, bytes), "D2H matrix");
    }
    void collect(size_t b0, size_t nv) const
    {
        const size_t E = m.elem_bytes;
        if (!m.sample_major) return pwrite_exact(fd, h_out, nv * K * E, data_off + (uint64_t)b0 * K * E, path);
        split_span(K, K >= 64 ? kMatrixWriteThreads : 1u, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) pwrite_exact(fd, h_out + k * pitch, nv * E, data_off + ((uint64_t)k * V + b0) * E, path);
        });
    }
};

// export's "counter": every block's packed records come back and are written to their place in the .pgen / .bed
struct PackWriter : Counter {
    size_t RK;
    const uint8_t *code_map;   // NULL: the identity
    uint8_t *d_out, *h_out;
    int fd;
    const std::string &path;
    uint64_t data_off;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const
    {
        launch_rows(b, NAMED(pgenhip_pack_records), NAMED(pgenhip_pack_records_at), nv, d_out, RK, code_map, PGENHIP_PACK_AUTO);
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_out, d_out, nv * RK), "D2H packed records"); }
    void collect(size_t b0, size_t nv) const { pwrite_exact(fd, h_out, nv * RK, data_off + (uint64_t)b0 * RK, path); }
};

// r^2 of a 4 x 4 table by the formula of pgenhip_pair_stats (include/pgen_hip.h): exact 64-bit terms, doubles, one rounding to float
float table_r2(const uint32_t *t, uint64_t &n_obs)
{
    uint64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (uint64_t a = 0; a < 3; a++)
        for (uint64_t b = 0; b < 3; b++) {
            const uint64_t c = t[4 * a + b];
            n += c;
            sx += a * c;
            sy += b * c;
            sxx += a * a * c;
            syy += b * b * c;
            sxy += a * b * c;
        }
    n_obs = n;
    const uint64_t p = n * sxy, q = sx * sy, cov = p >= q ? p - q : q - p;
    const uint64_t vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
    if (vx == 0 || vy == 0) return std::nanf("");
    const double c = (double)cov;
    return (float)((c * c) / ((double)vx * (double)vy));
}

// ld's counter: a block's pair entries (r^2, or tables with --counts) come back and become the block's lines at once; the blocks'
// texts are joined in variant order at the end, whichever shard made them
struct PairWriter : Counter {
    uint32_t W;
    const LdOptions &ld;
    const Pfile::IdxRecords &vars;
    const size_t (&col)[3];   // CHROM, POS, ID
    std::map<size_t, std::string> &pieces;
    std::mutex &mu;
    uint8_t *d_out, *h_out;
    size_t entry_bytes() const { return ld.counts ? 64u : 4u; }
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t nh, bool) const
    {
        launch_rows(b, NAMED(pgenhip_pair_stats), NAMED(pgenhip_pair_stats_at), nv + nh, nv, W, d_out, ld.counts ? PGENHIP_PAIR_TABLE : PGENHIP_PAIR_R2);
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_out, d_out, nv * W * entry_bytes()), "D2H pair entries"); }
    void collect(size_t b0, size_t nv) const
    {
        std::string text;
        for (size_t i = 0; i < nv; i++) {
            const StringRecord &ra = vars[b0 + i].second;
            // entries with b0 + i + d past the last kept variant were not written by the launch and are not read here
            for (size_t d = 1; d <= W && b0 + i + d < vars.size(); d++) {
                const StringRecord &rb = vars[b0 + i + d].second;
                if (ra.at(col[0]) != rb.at(col[0])) continue;
                const uint8_t *e = h_out + (i * W + (d - 1)) * entry_bytes();
                uint32_t t[16];
                uint64_t n_obs = 0;
                float r2;
                if (ld.counts) {
                    std::memcpy(t, e, 64);
                    r2 = table_r2(t, n_obs);
                } else {
                    std::memcpy(&r2, e, 4);
                }
                if (std::isnan(r2) || (double)r2 < ld.min_r2) continue;
                for (const StringRecord *r : {&ra, &rb})
                    for (int c = 0; c < 3; c++) {
                        text += r->at(col[c]);
                        text += '\t';
                    }
                append_double(text, (double)r2, 6);
                if (ld.counts) {
                    text += '\t';
                    append_u64(text, n_obs);
                    append_table_cells(text, t);
                }
                text += '\n';
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        pieces.emplace(b0, std::move(text));
    }
};

// kinship's counter: the upper block triangle of sample-pair tables, one device buffer per pair of rank tiles (ta <= tb); the
// shard's first block overwrites them, the others accumulate; they come back once per shard and the host adds the shards in u32
// (exact: a cell is at most the number of kept variants, which is a u32)
struct KinshipCounter : Counter {
    TileTriangle tri;
    std::vector<std::vector<uint32_t>> &totals;   // per pair of tiles
    std::mutex &mu;
    std::vector<uint32_t *> bufs;                 // device: 16 u32 per pair of ranks of a pair of tiles
    uint32_t *h_buf;                              // pinned, the largest buffer's size
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool first) const
    {
        const uint32_t flags = PGENHIP_SPAIR_AUTO | (first ? 0u : PGENHIP_SPAIR_ACCUMULATE);
        tri.each_pair([&](uint32_t ta, uint32_t tb) {
            launch_rows(b, NAMED(pgenhip_sample_pair_stats), NAMED(pgenhip_sample_pair_stats_at), nv, ta * tri.tile, tri.count(ta), tb * tri.tile,
                        tri.count(tb), bufs[tri.pair(ta, tb)], flags);
        });
    }
    void finish(pgenhip_ctx *ctx) const
    {
        tri.each_pair([&](uint32_t ta, uint32_t tb) {
            const size_t p = tri.pair(ta, tb), words = 16 * tri.count(ta) * tri.count(tb);
            check(pgenhip_memcpy_d2h(ctx, h_buf, bufs[p], words * 4), "D2H sample-pair tables");
            check(pgenhip_wait(ctx), "pgenhip_wait");
            std::lock_guard<std::mutex> lk(mu);
            uint32_t *dst = totals[p].data();
            for (size_t i = 0; i < words; i++) dst[i] += h_buf[i];
        });
    }
};

// grm's counter: per block the variants' counts come back, the host makes the two tables per variant and every pair of rank tiles
// of the upper block triangle gets two Gram launches (G, then N); the shard's first block overwrites the buffers, the others
// accumulate; they come back once per shard, filed under the shard's first variant so that the host can add the shards in order
struct GramCounter : Counter {
    TileTriangle tri;
    size_t bv;                                               // rows of a block at most: the N tables lie 4 * bv doubles behind the G tables
    ShardSums<std::vector<std::vector<double>>> &sums;       // per shard and pair of tiles p, G at 2 p, N at 2 p + 1
    std::mutex &mu;
    uint64_t &skipped;
    std::vector<double *> bufs;                              // device: count(ta) x count(tb) doubles, in the order of `sums`' vectors
    uint32_t *d_counts, *h_counts;
    double *d_tab, *h_tab, *h_buf;                           // h_buf: pinned, the largest buffer's size
    size_t first_b0 = 0;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t, bool first)
    {
        pgenhip_ctx *ctx = b.ctx;
        genotype_counts_now(b, nv, d_counts, h_counts);
        uint64_t zero_tables = 0;
        for (size_t j = 0; j < nv; j++) zero_tables += !stats::standardized_table(h_counts + 4 * j, h_tab + 4 * j, h_tab + 4 * (bv + j));
        {
            std::lock_guard<std::mutex> lk(mu);
            skipped += zero_tables;
        }
        check(pgenhip_memcpy_h2d(ctx, d_tab, h_tab, (size_t)(bv + nv) * 32), "H2D code values");
        const uint32_t flags = PGENHIP_GRAM_AUTO | (first ? 0u : PGENHIP_GRAM_ACCUMULATE);
        if (first) first_b0 = b0;
        tri.each_pair([&](uint32_t ta, uint32_t tb) {
            for (size_t m = 0; m < 2; m++)
                launch_rows(b, NAMED(pgenhip_sample_gram), NAMED(pgenhip_sample_gram_at), nv, d_tab + m * 4 * bv, ta * tri.tile, tri.count(ta), tb * tri.tile,
                            tri.count(tb), bufs[2 * tri.pair(ta, tb) + m], tri.count(tb), flags);
        });
    }
    void finish(pgenhip_ctx *ctx) const
    {
        std::vector<std::vector<double>> mine;
        tri.each_pair([&](uint32_t ta, uint32_t tb) {
            for (size_t m = 0; m < 2; m++) {
                const size_t n = tri.count(ta) * tri.count(tb);
                check(pgenhip_memcpy_d2h(ctx, h_buf, bufs[2 * tri.pair(ta, tb) + m], n * 8), "D2H Gram matrix");
                check(pgenhip_wait(ctx), "pgenhip_wait");
                mine.emplace_back(h_buf, h_buf + n);
            }
        });
        sums.file(first_b0, std::move(mine));
    }
};

// pca's counter of one pass: Q (K x L) goes up once per shard; per block the rows' tables go up and every group of at most sixteen
// columns gets one Gram product into the shard's K x L doubles (the first block overwrites, the others accumulate); they come back
// once per shard, filed under the shard's first variant so that the host can add the shards in order
struct PcaCounter : Counter {
    size_t K, L;
    const std::vector<double> &tables;                 // 4 per kept variant
    ShardSums<std::vector<double>> &sums;              // per shard K x L
    double *d_q, *d_y, *d_proj, *d_tab, *h_y;
    size_t first_b0 = 0;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t, bool first)
    {
        check(pgenhip_memcpy_h2d(b.ctx, d_tab, tables.data() + 4 * b0, (size_t)nv * 32), "H2D code values");
        const uint32_t flags = PGENHIP_GAPPLY_AUTO | (first ? 0u : PGENHIP_GAPPLY_ACCUMULATE);
        if (first) first_b0 = b0;
        column_groups(L, PGENHIP_GAPPLY_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            launch_rows(b, NAMED(pgenhip_gram_apply), NAMED(pgenhip_gram_apply_at), nv, (const double *)d_tab, (const double *)(d_q + c0), (uint64_t)L, (uint32_t)cg,
                        d_proj, d_y + c0, (uint64_t)L, flags);
        });
    }
    void finish(pgenhip_ctx *ctx) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_y, d_y, K * L * 8), "D2H Gram product");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        sums.file(first_b0, std::vector<double>(h_y, h_y + K * L));
    }
};

}  // namespace

OutputStats Pfile::output_freq(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                               const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    size_t col[5];
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](const Selection &sel) { pvar_columns(*this, sel.var_header, kVariantColumns, col); });
    const IdxRecords &var_idx_rcds = o.sel.var_idx_rcds;
    const KeptSamples &kept = o.kept;
    const size_t V = o.V;

    std::vector<uint32_t> counts(4 * V, 0u);
    const double t_body = now_s();
    if (V != 0 && variant_record_size() != 0) {
        count_blocks(*this, var_idx_rcds, kept, opt, "no HIP device: the genotype count path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            return VariantCounter{{}, counts, ctx.device<uint32_t>((size_t)(16 * bv), "device counts"), ctx.pinned<uint32_t>((size_t)(16 * bv), "pinned counts")};
        });
    }

    std::string text = "#CHROM\tPOS\tID\tREF\tALT\tHOM_REF_CT\tHET_REF_ALT_CTS\tTWO_ALT_GENO_CTS\tMISSING_CT\n";
    st.header_bytes = text.size();
    for (size_t j = 0; j < V; j++) {
        append_variant_columns(text, var_idx_rcds[j].second, col);
        for (int c = 0; c < 4; c++) {
            append_u64(text, counts[4 * j + (size_t)c]);
            text += c < 3 ? '\t' : '\n';
        }
    }
    finish_text(st, text, filename, t_body);
    return st;
}

OutputStats Pfile::output_sample_counts(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                        const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, true);
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t iid = o.iid, V = o.V, K = o.K;

    std::vector<uint64_t> totals(4 * K, 0u);
    const double t_body = now_s();
    if (V != 0 && K != 0) {   // else every count is zero and no device is touched
        std::mutex mu;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the sample count path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t) {
            return SampleCounter{{}, K, totals, mu, ctx.device<uint32_t>(16 * K, "device counts"), ctx.pinned<uint32_t>(16 * K, "pinned counts")};
        });
    }

    std::string text = "#IID\tHOM_REF_CT\tHET_CT\tHOM_ALT_CT\tMISSING_CT\n";
    st.header_bytes = text.size();
    for (size_t k = 0; k < K; k++) {
        text += sel.sam_idx_rcs[k].second.at(iid);
        for (int c = 0; c < 4; c++) {
            text += '\t';
            append_u64(text, totals[4 * k + (size_t)c]);
        }
        text += '\n';
    }
    finish_text(st, text, filename, t_body);
    return st;
}

ScoreWeights read_score_weights(const std::string &path)
{
    ScoreWeights sw;
    KeyedRows t = read_keyed_rows(path, 2, "a weights file has an ID column, an effect allele column and at least one score column", "variant ID",
                                  [&](const std::string &cell, const std::string &name, const std::string &where) {
        char *end = nullptr;
        errno = 0;
        const double x = std::strtod(cell.c_str(), &end);
        const bool fits = std::isfinite(x) && std::fabs(x) < 0x1.ffffffp127;   // rounds to a finite f32
        const float f = fits ? (float)x : 0.f;                                   // rounded to f32 once, here
        if (cell.empty() || *end != '\0' || !fits) throw PfileError(where + ": weight '" + cell + "' of score " + name + " is not a finite number");
        sw.w.push_back(f);
    });
    sw.names = std::move(t.names);
    sw.ids = std::move(t.lead[0]);
    sw.alleles = std::move(t.lead[1]);
    sw.lines = std::move(t.lines);
    return sw;
}

OutputStats Pfile::output_score(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                const std::string &weights_file, const std::string &filename, const ScoreOptions &sopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const ScoreWeights sw = read_score_weights(weights_file);
    const size_t C = sw.names.size();
    size_t iid = 0;
    std::vector<float> w;                 // matched rows x C, REF-effect rows negated
    std::vector<double> constant(C, 0.0); // the 2w of the REF-effect rows, added to every sample
    // the kept variants the file names, in the .pgen's order: they are the selection of every launch (the rows they replace live
    // on in `matched` until the command ends: freeing them is no part of seconds_filter)
    IdxRecords matched;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](Selection &sel) {
        iid = iid_column(*this, sel.sam_header);
        static const char *const kCols[3] = {"ID", "REF", "ALT"};
        size_t col[3];
        pvar_columns(*this, sel.var_header, kCols, col);
        std::map<std::string, size_t> row_of;
        for (size_t i = 0; i < sw.ids.size(); i++) row_of.emplace(sw.ids[i], i);
        std::vector<char> used(sw.ids.size(), 0);
        uint64_t flipped = 0, mismatched = 0;
        for (const auto &vr : sel.var_idx_rcds) {
            const auto it = row_of.find(vr.second.at(col[0]));
            if (it == row_of.end()) continue;
            const size_t i = it->second;
            if (used[i])
                throw PfileError(weights_file + " line " + std::to_string(sw.lines[i]) + ": variant ID '" + sw.ids[i] + "' occurs twice among the kept variants of " + pvar_path());
            used[i] = 1;
            const bool alt = sw.alleles[i] == vr.second.at(col[2]), ref = !alt && sw.alleles[i] == vr.second.at(col[1]);
            if (!alt && !ref) {
                mismatched++;
                continue;
            }
            for (size_t c = 0; c < C; c++) {
                const float x = sw.w[i * C + c];
                w.push_back(ref ? -x : x);
                if (ref) constant[c] += 2.0 * (double)x;
            }
            flipped += ref;
            matched.emplace_back(vr.first, StringRecord());
        }
        st.score_matched = matched.size();
        st.score_flipped = flipped;
        st.score_skipped = sw.ids.size() - matched.size();
        if (matched.empty())
            throw PfileError("no row of " + weights_file + " names a kept variant of " + pvar_path() + " by ID with its REF or ALT allele (" +
                             std::to_string(sw.ids.size()) + " rows, " + std::to_string(mismatched) + " with another allele)");
        sel.var_idx_rcds.swap(matched);
    }, t0);
    const Selection &msel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t M = o.V, K = o.K;

    std::vector<double> sums(K * C, 0.0);
    std::vector<uint64_t> missing(K, 0u);
    const double t_body = now_s();
    if (K != 0) {   // else the header alone and no device is touched
        std::mutex mu;
        count_blocks(*this, msel.var_idx_rcds, kept, opt, "no HIP device: the score path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            return ScoreCounter{{}, K, C, sopt.mean_imputation, w, sums, missing, mu,
                                ctx.device<float>(b * C * sizeof(float), "device weights"), ctx.device<float>(b * sizeof(float), "device mean dosages"),
                                ctx.pinned<float>(b * sizeof(float), "pinned mean dosages"),
                                ctx.device<uint32_t>(16 * b, "device variant counts"), ctx.pinned<uint32_t>(16 * b, "pinned variant counts"),
                                ctx.device<uint32_t>(16 * K, "device counts"), ctx.pinned<uint32_t>(16 * K, "pinned counts"),
                                ctx.device<double>(K * C * sizeof(double), "device scores"), ctx.pinned<double>(K * C * sizeof(double), "pinned scores")};
        });
    }

    std::string text = "#IID\tALLELE_CT\tDENOM";
    for (const std::string &name : sw.names) text += "\t" + name + (sopt.average ? "_AVG" : "_SUM");
    text += '\n';
    st.header_bytes = text.size();
    for (size_t k = 0; k < K; k++) {
        const uint64_t allele_ct = 2 * ((uint64_t)M - missing[k]), denom = sopt.mean_imputation ? 2 * (uint64_t)M : allele_ct;
        text += msel.sam_idx_rcs[k].second.at(iid);
        text += '\t';
        append_u64(text, allele_ct);
        text += '\t';
        append_u64(text, denom);
        for (size_t c = 0; c < C; c++) {
            const double sum = sums[k * C + c] + constant[c];
            text += '\t';
            if (sopt.average && denom == 0) text += "nan";
            else append_double(text, sopt.average ? sum / (double)denom : sum, 12);
        }
        text += '\n';
    }
    finish_text(st, text, filename, t_body);
    return st;
}

OutputStats Pfile::output_ld(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                             const std::string &filename, const LdOptions &ld, const OutputOptions &opt) const
{
    OutputStats st;
    static const char *const kCols[3] = {"CHROM", "POS", "ID"};
    size_t col[3];
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](const Selection &sel) { pvar_columns(*this, sel.var_header, kCols, col); });
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t V = o.V, K = o.K;

    std::string text = "#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tR2";
    if (ld.counts) {
        text += "\tN_OBS";
        append_table_header(text);
    }
    text += '\n';
    st.header_bytes = text.size();
    const double t_body = now_s();
    if (V >= 2 && K != 0) {   // else no pair or nothing to correlate: the header alone, no device touched
        const uint32_t W = (uint32_t)std::min<uint64_t>(ld.window, V - 1);   // no pair reaches further
        const uint64_t entry = ld.counts ? 64u : 4u;
        // left rows per block: their W entries each fill the block budget (or --block-rows)
        uint64_t bv = ld.block_rows ? ld.block_rows : std::max<uint64_t>(1, opt.block_text_bytes / ((uint64_t)W * entry));
        bv = std::min<uint64_t>(bv, V);
        std::map<size_t, std::string> pieces;
        std::mutex mu;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the pairwise path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t n) {
            const size_t bytes = (size_t)(n * W * entry);
            return PairWriter{{}, W, ld, sel.var_idx_rcds, col, pieces, mu, ctx.device<uint8_t>(bytes, "device pair entries"), ctx.pinned<uint8_t>(bytes, "pinned pair entries")};
        }, bv, W);
        for (auto &p : pieces) text += p.second;
    }
    finish_text(st, text, filename, t_body);
    return st;
}

OutputStats Pfile::output_kinship(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                  const std::string &filename, const KinshipOptions &kopt, const OutputOptions &opt) const
{
    OutputStats st;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, true);
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t iid = o.iid, V = o.V, K = o.K;

    std::string text = "#IID1\tIID2\tN\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP";
    if (kopt.counts) append_table_header(text);
    text += '\n';
    st.header_bytes = text.size();
    const double t_body = now_s();
    if (K >= 2) {   // else no pair: the header alone
        const TileTriangle tri{(uint32_t)K, std::max<uint32_t>(1u, kopt.tile)};
        const size_t tile = tri.tile;
        std::vector<std::vector<uint32_t>> totals;
        tri.each_pair([&](uint32_t ta, uint32_t tb) { totals.emplace_back(16 * tri.count(ta) * tri.count(tb), 0u); });
        if (V != 0) {   // else every table is zero and no device is touched
            std::mutex mu;
            count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the kinship path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t) {
                KinshipCounter kc{{}, tri, totals, mu, {}, nullptr};
                tri.each_pair([&](uint32_t ta, uint32_t tb) { kc.bufs.push_back(ctx.device<uint32_t>(64 * tri.count(ta) * tri.count(tb), "device sample-pair tables")); });
                kc.h_buf = ctx.pinned<uint32_t>(64 * tri.count(0) * tri.count(0), "pinned sample-pair tables");
                return kc;
            }, kopt.block_rows);
        }
        for (size_t a = 0; a < K; a++) {
            const size_t ta = a / tile, i = a % tile;
            for (size_t b = a + 1; b < K; b++) {
                const size_t tb = b / tile, l = b % tile;
                const uint32_t *t = totals[tri.pair(ta, tb)].data() + 16 * (i * tri.count((uint32_t)tb) + l);
                const stats::King k = stats::king(t);
                if (kopt.has_min && !(k.kinship >= kopt.min_kinship)) continue;   // nan lines go with the ones below the floor
                text += sel.sam_idx_rcs[a].second.at(iid);
                text += '\t';
                text += sel.sam_idx_rcs[b].second.at(iid);
                for (const uint64_t v : {k.n, k.hethet, k.ibs0, k.het1, k.het2}) {
                    text += '\t';
                    append_u64(text, v);
                }
                text += '\t';
                append_double(text, k.kinship, 6, true);
                if (kopt.counts) append_table_cells(text, t);
                text += '\n';
            }
        }
    }
    finish_text(st, text, filename, t_body);
    return st;
}

OutputStats Pfile::output_grm(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &out_prefix, const GrmOptions &gopt, const OutputOptions &opt) const
{
    OutputStats st;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, true);
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t iid = o.iid, V = o.V, K = o.K;
    const double t_body = now_s();

    const TileTriangle tri{(uint32_t)K, std::max<uint32_t>(1u, gopt.tile)};
    const size_t tile = tri.tile;
    // per pair of tiles p, G at 2 p and N at 2 p + 1: the shards' sums, added in shard order
    std::vector<std::vector<double>> totals;
    tri.each_pair([&](uint32_t ta, uint32_t tb) {
        for (int m = 0; m < 2; m++) totals.emplace_back(tri.count(ta) * tri.count(tb), 0.0);
    });
    if (K != 0 && V != 0) {   // else nothing is summed and no device is touched
        std::mutex mu;
        ShardSums<std::vector<std::vector<double>>> sums;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the grm path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            GramCounter gc{{}, tri, (size_t)bv, sums, mu, st.grm_skipped, {}, nullptr, nullptr, nullptr, nullptr, nullptr};
            tri.each_pair([&](uint32_t ta, uint32_t tb) {
                for (int m = 0; m < 2; m++) gc.bufs.push_back(ctx.device<double>(8 * tri.count(ta) * tri.count(tb), "device Gram matrix"));
            });
            gc.d_counts = ctx.device<uint32_t>((size_t)(16 * bv), "device counts");
            gc.h_counts = ctx.pinned<uint32_t>((size_t)(16 * bv), "pinned counts");
            gc.d_tab = ctx.device<double>((size_t)(64 * bv), "device code values");
            gc.h_tab = ctx.pinned<double>((size_t)(64 * bv), "pinned code values");
            gc.h_buf = ctx.pinned<double>(8 * tri.count(0) * tri.count(0), "pinned Gram matrix");
            return gc;
        }, gopt.block_rows);
        for (const auto &shard : sums.in_order())
            for (size_t q = 0; q < totals.size(); q++)
                for (size_t i = 0; i < totals[q].size(); i++) totals[q][i] += shard.second[q][i];
    }
    // entry (a, b) of matrix m, read from the block that holds (min, max): the square written is exactly symmetric
    auto entry = [&](size_t a, size_t b, size_t m) {
        const size_t lo = std::min(a, b), hi = std::max(a, b);
        const size_t ta = lo / tile, tb = hi / tile;
        return totals[2 * tri.pair(ta, tb) + m][(lo % tile) * tri.count((uint32_t)tb) + hi % tile];
    };
    auto grm = [&](size_t a, size_t b) {
        const double n = entry(a, b, 1);
        return n == 0.0 ? std::nan("") : entry(a, b, 0) / n;
    };
    std::string ids;
    for (size_t a = 0; a < K; a++) {
        const std::string &name = sel.sam_idx_rcs[a].second.at(iid);
        if (!gopt.rel) ids += name + '\t';   // FID = IID: the .psam files here carry no FID
        ids += name + '\n';
    }
    if (gopt.rel) {
        std::string text;
        for (size_t a = 0; a < K; a++)
            for (size_t b = 0; b < K; b++) {
                append_double(text, grm(a, b), 17, true);
                text += b + 1 < K ? '\t' : '\n';
            }
        st.file_bytes = text.size();
        write_text(text, out_prefix + ".rel");
        write_text(ids, out_prefix + ".rel.id");
    } else {
        std::vector<float> g, n;
        g.reserve(K * (K + 1) / 2);
        n.reserve(K * (K + 1) / 2);
        for (size_t a = 0; a < K; a++)
            for (size_t b = 0; b <= a; b++) {
                g.push_back((float)grm(a, b));
                n.push_back((float)entry(a, b, 1));
            }
        st.file_bytes = 8 * g.size();
        write_text(std::string(reinterpret_cast<const char *>(g.data()), 4 * g.size()), out_prefix + ".grm.bin");
        write_text(std::string(reinterpret_cast<const char *>(n.data()), 4 * n.size()), out_prefix + ".grm.N.bin");
        write_text(ids, out_prefix + ".grm.id");
    }
    st.body_bytes = st.file_bytes;
    st.seconds_body = now_s() - t_body;
    return st;
}

OutputStats Pfile::output_pca(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &out_prefix, const PcaOptions &popt, const OutputOptions &opt) const
{
    OutputStats st;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, true);
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t iid = o.iid, V = o.V, K = o.K, P = popt.pcs;
    const double t_body = now_s();
    std::string header = "#IID";
    for (size_t i = 0; i < P; i++) header += "\tPC" + std::to_string(i + 1);
    header += '\n';
    st.header_bytes = header.size();
    auto write_out = [&](const std::string &vals, const std::string &vecs) {
        st.file_bytes = header.size() + vecs.size();
        st.body_bytes = vecs.size();
        write_text(vals, out_prefix + ".eigenval");
        write_text(header + vecs, out_prefix + ".eigenvec");
        st.seconds_body = now_s() - t_body;
        return st;
    };
    if (K == 0 || V == 0) return write_out("", "");   // nothing to decompose and no device touched
    if (P > K) throw PfileError("--pcs " + std::to_string(P) + " asks for more components than the " + std::to_string(K) + " kept samples");
    static const char *const kNoDevice = "no HIP device: the pca path has no CPU fallback";

    // the tables: grm's table G per variant, from a first pass of genotype counts
    std::vector<uint32_t> counts(4 * V, 0u);
    count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
        return VariantCounter{{}, counts, ctx.device<uint32_t>((size_t)(16 * bv), "device counts"), ctx.pinned<uint32_t>((size_t)(16 * bv), "pinned counts")};
    }, popt.block_rows);
    std::vector<double> tables(4 * V, 0.0);
    for (size_t j = 0; j < V; j++) {
        double n[4];   // grm's table N, not used here
        st.pca_skipped += !stats::standardized_table(counts.data() + 4 * j, tables.data() + 4 * j, n);
    }
    const size_t V_used = V - (size_t)st.pca_skipped;
    if (V_used == 0) return write_out("", "");

    // the start: a seeded Gaussian K x L matrix, orthonormalised
    const size_t L = std::min(K, P + 10);
    std::vector<double> Q, Y(K * L), U, lambda;
    linalg::gaussian_start(popt.seed, K, L, Q);
    linalg::qr_thin(Q, K, L);

    double kernel_s = 0, setup_s = 0;
    for (;;) {
        // Y = M Q
        ShardSums<std::vector<double>> sums;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            PcaCounter pc{{}, K, L, tables, sums, ctx.device<double>(K * L * 8, "device Q"), ctx.device<double>(K * L * 8, "device Gram product"),
                          ctx.device<double>((size_t)(bv * PGENHIP_GAPPLY_MAX_COLUMNS * 8), "device projections"),
                          ctx.device<double>((size_t)(bv * 32), "device code values"), ctx.pinned<double>(K * L * 8, "pinned Gram product")};
            check(pgenhip_memcpy_h2d(ctx.get(), pc.d_q, Q.data(), K * L * 8), "H2D Q");
            return pc;
        }, popt.block_rows);
        kernel_s += st.seconds_kernel;
        setup_s += st.seconds_setup;
        std::fill(Y.begin(), Y.end(), 0.0);
        for (const auto &shard : sums.in_order())
            for (size_t i = 0; i < K * L; i++) Y[i] += shard.second[i];
        for (double &y : Y) y /= (double)V_used;
        st.pca_passes++;

        const double worst = linalg::rayleigh_ritz(Q, Y, K, L, P, lambda, U);
        st.pca_residual = lambda[0] > 0.0 ? worst / lambda[0] : 0.0;
        st.pca_converged = worst <= popt.tol * lambda[0];
        if (st.pca_converged || st.pca_passes >= popt.max_passes) break;
        Q = Y;
        linalg::qr_thin(Q, K, L);
    }
    st.seconds_kernel = kernel_s;
    st.seconds_setup = setup_s;
    if (!st.pca_converged)
        std::fprintf(stderr, "pgen-hip: warning: pca did not reach --tol within %llu passes (residual %.3g of lambda_1); the outputs are written all the same\n",
                     (unsigned long long)st.pca_passes, st.pca_residual);

    std::string vals, vecs;
    for (size_t i = 0; i < P; i++) {
        append_double(vals, lambda[i], 17);
        vals += '\n';
    }
    linalg::unit_columns_largest_positive(U, K, L, P);
    for (size_t k = 0; k < K; k++) {
        vecs += sel.sam_idx_rcs[k].second.at(iid);
        for (size_t i = 0; i < P; i++) {
            vecs += '\t';
            append_double(vecs, U[k * L + i], 17);
        }
        vecs += '\n';
    }
    return write_out(vals, vecs);
}

OutputStats Pfile::output_matrix(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                 const std::string &filename, const MatrixOptions &mopt, const OutputOptions &opt) const
{
    OutputStats st;
    size_t id_col = 0;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, true, [&](const Selection &sel) { id_col = column(sel.var_header, "ID", pvar_path()); });
    const Selection &sel = o.sel;
    const KeptSamples &kept = o.kept;
    const size_t iid_col = o.iid, V = o.V, K = o.K, E = mopt.elem_bytes;

    // .npy version 1.0: magic, version, u16 header length, the dict padded with spaces and ended by a newline so that the data
    // starts on a multiple of 64 bytes
    std::string dict = "{'descr': '" + mopt.descr + "', 'fortran_order': False, 'shape': (" +
                       std::to_string(mopt.sample_major ? K : V) + ", " + std::to_string(mopt.sample_major ? V : K) + "), }";
    while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';
    dict += '\n';
    std::string header("\x93NUMPY\x01\x00", 8);
    header += (char)(dict.size() & 0xFF);
    header += (char)(dict.size() >> 8);
    header += dict;
    st.header_bytes = header.size();
    st.body_bytes = (uint64_t)V * K * E;
    st.file_bytes = st.header_bytes + st.body_bytes;

    const double t_body = now_s();
    static const char *const kNoDevice = "no HIP device: the genotype matrix path has no CPU fallback";
    if (V != 0 && K != 0) const Shards probe(opt, kNoDevice);   // before the output file exists
    Fd out(filename, O_WRONLY | O_CREAT | O_TRUNC);
    pwrite_exact(out.get(), header.data(), header.size(), 0, filename);
    if (V != 0 && K != 0) {   // else a zero dimension: the header alone, no device touched
        // variants per block: block_text_bytes of matrix; a sample-major block is a column band whose row pieces hold at least
        // 4 096 elements where a 1-GiB buffer allows
        uint64_t bv = std::max<uint64_t>(1, opt.block_text_bytes / ((uint64_t)K * E));
        if (mopt.sample_major) bv = std::max<uint64_t>(bv, std::max<uint64_t>(1, std::min<uint64_t>(4096, (1ull << 30) / ((uint64_t)K * E))));
        bv = std::min<uint64_t>(bv, V);
        count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t n) {
            const uint64_t pitch = (n * E + 127) / 128 * 128;
            const size_t bytes = (size_t)(mopt.sample_major ? (uint64_t)K * pitch : n * K * E);
            return MatrixWriter{{}, K, V, mopt, pitch, ctx.device<uint8_t>(bytes, "device matrix"), ctx.pinned<uint8_t>(bytes, "pinned matrix"),
                                out.get(), filename, (uint64_t)header.size()};
        }, bv);
    }
    out.close();
    std::string ids;
    for (const auto &vr : sel.var_idx_rcds) ids += vr.second.at(id_col) + "\n";
    write_text(ids, filename + ".variants");
    ids.clear();
    for (const auto &sr : sel.sam_idx_rcs) ids += sr.second.at(iid_col) + "\n";
    write_text(ids, filename + ".samples");
    st.seconds_body = now_s() - t_body;
    return st;
}

// export's two halves, which `prune --export` also runs on the variants it kept (prune.h): the two metadata texts of a selection ...
void export_texts(const Pfile &pf, const Pfile::Selection &sel, const ExportOptions &eopt, std::string &var_text, std::string &sam_text)
{
    auto optional_column = [](const StringRecord &header, const char *name) {   // header.size(): the file has none
        return (size_t)(std::find(header.begin(), header.end(), std::string(name)) - header.begin());
    };
    auto join_rows = [](std::string &text, const Pfile::IdxRecords &rows) {
        for (const auto &ir : rows) {
            for (size_t c = 0; c < ir.second.size(); c++) {
                if (c) text += '\t';
                text += ir.second[c];
            }
            text += '\n';
        }
    };
    if (eopt.bed) {
        const StringRecord &vh = sel.var_header, &sh = sel.sam_header;
        const size_t chrom = column(vh, "CHROM", pf.pvar_path()), id = column(vh, "ID", pf.pvar_path()), pos = column(vh, "POS", pf.pvar_path()),
                     ref = column(vh, "REF", pf.pvar_path()), alt = column(vh, "ALT", pf.pvar_path());
        for (const auto &vr : sel.var_idx_rcds) {
            const StringRecord &r = vr.second;
            if (r.at(alt).find(',') != std::string::npos)
                throw PfileError("variant " + r.at(id) + " (row " + std::to_string(vr.first) + " of " + pf.pvar_path() + ") has more than one ALT allele (" +
                                 r.at(alt) + "): a .bed holds biallelic variants only");
            var_text += r.at(chrom) + '\t' + r.at(id) + "\t0\t" + r.at(pos) + '\t' + r.at(alt) + '\t' + r.at(ref) + '\n';
        }
        const size_t iid = iid_column(pf, sh), fid = optional_column(sh, "FID"), pat = optional_column(sh, "PAT"), mat = optional_column(sh, "MAT"),
                     sex = optional_column(sh, "SEX");
        for (const auto &sr : sel.sam_idx_rcs) {
            const StringRecord &r = sr.second;
            auto or_zero = [&](size_t c) { return c == sh.size() ? std::string("0") : r.at(c); };
            const std::string sx = sex == sh.size() ? std::string("0") : r.at(sex);
            sam_text += or_zero(fid) + '\t' + r.at(iid) + '\t' + or_zero(pat) + '\t' + or_zero(mat) + '\t' + (sx == "1" || sx == "2" ? sx : std::string("0")) + "\t-9\n";
        }
    } else {
        const auto [pvar_header, pvar_column_names] = pf.read_pvar_header();
        var_text = pvar_header + pvar_column_names;
        if (!var_text.empty() && var_text.back() != '\n') var_text += '\n';
        join_rows(var_text, sel.var_idx_rcds);
        const std::string psam = read_file(pf.psam_path());
        const size_t eol = psam.find('\n', (size_t)Pfile::find_metadata_file_header_start(psam));
        sam_text = eol == std::string::npos ? psam + "\n" : psam.substr(0, eol + 1);
        join_rows(sam_text, sel.sam_idx_rcs);
    }
}

// ... and the records of its variants packed on the device(s) and written with the texts (st.variants: the variants written)
void export_records(const Pfile &pf, const Pfile::IdxRecords &vars, const KeptSamples &kept, const std::string &out_prefix, const ExportOptions &eopt,
                    const OutputOptions &opt, OutputStats &st, const std::string &var_text, const std::string &sam_text)
{
    const std::string out_main = out_prefix + (eopt.bed ? ".bed" : ".pgen");
    const std::string out_var = out_prefix + (eopt.bed ? ".bim" : ".pvar"), out_sam = out_prefix + (eopt.bed ? ".fam" : ".psam");
    const size_t V = vars.size(), K = kept.rows.size(), RK = (K + 3) / 4;
    std::string header;
    if (eopt.bed) {
        header.assign("\x6C\x1B\x01", 3);   // variant-major
    } else {
        header.assign("\x6C\x1B\x02", 3);
        for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)V >> (8 * b));
        for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)K >> (8 * b));
        header += '\x40';
    }
    st.header_bytes = header.size();
    st.body_bytes = (uint64_t)V * RK;
    st.file_bytes = st.header_bytes + st.body_bytes;

    const double t_body = now_s();
    static const char *const kNoDevice = "no HIP device: the record pack path has no CPU fallback";
    if (V != 0 && K != 0) const Shards probe(opt, kNoDevice);   // before the output files exist
    Fd out(out_main, O_WRONLY | O_CREAT | O_TRUNC);
    pwrite_exact(out.get(), header.data(), header.size(), 0, out_main);
    if (V != 0 && K != 0) {   // else a zero dimension: the header alone, no device touched
        static const uint8_t kBedMap[4] = {3, 2, 0, 1};   // ALT as A1: 00 hom A1, 01 missing, 10 het, 11 hom A2
        count_blocks(pf, vars, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t bytes = (size_t)(bv * RK);
            return PackWriter{{}, RK, eopt.bed ? kBedMap : nullptr, ctx.device<uint8_t>(bytes, "device packed records"),
                              ctx.pinned<uint8_t>(bytes, "pinned packed records"), out.get(), out_main, (uint64_t)header.size()};
        });
    }
    out.close();
    write_text(var_text, out_var);
    write_text(sam_text, out_sam);
    st.seconds_body = now_s() - t_body;
}

void refuse_export_over_input(const Pfile &pf, const std::string &out_main)
{
    // the same file by another spelling or through a link is still the input
    std::error_code ec1, ec2;
    const auto in = std::filesystem::weakly_canonical(pf.pgen_path(), ec1), out = std::filesystem::weakly_canonical(out_main, ec2);
    if (out_main == pf.pgen_path() || (!ec1 && !ec2 && in == out))
        throw PfileError("export would overwrite its input: " + out_main + " is " + pf.pgen_path());
}

OutputStats Pfile::output_export(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                 const std::string &out_prefix, const ExportOptions &eopt, const OutputOptions &opt) const
{
    OutputStats st;
    if (!eopt.bed) refuse_export_over_input(*this, out_prefix + ".pgen");
    std::string var_text, sam_text;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](const Selection &sel) { export_texts(*this, sel, eopt, var_text, sam_text); });
    export_records(*this, o.sel.var_idx_rcds, o.kept, out_prefix, eopt, opt, st, var_text, sam_text);
    return st;
}

}  // namespace pgenhost
