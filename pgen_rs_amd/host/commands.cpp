// commands.cpp — the commands of pfile.h that the reference does not have: freq, sample-counts, score, assoc, matrix, ld, export,
// kinship, grm and pca, with the block loop they share, and import (VCF text to a fileset).  Line references are to the reference's src/pfile.rs.
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <map>
#include <mutex>
#include <thread>

#include "host_internal.h"
#include "linalg.h"

namespace pgenhost {

namespace {

void append_u64(std::string &s, uint64_t v)
{
    char buf[24];
    int n = 0;
    do {
        buf[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) s += buf[--n];
}

void write_text(const std::string &text, const std::string &filename)
{
    if (filename.empty()) {
        if (std::fwrite(text.data(), 1, text.size(), stdout) != text.size() || std::fflush(stdout) != 0)
            throw PfileError(std::string("write stdout: ") + std::strerror(errno));
    } else {
        Fd out(filename, O_WRONLY | O_CREAT | O_TRUNC);
        pwrite_exact(out.get(), text.data(), text.size(), 0, filename);
        out.close();
    }
}

// the last step of a command whose output is one text behind st.header_bytes of header: the byte counts, the text to `filename`
// (empty: stdout), the body's time
void finish_text(OutputStats &st, const std::string &text, const std::string &filename, double t_body)
{
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
}

// A staged block as a counter's launches see it
struct BlockRows {
    pgenhip_ctx *ctx;
    const uint8_t *d_rec;
    uint32_t R;
    const uint64_t *d_off;   // the rows' offsets in d_rec; NULL: records packed at stride R
};

// One ABI pair over the first n rows of a block: plain is pgenhip_X(ctx, d_records, stride, d_variant_idx, n, rest...), at is
// pgenhip_X_at(ctx, d_base, d_record_off, n, rest...); a failure names the entry that was called
#define NAMED(fn) fn, #fn
template <class Plain, class At, class... Rest>
void launch_rows(const BlockRows &b, Plain plain, const char *plain_name, At at, const char *at_name, uint32_t n, Rest... rest)
{
    if (b.d_off)
        check(at(b.ctx, b.d_rec, b.d_off, n, rest...), at_name);
    else
        check(plain(b.ctx, b.d_rec, b.R, nullptr, n, rest...), plain_name);
}

void genotype_counts(const BlockRows &b, uint32_t nv, uint32_t *d_counts)
{
    launch_rows(b, NAMED(pgenhip_genotype_counts), NAMED(pgenhip_genotype_counts_at), nv, d_counts, PGENHIP_COUNT_AUTO);
}

void sample_counts(const BlockRows &b, uint32_t nv, uint32_t *d_counts, bool accumulate)
{
    launch_rows(b, NAMED(pgenhip_sample_counts), NAMED(pgenhip_sample_counts_at), nv, d_counts,
                PGENHIP_SCOUNT_AUTO | (accumulate ? PGENHIP_SCOUNT_ACCUMULATE : 0u));
}

// The block loop of every command here.  Per shard: blocks of bv variants (block_rows, or with 0 as many as hold
// opt.block_text_bytes of records).  Block k's records are read into pinned buffer k % 2 while the device copies and counts block
// k - 1; each block's H2D copy and count launch are queued on the ctx stream.
// Fixed-width files: runs of consecutive records are read in one go and packed at stride R.  Variable-width files: the plain
// records are staged as they lie on disk (a span grows over gaps of up to R bytes, so a block stages at most 2R bytes per
// variant) and counted through their offsets in the staged bytes (the `_at` entry points).
// make(ctx, bv) builds a shard's counter, which provides
//   launch(rows, b0, nv, nh, first): queue the block's count launch over its nv rows (and the nh halo rows staged behind them;
//     b0: index of the block's first variant in `vars`; first: the shard's first block);
//   copy(ctx, nv): queue what goes back after it (outside the kernel timer);
//   collect(b0, nv): the block's work on the stream has finished (b0: index of its first variant in `vars`);
//   finish(ctx): after the shard's last block has been collected.
// halo: rows behind a block's own that are staged with it (ld: a block's left rows and the `window` rows that follow them, which
// may belong to the next block or shard); launch gets their number.  0: a block is its own rows.
template <class Make>
void count_blocks(const Pfile &pf, const Pfile::IdxRecords &vars, const KeptSamples &kept, const OutputOptions &opt, const char *no_device,
                  OutputStats &st, const Make &make, uint64_t block_rows = 0, size_t halo = 0)
{
    const uint32_t R = pf.variant_record_size();
    const Shards shards(opt, no_device);
    std::vector<double> kernel_s((size_t)shards.G, 0.0), setup_s((size_t)shards.G, 0.0);
    const std::string pgen = pf.pgen_path();
    const bool vw = pf.variable_width();
    shards.run(vars.size(), [&](int g, int device, size_t begin, size_t end) {
        const double t_worker = now_s();
        const Fd pgen_fd(pgen, O_RDONLY);
        const uint64_t bv = std::max<uint64_t>(1, std::min<uint64_t>(block_rows ? block_rows : opt.block_text_bytes / R, end - begin));
        const uint64_t bt = bv + halo;   // rows a block stages at most
        const size_t stage_bytes = (size_t)(bt * R) * (vw ? 2u : 1u);
        DeviceCtx ctx(device, pf.num_samples, &kept);
        uint8_t *d_rec = ctx.device<uint8_t>(stage_bytes, "device records");
        uint64_t *d_off = vw ? ctx.device<uint64_t>((size_t)(8 * bt), "device record offsets") : nullptr;
        uint8_t *h_rec[2] = {ctx.pinned<uint8_t>(stage_bytes, "pinned records"), ctx.pinned<uint8_t>(stage_bytes, "pinned records")};
        uint64_t *h_off[2] = {nullptr, nullptr};
        if (vw) {
            h_off[0] = ctx.pinned<uint64_t>((size_t)(16 * bt), "pinned record offsets");
            h_off[1] = h_off[0] + bt;
        }
        auto counter = make(ctx, bv);
        setup_s[(size_t)g] = now_s() - t_worker;

        size_t prev_b0 = 0, prev_nv = 0;   // the block in flight on the device
        auto collect = [&] {
            if (!prev_nv) return;
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            float ms = 0;
            if (pgenhip_timer_read(ctx.get(), &ms) == PGENHIP_OK) kernel_s[(size_t)g] += ms * 1e-3;
            counter.collect(prev_b0, prev_nv);
            prev_nv = 0;
        };
        for (size_t b0 = begin, k = 0; b0 < end; b0 += (size_t)bv, k++) {
            const size_t nv = std::min<size_t>((size_t)bv, end - b0);
            const size_t nh = std::min<size_t>(halo, vars.size() - (b0 + nv)), nt = nv + nh;
            uint8_t *dst = h_rec[k % 2];
            size_t staged = 0;
            for (size_t j = 0; j < nt;) {
                const uint64_t off0 = pf.record_offset(vars[b0 + j].first);
                size_t run = 1;
                uint64_t span = R;   // bytes of the file from off0 this run covers
                if (vw) {
                    h_off[k % 2][j] = staged;
                    while (j + run < nt) {
                        const uint64_t off = pf.record_offset(vars[b0 + j + run].first);
                        if (off > off0 + span + R) break;
                        h_off[k % 2][j + run] = staged + (off - off0);
                        span = off + R - off0;
                        run++;
                    }
                } else {
                    while (j + run < nt && vars[b0 + j + run].first == vars[b0 + j].first + run) run++;
                    span = (uint64_t)run * R;
                }
                pread_span(pgen_fd.get(), dst + staged, (size_t)span, off0, pgen, opt.read_threads);
                staged += (size_t)span;
                j += run;
            }
            collect();   // block k - 1 has been counted and what it returns is back; its pinned records are free again
            check(pgenhip_memcpy_h2d(ctx.get(), d_rec, dst, staged), "H2D records");
            if (vw) check(pgenhip_memcpy_h2d(ctx.get(), d_off, h_off[k % 2], nt * sizeof(uint64_t)), "H2D record offsets");
            check(pgenhip_timer_start(ctx.get()), "timer");
            counter.launch(BlockRows{ctx.get(), d_rec, R, d_off}, b0, (uint32_t)nv, (uint32_t)nh, k == 0);
            check(pgenhip_timer_mark(ctx.get()), "timer");
            counter.copy(ctx.get(), nv);
            prev_b0 = b0;
            prev_nv = nv;
        }
        collect();
        counter.finish(ctx.get());
    });
    st.seconds_kernel = *std::max_element(kernel_s.begin(), kernel_s.end());
    st.seconds_setup = *std::max_element(setup_s.begin(), setup_s.end());
}

// what a counter inherits for the steps it has no use for
struct Counter {
    void copy(pgenhip_ctx *, size_t) const {}
    void collect(size_t, size_t) const {}
    void finish(pgenhip_ctx *) const {}
};

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
            genotype_counts(b, nv, d_gc);
            check(pgenhip_memcpy_d2h(ctx, h_gc, d_gc, (size_t)nv * 16), "D2H counts");
            check(pgenhip_wait(ctx), "pgenhip_wait");
            for (uint32_t j = 0; j < nv; j++) {
                const uint64_t c0 = h_gc[4 * j], c1 = h_gc[4 * j + 1], c2 = h_gc[4 * j + 2], called = c0 + c1 + c2;
                h_miss[j] = called ? (float)((double)(c1 + 2 * c2) / (double)called) : 0.f;
            }
            check(pgenhip_memcpy_h2d(ctx, d_miss, h_miss, (size_t)nv * sizeof(float)), "H2D mean dosages");
        }
        check(pgenhip_memcpy_h2d(ctx, d_w, w.data() + b0 * C, (size_t)nv * C * sizeof(float)), "H2D weights");
        const uint32_t acc = first ? 0u : PGENHIP_SCORE_ACCUMULATE;
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_SCORE_MAX_COLUMNS) {
            const uint32_t cg = (uint32_t)std::min<size_t>(PGENHIP_SCORE_MAX_COLUMNS, C - c0);
            double *dst = d_scores + K * c0;   // group g's K x cg block behind the blocks of the groups before it
            launch_rows(b, NAMED(pgenhip_sample_scores), NAMED(pgenhip_sample_scores_at), nv, d_w + c0, C, cg, impute ? d_miss : nullptr, dst,
                        PGENHIP_SCORE_AUTO | acc);
        }
        sample_counts(b, nv, d_counts, !first);
    }
    void finish(pgenhip_ctx *ctx) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_scores, d_scores, K * C * sizeof(double)), "D2H scores");
        check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, K * 16), "D2H counts");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        std::lock_guard<std::mutex> lk(mu);
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_SCORE_MAX_COLUMNS) {
            const size_t cg = std::min<size_t>(PGENHIP_SCORE_MAX_COLUMNS, C - c0);
            for (size_t k = 0; k < K; k++)
                for (size_t c = 0; c < cg; c++) sums[k * C + c0 + c] += h_scores[K * c0 + k * cg + c];
        }
        for (size_t k = 0; k < K; k++) missing[k] += h_counts[4 * k + 3];
    }
};

// assoc's counter: per block the rows' genotype counts and their per-code sums of every value column (Q's columns, then the
// residualised phenotypes; uploaded once per shard), sixteen columns per launch; both come back block by block.  Group g's sums of
// a block are bv x cg x 4 doubles behind those of the groups before it.
struct AssocCounter : Counter {
    size_t C, bv;                     // value columns, rows of a full block
    std::vector<uint32_t> &counts;    // 4 per kept variant
    std::vector<double> &sums;        // per kept variant C x 4
    const double *d_values;
    uint32_t *d_gc, *h_gc;
    double *d_sums, *h_sums;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const
    {
        genotype_counts(b, nv, d_gc);
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_VSUM_MAX_COLUMNS) {
            const uint32_t cg = (uint32_t)std::min<size_t>(PGENHIP_VSUM_MAX_COLUMNS, C - c0);
            launch_rows(b, NAMED(pgenhip_variant_sums), NAMED(pgenhip_variant_sums_at), nv, d_values + c0, C, cg, d_sums + bv * 4 * c0, PGENHIP_VSUM_AUTO);
        }
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_gc, d_gc, nv * 16), "D2H counts");
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_VSUM_MAX_COLUMNS) {
            const size_t cg = std::min<size_t>(PGENHIP_VSUM_MAX_COLUMNS, C - c0);
            check(pgenhip_memcpy_d2h(ctx, h_sums + bv * 4 * c0, d_sums + bv * 4 * c0, nv * cg * 4 * sizeof(double)), "D2H sums");
        }
    }
    void collect(size_t b0, size_t nv) const
    {
        std::memcpy(counts.data() + 4 * b0, h_gc, nv * 16);
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_VSUM_MAX_COLUMNS) {
            const size_t cg = std::min<size_t>(PGENHIP_VSUM_MAX_COLUMNS, C - c0);
            const double *src = h_sums + bv * 4 * c0;
            for (size_t j = 0; j < nv; j++) std::memcpy(sums.data() + ((b0 + j) * C + c0) * 4, src + j * cg * 4, cg * 4 * sizeof(double));
        }
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
        char num[32];
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
                std::snprintf(num, sizeof num, "%.6g", (double)r2);
                text += num;
                if (ld.counts) {
                    text += '\t';
                    append_u64(text, n_obs);
                    for (int c = 0; c < 16; c++) {
                        text += '\t';
                        append_u64(text, t[c]);
                    }
                }
                text += '\n';
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        pieces.emplace(b0, std::move(text));
    }
};

// The upper block triangle of a K x K table of sample pairs, cut into square tiles of `tile` ranks: the pairs of tiles (ta, tb),
// ta <= tb, row-major over ta, tb.  That is the order of kinship's and grm's device buffers, of their launches and copies, and of
// the host's vectors.
struct TileTriangle {
    uint32_t K, tile;
    uint32_t tiles() const { return (uint32_t)(((uint64_t)K + tile - 1) / tile); }
    size_t count(uint32_t t) const { return std::min(tile, K - t * tile); }   // ranks of tile t
    size_t pair(size_t ta, size_t tb) const { return ta * tiles() - ta * (ta - 1) / 2 + (tb - ta); }   // (ta, tb)'s place in that order
    template <class Fn>
    void each_pair(const Fn &fn) const   // fn(ta, tb) in that order
    {
        for (uint32_t ta = 0; ta < tiles(); ta++)
            for (uint32_t tb = ta; tb < tiles(); tb++) fn(ta, tb);
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
    std::map<size_t, std::vector<std::vector<double>>> &sums;   // shard's first variant -> per pair of tiles, G at 2 p, N at 2 p + 1
    std::mutex &mu;
    uint64_t &skipped;
    std::vector<double *> bufs;                              // device: count(ta) x count(tb) doubles, in the order of `sums`' vectors
    uint32_t *d_counts, *h_counts;
    double *d_tab, *h_tab, *h_buf;                           // h_buf: pinned, the largest buffer's size
    size_t first_b0 = 0;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t, bool first)
    {
        pgenhip_ctx *ctx = b.ctx;
        genotype_counts(b, nv, d_counts);
        check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, (size_t)nv * 16), "D2H counts");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        uint64_t zero_tables = 0;
        for (size_t j = 0; j < nv; j++) {
            const uint64_t c0 = h_counts[4 * j], c1 = h_counts[4 * j + 1], c2 = h_counts[4 * j + 2];
            const uint64_t called = c0 + c1 + c2, alt = c1 + 2 * c2;
            double *g = h_tab + 4 * j, *n = h_tab + 4 * (bv + j);
            if (called == 0 || alt == 0 || alt == 2 * called) {   // no call, p == 0 or p == 1: the variant adds nothing
                for (int x = 0; x < 4; x++) g[x] = n[x] = 0.0;
                zero_tables++;
                continue;
            }
            const double p = (double)alt / (2.0 * (double)called);
            const double s = 1.0 / std::sqrt(2.0 * p * (1.0 - p));
            g[0] = (0.0 - 2.0 * p) * s;
            g[1] = (1.0 - 2.0 * p) * s;
            g[2] = (2.0 - 2.0 * p) * s;
            g[3] = 0.0;
            n[0] = n[1] = n[2] = 1.0;
            n[3] = 0.0;
        }
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
    void finish(pgenhip_ctx *ctx) const   // (count_blocks has launched at least one block: Shards::run skips a shard without variants)
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
        std::lock_guard<std::mutex> lk(mu);
        sums.emplace(first_b0, std::move(mine));
    }
};

// pca's counter of one pass: Q (K x L) goes up once per shard; per block the rows' tables go up and every group of at most sixteen
// columns gets one Gram product into the shard's K x L doubles (the first block overwrites, the others accumulate); they come back
// once per shard, filed under the shard's first variant so that the host can add the shards in order
struct PcaCounter : Counter {
    size_t K, L;
    const std::vector<double> &tables;                 // 4 per kept variant
    std::map<size_t, std::vector<double>> &sums;       // shard's first variant -> K x L
    std::mutex &mu;
    double *d_q, *d_y, *d_proj, *d_tab, *h_y;
    size_t first_b0 = 0;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t, bool first)
    {
        check(pgenhip_memcpy_h2d(b.ctx, d_tab, tables.data() + 4 * b0, (size_t)nv * 32), "H2D code values");
        const uint32_t flags = PGENHIP_GAPPLY_AUTO | (first ? 0u : PGENHIP_GAPPLY_ACCUMULATE);
        if (first) first_b0 = b0;
        for (size_t c0 = 0; c0 < L; c0 += PGENHIP_GAPPLY_MAX_COLUMNS) {
            const uint32_t cg = (uint32_t)std::min<size_t>(PGENHIP_GAPPLY_MAX_COLUMNS, L - c0);
            launch_rows(b, NAMED(pgenhip_gram_apply), NAMED(pgenhip_gram_apply_at), nv, (const double *)d_tab, (const double *)(d_q + c0), (uint64_t)L, cg,
                        d_proj, d_y + c0, (uint64_t)L, flags);
        }
    }
    void finish(pgenhip_ctx *ctx) const   // (count_blocks has launched at least one block)
    {
        check(pgenhip_memcpy_d2h(ctx, h_y, d_y, K * L * 8), "D2H Gram product");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        std::lock_guard<std::mutex> lk(mu);
        sums.emplace(first_b0, std::vector<double>(h_y, h_y + K * L));
    }
};

// splitmix64: the next state's output
uint64_t splitmix64(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

OutputStats Pfile::output_freq(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                               const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const IdxRecords &var_idx_rcds = sel.var_idx_rcds;
    // the five leading columns, copied verbatim from the pvar columns of these names
    static const char *const kCols[5] = {"CHROM", "POS", "ID", "REF", "ALT"};
    size_t col[5];
    for (int c = 0; c < 5; c++) col[c] = column(sel.var_header, kCols[c], pvar_path());
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = var_idx_rcds.size();
    st.variants = V;
    st.samples_kept = kept.rows.size();

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
        const StringRecord &r = var_idx_rcds[j].second;
        for (int c = 0; c < 5; c++) {
            text += r.at(col[c]);
            text += '\t';
        }
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
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;

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
    const std::string data = read_file(path);
    ScoreWeights sw;
    TsvReader reader(data, !data.empty() && data[0] == '#' ? 1 : 0);
    const StringRecord &head = reader.headers();
    if (head.size() < 3) throw PfileError(path + " line 1: a weights file has an ID column, an effect allele column and at least one score column");
    sw.names.assign(head.begin() + 2, head.end());
    const size_t C = sw.names.size();
    // the line a record starts on: the newlines in front of it, counted as the reader moves on
    size_t counted = 0, line = 1;
    auto line_at = [&](size_t pos) {
        for (; counted < pos; counted++) line += data[counted] == '\n';
        for (size_t p = pos; p < data.size() && (data[p] == '\n' || data[p] == '\r'); p++) {   // the empty lines the reader skips
            line += data[p] == '\n';
            counted = p + 1;
        }
        return line;
    };
    std::map<std::string, size_t> seen;   // ID -> line
    StringRecord rec;
    for (;;) {
        const size_t at = line_at(reader.position());
        bool more;
        try {
            more = reader.next(rec);
        } catch (const CsvError &) {
            throw PfileError(path + " line " + std::to_string(at) + ": expected " + std::to_string(C + 2) + " tab-separated cells like the header's");
        }
        if (!more) break;
        const auto dup = seen.emplace(rec[0], at);
        if (!dup.second)
            throw PfileError(path + " line " + std::to_string(at) + ": variant ID '" + rec[0] + "' occurs twice (first on line " + std::to_string(dup.first->second) + ")");
        for (size_t c = 0; c < C; c++) {
            const std::string &cell = rec[2 + c];
            char *end = nullptr;
            errno = 0;
            const double x = std::strtod(cell.c_str(), &end);
            const bool fits = std::isfinite(x) && std::fabs(x) < 0x1.ffffffp127;   // rounds to a finite f32
            const float f = fits ? (float)x : 0.f;                                   // rounded to f32 once, here
            if (cell.empty() || *end != '\0' || !fits)
                throw PfileError(path + " line " + std::to_string(at) + ": weight '" + cell + "' of score " + sw.names[c] + " is not a finite number");
            sw.w.push_back(f);
        }
        sw.ids.push_back(rec[0]);
        sw.alleles.push_back(rec[1]);
        sw.lines.push_back(at);
    }
    return sw;
}

OutputStats Pfile::output_score(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                const std::string &weights_file, const std::string &filename, const ScoreOptions &sopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const ScoreWeights sw = read_score_weights(weights_file);
    const size_t C = sw.names.size();
    Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    static const char *const kCols[3] = {"ID", "REF", "ALT"};
    size_t col[3];
    for (int c = 0; c < 3; c++) col[c] = column(sel.var_header, kCols[c], pvar_path());

    // the kept variants the file names, in the .pgen's order: they are the selection of every launch
    std::map<std::string, size_t> row_of;
    for (size_t i = 0; i < sw.ids.size(); i++) row_of.emplace(sw.ids[i], i);
    std::vector<char> used(sw.ids.size(), 0);
    Selection msel;
    std::vector<float> w;                 // matched rows x C, REF-effect rows negated
    std::vector<double> constant(C, 0.0); // the 2w of the REF-effect rows, added to every sample
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
        msel.var_idx_rcds.emplace_back(vr.first, StringRecord());
    }
    const size_t M = msel.var_idx_rcds.size();
    st.score_matched = M;
    st.score_flipped = flipped;
    st.score_skipped = sw.ids.size() - M;
    if (M == 0)
        throw PfileError("no row of " + weights_file + " names a kept variant of " + pvar_path() + " by ID with its REF or ALT allele (" +
                         std::to_string(sw.ids.size()) + " rows, " + std::to_string(mismatched) + " with another allele)");
    msel.sam_idx_rcs = std::move(sel.sam_idx_rcs);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, msel);
    const size_t K = kept.rows.size();
    st.variants = M;
    st.samples_kept = K;

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
    char buf[64];
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
            if (sopt.average && denom == 0) {
                text += "nan";
            } else {
                std::snprintf(buf, sizeof buf, "%.12g", sopt.average ? sum / (double)denom : sum);
                text += buf;
            }
        }
        text += '\n';
    }
    finish_text(st, text, filename, t_body);
    return st;
}

ValueTable read_value_table(const std::string &path)
{
    const std::string data = read_file(path);
    ValueTable vt;
    TsvReader reader(data, !data.empty() && data[0] == '#' ? 1 : 0);
    const StringRecord &head = reader.headers();
    if (head.size() < 2) throw PfileError(path + " line 1: a value file has an IID column and at least one value column");
    vt.names.assign(head.begin() + 1, head.end());
    const size_t C = vt.names.size();
    // the line a record starts on: the newlines in front of it, counted as the reader moves on
    size_t counted = 0, line = 1;
    auto line_at = [&](size_t pos) {
        for (; counted < pos; counted++) line += data[counted] == '\n';
        for (size_t p = pos; p < data.size() && (data[p] == '\n' || data[p] == '\r'); p++) {   // the empty lines the reader skips
            line += data[p] == '\n';
            counted = p + 1;
        }
        return line;
    };
    std::map<std::string, size_t> seen;   // IID -> line
    StringRecord rec;
    for (;;) {
        const size_t at = line_at(reader.position());
        bool more;
        try {
            more = reader.next(rec);
        } catch (const CsvError &) {
            throw PfileError(path + " line " + std::to_string(at) + ": expected " + std::to_string(C + 1) + " tab-separated cells like the header's");
        }
        if (!more) break;
        const auto dup = seen.emplace(rec[0], at);
        if (!dup.second)
            throw PfileError(path + " line " + std::to_string(at) + ": IID '" + rec[0] + "' occurs twice (first on line " + std::to_string(dup.first->second) + ")");
        for (size_t c = 0; c < C; c++) {
            const std::string &cell = rec[1 + c];
            if (cell.empty() || cell == "NA" || cell == "nan") {
                vt.x.push_back(std::nan(""));
                continue;
            }
            char *end = nullptr;
            const double x = std::strtod(cell.c_str(), &end);
            if (*end != '\0' || !std::isfinite(x))
                throw PfileError(path + " line " + std::to_string(at) + ": value '" + cell + "' of column " + vt.names[c] + " is not a finite number, NA or nan");
            vt.x.push_back(x);
        }
        vt.iids.push_back(rec[0]);
    }
    return vt;
}

namespace {

// ln Gamma(a + 1/2) - ln Gamma(a): the difference of two lgamma values loses 1e-16 of their size (6e6 at a = 5e5), so from a = 64 on
// the asymptotic series of the ratio itself
double lgamma_half_step(double a)
{
    if (a < 64.0) return std::lgamma(a + 0.5) - std::lgamma(a);
    const double i = 1.0 / a, i2 = i * i;
    return 0.5 * std::log(a) + i * (-1.0 / 8.0 + i2 * (1.0 / 192.0 + i2 * (-1.0 / 640.0 + i2 * (17.0 / 14336.0))));
}

// the continued fraction of the incomplete beta function by the modified Lentz method
double beta_cf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 100000; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

}  // namespace

double student_t_two_sided_p(double t, double df)
{
    if (std::isnan(t) || std::isnan(df) || df <= 0.0) return std::nan("");
    if (std::isinf(t)) return 0.0;
    if (t == 0.0) return 1.0;
    const double a = 0.5 * df, b = 0.5, t2 = t * t;
    const double x = df / (df + t2), y = t2 / (df + t2);                 // y = 1 - x without the cancellation
    // ln of x^a y^b / B(a, b): a ln x = -a log1p(t^2 / df); B(a, 1/2) = Gamma(a) sqrt(pi) / Gamma(a + 1/2)
    const double front = std::exp(lgamma_half_step(a) - 0.5 * std::log(M_PI) - a * std::log1p(t2 / df) + b * std::log(y));
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
    return 1.0 - front * beta_cf(b, a, y) / b;
}

OutputStats Pfile::output_assoc(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                const AssocOptions &aopt, const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const ValueTable ph = read_value_table(aopt.pheno_file);
    ValueTable cv;
    if (!aopt.covar_file.empty()) cv = read_value_table(aopt.covar_file);
    std::vector<size_t> pcol;   // the chosen phenotype columns
    if (aopt.pheno_names.empty()) {
        for (size_t c = 0; c < ph.names.size(); c++) pcol.push_back(c);
    } else {
        for (const std::string &name : aopt.pheno_names) {
            const size_t c = std::find(ph.names.begin(), ph.names.end(), name) - ph.names.begin();
            if (c == ph.names.size()) throw PfileError(aopt.pheno_file + " line 1: no phenotype column named '" + name + "'");
            pcol.push_back(c);
        }
    }
    const size_t P = pcol.size(), ncov = cv.names.size(), m = 1 + ncov, C = m + P;

    Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    static const char *const kCols[5] = {"CHROM", "POS", "ID", "REF", "ALT"};
    size_t col[5];
    for (int c = 0; c < 5; c++) col[c] = column(sel.var_header, kCols[c], pvar_path());

    // complete cases: a kept sample stays only with every chosen phenotype and every covariate
    std::map<std::string, size_t> ph_row, cv_row;
    for (size_t i = 0; i < ph.iids.size(); i++) ph_row.emplace(ph.iids[i], i);
    for (size_t i = 0; i < cv.iids.size(); i++) cv_row.emplace(cv.iids[i], i);
    IdxRecords stay;
    std::vector<double> y, x;   // n x P phenotypes, n x ncov covariates
    for (auto &sr : sel.sam_idx_rcs) {
        const auto pi = ph_row.find(sr.second.at(iid));
        const auto ci = ncov ? cv_row.find(sr.second.at(iid)) : cv_row.end();
        bool complete = pi != ph_row.end() && (!ncov || ci != cv_row.end());
        for (size_t p = 0; complete && p < P; p++) complete = !std::isnan(ph.x[pi->second * ph.names.size() + pcol[p]]);
        for (size_t c = 0; complete && c < ncov; c++) complete = !std::isnan(cv.x[ci->second * ncov + c]);
        if (!complete) continue;
        for (size_t p = 0; p < P; p++) y.push_back(ph.x[pi->second * ph.names.size() + pcol[p]]);
        for (size_t c = 0; c < ncov; c++) x.push_back(cv.x[ci->second * ncov + c]);
        stay.push_back(std::move(sr));
    }
    st.assoc_dropped = sel.sam_idx_rcs.size() - stay.size();
    sel.sam_idx_rcs = std::move(stay);
    const size_t n = sel.sam_idx_rcs.size();
    if (n == 0) throw PfileError("no kept sample has every chosen phenotype of " + aopt.pheno_file + (ncov ? " and every covariate of " + aopt.covar_file : std::string()));
    if (n < m + 2)
        throw PfileError("too few samples: " + std::to_string(n) + " complete samples leave " + std::to_string((long long)n - (long long)m - 1) +
                         " degrees of freedom for an intercept, " + std::to_string(ncov) + " covariates and the genotype");
    const double df = (double)(n - m - 1);

    // the value columns, n x C: Q's m columns (modified Gram-Schmidt, applied twice), then the residualised phenotypes
    std::vector<double> values(n * C, 0.0);
    auto at = [&](size_t k, size_t c) -> double & { return values[k * C + c]; };
    auto project_out = [&](size_t c, size_t upto) {   // column c minus its parts along columns [0, upto), twice
        for (int pass = 0; pass < 2; pass++)
            for (size_t q = 0; q < upto; q++) {
                double dot = 0.0;
                for (size_t k = 0; k < n; k++) dot += at(k, q) * at(k, c);
                for (size_t k = 0; k < n; k++) at(k, c) -= dot * at(k, q);
            }
    };
    auto norm = [&](size_t c) {
        double ss = 0.0;
        for (size_t k = 0; k < n; k++) ss += at(k, c) * at(k, c);
        return std::sqrt(ss);
    };
    for (size_t c = 0; c < m; c++) {
        for (size_t k = 0; k < n; k++) at(k, c) = c == 0 ? 1.0 : x[k * ncov + (c - 1)];
        const double before = norm(c);
        project_out(c, c);
        const double after = norm(c);
        if (!(after > 1e-10 * before))
            throw PfileError(aopt.covar_file + ": covariate " + (c ? cv.names[c - 1] : std::string("(intercept)")) + " is collinear with the intercept and the covariates before it");
        for (size_t k = 0; k < n; k++) at(k, c) /= after;
    }
    std::vector<double> rr(P, 0.0);
    for (size_t p = 0; p < P; p++) {
        for (size_t k = 0; k < n; k++) at(k, m + p) = y[k * P + p];
        project_out(m + p, m);
        for (size_t k = 0; k < n; k++) rr[p] += at(k, m + p) * at(k, m + p);
    }
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size();
    st.variants = V;
    st.samples_kept = n;

    std::vector<uint32_t> counts(4 * V, 0u);
    std::vector<double> sums(V * C * 4, 0.0);
    const double t_body = now_s();
    if (V != 0) {   // else the header alone and no device is touched
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the assoc path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            double *d_values = ctx.device<double>(n * C * sizeof(double), "device values");
            check(pgenhip_memcpy_h2d(ctx.get(), d_values, values.data(), n * C * sizeof(double)), "H2D values");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            return AssocCounter{{}, C, b, counts, sums, d_values,
                                ctx.device<uint32_t>(16 * b, "device variant counts"), ctx.pinned<uint32_t>(16 * b, "pinned variant counts"),
                                ctx.device<double>(b * C * 4 * sizeof(double), "device sums"), ctx.pinned<double>(b * C * 4 * sizeof(double), "pinned sums")};
        });
    }

    std::string text = "#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tP\n";
    st.header_bytes = text.size();
    char buf[64];
    auto number = [&](double v) {
        std::snprintf(buf, sizeof buf, "%.12g", v);
        text += '\t';
        text += buf;
    };
    for (size_t j = 0; j < V; j++) {
        const StringRecord &vr = sel.var_idx_rcds[j].second;
        const double c1 = counts[4 * j + 1], c2 = counts[4 * j + 2], c3 = counts[4 * j + 3], called = (double)counts[4 * j] + c1 + c2;
        const double mu = called > 0 ? (c1 + 2.0 * c2) / called : 0.0;
        const double *S = sums.data() + j * C * 4;
        auto tv = [&](size_t c) { return S[4 * c + 1] + 2.0 * S[4 * c + 2] + mu * S[4 * c + 3]; };
        const double gg = c1 + 4.0 * c2 + mu * mu * c3;
        double denom = gg;
        for (size_t q = 0; q < m; q++) denom -= tv(q) * tv(q);
        for (size_t p = 0; p < P; p++) {
            for (int c = 0; c < 5; c++) {
                if (c) text += '\t';
                text += vr.at(col[c]);
            }
            text += '\t';
            text += vr.at(col[4]);
            text += '\t';
            text += ph.names[pcol[p]];
            text += '\t';
            append_u64(text, n);
            text += '\t';
            append_u64(text, counts[4 * j + 3]);
            if (called > 0) number(0.5 * mu);
            else text += "\tNA";
            const double b = tv(m + p);
            const double rss = rr[p] - b * b / denom;
            if (!(called > 0) || !(denom > 1e-12 * gg) || !(rss > 0)) {
                text += "\tNA\tNA\tNA\tNA\n";
                continue;
            }
            const double beta = b / denom, se = std::sqrt(rss / df / denom), tstat = beta / se;
            number(beta);
            number(se);
            number(tstat);
            number(student_t_two_sided_p(tstat, df));
            text += '\n';
        }
    }
    finish_text(st, text, filename, t_body);
    return st;
}

OutputStats Pfile::output_ld(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                             const std::string &filename, const LdOptions &ld, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    static const char *const kCols[3] = {"CHROM", "POS", "ID"};
    size_t col[3];
    for (int c = 0; c < 3; c++) col[c] = column(sel.var_header, kCols[c], pvar_path());
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;

    std::string text = "#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tR2";
    if (ld.counts) {
        text += "\tN_OBS";
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) text += std::string("\tT") + (char)('0' + a) + (char)('0' + b);
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
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;

    std::string text = "#IID1\tIID2\tN\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP";
    if (kopt.counts) {
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) text += std::string("\tT") + (char)('0' + a) + (char)('0' + b);
    }
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
        char num[32];
        for (size_t a = 0; a < K; a++) {
            const size_t ta = a / tile, i = a % tile;
            for (size_t b = a + 1; b < K; b++) {
                const size_t tb = b / tile, l = b % tile;
                const uint32_t *t = totals[tri.pair(ta, tb)].data() + 16 * (i * tri.count((uint32_t)tb) + l);
                uint64_t n = 0;
                for (int x = 0; x < 3; x++)
                    for (int y = 0; y < 3; y++) n += t[4 * x + y];
                const uint64_t hethet = t[5], ibs0 = (uint64_t)t[2] + t[8], het1 = (uint64_t)t[4] + t[5] + t[6], het2 = (uint64_t)t[1] + t[5] + t[9];
                const uint64_t hmin = std::min(het1, het2);
                const double kin = hmin == 0 ? std::nan("") : 0.5 - ((double)(het1 + het2 - 2 * hethet) + 4.0 * (double)ibs0) / (4.0 * (double)hmin);
                if (kopt.has_min && !(kin >= kopt.min_kinship)) continue;   // nan lines go with the ones below the floor
                text += sel.sam_idx_rcs[a].second.at(iid);
                text += '\t';
                text += sel.sam_idx_rcs[b].second.at(iid);
                for (const uint64_t v : {n, hethet, ibs0, het1, het2}) {
                    text += '\t';
                    append_u64(text, v);
                }
                text += '\t';
                if (hmin == 0) {
                    text += "nan";
                } else {
                    std::snprintf(num, sizeof num, "%.6g", kin);
                    text += num;
                }
                if (kopt.counts) {
                    for (int c = 0; c < 16; c++) {
                        text += '\t';
                        append_u64(text, t[c]);
                    }
                }
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
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;
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
        std::map<size_t, std::vector<std::vector<double>>> sums;
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
        for (const auto &shard : sums)   // ordered by the shard's first variant
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
        char num[40];
        for (size_t a = 0; a < K; a++)
            for (size_t b = 0; b < K; b++) {
                const double v = grm(a, b);
                if (std::isnan(v)) {
                    text += "nan";
                } else {
                    std::snprintf(num, sizeof num, "%.17g", v);
                    text += num;
                }
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
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t iid = iid_column(*this, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size(), P = popt.pcs;
    st.variants = V;
    st.samples_kept = K;
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
        const uint64_t c0 = counts[4 * j], c1 = counts[4 * j + 1], c2 = counts[4 * j + 2];
        const uint64_t called = c0 + c1 + c2, alt = c1 + 2 * c2;
        if (called == 0 || alt == 0 || alt == 2 * called) {   // no call, p == 0 or p == 1: the variant adds nothing
            st.pca_skipped++;
            continue;
        }
        const double p = (double)alt / (2.0 * (double)called);
        const double s = 1.0 / std::sqrt(2.0 * p * (1.0 - p));
        double *g = tables.data() + 4 * j;
        g[0] = (0.0 - 2.0 * p) * s;
        g[1] = (1.0 - 2.0 * p) * s;
        g[2] = (2.0 - 2.0 * p) * s;
    }
    const size_t V_used = V - (size_t)st.pca_skipped;
    if (V_used == 0) return write_out("", "");

    // the start: a seeded Gaussian K x L matrix, orthonormalised
    const size_t L = std::min(K, P + 10);
    std::vector<double> Q(K * L), Y(K * L), U(K * L), T(L * L), W, lambda;
    uint64_t state = popt.seed;
    for (double &x : Q) {
        const double u1 = (double)((splitmix64(state) >> 11) + 1) * 0x1p-53, u2 = (double)(splitmix64(state) >> 11) * 0x1p-53;
        x = std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
    }
    linalg::qr_thin(Q, K, L);

    double kernel_s = 0, setup_s = 0;
    for (;;) {
        // Y = M Q
        std::mutex mu;
        std::map<size_t, std::vector<double>> sums;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            PcaCounter pc{{}, K, L, tables, sums, mu, ctx.device<double>(K * L * 8, "device Q"), ctx.device<double>(K * L * 8, "device Gram product"),
                          ctx.device<double>((size_t)(bv * PGENHIP_GAPPLY_MAX_COLUMNS * 8), "device projections"),
                          ctx.device<double>((size_t)(bv * 32), "device code values"), ctx.pinned<double>(K * L * 8, "pinned Gram product")};
            check(pgenhip_memcpy_h2d(ctx.get(), pc.d_q, Q.data(), K * L * 8), "H2D Q");
            return pc;
        }, popt.block_rows);
        kernel_s += st.seconds_kernel;
        setup_s += st.seconds_setup;
        std::fill(Y.begin(), Y.end(), 0.0);
        for (const auto &shard : sums)   // ordered by the shard's first variant
            for (size_t i = 0; i < K * L; i++) Y[i] += shard.second[i];
        for (double &y : Y) y /= (double)V_used;
        st.pca_passes++;

        // Rayleigh-Ritz: T = Q^T Y symmetrised = W Lambda W^T, U = Q W, residuals of the first P pairs
        for (size_t a = 0; a < L; a++)
            for (size_t b = 0; b < L; b++) {
                double dot = 0.0;
                for (size_t k = 0; k < K; k++) dot += Q[k * L + a] * Y[k * L + b];
                T[a * L + b] = dot;
            }
        for (size_t a = 0; a < L; a++)
            for (size_t b = a + 1; b < L; b++) T[a * L + b] = T[b * L + a] = 0.5 * (T[a * L + b] + T[b * L + a]);
        linalg::jacobi_eigh(T, L, lambda, W);
        double worst = 0.0;
        for (size_t i = 0; i < L; i++) {
            double rr = 0.0;
            for (size_t k = 0; k < K; k++) {
                double u = 0.0, yw = 0.0;
                for (size_t a = 0; a < L; a++) {
                    u += Q[k * L + a] * W[a * L + i];
                    yw += Y[k * L + a] * W[a * L + i];
                }
                U[k * L + i] = u;
                const double r = yw - lambda[i] * u;
                rr += r * r;
            }
            if (i < P) worst = std::max(worst, std::sqrt(rr));
        }
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
    char num[40];
    for (size_t i = 0; i < P; i++) {
        std::snprintf(num, sizeof num, "%.17g\n", lambda[i]);
        vals += num;
    }
    // unit norm, the largest-magnitude entry positive
    std::vector<double> scale(P, 1.0);
    for (size_t i = 0; i < P; i++) {
        double ss = 0.0, big = 0.0;
        for (size_t k = 0; k < K; k++) {
            ss += U[k * L + i] * U[k * L + i];
            if (std::fabs(U[k * L + i]) > std::fabs(big)) big = U[k * L + i];
        }
        scale[i] = (big < 0.0 ? -1.0 : 1.0) / (ss > 0.0 ? std::sqrt(ss) : 1.0);
    }
    for (size_t k = 0; k < K; k++) {
        vecs += sel.sam_idx_rcs[k].second.at(iid);
        for (size_t i = 0; i < P; i++) {
            std::snprintf(num, sizeof num, "\t%.17g", U[k * L + i] * scale[i]);
            vecs += num;
        }
        vecs += '\n';
    }
    return write_out(vals, vecs);
}

OutputStats Pfile::output_matrix(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                 const std::string &filename, const MatrixOptions &mopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const size_t id_col = column(sel.var_header, "ID", pvar_path()), iid_col = iid_column(*this, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size(), E = mopt.elem_bytes;
    st.variants = V;
    st.samples_kept = K;

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

OutputStats Pfile::output_export(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                 const std::string &out_prefix, const ExportOptions &eopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const std::string out_main = out_prefix + (eopt.bed ? ".bed" : ".pgen");
    const std::string out_var = out_prefix + (eopt.bed ? ".bim" : ".pvar"), out_sam = out_prefix + (eopt.bed ? ".fam" : ".psam");
    if (!eopt.bed) {   // the same file by another spelling or through a link is still the input
        std::error_code ec1, ec2;
        const auto in = std::filesystem::weakly_canonical(pgen_path(), ec1), out = std::filesystem::weakly_canonical(out_main, ec2);
        if (out_main == pgen_path() || (!ec1 && !ec2 && in == out))
            throw PfileError("export would overwrite its input: " + out_main + " is " + pgen_path());
    }
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    auto optional_column = [](const StringRecord &header, const char *name) {   // header.size(): the file has none
        return (size_t)(std::find(header.begin(), header.end(), std::string(name)) - header.begin());
    };
    auto join_rows = [](std::string &text, const IdxRecords &rows) {
        for (const auto &ir : rows) {
            for (size_t c = 0; c < ir.second.size(); c++) {
                if (c) text += '\t';
                text += ir.second[c];
            }
            text += '\n';
        }
    };
    std::string var_text, sam_text;
    if (eopt.bed) {
        const StringRecord &vh = sel.var_header, &sh = sel.sam_header;
        const size_t chrom = column(vh, "CHROM", pvar_path()), id = column(vh, "ID", pvar_path()), pos = column(vh, "POS", pvar_path()),
                     ref = column(vh, "REF", pvar_path()), alt = column(vh, "ALT", pvar_path());
        for (const auto &vr : sel.var_idx_rcds) {
            const StringRecord &r = vr.second;
            if (r.at(alt).find(',') != std::string::npos)
                throw PfileError("variant " + r.at(id) + " (row " + std::to_string(vr.first) + " of " + pvar_path() + ") has more than one ALT allele (" +
                                 r.at(alt) + "): a .bed holds biallelic variants only");
            var_text += r.at(chrom) + '\t' + r.at(id) + "\t0\t" + r.at(pos) + '\t' + r.at(alt) + '\t' + r.at(ref) + '\n';
        }
        const size_t iid = iid_column(*this, sh), fid = optional_column(sh, "FID"), pat = optional_column(sh, "PAT"), mat = optional_column(sh, "MAT"),
                     sex = optional_column(sh, "SEX");
        for (const auto &sr : sel.sam_idx_rcs) {
            const StringRecord &r = sr.second;
            auto or_zero = [&](size_t c) { return c == sh.size() ? std::string("0") : r.at(c); };
            const std::string sx = sex == sh.size() ? std::string("0") : r.at(sex);
            sam_text += or_zero(fid) + '\t' + r.at(iid) + '\t' + or_zero(pat) + '\t' + or_zero(mat) + '\t' + (sx == "1" || sx == "2" ? sx : std::string("0")) + "\t-9\n";
        }
    } else {
        const auto [pvar_header, pvar_column_names] = read_pvar_header();
        var_text = pvar_header + pvar_column_names;
        if (!var_text.empty() && var_text.back() != '\n') var_text += '\n';
        join_rows(var_text, sel.var_idx_rcds);
        const std::string psam = read_file(psam_path());
        const size_t eol = psam.find('\n', (size_t)find_metadata_file_header_start(psam));
        sam_text = eol == std::string::npos ? psam + "\n" : psam.substr(0, eol + 1);
        join_rows(sam_text, sel.sam_idx_rcs);
    }
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size(), RK = (K + 3) / 4;
    st.variants = V;
    st.samples_kept = K;
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
        count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t bytes = (size_t)(bv * RK);
            return PackWriter{{}, RK, eopt.bed ? kBedMap : nullptr, ctx.device<uint8_t>(bytes, "device packed records"),
                              ctx.pinned<uint8_t>(bytes, "pinned packed records"), out.get(), out_main, (uint64_t)header.size()};
        });
    }
    out.close();
    write_text(var_text, out_var);
    write_text(sam_text, out_sam);
    st.seconds_body = now_s() - t_body;
    return st;
}

// ---- import: VCF -> .pgen / .pvar / .psam ----------------------------------------------------------------------------------------------
namespace {

// The input's bytes in order: a plain file, or (first bytes 1F 8B) ONE zlib stream that goes on into the next gzip member when one
// ends, which reads bgzip's files and this tool's own `-o x.vcf.gz` as well as plain gzip.  (The members of a BGZF file could be
// inflated side by side; that is not built.)
class VcfSource {
  public:
    explicit VcfSource(const std::string &path) : path_(path), fd_(path, O_RDONLY)
    {
        uint8_t magic[2] = {0, 0};
        gz_ = ::pread(fd_.get(), magic, 2, 0) == 2 && magic[0] == 0x1F && magic[1] == 0x8B;
        if (gz_) {
            std::memset(&z_, 0, sizeof z_);
            if (inflateInit2(&z_, 15 + 16) != Z_OK) throw PfileError("inflateInit2 failed for " + path_);
            in_.resize(1u << 20);
        }
    }
    VcfSource(const VcfSource &) = delete;
    VcfSource &operator=(const VcfSource &) = delete;
    ~VcfSource()
    {
        if (gz_) inflateEnd(&z_);
    }
    // up to cap bytes; fewer only at the end of the input
    size_t read(uint8_t *dst, size_t cap)
    {
        size_t got = 0;
        while (got < cap && !eof_) {
            if (!gz_) {
                const size_t r = read_fd(dst + got, cap - got);
                if (r == 0) eof_ = true;
                got += r;
                continue;
            }
            if (z_.avail_in == 0) {
                const size_t r = read_fd(in_.data(), in_.size());
                if (r == 0) {
                    if (mid_member_) throw PfileError(path_ + ": the gzip stream ends inside a member");
                    eof_ = true;
                    break;
                }
                z_.next_in = in_.data();
                z_.avail_in = (uInt)r;
            }
            const size_t room = std::min<size_t>(cap - got, 1u << 30);
            z_.next_out = dst + got;
            z_.avail_out = (uInt)room;
            const int rc = inflate(&z_, Z_NO_FLUSH);
            got += room - z_.avail_out;
            if (rc == Z_STREAM_END) {   // the next member, if any bytes follow
                if (inflateReset(&z_) != Z_OK) throw PfileError("inflateReset failed for " + path_);
                mid_member_ = false;
            } else if (rc == Z_OK || rc == Z_BUF_ERROR) {
                mid_member_ = true;
            } else {
                throw PfileError(path_ + ": not a gzip stream (" + (z_.msg ? z_.msg : "inflate failed") + ")");
            }
        }
        return got;
    }

  private:
    size_t read_fd(uint8_t *dst, size_t cap)
    {
        for (;;) {
            const ssize_t r = ::read(fd_.get(), dst, cap);
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) throw PfileError("read " + path_ + ": " + std::strerror(errno));
            return (size_t)r;
        }
    }
    std::string path_;
    Fd fd_;
    bool gz_ = false, eof_ = false, mid_member_ = false;
    z_stream z_;
    std::vector<uint8_t> in_;
};

// a block of whole lines as the reader hands it over: the text and the kept lines' offsets lie in the slot's pinned buffers
struct ImportBlock {
    size_t text_len = 0, n = 0;
    std::vector<uint64_t> line_no;   // of the kept lines, 1-based in the input
    std::string pvar;                // their columns in front of FORMAT
    uint64_t skipped = 0;
    std::string error;               // the reader's first error: what() of the command
    bool last = false;
};

template <class F>
struct Finally {
    F f;
    ~Finally() { f(); }
};
template <class F>
Finally(F) -> Finally<F>;

std::string import_line_error(const std::string &path, uint64_t line, const std::string &what)
{
    return path + ": line " + std::to_string(line) + ": " + what;
}

}  // namespace

OutputStats import_vcf(const std::string &in_path, const std::string &out_prefix, const ImportOptions &iopt, const OutputOptions &opt)
{
    OutputStats st;
    const double t0 = now_s();
    VcfSource src(in_path);

    // the header: ## lines, then the #CHROM line; `carry` keeps what has been read behind it
    std::vector<uint8_t> carry;
    std::string pvar_text, columns;
    uint64_t header_lines = 0;
    {
        size_t pos = 0;
        bool eof = false;
        for (;;) {
            const uint8_t *nl = pos < carry.size() ? static_cast<const uint8_t *>(std::memchr(carry.data() + pos, '\n', carry.size() - pos)) : nullptr;
            if (!nl && !eof) {
                const size_t old = carry.size();
                carry.resize(old + (1u << 20));
                const size_t got = src.read(carry.data() + old, 1u << 20);
                carry.resize(old + got);
                eof = got == 0;
                continue;
            }
            if (!nl && pos == carry.size()) throw PfileError(in_path + ": no #CHROM line");
            const size_t stop = nl ? (size_t)(nl - carry.data()) : carry.size();
            std::string line(reinterpret_cast<const char *>(carry.data()) + pos, stop - pos);
            if (!line.empty() && line.back() == '\r') line.pop_back();
            pos = nl ? stop + 1 : stop;
            header_lines++;
            if (line.compare(0, 2, "##") == 0) {
                if (line.compare(0, 13, "##fileformat=") != 0 && line != "##source=pgen-rs") pvar_text += line + '\n';   // (filter writes those two itself)
                continue;
            }
            if (line.compare(0, 6, "#CHROM") != 0) throw PfileError(import_line_error(in_path, header_lines, "expected a ## line or the #CHROM line"));
            columns = line;
            break;
        }
        carry.erase(carry.begin(), carry.begin() + (ptrdiff_t)pos);
    }
    std::vector<std::string> names;
    for (size_t b = 0;;) {
        const size_t e = columns.find('\t', b);
        names.push_back(columns.substr(b, e == std::string::npos ? e : e - b));
        if (e == std::string::npos) break;
        b = e + 1;
    }
    const size_t format_col = (size_t)(std::find(names.begin(), names.end(), std::string("FORMAT")) - names.begin());
    if (format_col == names.size()) throw PfileError(in_path + ": no FORMAT column in the #CHROM line");
    const size_t N = names.size() - format_col - 1;
    if (N == 0) throw PfileError(in_path + ": no sample columns behind FORMAT");
    if (N > 0x7FFFFFFFull) throw PfileError(in_path + ": more than 2^31 - 1 samples");
    const size_t alt_col = (size_t)(std::find(names.begin(), names.begin() + (ptrdiff_t)format_col, std::string("ALT")) - names.begin());   // format_col: none
    for (size_t c = 0; c < format_col; c++) pvar_text += (c ? "\t" : "") + names[c];
    pvar_text += '\n';
    std::string sam_text = "#IID\tSEX\n";
    for (size_t k = 0; k < N; k++) sam_text += names[format_col + 1 + k] + "\tNA\n";
    st.samples_kept = N;
    st.seconds_filter = now_s() - t0;

    const double t_body = now_s();
    int n_dev = 0;
    check(pgenhip_device_count(&n_dev), "pgenhip_device_count");
    if (n_dev <= 0) throw PfileError("no HIP device: the GT parse path has no CPU fallback");   // before the output files exist
    const uint32_t R = pgenhip_variant_record_size((uint32_t)N);
    const size_t cap = (size_t)std::max<uint64_t>(opt.block_text_bytes, 1u << 16);
    // a line that passes the checks holds format_col columns, "GT" and N fields of two bytes at least
    const size_t max_lines = cap / (2 * N + 2 * format_col + 3) + 1;
    DeviceCtx ctx(0, (uint32_t)N);
    uint8_t *d_text = ctx.device<uint8_t>(cap, "device text");
    uint64_t *d_off = ctx.device<uint64_t>(16 * max_lines, "device line offsets");
    uint8_t *d_out = ctx.device<uint8_t>(max_lines * R, "device records");
    uint32_t *d_flags = ctx.device<uint32_t>(4 * max_lines, "device line flags");
    uint8_t *h_text[2];
    uint64_t *h_off[2];   // field_off of the kept lines, then (from max_lines) their line_end
    for (int s = 0; s < 2; s++) {
        h_text[s] = ctx.pinned<uint8_t>(cap, "pinned text");
        h_off[s] = ctx.pinned<uint64_t>(16 * max_lines, "pinned line offsets");
    }
    uint8_t *h_out = ctx.pinned<uint8_t>(max_lines * R, "pinned records");
    uint32_t *h_flags = ctx.pinned<uint32_t>(4 * max_lines, "pinned line flags");
    st.seconds_setup = now_s() - t_body;

    // the reader: fills, indexes and checks block k + 1 while block k is on the device
    ImportBlock blocks[2];
    int state[2] = {0, 0};   // 0 free, 1 filled
    bool stop = false;
    std::mutex mu;
    std::condition_variable cv;
    std::thread reader([&] {
        std::vector<uint64_t> ls(max_lines), fmt(max_lines), fo(max_lines), le(max_lines);
        uint64_t lines_before = header_lines;
        bool eof = false;
        for (size_t k = 0;; k++) {
            const int s = (int)(k % 2);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return state[s] == 0 || stop; });
                if (stop) return;
            }
            ImportBlock &b = blocks[s];
            b = ImportBlock();
            try {
                if (carry.size() > cap) throw PfileError(in_path + ": a line is longer than a block (--block-mib)");
                size_t len = carry.size();
                std::memcpy(h_text[s], carry.data(), len);
                carry.clear();
                if (!eof) {
                    len += src.read(h_text[s] + len, cap - len);
                    eof = len < cap;
                }
                uint64_t n = 0, consumed = 0;
                check(pgenhip_vcf_index_lines(h_text[s], len, (uint32_t)format_col, max_lines, eof ? PGENHIP_VCF_LAST_BLOCK : 0u, ls.data(), fmt.data(), fo.data(),
                                              le.data(), &n, &consumed), "pgenhip_vcf_index_lines");
                if (n == 0 && len == cap) throw PfileError(in_path + ": a line is longer than a block (--block-mib)");
                carry.assign(h_text[s] + consumed, h_text[s] + len);
                b.text_len = (size_t)consumed;
                const char *text = reinterpret_cast<const char *>(h_text[s]);
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t line = lines_before + i + 1;
                    if (fo[i] == UINT64_MAX) throw PfileError(import_line_error(in_path, line, "fewer columns than the #CHROM line has in front of the samples"));
                    const uint64_t flen = fo[i] - fmt[i];
                    if (flen < 2 || text[fmt[i]] != 'G' || text[fmt[i] + 1] != 'T' || (flen > 2 && text[fmt[i] + 2] != ':'))
                        throw PfileError(import_line_error(in_path, line, "FORMAT is '" + std::string(text + fmt[i], flen) + "': GT must come first"));
                    if (iopt.skip_multiallelic && alt_col != format_col) {   // the ALT column holds a ',': dropped here, in front of the kernel
                        uint64_t a = ls[i];
                        for (size_t c = 0; c < alt_col; c++) a = (uint64_t)(static_cast<const char *>(std::memchr(text + a, '\t', fmt[i] - a)) - text) + 1;
                        const void *a_end = std::memchr(text + a, '\t', fmt[i] - a);
                        if (std::memchr(text + a, ',', (size_t)(static_cast<const char *>(a_end) - (text + a)))) {
                            b.skipped++;
                            continue;
                        }
                    }
                    h_off[s][b.n] = fo[i];
                    h_off[s][max_lines + b.n] = le[i];
                    b.n++;
                    b.line_no.push_back(line);
                    if (fmt[i] > ls[i]) b.pvar.append(text + ls[i], fmt[i] - 1 - ls[i]);
                    b.pvar += '\n';
                }
                lines_before += n;
                b.last = eof && carry.empty();
            } catch (const std::exception &e) {
                b.error = e.what();
                b.last = true;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                state[s] = 1;
            }
            cv.notify_all();
            if (b.last) return;
        }
    });
    const std::string out_main = out_prefix + ".pgen", out_var = out_prefix + ".pvar", out_sam = out_prefix + ".psam";
    bool created = false, done = false;
    Finally cleanup{[&] {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        reader.join();
        if (created && !done)   // an error: no output file stays behind
            for (const std::string *p : {&out_main, &out_var, &out_sam}) ::unlink(p->c_str());
    }};

    Fd out(out_main, O_WRONLY | O_CREAT | O_TRUNC);
    created = true;
    uint64_t V = 0;
    for (size_t k = 0;; k++) {
        const int s = (int)(k % 2);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[s] == 1; });
        }
        const ImportBlock &b = blocks[s];
        if (!b.error.empty()) throw PfileError(b.error);
        if (b.n != 0) {
            if (V + b.n > 0xFFFFFFFFull) throw PfileError(in_path + ": more than 2^32 - 1 variants");
            check(pgenhip_memcpy_h2d(ctx.get(), d_text, h_text[s], b.text_len), "H2D text");
            check(pgenhip_memcpy_h2d(ctx.get(), d_off, h_off[s], b.n * sizeof(uint64_t)), "H2D field offsets");
            check(pgenhip_memcpy_h2d(ctx.get(), d_off + max_lines, h_off[s] + max_lines, b.n * sizeof(uint64_t)), "H2D line ends");
            check(pgenhip_timer_start(ctx.get()), "timer");
            check(pgenhip_parse_gt(ctx.get(), d_text, b.text_len, d_off, d_off + max_lines, (uint32_t)b.n, d_out, R, d_flags, PGENHIP_PARSE_AUTO), "pgenhip_parse_gt");
            check(pgenhip_timer_mark(ctx.get()), "timer");
            check(pgenhip_memcpy_d2h(ctx.get(), h_out, d_out, b.n * R), "D2H records");
            check(pgenhip_memcpy_d2h(ctx.get(), h_flags, d_flags, b.n * sizeof(uint32_t)), "D2H line flags");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            float ms = 0;
            if (pgenhip_timer_read(ctx.get(), &ms) == PGENHIP_OK) st.seconds_kernel += ms * 1e-3;
            for (size_t j = 0; j < b.n; j++) {
                const uint32_t f = h_flags[j];
                if (f & PGENHIP_PARSE_FIELD_COUNT)
                    throw PfileError(import_line_error(in_path, b.line_no[j], "the number of sample fields is not the " + std::to_string(N) + " of the #CHROM line"));
                if (f & PGENHIP_PARSE_BAD_CALL) throw PfileError(import_line_error(in_path, b.line_no[j], "a GT that is neither A nor A/B nor A|B"));
                if (f & PGENHIP_PARSE_ALLELE_RANGE)
                    throw PfileError(import_line_error(in_path, b.line_no[j], "an allele other than 0, 1 and '.' (this .pgen holds biallelic calls; --skip-multiallelic drops the lines whose ALT holds a ',')"));
                st.import_half_call += (f & PGENHIP_PARSE_HALF_CALL) != 0;
                st.import_haploid += (f & PGENHIP_PARSE_HAPLOID) != 0;
                st.import_phased += (f & PGENHIP_PARSE_PHASED) != 0;
            }
            pwrite_exact(out.get(), h_out, b.n * R, 12 + V * R, out_main);
            V += b.n;
            pvar_text += b.pvar;
        }
        st.import_skipped += b.skipped;
        const bool last = b.last;
        {
            std::lock_guard<std::mutex> lk(mu);
            state[s] = 0;
        }
        cv.notify_all();
        if (last) break;
    }
    std::string header("\x6C\x1B\x02", 3);
    for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)V >> (8 * b));
    for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)N >> (8 * b));
    header += '\x40';
    pwrite_exact(out.get(), header.data(), header.size(), 0, out_main);
    out.close();
    write_text(pvar_text, out_var);
    write_text(sam_text, out_sam);
    done = true;
    st.variants = V;
    st.header_bytes = header.size();
    st.body_bytes = V * R;
    st.file_bytes = st.header_bytes + st.body_bytes;
    st.seconds_body = now_s() - t_body;
    if (st.import_half_call) std::fprintf(stderr, "warning: %llu lines hold a half call (one allele '.'): stored as missing\n", (unsigned long long)st.import_half_call);
    if (st.import_haploid) std::fprintf(stderr, "warning: %llu lines hold a haploid call: stored as 0/0, 1/1 or missing\n", (unsigned long long)st.import_haploid);
    if (st.import_phased) std::fprintf(stderr, "warning: %llu lines hold a phased call: the phase is dropped\n", (unsigned long long)st.import_phased);
    return st;
}

}  // namespace pgenhost
