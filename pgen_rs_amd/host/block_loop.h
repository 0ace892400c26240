// block_loop.h — what the commands of commands.cpp, assoc.cpp and prune.cpp (and import.cpp) are built from below their own
// counters: the block loop over a shard's records with the counter it drives, the ABI pairs it launches, the column groups of a wide
// launch, the shards' sums in order, the tile triangle of the sample-pair commands, a command's opening, the cells its lines are
// made of, and the text a command ends with.
#pragma once
#include <fcntl.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <optional>

#include "host_internal.h"

namespace pgenhost {

inline void append_u64(std::string &s, uint64_t v)
{
    char buf[24];
    int n = 0;
    do {
        buf[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) s += buf[--n];
}

// one floating-point cell, %.<precision>g; nan_word: a NaN is written as "nan" whatever its sign (else as printf writes it)
inline void append_double(std::string &s, double v, int precision, bool nan_word = false)
{
    if (nan_word && std::isnan(v)) {
        s += "nan";
        return;
    }
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.*g", precision, v);
    s += buf;
}

// the sixteen cells of a 4 x 4 genotype table behind ld's and kinship's own columns: their header cells, and a line's
inline void append_table_header(std::string &s)
{
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) s += std::string("\tT") + (char)('0' + a) + (char)('0' + b);
}
inline void append_table_cells(std::string &s, const uint32_t *t)
{
    for (int c = 0; c < 16; c++) {
        s += '\t';
        append_u64(s, t[c]);
    }
}

// the .pvar columns of these names, in this order
template <size_t N>
void pvar_columns(const Pfile &pf, const StringRecord &header, const char *const (&names)[N], size_t (&col)[N])
{
    for (size_t c = 0; c < N; c++) col[c] = column(header, names[c], pf.pvar_path());
}

// the five leading columns of a per-variant line, copied verbatim from the .pvar columns of these names, a tab behind each
constexpr const char *kVariantColumns[5] = {"CHROM", "POS", "ID", "REF", "ALT"};
inline void append_variant_columns(std::string &s, const StringRecord &r, const size_t (&col)[5])
{
    for (int c = 0; c < 5; c++) {
        s += r.at(col[c]);
        s += '\t';
    }
}

inline void write_text(const std::string &text, const std::string &filename)
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
inline void finish_text(OutputStats &st, const std::string &text, const std::string &filename, double t_body)
{
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
}

// The opening of a command: the selection, what the command looks up in or builds from it (columns(sel), which may also replace
// the selection's rows by the ones the command goes on with), the .psam's IID column when the command prints it, all inside
// st.seconds_filter, which starts at t0 (a command that reads files of its own first takes t0 before them); then the checked kept
// samples and the two sizes into st
struct Opening {
    Pfile::Selection sel;
    size_t iid = 0;
    KeptSamples kept;
    size_t V = 0, K = 0;   // kept variants, kept samples
};
template <class Columns>
Opening open_selection(const Pfile &pf, const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                       const OutputOptions &opt, OutputStats &st, bool with_iid, const Columns &columns, double t0 = now_s())
{
    Opening o;
    o.sel = pf.select(sam_query, var_query, opt.filter_threads);
    columns(o.sel);
    if (with_iid) o.iid = iid_column(pf, o.sel.sam_header);
    st.seconds_filter = now_s() - t0;
    o.kept = check_selection(pf, o.sel);
    st.variants = o.V = o.sel.var_idx_rcds.size();
    st.samples_kept = o.K = o.kept.rows.size();
    return o;
}
inline Opening open_selection(const Pfile &pf, const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const OutputOptions &opt, OutputStats &st, bool with_iid)
{
    return open_selection(pf, sam_query, var_query, opt, st, with_iid, [](const Pfile::Selection &) {});
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

inline void genotype_counts(const BlockRows &b, uint32_t nv, uint32_t *d_counts)
{
    launch_rows(b, NAMED(pgenhip_genotype_counts), NAMED(pgenhip_genotype_counts_at), nv, d_counts, PGENHIP_COUNT_AUTO);
}

// the same counts on the host now: the launch, the copy and a wait, for a counter whose launches need the block's counts
inline void genotype_counts_now(const BlockRows &b, uint32_t nv, uint32_t *d_counts, uint32_t *h_counts)
{
    genotype_counts(b, nv, d_counts);
    check(pgenhip_memcpy_d2h(b.ctx, h_counts, d_counts, (size_t)nv * 16), "D2H counts");
    check(pgenhip_wait(b.ctx), "pgenhip_wait");
}

// fn(c0, cg) over C columns in groups of at most max_columns, the most one launch of a wide entry takes: group c0 .. c0 + cg
template <class Fn>
void column_groups(size_t C, size_t max_columns, const Fn &fn)
{
    for (size_t c0 = 0; c0 < C; c0 += max_columns) fn(c0, std::min(max_columns, C - c0));
}

inline void sample_counts(const BlockRows &b, uint32_t nv, uint32_t *d_counts, bool accumulate)
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

// What the shards of one count_blocks run sum up when FP64 addition must not depend on which shard ends first: every shard files
// its sums under its first variant (the b0 of the launch with first == true; count_blocks launches at least one block per shard:
// Shards::run skips a shard without variants), and in_order() hands them out by that variant, which is the shards' order
template <class Sums>
class ShardSums {
  public:
    void file(size_t first_b0, Sums sums)
    {
        std::lock_guard<std::mutex> lk(mu_);
        by_first_.emplace(first_b0, std::move(sums));
    }
    const std::map<size_t, Sums> &in_order() const { return by_first_; }

  private:
    std::mutex mu_;
    std::map<size_t, Sums> by_first_;
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

}  // namespace pgenhost
