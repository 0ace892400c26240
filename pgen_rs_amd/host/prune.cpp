// prune.cpp — `pgen-hip prune`: LD pruning of the kept variants on one device (pfile.h, Pfile::output_prune).  What needs no device
// is prune_plan.cpp's; the block loop is count_blocks'; `--export` runs export's own two halves (prune.h) on the variants kept.
#include <fcntl.h>
#include <unistd.h>

#include <cstring>

#include "block_loop.h"
#include "prune.h"
#include "prune_plan.h"

namespace pgenhost {

namespace {

// Everything of one run that lives on the device for the whole selection, and what comes back
struct PruneRun {
    size_t V;
    uint32_t W;
    uint64_t stride;     // u32 words per mask row
    float min_r2;
    uint64_t max_span;
    const std::vector<uint64_t> &keys;
    std::vector<uint32_t> counts;   // 4 per row
    std::vector<uint8_t> state;     // 1 kept, 2 removed
    uint64_t edges = 0, calls = 0;
    uint64_t *d_key = nullptr;
    uint32_t *d_fwd = nullptr, *d_bwd = nullptr, *d_prio = nullptr;
    uint8_t *d_state = nullptr;
    uint64_t *d_left = nullptr;
};

// prune's counter: per block the rows' counts come back (16 bytes each) and the block's edges are ORed into the resident masks; after
// the last block the priorities go up, the resolve loop runs and the state bytes come back
struct PruneCounter : Counter {
    PruneRun &run;
    uint32_t *d_counts, *h_counts;
    void launch(const BlockRows &b, size_t b0, uint32_t nv, uint32_t nh, bool) const
    {
        genotype_counts(b, nv, d_counts);
        launch_rows(b, NAMED(pgenhip_pair_mask), NAMED(pgenhip_pair_mask_at), nv + nh, nv, run.W, run.min_r2, (const uint64_t *)(run.d_key + b0), run.max_span,
                    run.d_fwd + b0 * run.stride, run.d_bwd + b0 * run.stride, run.stride, 0u);
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, nv * 16), "D2H variant counts"); }
    void collect(size_t b0, size_t nv) const { std::memcpy(run.counts.data() + 4 * b0, h_counts, nv * 16); }
    void finish(pgenhip_ctx *ctx) const
    {
        const size_t V = run.V;
        std::vector<uint32_t> prio(V);
        for (size_t j = 0; j < V; j++) prio[j] = prune_plan::priority(run.counts[4 * j], run.counts[4 * j + 1], run.counts[4 * j + 2]);
        check(pgenhip_memcpy_h2d(ctx, run.d_prio, prio.data(), 4 * V), "H2D priorities");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        uint64_t left = V;
        while (left != 0) {
            check(pgenhip_prune_resolve(ctx, run.d_fwd, run.d_bwd, run.stride, run.W, V, run.d_prio, run.d_state, run.d_left, PGENHIP_PRUNE_AUTO), "pgenhip_prune_resolve");
            check(pgenhip_memcpy_d2h(ctx, &left, run.d_left, 8), "D2H undecided count");
            check(pgenhip_wait(ctx), "pgenhip_wait");
            if (++run.calls > V) throw PfileError("prune: the resolve loop did not end within one call per variant");
        }
        run.state.resize(V);
        check(pgenhip_memcpy_d2h(ctx, run.state.data(), run.d_state, V), "D2H states");
        check(pgenhip_wait(ctx), "pgenhip_wait");
        // the JSON line's edge count: the forward mask's bits (W / 8 bytes per row, where r^2 would have been 4 W), through a bounded
        // host buffer
        const size_t words = (size_t)(V * run.stride), chunk = std::min<size_t>(words, (size_t)16 << 20);
        std::vector<uint32_t> part(chunk);
        for (size_t w0 = 0; w0 < words; w0 += chunk) {
            const size_t n = std::min(chunk, words - w0);
            check(pgenhip_memcpy_d2h(ctx, part.data(), run.d_fwd + w0, n * 4), "D2H forward mask");
            check(pgenhip_wait(ctx), "pgenhip_wait");
            for (size_t k = 0; k < n; k++) run.edges += (uint64_t)__builtin_popcount(part[k]);
        }
    }
};

// zero bytes on the device through one small pinned buffer
void zero_device(DeviceCtx &ctx, void *d, size_t bytes)
{
    const size_t chunk = std::min<size_t>(std::max<size_t>(bytes, 1), (size_t)8 << 20);
    uint8_t *z = ctx.pinned<uint8_t>(chunk, "pinned zeros");
    std::memset(z, 0, chunk);
    for (size_t off = 0; off < bytes; off += chunk)
        check(pgenhip_memcpy_h2d(ctx.get(), (uint8_t *)d + off, z, std::min(chunk, bytes - off)), "H2D zeros");
    check(pgenhip_wait(ctx.get()), "pgenhip_wait");
}

}  // namespace

OutputStats Pfile::output_prune(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                const std::string &out_prefix, const PruneOptions &popt, const OutputOptions &opt_in) const
{
    OutputStats st;
    OutputOptions opt = opt_in;   // the masks live on one device
    opt.n_gpus = 1;
    opt.n_shards = 1;
    const ExportOptions eopt;
    if (popt.with_export) refuse_export_over_input(*this, out_prefix + ".pgen");
    size_t id_col = 0;
    std::vector<uint64_t> keys;
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](const Selection &sel) {
        id_col = column(sel.var_header, "ID", pvar_path());
        const size_t chrom_col = column(sel.var_header, "CHROM", pvar_path()), pos_col = column(sel.var_header, "POS", pvar_path());
        std::vector<std::string> chrom;
        std::vector<uint64_t> pos;
        chrom.reserve(sel.var_idx_rcds.size());
        for (const auto &vr : sel.var_idx_rcds) {
            chrom.push_back(vr.second.at(chrom_col));
            if (popt.has_window_kb) {
                uint64_t p = 0;
                if (!prune_plan::parse_pos(vr.second.at(pos_col), p))
                    throw PfileError("POS '" + vr.second.at(pos_col) + "' of variant row " + std::to_string(vr.first) + " (line " + std::to_string(vr.first + 1) +
                                     " behind the column line) of " + pvar_path() + " is not a number below 2^32");
                pos.push_back(p);
            }
        }
        keys = prune_plan::keys(chrom, popt.has_window_kb ? &pos : nullptr);
    });
    const Selection &sel = o.sel;
    const size_t V = o.V, K = o.K;

    const double t_body = now_s();
    std::vector<uint8_t> state(V, PGENHIP_PRUNE_KEPT);
    if (V >= 2 && K != 0) {   // else nothing can be correlated: every variant is kept, no device touched
        const uint64_t max_span = popt.has_window_kb ? popt.window_kb * 1000ull : 0ull;
        uint64_t w = popt.window;
        if (popt.has_window_kb) w = prune_plan::window_for_span(keys, max_span, popt.window);
        const uint32_t W = (uint32_t)std::min<uint64_t>(w, V - 1);   // no pair reaches further
        PruneRun run{V, W, (W + 31u) / 32u, (float)popt.min_r2, max_span, keys, std::vector<uint32_t>(4 * V, 0u), {}};
        count_blocks(*this, sel.var_idx_rcds, o.kept, opt, "no HIP device: the prune path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            // the masks stay resident beside the blocks' buffers: they may take half of what the device has free now
            uint64_t free_bytes = 0;
            check(pgenhip_device_memory(ctx.get(), &free_bytes, nullptr), "pgenhip_device_memory");
            if (!prune_plan::masks_fit(V, W, free_bytes))
                throw PfileError("the pair masks of " + std::to_string(V) + " variants and a window of " + std::to_string(W) + " variants take " +
                                 std::to_string(prune_plan::mask_bytes(V, W)) + " bytes, more than half of the " + std::to_string(free_bytes) +
                                 " bytes the device has free: cap the window with --window <W>");
            const size_t mask = (size_t)(V * run.stride * 4);
            run.d_key = ctx.device<uint64_t>(8 * V, "device keys");
            run.d_fwd = ctx.device<uint32_t>(mask, "device forward mask");
            run.d_bwd = ctx.device<uint32_t>(mask, "device backward mask");
            run.d_prio = ctx.device<uint32_t>(4 * V, "device priorities");
            run.d_state = ctx.device<uint8_t>(V, "device states");
            run.d_left = ctx.device<uint64_t>(8, "device undecided count");
            zero_device(ctx, run.d_fwd, mask);
            zero_device(ctx, run.d_bwd, mask);
            zero_device(ctx, run.d_state, V);
            check(pgenhip_memcpy_h2d(ctx.get(), run.d_key, keys.data(), 8 * V), "H2D keys");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            return PruneCounter{{}, run, ctx.device<uint32_t>(16 * (size_t)bv, "device variant counts"), ctx.pinned<uint32_t>(16 * (size_t)bv, "pinned variant counts")};
        }, popt.block_rows, W);
        state = run.state;
        st.prune_edges = run.edges;
        st.prune_window = W;
        st.prune_calls = run.calls;
        st.prune_mask_bytes = prune_plan::mask_bytes(V, W);
    }

    std::string in_text, out_text;
    Selection kept_sel;
    for (size_t j = 0; j < V; j++) {
        const bool keep = state[j] == PGENHIP_PRUNE_KEPT;
        std::string &t = keep ? in_text : out_text;
        t += sel.var_idx_rcds[j].second.at(id_col);
        t += '\n';
        if (keep) st.prune_kept++;
        else st.prune_removed++;
        if (keep && popt.with_export) kept_sel.var_idx_rcds.push_back(sel.var_idx_rcds[j]);
    }
    if (popt.with_export) {
        kept_sel.sam_idx_rcs = sel.sam_idx_rcs;
        kept_sel.sam_header = sel.sam_header;
        kept_sel.var_header = sel.var_header;
        std::string var_text, sam_text;
        export_texts(*this, kept_sel, eopt, var_text, sam_text);
        OutputStats est;
        export_records(*this, kept_sel.var_idx_rcds, o.kept, out_prefix, eopt, opt, est, var_text, sam_text);
        st.seconds_kernel += est.seconds_kernel;
    }
    write_text(in_text, out_prefix + ".prune.in");
    write_text(out_text, out_prefix + ".prune.out");
    st.body_bytes = in_text.size() + out_text.size();
    st.file_bytes = st.body_bytes;
    st.seconds_body = now_s() - t_body;
    return st;
}

}  // namespace pgenhost
