// merge.cpp — merge_pfiles of merge.h: two to eight filesets' samples side by side in one fixed-width .pgen / .pvar / .psam.  The
// matching of variants and the check of the samples are merge_match.cpp's (pure); here the files are read, each block of output rows
// has its inputs' records staged and joined on the device (pgenhip_join_records), and the three files are written.
#include "merge.h"

#include <filesystem>

#include "block_loop.h"
#include "merge_match.h"

namespace pgenhost {

namespace {

template <class F>
struct Finally {
    F f;
    ~Finally() { f(); }
};
template <class F>
Finally(F) -> Finally<F>;

// a .pvar / .psam: `head` = the file's bytes up to and including its column-header line (the last leading '#' line), the rows behind it
struct MetaFile {
    std::string head;
    merge::Table table;
};

MetaFile read_meta(const std::string &path)
{
    const std::string text = read_file(path);
    MetaFile m;
    m.table.name = path;
    size_t pos = 0, head_end = 0;
    uint64_t line_no = 0;
    bool in_head = true;
    while (pos < text.size()) {
        const size_t nl = text.find('\n', pos);
        const size_t stop = nl == std::string::npos ? text.size() : nl, next = nl == std::string::npos ? text.size() : nl + 1;
        std::string line = text.substr(pos, stop - pos);
        line_no++;
        if (in_head && !line.empty() && line[0] == '#') {
            m.table.column_line = line;
            head_end = next;
        } else {
            in_head = false;
            if (!line.empty() && line != "\r") {
                m.table.rows.push_back(std::move(line));
                m.table.line_no.push_back(line_no);
            }
        }
        pos = next;
    }
    if (head_end == 0) throw PfileError(path + ": no column-header line (a leading line that starts with '#')");
    m.head = text.substr(0, head_end);
    if (m.head.back() != '\n') m.head += '\n';
    return m;
}

std::string json_array(const std::vector<uint64_t> &v)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) {
        if (i) s += ", ";
        append_u64(s, v[i]);
    }
    return s + "]";
}

}  // namespace

std::string MergeStats::json_counts() const
{
    std::string s = "\"inputs\": ";
    append_u64(s, inputs);
    s += ", \"samples\": ";
    append_u64(s, samples);
    s += ", \"variants\": ";
    append_u64(s, variants);
    s += ", \"flipped\": " + json_array(flipped) + ", \"absent\": " + json_array(absent) + ", \"dropped\": " + json_array(dropped) + ", \"id_conflicts\": ";
    append_u64(s, id_conflicts);
    return s;
}

MergeStats merge_pfiles(const std::vector<std::string> &prefixes, const std::string &out_prefix, const MergeOptions &mopt, const OutputOptions &opt)
{
    MergeStats st;
    const double t0 = now_s();
    const size_t P = prefixes.size();
    if (P < 2 || P > PGENHIP_JOIN_MAX_PARTS) throw PfileError("merge takes two to eight inputs");
    const std::string out_main = out_prefix + ".pgen", out_var = out_prefix + ".pvar", out_sam = out_prefix + ".psam";

    std::vector<Pfile> pf;
    std::vector<MetaFile> pvar, psam;
    for (const std::string &prefix : prefixes) {
        pf.push_back(Pfile::from_prefix(prefix));
        const Pfile &f = pf.back();
        {   // the same file by another spelling or through a link is still an input
            std::error_code ec1, ec2;
            const auto in = std::filesystem::weakly_canonical(f.pgen_path(), ec1), out = std::filesystem::weakly_canonical(out_main, ec2);
            if (out_main == f.pgen_path() || (!ec1 && !ec2 && in == out)) throw PfileError("merge would overwrite an input: " + out_main + " is " + f.pgen_path());
        }
        pvar.push_back(read_meta(f.pvar_path()));
        psam.push_back(read_meta(f.psam_path()));
        if (pvar.back().table.rows.size() != f.num_variants)
            throw PfileError(f.pvar_path() + " holds " + std::to_string(pvar.back().table.rows.size()) + " rows but " + f.pgen_path() + " " + std::to_string(f.num_variants) + " variants");
        if (psam.back().table.rows.size() != f.num_samples)
            throw PfileError(f.psam_path() + " holds " + std::to_string(psam.back().table.rows.size()) + " rows but " + f.pgen_path() + " " + std::to_string(f.num_samples) + " samples");
    }
    std::vector<merge::Table> vt, sm;
    for (size_t p = 0; p < P; p++) vt.push_back(std::move(pvar[p].table)), sm.push_back(std::move(psam[p].table));
    merge::Match m;
    try {
        merge::check_samples(sm);
        m = merge::match_variants(vt, mopt.with_union);
    } catch (const merge::MatchError &e) {
        throw PfileError(e.what());
    }
    const size_t V = m.from_input.size();
    uint64_t N = 0;
    for (const Pfile &f : pf) N += f.num_samples;
    if (N > 0x7FFFFFFFull) throw PfileError("the inputs hold more than 2^31 - 1 samples together");
    if (V > 0xFFFFFFFFull) throw PfileError("the output would hold more than 2^32 - 1 variants");
    // every record used must be a plain 2-bit record: check_selection's check, on the rows each input gives
    for (size_t p = 0; p < P; p++) {
        Pfile::Selection sel;
        for (size_t j = 0; j < V; j++)
            if (m.src[p][j] != merge::kAbsent) sel.var_idx_rcds.emplace_back((size_t)m.src[p][j], StringRecord());
        check_selection(pf[p], sel);
    }
    st.inputs = P, st.samples = N, st.variants = V;
    st.flipped = m.flipped, st.absent = m.absent, st.dropped = m.dropped, st.id_conflicts = m.id_conflicts;
    st.seconds_filter = now_s() - t0;
    if (mopt.dry_run) return st;

    const double t_body = now_s();
    int n_dev = 0;
    check(pgenhip_device_count(&n_dev), "pgenhip_device_count");
    if (n_dev <= 0) throw PfileError("no HIP device: the join path has no CPU fallback");   // before the output files exist
    const uint32_t R = pgenhip_variant_record_size((uint32_t)N);
    std::vector<uint32_t> Rp(P);
    uint64_t row_bytes = R;
    for (size_t p = 0; p < P; p++) row_bytes += Rp[p] = pf[p].variant_record_size();
    const size_t B = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(std::max<size_t>(V, 1), opt.block_text_bytes / std::max<uint64_t>(row_bytes, 1)));

    DeviceCtx ctx(0, (uint32_t)N);
    std::vector<uint8_t *> d_rec(P), h_rec(P), d_flip(P), h_flip(P);
    std::vector<uint64_t *> d_off(P), h_off(P);
    std::vector<std::unique_ptr<Fd>> in;
    for (size_t p = 0; p < P; p++) {
        in.push_back(std::make_unique<Fd>(pf[p].pgen_path(), O_RDONLY));
        d_rec[p] = ctx.device<uint8_t>(B * (size_t)Rp[p] + 16, "device records");
        d_off[p] = ctx.device<uint64_t>(B * sizeof(uint64_t), "device record offsets");
        d_flip[p] = ctx.device<uint8_t>(B, "device flip bytes");
        h_rec[p] = ctx.pinned<uint8_t>(B * (size_t)Rp[p] + 16, "pinned records");
        h_off[p] = ctx.pinned<uint64_t>(B * sizeof(uint64_t), "pinned record offsets");
        h_flip[p] = ctx.pinned<uint8_t>(B, "pinned flip bytes");
    }
    uint8_t *d_out = ctx.device<uint8_t>(B * (size_t)R + 16, "device output records");
    uint8_t *h_out = ctx.pinned<uint8_t>(B * (size_t)R + 16, "pinned output records");
    st.seconds_setup = now_s() - t_body;

    bool created = false, done = false;
    Finally cleanup{[&] {
        if (created && !done)   // an error: no output file stays behind
            for (const std::string *p : {&out_main, &out_var, &out_sam}) ::unlink(p->c_str());
    }};
    Fd out(out_main, O_WRONLY | O_CREAT | O_TRUNC);
    created = true;
    for (size_t j0 = 0; j0 < V; j0 += B) {
        const size_t n = std::min(B, V - j0);
        pgenhip_join_part parts[PGENHIP_JOIN_MAX_PARTS] = {};
        for (size_t p = 0; p < P; p++) {
            // the part's present records in output-row order, one pread per run of records that are neighbours in the file
            size_t k = 0;
            for (size_t i = 0; i < n;) {
                const int64_t r = m.src[p][j0 + i];
                h_flip[p][i] = m.flip[p][j0 + i];
                if (r == merge::kAbsent) {
                    h_off[p][i++] = PGENHIP_JOIN_ABSENT;
                    continue;
                }
                const uint64_t off = pf[p].record_offset((uint64_t)r);
                size_t run = 1;
                while (i + run < n && m.src[p][j0 + i + run] == r + (int64_t)run && pf[p].record_offset((uint64_t)r + run) == off + run * Rp[p]) run++;
                pread_span(in[p]->get(), h_rec[p] + k * Rp[p], run * (size_t)Rp[p], off, pf[p].pgen_path(), opt.read_threads);
                for (size_t q = 0; q < run; q++) {
                    h_off[p][i + q] = (k + q) * (uint64_t)Rp[p];
                    h_flip[p][i + q] = m.flip[p][j0 + i + q];
                }
                k += run, i += run;
            }
            if (k && Rp[p]) check(pgenhip_memcpy_h2d(ctx.get(), d_rec[p], h_rec[p], k * (size_t)Rp[p]), "H2D records");
            check(pgenhip_memcpy_h2d(ctx.get(), d_off[p], h_off[p], n * sizeof(uint64_t)), "H2D record offsets");
            check(pgenhip_memcpy_h2d(ctx.get(), d_flip[p], h_flip[p], n), "H2D flip bytes");
            parts[p].d_base = d_rec[p];
            parts[p].d_record_off = d_off[p];
            parts[p].d_flip = m.flipped[p] ? d_flip[p] : nullptr;
            parts[p].sample_count = pf[p].num_samples;
        }
        check(pgenhip_timer_start(ctx.get()), "timer");
        check(pgenhip_join_records(ctx.get(), parts, (uint32_t)P, (uint32_t)n, d_out, R, PGENHIP_JOIN_AUTO), "pgenhip_join_records");
        check(pgenhip_timer_mark(ctx.get()), "timer");
        if (R) check(pgenhip_memcpy_d2h(ctx.get(), h_out, d_out, n * (size_t)R), "D2H records");
        check(pgenhip_wait(ctx.get()), "pgenhip_wait");
        float ms = 0;
        if (pgenhip_timer_read(ctx.get(), &ms) == PGENHIP_OK) st.seconds_kernel += ms * 1e-3;
        pwrite_exact(out.get(), h_out, n * (size_t)R, 12 + (uint64_t)j0 * R, out_main);
    }
    std::string header("\x6C\x1B\x02", 3);
    for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)V >> (8 * b));
    for (int b = 0; b < 4; b++) header += (char)(uint8_t)((uint32_t)N >> (8 * b));
    header += '\x40';
    pwrite_exact(out.get(), header.data(), header.size(), 0, out_main);
    out.close();
    std::string var_text = pvar[0].head, sam_text = psam[0].head;
    for (size_t j = 0; j < V; j++) var_text += vt[m.from_input[j]].rows[(size_t)m.from_row[j]] + '\n';
    for (size_t p = 0; p < P; p++)
        for (const std::string &row : sm[p].rows) sam_text += row + '\n';
    write_text(var_text, out_var);
    write_text(sam_text, out_sam);
    done = true;
    st.file_bytes = header.size() + (uint64_t)V * R;
    st.seconds_body = now_s() - t_body;
    return st;
}

}  // namespace pgenhost
