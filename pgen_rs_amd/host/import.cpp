// import.cpp — import_vcf of pfile.h: VCF text (plain, gzip or BGZF) to a .pgen / .pvar / .psam fileset.  A reader thread fills, indexes
// and checks block k + 1 while the device parses the GT fields of block k.
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>

#include "block_loop.h"

namespace pgenhost {

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
