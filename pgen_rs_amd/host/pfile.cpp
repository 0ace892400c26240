// pfile.cpp — see pfile.h.  Line references are to /root/reference/src/pfile.rs.
#include "pfile.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <filesystem>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <thread>

#include "../../include/pgen_hip.h"
#include "bgzf.h"
#include "expr.h"

namespace pgenhost {

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

[[noreturn]] void fail_status(int rc, const std::string &what)
{
    std::string msg = what + ": " + pgenhip_strerror(rc);
    const char *detail = pgenhip_last_error_detail();
    if (detail && *detail) msg += std::string(" (") + detail + ")";
    throw PfileError(msg);
}

void check(int rc, const char *what)
{
    if (rc != PGENHIP_OK) fail_status(rc, what);
}

// std::io::BufRead::read_line: up to and including '\n'; empty at EOF
std::string read_line(const std::string &data, size_t &pos)
{
    if (pos >= data.size()) return std::string();
    size_t nl = data.find('\n', pos);
    size_t end = nl == std::string::npos ? data.size() : nl + 1;
    std::string line = data.substr(pos, end - pos);
    pos = end;
    return line;
}

// str::trim() of Rust for the ASCII whitespace that can occur here
std::string trim(const std::string &s)
{
    size_t b = 0, e = s.size();
    auto ws = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; };
    while (b < e && ws(s[b])) b++;
    while (e > b && ws(s[e - 1])) e--;
    return s.substr(b, e - b);
}

std::string hex2(uint8_t b)
{
    static const char *d = "0123456789abcdef";
    return std::string(1, d[b >> 4]) + d[b & 15];
}

void pread_exact(int fd, void *dst, size_t bytes, uint64_t offset, const std::string &path)
{
    uint8_t *p = static_cast<uint8_t *>(dst);
    while (bytes) {
        ssize_t r = pread(fd, p, bytes, (off_t)offset);
        if (r < 0) {
            if (errno == EINTR) continue;
            throw PfileError("read " + path + ": " + std::strerror(errno));
        }
        if (r == 0) throw PfileError("read " + path + ": failed to fill whole buffer (record past end of file)");  // :170 read_exact
        p += r;
        bytes -= (size_t)r;
        offset += (uint64_t)r;
    }
}

void pwrite_exact(int fd, const void *src, size_t bytes, uint64_t offset, const std::string &path)
{
    const uint8_t *p = static_cast<const uint8_t *>(src);
    while (bytes) {
        ssize_t w = pwrite(fd, p, bytes, (off_t)offset);
        if (w < 0) {
            if (errno == EINTR) continue;
            throw PfileError("write " + path + ": " + std::strerror(errno));
        }
        if (w == 0) throw PfileError("write " + path + ": failed to write whole buffer");  // BufWriter::write_all -> WriteZero
        p += w;
        bytes -= (size_t)w;
        offset += (uint64_t)w;
    }
}

// fn(lo, hi) over [0, bytes) cut into n slices, each on a thread of its own (n <= 1: on this thread); the first error is rethrown
// once every slice has ended
template <class Fn>
void split_span(size_t bytes, unsigned n, const Fn &fn)
{
    if (n <= 1) return fn(0, bytes);
    std::vector<std::thread> ts;
    std::string err;
    std::mutex mu;
    const size_t slice = (bytes + n - 1) / n;
    for (unsigned t = 0; t < n; t++) {
        const size_t lo = std::min(bytes, (size_t)t * slice), hi = std::min(bytes, lo + slice);
        if (lo == hi) continue;
        ts.emplace_back([&, lo, hi] {
            try {
                fn(lo, hi);
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                if (err.empty()) err = e.what();
            }
        });
    }
    for (auto &t : ts) t.join();
    if (!err.empty()) throw PfileError(err);
}

// `bytes` of the file at `off` into dst: one pread, or a few at once for long spans (one thread copies ~2-3 GB/s out of the page cache)
void pread_span(int fd, uint8_t *dst, size_t bytes, uint64_t off, const std::string &path, int read_threads)
{
    const unsigned n = bytes >= (64u << 20) ? (unsigned)std::max(1, read_threads) : 1u;
    split_span(bytes, n, [&](size_t lo, size_t hi) { pread_exact(fd, dst + lo, hi - lo, off + lo, path); });
}

// the same for writes: parallel pwrite()s of one block measured on tmpfs only fight over the page-allocation lock (8 writers:
// sys 9.6 s vs 2.3 s, wall unchanged), so the default is one writer
void pwrite_span(int fd, const uint8_t *src, size_t bytes, uint64_t off, const std::string &path, int write_threads)
{
    const unsigned n = bytes >= (8u << 20) ? (unsigned)std::max(1, write_threads) : 1u;
    split_span(bytes, n, [&](size_t lo, size_t hi) { pwrite_exact(fd, src + lo, hi - lo, off + lo, path); });
}

// runs f when it goes out of scope
template <class F>
struct OnExit {
    F f;
    ~OnExit() { f(); }
};
template <class F>
OnExit(F) -> OnExit<F>;

struct KeptSamples {
    std::vector<uint32_t> rows;
    bool all;   // every row kept: the K = N fast path
};

// The kept sample rows (:173: a row past the .pgen's samples is the reference's index panic) and a check of every kept variant
// row: past the .pgen's records, or (variable-width files) not stored as a plain 2-bit record of R bytes, the only kind that can
// take the path of :165-190
KeptSamples check_selection(const Pfile &pf, const Pfile::Selection &sel)
{
    const uint32_t N = pf.num_samples, R = pf.variant_record_size();
    KeptSamples kept;
    kept.rows.reserve(sel.sam_idx_rcs.size());
    for (const auto &ir : sel.sam_idx_rcs) {
        if (ir.first >= N) throw PfileError("index out of bounds: sample row " + std::to_string(ir.first) + " but the .pgen holds " + std::to_string(N) + " samples");
        kept.rows.push_back((uint32_t)ir.first);
    }
    kept.all = kept.rows.size() == (size_t)N;
    for (const auto &vr : sel.var_idx_rcds) {
        const size_t vi = vr.first;
        if (vi >= pf.num_variants)
            throw PfileError("variant row " + std::to_string(vi) + " is past the " + std::to_string(pf.num_variants) + " records of " + pf.pgen_path());
        if (pf.variable_width() && ((*pf.vw_record_type)[vi] != 0 || (*pf.vw_record_len)[vi] != R))
            throw PfileError(pf.pgen_path() + ": variant row " + std::to_string(vi) + " is stored compressed (record type " +
                             std::to_string((*pf.vw_record_type)[vi]) + ", " + std::to_string((*pf.vw_record_len)[vi]) + " bytes); only uncompressed 2-bit records are supported");
    }
    return kept;
}

// One ctx and the device and pinned buffers allocated through it.  The destructor frees the pinned buffers, then the device
// buffers, each in the order of allocation, and destroys the ctx last.
class DeviceCtx {
  public:
    // kept: null (or every sample) decodes all samples
    DeviceCtx(int device, uint32_t n_samples, const KeptSamples *kept = nullptr)
    {
        const bool all = !kept || kept->all;
        // a filter that kept NOBODY is an empty list, not "all samples": say so with the flag (rows.data() is NULL then)
        check(pgenhip_create(&ctx_, device, n_samples, all ? nullptr : kept->rows.data(), kept ? (uint32_t)kept->rows.size() : 0u,
                             all ? 0u : PGENHIP_CREATE_KEEP_LIST), "pgenhip_create");
    }
    DeviceCtx(const DeviceCtx &) = delete;
    DeviceCtx &operator=(const DeviceCtx &) = delete;
    ~DeviceCtx()
    {
        for (void *p : pinned_) pgenhip_host_free_pinned(ctx_, p);
        for (void *p : device_) pgenhip_device_free(ctx_, p);
        pgenhip_destroy(ctx_);
    }
    pgenhip_ctx *get() const { return ctx_; }
    template <class T>
    T *device(size_t bytes, const char *what)
    {
        void *p = nullptr;
        check(pgenhip_device_malloc(ctx_, &p, bytes), what);
        device_.push_back(p);
        return static_cast<T *>(p);
    }
    template <class T>
    T *pinned(size_t bytes, const char *what)
    {
        void *p = nullptr;
        check(pgenhip_host_malloc_pinned(ctx_, &p, bytes), what);
        pinned_.push_back(p);
        return static_cast<T *>(p);
    }

  private:
    pgenhip_ctx *ctx_ = nullptr;
    std::vector<void *> device_, pinned_;
};

// The variant shards of a run: opt.n_shards contiguous ranges of the kept-variant list (0: one per device used), dealt round-robin
// over the devices.  run() calls fn(g, device, begin, end) for every non-empty shard, each on a thread of its own and shard 0 on
// the calling thread, and rethrows the first error once every shard has ended.
struct Shards {
    int n_use, G;   // devices used, shards
    Shards(const OutputOptions &opt, const char *no_device)
    {
        int n_dev = 0;
        check(pgenhip_device_count(&n_dev), "pgenhip_device_count");
        if (n_dev <= 0) throw PfileError(no_device);
        n_use = std::max(1, std::min(opt.n_gpus, n_dev));
        G = opt.n_shards > 0 ? opt.n_shards : n_use;
    }
    template <class Fn>
    void run(size_t V, const Fn &fn) const
    {
        std::string err;
        std::mutex mu;
        auto worker = [&](int g) {
            try {
                // sizes differ by <= 1: the one partitioner
                uint64_t begin = 0, end = 0;
                check(pgenhip_shard_range(V, (uint32_t)G, (uint32_t)g, &begin, &end), "pgenhip_shard_range");
                if (begin != end) fn(g, g % n_use, (size_t)begin, (size_t)end);
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                if (err.empty()) err = e.what();
            }
        };
        std::vector<std::thread> threads;
        for (int g = 1; g < G; g++) threads.emplace_back(worker, g);
        worker(0);
        for (auto &t : threads) t.join();
        if (!err.empty()) throw PfileError(err);
    }
};

}  // namespace

std::string read_file(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw PfileError("open " + path + ": " + std::strerror(errno));  // File::open(..).unwrap()
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// :38-76
Pfile Pfile::from_prefix(const std::string &pfile_prefix)
{
    Pfile pf;
    pf.pfile_prefix = pfile_prefix;
    const std::string path = pf.pgen_path();
    const Fd file(path, O_RDONLY);  // :41
    const int fd = file.get();
    uint8_t hdr[12];
    ssize_t got = pread(fd, hdr, sizeof hdr, 0);
    if (got != (ssize_t)sizeof hdr) throw PfileError("read " + path + ": failed to fill whole buffer");  // :45 read_exact
    if (hdr[0] == 0x6C && hdr[1] == 0x1B && hdr[2] == 0x10) {
        // the standard variable-width mode: the header walk of src/pgen.rs:21-258.  (Every other mode byte — 0x01 .bed, 0x03 / 0x04
        // fixed-width dosage, 0x20 / 0x21 — keeps the reference's refusal below, :53: their bytes 3.. are not this header.)
        pgenhip_vw_header vh;
        int vrc = pgenhip_vw_parse_header(hdr, &vh);
        if (vrc == PGENHIP_ERR_BAD_FLAGS)
            throw PfileError(path + ": storage mode 0x" + hex2(hdr[2]) + ": unsupported header format byte (" + pgenhip_last_error_detail() + ")");  // src/pgen.rs:58, :64
        check(vrc, "pgenhip_vw_parse_header");
        // the header's counts are 32 untrusted bits: nothing is allocated from them before the file has shown that it holds the tables
        struct stat sb;
        if (fstat(fd, &sb) != 0) throw PfileError("stat " + path + ": " + std::strerror(errno));
        const uint64_t file_size = (uint64_t)sb.st_size;
        if (vh.variant_records_offset > file_size)
            throw PfileError(path + ": failed to fill whole buffer (the header promises " + std::to_string(vh.variant_records_offset) +
                             " bytes of offset and type / length tables, the file has " + std::to_string(file_size) + ")");  // src/pgen.rs:147, :219 read_exact
        std::vector<uint8_t> index((size_t)(vh.variant_records_offset - 12ull));
        pread_exact(fd, index.data(), index.size(), 12, path);
        auto types = std::make_shared<std::vector<uint8_t>>(vh.variant_count);
        auto lens = std::make_shared<std::vector<uint32_t>>(vh.variant_count);
        auto offs = std::make_shared<std::vector<uint64_t>>(vh.variant_count);
        vrc = pgenhip_vw_walk_index(&vh, index.data(), index.size(), types->data(), lens->data(), offs->data());
        if (vrc == PGENHIP_ERR_BAD_INDEX) throw PfileError(path + ": " + pgenhip_last_error_detail());  // src/pgen.rs:160-165 panic
        check(vrc, "pgenhip_vw_walk_index");
        // records ascend and do not overlap (the walk checked that), so the last one bounds them all
        if (vh.variant_count && offs->back() + (uint64_t)lens->back() > file_size)
            throw PfileError(path + ": variant records run past the end of the file (" + std::to_string(offs->back() + (uint64_t)lens->back()) + " > " +
                             std::to_string(file_size) + ")");
        pf.storage_mode = hdr[2];
        pf.num_variants = vh.variant_count;
        pf.num_samples = vh.sample_count;
        pf.vw_record_type = types;
        pf.vw_record_len = lens;
        pf.vw_record_off = offs;
        return pf;
    }
    int rc = pgenhip_parse_header(hdr, &pf.num_variants, &pf.num_samples);
    if (rc == PGENHIP_ERR_BAD_MAGIC) throw PfileError(path + ": assertion failed: magic number is not [0x6C, 0x1B]");          // :47
    if (rc == PGENHIP_ERR_BAD_MODE) throw PfileError(path + ": assertion failed: storage_mode == 0x02 (only the fixed-width mode is supported)");  // :53
    if (rc == PGENHIP_ERR_BAD_FLAGS) throw PfileError(path + ": assertion failed: header byte 11 is not 0x40");                // :69
    check(rc, "pgenhip_parse_header");
    return pf;
}

// :196-200
uint32_t Pfile::variant_record_size() const { return pgenhip_variant_record_size(num_samples); }

uint64_t Pfile::record_offset(uint64_t var_idx) const
{
    if (variable_width()) return (*vw_record_off)[(size_t)var_idx];
    return pgenhip_record_offset(var_idx, variant_record_size());  // :165, widened before the multiply
}

// :202-220
std::pair<std::string, std::string> Pfile::read_pvar_header() const
{
    const std::string data = read_file(pvar_path());
    std::vector<std::string> header_lines;
    size_t pos = 0;
    for (;;) {
        std::string buf = read_line(data, pos);
        if (!buf.empty() && buf[0] == '#')
            header_lines.push_back(buf);
        else
            break;
    }
    if (header_lines.empty()) throw PfileError(pvar_path() + ": no '#' header line (called `Option::unwrap()` on a `None` value)");  // :217
    std::string header = header_lines.back();
    header_lines.pop_back();
    std::string joined;
    for (const auto &l : header_lines) joined += l;
    return {joined, header};
}

// :248-268
uint64_t Pfile::find_metadata_file_header_start(const std::string &data)
{
    size_t pos = 0;
    std::string prev_buf, buf;
    for (;;) {
        prev_buf = buf;
        buf = read_line(data, pos);
        if (buf.empty() || buf[0] != '#') {
            const uint64_t current_pos = pos;
            const uint64_t offset = (uint64_t)(buf.size() + prev_buf.size()) - 1ull;  // wraps like Rust would panic only in debug
            return current_pos - offset;
        }
    }
}

// :312-335
namespace {

// src/pfile.rs:312-335 for the records of one reader, indices starting at `first_idx`.
Pfile::IdxRecords filter_records(TsvReader &reader, const std::optional<std::string> &query, size_t first_idx)
{
    Pfile::IdxRecords kept;
    std::optional<Expr> expr;
    if (query) {
        expr.emplace(*query);
        expr->bind(reader.headers());
    }
    StringRecord rcd;
    size_t idx = first_idx;
    while (reader.next(rcd)) {
        const bool keep = expr ? expr->eval_boolean(rcd) : true;  // :321-329
        if (keep) kept.emplace_back(idx, rcd);                    // :330-332
        idx++;
    }
    return kept;
}

}  // namespace

// N2: the reference walks the metadata file on one thread (2.7 s of its chr22 runs,
// README.md:164-168).  Records are independent, so a big file without quotes — a quoted field may
// hold a line break, which would make a split point ambiguous — is cut at line ends into one piece
// per thread; every piece is parsed and filtered like the whole (same header row, same expression),
// and the kept records are concatenated in file order with their indices shifted by the number of
// records before the piece.  Any error re-runs the serial walk so that the message (record and line
// numbers) is the one the serial reader gives.
Pfile::IdxRecords Pfile::filter_metadata(TsvReader &reader, const std::optional<std::string> &query, int filter_threads)
{
    const std::string &data = reader.data();
    const size_t begin = reader.position(), end = reader.end_position();
    const size_t kMinBytesPerThread = 1u << 20;
    size_t n_threads = std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), 16u, (end - begin) / kMinBytesPerThread});
    if (filter_threads > 0) n_threads = (size_t)filter_threads;  // `--filter-threads` (1 = the serial walk of the reference)
    if (n_threads < 2 || begin >= end || memchr(data.data() + begin, '"', end - begin) != nullptr)
        return filter_records(reader, query, 0);

    // piece boundaries: just behind a '\n' (files that end records with a lone '\r' stay in one piece)
    std::vector<size_t> cuts{begin};
    for (size_t t = 1; t < n_threads; t++) {
        const size_t want = begin + (end - begin) / n_threads * t;
        if (want <= cuts.back()) continue;
        const void *nl = memchr(data.data() + want, '\n', end - want);
        if (!nl) break;
        const size_t cut = (size_t)(static_cast<const char *>(nl) - data.data()) + 1u;
        if (cut > cuts.back() && cut < end) cuts.push_back(cut);
    }
    cuts.push_back(end);
    const size_t n_pieces = cuts.size() - 1u;
    if (n_pieces < 2) return filter_records(reader, query, 0);

    std::vector<IdxRecords> kept(n_pieces);
    std::vector<size_t> n_records(n_pieces, 0);
    std::vector<char> failed(n_pieces, 0);
    std::vector<std::thread> workers;
    for (size_t t = 0; t < n_pieces; t++) {
        workers.emplace_back([&, t] {
            try {
                TsvReader piece(reader, cuts[t], cuts[t + 1u]);
                kept[t] = filter_records(piece, query, 0);  // indices local to the piece
                n_records[t] = piece.records_read();
            } catch (...) {
                failed[t] = 1;
            }
        });
    }
    for (auto &w : workers) w.join();
    if (std::find(failed.begin(), failed.end(), (char)1) != failed.end()) return filter_records(reader, query, 0);  // throws the serial error

    size_t total = 0;
    for (const auto &k : kept) total += k.size();
    IdxRecords all;
    all.reserve(total);
    size_t base = 0;
    for (size_t t = 0; t < n_pieces; t++) {
        for (auto &kv : kept[t]) all.emplace_back(kv.first + base, std::move(kv.second));
        base += n_records[t];
    }
    return all;
}

Pfile::Selection Pfile::select(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query, int filter_threads) const
{
    Selection sel;
    const std::string psam = read_file(psam_path());  // :111
    TsvReader psam_reader(psam, find_metadata_file_header_start(psam));
    sel.sam_header = psam_reader.headers();  // :112
    const std::string pvar = read_file(pvar_path());
    TsvReader pvar_reader(pvar, find_metadata_file_header_start(pvar));
    sel.var_header = pvar_reader.headers();
    sel.var_idx_rcds = filter_metadata(pvar_reader, var_query, filter_threads);  // :127
    sel.sam_idx_rcs = filter_metadata(psam_reader, sam_query, filter_threads);   // :128
    return sel;
}

void Pfile::query_metadata(TsvReader &reader, const std::optional<std::string> &query, const std::string &f_string, std::string &out)
{
    std::optional<Expr> filter;
    if (query) {
        filter.emplace(*query);
        filter->bind(reader.headers());
    }
    Expr fmt(f_string);
    fmt.bind(reader.headers());
    StringRecord rcd;
    while (reader.next(rcd)) {
        const bool keep = filter ? filter->eval_boolean(rcd) : true;  // :93-95
        if (keep) {
            out += fmt.eval_string(rcd);  // :97
            out += '\n';                  // println!
        }
    }
}

// :110-146 minus the file handling
std::string Pfile::vcf_header(const IdxRecords &sam_idx_rcs, const StringRecord &sam_header) const
{
    auto [pvar_header, pvar_column_names] = read_pvar_header();  // :110
    size_t iid = sam_header.size();
    for (size_t c = 0; c < sam_header.size(); c++) {  // :114-124 find_map: first match
        if (sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());  // :125-126
    std::string sam_ids;  // :130-134
    for (size_t k = 0; k < sam_idx_rcs.size(); k++) {
        if (k) sam_ids += '\t';
        sam_ids += sam_idx_rcs[k].second.at(iid);
    }
    std::string h = "##fileformat=VCFv4.2\n##source=pgen-rs\n";  // :139-140
    h += pvar_header;                                              // :141
    h += trim(pvar_column_names);                                  // :144-145
    h += "\tFORMAT\t" + sam_ids + "\n";                            // :146
    return h;
}

// :104-194
OutputStats Pfile::output_vcf(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    // The HIP runtime's first call (device discovery, loading the code object) costs 30-80 ms: let it run beside the metadata walk
    // instead of in front of the first block.  A throw-away ctx on every device this run will use; errors are left to the real
    // creates below, which report them.
    std::thread hip_warm_up([n = std::max(1, opt.n_gpus)] {
        int n_dev = 0;
        if (pgenhip_device_count(&n_dev) != PGENHIP_OK) return;
        for (int d = 0; d < std::min(n, n_dev); d++) {
            pgenhip_ctx *c = nullptr;
            if (pgenhip_create(&c, d, 4, nullptr, 0, 0) == PGENHIP_OK) pgenhip_destroy(c);
        }
    });
    OnExit warm_up_join{[&] {
        if (hip_warm_up.joinable()) hip_warm_up.join();
    }};
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    const IdxRecords &var_idx_rcds = sel.var_idx_rcds;
    const std::string header = vcf_header(sel.sam_idx_rcs, sel.sam_header);
    st.seconds_filter = now_s() - t0;

    Fd out(filename, O_WRONLY | O_CREAT | O_TRUNC);  // :136 File::create
    const int fd = out.get();
    const unsigned n_compress = (unsigned)(opt.compress_threads > 0 ? opt.compress_threads : std::min(32u, std::max(1u, std::thread::hardware_concurrency())));
    if (opt.bgzf) {
        BgzfWriter hw(fd, filename, opt.bgzf_level, 1);
        hw.write(header.data(), header.size());   // its own BGZF member(s); the body's members follow
        st.file_bytes = hw.bytes_out();
    } else {
        pwrite_exact(fd, header.data(), header.size(), 0, filename);  // :139-146
    }
    // BGZF: every member is independent, so the shards' streams simply follow each other; shard 0 appends to the file itself, the
    // others to temporary files that are appended in shard order at the end (one device: no temporary file).  A shard creates its
    // file with O_EXCL after every name has been unlinked, so nothing found at a name is followed or appended, and every file this
    // run created is unlinked on the way out.
    auto shard_tmp = [&](size_t g) { return filename + ".shard" + std::to_string(g) + ".tmp"; };
    std::vector<char> tmp_made;   // per shard: its temporary file exists
    OnExit unlink_tmps{[&] {
        for (size_t g = 1; g < tmp_made.size(); g++)
            if (tmp_made[g]) unlink(shard_tmp(g).c_str());
    }};
    auto finish_bgzf = [&] {
        std::vector<uint8_t> buf(8u << 20);
        for (size_t g = 1; g < tmp_made.size(); g++) {
            if (!tmp_made[g]) continue;   // a shard without variants made none
            const std::string tmp = shard_tmp(g);
            const Fd in(tmp, O_RDONLY);
            for (;;) {
                ssize_t r = read(in.get(), buf.data(), buf.size());
                if (r < 0 && errno == EINTR) continue;
                if (r < 0) throw PfileError("read " + tmp + ": " + std::strerror(errno));
                if (r == 0) break;
                out.write_all(buf.data(), (size_t)r);
                st.file_bytes += (uint64_t)r;
            }
            unlink(tmp.c_str());
            tmp_made[g] = 0;
        }
        BgzfWriter ew(fd, filename, opt.bgzf_level, 1);
        ew.finish();
        st.file_bytes += ew.bytes_out();
    };

    // ---- geometry of the body (:156-192): line j = prefix_j + K x "\tA/B" + "\n"
    const KeptSamples kept = check_selection(*this, sel);
    const uint32_t R = variant_record_size();
    const size_t V = var_idx_rcds.size();
    const uint64_t K = kept.rows.size();
    std::vector<uint64_t> file_off(V + 1, 0);  // body-relative offset of each line
    uint64_t max_prefix = 0;
    for (size_t j = 0; j < V; j++) {
        uint64_t plen = 2;  // "GT" (:161)
        for (const auto &col : var_idx_rcds[j].second) plen += col.size() + 1;  // col + '\t' (:157-160)
        max_prefix = std::max(max_prefix, plen);
        file_off[j + 1] = file_off[j] + plen + 4ull * K + 1ull;
    }
    const uint64_t max_line = max_prefix + 4ull * K + 1ull;
    st.variants = V;
    st.samples_kept = K;
    st.header_bytes = header.size();
    st.body_bytes = file_off[V];
    if (!opt.bgzf) st.file_bytes = st.header_bytes + st.body_bytes;
    if (V == 0) {
        if (opt.bgzf) finish_bgzf();
        out.close();
        return st;
    }

    if (hip_warm_up.joinable()) hip_warm_up.join();
    const Shards shards(opt, "no HIP device: the GT decode/emit path has no CPU fallback");
    const size_t G = (size_t)shards.G;
    const double t_body = now_s();
    std::vector<double> kernel_s(G, 0.0), setup_s(G, 0.0);
    std::vector<uint64_t> shard_out(G, 0);   // BGZF: compressed bytes per shard
    if (opt.bgzf) {
        for (size_t g = 1; g < G; g++) unlink(shard_tmp(g).c_str());
        tmp_made.assign(G, 0);
    }
    const std::string pgen = pgen_path();
    const unsigned compress_threads = std::max(1u, n_compress / (unsigned)std::max(1, std::min(shards.G, shards.n_use)));

    // Per shard: two buffer sets, each with its own ctx/stream.  The producer (the shard's thread) reads records + builds prefixes
    // for block k and queues H2D -> kernel -> D2H on set k%2; a consumer thread waits for that set, writes its text at the
    // precomputed file offset, and hands the set back.  File staging, PCIe copies, the kernel and the file writes of neighbouring
    // blocks overlap.
    shards.run(V, [&](int g, int device, size_t begin, size_t end) {
        const double t_worker = now_s();
        const Fd pgen_fd(pgen, O_RDONLY);  // :149 (unbuffered on purpose, :150-152)
        // BGZF: this shard's ordered, parallel deflate writer (shard 0: the output file behind the header; others: a temporary file)
        std::optional<Fd> tmp;
        std::optional<BgzfWriter> zw;
        if (opt.bgzf && g > 0) {
            tmp.emplace(shard_tmp((size_t)g), O_WRONLY | O_CREAT | O_EXCL);
            tmp_made[(size_t)g] = 1;
        }
        if (opt.bgzf) zw.emplace(tmp ? tmp->get() : fd, tmp ? shard_tmp((size_t)g) : filename, opt.bgzf_level, compress_threads);

        // ---- block and launch plan
        // variants per block: bounded by the text budget — and by the same budget of RECORD bytes, so that a run that keeps few
        // samples (little text per record) still moves in several blocks and its file reads overlap the copies and the kernel
        const uint64_t bv = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(opt.block_text_bytes / max_line, opt.block_text_bytes / std::max<uint32_t>(R, 1u)), end - begin));
        const size_t n_blocks = (end - begin + (size_t)bv - 1) / (size_t)bv;
        // A block is the unit of file staging, of the D2H copy and of the file write.  A LAUNCH covers several consecutive blocks
        // (up to the launch budget of text or record bytes): its records are staged block by block while the blocks of the launch
        // before it are copied out and written, so the host pipeline keeps the cadence of small blocks and the kernel sees launches
        // of up to 2 GiB (a 128-MiB launch of the chr22 shape is two work items deep: 39 us where its share of a large launch costs
        // 25 us, profiles/r03_cli_kernels.md).  Launch sizes ramp 1, 2, 4, ... blocks so the first byte leaves as early as before.
        const uint64_t blocks_per_launch_max = std::max<uint64_t>(1, std::min<uint64_t>(opt.launch_bytes / std::max<uint64_t>(1, std::max<uint64_t>(bv * max_line, bv * R)), n_blocks));
        struct LaunchPlan {
            size_t first_block, n_blocks;
        };
        std::vector<LaunchPlan> plan;
        size_t widest = 1;
        for (size_t k = 0, step = 1; k < n_blocks; step = (size_t)std::min<uint64_t>(2 * (uint64_t)step, blocks_per_launch_max)) {
            const size_t n = (size_t)std::min<uint64_t>(std::min<uint64_t>(step, blocks_per_launch_max), n_blocks - k);
            plan.push_back(LaunchPlan{k, n});
            widest = std::max(widest, n);
            k += n;
        }
        const uint64_t lv = std::min<uint64_t>(bv * widest, end - begin);   // variants of the widest launch
        auto launch_b0 = [&](size_t u) { return begin + plan[u].first_block * (size_t)bv; };
        auto launch_nv = [&](size_t u) { return std::min<size_t>(plan[u].n_blocks * (size_t)bv, end - launch_b0(u)); };

        // ---- buffers: device sets (one launch each) with their own ctx / stream, sized for the widest launch
        const int n_sets = plan.size() > 1 ? 2 : 1;
        const int n_text = n_blocks > 1 ? 2 : 1;   // pinned text buffers (one block each)
        struct DeviceSet {
            pgenhip_ctx *ctx;
            uint8_t *rec;
            char *blob;
            uint64_t *poff, *loff;   // prefix and line offsets of the launch
            uint8_t *text;
        };
        std::optional<DeviceCtx> ctxs[2];
        DeviceSet sets[2] = {};
        for (int s = 0; s < n_sets; s++) {
            DeviceCtx &c = ctxs[s].emplace(device, num_samples, &kept);
            sets[s].ctx = c.get();
            sets[s].rec = c.device<uint8_t>((size_t)(lv * R), "device records");
            sets[s].blob = c.device<char>((size_t)(lv * max_prefix), "device prefixes");
            sets[s].poff = c.device<uint64_t>((size_t)(2 * (lv + 1) * sizeof(uint64_t)), "device offsets");
            sets[s].loff = sets[s].poff + (lv + 1);
            sets[s].text = c.device<uint8_t>((size_t)(lv * max_line), "device text");
        }
        // pinned staging through set 0's ctx: ONE set of input buffers (each block's H2D is waited for before the next block is
        // staged) and the text buffers
        uint8_t *h_rec = ctxs[0]->pinned<uint8_t>((size_t)(bv * R), "pinned records");
        char *h_blob = ctxs[0]->pinned<char>((size_t)(bv * max_prefix), "pinned prefixes");
        uint64_t *h_poff = ctxs[0]->pinned<uint64_t>((size_t)(2 * (bv + 1) * sizeof(uint64_t)), "pinned offsets");
        uint64_t *h_loff = h_poff + (bv + 1);
        uint8_t *h_text[2] = {nullptr, nullptr};
        for (int t = 0; t < n_text; t++) h_text[t] = ctxs[0]->pinned<uint8_t>((size_t)(bv * max_line), "pinned text");

        // ---- consumer: waits for a block's D2H copy, writes its text and hands the text buffer back
        struct InFlight {
            int text;      // pinned text buffer
            int set;       // device set (stream) the copy was queued on
            bool first;    // first block of its launch: the kernel's time is read here
            size_t b0;
            uint64_t bytes;
        };
        std::mutex mu;
        std::condition_variable cv;
        std::deque<InFlight> inflight;
        bool text_busy[2] = {false, false};
        uint64_t pushed[2] = {0, 0}, consumed[2] = {0, 0};   // blocks per device set
        bool producer_done = false;
        std::string consumer_err;
        std::thread consumer([&] {
            try {
                for (;;) {
                    InFlight job;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return !inflight.empty() || producer_done; });
                        if (inflight.empty()) return;
                        job = inflight.front();
                        inflight.pop_front();
                    }
                    check(pgenhip_wait(sets[job.set].ctx), "pgenhip_wait");
                    float ms = 0;
                    if (job.first && pgenhip_timer_read(sets[job.set].ctx, &ms) == PGENHIP_OK) kernel_s[(size_t)g] += ms * 1e-3;
                    if (zw)
                        zw->write(h_text[job.text], (size_t)job.bytes);   // blocks arrive in order: the members are appended in order
                    else   // every line has a known length, so ranges land at precomputed offsets in any order
                        pwrite_span(fd, h_text[job.text], (size_t)job.bytes, header.size() + file_off[job.b0], filename, opt.write_threads);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        text_busy[job.text] = false;
                        consumed[job.set]++;
                    }
                    cv.notify_all();
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                consumer_err = e.what();
                text_busy[0] = text_busy[1] = false;
                cv.notify_all();
            }
        });
        auto join_consumer = [&] {
            {
                std::lock_guard<std::mutex> lk(mu);
                producer_done = true;
            }
            cv.notify_all();
            if (consumer.joinable()) consumer.join();
        };
        OnExit consumer_join{join_consumer};   // before the buffers it reads are freed

        // ---- block j of launch u: records from the file, prefixes joined, offsets — into the pinned staging set, then to their
        // place in the launch's device buffers (on the launch's own stream, idle by now: see wait_set_idle)
        std::vector<uint64_t> blob_len(plan.size(), 0);   // prefix bytes staged so far, per launch
        auto stage_block = [&](size_t u, size_t j) {
            const DeviceSet &D = sets[u % (size_t)n_sets];
            const size_t r0 = j * (size_t)bv, b0 = launch_b0(u) + r0;
            const size_t nv = std::min<size_t>((size_t)bv, end - b0);
            // :165-170 once per run of consecutive variant indices instead of once per variant
            for (size_t j2 = 0; j2 < nv;) {
                size_t run = 1;
                // (variable-width files: consecutive plain records are adjacent on disk too when nothing compressed lies between them)
                while (j2 + run < nv && var_idx_rcds[b0 + j2 + run].first == var_idx_rcds[b0 + j2].first + run &&
                       record_offset(var_idx_rcds[b0 + j2 + run].first) == record_offset(var_idx_rcds[b0 + j2].first) + run * (uint64_t)R)
                    run++;
                pread_span(pgen_fd.get(), h_rec + j2 * R, run * (size_t)R, record_offset(var_idx_rcds[b0 + j2].first), pgen, opt.read_threads);
                j2 += run;
            }
            // :157-161 joined once per variant: col '\t' col '\t' ... "GT"; offsets count from the start of the LAUNCH's blob / text
            const uint64_t blob0 = blob_len[u], text0 = file_off[launch_b0(u)];
            uint64_t bp = 0;
            for (size_t i = 0; i < nv; i++) {
                h_poff[i] = blob0 + bp;
                h_loff[i] = file_off[b0 + i] - text0;
                for (const auto &col : var_idx_rcds[b0 + i].second) {
                    std::memcpy(h_blob + bp, col.data(), col.size());
                    bp += col.size();
                    h_blob[bp++] = '\t';
                }
                h_blob[bp++] = 'G';
                h_blob[bp++] = 'T';
            }
            h_poff[nv] = blob0 + bp;                       // (the next block's first entry, or the launch's end)
            h_loff[nv] = file_off[b0 + nv] - text0;
            blob_len[u] = blob0 + bp;
            check(pgenhip_memcpy_h2d(D.ctx, D.rec + r0 * (size_t)R, h_rec, nv * (size_t)R), "H2D records");
            check(pgenhip_memcpy_h2d(D.ctx, D.blob + blob0, h_blob, (size_t)bp), "H2D prefixes");
            check(pgenhip_memcpy_h2d(D.ctx, D.poff + r0, h_poff, (nv + 1) * sizeof(uint64_t)), "H2D prefix offsets");
            check(pgenhip_memcpy_h2d(D.ctx, D.loff + r0, h_loff, (nv + 1) * sizeof(uint64_t)), "H2D line offsets");
            check(pgenhip_wait(D.ctx), "pgenhip_wait");   // the staging set is free again
        };
        auto launch = [&](size_t u) {
            const DeviceSet &D = sets[u % (size_t)n_sets];
            check(pgenhip_timer_start(D.ctx), "timer");
            check(pgenhip_emit_lines(D.ctx, D.rec, R, nullptr, (uint32_t)launch_nv(u), D.blob, D.poff, D.loff, max_prefix, D.text, 0), "pgenhip_emit_lines");
            check(pgenhip_timer_mark(D.ctx), "timer");
        };
        // block j of launch u leaves: D2H into a free pinned text buffer, then the consumer's
        auto drain_block = [&](size_t u, size_t j) {
            const int si = (int)(u % (size_t)n_sets), ti = (int)((plan[u].first_block + j) % (size_t)n_text);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !text_busy[ti] || !consumer_err.empty(); });
                if (!consumer_err.empty()) throw PfileError(consumer_err);
                text_busy[ti] = true;
            }
            const size_t b0 = launch_b0(u) + j * (size_t)bv, nv = std::min<size_t>((size_t)bv, end - b0);
            const uint64_t block_bytes = file_off[b0 + nv] - file_off[b0];
            check(pgenhip_memcpy_d2h(sets[si].ctx, h_text[ti], sets[si].text + (file_off[b0] - file_off[launch_b0(u)]), (size_t)block_bytes), "D2H text");
            {
                std::lock_guard<std::mutex> lk(mu);
                inflight.push_back(InFlight{ti, si, j == 0, b0, block_bytes});
                pushed[si]++;
            }
            cv.notify_all();
        };
        // a device set is staged into again only once every block of its previous launch has been written: its stream is idle
        // then, so the producer's waits in stage_block never meet the consumer's on the same stream
        auto wait_set_idle = [&](size_t u) {
            const int si = (int)(u % (size_t)n_sets);
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return consumed[si] == pushed[si] || !consumer_err.empty(); });
            if (!consumer_err.empty()) throw PfileError(consumer_err);
        };

        // ---- schedule
        setup_s[(size_t)g] = now_s() - t_worker;
        for (size_t j = 0; j < plan[0].n_blocks; j++) stage_block(0, j);
        launch(0);
        for (size_t u = 0; u < plan.size(); u++) {
            const size_t n_u = plan[u].n_blocks, n_next = u + 1 < plan.size() ? plan[u + 1].n_blocks : 0;
            size_t staged = 0;
            for (size_t j = 0; j < n_u; j++) {
                drain_block(u, j);
                // the next launch's share of staging, so that it is complete when this launch's last block has been queued
                while (staged < n_next && staged * n_u < (j + 1) * n_next) {
                    if (staged == 0) wait_set_idle(u + 1);
                    stage_block(u + 1, staged++);
                }
            }
            if (n_next) launch(u + 1);
        }
        join_consumer();
        if (!consumer_err.empty()) throw PfileError(consumer_err);
        if (zw) shard_out[(size_t)g] = zw->bytes_out();
        if (tmp) tmp->close();
    });
    if (opt.bgzf) {
        st.file_bytes += shard_out[0];
        finish_bgzf();
    }
    out.close();
    st.seconds_body = now_s() - t_body;
    st.seconds_kernel = *std::max_element(kernel_s.begin(), kernel_s.end());
    st.seconds_setup = *std::max_element(setup_s.begin(), setup_s.end());
    return st;
}

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

// The block loop of freq and sample-counts.  Per shard: blocks of bv variants.  Block k's records are read into pinned buffer k % 2
// while the device copies and counts block k - 1; each block's H2D copy and count launch are queued on the ctx stream.
// Fixed-width files: runs of consecutive records are read in one go and packed at stride R.  Variable-width files: the plain
// records are staged as they lie on disk (a span grows over gaps of up to R bytes, so a block stages at most 2R bytes per
// variant) and counted through their offsets in the staged bytes (the `_at` entry points).
// make(ctx, bv) builds a shard's counter, which provides
//   launch(ctx, d_rec, d_off, b0, nv, nh): queue the block's count launch over its nv rows (and the nh halo rows staged behind
//     them; d_off NULL: records packed at stride R; b0: index of the block's first variant in `vars`);
//   copy(ctx, nv): queue what goes back after it (outside the kernel timer);
//   collect(b0, nv): the block's work on the stream has finished (b0: index of its first variant in `vars`);
//   finish(ctx): after the shard's last block has been collected.
// halo: rows behind a block's own that are staged with it (ld: a block's left rows and the `window` rows that follow them, which
// may belong to the next block or shard); launch gets their number as its last argument.  0: a block is its own rows.
template <class Make>
void count_blocks(const Pfile &pf, const Pfile::IdxRecords &vars, const KeptSamples &kept, const OutputOptions &opt, const char *no_device,
                  OutputStats &st, const Make &make, size_t halo = 0)
{
    const uint32_t R = pf.variant_record_size();
    const Shards shards(opt, no_device);
    std::vector<double> kernel_s((size_t)shards.G, 0.0), setup_s((size_t)shards.G, 0.0);
    const std::string pgen = pf.pgen_path();
    const bool vw = pf.variable_width();
    shards.run(vars.size(), [&](int g, int device, size_t begin, size_t end) {
        const double t_worker = now_s();
        const Fd pgen_fd(pgen, O_RDONLY);
        const uint64_t bv = std::max<uint64_t>(1, std::min<uint64_t>(opt.block_text_bytes / R, end - begin));
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
            counter.launch(ctx.get(), d_rec, d_off, b0, (uint32_t)nv, (uint32_t)nh);
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

// freq's counter: 16 bytes per variant, copied back block by block
struct VariantCounter {
    uint32_t R;
    std::vector<uint32_t> &counts;   // 4 per kept variant
    uint32_t *d_counts, *h_counts;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t) const
    {
        if (d_off)
            check(pgenhip_genotype_counts_at(ctx, d_rec, d_off, nv, d_counts, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts_at");
        else
            check(pgenhip_genotype_counts(ctx, d_rec, R, nullptr, nv, d_counts, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts");
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_counts, d_counts, nv * 16), "D2H counts"); }
    void collect(size_t b0, size_t nv) const { std::memcpy(counts.data() + 4 * b0, h_counts, nv * 16); }
    void finish(pgenhip_ctx *) const {}
};

// sample-counts' counter: every block of the shard accumulates into one device buffer of 16 bytes per kept sample (the first
// overwrites it), copied back once; the host sums the shards in u64
struct SampleCounter {
    uint32_t R;
    size_t K;
    std::vector<uint64_t> &totals;   // 4 per kept sample
    std::mutex &mu;
    uint32_t *d_counts, *h_counts;
    bool first = true;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t)
    {
        const uint32_t flags = PGENHIP_SCOUNT_AUTO | (first ? 0u : PGENHIP_SCOUNT_ACCUMULATE);
        first = false;
        if (d_off)
            check(pgenhip_sample_counts_at(ctx, d_rec, d_off, nv, d_counts, flags), "pgenhip_sample_counts_at");
        else
            check(pgenhip_sample_counts(ctx, d_rec, R, nullptr, nv, d_counts, flags), "pgenhip_sample_counts");
    }
    void copy(pgenhip_ctx *, size_t) const {}
    void collect(size_t, size_t) const {}
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
struct ScoreCounter {
    uint32_t R;
    size_t K, C;                      // kept samples, score columns
    bool impute;
    const std::vector<float> &w;      // matched rows x C, the sign of REF-effect rows flipped
    std::vector<double> &sums;        // K x C
    std::vector<uint64_t> &missing;   // K
    std::mutex &mu;
    float *d_w, *d_miss, *h_miss;
    uint32_t *d_gc, *h_gc, *d_counts, *h_counts;
    double *d_scores, *h_scores;
    bool first = true;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t b0, uint32_t nv, uint32_t)
    {
        if (impute) {
            if (d_off)
                check(pgenhip_genotype_counts_at(ctx, d_rec, d_off, nv, d_gc, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts_at");
            else
                check(pgenhip_genotype_counts(ctx, d_rec, R, nullptr, nv, d_gc, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts");
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
            if (d_off)
                check(pgenhip_sample_scores_at(ctx, d_rec, d_off, nv, d_w + c0, C, cg, impute ? d_miss : nullptr, dst, PGENHIP_SCORE_AUTO | acc), "pgenhip_sample_scores_at");
            else
                check(pgenhip_sample_scores(ctx, d_rec, R, nullptr, nv, d_w + c0, C, cg, impute ? d_miss : nullptr, dst, PGENHIP_SCORE_AUTO | acc), "pgenhip_sample_scores");
        }
        const uint32_t cflags = PGENHIP_SCOUNT_AUTO | (first ? 0u : PGENHIP_SCOUNT_ACCUMULATE);
        if (d_off)
            check(pgenhip_sample_counts_at(ctx, d_rec, d_off, nv, d_counts, cflags), "pgenhip_sample_counts_at");
        else
            check(pgenhip_sample_counts(ctx, d_rec, R, nullptr, nv, d_counts, cflags), "pgenhip_sample_counts");
        first = false;
    }
    void copy(pgenhip_ctx *, size_t) const {}
    void collect(size_t, size_t) const {}
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
struct AssocCounter {
    uint32_t R;
    size_t C, bv;                     // value columns, rows of a full block
    std::vector<uint32_t> &counts;    // 4 per kept variant
    std::vector<double> &sums;        // per kept variant C x 4
    const double *d_values;
    uint32_t *d_gc, *h_gc;
    double *d_sums, *h_sums;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t) const
    {
        if (d_off)
            check(pgenhip_genotype_counts_at(ctx, d_rec, d_off, nv, d_gc, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts_at");
        else
            check(pgenhip_genotype_counts(ctx, d_rec, R, nullptr, nv, d_gc, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts");
        for (size_t c0 = 0; c0 < C; c0 += PGENHIP_VSUM_MAX_COLUMNS) {
            const uint32_t cg = (uint32_t)std::min<size_t>(PGENHIP_VSUM_MAX_COLUMNS, C - c0);
            double *dst = d_sums + bv * 4 * c0;
            if (d_off)
                check(pgenhip_variant_sums_at(ctx, d_rec, d_off, nv, d_values + c0, C, cg, dst, PGENHIP_VSUM_AUTO), "pgenhip_variant_sums_at");
            else
                check(pgenhip_variant_sums(ctx, d_rec, R, nullptr, nv, d_values + c0, C, cg, dst, PGENHIP_VSUM_AUTO), "pgenhip_variant_sums");
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
    void finish(pgenhip_ctx *) const {}
};

// matrix's "counter": every block is decoded into one device buffer, copied back and written to its place in the .npy file.
// Variant-major: a block is nv consecutive rows of the file, one pwrite.  Sample-major: a block is a column band, K pieces of
// nv elements, written from a few threads.
constexpr unsigned kMatrixWriteThreads = 4;   // a constant like the BGZF pool's cap, never the machine's CPU count
struct MatrixWriter {
    uint32_t R;
    size_t K, V;
    const MatrixOptions &m;
    uint64_t pitch;   // sample-major: bytes between the device buffer's rows (a multiple of 128)
    uint8_t *d_out, *h_out;
    int fd;
    const std::string &path;
    uint64_t data_off;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t) const
    {
        const uint32_t flags = PGENHIP_MATRIX_AUTO | (m.sample_major ? PGENHIP_MATRIX_SAMPLE_MAJOR : 0u);
        const uint64_t stride = m.sample_major ? pitch : (uint64_t)K * m.elem_bytes;
        if (d_off)
            check(pgenhip_decode_matrix_at(ctx, d_rec, d_off, nv, d_out, stride, m.elem_bytes, m.values, flags), "pgenhip_decode_matrix_at");
        else
            check(pgenhip_decode_matrix(ctx, d_rec, R, nullptr, nv, d_out, stride, m.elem_bytes, m.values, flags), "pgenhip_decode_matrix");
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
    void finish(pgenhip_ctx *) const {}
};

// export's "counter": every block's packed records come back and are written to their place in the .pgen / .bed
struct PackWriter {
    uint32_t R;
    size_t RK;
    const uint8_t *code_map;   // NULL: the identity
    uint8_t *d_out, *h_out;
    int fd;
    const std::string &path;
    uint64_t data_off;
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t) const
    {
        if (d_off)
            check(pgenhip_pack_records_at(ctx, d_rec, d_off, nv, d_out, RK, code_map, PGENHIP_PACK_AUTO), "pgenhip_pack_records_at");
        else
            check(pgenhip_pack_records(ctx, d_rec, R, nullptr, nv, d_out, RK, code_map, PGENHIP_PACK_AUTO), "pgenhip_pack_records");
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const { check(pgenhip_memcpy_d2h(ctx, h_out, d_out, nv * RK), "D2H packed records"); }
    void collect(size_t b0, size_t nv) const { pwrite_exact(fd, h_out, nv * RK, data_off + (uint64_t)b0 * RK, path); }
    void finish(pgenhip_ctx *) const {}
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
struct PairWriter {
    uint32_t R, W;
    const LdOptions &ld;
    const Pfile::IdxRecords &vars;
    const size_t (&col)[3];   // CHROM, POS, ID
    std::map<size_t, std::string> &pieces;
    std::mutex &mu;
    uint8_t *d_out, *h_out;
    size_t entry_bytes() const { return ld.counts ? 64u : 4u; }
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t nh) const
    {
        const uint32_t flags = ld.counts ? PGENHIP_PAIR_TABLE : PGENHIP_PAIR_R2;
        if (d_off)
            check(pgenhip_pair_stats_at(ctx, d_rec, d_off, nv + nh, nv, W, d_out, flags), "pgenhip_pair_stats_at");
        else
            check(pgenhip_pair_stats(ctx, d_rec, R, nullptr, nv + nh, nv, W, d_out, flags), "pgenhip_pair_stats");
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
    void finish(pgenhip_ctx *) const {}
};

// kinship's counter: the upper block triangle of sample-pair tables, one device buffer per pair of rank tiles (ta <= tb); the
// shard's first block overwrites them, the others accumulate; they come back once per shard and the host adds the shards in u32
// (exact: a cell is at most the number of kept variants, which is a u32)
struct KinshipCounter {
    uint32_t R, K, tile, tiles;
    std::vector<std::vector<uint32_t>> &totals;   // per pair of tiles, in the order of `bufs`
    std::mutex &mu;
    std::vector<uint32_t *> bufs;                 // device: 16 u32 per pair of ranks of tiles (ta, tb), ta <= tb, row-major over ta, tb
    uint32_t *h_buf;                              // pinned, the largest buffer's size
    bool first = true;
    uint32_t count(uint32_t t) const { return std::min(tile, K - t * tile); }
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t, uint32_t nv, uint32_t)
    {
        const uint32_t flags = PGENHIP_SPAIR_AUTO | (first ? 0u : PGENHIP_SPAIR_ACCUMULATE);
        first = false;
        size_t p = 0;
        for (uint32_t ta = 0; ta < tiles; ta++)
            for (uint32_t tb = ta; tb < tiles; tb++, p++) {
                if (d_off)
                    check(pgenhip_sample_pair_stats_at(ctx, d_rec, d_off, nv, ta * tile, count(ta), tb * tile, count(tb), bufs[p], flags), "pgenhip_sample_pair_stats_at");
                else
                    check(pgenhip_sample_pair_stats(ctx, d_rec, R, nullptr, nv, ta * tile, count(ta), tb * tile, count(tb), bufs[p], flags), "pgenhip_sample_pair_stats");
            }
    }
    void copy(pgenhip_ctx *, size_t) const {}
    void collect(size_t, size_t) const {}
    void finish(pgenhip_ctx *ctx) const
    {
        size_t p = 0;
        for (uint32_t ta = 0; ta < tiles; ta++)
            for (uint32_t tb = ta; tb < tiles; tb++, p++) {
                const size_t words = (size_t)16 * count(ta) * count(tb);
                check(pgenhip_memcpy_d2h(ctx, h_buf, bufs[p], words * 4), "D2H sample-pair tables");
                check(pgenhip_wait(ctx), "pgenhip_wait");
                std::lock_guard<std::mutex> lk(mu);
                uint32_t *dst = totals[p].data();
                for (size_t i = 0; i < words; i++) dst[i] += h_buf[i];
            }
    }
};

// grm's counter: per block the variants' counts come back, the host makes the two tables per variant and every pair of rank tiles
// of the upper block triangle gets two Gram launches (G, then N); the shard's first block overwrites the buffers, the others
// accumulate; they come back once per shard, filed under the shard's first variant so that the host can add the shards in order
struct GramCounter {
    uint32_t R, K, tile, tiles;
    size_t bv;                                               // rows of a block at most: the N tables lie 4 * bv doubles behind the G tables
    std::map<size_t, std::vector<std::vector<double>>> &sums;   // shard's first variant -> per pair of tiles, G at 2 p, N at 2 p + 1
    std::mutex &mu;
    uint64_t &skipped;
    std::vector<double *> bufs;                              // device: count(ta) x count(tb) doubles, in the order of `sums`' vectors
    uint32_t *d_counts, *h_counts;
    double *d_tab, *h_tab, *h_buf;                           // h_buf: pinned, the largest buffer's size
    bool first = true;
    size_t first_b0 = 0;
    uint32_t count(uint32_t t) const { return std::min(tile, K - t * tile); }
    void launch(pgenhip_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_off, size_t b0, uint32_t nv, uint32_t)
    {
        if (d_off)
            check(pgenhip_genotype_counts_at(ctx, d_rec, d_off, nv, d_counts, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts_at");
        else
            check(pgenhip_genotype_counts(ctx, d_rec, R, nullptr, nv, d_counts, PGENHIP_COUNT_AUTO), "pgenhip_genotype_counts");
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
        first = false;
        size_t p = 0;
        for (uint32_t ta = 0; ta < tiles; ta++)
            for (uint32_t tb = ta; tb < tiles; tb++, p++)
                for (size_t m = 0; m < 2; m++) {
                    const double *tab = d_tab + m * 4 * bv;
                    if (d_off)
                        check(pgenhip_sample_gram_at(ctx, d_rec, d_off, nv, tab, ta * tile, count(ta), tb * tile, count(tb), bufs[2 * p + m], count(tb), flags), "pgenhip_sample_gram_at");
                    else
                        check(pgenhip_sample_gram(ctx, d_rec, R, nullptr, nv, tab, ta * tile, count(ta), tb * tile, count(tb), bufs[2 * p + m], count(tb), flags), "pgenhip_sample_gram");
                }
    }
    void copy(pgenhip_ctx *, size_t) const {}
    void collect(size_t, size_t) const {}
    void finish(pgenhip_ctx *ctx) const
    {
        if (first) return;   // a shard without variants
        std::vector<std::vector<double>> mine;
        size_t p = 0;
        for (uint32_t ta = 0; ta < tiles; ta++)
            for (uint32_t tb = ta; tb < tiles; tb++, p++)
                for (size_t m = 0; m < 2; m++) {
                    const size_t n = (size_t)count(ta) * count(tb);
                    check(pgenhip_memcpy_d2h(ctx, h_buf, bufs[2 * p + m], n * 8), "D2H Gram matrix");
                    check(pgenhip_wait(ctx), "pgenhip_wait");
                    mine.emplace_back(h_buf, h_buf + n);
                }
        std::lock_guard<std::mutex> lk(mu);
        sums.emplace(first_b0, std::move(mine));
    }
};

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
    for (int c = 0; c < 5; c++) {
        col[c] = std::find(sel.var_header.begin(), sel.var_header.end(), std::string(kCols[c])) - sel.var_header.begin();
        if (col[c] == sel.var_header.size()) throw PfileError(std::string(kCols[c]) + " not among the headers of " + pvar_path());
    }
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const uint32_t R = variant_record_size();
    const size_t V = var_idx_rcds.size();
    st.variants = V;
    st.samples_kept = kept.rows.size();

    std::vector<uint32_t> counts(4 * V, 0u);
    const double t_body = now_s();
    if (V != 0 && R != 0) {
        count_blocks(*this, var_idx_rcds, kept, opt, "no HIP device: the genotype count path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            return VariantCounter{R, counts, ctx.device<uint32_t>((size_t)(16 * bv), "device counts"), ctx.pinned<uint32_t>((size_t)(16 * bv), "pinned counts")};
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
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
    return st;
}

OutputStats Pfile::output_sample_counts(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                        const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    size_t iid = sel.sam_header.size();   // vcf_header's rule (:114-126): the first column named IID
    for (size_t c = 0; c < sel.sam_header.size(); c++) {
        if (sel.sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sel.sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;

    std::vector<uint64_t> totals(4 * K, 0u);
    const double t_body = now_s();
    if (V != 0 && K != 0) {   // else every count is zero and no device is touched
        const uint32_t R = variant_record_size();
        std::mutex mu;
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the sample count path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t) {
            return SampleCounter{R, K, totals, mu, ctx.device<uint32_t>(16 * K, "device counts"), ctx.pinned<uint32_t>(16 * K, "pinned counts")};
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
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
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
    size_t iid = sel.sam_header.size();   // vcf_header's rule (:114-126): the first column named IID
    for (size_t c = 0; c < sel.sam_header.size(); c++) {
        if (sel.sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sel.sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());
    static const char *const kCols[3] = {"ID", "REF", "ALT"};
    size_t col[3];
    for (int c = 0; c < 3; c++) {
        col[c] = std::find(sel.var_header.begin(), sel.var_header.end(), std::string(kCols[c])) - sel.var_header.begin();
        if (col[c] == sel.var_header.size()) throw PfileError(std::string(kCols[c]) + " not among the headers of " + pvar_path());
    }

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
        const uint32_t R = variant_record_size();
        std::mutex mu;
        count_blocks(*this, msel.var_idx_rcds, kept, opt, "no HIP device: the score path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            return ScoreCounter{R, K, C, sopt.mean_imputation, w, sums, missing, mu,
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
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
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
    size_t iid = sel.sam_header.size();   // vcf_header's rule (:114-126): the first column named IID
    for (size_t c = 0; c < sel.sam_header.size(); c++) {
        if (sel.sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sel.sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());
    static const char *const kCols[5] = {"CHROM", "POS", "ID", "REF", "ALT"};
    size_t col[5];
    for (int c = 0; c < 5; c++) {
        col[c] = std::find(sel.var_header.begin(), sel.var_header.end(), std::string(kCols[c])) - sel.var_header.begin();
        if (col[c] == sel.var_header.size()) throw PfileError(std::string(kCols[c]) + " not among the headers of " + pvar_path());
    }

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
        const uint32_t R = variant_record_size();
        count_blocks(*this, sel.var_idx_rcds, kept, opt, "no HIP device: the assoc path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            double *d_values = ctx.device<double>(n * C * sizeof(double), "device values");
            check(pgenhip_memcpy_h2d(ctx.get(), d_values, values.data(), n * C * sizeof(double)), "H2D values");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            return AssocCounter{R, C, b, counts, sums, d_values,
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
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
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
    for (int c = 0; c < 3; c++) {
        col[c] = std::find(sel.var_header.begin(), sel.var_header.end(), std::string(kCols[c])) - sel.var_header.begin();
        if (col[c] == sel.var_header.size()) throw PfileError(std::string(kCols[c]) + " not among the headers of " + pvar_path());
    }
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
        const uint32_t R = variant_record_size();
        const uint32_t W = (uint32_t)std::min<uint64_t>(ld.window, V - 1);   // no pair reaches further
        const uint64_t entry = ld.counts ? 64u : 4u;
        // left rows per block: their W entries each fill the block budget (or --block-rows)
        uint64_t bv = ld.block_rows ? ld.block_rows : std::max<uint64_t>(1, opt.block_text_bytes / ((uint64_t)W * entry));
        bv = std::min<uint64_t>(bv, V);
        OutputOptions blocks = opt;
        blocks.block_text_bytes = bv * R;   // count_blocks sizes its blocks by record bytes
        std::map<size_t, std::string> pieces;
        std::mutex mu;
        count_blocks(*this, sel.var_idx_rcds, kept, blocks, "no HIP device: the pairwise path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t n) {
            const size_t bytes = (size_t)(n * W * entry);
            return PairWriter{R, W, ld, sel.var_idx_rcds, col, pieces, mu, ctx.device<uint8_t>(bytes, "device pair entries"), ctx.pinned<uint8_t>(bytes, "pinned pair entries")};
        }, W);
        for (auto &p : pieces) text += p.second;
    }
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
    return st;
}

OutputStats Pfile::output_kinship(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                  const std::string &filename, const KinshipOptions &kopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    size_t iid = sel.sam_header.size();   // vcf_header's rule (:114-126): the first column named IID
    for (size_t c = 0; c < sel.sam_header.size(); c++) {
        if (sel.sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sel.sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());
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
        const uint32_t tile = std::max<uint32_t>(1u, kopt.tile), tiles = (uint32_t)((K + tile - 1) / tile);
        auto count = [&](uint32_t t) { return (size_t)std::min<uint64_t>(tile, K - (uint64_t)t * tile); };
        std::vector<std::vector<uint32_t>> totals;
        for (uint32_t ta = 0; ta < tiles; ta++)
            for (uint32_t tb = ta; tb < tiles; tb++) totals.emplace_back(16 * count(ta) * count(tb), 0u);
        if (V != 0) {   // else every table is zero and no device is touched
            const uint32_t R = variant_record_size();
            std::mutex mu;
            OutputOptions blocks = opt;
            if (kopt.block_rows) blocks.block_text_bytes = kopt.block_rows * R;   // count_blocks sizes its blocks by record bytes
            count_blocks(*this, sel.var_idx_rcds, kept, blocks, "no HIP device: the kinship path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t) {
                KinshipCounter kc{R, (uint32_t)K, tile, tiles, totals, mu, {}, nullptr};
                for (uint32_t ta = 0; ta < tiles; ta++)
                    for (uint32_t tb = ta; tb < tiles; tb++) kc.bufs.push_back(ctx.device<uint32_t>(64 * count(ta) * count(tb), "device sample-pair tables"));
                kc.h_buf = ctx.pinned<uint32_t>(64 * count(0) * count(0), "pinned sample-pair tables");
                return kc;
            });
        }
        // first buffer of each tile row: pair (ta, tb) is at row_first[ta] + tb - ta
        std::vector<size_t> row_first(tiles);
        for (size_t ta = 0, p = 0; ta < tiles; p += tiles - ta, ta++) row_first[ta] = p;
        char num[32];
        for (size_t a = 0; a < K; a++) {
            const size_t ta = a / tile, i = a % tile;
            for (size_t b = a + 1; b < K; b++) {
                const size_t tb = b / tile, l = b % tile;
                const uint32_t *t = totals[row_first[ta] + tb - ta].data() + 16 * (i * count((uint32_t)tb) + l);
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
    st.body_bytes = text.size() - st.header_bytes;
    st.file_bytes = text.size();
    write_text(text, filename);
    st.seconds_body = now_s() - t_body;
    return st;
}

OutputStats Pfile::output_grm(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &out_prefix, const GrmOptions &gopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    size_t iid = sel.sam_header.size();   // vcf_header's rule (:114-126): the first column named IID
    for (size_t c = 0; c < sel.sam_header.size(); c++) {
        if (sel.sam_header[c] == "IID") {
            iid = c;
            break;
        }
    }
    if (iid == sel.sam_header.size()) throw PfileError("IID not among the headers of " + psam_path());
    st.seconds_filter = now_s() - t0;

    const KeptSamples kept = check_selection(*this, sel);
    const size_t V = sel.var_idx_rcds.size(), K = kept.rows.size();
    st.variants = V;
    st.samples_kept = K;
    const double t_body = now_s();

    const uint32_t tile = std::max<uint32_t>(1u, gopt.tile), tiles = (uint32_t)((K + tile - 1) / tile);
    auto count = [&](uint32_t t) { return (size_t)std::min<uint64_t>(tile, K - (uint64_t)t * tile); };
    // per pair of tiles (ta <= tb, row-major), G at 2 p and N at 2 p + 1: the shards' sums, added in shard order
    std::vector<std::vector<double>> totals;
    for (uint32_t ta = 0; ta < tiles; ta++)
        for (uint32_t tb = ta; tb < tiles; tb++)
            for (int m = 0; m < 2; m++) totals.emplace_back(count(ta) * count(tb), 0.0);
    if (K != 0 && V != 0) {   // else nothing is summed and no device is touched
        const uint32_t R = variant_record_size();
        std::mutex mu;
        std::map<size_t, std::vector<std::vector<double>>> sums;
        OutputOptions blocks = opt;
        if (gopt.block_rows) blocks.block_text_bytes = gopt.block_rows * R;   // count_blocks sizes its blocks by record bytes
        count_blocks(*this, sel.var_idx_rcds, kept, blocks, "no HIP device: the grm path has no CPU fallback", st, [&](DeviceCtx &ctx, uint64_t bv) {
            GramCounter gc{R, (uint32_t)K, tile, tiles, (size_t)bv, sums, mu, st.grm_skipped, {}, nullptr, nullptr, nullptr, nullptr, nullptr};
            for (uint32_t ta = 0; ta < tiles; ta++)
                for (uint32_t tb = ta; tb < tiles; tb++)
                    for (int m = 0; m < 2; m++) gc.bufs.push_back(ctx.device<double>(8 * count(ta) * count(tb), "device Gram matrix"));
            gc.d_counts = ctx.device<uint32_t>((size_t)(16 * bv), "device counts");
            gc.h_counts = ctx.pinned<uint32_t>((size_t)(16 * bv), "pinned counts");
            gc.d_tab = ctx.device<double>((size_t)(64 * bv), "device code values");
            gc.h_tab = ctx.pinned<double>((size_t)(64 * bv), "pinned code values");
            gc.h_buf = ctx.pinned<double>(8 * count(0) * count(0), "pinned Gram matrix");
            return gc;
        });
        for (const auto &shard : sums)   // ordered by the shard's first variant
            for (size_t q = 0; q < totals.size(); q++)
                for (size_t i = 0; i < totals[q].size(); i++) totals[q][i] += shard.second[q][i];
    }
    // first buffer pair of each tile row: pair (ta, tb) is at row_first[ta] + tb - ta
    std::vector<size_t> row_first(tiles);
    for (size_t ta = 0, p = 0; ta < tiles; p += tiles - ta, ta++) row_first[ta] = p;
    // entry (a, b) of matrix m, read from the block that holds (min, max): the square written is exactly symmetric
    auto entry = [&](size_t a, size_t b, size_t m) {
        const size_t lo = std::min(a, b), hi = std::max(a, b);
        const size_t ta = lo / tile, tb = hi / tile;
        return totals[2 * (row_first[ta] + tb - ta) + m][(lo % tile) * count((uint32_t)tb) + hi % tile];
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

OutputStats Pfile::output_matrix(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                 const std::string &filename, const MatrixOptions &mopt, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    const Selection sel = select(sam_query, var_query, opt.filter_threads);
    auto column = [](const StringRecord &header, const char *name, const std::string &file) {
        for (size_t c = 0; c < header.size(); c++)
            if (header[c] == name) return c;
        throw PfileError(std::string(name) + " not among the headers of " + file);
    };
    const size_t id_col = column(sel.var_header, "ID", pvar_path()), iid_col = column(sel.sam_header, "IID", psam_path());
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
        const uint32_t R = variant_record_size();
        // variants per block: block_text_bytes of matrix; a sample-major block is a column band whose row pieces hold at least
        // 4 096 elements where a 1-GiB buffer allows
        uint64_t bv = std::max<uint64_t>(1, opt.block_text_bytes / ((uint64_t)K * E));
        if (mopt.sample_major) bv = std::max<uint64_t>(bv, std::max<uint64_t>(1, std::min<uint64_t>(4096, (1ull << 30) / ((uint64_t)K * E))));
        bv = std::min<uint64_t>(bv, V);
        OutputOptions blocks = opt;
        blocks.block_text_bytes = bv * R;   // count_blocks sizes its blocks by record bytes
        count_blocks(*this, sel.var_idx_rcds, kept, blocks, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t n) {
            const uint64_t pitch = (n * E + 127) / 128 * 128;
            const size_t bytes = (size_t)(mopt.sample_major ? (uint64_t)K * pitch : n * K * E);
            return MatrixWriter{R, K, V, mopt, pitch, ctx.device<uint8_t>(bytes, "device matrix"), ctx.pinned<uint8_t>(bytes, "pinned matrix"),
                                out.get(), filename, (uint64_t)header.size()};
        });
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
    auto column = [](const StringRecord &header, const char *name) {
        for (size_t c = 0; c < header.size(); c++)
            if (header[c] == name) return c;
        return header.size();
    };
    auto need = [&](const StringRecord &header, const char *name, const std::string &file) {
        const size_t c = column(header, name);
        if (c == header.size()) throw PfileError(std::string(name) + " not among the headers of " + file);
        return c;
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
        const size_t chrom = need(vh, "CHROM", pvar_path()), id = need(vh, "ID", pvar_path()), pos = need(vh, "POS", pvar_path()),
                     ref = need(vh, "REF", pvar_path()), alt = need(vh, "ALT", pvar_path());
        for (const auto &vr : sel.var_idx_rcds) {
            const StringRecord &r = vr.second;
            if (r.at(alt).find(',') != std::string::npos)
                throw PfileError("variant " + r.at(id) + " (row " + std::to_string(vr.first) + " of " + pvar_path() + ") has more than one ALT allele (" +
                                 r.at(alt) + "): a .bed holds biallelic variants only");
            var_text += r.at(chrom) + '\t' + r.at(id) + "\t0\t" + r.at(pos) + '\t' + r.at(alt) + '\t' + r.at(ref) + '\n';
        }
        const size_t iid = need(sh, "IID", psam_path()), fid = column(sh, "FID"), pat = column(sh, "PAT"), mat = column(sh, "MAT"), sex = column(sh, "SEX");
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
        const uint32_t R = variant_record_size();
        count_blocks(*this, sel.var_idx_rcds, kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t bytes = (size_t)(bv * RK);
            return PackWriter{R, RK, eopt.bed ? kBedMap : nullptr, ctx.device<uint8_t>(bytes, "device packed records"),
                              ctx.pinned<uint8_t>(bytes, "pinned packed records"), out.get(), out_main, (uint64_t)header.size()};
        });
    }
    out.close();
    write_text(var_text, out_var);
    write_text(sam_text, out_sam);
    st.seconds_body = now_s() - t_body;
    return st;
}

namespace {
uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

void synth_pfile(const std::string &prefix, uint32_t variants, uint32_t samples, uint32_t keep_modulus, uint64_t seed)
{
    const uint32_t R = pgenhip_variant_record_size(samples);
    {
        FILE *f = std::fopen((prefix + ".pvar").c_str(), "wb");
        if (!f) throw PfileError("create " + prefix + ".pvar: " + std::strerror(errno));
        std::fputs("##fileformat=VCFv4.2\n##source=pgen-hip synth\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", f);
        for (uint32_t i = 0; i < variants; i++) std::fprintf(f, "22\t%llu\tsnp%u\tA\tG\t100\tPASS\t.\n", 16050000ull + 7ull * i, i);
        std::fclose(f);
        f = std::fopen((prefix + ".psam").c_str(), "wb");
        if (!f) throw PfileError("create " + prefix + ".psam: " + std::strerror(errno));
        std::fputs("#IID\tSEX\tKEEP\n", f);
        for (uint32_t i = 0; i < samples; i++)
            std::fprintf(f, "S%06u\tNA\t%d\n", i, keep_modulus && splitmix64(0x4D41534Bull ^ (uint64_t)i) % keep_modulus == 0 ? 1 : 0);
        std::fclose(f);
    }
    const Fd out(prefix + ".pgen", O_WRONLY | O_CREAT | O_TRUNC);
    uint8_t hdr[12] = {0x6C, 0x1B, 0x02, 0, 0, 0, 0, 0, 0, 0, 0, 0x40};
    for (int b = 0; b < 4; b++) {
        hdr[3 + b] = (uint8_t)(variants >> (8 * b));
        hdr[7 + b] = (uint8_t)(samples >> (8 * b));
    }
    pwrite_exact(out.get(), hdr, sizeof hdr, 0, prefix + ".pgen");
    if (variants == 0 || R == 0) return;
    DeviceCtx ctx(0, samples);
    const uint64_t bv = std::max<uint64_t>(1, std::min<uint64_t>((256ull << 20) / R, variants));
    uint8_t *h_rec = ctx.pinned<uint8_t>((size_t)(bv * R), "pinned records");
    uint8_t *d_rec = ctx.device<uint8_t>((size_t)(bv * R), "device records");
    for (uint64_t v0 = 0; v0 < variants; v0 += bv) {
        const uint32_t nv = (uint32_t)std::min<uint64_t>(bv, variants - v0);
        check(pgenhip_synth_records(ctx.get(), d_rec, R, v0, nv, seed, 0), "pgenhip_synth_records");
        check(pgenhip_memcpy_d2h(ctx.get(), h_rec, d_rec, (size_t)nv * R), "D2H records");
        check(pgenhip_wait(ctx.get()), "pgenhip_wait");
        pwrite_exact(out.get(), h_rec, (size_t)nv * R, 12ull + v0 * R, prefix + ".pgen");
    }
}

}  // namespace pgenhost
