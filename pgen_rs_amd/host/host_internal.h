// host_internal.h — what pfile.cpp (the restatement of src/pfile.rs) and commands.cpp / assoc.cpp / prune.cpp / import.cpp (the
// commands the reference does not have) share below the public surface of pfile.h: status checks, file spans, the keyed tables that
// score and assoc read, the checked selection, a ctx with its buffers, the shards.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pgen_hip.h"
#include "pfile.h"

namespace pgenhost {

double now_s();   // a steady clock, seconds

// throws a PfileError "<what>: <status text> (<detail>)" unless rc is PGENHIP_OK
void check(int rc, const char *what);

void pwrite_exact(int fd, const void *src, size_t bytes, uint64_t offset, const std::string &path);

// `bytes` of the file at `off` into dst: one pread, or a few at once for long spans (one thread copies ~2-3 GB/s out of the page cache)
void pread_span(int fd, uint8_t *dst, size_t bytes, uint64_t off, const std::string &path, int read_threads);

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

// the first column of `header` named `name`
inline size_t column(const StringRecord &header, const char *name, const std::string &file)
{
    for (size_t c = 0; c < header.size(); c++)
        if (header[c] == name) return c;
    throw PfileError(std::string(name) + " not among the headers of " + file);
}

// vcf_header's rule (src/pfile.rs:114-126): the first .psam column named IID
inline size_t iid_column(const Pfile &pf, const StringRecord &sam_header) { return column(sam_header, "IID", pf.psam_path()); }

// The reader under read_score_weights and read_value_table: a tab-separated file with a header line (a leading '#' allowed) whose
// rows are n_lead text columns, the first of them the row's key, and one value per header cell behind them.  A PfileError names the
// line of a row with another number of cells than the header and of a key that occurs twice (key_name says what the key is);
// too_narrow words the one about a header without a value column.  cell(text, name, where) takes every value cell in row order
// with its column's header cell and "<path> line <n>", and throws what it cannot parse.
struct KeyedRows {
    std::vector<std::string> names;               // the value columns' header cells
    std::vector<std::vector<std::string>> lead;   // per leading column, per row
    std::vector<size_t> lines;                    // the file line each row starts on
};
template <class Cell>
KeyedRows read_keyed_rows(const std::string &path, size_t n_lead, const char *too_narrow, const char *key_name, const Cell &cell)
{
    const std::string data = read_file(path);
    KeyedRows t;
    TsvReader reader(data, !data.empty() && data[0] == '#' ? 1 : 0);
    const StringRecord &head = reader.headers();
    if (head.size() < n_lead + 1) throw PfileError(path + " line 1: " + too_narrow);
    t.names.assign(head.begin() + n_lead, head.end());
    t.lead.resize(n_lead);
    const size_t C = t.names.size();
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
    std::map<std::string, size_t> seen;   // key -> line
    StringRecord rec;
    for (;;) {
        const size_t at = line_at(reader.position());
        const std::string where = path + " line " + std::to_string(at);
        bool more;
        try {
            more = reader.next(rec);
        } catch (const CsvError &) {
            throw PfileError(where + ": expected " + std::to_string(C + n_lead) + " tab-separated cells like the header's");
        }
        if (!more) break;
        const auto dup = seen.emplace(rec[0], at);
        if (!dup.second) throw PfileError(where + ": " + key_name + " '" + rec[0] + "' occurs twice (first on line " + std::to_string(dup.first->second) + ")");
        for (size_t c = 0; c < C; c++) cell(rec[n_lead + c], t.names[c], where);
        for (size_t l = 0; l < n_lead; l++) t.lead[l].push_back(rec[l]);
        t.lines.push_back(at);
    }
    return t;
}

struct KeptSamples {
    std::vector<uint32_t> rows;
    bool all;   // every row kept: the K = N fast path
};

// The kept sample rows (:173: a row past the .pgen's samples is the reference's index panic) and a check of every kept variant
// row: past the .pgen's records, or (variable-width files) not stored as a plain 2-bit record of R bytes, the only kind that can
// take the path of :165-190
KeptSamples check_selection(const Pfile &pf, const Pfile::Selection &sel);

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

}  // namespace pgenhost
