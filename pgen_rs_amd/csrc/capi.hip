// capi.hip — the extern "C" boundary of libpgen_hip.so (declared in include/pgen_hip.h).
// Host-side argument checking, context/stream ownership and kernel selection; no CPU compute
// path exists here: every decode goes through a gfx950 kernel or fails with a status code.
#include "../../include/pgen_hip.h"

#include <algorithm>
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "host_pure.h"
#include "kernels.h"
#include "launch_plan.h"

using namespace pgenhip;

struct pgenhip_ctx {
    int device = 0;
    int num_cus = 256;
    uint32_t sample_count = 0;
    uint32_t record_size = 0;
    uint32_t kept_count = 0;
    bool subset = false;
    bool identity = false;             // a kept list that names every sample: AUTO takes the all-samples kernels
    uint32_t *d_kept = nullptr;
    uint8_t *d_count_mask = nullptr;   // genotype counts with a kept subset: the kept samples as a 2-bit mask (gt_count.hip)
    uint32_t *d_scount_rank = nullptr; // per-sample counts with that mask: kept samples before each 64-sample chunk (gt_scount.hip)
    uint32_t *d_seg_rank = nullptr;    // segment kernels: kept samples before each segment
    uint32_t max_seg_count = 0;        // segment kernels: most kept samples in one segment
    uint8_t *d_compact = nullptr;      // two-pass path for sparse keeps on long records: compact records of one chunk of rows,
    size_t compact_bytes = 0;          // one slice of compact_bytes per launch in flight (the slice follows the launch's counter block)
    uint32_t launch_slot = 0;          // ring slot of the launch being queued (claim_counters)
    uint64_t *d_work = nullptr;        // stream kernel: ring of PGENHIP_LAUNCHES_IN_FLIGHT counter blocks (8 work-queue heads 128 B apart + an exit counter)
    uint32_t launch_seq = 0;           // next counter block of the ring
    bool work_dirty = false;           // a launch failed: counters may be non-zero, re-zero the ring before the next launch
    Tuning tune;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr;
    hipEvent_t ev_stop = nullptr;
};

namespace {

int fail(int status, const char *what) { return pgenhip::set_detail(status, what); }

int fail_hip(hipError_t e, const char *where)
{
    pgenhip::set_detail(0, (std::string(where) + ": " + hipGetErrorString(e)).c_str());
    (void)hipGetLastError();  // clear the sticky error
    return (e == hipErrorOutOfMemory) ? PGENHIP_ERR_OOM : PGENHIP_ERR_HIP;
}

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t e__ = (expr);                           \
        if (e__ != hipSuccess) return fail_hip(e__, #expr); \
    } while (0)

int bind(const pgenhip_ctx *ctx)
{
    if (!ctx) return fail(PGENHIP_ERR_BAD_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return PGENHIP_OK;
}

// What the emit entry points run is decided in plan::emit (launch_plan.h): the shapes each kernel takes, AUTO's chains and their
// measured thresholds, the forced kernel ids, the chunks of the two passes
namespace E = plan::emit;
using E::Emit;

constexpr size_t kWorkBlockBytes = (kMaxQueueRanges + 1u) * 128u;  // the heads 128 B apart + the exit counter
constexpr size_t kWorkBlockWords = kWorkBlockBytes / sizeof(uint64_t);
// pgenhip_emit_lines: a bound on the line length (max_prefix_bytes + 4K + 1) below which every kernel can plan its tiles, batches and
// seams; larger bounds are PGENHIP_ERR_TOO_LARGE before any launch
constexpr uint64_t kMaxLineBytes = 1ull << 31;

}  // namespace

extern "C" {

int pgenhip_device_count(int *count)
{
    if (!count) return fail(PGENHIP_ERR_BAD_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail_hip(e, "hipGetDeviceCount");
    }
    *count = n;
    return PGENHIP_OK;
}

int pgenhip_create(pgenhip_ctx **out, int device_ordinal, uint32_t sample_count,
                   const uint32_t *kept_idx, uint32_t kept_count, uint32_t flags)
{
    if (!out) return fail(PGENHIP_ERR_BAD_ARG, "ctx out-pointer is NULL");
    *out = nullptr;
    if (flags & ~PGENHIP_CREATE_KEEP_LIST) return fail(PGENHIP_ERR_BAD_ARG, "unknown create flag");
    const bool subset = (flags & PGENHIP_CREATE_KEEP_LIST) != 0u || kept_idx != nullptr;
    if (subset && kept_count && !kept_idx) return fail(PGENHIP_ERR_BAD_ARG, "kept_count > 0 with a NULL kept_idx");
    if (sample_count > 0x7FFFFFFFu) return fail(PGENHIP_ERR_TOO_LARGE, "sample_count > 2^31-1");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(PGENHIP_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    }
    if (device_ordinal < 0 || device_ordinal >= n) return fail(PGENHIP_ERR_NO_DEVICE, "device ordinal out of range");
    if (subset) {
        for (uint32_t k = 0; k < kept_count; k++) {
            if (kept_idx[k] >= sample_count) return fail(PGENHIP_ERR_INDEX_RANGE, "kept_idx entry >= sample_count");
            if (k && kept_idx[k] <= kept_idx[k - 1]) return fail(PGENHIP_ERR_BAD_ARG, "kept_idx not strictly ascending");
        }
    }
    pgenhip_ctx *ctx = new (std::nothrow) pgenhip_ctx();
    if (!ctx) return fail(PGENHIP_ERR_OOM, "ctx");
    ctx->device = device_ordinal;
    ctx->sample_count = sample_count;
    ctx->record_size = pgenhip_variant_record_size(sample_count);
    ctx->subset = subset;
    ctx->identity = subset && kept_count == sample_count;  // strictly ascending and complete = 0..N-1
    ctx->kept_count = subset ? kept_count : sample_count;

    int rc = PGENHIP_OK;
    do {
        if ((e = hipSetDevice(device_ordinal)) != hipSuccess) { rc = fail_hip(e, "hipSetDevice"); break; }
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, device_ordinal)) != hipSuccess) { rc = fail_hip(e, "hipGetDeviceProperties"); break; }
        ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) { rc = fail_hip(e, "hipStreamCreate"); break; }
        ctx->stream = ctx->own_stream;
        if ((e = hipEventCreate(&ctx->ev_start)) != hipSuccess) { rc = fail_hip(e, "hipEventCreate"); break; }
        if ((e = hipEventCreate(&ctx->ev_stop)) != hipSuccess) { rc = fail_hip(e, "hipEventCreate"); break; }
        if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_work), PGENHIP_LAUNCHES_IN_FLIGHT * kWorkBlockBytes)) != hipSuccess) { rc = fail_hip(e, "hipMalloc(work counters)"); break; }
        if ((e = hipMemset(ctx->d_work, 0, PGENHIP_LAUNCHES_IN_FLIGHT * kWorkBlockBytes)) != hipSuccess) { rc = fail_hip(e, "hipMemset(work counters)"); break; }  // the kernels leave them zero
        if (ctx->subset) {
            size_t bytes = (size_t)(kept_count ? kept_count : 1u) * sizeof(uint32_t);
            if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_kept), bytes)) != hipSuccess) { rc = fail_hip(e, "hipMalloc(kept_idx)"); break; }
            if (kept_count) {
                if ((e = hipMemcpy(ctx->d_kept, kept_idx, (size_t)kept_count * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) { rc = fail_hip(e, "hipMemcpy(kept_idx)"); break; }
            }
            // kept samples before each 16 384-sample segment (what the segment kernels slice the list by)
            const uint32_t n_seg = (sample_count + kScanSegmentSamples - 1u) / kScanSegmentSamples;
            const uint32_t n_seg_eff = n_seg ? n_seg : 1u;
            std::vector<uint32_t> seg_rank((size_t)n_seg_eff + 1u, 0u);
            for (uint32_t k = 0; k < kept_count; k++) seg_rank[(size_t)(kept_idx[k] / kScanSegmentSamples) + 1u]++;
            for (uint32_t g = 0; g < n_seg_eff; g++) {
                ctx->max_seg_count = std::max(ctx->max_seg_count, seg_rank[g + 1u]);
                seg_rank[g + 1u] += seg_rank[g];
            }
            if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_seg_rank), seg_rank.size() * sizeof(uint32_t))) != hipSuccess) { rc = fail_hip(e, "hipMalloc(segment ranks)"); break; }
            if ((e = hipMemcpy(ctx->d_seg_rank, seg_rank.data(), seg_rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) { rc = fail_hip(e, "hipMemcpy(segment ranks)"); break; }
            // genotype counts: the kept list as a record-shaped mask (0b01 per kept sample) behind 16 zero bytes, so that the count kernel
            // ANDs it into the record words; an identity list counts like "all samples" and needs none
            if (!ctx->identity) {
                std::vector<uint8_t> mask(gt_count_mask_bytes(ctx->record_size), 0u);
                for (uint32_t k = 0; k < kept_count; k++) mask[16u + kept_idx[k] / 4u] |= (uint8_t)(1u << (2u * (kept_idx[k] % 4u)));
                if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_count_mask), mask.size())) != hipSuccess) { rc = fail_hip(e, "hipMalloc(count mask)"); break; }
                if ((e = hipMemcpy(ctx->d_count_mask, mask.data(), mask.size(), hipMemcpyHostToDevice)) != hipSuccess) { rc = fail_hip(e, "hipMemcpy(count mask)"); break; }
                // per-sample counts: a sample's rank = kept samples before its 64-sample chunk + the mask bits below it in the chunk
                std::vector<uint32_t> rank((size_t)(sample_count + 63u) / 64u + 1u, 0u);
                for (uint32_t k = 0; k < kept_count; k++) rank[(size_t)(kept_idx[k] / 64u) + 1u]++;
                for (size_t q = 1; q < rank.size(); q++) rank[q] += rank[q - 1u];
                if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_scount_rank), rank.size() * sizeof(uint32_t))) != hipSuccess) { rc = fail_hip(e, "hipMalloc(sample ranks)"); break; }
                if ((e = hipMemcpy(ctx->d_scount_rank, rank.data(), rank.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) { rc = fail_hip(e, "hipMemcpy(sample ranks)"); break; }
            }
            // two-pass path (sparse keeps on long records): scratch for the compact records of one chunk of rows per launch in flight
            // (config 5's per-GPU shard, 125 000 rows x 1 250 bytes, is five chunks; a chunk stays in the 256-MiB Infinity Cache
            // between the two passes); allocated here so that no launch ever allocates
            if (E::two_pass_shape(sample_count, kept_count)) {
                ctx->compact_bytes = E::kCompactSliceBytes;
                if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_compact), PGENHIP_LAUNCHES_IN_FLIGHT * ctx->compact_bytes)) != hipSuccess) { rc = fail_hip(e, "hipMalloc(compact records)"); break; }
            }
        }
    } while (0);
    if (rc != PGENHIP_OK) {
        const std::string keep = pgenhip_last_error_detail();
        pgenhip_destroy(ctx);
        pgenhip::set_detail(0, keep.c_str());
        return rc;
    }
    *out = ctx;
    return PGENHIP_OK;
}

int pgenhip_destroy(pgenhip_ctx *ctx)
{
    if (!ctx) return PGENHIP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->d_kept) (void)hipFree(ctx->d_kept);
    if (ctx->d_count_mask) (void)hipFree(ctx->d_count_mask);
    if (ctx->d_scount_rank) (void)hipFree(ctx->d_scount_rank);
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    if (ctx->d_seg_rank) (void)hipFree(ctx->d_seg_rank);
    if (ctx->d_compact) (void)hipFree(ctx->d_compact);
    if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
    if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return PGENHIP_OK;
}

int pgenhip_set_stream(pgenhip_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(PGENHIP_ERR_BAD_ARG, "ctx is NULL");
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);  // nullptr = the default (null) stream
    return PGENHIP_OK;
}

int pgenhip_reset_stream(pgenhip_ctx *ctx)
{
    if (!ctx) return fail(PGENHIP_ERR_BAD_ARG, "ctx is NULL");
    ctx->stream = ctx->own_stream;
    return PGENHIP_OK;
}

uint32_t pgenhip_sample_count(const pgenhip_ctx *ctx) { return ctx ? ctx->sample_count : 0u; }
uint32_t pgenhip_kept_count(const pgenhip_ctx *ctx) { return ctx ? ctx->kept_count : 0u; }
uint64_t pgenhip_gt_row_bytes(const pgenhip_ctx *ctx) { return ctx ? 4ull * ctx->kept_count + 1ull : 0ull; }

// The selected rows of a call (kernels.h, RowSource), checked and filled in for every entry point: by stride, by stride and
// d_variant_idx, or by d_record_off (the *_at entries; record_stride is then not used).
static int select_rows(const pgenhip_ctx *ctx, RowSource &a, const void *d_records, uint64_t record_stride,
                       const uint32_t *d_variant_idx, const uint64_t *d_record_off, uint32_t n_variants)
{
    if (n_variants && ctx->record_size && !d_records) return fail(PGENHIP_ERR_BAD_ARG, "d_records is NULL");
    if (n_variants > 1 && !d_variant_idx && !d_record_off && record_stride < ctx->record_size)
        return fail(PGENHIP_ERR_BAD_ARG, "record_stride < record size");
    a.records = static_cast<const uint8_t *>(d_records);
    a.record_stride = record_stride;
    a.variant_idx = d_variant_idx;
    a.record_off = d_record_off;
    a.n_variants = n_variants;
    a.sample_count = ctx->sample_count;
    a.record_size = ctx->record_size;
    return PGENHIP_OK;
}

// The bound on the bytes the selected records span.  A record's address is plain 64-bit pointer arithmetic in the kernels (row_record,
// gt_common.hip.h) and the bound is decode_matrix's, 2^52 bytes: by stride, all rows' records lie inside the span; with a variant
// list the row numbers live on the device (as record_off's offsets do) and only the stride itself is bounded.
static constexpr uint64_t kMaxSpan = 1ull << 52;
static bool record_span_too_large(uint64_t record_stride, const uint32_t *d_variant_idx, const uint64_t *d_record_off, uint32_t n_variants)
{
    if (n_variants <= 1 || d_record_off) return false;
    return record_stride >= (d_variant_idx ? kMaxSpan : kMaxSpan / n_variants);
}

// the *_at entries' own check, in front of their core (which reports a NULL ctx)
static int check_record_off(const pgenhip_ctx *ctx, const uint64_t *d_record_off, uint32_t n_variants)
{
    if (ctx && n_variants && !d_record_off) return fail(PGENHIP_ERR_BAD_ARG, "d_record_off is NULL");
    return PGENHIP_OK;
}

static int fill_args(pgenhip_ctx *ctx, EmitArgs &a, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                     const uint64_t *d_record_off, uint32_t n_variants, void *d_out)
{
    if (n_variants && (!d_out)) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    const int rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_idx = ctx->subset ? ctx->d_kept : nullptr;
    a.kept_count = ctx->kept_count;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_stride = 0;
    a.prefix_blob = nullptr;
    a.prefix_off = nullptr;
    a.line_off = nullptr;
    a.max_line_bytes = 0;
    a.work_counters = nullptr;
    return PGENHIP_OK;
}

// Every launch gets its own counter block from the ring, so launches of one ctx queued on different streams
// never share work-queue heads (include/pgen_hip.h, "Streams").  After a failed launch the ring is re-zeroed
// in stream order first.
static int claim_counters(pgenhip_ctx *ctx, EmitArgs &a)
{
    if (ctx->work_dirty) {
        HIP_TRY(hipMemsetAsync(ctx->d_work, 0, PGENHIP_LAUNCHES_IN_FLIGHT * kWorkBlockBytes, ctx->stream));
        ctx->work_dirty = false;
    }
    ctx->launch_slot = ctx->launch_seq++ % PGENHIP_LAUNCHES_IN_FLIGHT;
    a.work_counters = ctx->d_work + (size_t)ctx->launch_slot * kWorkBlockWords;
    return PGENHIP_OK;
}

#define LAUNCH_TRY(expr)                           \
    do {                                           \
        hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess) {                   \
            ctx->work_dirty = true;                \
            return fail_hip(e__, #expr);           \
        }                                          \
    } while (0)

// The one place a kernel id (the flags of the emit entry points) becomes what runs: AUTO by shape, a forced id where its kernel takes
// the shape.  Only AUTO treats an identity list (`--include-sam` that keeps everybody: same bytes) as all samples: forced kernels see the list.
static int choose(const pgenhip_ctx *ctx, EmitArgs &a, uint32_t kernel, Emit &out)
{
    if (kernel == PGENHIP_KERNEL_AUTO) {
        if (ctx->identity) a.kept_idx = nullptr;
        const E::Shape s = emit_shape(a);
        out = a.kept_idx == nullptr ? E::choose_all_samples(s)
                                    : E::choose_subset(s, ctx->tune.scan_rowpick != 0, ctx->tune.scan_two_pass != 0, ctx->max_seg_count, ctx->num_cus);
        return PGENHIP_OK;
    }
    const E::Shape s = emit_shape(a);
    out = E::forced(kernel, s.lines);
    if (E::accepts(kernel, s)) return PGENHIP_OK;
    const char *needs = "not a kernel id: the emit entry points take PGENHIP_KERNEL_AUTO, _ROWS, _FLAT, _SCAN, _WIDE, _PICK, _RUNS or _ROWPICK";
    switch (kernel) {   // a forced kernel's refusal
        case PGENHIP_KERNEL_FLAT: needs = "PGENHIP_KERNEL_FLAT needs GT segments, all samples kept, N >= 8 and out_stride == 4N+1"; break;
        case PGENHIP_KERNEL_SCAN: needs = "PGENHIP_KERNEL_SCAN needs a kept-sample list and N >= 61 (records of >= 16 bytes)"; break;
        case PGENHIP_KERNEL_WIDE: needs = "PGENHIP_KERNEL_WIDE needs all samples kept, N >= 1024 and (GT segments) out_stride == 4N+1"; break;
        case PGENHIP_KERNEL_PICK: needs = "PGENHIP_KERNEL_PICK needs K >= 1, 61 <= N <= 4096 and (GT segments) out_stride == 4K+1"; break;
        case PGENHIP_KERNEL_RUNS:
            needs = s.lines ? "PGENHIP_KERNEL_RUNS (lines) needs dense records, >= 8 kept samples (of <= 4096 with a keep list) and two lines per item"
                            : "PGENHIP_KERNEL_RUNS needs all samples kept, 8 <= N <= 3831, dense records and text, no variant gather";
            break;
        case PGENHIP_KERNEL_ROWPICK:   // (its launcher refuses more than 4 096 segments: PGENHIP_ERR_HIP)
            needs = "PGENHIP_KERNEL_ROWPICK needs a kept-sample list of 1 .. 16384 samples and N >= 61";
            break;
    }
    return fail(PGENHIP_ERR_BAD_ARG, needs);
}

static int run(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc, Emit choice);

// The two passes (plan::emit::two_pass), chunk by chunk of plan::emit::chunks: pointer arithmetic and launches only
static int dispatch_two_pass(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc)
{
    const uint32_t rc_bytes = (a.kept_count + 3u) / 4u;
    uint8_t *const scratch = ctx->d_compact + (size_t)ctx->launch_slot * ctx->compact_bytes;  // this launch's own slice
    const bool rowpick_on = ctx->tune.scan_rowpick != 0;
    const uint64_t round_rows = rowpick_on ? gt_rowpick_resident_waves(a, ctx->tune, ctx->num_cus, true) : 0ull;
    const E::Chunks chunks = E::chunks(emit_shape(a), ctx->compact_bytes, ctx->tune.scan_chunk_rows, rowpick_on, round_rows, ctx->num_cus);
    for (uint64_t row0 = 0; row0 < a.n_variants; row0 += chunks.rows) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunks.rows, (uint64_t)a.n_variants - row0);
        EmitArgs c = a;  // pass 1: this chunk's rows -> compact records
        if (a.record_off) c.record_off = a.record_off + row0;
        else if (a.variant_idx) c.variant_idx = a.variant_idx + row0;
        else c.records = a.records + row0 * a.record_stride;
        c.n_variants = n;
        c.out = scratch;
        c.out_stride = rc_bytes;
        c.prefix_blob = nullptr;
        c.prefix_off = nullptr;
        c.line_off = nullptr;
        if (E::chunk_by_row_owner(chunks, n))
            LAUNCH_TRY(launch_gt_rowpick(c, sc, ctx->tune, ctx->num_cus, ctx->stream, true));   // a wave per row: whole compact records, wide stores
        else
            LAUNCH_TRY(launch_gt_scan(c, sc, ctx->tune, ctx->num_cus, ctx->stream, true));
        EmitArgs d = a;  // pass 2: a block of n mode-0x02 records of K samples, all of them kept
        d.records = scratch;
        d.record_stride = rc_bytes;
        d.variant_idx = nullptr;
        d.record_off = nullptr;
        d.n_variants = n;
        d.sample_count = a.kept_count;
        d.record_size = rc_bytes;
        d.kept_idx = nullptr;
        if (a.line_off) {
            d.prefix_off = a.prefix_off + row0;  // offsets are absolute: the same blob and output base
            d.line_off = a.line_off + row0;
        } else {
            d.out = a.out + row0 * a.out_stride;
        }
        const int rc = run(ctx, d, sc, E::choose_all_samples(emit_shape(d)));
        if (rc) return rc;
    }
    return PGENHIP_OK;
}

// The only launches of the emit kernels (beside the compact passes above), each under LAUNCH_TRY: a failed launch marks the counter ring dirty
static int run(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc, Emit choice)
{
    const Tuning &t = ctx->tune;
    switch (choice) {
        case Emit::Rows: LAUNCH_TRY(launch_gt_rows(a, ctx->num_cus, ctx->stream)); break;
        case Emit::Flat: LAUNCH_TRY(launch_gt_flat(a, t, ctx->num_cus, ctx->stream)); break;
        case Emit::Wide: LAUNCH_TRY(launch_gt_wide(a, t, ctx->num_cus, ctx->stream)); break;
        case Emit::Runs: LAUNCH_TRY(launch_gt_runs(a, t, ctx->num_cus, ctx->stream)); break;
        case Emit::LineRuns: LAUNCH_TRY(launch_gt_lineruns(a, t, ctx->num_cus, ctx->stream)); break;
        case Emit::Pick: LAUNCH_TRY(launch_gt_pick(a, t, ctx->num_cus, ctx->stream)); break;
        case Emit::Scan: LAUNCH_TRY(launch_gt_scan(a, sc, t, ctx->num_cus, ctx->stream)); break;
        case Emit::RowPick: LAUNCH_TRY(launch_gt_rowpick(a, sc, t, ctx->num_cus, ctx->stream)); break;
        case Emit::TwoPass: return dispatch_two_pass(ctx, a, sc);
    }
    return PGENHIP_OK;
}

// pgenhip_emit_lines' own inputs
struct LineInputs {
    const void *prefix_blob;
    const uint64_t *prefix_off, *line_off;
    uint64_t max_prefix_bytes;
};

// The three emit entry points: GT segments at d_out + j * out_stride (lines == nullptr), or full lines at d_out + line_off[j].
// Every launch claims its counter block before the choice (a refused forced kernel has claimed one too).
static int emit_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                     const uint64_t *d_record_off, uint32_t n_variants, void *d_out, uint64_t out_stride, const LineInputs *lines, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    EmitArgs a;
    rc = fill_args(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants, d_out);
    if (rc) return rc;
    if (lines) {
        if (n_variants == 0) return PGENHIP_OK;
        if (!lines->prefix_off || !lines->line_off) return fail(PGENHIP_ERR_BAD_ARG, "offset arrays are NULL");
        if (lines->max_prefix_bytes && !lines->prefix_blob) return fail(PGENHIP_ERR_BAD_ARG, "d_prefix_blob is NULL");
        // the kernels plan tiles, batches and seams from the bound in 32 bits (gt_rows.hip: tiles per row, grid-stride over V x tiles)
        if (lines->max_prefix_bytes >= kMaxLineBytes || lines->max_prefix_bytes + 4ull * ctx->kept_count + 1ull >= kMaxLineBytes)
            return fail(PGENHIP_ERR_TOO_LARGE, "max_prefix_bytes + 4K + 1 >= 2^31");
        a.prefix_blob = static_cast<const uint8_t *>(lines->prefix_blob);
        a.prefix_off = lines->prefix_off;
        a.line_off = lines->line_off;
        a.max_line_bytes = lines->max_prefix_bytes + 4ull * ctx->kept_count + 1ull;
    } else {
        if (n_variants > 1 && out_stride < 4ull * ctx->kept_count + 1ull) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < 4K+1");
        if (flags & ~PGENHIP_KERNEL_MASK) return fail(PGENHIP_ERR_BAD_ARG, "unknown decode_emit flag");
        a.out_stride = out_stride;
        if (n_variants == 0) return PGENHIP_OK;
    }
    rc = claim_counters(ctx, a);
    if (rc) return rc;
    Emit choice;
    rc = choose(ctx, a, flags, choice);
    if (rc) return rc;
    const ScanArgs sc{ctx->d_seg_rank, ctx->max_seg_count, (uint32_t)ctx->tune.align_stores};
    return run(ctx, a, sc, choice);
}

int pgenhip_decode_emit(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride,
                        const uint32_t *d_variant_idx, uint32_t n_variants,
                        void *d_out, uint64_t out_stride, uint32_t flags)
{
    return emit_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_out, out_stride, nullptr, flags);
}

int pgenhip_decode_emit_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                           void *d_out, uint64_t out_stride, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return emit_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_out, out_stride, nullptr, flags);
}

int pgenhip_emit_lines(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride,
                       const uint32_t *d_variant_idx, uint32_t n_variants,
                       const void *d_prefix_blob, const uint64_t *d_prefix_off,
                       const uint64_t *d_line_off, uint64_t max_prefix_bytes,
                       void *d_out, uint32_t flags)
{
    const LineInputs lines{d_prefix_blob, d_prefix_off, d_line_off, max_prefix_bytes};
    return emit_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_out, 0, &lines, flags);
}

static int genotype_counts_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                                const uint64_t *d_record_off, uint32_t n_variants, uint32_t *d_counts, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags > PGENHIP_COUNT_ROWS_PER_WAVE) return fail(PGENHIP_ERR_BAD_ARG, "unknown genotype_counts flag");
    if (n_variants == 0) return PGENHIP_OK;
    if (!d_counts) return fail(PGENHIP_ERR_BAD_ARG, "d_counts is NULL");
    CountArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_count = ctx->kept_count;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.counts = d_counts;
    // AUTO: a wave per row once a row spans more chunks than 32 lanes take in three passes (N > 6 084), else several rows per wave
    const bool wave_per_row = plan::count::wave_per_row(flags == PGENHIP_COUNT_WAVE_PER_ROW, flags == PGENHIP_COUNT_ROWS_PER_WAVE, ctx->record_size);
    HIP_TRY(launch_gt_count(a, wave_per_row, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_genotype_counts(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                            uint32_t n_variants, uint32_t *d_counts, uint32_t flags)
{
    return genotype_counts_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_counts, flags);
}

int pgenhip_genotype_counts_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                               uint32_t *d_counts, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return genotype_counts_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_counts, flags);
}

static int sample_counts_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                              const uint64_t *d_record_off, uint32_t n_variants, uint32_t *d_counts, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_SCOUNT_SHAPE_MASK | PGENHIP_SCOUNT_ACCUMULATE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown sample_counts flag");
    const uint32_t shape = flags & PGENHIP_SCOUNT_SHAPE_MASK;
    if (shape != PGENHIP_SCOUNT_AUTO && shape != PGENHIP_SCOUNT_ROWS) return fail(PGENHIP_ERR_BAD_ARG, "sample_counts supports shapes AUTO and ROWS");
    const bool accumulate = (flags & PGENHIP_SCOUNT_ACCUMULATE) != 0u;
    const uint32_t K = ctx->kept_count;
    if (K == 0u) return PGENHIP_OK;   // nothing to write
    if (!d_counts) return fail(PGENHIP_ERR_BAD_ARG, "d_counts is NULL");
    if ((uintptr_t)d_counts & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_counts is not 4-byte aligned");
    ScountArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (!accumulate) HIP_TRY(hipMemsetAsync(d_counts, 0, 16ull * K, ctx->stream));   // the kernel only adds
    if (n_variants == 0) return PGENHIP_OK;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.kept_rank = ctx->d_scount_rank;
    a.counts = d_counts;
    HIP_TRY(launch_gt_scount(a, ctx->tune.scount_slices, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_sample_counts(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, uint32_t *d_counts, uint32_t flags)
{
    return sample_counts_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_counts, flags);
}

int pgenhip_sample_counts_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             uint32_t *d_counts, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return sample_counts_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_counts, flags);
}

static int sample_scores_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                              const uint64_t *d_record_off, uint32_t n_variants, const float *d_weights, uint64_t w_stride,
                              uint32_t n_columns, const float *d_miss, double *d_scores, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_SCORE_SHAPE_MASK | PGENHIP_SCORE_ACCUMULATE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown sample_scores flag");
    const uint32_t shape = flags & PGENHIP_SCORE_SHAPE_MASK;
    if (shape != PGENHIP_SCORE_AUTO && shape != PGENHIP_SCORE_ROWS) return fail(PGENHIP_ERR_BAD_ARG, "sample_scores supports shapes AUTO and ROWS");
    const bool accumulate = (flags & PGENHIP_SCORE_ACCUMULATE) != 0u;
    if (n_columns == 0u || n_columns > PGENHIP_SCORE_MAX_COLUMNS) return fail(PGENHIP_ERR_BAD_ARG, "n_columns must be 1 .. PGENHIP_SCORE_MAX_COLUMNS");
    if (n_variants > 1 && w_stride < n_columns) return fail(PGENHIP_ERR_BAD_ARG, "w_stride < n_columns");
    if (n_variants && !d_weights) return fail(PGENHIP_ERR_BAD_ARG, "d_weights is NULL");
    if ((uintptr_t)d_weights & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_weights is not 4-byte aligned");
    if ((uintptr_t)d_miss & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_miss is not 4-byte aligned");
    const uint32_t K = ctx->kept_count;
    if (K != 0u && !d_scores) return fail(PGENHIP_ERR_BAD_ARG, "d_scores is NULL");
    if (K != 0u && ((uintptr_t)d_scores & 7u)) return fail(PGENHIP_ERR_BAD_ARG, "d_scores is not 8-byte aligned");
    // byte offsets are 64-bit arithmetic in the kernel; the bound is decode_matrix's (2^52 bytes)
    if ((n_variants > 1 && w_stride >= kMaxSpan / 4u / n_variants) || record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "score offsets do not fit the kernel's index types");
    if (K == 0u) return PGENHIP_OK;   // nothing to write
    ScoreArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (!accumulate) HIP_TRY(hipMemsetAsync(d_scores, 0, sizeof(double) * K * n_columns, ctx->stream));   // the kernel only adds
    if (n_variants == 0) return PGENHIP_OK;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.kept_rank = ctx->d_scount_rank;
    a.weights = d_weights;
    a.w_stride = w_stride;
    a.n_columns = n_columns;
    a.miss = d_miss;
    a.scores = d_scores;
    HIP_TRY(launch_gt_score(a, ctx->tune.score_slices, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_sample_scores(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, const float *d_weights, uint64_t w_stride, uint32_t n_columns,
                          const float *d_miss, double *d_scores, uint32_t flags)
{
    return sample_scores_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_weights, w_stride, n_columns, d_miss, d_scores, flags);
}

int pgenhip_sample_scores_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             const float *d_weights, uint64_t w_stride, uint32_t n_columns,
                             const float *d_miss, double *d_scores, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return sample_scores_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_weights, w_stride, n_columns, d_miss, d_scores, flags);
}

static int variant_sums_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                             const uint64_t *d_record_off, uint32_t n_variants, const double *d_values, uint64_t v_stride,
                             uint32_t n_columns, double *d_sums, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~PGENHIP_VSUM_SHAPE_MASK) return fail(PGENHIP_ERR_BAD_ARG, "unknown variant_sums flag");
    const uint32_t shape = flags & PGENHIP_VSUM_SHAPE_MASK;
    if (shape > PGENHIP_VSUM_MFMA) return fail(PGENHIP_ERR_BAD_ARG, "variant_sums supports shapes AUTO, GENERAL and MFMA");
    if (n_columns == 0u || n_columns > PGENHIP_VSUM_MAX_COLUMNS) return fail(PGENHIP_ERR_BAD_ARG, "n_columns must be 1 .. PGENHIP_VSUM_MAX_COLUMNS");
    const uint32_t K = ctx->kept_count;
    if (K > 1u && v_stride < n_columns) return fail(PGENHIP_ERR_BAD_ARG, "v_stride < n_columns");
    if (K != 0u && n_variants && !d_values) return fail(PGENHIP_ERR_BAD_ARG, "d_values is NULL");
    if ((uintptr_t)d_values & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_values is not 8-byte aligned");
    if (n_variants && !d_sums) return fail(PGENHIP_ERR_BAD_ARG, "d_sums is NULL");
    if ((uintptr_t)d_sums & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_sums is not 8-byte aligned");
    if (shape == PGENHIP_VSUM_MFMA && K == 0u) return fail(PGENHIP_ERR_BAD_ARG, "the MFMA shape needs at least one kept sample");
    // byte offsets are 64-bit arithmetic in the kernel; the bound is decode_matrix's (2^52 bytes)
    if ((K > 1u && v_stride >= kMaxSpan / 8u / K) || (uint64_t)n_variants * n_columns >= kMaxSpan / 32u ||
        record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "variant_sums offsets do not fit the kernel's index types");
    if (n_variants == 0) return PGENHIP_OK;
    VsumArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.kept_rank = ctx->d_scount_rank;
    a.values = d_values;
    a.v_stride = v_stride;
    a.n_columns = n_columns;
    a.sums = d_sums;
    const size_t out_bytes = sizeof(double) * 4u * n_columns * (size_t)n_variants;
    if (K == 0u) {   // no sample: zeros
        HIP_TRY(hipMemsetAsync(d_sums, 0, out_bytes, ctx->stream));
        return PGENHIP_OK;
    }
    if (shape == PGENHIP_VSUM_GENERAL) {
        HIP_TRY(launch_gt_vsum_general(a, ctx->tune.vsum_blocks, ctx->num_cus, ctx->stream));
    } else {   // AUTO: the matrix-core shape wherever it applies (K >= 1)
        if (plan::vsum::mfma_atomic(a.record_size)) HIP_TRY(hipMemsetAsync(d_sums, 0, out_bytes, ctx->stream));   // tiles of a row meet in atomics: the kernel only adds
        HIP_TRY(launch_gt_vsum_mfma(a, ctx->tune.vsum_blocks, ctx->num_cus, ctx->stream));
    }
    return PGENHIP_OK;
}

int pgenhip_variant_sums(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                         uint32_t n_variants, const double *d_values, uint64_t v_stride, uint32_t n_columns, double *d_sums,
                         uint32_t flags)
{
    return variant_sums_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_values, v_stride, n_columns, d_sums, flags);
}

int pgenhip_variant_sums_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                            const double *d_values, uint64_t v_stride, uint32_t n_columns, double *d_sums, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return variant_sums_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_values, v_stride, n_columns, d_sums, flags);
}

static int variant_logistic_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                                 const uint64_t *d_record_off, uint32_t n_variants, const double *d_code_values, const double *d_design,
                                 uint64_t x_stride, uint32_t n_cov, const double *d_y, const double *d_start, uint32_t max_iter, double tol,
                                 double *d_coef, uint64_t c_stride, double *d_se, uint32_t *d_status, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~PGENHIP_LOGIT_SHAPE_MASK) return fail(PGENHIP_ERR_BAD_ARG, "unknown variant_logistic flag");
    const uint32_t shape = flags & PGENHIP_LOGIT_SHAPE_MASK;
    if (shape > PGENHIP_LOGIT_FAST) return fail(PGENHIP_ERR_BAD_ARG, "variant_logistic supports shapes AUTO, GENERAL and FAST");
    if (n_cov == 0u || n_cov > PGENHIP_LOGIT_MAX_COVARIATES) return fail(PGENHIP_ERR_BAD_ARG, "n_cov must be 1 .. PGENHIP_LOGIT_MAX_COVARIATES");
    if (max_iter == 0u || max_iter > PGENHIP_LOGIT_MAX_ITER) return fail(PGENHIP_ERR_BAD_ARG, "max_iter must be 1 .. PGENHIP_LOGIT_MAX_ITER");
    if (!(tol >= 0.0)) return fail(PGENHIP_ERR_BAD_ARG, "tol is NaN or negative");
    const uint32_t K = ctx->kept_count;
    if (K > 1u && x_stride < n_cov) return fail(PGENHIP_ERR_BAD_ARG, "x_stride < n_cov");
    if (n_variants > 1u && c_stride < n_cov + 1u) return fail(PGENHIP_ERR_BAD_ARG, "c_stride < n_cov + 1");
    if (n_variants && (!d_code_values || !d_start || !d_coef || !d_se || !d_status))
        return fail(PGENHIP_ERR_BAD_ARG, "d_code_values, d_start, d_coef, d_se or d_status is NULL");
    if (n_variants && K != 0u && (!d_design || !d_y)) return fail(PGENHIP_ERR_BAD_ARG, "d_design or d_y is NULL");
    if (((uintptr_t)d_code_values | (uintptr_t)d_design | (uintptr_t)d_y | (uintptr_t)d_start | (uintptr_t)d_coef | (uintptr_t)d_se) & 7u)
        return fail(PGENHIP_ERR_BAD_ARG, "d_code_values, d_design, d_y, d_start, d_coef or d_se is not 8-byte aligned");
    if ((uintptr_t)d_status & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_status is not 4-byte aligned");
    // byte offsets are 64-bit arithmetic in the kernel; the bound is decode_matrix's (2^52 bytes)
    if ((K > 1u && x_stride >= kMaxSpan / 8u / K) || (n_variants > 1u && c_stride >= kMaxSpan / 8u / n_variants) ||
        record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "variant_logistic offsets do not fit the kernel's index types");
    if (n_variants == 0) return PGENHIP_OK;
    LogitArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (K == 0u) a.sample_count = 0u;   // no sample is included: every row ends SINGULAR at its first evaluation, nothing per sample is read
    a.kept_mask = ctx->d_count_mask;    // NULL with all samples kept or an identity list
    a.kept_rank = ctx->d_scount_rank;
    a.code_values = d_code_values;
    a.design = d_design;
    a.x_stride = x_stride;
    a.n_cov = n_cov;
    a.y = d_y;
    a.start = d_start;
    a.max_iter = max_iter;
    a.tol = tol;
    a.coef = d_coef;
    a.c_stride = c_stride;
    a.se = d_se;
    a.status = d_status;
    if (shape == PGENHIP_LOGIT_GENERAL) HIP_TRY(launch_gt_logit_general(a, ctx->tune.logit_blocks, ctx->num_cus, ctx->stream));
    else HIP_TRY(launch_gt_logit_fast(a, ctx->tune.logit_blocks, ctx->num_cus, ctx->stream));   // AUTO: FAST applies to every shape
    return PGENHIP_OK;
}

int pgenhip_variant_logistic(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                             uint32_t n_variants, const double *d_code_values, const double *d_design, uint64_t x_stride,
                             uint32_t n_cov, const double *d_y, const double *d_start, uint32_t max_iter, double tol,
                             double *d_coef, uint64_t c_stride, double *d_se, uint32_t *d_status, uint32_t flags)
{
    return variant_logistic_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_code_values, d_design, x_stride, n_cov,
                                 d_y, d_start, max_iter, tol, d_coef, c_stride, d_se, d_status, flags);
}

int pgenhip_variant_logistic_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                                const double *d_code_values, const double *d_design, uint64_t x_stride, uint32_t n_cov,
                                const double *d_y, const double *d_start, uint32_t max_iter, double tol, double *d_coef,
                                uint64_t c_stride, double *d_se, uint32_t *d_status, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return variant_logistic_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_code_values, d_design, x_stride, n_cov, d_y, d_start,
                                 max_iter, tol, d_coef, c_stride, d_se, d_status, flags);
}

static int decode_matrix_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                              const uint64_t *d_record_off, uint32_t n_variants, void *d_out, uint64_t out_stride, uint32_t elem_bytes,
                              const void *code_values, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_MATRIX_SHAPE_MASK | PGENHIP_MATRIX_SAMPLE_MAJOR)) return fail(PGENHIP_ERR_BAD_ARG, "unknown decode_matrix flag");
    const uint32_t shape = flags & PGENHIP_MATRIX_SHAPE_MASK;
    if (shape > PGENHIP_MATRIX_TILE) return fail(PGENHIP_ERR_BAD_ARG, "decode_matrix supports shapes AUTO, GENERAL, STREAM and TILE");
    if (elem_bytes != 1u && elem_bytes != 2u && elem_bytes != 4u) return fail(PGENHIP_ERR_BAD_ARG, "elem_bytes must be 1, 2 or 4");
    const bool sample_major = (flags & PGENHIP_MATRIX_SAMPLE_MAJOR) != 0u;
    const uint32_t K = ctx->kept_count;
    const bool all_kept = !ctx->subset || ctx->identity;
    if (shape == PGENHIP_MATRIX_STREAM && (!all_kept || sample_major))
        return fail(PGENHIP_ERR_BAD_ARG, "PGENHIP_MATRIX_STREAM needs all samples kept and the variant-major orientation");
    if (shape == PGENHIP_MATRIX_TILE && (!all_kept || !sample_major))
        return fail(PGENHIP_ERR_BAD_ARG, "PGENHIP_MATRIX_TILE needs all samples kept and the sample-major orientation");
    if (n_variants == 0 || K == 0u) return PGENHIP_OK;   // nothing to write
    if (!d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    if ((uintptr_t)d_out % elem_bytes || out_stride % elem_bytes) return fail(PGENHIP_ERR_BAD_ARG, "d_out and out_stride must be multiples of elem_bytes");
    MatrixArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    const uint64_t rows = sample_major ? K : n_variants, inner = sample_major ? n_variants : K;
    if (rows > 1 && out_stride < inner * elem_bytes) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < one output row");
    // the kernels index elements and 16-byte chunks in 64 bits and divide through a double reciprocal: exact below 2^52
    if ((uint64_t)n_variants * K >= kMaxSpan / 16u || (rows > 1 && out_stride >= kMaxSpan / rows) ||
        record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "matrix offsets do not fit the kernels' index types");
    a.kept_idx = all_kept ? nullptr : ctx->d_kept;
    a.kept_count = K;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_stride = out_stride;
    a.elem_bytes = elem_bytes;
    a.sample_major = sample_major ? 1u : 0u;
    const uint32_t all_ones = elem_bytes == 4u ? 0xFFFFFFFFu : (1u << (8u * elem_bytes)) - 1u;
    for (uint32_t c = 0; c < 4u; c++) {
        uint32_t v = c == 3u ? all_ones : c;
        if (code_values) {
            const uint8_t *p = static_cast<const uint8_t *>(code_values) + (size_t)c * elem_bytes;
            v = 0u;
            for (uint32_t b = 0; b < elem_bytes; b++) v |= (uint32_t)p[b] << (8u * b);
        }
        a.tab[c] = v;
    }
    // (the kernels' notion of "all samples kept": no list, K == N)
    const bool no_list = a.kept_idx == nullptr && a.kept_count == a.sample_count;
    const uint32_t out_align = (uint32_t)((uintptr_t)a.out & 15u);
    if (shape == PGENHIP_MATRIX_TILE && !plan::matrix::tile_applicable(no_list, sample_major, out_align, out_stride, K))
        return fail(PGENHIP_ERR_BAD_ARG, "PGENHIP_MATRIX_TILE needs d_out and out_stride to be multiples of 16 bytes");
    const int blocks = ctx->tune.matrix_blocks;
    static_assert(plan::matrix::kGeneral == PGENHIP_MATRIX_GENERAL && plan::matrix::kStream == PGENHIP_MATRIX_STREAM && plan::matrix::kTile == PGENHIP_MATRIX_TILE,
                  "plan::matrix::Shape carries the ABI's values");
    const uint32_t run = shape != PGENHIP_MATRIX_AUTO ? shape : plan::matrix::auto_shape(no_list, sample_major, out_align, out_stride, K);
    if (run == PGENHIP_MATRIX_STREAM)
        HIP_TRY(launch_gt_matrix_stream(a, blocks, ctx->num_cus, ctx->stream));
    else if (run == PGENHIP_MATRIX_TILE)
        HIP_TRY(launch_gt_matrix_tile(a, blocks, ctx->num_cus, ctx->stream));
    else
        HIP_TRY(launch_gt_matrix_general(a, blocks, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_decode_matrix(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, void *d_out, uint64_t out_stride, uint32_t elem_bytes,
                          const void *code_values, uint32_t flags)
{
    return decode_matrix_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_out, out_stride, elem_bytes, code_values, flags);
}

int pgenhip_decode_matrix_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             void *d_out, uint64_t out_stride, uint32_t elem_bytes, const void *code_values, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return decode_matrix_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_out, out_stride, elem_bytes, code_values, flags);
}

static int pair_stats_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                           const uint64_t *d_record_off, uint32_t n_variants, uint32_t n_left, uint32_t window, void *d_out, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags > PGENHIP_PAIR_R2) return fail(PGENHIP_ERR_BAD_ARG, "unknown pair_stats flag");
    if (window == 0u) return fail(PGENHIP_ERR_BAD_ARG, "window is 0");
    if (n_left > n_variants) return fail(PGENHIP_ERR_BAD_ARG, "n_left > n_variants");
    if (n_left == 0u || n_variants <= 1u) return PGENHIP_OK;   // no pair exists
    if (!d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    const bool r2 = flags == PGENHIP_PAIR_R2;
    if ((uintptr_t)d_out & (r2 ? 3u : 15u))
        return fail(PGENHIP_ERR_BAD_ARG, r2 ? "d_out is not 4-byte aligned" : "d_out is not 16-byte aligned (PGENHIP_PAIR_TABLE)");
    // the kernel forms byte offsets of pair entries in 64 bits; the bound is the other kernels' (2^52 bytes), taken on the
    // table entry's 64 bytes whichever the mode
    if ((uint64_t)n_left * window >= (1ull << 52) / 64u) return fail(PGENHIP_ERR_TOO_LARGE, "n_left * window * 64 >= 2^52");
    PairArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_count = ctx->kept_count;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.n_left = n_left;
    a.window = window;
    a.out = d_out;
    a.r2 = r2 ? 1u : 0u;
    HIP_TRY(launch_gt_pair(a, ctx->tune.pair_blocks, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_pair_stats(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                       uint32_t n_variants, uint32_t n_left, uint32_t window, void *d_out, uint32_t flags)
{
    return pair_stats_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, n_left, window, d_out, flags);
}

int pgenhip_pair_stats_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                          uint32_t n_left, uint32_t window, void *d_out, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return pair_stats_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, n_left, window, d_out, flags);
}

static int pair_mask_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          const uint64_t *d_record_off, uint32_t n_variants, uint32_t n_left, uint32_t window, float min_r2,
                          const uint64_t *d_key, uint64_t max_span, uint32_t *d_fwd, uint32_t *d_bwd, uint64_t mask_stride, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags != 0u) return fail(PGENHIP_ERR_BAD_ARG, "unknown pair_mask flag");
    if (window == 0u) return fail(PGENHIP_ERR_BAD_ARG, "window is 0");
    if (n_left > n_variants) return fail(PGENHIP_ERR_BAD_ARG, "n_left > n_variants");
    if (min_r2 != min_r2) return fail(PGENHIP_ERR_BAD_ARG, "min_r2 is NaN");
    if ((uintptr_t)d_key & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_key is not 8-byte aligned");
    if (n_left == 0u || n_variants <= 1u) return PGENHIP_OK;   // no pair exists
    if (!d_fwd) return fail(PGENHIP_ERR_BAD_ARG, "d_fwd is NULL");
    if (((uintptr_t)d_fwd | (uintptr_t)d_bwd) & 3u) return fail(PGENHIP_ERR_BAD_ARG, "a mask is not 4-byte aligned");
    // rows the masks address: the left rows of d_fwd, every row of d_bwd
    if ((d_bwd ? n_variants : n_left) > 1u && mask_stride < plan::prune::mask_words(window))
        return fail(PGENHIP_ERR_BAD_ARG, "mask_stride < ceil(window / 32)");
    // a mask word's byte offset is 64-bit arithmetic in the kernel; the bound is the other kernels' (2^52 bytes)
    if (mask_stride >= kMaxSpan / 4u / n_variants) return fail(PGENHIP_ERR_TOO_LARGE, "n_variants * mask_stride * 4 >= 2^52");
    PairMaskArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_count = ctx->kept_count;
    a.kept_mask = ctx->d_count_mask;   // NULL with all samples kept or an identity list
    a.n_left = n_left;
    a.window = window;
    a.out = nullptr;
    a.r2 = 1u;
    a.min_r2 = min_r2;
    a.key = d_key;
    a.max_span = max_span;
    a.fwd = d_fwd;
    a.bwd = d_bwd;
    a.mask_stride = mask_stride;
    HIP_TRY(launch_gt_pair_mask(a, ctx->tune.pair_blocks, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_pair_mask(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                      uint32_t n_variants, uint32_t n_left, uint32_t window, float min_r2, const uint64_t *d_key, uint64_t max_span,
                      uint32_t *d_fwd, uint32_t *d_bwd, uint64_t mask_stride, uint32_t flags)
{
    return pair_mask_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, n_left, window, min_r2, d_key, max_span, d_fwd,
                          d_bwd, mask_stride, flags);
}

int pgenhip_pair_mask_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants, uint32_t n_left,
                         uint32_t window, float min_r2, const uint64_t *d_key, uint64_t max_span, uint32_t *d_fwd, uint32_t *d_bwd,
                         uint64_t mask_stride, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return pair_mask_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, n_left, window, min_r2, d_key, max_span, d_fwd, d_bwd,
                          mask_stride, flags);
}

int pgenhip_prune_resolve(pgenhip_ctx *ctx, const uint32_t *d_fwd, const uint32_t *d_bwd, uint64_t mask_stride, uint32_t window,
                          uint64_t n_rows, const uint32_t *d_priority, uint8_t *d_state, uint64_t *d_undecided, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags > PGENHIP_PRUNE_BLOCK) return fail(PGENHIP_ERR_BAD_ARG, "prune_resolve supports shapes AUTO, GENERAL and BLOCK");
    if (window == 0u) return fail(PGENHIP_ERR_BAD_ARG, "window is 0");
    if (n_rows != 0u && (!d_fwd || !d_bwd || !d_state)) return fail(PGENHIP_ERR_BAD_ARG, "d_fwd, d_bwd or d_state is NULL");
    if (n_rows != 0u && !d_undecided) return fail(PGENHIP_ERR_BAD_ARG, "d_undecided is NULL");
    if (((uintptr_t)d_fwd | (uintptr_t)d_bwd) & 3u) return fail(PGENHIP_ERR_BAD_ARG, "a mask is not 4-byte aligned");
    if ((uintptr_t)d_priority & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_priority is not 4-byte aligned");
    if ((uintptr_t)d_undecided & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_undecided is not 8-byte aligned");
    if (n_rows > 1u && mask_stride < plan::prune::mask_words(window)) return fail(PGENHIP_ERR_BAD_ARG, "mask_stride < ceil(window / 32)");
    if (n_rows > 1u && (n_rows >= kMaxSpan / 4u || mask_stride >= kMaxSpan / 4u / n_rows))
        return fail(PGENHIP_ERR_TOO_LARGE, "n_rows * mask_stride * 4 >= 2^52");
    if (d_undecided) HIP_TRY(hipMemsetAsync(d_undecided, 0, sizeof(uint64_t), ctx->stream));   // the kernels add the rows they leave undecided
    if (n_rows == 0u) return PGENHIP_OK;
    PruneArgs a;
    a.fwd = d_fwd;
    a.bwd = d_bwd;
    a.mask_stride = n_rows > 1u ? mask_stride : 0u;   // (one row: its words are at the masks' start whatever the stride)
    a.window = (uint32_t)std::min<uint64_t>(window, n_rows - 1u);   // no farther neighbour is a row: its bit is never read
    a.n_rows = n_rows;
    a.priority = d_priority;
    a.state = d_state;
    a.undecided = reinterpret_cast<unsigned long long *>(d_undecided);
    static_assert(PGENHIP_PRUNE_UNDECIDED == 0u && PGENHIP_PRUNE_KEPT == 1u && PGENHIP_PRUNE_REMOVED == 2u, "gt_prune.hip's state bytes");
    const bool block = flags == PGENHIP_PRUNE_BLOCK || (flags == PGENHIP_PRUNE_AUTO && plan::prune::auto_block(n_rows, window));
    if (block)
        HIP_TRY(launch_gt_prune_block(a, ctx->tune.prune_blocks, ctx->num_cus, ctx->stream));
    else
        HIP_TRY(launch_gt_prune_general(a, ctx->tune.prune_blocks, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

static int sample_pair_stats_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                                  const uint64_t *d_record_off, uint32_t n_variants, uint32_t a_begin, uint32_t a_count,
                                  uint32_t b_begin, uint32_t b_count, uint32_t *d_out, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_SPAIR_SHAPE_MASK | PGENHIP_SPAIR_ACCUMULATE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown sample_pair_stats flag");
    const uint32_t shape = flags & PGENHIP_SPAIR_SHAPE_MASK;
    if (shape > PGENHIP_SPAIR_MFMA) return fail(PGENHIP_ERR_BAD_ARG, "sample_pair_stats supports shapes AUTO, GENERAL and MFMA");
    const bool accumulate = (flags & PGENHIP_SPAIR_ACCUMULATE) != 0u;
    const uint64_t K = ctx->kept_count;
    if ((uint64_t)a_begin + a_count > K || (uint64_t)b_begin + b_count > K) return fail(PGENHIP_ERR_BAD_ARG, "a sample range ends past the kept count");
    const uint64_t pairs = (uint64_t)a_count * b_count;
    if (pairs != 0u && !d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    if (pairs != 0u && ((uintptr_t)d_out & 15u)) return fail(PGENHIP_ERR_BAD_ARG, "d_out is not 16-byte aligned");
    // byte offsets of table entries and records are 64-bit arithmetic in the kernels; the bounds are decode_matrix's (2^52 bytes)
    if (pairs >= kMaxSpan / 64u || record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "sample_pair_stats offsets do not fit the kernels' index types");
    if (pairs == 0u) return PGENHIP_OK;   // nothing to write
    SpairArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (!accumulate) HIP_TRY(hipMemsetAsync(d_out, 0, 64u * pairs, ctx->stream));   // the kernels only add
    if (n_variants == 0) return PGENHIP_OK;
    a.kept_idx = (!ctx->subset || ctx->identity) ? nullptr : ctx->d_kept;
    a.a_begin = a_begin;
    a.a_count = a_count;
    a.b_begin = b_begin;
    a.b_count = b_count;
    a.out = d_out;
    // AUTO: the matrix-core shape.  It measured 2.8-49 x ahead of GENERAL on every shape of tools/spair_bench.py (DESIGN.md §15,
    // profiles/r10_spair); ranges of a few pairs, where a 64 x 64 tile is mostly padding, were not measured
    const bool mfma = shape != PGENHIP_SPAIR_GENERAL;
    if (mfma)
        HIP_TRY(launch_gt_spair_mfma(a, ctx->tune.spair_slices, ctx->num_cus, ctx->stream));
    else
        HIP_TRY(launch_gt_spair_general(a, ctx->tune.spair_slices, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_sample_pair_stats(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                              uint32_t n_variants, uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count,
                              uint32_t *d_out, uint32_t flags)
{
    return sample_pair_stats_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, a_begin, a_count, b_begin, b_count, d_out, flags);
}

int pgenhip_sample_pair_stats_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                                 uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count, uint32_t *d_out, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return sample_pair_stats_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, a_begin, a_count, b_begin, b_count, d_out, flags);
}

static int sample_gram_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                            const uint64_t *d_record_off, uint32_t n_variants, const double *d_code_values, uint32_t a_begin,
                            uint32_t a_count, uint32_t b_begin, uint32_t b_count, double *d_out, uint64_t out_stride, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_GRAM_SHAPE_MASK | PGENHIP_GRAM_ACCUMULATE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown sample_gram flag");
    const uint32_t shape = flags & PGENHIP_GRAM_SHAPE_MASK;
    if (shape > PGENHIP_GRAM_MFMA) return fail(PGENHIP_ERR_BAD_ARG, "sample_gram supports shapes AUTO, GENERAL and MFMA");
    const bool accumulate = (flags & PGENHIP_GRAM_ACCUMULATE) != 0u;
    const uint64_t K = ctx->kept_count;
    if ((uint64_t)a_begin + a_count > K || (uint64_t)b_begin + b_count > K) return fail(PGENHIP_ERR_BAD_ARG, "a sample range ends past the kept count");
    if (n_variants && !d_code_values) return fail(PGENHIP_ERR_BAD_ARG, "d_code_values is NULL");
    if ((uintptr_t)d_code_values & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_code_values is not 8-byte aligned");
    const uint64_t pairs = (uint64_t)a_count * b_count;
    if (pairs != 0u && !d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    if (pairs != 0u && ((uintptr_t)d_out & 7u)) return fail(PGENHIP_ERR_BAD_ARG, "d_out is not 8-byte aligned");
    if (a_count > 1u && out_stride < b_count) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < b_count");
    // byte offsets of entries, tables and records are 64-bit arithmetic in the kernels; the bounds are decode_matrix's (2^52 bytes)
    if ((a_count > 1u && out_stride >= kMaxSpan / 8u / a_count) || (uint64_t)n_variants * 32u >= kMaxSpan ||
        record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "sample_gram offsets do not fit the kernels' index types");
    if (pairs == 0u) return PGENHIP_OK;   // nothing to write
    GramArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    a.kept_idx = (!ctx->subset || ctx->identity) ? nullptr : ctx->d_kept;
    a.a_begin = a_begin;
    a.a_count = a_count;
    a.b_begin = b_begin;
    a.b_count = b_count;
    a.code_values = d_code_values;
    a.out = d_out;
    a.out_stride = a_count > 1u ? out_stride : b_count;
    // AUTO: the matrix-core shape
    const bool mfma = shape != PGENHIP_GRAM_GENERAL;
    const uint32_t slices = n_variants == 0u ? 1u   // (nothing is launched)
                            : mfma ? plan::gram::mfma_slices(n_variants, a_count, b_count, ctx->tune.gram_slices, ctx->num_cus)
                                   : plan::gram::general_slices(n_variants, a_count, b_count, ctx->tune.gram_slices, ctx->num_cus);
    // one slice that overwrites: every entry has one owner and is stored.  Else the kernels only add, to zeros or to what is there
    a.store = (!accumulate && n_variants != 0u && slices == 1u) ? 1u : 0u;
    if (!accumulate && !a.store)
        HIP_TRY(hipMemset2DAsync(d_out, 8u * (size_t)a.out_stride, 0, 8u * (size_t)b_count, a_count, ctx->stream));
    if (n_variants == 0) return PGENHIP_OK;
    if (mfma)
        HIP_TRY(launch_gt_gram_mfma(a, slices, ctx->stream));
    else
        HIP_TRY(launch_gt_gram_general(a, slices, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_sample_gram(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                        uint32_t n_variants, const double *d_code_values, uint32_t a_begin, uint32_t a_count, uint32_t b_begin,
                        uint32_t b_count, double *d_out, uint64_t out_stride, uint32_t flags)
{
    return sample_gram_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_code_values, a_begin, a_count, b_begin,
                            b_count, d_out, out_stride, flags);
}

int pgenhip_sample_gram_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                           const double *d_code_values, uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count,
                           double *d_out, uint64_t out_stride, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return sample_gram_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_code_values, a_begin, a_count, b_begin, b_count, d_out,
                            out_stride, flags);
}

static int gram_apply_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                           const uint64_t *d_record_off, uint32_t n_variants, const double *d_code_values, const double *d_q,
                           uint64_t q_stride, uint32_t n_columns, double *d_proj, double *d_out, uint64_t out_stride, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags & ~(PGENHIP_GAPPLY_SHAPE_MASK | PGENHIP_GAPPLY_ACCUMULATE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown gram_apply flag");
    const uint32_t shape = flags & PGENHIP_GAPPLY_SHAPE_MASK;
    if (shape > PGENHIP_GAPPLY_MFMA) return fail(PGENHIP_ERR_BAD_ARG, "gram_apply supports shapes AUTO, GENERAL and MFMA");
    const bool accumulate = (flags & PGENHIP_GAPPLY_ACCUMULATE) != 0u;
    if (n_columns == 0u || n_columns > PGENHIP_GAPPLY_MAX_COLUMNS) return fail(PGENHIP_ERR_BAD_ARG, "n_columns must be 1 .. 16");
    const uint64_t K = ctx->kept_count, C = n_columns;
    if (K > 1u && q_stride < C) return fail(PGENHIP_ERR_BAD_ARG, "q_stride < n_columns");
    if (K > 1u && out_stride < C) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < n_columns");
    // what is read or written: tables and q with rows and samples, proj with rows, out with samples
    const bool rows = n_variants != 0u, samples = K != 0u;
    if (rows && samples && (!d_code_values || ((uintptr_t)d_code_values & 7u))) return fail(PGENHIP_ERR_BAD_ARG, "d_code_values is NULL or not 8-byte aligned");
    if (rows && samples && (!d_q || ((uintptr_t)d_q & 7u))) return fail(PGENHIP_ERR_BAD_ARG, "d_q is NULL or not 8-byte aligned");
    if (rows && (!d_proj || ((uintptr_t)d_proj & 7u))) return fail(PGENHIP_ERR_BAD_ARG, "d_proj is NULL or not 8-byte aligned");
    if (samples && !(accumulate && !rows) && (!d_out || ((uintptr_t)d_out & 7u))) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL or not 8-byte aligned");
    // byte offsets of entries, tables and records are 64-bit arithmetic in the kernels; the bounds are decode_matrix's (2^52 bytes)
    if ((K > 1u && (q_stride >= kMaxSpan / 8u / K || out_stride >= kMaxSpan / 8u / K)) || (uint64_t)n_variants * C * 8u >= kMaxSpan ||
        record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "gram_apply offsets do not fit the kernels' index types");
    GapplyArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (!samples) {   // no sample: every projection is an empty sum, and there is no Y
        if (rows) HIP_TRY(hipMemsetAsync(d_proj, 0, 8u * (size_t)n_variants * C, ctx->stream));
        return PGENHIP_OK;
    }
    a.kept_idx = (!ctx->subset || ctx->identity) ? nullptr : ctx->d_kept;
    a.kept_count = (uint32_t)K;
    a.code_values = d_code_values;
    a.q = d_q;
    a.q_stride = K > 1u ? q_stride : C;
    a.n_columns = n_columns;
    a.proj = d_proj;
    a.out = d_out;
    a.out_stride = K > 1u ? out_stride : C;
    // AUTO: the matrix-core shape
    const bool mfma = shape != PGENHIP_GAPPLY_GENERAL;
    if (!rows) {
        if (!accumulate) HIP_TRY(hipMemset2DAsync(d_out, 8u * (size_t)a.out_stride, 0, 8u * (size_t)C, K, ctx->stream));
        return PGENHIP_OK;
    }
    const plan::gapply::Plan p = plan::gapply::plan(n_variants, (uint32_t)K, n_columns, mfma, ctx->tune.gapply_sample_slices, ctx->tune.gapply_row_slices, ctx->num_cus);
    // a pass with one slice that overwrites: every entry has one owner and is stored.  Else the kernels only add, to zeros or to what is there
    a.p_store = p.sample_slices == 1u ? 1u : 0u;
    a.y_store = (!accumulate && p.row_slices == 1u) ? 1u : 0u;
    if (!a.p_store) HIP_TRY(hipMemsetAsync(d_proj, 0, 8u * (size_t)n_variants * C, ctx->stream));
    if (!accumulate && !a.y_store) HIP_TRY(hipMemset2DAsync(d_out, 8u * (size_t)a.out_stride, 0, 8u * (size_t)C, K, ctx->stream));
    HIP_TRY(launch_gt_gapply_p(a, mfma, p.p_tiles, p.p_grid, p.sample_slices, ctx->stream));
    HIP_TRY(launch_gt_gapply_y(a, mfma, p.y_tiles, p.y_grid, p.row_slices, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_gram_apply(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                       uint32_t n_variants, const double *d_code_values, const double *d_q, uint64_t q_stride,
                       uint32_t n_columns, double *d_proj, double *d_out, uint64_t out_stride, uint32_t flags)
{
    return gram_apply_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_code_values, d_q, q_stride, n_columns,
                           d_proj, d_out, out_stride, flags);
}

int pgenhip_gram_apply_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                          const double *d_code_values, const double *d_q, uint64_t q_stride, uint32_t n_columns,
                          double *d_proj, double *d_out, uint64_t out_stride, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return gram_apply_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_code_values, d_q, q_stride, n_columns, d_proj, d_out,
                           out_stride, flags);
}

static int pack_records_core(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                             const uint64_t *d_record_off, uint32_t n_variants, void *d_out, uint64_t out_stride,
                             const uint8_t *code_map, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags > PGENHIP_PACK_GATHER) return fail(PGENHIP_ERR_BAD_ARG, "unknown pack_records flag");
    uint32_t map8 = kPackIdentityMap;
    if (code_map) {
        map8 = 0u;
        for (uint32_t c = 0; c < 4u; c++) {
            if (code_map[c] > 3u) return fail(PGENHIP_ERR_BAD_ARG, "code_map entry > 3");
            map8 |= (uint32_t)code_map[c] << (2u * c);
        }
    }
    const uint32_t K = ctx->kept_count, RK = (K + 3u) / 4u;
    const bool all_kept = !ctx->subset || ctx->identity;
    if (flags == PGENHIP_PACK_DENSE && !all_kept) return fail(PGENHIP_ERR_BAD_ARG, "PGENHIP_PACK_DENSE needs all samples kept");
    if (flags == PGENHIP_PACK_GATHER && (!ctx->subset || K == 0u))
        return fail(PGENHIP_ERR_BAD_ARG, "PGENHIP_PACK_GATHER needs a kept list of at least one sample");
    if (n_variants == 0 || K == 0u) return PGENHIP_OK;   // nothing to write
    if (!d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    PackArgs a;
    rc = select_rows(ctx, a, d_records, record_stride, d_variant_idx, d_record_off, n_variants);
    if (rc) return rc;
    if (n_variants > 1 && out_stride < RK) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < one packed record");
    // byte offsets are 64-bit arithmetic in the kernels; the bound is decode_matrix's (2^52 bytes)
    if ((n_variants > 1 && out_stride >= kMaxSpan / n_variants) || record_span_too_large(record_stride, d_variant_idx, d_record_off, n_variants))
        return fail(PGENHIP_ERR_TOO_LARGE, "pack offsets do not fit the kernels' index types");
    a.kept_count = K;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_stride = out_stride;
    a.map8 = map8;
    const int blocks = ctx->tune.pack_blocks;
    a.kept_idx = all_kept ? nullptr : ctx->d_kept;
    if (flags == PGENHIP_PACK_DENSE || (flags == PGENHIP_PACK_AUTO && plan::pack::dense_applicable(a.kept_idx != nullptr, K, a.sample_count))) {
        HIP_TRY(launch_gt_pack_dense(a, blocks, ctx->num_cus, ctx->stream));
    } else if (flags == PGENHIP_PACK_GATHER || (flags == PGENHIP_PACK_AUTO && plan::pack::gather_applicable(a.kept_idx != nullptr, K))) {
        a.kept_idx = ctx->d_kept;   // forced on an identity list: the list is there
        HIP_TRY(launch_gt_pack_gather(a, blocks, ctx->num_cus, ctx->stream));
    } else {
        HIP_TRY(launch_gt_pack_general(a, blocks, ctx->num_cus, ctx->stream));
    }
    return PGENHIP_OK;
}

uint32_t pgenhip_packed_record_size(const pgenhip_ctx *ctx) { return ctx ? (ctx->kept_count + 3u) / 4u : 0u; }

int pgenhip_pack_records(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                         uint32_t n_variants, void *d_out, uint64_t out_stride, const uint8_t *code_map, uint32_t flags)
{
    return pack_records_core(ctx, d_records, record_stride, d_variant_idx, nullptr, n_variants, d_out, out_stride, code_map, flags);
}

int pgenhip_pack_records_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                            void *d_out, uint64_t out_stride, const uint8_t *code_map, uint32_t flags)
{
    if (const int rc = check_record_off(ctx, d_record_off, n_variants)) return rc;
    return pack_records_core(ctx, d_base, 0, nullptr, d_record_off, n_variants, d_out, out_stride, code_map, flags);
}

int pgenhip_parse_gt(pgenhip_ctx *ctx, const void *d_text, uint64_t text_len, const uint64_t *d_field_off, const uint64_t *d_line_end,
                     uint32_t n_lines, void *d_out, uint64_t out_stride, uint32_t *d_line_flags, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const uint32_t shape = flags & PGENHIP_PARSE_SHAPE_MASK;
    if ((flags & ~PGENHIP_PARSE_SHAPE_MASK) || shape > PGENHIP_PARSE_FIXED) return fail(PGENHIP_ERR_BAD_ARG, "unknown parse_gt flag");
    if (ctx->subset && !ctx->identity) return fail(PGENHIP_ERR_BAD_ARG, "parse_gt needs all samples kept (subsets are pack_records' job)");
    if (n_lines == 0) return PGENHIP_OK;   // nothing to write
    const uint32_t R = ctx->record_size;
    if (!d_field_off || !d_line_end || !d_line_flags) return fail(PGENHIP_ERR_BAD_ARG, "d_field_off, d_line_end or d_line_flags is NULL");
    if (!d_text && text_len) return fail(PGENHIP_ERR_BAD_ARG, "d_text is NULL");
    if (!d_out && R) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    if ((uintptr_t)d_line_flags & 3u) return fail(PGENHIP_ERR_BAD_ARG, "d_line_flags is not 4-byte aligned");
    if (((uintptr_t)d_field_off | (uintptr_t)d_line_end) & 7u) return fail(PGENHIP_ERR_BAD_ARG, "d_field_off or d_line_end is not 8-byte aligned");
    if (n_lines > 1 && out_stride < R) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < one record");
    // byte offsets are 64-bit arithmetic in the kernels; the bound is decode_matrix's (2^52 bytes)
    if (n_lines > 1 && out_stride >= kMaxSpan / n_lines) return fail(PGENHIP_ERR_TOO_LARGE, "parse offsets do not fit the kernels' index types");
    ParseArgs a;
    a.text = static_cast<const uint8_t *>(d_text);
    a.text_len = text_len;
    a.field_off = d_field_off;
    a.line_end = d_line_end;
    a.n_lines = n_lines;
    a.sample_count = ctx->sample_count;
    a.record_size = R;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_stride = out_stride;
    a.line_flags = d_line_flags;
    const int blocks = ctx->tune.parse_blocks;
    if (shape == PGENHIP_PARSE_GENERAL || (shape == PGENHIP_PARSE_AUTO && !plan::parse::kAutoFixedFirst)) {
        HIP_TRY(launch_gt_parse_general(a, false, blocks, ctx->num_cus, ctx->stream));
        return PGENHIP_OK;
    }
    HIP_TRY(hipMemsetAsync(d_line_flags, 0, 4u * (size_t)n_lines, ctx->stream));   // FIXED ORs into the flag words
    if (shape == PGENHIP_PARSE_FIXED) {
        // a declined line's record bytes stay untouched: decide every line first, then write the lines that were taken
        HIP_TRY(launch_gt_parse_fixed(a, true, false, blocks, ctx->num_cus, ctx->stream));
        HIP_TRY(launch_gt_parse_fixed(a, false, true, blocks, ctx->num_cus, ctx->stream));
    } else {
        // AUTO: one FIXED pass that writes as it decides, then GENERAL rewrites the declined lines, flag words included
        HIP_TRY(launch_gt_parse_fixed(a, true, true, blocks, ctx->num_cus, ctx->stream));
        HIP_TRY(launch_gt_parse_general(a, true, blocks, ctx->num_cus, ctx->stream));
    }
    return PGENHIP_OK;
}

int pgenhip_join_records(pgenhip_ctx *ctx, const pgenhip_join_part *parts, uint32_t n_parts, uint32_t n_variants, void *d_out,
                         uint64_t out_stride, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (flags > PGENHIP_JOIN_STREAM) return fail(PGENHIP_ERR_BAD_ARG, "unknown join_records flag");
    if (!parts) return fail(PGENHIP_ERR_BAD_ARG, "parts is NULL");
    if (n_parts == 0u || n_parts > PGENHIP_JOIN_MAX_PARTS) return fail(PGENHIP_ERR_BAD_ARG, "n_parts must be 1 .. PGENHIP_JOIN_MAX_PARTS");
    if (ctx->subset && !ctx->identity) return fail(PGENHIP_ERR_BAD_ARG, "join_records needs all samples kept (subsets are pack_records' job)");
    uint64_t sum = 0u;
    for (uint32_t p = 0; p < n_parts; p++) {
        if (parts[p].reserved != 0u) return fail(PGENHIP_ERR_BAD_ARG, "a part's reserved field is not 0");
        sum += parts[p].sample_count;
    }
    if (sum != ctx->sample_count) return fail(PGENHIP_ERR_BAD_ARG, "the parts' sample counts do not add up to the ctx's sample count");
    if (n_variants == 0 || sum == 0u) return PGENHIP_OK;   // nothing to write
    const uint32_t R = ctx->record_size;
    JoinArgs a{};
    for (uint32_t p = 0; p < n_parts; p++) {   // the table holds the parts that have samples
        const pgenhip_join_part &s = parts[p];
        if (s.sample_count == 0u) continue;
        if (!s.d_base || !s.d_record_off) return fail(PGENHIP_ERR_BAD_ARG, "a part with samples has a NULL d_base or d_record_off");
        if ((uintptr_t)s.d_record_off & 7u) return fail(PGENHIP_ERR_BAD_ARG, "a part's d_record_off is not 8-byte aligned");
        JoinPart &t = a.part[a.n_parts];
        t.base = static_cast<const uint8_t *>(s.d_base);
        t.record_off = s.d_record_off;
        t.flip = s.d_flip;
        t.start = a.n_parts ? a.part[a.n_parts - 1u].start + a.part[a.n_parts - 1u].count : 0u;
        t.count = s.sample_count;
        a.n_parts++;
    }
    if (!d_out) return fail(PGENHIP_ERR_BAD_ARG, "d_out is NULL");
    if (n_variants > 1 && out_stride < R) return fail(PGENHIP_ERR_BAD_ARG, "out_stride < one record");
    // byte offsets are 64-bit arithmetic in the kernels; the bound is decode_matrix's (2^52 bytes)
    if (n_variants > 1 && out_stride >= kMaxSpan / n_variants) return fail(PGENHIP_ERR_TOO_LARGE, "join offsets do not fit the kernels' index types");
    a.n_variants = n_variants;
    a.sample_count = ctx->sample_count;
    a.record_size = R;
    a.out = static_cast<uint8_t *>(d_out);
    a.out_stride = out_stride;
    const int blocks = ctx->tune.join_blocks;
    if (flags == PGENHIP_JOIN_STREAM || (flags == PGENHIP_JOIN_AUTO && plan::join::auto_stream(R, n_variants, a.n_parts))) {
        HIP_TRY(launch_gt_join_stream(a, blocks, ctx->num_cus, ctx->stream));
    } else {
        HIP_TRY(launch_gt_join_general(a, blocks, ctx->num_cus, ctx->stream));
    }
    return PGENHIP_OK;
}

int pgenhip_tune(pgenhip_ctx *ctx, uint32_t knob, int32_t value)
{
    if (!ctx) return fail(PGENHIP_ERR_BAD_ARG, "ctx is NULL");
    const Tuning d;  // the defaults
    Tuning &t = ctx->tune;
    switch (knob) {
        case PGENHIP_KNOB_WIDE_BLOCKS_PER_CU: t.wide_blocks_per_cu = value > 0 ? value : d.wide_blocks_per_cu; break;
        case PGENHIP_KNOB_WIDE_RANGES:
            if (value < 0 || value > (int32_t)kMaxQueueRanges || (value & (value - 1)) != 0) return fail(PGENHIP_ERR_BAD_ARG, "ranges must be a power of two up to 64");
            t.wide_ranges = value ? value : d.wide_ranges;
            break;
        case PGENHIP_KNOB_FLAT_BLOCKS_PER_CU: t.flat_blocks_per_cu = value > 0 ? value : d.flat_blocks_per_cu; break;
        case PGENHIP_KNOB_SCAN_BLOCKS_PER_CU: t.scan_blocks_per_cu = value > 0 ? value : d.scan_blocks_per_cu; break;
        case PGENHIP_KNOB_PICK_BATCH_BYTES: t.pick_batch_bytes = value > 0 ? value : d.pick_batch_bytes; break;
        case PGENHIP_KNOB_SCAN_XCD_MAP: t.scan_xcd_map = value < 0 ? 0 : 1; break;
        case PGENHIP_KNOB_SCAN_CHUNK_ROWS: t.scan_chunk_rows = value > 0 ? value : d.scan_chunk_rows; break;
        case PGENHIP_KNOB_SCAN_TWO_PASS: t.scan_two_pass = value < 0 ? 0 : 1; break;
        case PGENHIP_KNOB_ROWPICK_BLOCKS_PER_CU: t.rowpick_blocks_per_cu = value > 0 ? value : d.rowpick_blocks_per_cu; break;
        case PGENHIP_KNOB_SCAN_ROWPICK: t.scan_rowpick = value < 0 ? 0 : 1; break;
        case PGENHIP_KNOB_ALIGN_STORES: t.align_stores = value < 0 ? 0 : 1; break;
        case PGENHIP_KNOB_RUNS_ROWS: t.runs_rows = value > 0 ? value : d.runs_rows; break;
        case PGENHIP_KNOB_SCOUNT_SLICES: t.scount_slices = value > 0 ? value : d.scount_slices; break;
        case PGENHIP_KNOB_SCORE_SLICES: t.score_slices = value > 0 ? value : d.score_slices; break;
        case PGENHIP_KNOB_MATRIX_BLOCKS: t.matrix_blocks = value > 0 ? value : d.matrix_blocks; break;
        case PGENHIP_KNOB_PAIR_BLOCKS: t.pair_blocks = value > 0 ? value : d.pair_blocks; break;
        case PGENHIP_KNOB_PACK_BLOCKS: t.pack_blocks = value > 0 ? value : d.pack_blocks; break;
        case PGENHIP_KNOB_PARSE_BLOCKS: t.parse_blocks = value > 0 ? value : d.parse_blocks; break;
        case PGENHIP_KNOB_JOIN_BLOCKS: t.join_blocks = value > 0 ? value : d.join_blocks; break;
        case PGENHIP_KNOB_PRUNE_BLOCKS: t.prune_blocks = value > 0 ? value : d.prune_blocks; break;
        case PGENHIP_KNOB_SPAIR_SLICES: t.spair_slices = value > 0 ? value : d.spair_slices; break;
        case PGENHIP_KNOB_VSUM_BLOCKS: t.vsum_blocks = value > 0 ? value : d.vsum_blocks; break;
        case PGENHIP_KNOB_LOGIT_BLOCKS: t.logit_blocks = value > 0 ? value : d.logit_blocks; break;
        case PGENHIP_KNOB_GRAM_SLICES: t.gram_slices = value > 0 ? value : d.gram_slices; break;
        case PGENHIP_KNOB_GAPPLY_SAMPLE_SLICES: t.gapply_sample_slices = value > 0 ? value : d.gapply_sample_slices; break;
        case PGENHIP_KNOB_GAPPLY_ROW_SLICES: t.gapply_row_slices = value > 0 ? value : d.gapply_row_slices; break;
        case PGENHIP_KNOB_STORE_POLICY:
            if (value < 0 || value > 2) return fail(PGENHIP_ERR_BAD_ARG, "store policy must be 0 (rule), 1 (nt) or 2 (nt sc1)");
            t.store_policy = value;
            break;
        case PGENHIP_KNOB_WIDE_BURST:
            if (value < 0 || value > 2) return fail(PGENHIP_ERR_BAD_ARG, "burst must be 0 (rule), 1 or 2");
            t.wide_burst = value;
            break;
        default: return fail(PGENHIP_ERR_BAD_ARG, "unknown knob");
    }
    return PGENHIP_OK;
}

int pgenhip_wait(pgenhip_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_timer_start(pgenhip_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_timer_stop(pgenhip_ctx *ctx, float *elapsed_ms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!elapsed_ms) return fail(PGENHIP_ERR_BAD_ARG, "elapsed_ms is NULL");
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev_stop));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->ev_start, ctx->ev_stop));
    return PGENHIP_OK;
}

int pgenhip_timer_mark(pgenhip_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_timer_read(pgenhip_ctx *ctx, float *elapsed_ms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!elapsed_ms) return fail(PGENHIP_ERR_BAD_ARG, "elapsed_ms is NULL");
    HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->ev_start, ctx->ev_stop));
    return PGENHIP_OK;
}

int pgenhip_device_malloc(pgenhip_ctx *ctx, void **d_ptr, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_ptr) return fail(PGENHIP_ERR_BAD_ARG, "d_ptr is NULL");
    *d_ptr = nullptr;
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1));
    return PGENHIP_OK;
}

int pgenhip_device_free(pgenhip_ctx *ctx, void *d_ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (d_ptr) HIP_TRY(hipFree(d_ptr));
    return PGENHIP_OK;
}

int pgenhip_host_malloc_pinned(pgenhip_ctx *ctx, void **h_ptr, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!h_ptr) return fail(PGENHIP_ERR_BAD_ARG, "h_ptr is NULL");
    *h_ptr = nullptr;
    HIP_TRY(hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return PGENHIP_OK;
}

int pgenhip_host_free_pinned(pgenhip_ctx *ctx, void *h_ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (h_ptr) HIP_TRY(hipHostFree(h_ptr));
    return PGENHIP_OK;
}

int pgenhip_memcpy_h2d(pgenhip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (bytes && (!d_dst || !h_src)) return fail(PGENHIP_ERR_BAD_ARG, "NULL pointer");
    if (bytes) HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_memcpy_d2h(pgenhip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (bytes && (!h_dst || !d_src)) return fail(PGENHIP_ERR_BAD_ARG, "NULL pointer");
    if (bytes) HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PGENHIP_OK;
}

int pgenhip_device_memory(pgenhip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!free_bytes && !total_bytes) return fail(PGENHIP_ERR_BAD_ARG, "free_bytes and total_bytes are both NULL");
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return PGENHIP_OK;
}

int pgenhip_synth_records(pgenhip_ctx *ctx, void *d_dst, uint64_t record_stride,
                          uint64_t first_variant, uint32_t n_variants, uint64_t seed, uint32_t flags)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_variants && ctx->record_size && !d_dst) return fail(PGENHIP_ERR_BAD_ARG, "d_dst is NULL");
    if (n_variants > 1 && record_stride < ctx->record_size) return fail(PGENHIP_ERR_BAD_ARG, "record_stride < record size");
    if (flags & ~(PGENHIP_SYNTH_DIRTY_PAD | PGENHIP_SYNTH_HWE)) return fail(PGENHIP_ERR_BAD_ARG, "unknown synth flag");
    if (flags & PGENHIP_SYNTH_HWE) {
        HIP_TRY(launch_synth_records_hwe(static_cast<uint8_t *>(d_dst), record_stride, ctx->sample_count, first_variant, n_variants, seed,
                                         ctx->num_cus, ctx->stream));
        return PGENHIP_OK;
    }
    HIP_TRY(launch_synth_records(static_cast<uint8_t *>(d_dst), record_stride, ctx->sample_count, first_variant,
                                 n_variants, seed, (flags & PGENHIP_SYNTH_DIRTY_PAD) != 0, ctx->num_cus, ctx->stream));
    return PGENHIP_OK;
}

}  // extern "C"
