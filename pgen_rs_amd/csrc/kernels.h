// kernels.h — host-callable launchers of the gfx950 kernels (internal to libpgen_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch_plan.h"

namespace pgenhip {

// Which records a launch reads: the selected rows of every kernel family (each argument struct below starts with these fields).
struct RowSource {
    const uint8_t *records;       // device; row r at records + r*record_stride
    uint64_t record_stride;
    const uint32_t *variant_idx;  // device or nullptr (identity)
    const uint64_t *record_off;   // device or nullptr; when set, row j's record starts at records + record_off[j] (byte offsets:
                                  // uncompressed records of a variable-width .pgen) and variant_idx / record_stride are not used
    uint32_t n_variants;
    uint32_t sample_count;        // N
    uint32_t record_size;         // R = ceil(N/4)
};

// One launch = one block of kept variants (src/pfile.rs:156 outer loop, many iterations at once).
struct EmitArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples)
    uint32_t kept_count;          // K (== N when kept_idx is nullptr)
    uint8_t *out;                 // device
    uint64_t out_stride;          // GT-segment mode: row j at out + j*out_stride
    // full-line mode (all three non-null): line j at out + line_off[j], prefix bytes first
    const uint8_t *prefix_blob;
    const uint64_t *prefix_off;
    const uint64_t *line_off;
    uint64_t max_line_bytes;      // upper bound of any line's byte length (prefix + 4K + 1)
    uint64_t *work_counters;      // device scratch owned by the ctx, one block per launch in flight: 8 x 128-B-spaced work-queue heads + a block-exit counter at +1024 B; zero between launches (the last block out re-zeroes them)
};

// Work-queue kernels: up to kMaxQueueRanges contiguous item ranges per launch, one 128-B-spaced head word each, and the block-exit
// counter behind them (a launch's counter block: (kMaxQueueRanges + 1) * 128 bytes; capi.hip keeps a ring of them)
constexpr uint32_t kMaxQueueRanges = 64;

// Launch-shape knobs, resolved ONCE per context: pgenhip_create sets the measured defaults below and
// pgenhip_tune overrides one (tests force small grids to exercise ring reuse; A/B probes).  Nothing on the
// launch path reads the process environment.
struct Tuning {
    int wide_blocks_per_cu = 0;    // stream kernel: 0 = by shape (plan::wide::rule: what the occupancy API says is resident, two on short launches)
    int wide_ranges = 0;           // stream kernel: work-queue ranges = write fronts of a launch (power of two <= 64); 0 = by shape (plan::wide::rule: 8 for rows of several spans and long RUNS launches, else 2)
    int flat_blocks_per_cu = 64;   // flat kernel: grid cap
    int scan_blocks_per_cu = 0;    // segment kernel: 0 = the measured rule (2 from ~0.6 % kept, else what the occupancy API says)
    int pick_batch_bytes = 32768;  // short-record pick kernel: text per batch (one store drain per batch)
    int scan_xcd_map = 1;          // segment kernels: all blocks of a row group on one XCD (seam lines merge in one L2); 0 = plain map
    int scan_chunk_rows = 0;       // two-pass path: rows per chunk (0 = as many as the launch's 32-MiB compact-scratch slice holds; tests force small chunks)
    int scan_two_pass = 1;         // sparse keeps on long records: compact pass + all-samples pass (0 = single-pass segment kernel)
    int rowpick_blocks_per_cu = 0; // row-owner kernel: cap on resident blocks per CU (0 = what the occupancy API says)
    int scan_rowpick = 1;          // kept subsets on long records, many rows: the row-owner kernel where it measures ahead (its single pass, or its
                                   // compact pass of the two passes); 0 = never (the segment kernels: single pass or segment compact pass)
    int align_stores = 1;          // subset kernels: lanes <-> chunks shifted so that every store instruction covers whole 128-byte lines (0 = from the first whole chunk)
    int runs_rows = 0;             // RUNS mode of the stream kernel: rows per work item (0 = as many as one wide load / one span holds)
    int scount_slices = 0;         // per-sample counts: row ranges per column tile (0 = as many as fill the chip's resident blocks)
    int score_slices = 0;          // per-sample scores: row ranges per column tile (0 = by shape: the chip's resident blocks, at least 512 rows each)
    int matrix_blocks = 0;         // genotype matrix kernels: grid size in blocks (0 = by shape, capped per CU)
    int pair_blocks = 0;           // pairwise kernel: grid size in blocks (0 = by shape, capped per CU)
    int pack_blocks = 0;           // pack kernels: grid size in blocks (0 = by shape, capped per CU)
    int parse_blocks = 0;          // GT text parse kernels: grid size in blocks (0 = by shape, capped per CU)
    int join_blocks = 0;           // join kernels: grid size in blocks (0 = by shape, capped per CU)
    int prune_blocks = 0;          // prune resolve kernels: grid size in blocks (0 = by shape); for BLOCK thereby the rows of a range
    int spair_slices = 0;          // pairwise sample tables: row ranges per sample tile (0 = by shape: the chip's resident blocks, at least 256 rows each)
    int vsum_blocks = 0;           // per-variant sums: grid size in blocks (0 = by shape, capped per CU)
    int logit_blocks = 0;          // per-variant logistic regression: grid size in blocks (0 = by shape, capped per CU)
    int gram_slices = 0;           // sample Gram matrix: row ranges per rank tile (0 = by shape: the chip's resident blocks, at least 256 rows each)
    int gapply_sample_slices = 0;  // Gram product, P pass: sample ranges per row tile (0 = by shape: the chip's resident blocks, at least 4096 samples each)
    int gapply_row_slices = 0;     // Gram product, Y pass: row ranges per sample tile (0 = by shape: the chip's resident blocks, at least 256 rows each)
    int store_policy = 0;          // stream kernel (row items, LINES, RUNS): how text is stored (0 = the measured rule, plan::wide::rule, 1 = nt, 2 = nt sc1, write-through)
    int wide_burst = 0;            // stream kernel (row items, LINES): plain store steps issued back to back (0 = the measured rule: 1 on long launches of rows of several spans, else 2)
};

// rows are gathered (variant list or byte offsets): the HAS_VIDX instantiations
__host__ __device__ inline bool gathered(const RowSource &a) { return a.variant_idx != nullptr || a.record_off != nullptr; }

// The scalars the emit path decides from (plan::emit of launch_plan.h: applicability, AUTO, launch plans)
__host__ __device__ inline plan::emit::Shape emit_shape(const EmitArgs &a)
{
    plan::emit::Shape s{};
    s.N = a.sample_count, s.K = a.kept_count, s.R = a.record_size, s.V = a.n_variants;
    s.kept_list = a.kept_idx != nullptr;
    s.lines = a.line_off != nullptr;   // (the entry point refuses full lines without prefix_off)
    s.gathered = gathered(a);
    s.records_dense = a.n_variants <= 1u || a.record_stride == a.record_size;
    s.out_dense = a.n_variants <= 1u || a.out_stride == 4ull * a.kept_count + 1ull;
    s.max_line_bytes = a.max_line_bytes;
    s.prefix_blob = a.prefix_blob != nullptr;
    return s;
}

// The emit launchers.  Which shapes each takes is plan::emit's (flat, wide, wide_lines, runs, lineruns, pick, rowpick_takes); the
// work-queue kernels (wide, runs, lineruns) also refuse a null a.work_counters.
// General row-tiled kernel: any alignment, any strides, list gather for kept subsets.
hipError_t launch_gt_rows(const EmitArgs &a, int num_cus, hipStream_t stream);

// Dense all-samples stream kernel (K = N, out_stride == 4N+1): every lane owns one aligned
// 16-byte chunk of the whole launch's output stream.
hipError_t launch_gt_flat(const EmitArgs &a, const Tuning &t, int num_cus, hipStream_t stream);

// Same contract as the flat kernel, but records are staged with wide (16 B/lane) loads through LDS by a loader
// wave and storer waves issue 16 coalesced 1-KiB stores per work item (rows >= 4 KiB of text); also full lines
// (line_off / prefix_off set).
hipError_t launch_gt_wide(const EmitArgs &a, const Tuning &t, int num_cus, hipStream_t stream);
// RUNS mode of the same kernel for SHORT rows (8 <= N <= ~2000, dense records and dense text, no gather): a work item
// is a run of consecutive rows — one wide load of their contiguous record bytes, their text as one contiguous run.
hipError_t launch_gt_runs(const EmitArgs &a, const Tuning &t, int num_cus, hipStream_t stream);
// Runs of FULL LINES (line_off / prefix_off set) on short rows, all samples kept, dense records: prefixes, GT text and '\n' of a
// run of lines assembled in the storers' LDS stages and stored as whole 128-B lines (gt_wide.hip, gt_lineruns_kernel).
hipError_t launch_gt_lineruns(const EmitArgs &a, const Tuning &t, int num_cus, hipStream_t stream);

// Kept-subset segment kernels: number of kept samples before each segment of kScanSegmentSamples samples.
using plan::emit::kScanSegmentSamples;
struct ScanArgs {
    const uint32_t *seg_rank;    // device; n_segments + 1 entries
    uint32_t max_seg_count;      // most kept samples in any one segment
    uint32_t align_stores;       // Tuning::align_stores
};
using plan::emit::kCompactMaxSegCodes;   // the compact pass takes segments with at most this many kept samples
// compact = true: write each row's COMPACT record (the K kept codes packed like a mode-0x02 record of K samples) to a.out + j * a.out_stride
// instead of text: the first pass of the two-pass path for sparse keeps (capi.hip)
hipError_t launch_gt_scan(const EmitArgs &a, const ScanArgs &sc, const Tuning &t, int num_cus, hipStream_t stream, bool compact = false);

// Sparse kept subsets on long records, one wave per ROW (gt_rowpick.hip): the whole kept list as the LDS table, the row's compact
// record assembled in LDS segment by segment, its text written in one go.  Any strides / gathers / full lines.
using plan::emit::kRowPickMaxKept;
// compact = true: the row's COMPACT record (ceil(K / 4) bytes at a.out + row * a.out_stride) instead of its text: first pass of the two-pass path
uint32_t gt_rowpick_resident_waves(const EmitArgs &a, const Tuning &t, int num_cus, bool compact);   // rows of one round (0: not applicable)
hipError_t launch_gt_rowpick(const EmitArgs &a, const ScanArgs &sc, const Tuning &t, int num_cus, hipStream_t stream, bool compact = false);

// kept subsets on short records (N <= 4096): output-driven pick through the kept list, no compaction (gt_pick.hip)
hipError_t launch_gt_pick(const EmitArgs &a, const Tuning &t, int num_cus, hipStream_t stream);

// Per-variant genotype counts (gt_count.hip): four u32 per selected row at counts + 4 * j (hom-ref, het, hom-alt, missing).
struct CountArgs : RowSource {
    uint32_t kept_count;          // K (== N without a mask)
    const uint8_t *kept_mask;     // device or nullptr (all samples): 16 zero bytes, then 2 bits per sample like a record (0b01 = kept), then zeros
    uint32_t *counts;             // device
};
// Bytes of the ctx's kept mask buffer for records of R bytes: the mask behind 16 zero bytes, zeros up to the last chunk a row can touch
inline size_t gt_count_mask_bytes(uint32_t record_size) { return 16u * ((size_t)(record_size + 30u) / 16u + 2u); }
// wave_per_row: one wave per row (long rows); else 4 .. 32 lanes per row, several rows per wave (short rows); AUTO's choice is
// plan::count::wave_per_row
hipError_t launch_gt_count(const CountArgs &a, bool wave_per_row, int num_cus, hipStream_t stream);

// Per-sample genotype counts (gt_scount.hip): the counts of the selected rows added into counts[4 * k + c] for every kept
// sample k (hom-ref, het, hom-alt, missing; u32 modular).
struct ScountArgs : RowSource {
    const uint8_t *kept_mask;     // device or nullptr (all samples): the ctx's count mask (CountArgs::kept_mask)
    const uint32_t *kept_rank;    // device, with kept_mask: kept samples before each 64-sample chunk
    uint32_t *counts;             // device, 4-byte aligned
};
// slices_per_tile: row ranges per column tile (0 = as many as fill the chip's resident blocks)
hipError_t launch_gt_scount(const ScountArgs &a, int slices_per_tile, int num_cus, hipStream_t stream);

// Per-sample weighted dosage sums (gt_score.hip): for every kept sample k and column c < n_columns the FP64 sum over the selected
// rows j of (double)weights[j * w_stride + c] * D(j, k), added into scores[k * n_columns + c]; D = 0, 1, 2 for codes 0, 1, 2 and
// (double)miss[j] for code 3 (0 without miss).  weights and miss are indexed by the row's position in the selection.
struct ScoreArgs : RowSource {
    const uint8_t *kept_mask;     // device or nullptr (all samples): the ctx's count mask (CountArgs::kept_mask)
    const uint32_t *kept_rank;    // device, with kept_mask: kept samples before each 64-sample chunk
    const float *weights;         // device, 4-byte aligned
    uint64_t w_stride;            // floats between the weight rows
    uint32_t n_columns;           // C, 1 .. 8
    const float *miss;            // device, 4-byte aligned, or nullptr
    double *scores;               // device, 8-byte aligned, ordinary device memory (hardware FP64 atomics)
};
// slices_per_tile: row ranges per column tile (0 = by shape)
hipError_t launch_gt_score(const ScoreArgs &a, int slices_per_tile, int num_cus, hipStream_t stream);

// Per-variant sums of per-sample values by genotype code (gt_vsum.hip): for every selected row j, column c < n_columns and code x
// the FP64 sum over the kept samples k with code x in row j of values[k * v_stride + c], at sums[(j * n_columns + c) * 4 + x].
struct VsumArgs : RowSource {
    const uint8_t *kept_mask;     // device or nullptr (all samples): the ctx's count mask (CountArgs::kept_mask)
    const uint32_t *kept_rank;    // device, with kept_mask: kept samples before each 64-sample chunk
    const double *values;         // device, 8-byte aligned, K x n_columns
    uint64_t v_stride;            // doubles between the value rows
    uint32_t n_columns;           // C, 1 .. 16
    double *sums;                 // device, 8-byte aligned, ordinary device memory (hardware FP64 atomics)
};
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loops and the multi-tile combine)
hipError_t launch_gt_vsum_general(const VsumArgs &a, int blocks, int num_cus, hipStream_t stream);
// the matrix-core shape: any layout, any keep set with K >= 1.  It only ADDS when plan::vsum::mfma_atomic(record_size) (rows of
// more than one tile): the caller zeroes the sums first
hipError_t launch_gt_vsum_mfma(const VsumArgs &a, int blocks, int num_cus, hipStream_t stream);

// Numeric genotype matrix (gt_matrix.hip):element (j, k) = the pattern of the code of kept sample k in selected row j.
struct MatrixArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples, or an identity list)
    uint32_t kept_count;          // K (== N when kept_idx is nullptr)
    uint8_t *out;                 // device, a multiple of elem_bytes
    uint64_t out_stride;          // bytes between output rows (variant-major: rows are variants; sample-major: kept samples)
    uint32_t elem_bytes;          // 1, 2 or 4
    uint32_t sample_major;        // 0: (j, k) at out + j*out_stride + k*elem_bytes; 1: at out + k*out_stride + j*elem_bytes
    uint32_t tab[4];              // the patterns of codes 0-3, zero-extended
};
// STREAM needs variant-major with all samples kept, TILE sample-major with all samples kept and out, out_stride multiples of 16
// (plan::matrix::stream_applicable, tile_applicable; AUTO asks plan::matrix::auto_shape)
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loops)
hipError_t launch_gt_matrix_general(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_matrix_stream(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_matrix_tile(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream);

// Windowed pairwise tables (gt_pair.hip): pair (i, i + d), i < n_left, 1 <= d <= window, i + d < n_variants, at pair index
// p = i * window + d - 1: sixteen u32 at out + 64 p (T[a][b] at word 4 a + b), or with r2 one float at out + 4 p.
struct PairArgs : RowSource {
    uint32_t kept_count;          // K (== N without a mask)
    const uint8_t *kept_mask;     // device or nullptr (all samples): the ctx's count mask (CountArgs::kept_mask)
    uint32_t n_left;              // <= n_variants
    uint32_t window;              // W >= 1
    void *out;                    // device; 16-byte aligned for tables, 4-byte aligned for r2
    uint32_t r2;                  // 0: tables; 1: r^2
};
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loop)
hipError_t launch_gt_pair(const PairArgs &a, int blocks, int num_cus, hipStream_t stream);
// One bit per pair instead (same kernel, third epilogue; out and r2 are not used): the pair is an edge iff its r^2 (PairArgs' r2
// value) > min_r2 and key[j] - key[i] (mod 2^64) <= max_span; bit (d - 1) & 31 of fwd[i * mask_stride + (d - 1) / 32] and of
// bwd[j * mask_stride + (d - 1) / 32] is then ORed in (atomics).  Nothing else is written.
struct PairMaskArgs : PairArgs {
    float min_r2;                 // not NaN
    const uint64_t *key;          // device or nullptr (every pair is inside the span), one per selected row
    uint64_t max_span;
    uint32_t *fwd;                // device, 4-byte aligned
    uint32_t *bwd;                // device or nullptr (forward mask only)
    uint64_t mask_stride;         // u32 words per mask row, >= ceil(window / 32)
};
hipError_t launch_gt_pair_mask(const PairMaskArgs &a, int blocks, int num_cus, hipStream_t stream);

// Greedy independent set of the graph two such masks hold (gt_prune.hip): state[v] 0 undecided, 1 kept, 2 removed.  Row u beats v
// iff priority[u] > priority[v], or they are equal (or priority is nullptr) and u < v.  A sweep decides every undecided row whose
// beating neighbours are all decided: kept iff none of them is kept.  States only go from 0 to their final value.
struct PruneArgs {
    const uint32_t *fwd, *bwd;    // device; bit d - 1 of row v: neighbour v + d / v - d
    uint64_t mask_stride;         // u32 words per mask row
    uint32_t window;              // bits d - 1 >= window are ignored
    uint64_t n_rows;
    const uint32_t *priority;     // device or nullptr
    uint8_t *state;               // device
    unsigned long long *undecided;   // device, zero at launch: every block adds the rows it leaves undecided
};
// blocks: forced grid size (0 = by shape).  GENERAL: a lane per row, one sweep.  BLOCK: a workgroup per contiguous range of rows
// (plan::prune::block_plan), swept to a local fixed point in LDS.
hipError_t launch_gt_prune_general(const PruneArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_prune_block(const PruneArgs &a, int blocks, int num_cus, hipStream_t stream);

// Pairwise sample tables (gt_spair.hip): for a = a_begin + i, b = b_begin + l (ranks in the kept list) the number of selected rows
// in which a has code x and b has code y, ADDED to out[16 * (i * b_count + l) + 4 * x + y] (u32, modular).
struct SpairArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples, or an identity list): rank -> sample
    uint32_t a_begin, a_count;    // a_begin + a_count <= K
    uint32_t b_begin, b_count;    // b_begin + b_count <= K
    uint32_t *out;                // device, 16-byte aligned
};
// slices_per_tile: row ranges per sample tile, each summed by one block (0 = by shape)
hipError_t launch_gt_spair_general(const SpairArgs &a, int slices_per_tile, int num_cus, hipStream_t stream);
hipError_t launch_gt_spair_mfma(const SpairArgs &a, int slices_per_tile, int num_cus, hipStream_t stream);

// Sample Gram matrix (gt_gram.hip): for a = a_begin + i, b = b_begin + l (ranks in the kept list) the FP64 sum over the selected rows
// j of t_j[x_j(a)] * t_j[x_j(b)], t_j = code_values[4 j .. 4 j + 3] (indexed by the row's position in the selection), at
// out[i * out_stride + l]: stored when `store`, else ADDED (FP64 atomics; the caller zeroes the entries first unless it accumulates).
struct GramArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples, or an identity list): rank -> sample
    uint32_t a_begin, a_count;    // a_begin + a_count <= K
    uint32_t b_begin, b_count;    // b_begin + b_count <= K
    const double *code_values;    // device, 8-byte aligned, four per selected row
    double *out;                  // device, 8-byte aligned, ordinary device memory (hardware FP64 atomics)
    uint64_t out_stride;          // doubles between the output rows
    uint32_t store;               // 1: every entry has one owner and is overwritten (one slice, no ACCUMULATE): plain stores
};
// slices: row ranges per tile (plan::gram::general_slices / mfma_slices); 1 means every entry has one owner
hipError_t launch_gt_gram_general(const GramArgs &a, uint32_t slices, hipStream_t stream);
hipError_t launch_gt_gram_mfma(const GramArgs &a, uint32_t slices, hipStream_t stream);

// Gram product (gt_gapply.hip): with Z[j][k] = t_j[x_j(k)] over the selected rows j and ALL kept samples k (ranks), the P pass gives
// proj[j * n_columns + c] = sum over k of Z[j][k] * q[k * q_stride + c] and the Y pass out[k * out_stride + c] = sum over j of
// Z[j][k] * proj[j * n_columns + c].  A pass with one slice that overwrites stores; everything else ADDS with FP64 atomics (the caller
// zeroes first unless it accumulates).
struct GapplyArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples, or an identity list): rank -> sample
    uint32_t kept_count;          // K >= 1
    const double *code_values;    // device, 8-byte aligned, four per selected row
    const double *q;              // device, 8-byte aligned, K rows of n_columns
    uint64_t q_stride;            // doubles between the rows of q
    uint32_t n_columns;           // C, 1 .. 16
    double *proj;                 // device, 8-byte aligned, n_variants x n_columns, ordinary device memory (hardware FP64 atomics)
    double *out;                  // device, 8-byte aligned, ordinary device memory
    uint64_t out_stride;          // doubles between the rows of out
    uint32_t p_store, y_store;    // 1: the pass has one slice (and out is overwritten): every entry has one owner and is stored
};
// tiles / grid / slices of each pass: plan::gapply::plan of the same shape
hipError_t launch_gt_gapply_p(const GapplyArgs &a, bool mfma, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream);
hipError_t launch_gt_gapply_y(const GapplyArgs &a, bool mfma, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream);

// Per-variant logistic regression (gt_logit.hip): for every selected row j the Newton iteration of include/pgen_hip.h on
// X = [design, t_j[code]] over the kept samples whose table entry is not NaN; coefficients, the genotype's standard error and a
// status word per row.
struct LogitArgs : RowSource {
    const uint8_t *kept_mask;     // device or nullptr (all samples): the ctx's count mask (CountArgs::kept_mask)
    const uint32_t *kept_rank;    // device, with kept_mask: kept samples before each 64-sample chunk
    const double *code_values;    // device, 8-byte aligned, four per selected row
    const double *design;         // device, 8-byte aligned, K x n_cov
    uint64_t x_stride;            // doubles between the design rows
    uint32_t n_cov;               // 1 .. 15
    const double *y;              // device, K values
    const double *start;          // device, n_cov values
    uint32_t max_iter;            // 1 .. 64
    double tol;
    double *coef;                 // device, n_variants x (n_cov + 1)
    uint64_t c_stride;            // doubles between the coefficient rows
    double *se;                   // device, n_variants
    uint32_t *status;             // device, n_variants
};
// sample_count == 0 in the arguments means "no sample is included" (K == 0): every row ends SINGULAR at its first evaluation.
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loops)
hipError_t launch_gt_logit_general(const LogitArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_logit_fast(const LogitArgs &a, int blocks, int num_cus, hipStream_t stream);

// Packed records (gt_pack.hip): row j = the mode-0x02 record of the K kept samples of selected row j, ceil(K / 4) bytes at
// out + j * out_stride, every code sent through a 2-bit -> 2-bit map, pad bits zero.
struct PackArgs : RowSource {
    const uint32_t *kept_idx;     // device or nullptr (all samples, or an identity list)
    uint32_t kept_count;          // K (== N when kept_idx is nullptr)
    uint8_t *out;                 // device, any alignment
    uint64_t out_stride;          // bytes between output rows
    uint32_t map8;                // the code written for input code c at bits 2c, 2c + 1
};
constexpr uint32_t kPackIdentityMap = 0xE4u;
// DENSE needs all samples kept, GATHER a kept list with K >= 1 (plan::pack::dense_applicable, gather_applicable)
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loops)
hipError_t launch_gt_pack_general(const PackArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_pack_dense(const PackArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_pack_gather(const PackArgs &a, int blocks, int num_cus, hipStream_t stream);

// GT text -> records (gt_parse.hip): for line j the sample fields of text[field_off[j], line_end[j]) become the mode-0x02 record of
// N samples at out + j * out_stride (pad bits zero) and the line's PGENHIP_PARSE_* flag word.  Offsets past text_len are clamped.
struct ParseArgs {
    const uint8_t *text;          // device, any alignment
    uint64_t text_len;
    const uint64_t *field_off;    // device: the tab in front of sample 0's field
    const uint64_t *line_end;     // device: one past the last field's last byte
    uint32_t n_lines;
    uint32_t sample_count;        // N
    uint32_t record_size;         // R = ceil(N/4)
    uint8_t *out;                 // device, any alignment
    uint64_t out_stride;
    uint32_t *line_flags;         // device, one word per line
};
// GENERAL: any field width; overwrites a line's R record bytes and its flag word.  declined_only: takes the lines whose flag word
// has PGENHIP_PARSE_DECLINED (AUTO's second pass) and leaves the others alone.
hipError_t launch_gt_parse_general(const ParseArgs &a, bool declined_only, int blocks, int num_cus, hipStream_t stream);
// FIXED: regions of exactly 4N bytes of `\t[01.][/|][01.]`.  validate: ORs PHASED / HALF_CALL / DECLINED into the flag words (zero
// before the launch); write: stores the record bytes — with validate, of every 4N-byte line (AUTO: GENERAL rewrites the declined
// ones), without, of the lines a validate launch before it did not decline (forced FIXED).
hipError_t launch_gt_parse_fixed(const ParseArgs &a, bool validate, bool write, int blocks, int num_cus, hipStream_t stream);

// Sample-wise join (gt_join.hip): row j = the mode-0x02 record of N = sum count samples at out + j * out_stride, part p's samples at
// start .. start + count - 1, pad bits zero.  The table holds the parts that have samples, in order, their ranges tiling [0, N).
struct JoinPart {
    const uint8_t *base;          // device, any alignment
    const uint64_t *record_off;   // device: byte offset of row j's record from base, or PGENHIP_JOIN_ABSENT (code 3, nothing read)
    const uint8_t *flip;          // device or nullptr: flip[j] != 0 exchanges codes 0 and 2
    uint32_t start, count;        // first output sample, samples (count >= 1)
};
struct JoinArgs {
    JoinPart part[PGENHIP_JOIN_MAX_PARTS];
    uint32_t n_parts;
    uint32_t n_variants;
    uint32_t sample_count;        // N
    uint32_t record_size;         // R = ceil(N/4)
    uint8_t *out;                 // device, any alignment
    uint64_t out_stride;
};
// blocks: forced grid size (0 = by shape; tests force small grids to walk the grid-stride loops)
hipError_t launch_gt_join_general(const JoinArgs &a, int blocks, int num_cus, hipStream_t stream);
hipError_t launch_gt_join_stream(const JoinArgs &a, int blocks, int num_cus, hipStream_t stream);

// Deterministic synthetic records (SURVEY.md §8d counter-based generator).
hipError_t launch_synth_records(uint8_t *dst, uint64_t record_stride, uint32_t sample_count,
                                uint64_t first_variant, uint32_t n_variants, uint64_t seed,
                                bool dirty_pad, int num_cus, hipStream_t stream);

// "hwe" value distribution (per-variant allele frequency, Hardy-Weinberg genotype proportions, 0.1 % missing)
hipError_t launch_synth_records_hwe(uint8_t *dst, uint64_t record_stride, uint32_t sample_count, uint64_t first_variant,
                                    uint32_t n_variants, uint64_t seed, int num_cus, hipStream_t stream);

}  // namespace pgenhip
