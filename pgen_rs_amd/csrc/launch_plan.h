// launch_plan.h — the launch plans of the analysis kernels (gt_count, gt_scount, gt_score, gt_vsum, gt_matrix, gt_pair, gt_pack,
// gt_spair, gt_gram, gt_gapply, gt_parse, gt_join, gt_prune, gt_logit) and the launch rule of the stream kernel (gt_wide): lanes per row, tiles, row ranges ("slices"), grid
// caps, store policy and write fronts, as functions of scalars; and the emit path (namespace emit): the shapes each emit kernel takes,
// AUTO's chains and the forced kernel ids, the chunks of the two passes, and the launch plans of the segment, row-owner and pick
// kernels.  The single statement
// of every plan: capi.hip and the launchers call it, the kernels take their constants and their row ranges from it, and the tests compile this
// header for the host (tests/plan_probe.cpp, tests/gapply_plan_probe.cpp, tests/wide_plan_probe.cpp, tests/emit_plan_probe.cpp,
// tests/parse_plan_probe.cpp, tests/join_plan_probe.cpp, tests/prune_plan_probe.cpp, tests/logit_plan_probe.cpp) and run it.
// Plain C++17 on purpose: no HIP header, no kernel argument struct (emit::Shape is a struct of scalars).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/pgen_hip.h"   // the kernel ids (plain C)

#ifdef __HIPCC__
#define PGENHIP_PLAN_HD __host__ __device__ __attribute__((always_inline))
#else
#define PGENHIP_PLAN_HD
#endif

namespace pgenhip::plan {

// ---- shared ----------------------------------------------------------------------------------------------------------------------
// the chip's CUs as a launcher was told them (0: unknown, planned as 256)
PGENHIP_PLAN_HD inline uint64_t cu_count(int num_cus) { return (uint64_t)(num_cus > 0 ? num_cus : 256); }

// blocks of a grid-stride launch over `work` blocks' worth of items: capped at per_cu blocks per CU, or at the forced size; never 0
PGENHIP_PLAN_HD inline uint32_t grid_blocks(uint64_t work, uint32_t per_cu, int num_cus, int forced)
{
    const uint64_t cap = forced > 0 ? (uint64_t)forced : cu_count(num_cus) * per_cu;
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(work, cap));
}

// rows [begin, end) of slice `slice` of `slices`: the slices tile [0, V) in order, and none is empty while slices <= V
struct RowRange {
    uint64_t begin, end;
};
PGENHIP_PLAN_HD inline RowRange slice_rows(uint64_t V, uint32_t slice, uint32_t slices) { return {V * slice / slices, V * (slice + 1u) / slices}; }

// ---- gt_count: per-variant counts --------------------------------------------------------------------------------------------------
namespace count {

constexpr int kThreads = 256;
constexpr uint32_t kBlocksPerCu = 8;   // 32 waves per CU: up to 128 KiB of record loads in flight per CU on long rows

// the most aligned 16-byte chunks a row of R bytes can touch
PGENHIP_PLAN_HD constexpr uint32_t max_chunks(uint32_t record_size) { return (record_size + 30u) / 16u; }

// lanes per row of the short-row shape: as many as three passes over the row's chunks need (64: rows this long take the
// wave-per-row shape under AUTO)
PGENHIP_PLAN_HD constexpr uint32_t lanes_per_row(uint32_t record_size)
{
    const uint32_t chunks = max_chunks(record_size);
    return chunks <= 12u ? 4u : chunks <= 24u ? 8u : chunks <= 48u ? 16u : chunks <= 96u ? 32u : 64u;
}

// a wave per row: asked for, or AUTO (neither shape asked for) where the ladder says 64 lanes
PGENHIP_PLAN_HD constexpr bool wave_per_row(bool asked_wave_per_row, bool asked_rows_per_wave, uint32_t record_size)
{
    return asked_wave_per_row || (!asked_rows_per_wave && lanes_per_row(record_size) == 64u);
}

// the instantiation: G lanes per row, RU rows per group in flight, U chunks per lane per pass
struct Shape {
    uint32_t G, RU, U;
};
PGENHIP_PLAN_HD constexpr Shape shape(uint32_t record_size, bool wave_per_row)
{
    if (wave_per_row) return {64u, 1u, 4u};
    const uint32_t g = lanes_per_row(record_size);
    return {g < 32u ? g : 32u, 2u, 1u};   // (forced on long rows: G = 32, more passes per row)
}

PGENHIP_PLAN_HD constexpr uint32_t rows_per_step(uint32_t G, uint32_t RU) { return (64u / G) * RU; }   // rows a wave takes per turn of its loop
PGENHIP_PLAN_HD constexpr uint32_t rows_per_block(uint32_t G, uint32_t RU) { return (uint32_t)(kThreads / 64) * rows_per_step(G, RU); }

PGENHIP_PLAN_HD inline uint32_t grid(uint32_t n_variants, uint32_t G, uint32_t RU, int num_cus)
{
    const uint64_t per_block = rows_per_block(G, RU);
    return grid_blocks(((uint64_t)n_variants + per_block - 1u) / per_block, kBlocksPerCu, num_cus, 0);
}

// passes over the most chunks a row can span
PGENHIP_PLAN_HD constexpr uint32_t passes(uint32_t record_size, uint32_t G, uint32_t U) { return (max_chunks(record_size) + G * U - 1u) / (G * U); }

}  // namespace count

// ---- gt_scount: per-sample counts --------------------------------------------------------------------------------------------------
namespace scount {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBatch = 8;                           // rows per carry-save batch
constexpr int kHiBits = 8;                               // batch counter bits
constexpr uint32_t kWindowBatches = (1u << kHiBits) - 1u;   // batches between flushes (2 040 rows; a counter holds 2 047)
constexpr uint32_t kColWords = 65;                       // LDS words per 64-sample column chunk and category
constexpr uint32_t kMaxBlocksPerCu = 4;
constexpr uint32_t kLdsPerCu = 160u * 1024u;

// rows side by side in a block of G lanes per row
PGENHIP_PLAN_HD constexpr uint32_t slots(uint32_t G) { return kWaves * (64u / G); }

// the hi planes a flush reads after `batches` batches (<= kWindowBatches): planes past the batch count's bit length are zero
PGENHIP_PLAN_HD inline int hi_planes(uint32_t batches) { return 32 - __builtin_clz(batches | 1u); }

struct Plan {
    uint32_t G, tiles, cols, slices;
    size_t lds_bytes;
};

// slices_per_tile: forced (0 = as many as fill the chip's resident blocks); never more than one batch of every slot leaves rows for
PGENHIP_PLAN_HD inline Plan plan(uint32_t record_size, uint32_t n_variants, int num_cus, int slices_per_tile)
{
    Plan p{};
    const uint32_t C = (record_size + 15u) / 16u;   // column chunks of a row
    p.G = C <= 4u ? 4u : C <= 8u ? 8u : C <= 16u ? 16u : C <= 32u ? 32u : 64u;
    p.tiles = (C + p.G - 1u) / p.G;
    p.cols = p.tiles == 1u ? C : p.G;
    p.lds_bytes = (size_t)3u * p.cols * kColWords * sizeof(uint32_t);
    const uint32_t per_cu = std::max<uint32_t>(1u, std::min<uint32_t>(kMaxBlocksPerCu, kLdsPerCu / (uint32_t)p.lds_bytes));
    const uint64_t target = cu_count(num_cus) * per_cu;
    const uint64_t rows_per_block_step = (uint64_t)slots(p.G) * kBatch;   // one batch of every slot
    uint64_t s = slices_per_tile > 0 ? (uint64_t)slices_per_tile : std::max<uint64_t>(1u, target / p.tiles);
    s = std::min<uint64_t>(s, std::max<uint64_t>(1u, (n_variants + rows_per_block_step - 1u) / rows_per_block_step));
    p.slices = (uint32_t)std::min<uint64_t>(s, 0x7FFFFFFFull / p.tiles);
    return p;
}

}  // namespace scount

// ---- gt_score: per-sample weighted sums --------------------------------------------------------------------------------------------
namespace score {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxBlocksPerCu = 4;
constexpr uint32_t kMinSliceRows = 512;   // rows a slice takes at least when the plan is not forced: a block's flush is worth that many rows

PGENHIP_PLAN_HD constexpr uint32_t lane_bytes(uint32_t columns) { return columns <= 2u ? 4u : columns <= 4u ? 2u : 1u; }
PGENHIP_PLAN_HD constexpr uint32_t batch_rows(uint32_t columns) { return columns <= 4u ? 4u : 2u; }

// rows side by side in a block of 2^log_g lanes per row
PGENHIP_PLAN_HD constexpr uint32_t slots(uint32_t log_g) { return kWaves * (64u >> log_g); }

struct Plan {
    uint32_t bytes, log_g, tiles, slices;
};

PGENHIP_PLAN_HD inline Plan plan(uint32_t record_size, uint32_t n_variants, uint32_t n_columns, int num_cus, int slices_per_tile)
{
    Plan p{};
    p.bytes = lane_bytes(n_columns);
    const uint32_t units = (record_size + p.bytes - 1u) / p.bytes;   // units of a row
    p.log_g = 0u;
    while (p.log_g < 6u && (1u << p.log_g) < units) p.log_g++;
    const uint32_t G = 1u << p.log_g;
    p.tiles = (units + G - 1u) / G;
    const uint64_t target = cu_count(num_cus) * kMaxBlocksPerCu;
    const uint64_t step_rows = (uint64_t)slots(p.log_g) * batch_rows(n_columns);   // one batch of every slot
    uint64_t s;
    if (slices_per_tile > 0) {
        s = (uint64_t)slices_per_tile;
    } else {
        s = std::max<uint64_t>(1u, target / p.tiles);
        s = std::min<uint64_t>(s, std::max<uint64_t>(1u, n_variants / kMinSliceRows));
    }
    s = std::min<uint64_t>(s, std::max<uint64_t>(1u, (n_variants + step_rows - 1u) / step_rows));
    p.slices = (uint32_t)std::min<uint64_t>(s, 0x7FFFFFFFull / p.tiles);
    return p;
}

}  // namespace score

// ---- gt_vsum: per-variant sums -----------------------------------------------------------------------------------------------------
namespace vsum {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBlocksPerCu = 8;
constexpr uint32_t kTileBytes = 32;       // record bytes (MFMA steps) of a tile: 128 samples, 32 A registers (64 VGPRs) per lane
constexpr uint32_t kGroupRows = 4;        // rows of one MFMA
constexpr uint32_t kMinSliceRows = 256;   // rows a slice takes at least when the plan is not forced: a block's A load is worth that many rows

// groups of kGroupRows rows; a slice is a range of groups (slice_rows over the groups)
PGENHIP_PLAN_HD constexpr uint64_t groups(uint64_t n_variants) { return (n_variants + kGroupRows - 1u) / kGroupRows; }

// MFMA: tiles of one row meet in atomics (the caller zeroes the sums first) when a row has more than one
PGENHIP_PLAN_HD constexpr bool mfma_atomic(uint32_t record_size) { return record_size > kTileBytes; }

struct MfmaPlan {
    uint32_t tiles, slices, grid;
};

// blocks: forced grid size, which also forces the slices (0 = by shape)
PGENHIP_PLAN_HD inline MfmaPlan mfma_plan(uint32_t record_size, uint32_t n_variants, int num_cus, int blocks)
{
    MfmaPlan p{};
    p.tiles = (record_size + kTileBytes - 1u) / kTileBytes;
    const uint64_t target = cu_count(num_cus) * kBlocksPerCu;
    uint64_t s;
    if (blocks > 0) {
        s = (uint64_t)blocks;
    } else {
        s = std::max<uint64_t>(1u, target / p.tiles);
        s = std::min<uint64_t>(s, std::max<uint64_t>(1u, n_variants / kMinSliceRows));
    }
    s = std::min<uint64_t>(s, (groups(n_variants) + kWaves - 1u) / kWaves);   // at least one group per wave
    p.slices = (uint32_t)std::min<uint64_t>(s, 0x7FFFFFFFull / p.tiles);
    const uint64_t items = (uint64_t)p.tiles * p.slices;
    p.grid = (uint32_t)std::min<uint64_t>(items, blocks > 0 ? (uint64_t)blocks : target);
    return p;
}

// GENERAL: a wave per (row, column), the rest by grid stride
PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_variants, uint32_t n_columns, int num_cus, int blocks)
{
    return grid_blocks(((uint64_t)n_variants * n_columns + kWaves - 1u) / kWaves, kBlocksPerCu, num_cus, blocks);
}

}  // namespace vsum

// ---- gt_matrix: numeric genotype matrix --------------------------------------------------------------------------------------------
namespace matrix {

constexpr int kThreads = 256;
constexpr uint32_t kBlocksPerCu = 8;         // grid cap of the grid-stride kernels
constexpr uint32_t kLongRowBytes = 4096;     // STREAM: output rows from this size take the division-free rows kernel
constexpr uint32_t kTileVariants = 128;      // TILE: rows of a block's tile (16 per lane x 8 lanes)
constexpr uint32_t kWaveSamples = 128;       // TILE: samples of one wave (16 per lane x 8 lanes)
constexpr uint32_t kTileSamples = 512;       // TILE: samples of a block's tile = 128 record bytes, one line per row
constexpr uint32_t kTileBlocksPerCu = 4;     // TILE: grid cap (16 KiB of LDS per block)

enum Shape : uint32_t { kGeneral = 1u, kStream = 2u, kTile = 3u };   // the values of PGENHIP_MATRIX_GENERAL / _STREAM / _TILE

// STREAM: variant-major, all samples kept
PGENHIP_PLAN_HD constexpr bool stream_applicable(bool all_kept, bool sample_major) { return all_kept && !sample_major; }

// TILE: sample-major, all samples kept, out and out_stride multiples of 16 (one output row: the stride is not used)
PGENHIP_PLAN_HD constexpr bool tile_applicable(bool all_kept, bool sample_major, uint32_t out_align, uint64_t out_stride, uint32_t kept_count)
{
    return all_kept && sample_major && out_align == 0u && (out_stride % 16u == 0u || kept_count <= 1u);
}

// what AUTO launches; out_align = out & 15
PGENHIP_PLAN_HD constexpr Shape auto_shape(bool all_kept, bool sample_major, uint32_t out_align, uint64_t out_stride, uint32_t kept_count)
{
    return stream_applicable(all_kept, sample_major)                                   ? kStream
           : tile_applicable(all_kept, sample_major, out_align, out_stride, kept_count) ? kTile
                                                                                        : kGeneral;
}

PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_variants, uint32_t kept_count, int num_cus, int blocks)
{
    return grid_blocks(((uint64_t)n_variants * kept_count + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
}

struct StreamPlan {
    bool dense;         // the whole matrix is one span of bytes (else every row is a span of its own)
    bool long_rows;     // the rows kernel: grid_x blocks along a row's chunks, grid_y along the rows
    uint64_t per_row;   // aligned chunks a row can touch at any phase
    uint64_t total;     // chunks (lanes' work items) of the launch
    uint32_t grid_x, grid_y;
};

PGENHIP_PLAN_HD inline StreamPlan stream_plan(uint32_t n_variants, uint32_t kept_count, uint32_t elem_bytes, uint32_t out_align, uint64_t out_stride,
                                              int num_cus, int blocks)
{
    StreamPlan p{};
    const uint64_t row_bytes = (uint64_t)kept_count * elem_bytes;
    p.dense = n_variants == 1u || out_stride == row_bytes;
    p.per_row = (row_bytes + 15u) / 16u + 1u;
    p.total = p.dense ? (out_align + row_bytes * n_variants + 15u) / 16u : p.per_row * n_variants;
    p.long_rows = row_bytes >= kLongRowBytes;
    if (p.long_rows) {
        p.grid_x = grid_blocks((p.per_row + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks > 0 ? 1 : 0);
        const uint32_t gy = (uint32_t)std::min<uint64_t>(n_variants, std::max<uint32_t>(1u, grid_blocks(~0ull, kBlocksPerCu, num_cus, blocks) / p.grid_x));
        p.grid_y = std::min<uint32_t>(gy, 65535u);
    } else {
        p.grid_x = grid_blocks((p.total + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
        p.grid_y = 1u;
    }
    return p;
}

struct TilePlan {
    uint64_t v_tiles, bands, total;   // a launch walks bands x variant tiles, variant tile fastest
    uint32_t grid;
};

PGENHIP_PLAN_HD inline TilePlan tile_plan(uint32_t n_variants, uint32_t sample_count, int num_cus, int blocks)
{
    TilePlan p{};
    p.v_tiles = ((uint64_t)n_variants + kTileVariants - 1u) / kTileVariants;
    p.bands = ((uint64_t)sample_count + kTileSamples - 1u) / kTileSamples;
    p.total = p.v_tiles * p.bands;
    p.grid = grid_blocks(p.total, kTileBlocksPerCu, num_cus, blocks);
    return p;
}

}  // namespace matrix

// ---- gt_pair: windowed pairwise tables ---------------------------------------------------------------------------------------------
namespace pair {

constexpr int kThreads = 64;                            // one wave per tile
constexpr uint32_t kTile = 16;                          // TL = TR
constexpr uint32_t kChunkWords = 16;                    // 32-sample words per staged chunk: 512 samples, 128 record bytes per row
constexpr uint32_t kBlocksPerCu = 16;

struct Plan {
    uint64_t w_eff, tiles_per_left, n_items;
    uint32_t grid;
};

// n_left >= 1, n_variants >= 2; blocks: forced grid size (0 = by shape)
PGENHIP_PLAN_HD inline Plan plan(uint32_t n_variants, uint32_t n_left, uint32_t window, int num_cus, int blocks)
{
    Plan p{};
    const uint64_t V = n_variants;
    p.w_eff = window < V - 1 ? window : V - 1;
    const uint64_t left_tiles = ((uint64_t)n_left + kTile - 1u) / kTile, right_tiles = (V + kTile - 1u) / kTile;
    p.tiles_per_left = (kTile - 1u + p.w_eff) / kTile + 1u;   // the right tiles rows i0 .. i0 + 15 reach with d <= W, the diagonal one included
    if (p.tiles_per_left > right_tiles) p.tiles_per_left = right_tiles;
    p.n_items = left_tiles * p.tiles_per_left;
    p.grid = blocks > 0 ? (uint32_t)blocks : grid_blocks(p.n_items, kBlocksPerCu, num_cus, 0);
    return p;
}

}  // namespace pair

// ---- gt_pack: packed records -------------------------------------------------------------------------------------------------------
namespace pack {

constexpr int kThreads = 256;
constexpr uint32_t kBlocksPerCu = 8;       // grid cap of the grid-stride kernels
constexpr uint32_t kPartChunks = 256u;     // DENSE, wave per row: chunks of one part (4 passes of 64 lanes)
constexpr uint32_t kStreamRunBytes = 65536u;   // DENSE, dense rows as one stream: bytes of a run of rows (16 parts)

PGENHIP_PLAN_HD constexpr bool dense_applicable(bool has_kept_list, uint32_t kept_count, uint32_t sample_count) { return !has_kept_list && kept_count == sample_count; }
PGENHIP_PLAN_HD constexpr bool gather_applicable(bool has_kept_list, uint32_t kept_count) { return has_kept_list && kept_count >= 1u; }

PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_variants, uint32_t kept_count, int num_cus, int blocks)
{
    return grid_blocks(((uint64_t)n_variants * ((kept_count + 3u) >> 2) + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
}

struct GatherPlan {
    uint32_t Q;       // output dwords of a row
    uint64_t total;   // lanes' work items
    uint32_t grid;
};
PGENHIP_PLAN_HD inline GatherPlan gather_plan(uint32_t n_variants, uint32_t kept_count, int num_cus, int blocks)
{
    GatherPlan p{};
    p.Q = (kept_count + 15u) >> 4;
    p.total = (uint64_t)n_variants * p.Q;
    p.grid = grid_blocks((p.total + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
    return p;
}

struct DensePlan {
    uint32_t G, P;    // lanes per row, passes per work item
    uint32_t parts;   // work items of a row
    uint64_t items;
    uint32_t grid;
};
// lanes per row: as many as three passes over the row's chunks need; from 97 chunks a wave per row, cut into parts
PGENHIP_PLAN_HD inline DensePlan dense_plan(uint32_t record_size, uint32_t n_variants, int num_cus, int blocks)
{
    DensePlan p{};
    const uint32_t chunks = (record_size + 30u) / 16u;   // the most aligned chunks a destination row can touch
    p.G = chunks <= 12u ? 4u : chunks <= 24u ? 8u : chunks <= 48u ? 16u : chunks <= 96u ? 32u : 64u;
    p.P = p.G == 64u ? kPartChunks / 64u : 3u;
    p.parts = (chunks + p.G * p.P - 1u) / (p.G * p.P);
    const uint64_t row_groups = ((uint64_t)n_variants + 64u / p.G - 1u) / (64u / p.G);
    p.items = row_groups * p.parts;
    p.grid = grid_blocks((p.items + kThreads / 64 - 1u) / (kThreads / 64), kBlocksPerCu, num_cus, blocks);
    return p;
}

// Dense records into dense output with no pad bits (N a multiple of 4) are one byte stream: runs of run_rows rows go as ONE row
PGENHIP_PLAN_HD inline uint64_t run_rows(uint32_t record_size) { return kStreamRunBytes / record_size; }
PGENHIP_PLAN_HD inline bool merge_runs(bool gathered, uint32_t sample_count, uint32_t record_size, uint64_t record_stride, uint64_t out_stride, uint32_t n_variants)
{
    const uint64_t m = run_rows(record_size);
    return !gathered && (sample_count & 3u) == 0u && record_stride == record_size && out_stride == record_size && m >= 2u && n_variants >= 2u * m;
}

}  // namespace pack

// ---- gt_spair, gt_gram: pairs of samples summed over rows --------------------------------------------------------------------------
namespace sample_pairs {

constexpr int kThreads = 256;              // lanes of a block; GENERAL owns one pair per lane
constexpr uint32_t kTile = 64;             // ranks of a block tile, per operand
constexpr uint32_t kMaxGridTiles = 1u << 20;   // tiles (pair blocks) side by side in the grid; a block strides over the rest
constexpr uint32_t kMaxGridBlocks = 1u << 22;
constexpr uint32_t kMinSliceRows = 256;    // rows a slice takes at least when the plan is not forced
constexpr uint32_t kGeneralBlocksPerCu = 8;
constexpr uint32_t kMfmaBlocksPerCu = 2;   // what the MFMA kernels are compiled for

// row ranges of a launch: forced, or as many as bring the grid to the chip's resident blocks, of at least kMinSliceRows rows each;
// never more than there are units of `unit_rows` rows (so no slice is empty), the grid stays below kMaxGridBlocks, and never fewer
// than min_slices
PGENHIP_PLAN_HD inline uint32_t pair_slices(uint32_t n_variants, uint64_t grid_items, int forced, int num_cus, uint32_t blocks_per_cu, uint32_t unit_rows,
                                            uint64_t min_slices)
{
    const uint64_t target = cu_count(num_cus) * blocks_per_cu;
    uint64_t s;
    if (forced > 0) {
        s = (uint64_t)forced;
    } else {
        s = std::max<uint64_t>(1u, target / grid_items);
        s = std::min<uint64_t>(s, std::max<uint64_t>(1u, n_variants / kMinSliceRows));
    }
    s = std::min<uint64_t>(s, ((uint64_t)n_variants + unit_rows - 1u) / unit_rows);
    s = std::min<uint64_t>(s, kMaxGridBlocks / grid_items);
    return (uint32_t)std::max<uint64_t>(s, min_slices);
}

// MFMA: tiles of kTile x kTile ranks
PGENHIP_PLAN_HD constexpr uint32_t range_tiles(uint32_t count) { return (count + kTile - 1u) / kTile; }
PGENHIP_PLAN_HD constexpr uint64_t tiles(uint32_t a_count, uint32_t b_count) { return (uint64_t)range_tiles(a_count) * range_tiles(b_count); }
PGENHIP_PLAN_HD inline uint32_t grid_tiles(uint32_t a_count, uint32_t b_count) { return (uint32_t)std::min<uint64_t>(tiles(a_count, b_count), kMaxGridTiles); }

// GENERAL: blocks of kThreads pairs
PGENHIP_PLAN_HD constexpr uint64_t pair_blocks(uint32_t a_count, uint32_t b_count) { return ((uint64_t)a_count * b_count + kThreads - 1u) / kThreads; }
PGENHIP_PLAN_HD inline uint32_t grid_pairs(uint32_t a_count, uint32_t b_count) { return (uint32_t)std::min<uint64_t>(pair_blocks(a_count, b_count), kMaxGridTiles); }

}  // namespace sample_pairs

namespace spair {

using namespace sample_pairs;
constexpr uint32_t kStepRows = 64;         // rows of one MFMA step (the instruction's k)

// a slice stays below 2^31 rows, so an i32 accumulator stays below its sign bit
PGENHIP_PLAN_HD constexpr uint64_t min_slices(uint32_t n_variants) { return ((uint64_t)n_variants >> 30) + 1u; }

PGENHIP_PLAN_HD inline uint32_t general_slices(uint32_t n_variants, uint32_t a_count, uint32_t b_count, int forced, int num_cus)
{
    return pair_slices(n_variants, grid_pairs(a_count, b_count), forced, num_cus, kGeneralBlocksPerCu, 1u, min_slices(n_variants));
}
PGENHIP_PLAN_HD inline uint32_t mfma_slices(uint32_t n_variants, uint32_t a_count, uint32_t b_count, int forced, int num_cus)
{
    return pair_slices(n_variants, grid_tiles(a_count, b_count), forced, num_cus, kMfmaBlocksPerCu, kStepRows, min_slices(n_variants));
}

}  // namespace spair

namespace gram {

using namespace sample_pairs;
constexpr uint32_t kStepRows = 32;         // rows expanded per step: eight MFMA row groups
constexpr uint32_t kGroupRows = 4;         // rows of one MFMA (the instruction's k)

PGENHIP_PLAN_HD inline uint32_t general_slices(uint32_t n_variants, uint32_t a_count, uint32_t b_count, int forced, int num_cus)
{
    return pair_slices(n_variants, grid_pairs(a_count, b_count), forced, num_cus, kGeneralBlocksPerCu, 1u, 1u);
}
PGENHIP_PLAN_HD inline uint32_t mfma_slices(uint32_t n_variants, uint32_t a_count, uint32_t b_count, int forced, int num_cus)
{
    return pair_slices(n_variants, grid_tiles(a_count, b_count), forced, num_cus, kMfmaBlocksPerCu, kStepRows, 1u);
}

}  // namespace gram

// ---- gt_gapply: Z^T (Z Q) in two passes ----------------------------------------------------------------------------------------------
namespace gapply {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kGroup = 4;               // the k of one v_mfma_f64_16x16x4_f64: samples in the P pass, rows in the Y pass
constexpr uint32_t kRowTile = 64;            // P pass, MFMA: rows of a block (16 per wave), which share every staged tile of Q
constexpr uint32_t kStepSamples = 64;        // P pass: samples of one staged tile of Q; also the unit sample slices are cut in
constexpr uint32_t kSampleTile = 256;        // Y pass, MFMA: samples of a block (64 per wave)
constexpr uint32_t kStepRows = 64;           // Y pass, MFMA: rows of one staged tile of P (and of their tables)
constexpr uint32_t kMinSliceSamples = 4096;  // samples a P-pass slice takes at least when the plan is not forced
constexpr uint32_t kMinSliceRows = 256;      // rows a Y-pass slice takes at least when the plan is not forced
constexpr uint32_t kMaxGridTiles = 1u << 20;   // tiles side by side in the grid; a block strides over the rest
constexpr uint32_t kMaxGridBlocks = 1u << 22;
constexpr uint32_t kGeneralBlocksPerCu = 8;
constexpr uint32_t kMfmaBlocksPerCu = 2;

// ranges the reduction dimension of a pass is cut into: forced, or as many as bring the grid to the chip's resident blocks, of at
// least min_slice each; never more than there are units (so no range is empty), and the grid stays below kMaxGridBlocks
PGENHIP_PLAN_HD inline uint32_t cut(uint64_t extent, uint32_t unit, uint32_t min_slice, uint64_t grid_tiles, int forced, int num_cus, uint32_t per_cu)
{
    const uint64_t target = cu_count(num_cus) * per_cu;
    uint64_t s;
    if (forced > 0) {
        s = (uint64_t)forced;
    } else {
        s = std::max<uint64_t>(1u, target / grid_tiles);
        s = std::min<uint64_t>(s, std::max<uint64_t>(1u, extent / min_slice));
    }
    s = std::min<uint64_t>(s, (extent + unit - 1u) / unit);
    s = std::min<uint64_t>(s, kMaxGridBlocks / grid_tiles);
    return (uint32_t)std::max<uint64_t>(s, 1u);
}

// samples [begin, end) of slice `slice` of the P pass: whole units of kStepSamples, the last one ends at K
PGENHIP_PLAN_HD inline RowRange slice_samples(uint64_t K, uint32_t slice, uint32_t slices)
{
    const RowRange u = slice_rows((K + kStepSamples - 1u) / kStepSamples, slice, slices);
    return {u.begin * kStepSamples, std::min<uint64_t>(u.end * kStepSamples, K)};
}

struct Plan {
    uint64_t p_tiles, y_tiles;         // P pass: row tiles (MFMA) or blocks of (row, column) waves (GENERAL); Y pass: sample tiles or entry blocks
    uint32_t p_grid, y_grid;           // tiles side by side in the grid
    uint32_t sample_slices, row_slices;   // the grids are p_grid * sample_slices and y_grid * row_slices blocks
};

// n_variants, kept_count, n_columns >= 1
PGENHIP_PLAN_HD inline Plan plan(uint32_t n_variants, uint32_t kept_count, uint32_t n_columns, bool mfma, int forced_sample_slices, int forced_row_slices,
                                 int num_cus)
{
    Plan p{};
    const uint64_t V = n_variants, K = kept_count, C = n_columns;
    p.p_tiles = mfma ? (V + kRowTile - 1u) / kRowTile : (V * C + kWaves - 1u) / kWaves;
    p.y_tiles = mfma ? (K + kSampleTile - 1u) / kSampleTile : (K * C + kThreads - 1u) / kThreads;
    p.p_grid = (uint32_t)std::min<uint64_t>(p.p_tiles, kMaxGridTiles);
    p.y_grid = (uint32_t)std::min<uint64_t>(p.y_tiles, kMaxGridTiles);
    const uint32_t per_cu = mfma ? kMfmaBlocksPerCu : kGeneralBlocksPerCu;
    p.sample_slices = cut(K, kStepSamples, kMinSliceSamples, p.p_grid, forced_sample_slices, num_cus, per_cu);
    p.row_slices = cut(V, mfma ? kStepRows : 1u, kMinSliceRows, p.y_grid, forced_row_slices, num_cus, per_cu);
    return p;
}

}  // namespace gapply

// ---- gt_wide: the work-queue stream kernel (row items, LINES, RUNS) -------------------------------------------------------------------
namespace wide {

constexpr int kThreads = 512;              // 1 loader wave + kStorers storer waves
constexpr uint32_t kStorers = 7;           // items of one step of a block
constexpr uint32_t kSpanChunks = 1024;     // 16-byte chunks of one work item: 16 stores x 64 lanes
constexpr uint64_t kShortLaunchBytes = 1000000000ull;     // text per launch up to which a launch counts as short (two blocks per CU, nt stores)
constexpr uint64_t kWtOneSpanMaxBytes = 4500000000ull;    // rows of one span: text per launch up to which write-through stores are ahead (crossover between 3.8 and 5.6 GB)
constexpr uint64_t kBurstOneMinBytes = 9000000000ull;     // rows of several spans: text per launch from which single store steps are ahead of bursts of two (crossover between 6 and 12 GB)
constexpr uint64_t kRunsLongBytes = 3000000000ull;        // RUNS: text per launch above which the launch takes every resident block and eight write fronts (ahead from 1.9 GB, behind at 0.9 GB)
constexpr uint32_t kFrontSteps = 64;       // rows of several spans take eight write fronts from this many steps per block
constexpr uint32_t kStoreNt = 1, kStoreWt = 2;   // the values of PGENHIP_KNOB_STORE_POLICY: nt, nt sc1 (write-through)

// spans (work items) of a row of row_bytes of text: a row owns floor(S/16) or ceil(S/16) chunks (one more for row 0 with an unaligned
// pointer), and its first span starts up to 63 chunks before them (1-KiB-aligned span grid)
PGENHIP_PLAN_HD constexpr uint32_t spans_per_row(uint64_t row_bytes) { return (uint32_t)(((row_bytes + 15u) / 16u + 1u + 63u + kSpanChunks - 1u) / kSpanChunks); }

// steps a launch of n_items items needs: every step of a block takes kStorers items
PGENHIP_PLAN_HD constexpr uint64_t steps(uint64_t n_items) { return (n_items + kStorers - 1u) / kStorers; }

struct Rule {
    uint32_t policy;          // kStoreNt or kStoreWt
    uint32_t burst;           // plain store steps issued back to back
    uint32_t blocks_per_cu;
    uint32_t fronts;          // work-queue ranges = write fronts of the launch
    uint32_t grid;            // blocks
};

// The kernel a launch runs (store policy, burst): the part of the rule that does not need that kernel's occupancy figure.
// text_bytes: GT text of the launch (full lines: without their prefixes); runs: the RUNS mode (short rows, several rows per item).
//
// Store policy (profiles/r04_short_launches.md, both policies interleaved in one process, two boxes).  Write-through (nt sc1)
// stores are ahead on LONG launches of rows of several spans — N = 500 000: 12 GB -2.4 / -3.4 %, the 212-GB launch of BASELINE
// configs[2] 33.90 -> 32.56 ms (-3.9 %), N = 5 000 / 20 000 / 100 000 at 12 GB -1.4 / -1.9 / -2.2 % — and on rows of one span in the
// middle sizes (N = 2 504: 1 GB -1.9 %, 2 GB -2.0 / -2.2 %, 3.8 GB of text -2.1 %); they are BEHIND on rows of one span from 5.6 GB of
// text (+1.3 %, 8 GB +1.2 %, the 11.7-GB chr22 block +1.3 % on both boxes) and level on short launches (134 MB +0.9 %, the 0.5-GB
// second pass of the two passes +0.3 %: no end-of-kernel flush worth having shows at any size).  The rule takes write-through where
// it measured ahead by more than the spread: above the short-launch size of the blocks-per-CU rule below, rows of several
// spans at any size, rows of one span up to kWtOneSpanMaxBytes.  (Full lines through this kernel follow the same rule by the
// size of their GT text: the same stores behind a prefix each; not measured separately.)
// RUNS: nt; write-through measured level on these launches (N = 300: 134 MB -2.3 % inside a spread of 9 %, 255 MB -0.6 / -1.1 %,
// 1 GB level), so only the knob selects it.
// The joint grid of profiles/r05_stream_rule.md (policy x fronts x blocks per CU x burst in one process) confirms every branch above
// on its own axis: no other policy is ahead of the rule's beyond the spread on any of its ten shapes.
//
// Burst: 2 (text of both steps first, then both stores); 1 / 4 / 8 lost under nt on the chr22 block (profiles/r01_kernel_sweeps.md).
// Rows of several spans from kBurstOneMinBytes: 1 (profiles/r05_stream_rule.md, all bursts interleaved under the rule's other choices) —
// the 212-GB launch of BASELINE configs[2] 32 754 -> 32 389 us (-1.1 %, spread 0.3 %), 12 GB of N = 20 000 / 100 000 / 500 000
// -0.8 / -0.8 / -0.4 % (spreads 0.1-0.2 %), and under forced nt stores by more (-2.8 % at 212 GB); BEHIND below that: 6 / 3 / 1.5 GB
// of N = 20 000 +0.8 / +2.0 / +1.5 %, 2 GB of N = 4 940 +1.8 %, the 0.5-GB second pass of the two passes +4.8 %, and on rows of one
// span at every size (N = 2 504: 2 / 4 GB +2.0 / +2.2 %, the chr22 block +1.4 %).  Bursts of 4 were within 0.6 % of 2 everywhere,
// on either side (-0.5 % at 6 and 12 GB of long rows, +0.6 % at 2 GB of N = 4 940): not taken, and not instantiated.
PGENHIP_PLAN_HD inline Rule kernel_choice(uint64_t text_bytes, uint32_t spans, bool runs, int forced_policy, int forced_burst)
{
    Rule r{};
    const bool wt_rule = !runs && text_bytes > kShortLaunchBytes && (spans > 1u || text_bytes <= kWtOneSpanMaxBytes);
    r.policy = forced_policy == 0 ? (wt_rule ? kStoreWt : kStoreNt) : (forced_policy == (int)kStoreWt ? kStoreWt : kStoreNt);
    r.burst = forced_burst > 0 ? (uint32_t)forced_burst : (!runs && spans > 1u && text_bytes >= kBurstOneMinBytes ? 1u : 2u);   // (RUNS has no burst: 2 by convention)
    return r;
}

// The whole launch decision.  steps_needed: steps(n_items); occupancy: resident blocks per CU of kernel_choice's kernel, as the
// occupancy API says (>= 1; RUNS: 3); forced_*: the knobs (0 = by rule).
//
// Blocks per CU.  Long launches run exactly what is resident (62 VGPRs -> 8 waves/SIMD -> four 512-thread blocks per CU; 25 KB of
// LDS each): blocks beyond that would only start when the queue is already empty.  Interleaved A/B on the chr22 block: 2 blocks/CU
// 2.12 ms, 4 blocks/CU 2.00 ms (profiles/r01_kernel_sweeps.md).  SHORT launches (up to ~1 GB of text: a CLI block, a chunk of the two
// passes) run faster with two blocks per CU (round 3, profiles/r03_kernel_sweeps.md §6).  On a re-used output buffer (what the CLI
// does) the advantage is large and holds up to ~4.5 GB (N = 2 504: 134 MB 0.51 against 0.45 of roofline, 2.2 GB 0.77 / 0.71, 6 GB
// 0.69 / 0.73); on FRESH output regions (one call cut into pieces of that size, tools/split_probe.py) it is small and ends earlier:
// 134 MB 0.457 / 0.442, 0.5 GB level (K = 4 940: 0.584 / 0.569), 2 GB 0.613 / 0.642 — so the rule takes the size both agree on.
// RUNS: two, not the three the occupancy API allows (45 KB of LDS each): level on 11-GB launches (N = 100 / 300 / 1 000 / 1 900:
// 0.686 / 0.680 / 0.698 / 0.707 against 0.683 / 0.681 / 0.703 / 0.690) and 8-9 % ahead on the 255-MB launch of the reference's own
// dataset shape (0.505 against 0.469), whose blocks run only three steps each (round 3: on one box three were ahead again from
// ~5.5 GB of re-used output — 6.4 M rows of N = 300: 0.73 against 0.69 — which round 2's boxes did not show).  With EIGHT write fronts
// the three are ahead on every long launch (profiles/r05_stream_rule.md, N = 300: 1.9 / 3.8 / 6.6 / 10.4 GB of text -4.9 / -7.2 / -5.8 / -5.6 %,
// N = 100 / 1 000 at 11 GB -5.4 / -5.0 %; with two fronts only -0.7 .. -3.5 % at 7-11 GB) and behind on short ones (0.9 GB +5.1 %, 0.5 GB
// +6.4 %, 255 MB +3.7 %): the occupancy figure above kRunsLongBytes, on the far side of the one size (1.9 GB, re-used output) that
// the fresh-region effect above could still reach.
//
// Write fronts.  Rows of several spans on a launch of >= kFrontSteps steps per block: 8 — on the 212-GB launch of BASELINE
// configs[2] two fronts ran at 0.73 or 0.78 of roofline depending on where the driver had put the buffer (stable per allocation,
// 5-7 % apart), eight at 0.784 on every box; 0.765 -> 0.784 on the 266-GB shard of configs[3]; +0.4-2.4 % on 12-GB launches of
// N = 5 000 .. 100 000.  Rows of one span (the chr22 shape): 2 — four or eight were level on one box and 1.6-2.4 % behind on another
// (interleaved in one process, chr22 block: 8 ranges 2.058 ms, 4: 2.045, 2: 2.038, 1: 2.039); short launches (the 0.8-GB second pass
// of the two-pass path: 15 steps per block): 2 — eight cost 9 % there (profiles/r02_kernel_sweeps.md).  RUNS: 2 (1 .. 64 measured level
// with two blocks per CU); 8 above kRunsLongBytes, where they are what makes the third block per CU pay (above).
// The joint grid of profiles/r05_stream_rule.md leaves the rest as it was: on the chr22 block four or eight fronts are 2.2-2.6 % AHEAD
// on one output allocation and 0.4-1.9 % BEHIND on three others of the same process, under either policy and any burst (no arm closes
// that placement spread); rows of several spans keep 8 fronts and the occupancy figure (4 / 16 fronts, 3 blocks: within 0.4 %).
PGENHIP_PLAN_HD inline Rule rule(uint64_t text_bytes, uint32_t spans, bool runs, uint64_t steps_needed, int occupancy, int num_cus, int forced_policy,
                                 int forced_blocks_per_cu, int forced_fronts, int forced_burst)
{
    Rule r = kernel_choice(text_bytes, spans, runs, forced_policy, forced_burst);
    const bool runs_long = runs && text_bytes > kRunsLongBytes;
    int per_cu = runs && !runs_long ? 2 : std::max(occupancy, 1);   // (short RUNS launches: two whatever the occupancy figure, as ever)
    if (!runs && text_bytes <= kShortLaunchBytes && per_cu > 2) per_cu = 2;
    if (forced_blocks_per_cu > 0) per_cu = forced_blocks_per_cu;
    r.blocks_per_cu = (uint32_t)per_cu;
    r.grid = grid_blocks(steps_needed, r.blocks_per_cu, num_cus, 0);
    r.fronts = forced_fronts > 0 ? (uint32_t)forced_fronts : (runs ? runs_long : spans > 1u && steps_needed >= (uint64_t)kFrontSteps * r.grid) ? 8u : 2u;
    return r;
}

}  // namespace wide

// ---- the emit path: what pgenhip_decode_emit / _at / pgenhip_emit_lines run, and the launch plans of its kernels ----------------------
namespace emit {

// ---- constants (kernels.h and the .hip files take them from here)
constexpr uint32_t kWaves = 4;                        // waves of a block of the segment, row-owner and pick kernels (256 threads)
// Kept-subset segment kernels: the kept list is sliced by segments of this many samples (4 KiB of every record)
constexpr uint32_t kScanSegmentSamples = 16384u;
// The compact pass takes segments with at most this many kept samples (a quarter of a segment; the two-pass band is <= 4.5 %
// kept overall, so only a very clustered list has more in one segment: two_pass() then stays with the single-pass kernel)
constexpr uint32_t kCompactMaxSegCodes = 4096u;
// Two-pass path: every launch in flight has its own slice of compact-record scratch, like its own counter block (launches of one
// ctx on different streams may overlap: include/pgen_hip.h, "Streams").  A slice holds one chunk of rows between the two passes;
// a chunk stays in the 256-MiB Infinity Cache, so a smaller one costs only its two extra kernel launches.
constexpr size_t kCompactSliceBytes = 32u << 20;
// row-owner kernel (gt_rowpick.hip): the whole kept list is its LDS table; segments of a row; rows every resident wave must own under AUTO
constexpr uint32_t kRowPickMaxKept = 16384u;
constexpr uint32_t kRowPickMaxSegments = 4096u;       // N <= 64 Mi samples
constexpr uint32_t kRowPickRowsPerWave = 8u;
// RUNS and line-run modes of the stream kernel (gt_wide.hip): one 16-B-per-lane load (+ the two shared extra pieces) covers a run's
// record bytes at any alignment + 1 byte: 15 + B*R + 1 <= 66 * 16; the run's chunks (+ up to 63 of lead) fit one 1 024-chunk span:
// B*S/16 + 2 + 63 <= 1 024
constexpr uint32_t kRunLoadBytes = 1040u;
constexpr uint32_t kRunSpanBytes = 15328u;
constexpr uint32_t kLrMaxRows = 30;                   // line runs: lines per item (+ the line behind the run)
constexpr uint32_t kLrPfxBytes = 768;                 // line runs: LDS area of the prefixes of B + 1 lines
constexpr uint32_t kLrTabMaxSamples = 4096;           // line runs with a kept list: its u16 copy lives in LDS

// the pick family (gt_pick.hip)
namespace pick_family {
constexpr uint32_t kMaxSamples = 4096;          // R <= 1024: one 16-B piece per lane covers a record
constexpr uint32_t kStageBytes = 8192;          // per wave: B rows at the padded pitch (PACKED: the batch's contiguous record bytes)
constexpr int kMaxBatchRows = 12;               // load instructions per batch (one per row; PACKED: one per KiB of the batch's records)
constexpr uint32_t kMaxPackedRows = 64;         // PACKED batches: rows (their heads are prepared by lane <-> row)
constexpr uint32_t kPfxBytes = 2048;            // full lines: prefix bytes of a batch (+ the row behind it) that the stage holds
constexpr uint32_t kMaxLinesRows = 62;          // full lines: rows of a batch of gt_pick_lines_kernel
constexpr uint64_t kMaxLinesPrefix = 993;       // full lines: the longest prefix gt_pick_lines_kernel's seams take
}  // namespace pick_family

// ---- the shape of a call: everything the emit path decides from (kernels.h fills it from an EmitArgs: emit_shape)
struct Shape {
    uint32_t N, K, R, V;       // samples, kept samples, record bytes, rows
    bool kept_list;            // a kept list is present (AUTO has dropped an identity list by then)
    bool lines;                // full lines (else GT segments at a pitch)
    bool gathered;             // rows by variant list or record byte offsets
    bool records_dense;        // record_stride == record_size, or V <= 1
    bool out_dense;            // GT segments: out_stride == 4K + 1, or V <= 1
    uint64_t max_line_bytes;   // full lines: bound on prefix + 4K + 1
    bool prefix_blob;          // full lines: prefix bytes are present
};

PGENHIP_PLAN_HD constexpr uint32_t row_text_bytes(uint32_t K) { return 4u * K + 1u; }
// full lines: the bound on a prefix's length
PGENHIP_PLAN_HD constexpr uint64_t max_prefix(const Shape &s) { return s.max_line_bytes - (4ull * s.K + 1ull); }
PGENHIP_PLAN_HD constexpr uint32_t n_segments(uint32_t N) { return (N + kScanSegmentSamples - 1u) / kScanSegmentSamples; }

// ---- applicability: the shapes each kernel takes (the launchers that need work-queue counters refuse a null pointer themselves)
// flat: N >= 8: a row is >= 33 bytes, so a 16-byte chunk meets at most one '\n', and R >= 2
PGENHIP_PLAN_HD constexpr bool flat(const Shape &s) { return !s.kept_list && !s.lines && s.N >= 8u && s.out_dense; }
// stream kernel, row items: rows of >= 4 KiB keep a wave's span reasonably full; R >= 16 for the clamped window reads
PGENHIP_PLAN_HD constexpr bool wide(const Shape &s) { return !s.kept_list && !s.lines && s.N >= 1024u && s.out_dense; }
// full lines through the stream kernel: all samples kept, rows of >= 4 KiB
PGENHIP_PLAN_HD constexpr bool wide_lines(const Shape &s) { return !s.kept_list && s.lines && s.N >= 1024u; }

// RUNS: rows per work item (what one wide load and one span hold; 0 from N = 3 832)
PGENHIP_PLAN_HD constexpr uint32_t run_rows(const Shape &s)
{
    if (s.R == 0u) return 0u;
    const uint32_t by_load = kRunLoadBytes / s.R, by_span = kRunSpanBytes / row_text_bytes(s.K);
    return by_load < by_span ? by_load : by_span;
}
// all samples kept, dense records AND dense text (both are then contiguous over a run of rows), rows of >= 33 bytes
// (a 16-byte chunk meets at most one '\n') and at least one whole row per item (N <= 3 831)
PGENHIP_PLAN_HD constexpr bool runs(const Shape &s)
{
    return !s.kept_list && !s.lines && !s.gathered && s.N >= 8u && s.out_dense && s.records_dense && run_rows(s) >= 1u;
}
// AUTO takes the RUNS mode where an item holds at least two rows (N <= 1 915); with one row per item it is the row-item
// kernel's work item with LDS-staged text, measured against it in profiles/r02_kernel_sweeps.md
PGENHIP_PLAN_HD constexpr bool runs_preferred(const Shape &s) { return runs(s) && run_rows(s) >= 2u; }

// line runs: lines per work item (records of one wide load, prefix bytes of the slab, one span of text)
PGENHIP_PLAN_HD inline uint32_t lineruns_rows(const Shape &s)
{
    if (s.R == 0u || s.max_line_bytes == 0ull || s.max_line_bytes > kRunSpanBytes) return 0u;
    const uint32_t prefix = (uint32_t)s.max_line_bytes - row_text_bytes(s.K);
    uint32_t b = kRunLoadBytes / s.R;                                          // one wide load of the run's records (+ 1 byte)
    if (s.kept_list && b) b--;                                                 // kept list: + the whole record behind the run
    b = std::min<uint32_t>(b, kRunSpanBytes / (uint32_t)s.max_line_bytes);     // the run's chunks (+ lead) fit one span
    b = std::min<uint32_t>(b, kLrMaxRows);
    if (prefix) b = std::min<uint32_t>(b, (kLrPfxBytes - 16u) / prefix - (((kLrPfxBytes - 16u) / prefix) ? 1u : 0u));  // prefixes of B + 1 lines
    return b;
}
// all samples, or a kept list of >= 8 samples out of <= 4 096; lines of >= 33 bytes of GT text (a 16-byte chunk meets at most one
// '\n'); dense records; at least two lines per item
PGENHIP_PLAN_HD inline bool lineruns(const Shape &s)
{
    const bool samples_ok = !s.kept_list ? s.N >= 8u : (s.N <= kLrTabMaxSamples && s.K >= 8u);
    return samples_ok && s.lines && !s.gathered && s.records_dense && lineruns_rows(s) >= 2u;
}
// line runs, phase B: lanes per seam (log2) by the launch's longest prefix + the '\n' in front of it, four bytes per lane
PGENHIP_PLAN_HD constexpr uint32_t lineruns_seam_shift(uint32_t seam_bytes)
{
    return seam_bytes <= 16u ? 2u : (seam_bytes <= 32u ? 3u : (seam_bytes <= 64u ? 4u : (seam_bytes <= 128u ? 5u : 6u)));
}

// pick family: record of one tile (16 <= R <= 1024), at least one kept sample (rows of >= 17 bytes: a 16-B chunk touches at most
// two rows; K = 1, 2, 3: up to four, built byte by byte), dense output pitch or full lines (rows then go out one by one behind
// their prefixes).  No kept list: all samples kept — the same kernel with the identity in place of the table
PGENHIP_PLAN_HD constexpr bool pick(const Shape &s) { return s.N <= pick_family::kMaxSamples && s.R >= 16u && s.K >= 1u && (s.lines || s.out_dense); }

// row owner, what its launcher takes: K <= 16 384 kept samples (the table + a compact record per wave fit the LDS with several
// blocks per CU), records of at least one 16-byte piece, at most 4 096 segments
PGENHIP_PLAN_HD constexpr bool rowpick_takes(const Shape &s)
{
    return s.kept_list && s.K <= kRowPickMaxKept && n_segments(s.N) >= 1u && n_segments(s.N) <= kRowPickMaxSegments && s.R >= 16u;
}
// ... and what AUTO requires: at least one kept sample and enough rows that every resident wave owns some
PGENHIP_PLAN_HD constexpr bool rowpick(const Shape &s, int num_cus)
{
    return rowpick_takes(s) && s.K >= 1u && (uint64_t)s.V >= (uint64_t)kRowPickRowsPerWave * (uint64_t)num_cus * kWaves;
}

// lanes per line of the prefix copy (copy_prefix_rows, gt_common.hip.h) as log2, by the launch's longest prefix (ms for 1 M lines of
// 2 504 samples with 30 / 100 / 166-byte prefixes: 8 lanes 0.055 / 0.123 / 0.217, 16 lanes 0.076 / 0.117 / 0.162, 32 lanes - / 0.136 / 0.171)
PGENHIP_PLAN_HD constexpr uint32_t prefix_copy_shift(uint64_t max_prefix_bytes) { return max_prefix_bytes <= 48ull ? 3u : 4u; }

// ---- AUTO
// What an emit call runs: one of the launchers of kernels.h, or the two passes
enum class Emit { Rows, Flat, Wide, Runs, LineRuns, Pick, Scan, RowPick, TwoPass };

// Sparse keeps on long records (BASELINE config 5: 1 % of 500 000 samples) go through TWO passes: the segment kernel writes each
// row's COMPACT record (the K kept codes packed like a mode-0x02 record of K samples: 41-byte pieces instead of 656-byte pieces of
// text per row and segment) and the all-samples kernels turn those into text with whole-line stores.  Worth it while the text is
// small against the records.  Measured band (N = 500 000, profiles/r02_kernel_sweeps.md): 0.5 % kept -2 %, 0.65 % +4 %, 1 % +15 %,
// 2 % +11 %, 4 % +7 %, 5 % level, 10 % -4 %  ->  0.6 % .. 4.5 % kept.
// (Short records, N <= 4 096, were tried through the same two passes with a COMPACT instantiation of the short-record pick
// kernel: 0.42-0.50 of roofline against the single pass's 0.52-0.63 at every density — the compaction costs more than the text
// it saves there; profiles/r02_kernel_sweeps.md.)
// pgenhip_create allocates the compact scratch for exactly these contexts.
PGENHIP_PLAN_HD constexpr bool two_pass_shape(uint32_t N, uint32_t K)
{
    return N > 4096u && K >= 8u && (uint64_t)K * 170ull >= (uint64_t)N && (uint64_t)K * 22ull <= (uint64_t)N;
}

// measured crossover (profiles/r01_kernel_sweeps.md: N = 500 000, 0.2 % kept list gather 1.13 ms vs 1.49 ms,
// 0.4 % kept 1.51 vs 1.47; round 2, with the faster segment kernel: 0.25 % 1.33 vs 1.51, 0.33 % 1.48 vs 1.52, 0.4 % 1.60 vs 1.57): below ~1/280 kept on long records the list gather touches only the kept
// samples' lines and wins; everywhere else the segment kernels do (they read each record once, wide)
PGENHIP_PLAN_HD constexpr bool very_sparse(uint32_t N, uint32_t K) { return N >= 65536u && (uint64_t)K * 280ull <= N; }

// Kept subsets on long records through the row-owner kernel WRITING TEXT (gt_rowpick.hip, one pass): the whole kept list fits its LDS
// table (K <= 16 384) and the launch has enough rows for every resident wave.  Where it is ahead of the segment kernel / the two passes
// (profiles/r03_kernel_sweeps.md §7, fraction of roofline against the previous dispatch):
//   * records of one full segment and a thin second one (16 384 < N < 24 576): the segment kernel's blocks are unbalanced there —
//     N = 16 385 with 10 / 50 % kept 0.57 / 0.55 against 0.39 / 0.38, N = 20 000 with 10 / 30 / 80 % 0.60 / 0.57 / 0.51 against 0.50 / 0.43 / 0.43;
//   * 2 % .. 20 % kept on longer records: N = 30 000 5 % 0.62 / 0.53, N = 60 000 10 % 0.60 / 0.58, N = 100 000 2 / 5 % 0.65 / 0.62 against 0.62 / 0.56,
//     N = 500 000 3.2 % 0.62 / 0.58 (level from ~20 %: N = 60 000 25 % 0.565 / 0.571; behind at 50 %).
// Below 2 % the two passes keep the sparse band (BASELINE configs[4], 1 % of 500 000: one pass reads 86 % and writes 14 % of its bytes
// everywhere at once and runs at the copy ceiling, 3-6 % behind; N = 200 000 1 %: 0.635 against 0.658).
// rowpick_on: PGENHIP_KNOB_SCAN_ROWPICK (-1 takes it nowhere).
PGENHIP_PLAN_HD constexpr bool rowpick_shape(const Shape &s, bool rowpick_on, int num_cus)
{
    if (!rowpick_on || s.N <= kScanSegmentSamples || very_sparse(s.N, s.K) || !rowpick(s, num_cus)) return false;
    if (s.N < 24576u) return true;
    return (uint64_t)s.K * 50ull >= s.N && (uint64_t)s.K * 5ull <= s.N;
}

// AUTO for all samples kept: GT segments at a pitch, or full lines.  Two chains: their sample thresholds were measured per mode.
PGENHIP_PLAN_HD inline Emit choose_all_samples(const Shape &s)
{
    if (s.lines) {
        // long rows: the work-queue stream kernel writes the GT segments in place behind their prefixes (+ a small prefix copy).
        // From N = 1 400: at N = 1 024 / 1 200 it runs at 0.45 / 0.49 of roofline against 0.48-0.51 for the two kernels below, at
        // N = 1 500 / 1 900 at 0.56 / 0.60 against 0.49-0.55 (profiles/r02_kernel_sweeps.md)
        if (wide_lines(s) && s.N >= 1400u) return Emit::Wide;
        // short rows, dense records: runs of whole lines (prefix + GT + '\n') assembled in LDS and stored as whole 128-B lines.
        // Ahead of the pick family's full-line kernel while a run holds seven lines or more (prefixes up to ~90 bytes) and N < 1 000:
        // 30-byte prefixes, N = 100 / 300 / 500: 0.41 / 0.51 / 0.53 of roofline against 0.36 / 0.44 / 0.49; with 166-byte prefixes a run
        // is three or four lines and the pick family is ahead at every N (0.37-0.52 against 0.14-0.50); from N = 1 000 it is level or
        // ahead with short prefixes too (profiles/r03_logs/lines_sweep_after.log)
        if (lineruns(s) && lineruns_rows(s) >= 7u && s.N < 1000u) return Emit::LineRuns;
        // the pick family (identity for a table): rows' interiors + batched seams (gt_pick_lines_kernel); gathered / padded records:
        // row by row (it writes the prefixes too)
        if (pick(s)) return Emit::Pick;
        return Emit::Rows;
    }
    // short rows, dense records (8 <= N <= 1915): runs of rows as one work item, text staged through LDS in 4-KiB groups
    // so that every 128-B line leaves whole: 0.68-0.71 of roofline from N = 100 to 1500 where the flat kernel had
    // 0.42-0.56, the pick kernel 0.31-0.62 and the row-item stream kernel 0.51-0.65 (profiles/r02_kernel_sweeps.md)
    if (runs_preferred(s)) return Emit::Runs;
    // short rows that are gathered or padded (no contiguous runs): batches of rows through gt_pick.hip with the identity for a
    // table, several rows per load instruction.  Gathered rows, fraction of roofline, pick / flat / row-item stream kernel:
    // N = 64 0.46 / 0.28 / -, 300 0.49 / 0.31 / -, 1 399 0.58 / 0.40 / 0.52, 1 500 0.58 / 0.40 / 0.54, 2 504 0.59 / 0.41 / 0.68
    if (pick(s) && s.N < 2000u) return Emit::Pick;
    if (wide(s)) return Emit::Wide;
    if (flat(s)) return Emit::Flat;
    return Emit::Rows;
}

// Two passes for sparse keeps on long records, chunk by chunk of as many rows as the compact scratch holds: (1) the row-owner kernel
// (chunks of many rows; else the segment kernel) compacts each row's kept codes into a K-sample record, (2) what
// choose_all_samples picks for those records turns them into text.  two_pass_on: PGENHIP_KNOB_SCAN_TWO_PASS; max_seg_count: the
// most kept samples in one segment.
// (full lines: only where the second pass is the stream kernel's LINES mode, K >= 1 024 — below that it would flush row by row)
PGENHIP_PLAN_HD constexpr bool two_pass(const Shape &s, bool two_pass_on, uint32_t max_seg_count)
{
    return two_pass_on && two_pass_shape(s.N, s.K) && s.kept_list && s.R >= 16u && max_seg_count <= kCompactMaxSegCodes &&
           (s.lines ? s.K >= 1024u : s.out_dense);
}

// AUTO for a kept subset that is not the identity: one chain for GT segments and full lines (where a kernel writes full lines it
// writes the prefixes too)
PGENHIP_PLAN_HD inline Emit choose_subset(const Shape &s, bool rowpick_on, bool two_pass_on, uint32_t max_seg_count, int num_cus)
{
    if (rowpick_shape(s, rowpick_on, num_cus)) return Emit::RowPick;
    if (two_pass(s, two_pass_on, max_seg_count) && !very_sparse(s.N, s.K)) return Emit::TwoPass;
    // full lines only (the line-run kernel takes nothing else): kept subset on VERY short dense records: runs of whole lines, picks through
    // its LDS kept table (N = 100, 30-byte prefixes, 50 / 10 % kept: 0.28 / 0.13 of roofline against 0.23 / 0.10 for the pick family's
    // full-line kernel; from N = 300 that kernel is level or ahead — N = 500: 0.48 / 0.27 against 0.39 / 0.15 — and with long prefixes
    // always: profiles/r03_logs/lines_sweep_after.log)
    if (lineruns(s) && lineruns_rows(s) >= 7u && s.N < 300u) return Emit::LineRuns;
    // short records (the 1000 Genomes shape with a sample filter): output-driven pick, any density (full lines: interiors + batched
    // seams; gathered / padded records: row by row)
    if (pick(s)) return Emit::Pick;
    if (very_sparse(s.N, s.K) || s.R < 16u) return Emit::Rows;
    // the segment kernel (full lines: each GT segment behind its prefix, the prefix kernel the rest)
    return Emit::Scan;
}

// ---- forced kernel ids (PGENHIP_KERNEL_* of include/pgen_hip.h, AUTO excepted)
// is it a kernel id of the emit entry points?
PGENHIP_PLAN_HD constexpr bool is_kernel_id(uint32_t kernel)
{
    return kernel == PGENHIP_KERNEL_AUTO || kernel == PGENHIP_KERNEL_ROWS || kernel == PGENHIP_KERNEL_FLAT || kernel == PGENHIP_KERNEL_SCAN ||
           kernel == PGENHIP_KERNEL_WIDE || kernel == PGENHIP_KERNEL_PICK || kernel == PGENHIP_KERNEL_RUNS || kernel == PGENHIP_KERNEL_ROWPICK;
}
// what a forced id runs (RUNS: the line-run kernel for full lines)
PGENHIP_PLAN_HD constexpr Emit forced(uint32_t kernel, bool lines)
{
    return kernel == PGENHIP_KERNEL_FLAT      ? Emit::Flat
           : kernel == PGENHIP_KERNEL_SCAN    ? Emit::Scan
           : kernel == PGENHIP_KERNEL_WIDE    ? Emit::Wide
           : kernel == PGENHIP_KERNEL_PICK    ? Emit::Pick
           : kernel == PGENHIP_KERNEL_RUNS    ? (lines ? Emit::LineRuns : Emit::Runs)
           : kernel == PGENHIP_KERNEL_ROWPICK ? Emit::RowPick
                                              : Emit::Rows;
}
// does a call of shape s take this id?  A forced kernel sees the ctx's kept list, an identity list included.  (ROWPICK: its launcher
// still refuses more than kRowPickMaxSegments segments)
PGENHIP_PLAN_HD inline bool accepts(uint32_t kernel, const Shape &s)
{
    switch (kernel) {
        case PGENHIP_KERNEL_AUTO:
        case PGENHIP_KERNEL_ROWS: return true;
        case PGENHIP_KERNEL_FLAT: return flat(s);
        case PGENHIP_KERNEL_SCAN: return s.kept_list && s.R >= 16u;
        case PGENHIP_KERNEL_WIDE: return s.lines ? wide_lines(s) : wide(s);
        case PGENHIP_KERNEL_PICK: return pick(s);
        case PGENHIP_KERNEL_RUNS: return s.lines ? lineruns(s) : runs(s);
        case PGENHIP_KERNEL_ROWPICK: return s.kept_list && s.R >= 16u && s.K >= 1u && s.K <= kRowPickMaxKept;
        default: return false;
    }
}

// ---- the two passes, chunk by chunk
struct Chunks {
    uint64_t rows;    // rows of a chunk (the last one may be shorter)
    bool row_owner;   // pass 1 of a full chunk is the row-owner kernel (else the segment kernel)
};
// slice_bytes: the launch's compact scratch; forced_rows: PGENHIP_KNOB_SCAN_CHUNK_ROWS (0 = as many as the slice holds); round_rows:
// rows of one resident round of the row owner's compact pass (0: it does not take the shape).  The row-owner compact pass deals
// rows to its resident waves round-robin: whole rounds per chunk
PGENHIP_PLAN_HD inline Chunks chunks(const Shape &s, uint64_t slice_bytes, int forced_rows, bool rowpick_on, uint64_t round_rows, int num_cus)
{
    Chunks c{std::max<uint64_t>(1ull, slice_bytes / ((s.K + 3u) / 4u)), false};
    if (forced_rows > 0) c.rows = std::min<uint64_t>(c.rows, (uint64_t)forced_rows);
    if (rowpick_on) {
        Shape probe = s;
        probe.V = (uint32_t)std::min<uint64_t>(c.rows, s.V);
        c.row_owner = rowpick(probe, num_cus);
        if (c.row_owner && round_rows && c.rows > round_rows && forced_rows <= 0) c.rows -= c.rows % round_rows;
    }
    return c;
}
// pass 1 of a chunk of n rows through the row owner?  (a short last chunk: the segment kernel cuts it finer)
PGENHIP_PLAN_HD constexpr bool chunk_by_row_owner(const Chunks &c, uint32_t n) { return c.row_owner && (uint64_t)n * 2ull >= c.rows; }

// ---- launch plan of the segment kernels (gt_scan.hip): text, or the compact pass
struct ScanPlan {
    uint32_t n_seg;        // segments of a row (at least 1)
    uint32_t per_cu;       // blocks per CU planned for
    uint32_t groups;       // row groups: blocks per segment
    uint32_t xcd_groups;   // row groups under the XCD-aware block map (0: plain map)
    uint32_t bands;
    uint32_t grid;
};
// occupancy: resident blocks per CU of the kernel as the occupancy API says (>= 1); forced_per_cu: PGENHIP_KNOB_SCAN_BLOCKS_PER_CU.
// Every block walks the same number of rows, so the launch must be exactly ONE resident round: a grid that exceeds residency by a few
// blocks runs those in a second round that takes as long as the first.
// One kernel for every density (round 1's three-segment gather kernel kept a 0.8-2 % band; with the XCD-aware block map and
// two blocks per CU the pick kernel is ahead there too: 1.5 % kept 1.85 vs 1.99 ms, profiles/r02_kernel_sweeps.md).
// Blocks per CU: the occupancy API says 3 (32 KiB table + 16 KiB of stages); from ~0.6 % kept upwards 2 measure the same or
// better (+5-9 % at 1-3 % kept, level from 30 %), below that 3 do (the kernel is then a pure record reader).  Compact pass: two
// blocks per CU (3: -1 %, 5: -6 %).
PGENHIP_PLAN_HD inline ScanPlan scan_plan(uint32_t N, uint32_t K, uint32_t V, bool compact, int occupancy, int forced_per_cu, bool xcd_map, int num_cus)
{
    ScanPlan p{};
    p.n_seg = n_segments(N) ? n_segments(N) : 1u;
    const uint64_t groups_needed = ((uint64_t)V + kWaves - 1ull) / kWaves;
    const int preferred = compact || (uint64_t)K * 170ull >= (uint64_t)N ? 2 : 0;
    int per_cu = std::max(occupancy, 1);
    if (preferred > 0 && preferred < per_cu) per_cu = preferred;
    if (forced_per_cu > 0) per_cu = forced_per_cu;
    p.per_cu = (uint32_t)per_cu;
    uint64_t groups = (uint64_t)(p.per_cu * (uint32_t)num_cus) / p.n_seg;   // floor: never a partial second round
    if (groups < 1ull) groups = 1ull;   // more segments than resident blocks (N > ~16 M samples): rounds are unavoidable
    if (groups > groups_needed) groups = groups_needed;
    p.groups = (uint32_t)groups;
    p.xcd_groups = xcd_map ? (uint32_t)(groups & ~7ull) : 0u;
    p.grid = (uint32_t)(groups * p.n_seg);
    // Eight bands where the text dominates the traffic (>= 10 % kept: N = 500 000, 10 % kept 0.599 -> 0.626 of roofline, 50 % 0.589 ->
    // 0.593); one front where the launch is mostly a record reader (1 % kept, compact pass: 0.634 vs 0.614 banded; 0.3 % single pass:
    // 0.741 vs 0.693) — reads like the one narrow window, writes like several fronts (profiles/r02_kernel_sweeps.md)
    const bool banded = !compact && (uint64_t)K * 10ull >= (uint64_t)N && groups % 8ull == 0ull && groups_needed >= 64ull * groups;
    p.bands = banded ? 8u : 1u;   // (every band holds the same number of row groups)
    return p;
}

// ---- launch plan of the row-owner kernel (gt_rowpick.hip)
// bytes of dynamic LDS: table (K + 8 u16, 16-B rounded) | kept-before-segment (n_seg + 1 u32, 16-B rounded) | per wave: stage + compact record
PGENHIP_PLAN_HD constexpr uint32_t rowpick_table_bytes(uint32_t K) { return (2u * (K + 8u) + 15u) & ~15u; }
PGENHIP_PLAN_HD constexpr uint32_t rowpick_rank_bytes(uint32_t n_seg) { return (4u * (n_seg + 1u) + 15u) & ~15u; }
PGENHIP_PLAN_HD constexpr uint32_t rowpick_codes_bytes(uint32_t K) { return ((K + 3u) / 4u + 16u + 15u) & ~15u; }   // + slack behind the record for the flush's fifth code
PGENHIP_PLAN_HD constexpr uint32_t rowpick_lds_bytes(uint32_t N, uint32_t K)
{
    return rowpick_table_bytes(K) + rowpick_rank_bytes(n_segments(N)) + kWaves * (kScanSegmentSamples / 4u + rowpick_codes_bytes(K));
}
struct RowPickPlan {
    uint32_t per_cu;
    uint32_t max_blocks;   // one resident round
    uint32_t grid;
};
// a shape that rowpick_takes; occupancy: resident blocks per CU with rowpick_lds_bytes of LDS, as the occupancy API says (>= 1);
// forced_per_cu: PGENHIP_KNOB_ROWPICK_BLOCKS_PER_CU (a cap).
// Two blocks per CU measure best on long records (the loads of 8 waves per CU already saturate the read path: tools/readbench.hip; 3:
// level, 5: -3 %); on records of barely more than one segment, where a row is mostly text to write, all that fit (N = 16 385 with
// 10 % kept: 0.51 / 0.57 / 0.56 of roofline at 2 / 3 / 4 per CU; N = 20 000 with 30 %: 0.52 / 0.56 / 0.57)
PGENHIP_PLAN_HD inline RowPickPlan rowpick_plan(uint32_t N, uint32_t V, bool compact, int occupancy, int forced_per_cu, int num_cus)
{
    RowPickPlan p{};
    int per_cu = std::max(occupancy, 1);
    const int want = forced_per_cu > 0 ? forced_per_cu : (!compact && N < 24576u ? 4 : 2);
    if (want < per_cu) per_cu = want;
    p.per_cu = (uint32_t)per_cu;
    p.max_blocks = p.per_cu * (uint32_t)num_cus;
    const uint64_t need = ((uint64_t)V + kWaves - 1ull) / kWaves;
    p.grid = (uint32_t)(need < p.max_blocks ? need : p.max_blocks);
    return p;
}

// ---- launch plans of the pick family (gt_pick.hip)
struct PickPlan {
    bool packed;           // dense records and no gather: the batch's records are one contiguous run (rows at pitch R, up to 64 of them)
    uint32_t pitch;        // bytes between the rows of a batch in the stage
    uint32_t batch_rows;
};
// rows per batch: ~32 KiB of text per batch (8 / 16 / 32 / 64 KiB at 50 % kept on the chr22 shape: 1.44 / 1.41 / 1.37 / 1.36 ms),
// what the stage holds, what the register buffer holds.  batch_bytes: PGENHIP_KNOB_PICK_BATCH_BYTES (<= 0: 32 768)
PGENHIP_PLAN_HD inline PickPlan pick_plan(const Shape &s, int batch_bytes)
{
    PickPlan p{};
    const uint32_t pieces = (s.R + 15u) / 16u;
    const uint32_t text = batch_bytes > 0 ? (uint32_t)batch_bytes : 32768u;
    uint32_t b = (text + row_text_bytes(s.K) - 1u) / row_text_bytes(s.K);
    b = b < 1u ? 1u : b;
    p.packed = !s.gathered && s.records_dense;
    if (p.packed) {
        p.pitch = s.R;
        if (b > pick_family::kMaxPackedRows) b = pick_family::kMaxPackedRows;
        if (b > (pick_family::kStageBytes - 16u) / p.pitch) b = (pick_family::kStageBytes - 16u) / p.pitch;  // 15 bytes of misalignment + B * R <= 8 192: >= 7 rows, <= 8 loads
    } else {
        // row-by-row loads, G rows per instruction: lanes per row = the record's pieces rounded up to a power of two
        uint32_t lpr = 1u;
        while (lpr < pieces) lpr <<= 1;
        p.pitch = lpr * 16u;
        const uint32_t rows_per_load = 64u / lpr;
        if (b > (uint32_t)pick_family::kMaxBatchRows * rows_per_load) b = (uint32_t)pick_family::kMaxBatchRows * rows_per_load;
        if (b > pick_family::kMaxPackedRows) b = pick_family::kMaxPackedRows;
        if (b > pick_family::kStageBytes / p.pitch) b = pick_family::kStageBytes / p.pitch;  // >= 8 (pitch <= 1024)
    }
    p.batch_rows = b;
    return p;
}
struct PickLinesPlan {
    bool taken;            // gt_pick_lines_kernel runs (else the row-by-row kernel)
    int32_t batch_rows;    // (below 2: not taken)
    uint32_t cps_shift;    // log2 of the chunk slots (lanes) per seam
};
// full lines of dense records: interiors + seams, every byte written once as part of a whole chunk (gt_pick_lines_kernel); row by
// row where a batch would hold fewer than two rows, or prefixes are longer than kMaxLinesPrefix bytes
PGENHIP_PLAN_HD inline int32_t pick_lines_rows(uint32_t R, uint64_t prefix, uint32_t batch_rows)
{
    uint32_t bl = batch_rows;
    if (bl > pick_family::kMaxLinesRows) bl = pick_family::kMaxLinesRows;
    if (15u + (bl + 1u) * R > pick_family::kStageBytes) bl = (pick_family::kStageBytes - 15u) / R - 1u;           // the row behind the batch comes along
    if (prefix != 0ull && (uint64_t)(bl + 1u) * prefix > pick_family::kPfxBytes - 16u) bl = (uint32_t)((pick_family::kPfxBytes - 16u) / prefix) - 1u;   // and its prefix (two 1-KiB loads from the 16-B boundary below)
    return (int32_t)bl;
}
PGENHIP_PLAN_HD constexpr uint32_t pick_cps_shift(uint64_t prefix)
{
    const uint32_t seam_chunks = (uint32_t)((prefix + 31ull) / 16ull);   // a seam is at most P + 31 bytes
    return seam_chunks <= 4u ? 2u : (seam_chunks <= 8u ? 3u : (seam_chunks <= 16u ? 4u : (seam_chunks <= 32u ? 5u : 6u)));
}
PGENHIP_PLAN_HD inline PickLinesPlan pick_lines_plan(const Shape &s, const PickPlan &pp)
{
    PickLinesPlan p{};
    if (!(s.lines && pp.packed && s.K >= 4u && s.prefix_blob)) return p;
    p.batch_rows = pick_lines_rows(s.R, max_prefix(s), pp.batch_rows);
    p.cps_shift = pick_cps_shift(max_prefix(s));
    p.taken = max_prefix(s) <= pick_family::kMaxLinesPrefix && p.batch_rows >= 2 && p.batch_rows <= (int32_t)pick_family::kMaxLinesRows;
    return p;
}

}  // namespace emit

// ---- gt_parse: GT text -> mode-0x02 records (the inverse of the emit path) ------------------------------------------------------------
namespace parse {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBlocksPerCu = 8;          // grid cap of both grid-stride kernels
// FIXED: a piece is one work item — kPieceBytes record bytes = kPieceSamples fields = kPieceText text bytes (one 16-byte load at
// any alignment; byte loads on a line's last, partial piece).  A lane takes kLanePieces of them per turn, kThreads items apart.
constexpr uint32_t kPieceBytes = 1;
constexpr uint32_t kPieceSamples = 4u * kPieceBytes;
constexpr uint32_t kPieceText = 4u * kPieceSamples;
constexpr uint32_t kLanePieces = 4;
constexpr uint32_t kBlockPieces = (uint32_t)kThreads * kLanePieces;   // items of a block per turn
// GENERAL: text bytes of one chunk of a line (kChunkLaneBytes per lane); the tab count runs on from chunk to chunk
constexpr uint32_t kChunkLaneBytes = 4;
constexpr uint32_t kChunkBytes = (uint32_t)kThreads * kChunkLaneBytes;

// FIXED: pieces of a line.  A line of no samples still has one, which only checks that the region is empty.
PGENHIP_PLAN_HD constexpr uint32_t pieces_per_line(uint32_t record_size) { return record_size == 0u ? 1u : (record_size + kPieceBytes - 1u) / kPieceBytes; }
// record bytes [begin, end) of piece p of a line of R bytes: the pieces tile [0, R) in order
PGENHIP_PLAN_HD constexpr RowRange piece_bytes(uint32_t record_size, uint32_t piece)
{
    return {std::min<uint64_t>((uint64_t)piece * kPieceBytes, record_size), std::min<uint64_t>(((uint64_t)piece + 1u) * kPieceBytes, record_size)};
}
// FIXED: the launch is flat over (line, piece): item i is piece i % P of line i / P, kBlockPieces consecutive items per block and
// turn, so a block holds kBlockPieces / P lines of short rows (rows_per_block; at least part of two when P does not divide
// kBlockPieces) and a long row spreads over ceil(P / kBlockPieces) blocks.
PGENHIP_PLAN_HD constexpr uint32_t rows_per_block(uint32_t record_size) { return std::max<uint32_t>(1u, kBlockPieces / pieces_per_line(record_size)); }
PGENHIP_PLAN_HD constexpr uint32_t blocks_per_row(uint32_t record_size) { return (pieces_per_line(record_size) + kBlockPieces - 1u) / kBlockPieces; }

struct FixedPlan {
    uint32_t pieces;   // per line
    uint64_t total;    // items of the launch
    uint32_t grid;
};
// blocks: forced grid size (0 = by shape)
PGENHIP_PLAN_HD inline FixedPlan fixed_plan(uint32_t record_size, uint32_t n_lines, int num_cus, int blocks)
{
    FixedPlan p{};
    p.pieces = pieces_per_line(record_size);
    p.total = (uint64_t)n_lines * p.pieces;
    p.grid = grid_blocks((p.total + kBlockPieces - 1u) / kBlockPieces, kBlocksPerCu, num_cus, blocks);
    return p;
}

// GENERAL: a block per line, the lines by grid stride.  One line is not split over blocks: a call with few very long lines uses
// few CUs (as pair_stats' tiles do with few rows).
PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_lines, int num_cus, int blocks) { return grid_blocks(n_lines, kBlocksPerCu, num_cus, blocks); }
// chunks a region of `bytes` text bytes takes when it starts `lead` bytes (0 .. 3) behind a 4-byte boundary
PGENHIP_PLAN_HD constexpr uint64_t general_chunks(uint64_t bytes, uint32_t lead) { return (bytes + lead + kChunkBytes - 1u) / kChunkBytes; }

// AUTO: the FIXED pass over every line, then a GENERAL pass that takes the declined lines only.  GENERAL alone, the other
// candidate, measured 6.9-14 x behind the two passes on fixed-width text (chr22 29.3 against 3.9 ms, basic2 55.9 against 3.9 ms, a
// block of configs[2] 10.2 against 1.5 ms: profiles/r14_parse/parse_bench.jsonl).
constexpr bool kAutoFixedFirst = true;

}  // namespace parse

// ---- gt_join: sample-wise join of records ----------------------------------------------------------------------------------------
namespace join {

constexpr int kThreads = 256;
constexpr uint32_t kBlocksPerCu = 8;     // grid cap of both grid-stride kernels
constexpr uint32_t kChunkBytes = 16u;    // STREAM: a lane's piece of an output row, aligned in memory (64 samples)

// GENERAL: a lane per output byte
PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_variants, uint32_t record_size, int num_cus, int blocks)
{
    return grid_blocks(((uint64_t)n_variants * record_size + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
}

// STREAM: the most aligned chunks a row of R bytes can touch, whatever its address (R = 1 at byte 15 of a chunk: one)
PGENHIP_PLAN_HD constexpr uint32_t chunks_per_row(uint32_t record_size) { return (record_size + 2u * kChunkBytes - 2u) / kChunkBytes; }
// row bytes [begin, end) under chunk c of a row whose first byte lies `mis` bytes (0 .. 15) behind a chunk boundary: the chunks
// tile [0, R) in order; the last one is empty when the row's address leaves it nothing
PGENHIP_PLAN_HD inline RowRange chunk_bytes(uint32_t record_size, uint32_t mis, uint32_t chunk)
{
    const int64_t b0 = (int64_t)kChunkBytes * chunk - mis;
    const int64_t lo = std::min<int64_t>(std::max<int64_t>(b0, 0), record_size), hi = std::max<int64_t>(lo, std::min<int64_t>(b0 + kChunkBytes, record_size));
    return {(uint64_t)lo, (uint64_t)hi};
}
// The launch is flat over (row, chunk): item i is chunk i % C of row i / C, kThreads consecutive items per block and turn, so a
// block holds kThreads / C rows of short records and a long row spreads over ceil(C / kThreads) blocks.
PGENHIP_PLAN_HD constexpr uint32_t rows_per_block(uint32_t record_size) { return std::max<uint32_t>(1u, (uint32_t)kThreads / chunks_per_row(record_size)); }
PGENHIP_PLAN_HD constexpr uint32_t blocks_per_row(uint32_t record_size) { return (chunks_per_row(record_size) + kThreads - 1u) / kThreads; }

struct StreamPlan {
    uint32_t chunks;   // per row
    uint64_t total;    // items of the launch
    uint32_t grid;
};
// blocks: forced grid size (0 = by shape)
PGENHIP_PLAN_HD inline StreamPlan stream_plan(uint32_t record_size, uint32_t n_variants, int num_cus, int blocks)
{
    StreamPlan p{};
    p.chunks = chunks_per_row(record_size);
    p.total = (uint64_t)n_variants * p.chunks;
    p.grid = grid_blocks((p.total + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
    return p;
}

// AUTO: STREAM on every shape.  It measured ahead of GENERAL in every case run (two and eight parts, flipped or not: chr22 1.9-3.0 x,
// basic2 2.3-3.8 x, a block of configs[2] 20-24 x: profiles/r15_join/join_bench.jsonl), so the rule has no edge.
PGENHIP_PLAN_HD constexpr bool auto_stream(uint32_t /*record_size*/, uint32_t /*n_variants*/, uint32_t /*n_parts*/) { return true; }

}  // namespace join

// ---- gt_prune: greedy independent set of a windowed pair mask --------------------------------------------------------------------
namespace prune {

constexpr int kThreads = 256;
constexpr uint32_t kBlocksPerCu = 8;      // grid cap of both kernels
constexpr uint32_t kChunkRows = 1024u;    // BLOCK: rows a workgroup sweeps to a fixed point at a time (one turn of its range)
constexpr uint32_t kHaloRows = 512u;      // BLOCK: rows on either side of a turn whose states are in LDS too; farther neighbours are read from memory
constexpr uint32_t kLdsRows = kChunkRows + 2u * kHaloRows;   // one state byte each

// u32 words that hold a row's `window` bits
PGENHIP_PLAN_HD constexpr uint64_t mask_words(uint32_t window) { return ((uint64_t)window + 31u) / 32u; }
// BLOCK: the rows before / behind a turn that are staged (the whole window where it fits)
PGENHIP_PLAN_HD constexpr uint32_t halo_rows(uint32_t window) { return window < kHaloRows ? window : kHaloRows; }

// GENERAL: a lane per row, grid-stride
PGENHIP_PLAN_HD inline uint32_t general_grid(uint64_t n_rows, int num_cus, int blocks)
{
    return grid_blocks((n_rows + kThreads - 1u) / kThreads, kBlocksPerCu, num_cus, blocks);
}

// BLOCK: block b owns rows [b * range_rows, min((b + 1) * range_rows, n_rows)) and walks them in turns of kChunkRows; no block is
// empty.  blocks: forced grid size (0 = by shape: a turn per block, capped per CU); a forced grid larger than the rows shrinks to them.
struct BlockPlan {
    uint64_t range_rows;
    uint32_t grid;
};
PGENHIP_PLAN_HD inline BlockPlan block_plan(uint64_t n_rows, int num_cus, int blocks)
{
    BlockPlan p{};
    const uint64_t rows = std::max<uint64_t>(n_rows, 1u);
    const uint64_t want = blocks > 0 ? std::min<uint64_t>((uint64_t)blocks, rows) : grid_blocks((rows + kChunkRows - 1u) / kChunkRows, kBlocksPerCu, num_cus, 0);
    p.range_rows = (rows + want - 1u) / want;
    p.grid = (uint32_t)((rows + p.range_rows - 1u) / p.range_rows);
    return p;
}

// AUTO: BLOCK on every shape.  On masks of synthetic rows with LD (tools/prune_bench.py: about 7 edges per row, 4 096 to 1 048 576
// rows, W = 32 and 128) it ended in 2-3 calls against GENERAL's 10-14 and in 0.60-0.72 x its time in every case run
// (profiles/r16_prune/prune_bench_resolve.jsonl), so the rule has no edge.  Edge densities of real data are unmeasured.
PGENHIP_PLAN_HD constexpr bool auto_block(uint64_t /*n_rows*/, uint32_t /*window*/) { return true; }

}  // namespace prune

// ---- gt_logit: per-variant logistic regression -------------------------------------------------------------------------------------
namespace logit {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxP = 16;            // design columns with the genotype: PGENHIP_LOGIT_MAX_COVARIATES + 1
constexpr uint32_t kSums = kMaxP * (kMaxP + 1u) / 2u + kMaxP;   // the lower half of H, then the gradient
constexpr uint32_t kBlocksPerCu = 8;      // grid cap; the FAST kernel's registers leave fewer resident, the rest queue

// FAST is compiled for p = n_cov + 1 rounded up to a bucket: the accumulators of a lane are bucket * (bucket + 1) / 2 + bucket
// FP64 registers.  At 16 they do not fit one wave's 256 VGPRs at all, and at 12 the compiler fits them only with copies through
// AGPRs and one wave per SIMD, so above 8 the rows of H are dealt to two waves
PGENHIP_PLAN_HD constexpr uint32_t bucket(uint32_t p) { return p <= 4u ? 4u : p <= 8u ? 8u : p <= 12u ? 12u : 16u; }
PGENHIP_PLAN_HD constexpr uint32_t waves_per_row(uint32_t bucket) { return bucket > 8u ? 2u : 1u; }
// rows a block carries through the iterations together (they share every design value through the CU's L1)
PGENHIP_PLAN_HD constexpr uint32_t group_rows(uint32_t bucket) { return kWaves / waves_per_row(bucket); }
PGENHIP_PLAN_HD constexpr uint64_t groups(uint64_t n_variants, uint32_t bucket) { return (n_variants + group_rows(bucket) - 1u) / group_rows(bucket); }
// which of a row's waves owns row a of H (and entry a of the gradient): rows 0, 3, 4, 7, ... and 1, 2, 5, 6, ... hold the same number
// of entries of the lower half
PGENHIP_PLAN_HD constexpr uint32_t row_part(uint32_t a, uint32_t waves) { return waves == 1u ? 0u : (((a & 3u) == 0u || (a & 3u) == 3u) ? 0u : 1u); }
// FP64 FMAs per included sample that the sums themselves take (the issue bound: 4 cycles each per 64 samples)
PGENHIP_PLAN_HD constexpr uint32_t sum_fmas(uint32_t p) { return p * (p + 1u) / 2u + p; }

// blocks: forced grid size (0 = by shape)
PGENHIP_PLAN_HD inline uint32_t fast_grid(uint32_t n_variants, uint32_t p, int num_cus, int blocks)
{
    return grid_blocks(groups(n_variants, bucket(p)), kBlocksPerCu, num_cus, blocks);
}
// GENERAL: a block per row, the rest by grid stride
PGENHIP_PLAN_HD inline uint32_t general_grid(uint32_t n_variants, int num_cus, int blocks) { return grid_blocks(n_variants, kBlocksPerCu, num_cus, blocks); }

}  // namespace logit

}  // namespace pgenhip::plan
