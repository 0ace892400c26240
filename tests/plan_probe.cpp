// plan_probe.cpp — csrc/launch_plan.h as a shared object for the tests (tests/launch_plan.py compiles and loads it): one extern "C"
// function per plan function, scalars in through `in`, results out through `out`, and the plan constants by name.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace P = pgenhip::plan;
typedef const int64_t *In;
typedef uint64_t *Out;

namespace {
struct Constant {
    const char *name;
    uint64_t value;
};
#define K(ns, name) {#ns "." #name, (uint64_t)P::ns::name}
const Constant kConstants[] = {
    K(count, kThreads), K(count, kBlocksPerCu),
    K(scount, kThreads), K(scount, kWaves), K(scount, kBatch), K(scount, kHiBits), K(scount, kWindowBatches), K(scount, kColWords),
    K(scount, kMaxBlocksPerCu), K(scount, kLdsPerCu),
    K(score, kThreads), K(score, kWaves), K(score, kMaxBlocksPerCu), K(score, kMinSliceRows),
    K(vsum, kThreads), K(vsum, kWaves), K(vsum, kBlocksPerCu), K(vsum, kTileBytes), K(vsum, kGroupRows), K(vsum, kMinSliceRows),
    K(matrix, kThreads), K(matrix, kBlocksPerCu), K(matrix, kLongRowBytes), K(matrix, kTileVariants), K(matrix, kWaveSamples),
    K(matrix, kTileSamples), K(matrix, kTileBlocksPerCu), K(matrix, kGeneral), K(matrix, kStream), K(matrix, kTile),
    K(pair, kThreads), K(pair, kTile), K(pair, kChunkWords), K(pair, kBlocksPerCu),
    K(pack, kThreads), K(pack, kBlocksPerCu), K(pack, kPartChunks), K(pack, kStreamRunBytes),
    K(spair, kThreads), K(spair, kTile), K(spair, kStepRows), K(spair, kMaxGridTiles), K(spair, kMaxGridBlocks), K(spair, kMinSliceRows),
    K(spair, kGeneralBlocksPerCu), K(spair, kMfmaBlocksPerCu),
    K(gram, kThreads), K(gram, kTile), K(gram, kStepRows), K(gram, kGroupRows), K(gram, kMaxGridTiles), K(gram, kMaxGridBlocks),
    K(gram, kMinSliceRows), K(gram, kGeneralBlocksPerCu), K(gram, kMfmaBlocksPerCu),
};
#undef K
}  // namespace

extern "C" {

// constant i: its name ("family.kName") and value; nullptr past the last
const char *plan_constant(uint32_t i, uint64_t *value)
{
    if (i >= sizeof(kConstants) / sizeof(kConstants[0])) return nullptr;
    *value = kConstants[i].value;
    return kConstants[i].name;
}

// ---- shared
void cu_count(In in, Out out) { out[0] = P::cu_count((int)in[0]); }
void grid_blocks(In in, Out out) { out[0] = P::grid_blocks((uint64_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]); }
void slice_rows(In in, Out out)
{
    const P::RowRange r = P::slice_rows((uint64_t)in[0], (uint32_t)in[1], (uint32_t)in[2]);
    out[0] = r.begin, out[1] = r.end;
}

// ---- count
void count_lanes_per_row(In in, Out out) { out[0] = P::count::lanes_per_row((uint32_t)in[0]), out[1] = P::count::max_chunks((uint32_t)in[0]); }
void count_shape(In in, Out out)   // record_size, WAVE_PER_ROW asked, ROWS_PER_WAVE asked
{
    const bool wave = P::count::wave_per_row(in[1] != 0, in[2] != 0, (uint32_t)in[0]);
    const P::count::Shape s = P::count::shape((uint32_t)in[0], wave);
    out[0] = wave, out[1] = s.G, out[2] = s.RU, out[3] = s.U;
}
void count_grid(In in, Out out)   // n_variants, G, RU, num_cus
{
    out[0] = P::count::rows_per_step((uint32_t)in[1], (uint32_t)in[2]);
    out[1] = P::count::rows_per_block((uint32_t)in[1], (uint32_t)in[2]);
    out[2] = P::count::grid((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3]);
}
void count_passes(In in, Out out) { out[0] = P::count::passes((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2]); }

// ---- scount
void scount_plan(In in, Out out)   // record_size, n_variants, num_cus, slices_per_tile
{
    const P::scount::Plan p = P::scount::plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.G, out[1] = p.tiles, out[2] = p.cols, out[3] = p.slices, out[4] = p.lds_bytes, out[5] = P::scount::slots(p.G);
}
void scount_hi_planes(In in, Out out) { out[0] = (uint64_t)P::scount::hi_planes((uint32_t)in[0]); }

// ---- score
void score_plan(In in, Out out)   // record_size, n_variants, n_columns, num_cus, slices_per_tile
{
    const P::score::Plan p = P::score::plan((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
    out[0] = p.bytes, out[1] = P::score::batch_rows((uint32_t)in[2]), out[2] = p.log_g, out[3] = p.tiles, out[4] = p.slices, out[5] = P::score::slots(p.log_g);
}

// ---- vsum
void vsum_mfma_plan(In in, Out out)   // record_size, n_variants, num_cus, blocks
{
    const P::vsum::MfmaPlan p = P::vsum::mfma_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.tiles, out[1] = p.slices, out[2] = p.grid, out[3] = P::vsum::mfma_atomic((uint32_t)in[0]), out[4] = P::vsum::groups((uint64_t)in[1]);
}
void vsum_general_grid(In in, Out out) { out[0] = P::vsum::general_grid((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]); }

// ---- matrix
void matrix_auto_shape(In in, Out out)   // all_kept, sample_major, out & 15, out_stride, kept_count
{
    out[0] = P::matrix::auto_shape(in[0] != 0, in[1] != 0, (uint32_t)in[2], (uint64_t)in[3], (uint32_t)in[4]);
    out[1] = P::matrix::stream_applicable(in[0] != 0, in[1] != 0);
    out[2] = P::matrix::tile_applicable(in[0] != 0, in[1] != 0, (uint32_t)in[2], (uint64_t)in[3], (uint32_t)in[4]);
}
void matrix_stream_plan(In in, Out out)   // n_variants, kept_count, elem_bytes, out & 15, out_stride, num_cus, blocks
{
    const P::matrix::StreamPlan p = P::matrix::stream_plan((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint64_t)in[4], (int)in[5], (int)in[6]);
    out[0] = p.dense, out[1] = p.long_rows, out[2] = p.per_row, out[3] = p.total, out[4] = p.grid_x, out[5] = p.grid_y;
}
void matrix_tile_plan(In in, Out out)   // n_variants, sample_count, num_cus, blocks
{
    const P::matrix::TilePlan p = P::matrix::tile_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.v_tiles, out[1] = p.bands, out[2] = p.total, out[3] = p.grid;
}
void matrix_general_grid(In in, Out out) { out[0] = P::matrix::general_grid((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]); }

// ---- pair
void pair_plan(In in, Out out)   // n_variants, n_left, window, num_cus, blocks
{
    const P::pair::Plan p = P::pair::plan((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
    out[0] = p.w_eff, out[1] = p.tiles_per_left, out[2] = p.n_items, out[3] = p.grid;
}

// ---- pack
void pack_applicable(In in, Out out)   // has a kept list, kept_count, sample_count
{
    out[0] = P::pack::dense_applicable(in[0] != 0, (uint32_t)in[1], (uint32_t)in[2]), out[1] = P::pack::gather_applicable(in[0] != 0, (uint32_t)in[1]);
}
void pack_general_grid(In in, Out out) { out[0] = P::pack::general_grid((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]); }
void pack_gather_plan(In in, Out out)   // n_variants, kept_count, num_cus, blocks
{
    const P::pack::GatherPlan p = P::pack::gather_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.Q, out[1] = p.total, out[2] = p.grid;
}
void pack_dense_plan(In in, Out out)   // record_size, n_variants, num_cus, blocks
{
    const P::pack::DensePlan p = P::pack::dense_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.G, out[1] = p.P, out[2] = p.parts, out[3] = p.items, out[4] = p.grid;
}
void pack_merge_runs(In in, Out out)   // gathered, sample_count, record_size, record_stride, out_stride, n_variants
{
    out[0] = P::pack::merge_runs(in[0] != 0, (uint32_t)in[1], (uint32_t)in[2], (uint64_t)in[3], (uint64_t)in[4], (uint32_t)in[5]);
    out[1] = P::pack::run_rows((uint32_t)in[2]);
}

// ---- spair, gram
void sample_pair_tiles(In in, Out out)   // a_count, b_count
{
    const uint32_t a = (uint32_t)in[0], b = (uint32_t)in[1];
    out[0] = P::sample_pairs::tiles(a, b), out[1] = P::sample_pairs::grid_tiles(a, b);
    out[2] = P::sample_pairs::pair_blocks(a, b), out[3] = P::sample_pairs::grid_pairs(a, b);
}
void pair_slices(In in, Out out)   // n_variants, grid_items, forced, num_cus, blocks_per_cu, unit_rows, min_slices
{
    out[0] = P::sample_pairs::pair_slices((uint32_t)in[0], (uint64_t)in[1], (int)in[2], (int)in[3], (uint32_t)in[4], (uint32_t)in[5], (uint64_t)in[6]);
}
void spair_slices(In in, Out out)   // n_variants, a_count, b_count, forced, num_cus
{
    out[0] = P::spair::general_slices((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
    out[1] = P::spair::mfma_slices((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
}
void gram_slices(In in, Out out)   // n_variants, a_count, b_count, forced, num_cus
{
    out[0] = P::gram::general_slices((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
    out[1] = P::gram::mfma_slices((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (int)in[3], (int)in[4]);
}

}  // extern "C"
