// gapply_plan_probe.cpp — namespace plan::gapply of csrc/launch_plan.h as a shared object for the tests (tests/gapply_plan.py compiles
// and loads it, as tests/launch_plan.py does with plan_probe.cpp): scalars in through `in`, results out through `out`.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace G = pgenhip::plan::gapply;

extern "C" {

void gapply_constants(const int64_t *, uint64_t *out)
{
    out[0] = G::kThreads, out[1] = G::kWaves, out[2] = G::kGroup, out[3] = G::kRowTile, out[4] = G::kStepSamples, out[5] = G::kSampleTile;
    out[6] = G::kStepRows, out[7] = G::kMinSliceSamples, out[8] = G::kMinSliceRows, out[9] = G::kMaxGridTiles, out[10] = G::kMaxGridBlocks;
}

void gapply_plan(const int64_t *in, uint64_t *out)   // n_variants, kept_count, n_columns, mfma, forced sample slices, forced row slices, num_cus
{
    const G::Plan p = G::plan((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], in[3] != 0, (int)in[4], (int)in[5], (int)in[6]);
    out[0] = p.p_tiles, out[1] = p.y_tiles, out[2] = p.p_grid, out[3] = p.y_grid, out[4] = p.sample_slices, out[5] = p.row_slices;
}

void gapply_slice_samples(const int64_t *in, uint64_t *out)   // K, slice, slices
{
    const pgenhip::plan::RowRange r = G::slice_samples((uint64_t)in[0], (uint32_t)in[1], (uint32_t)in[2]);
    out[0] = r.begin, out[1] = r.end;
}

}  // extern "C"
