// prune_plan_probe.cpp — namespace plan::prune of csrc/launch_plan.h (gt_prune.hip's launch plans) as a shared object for the tests:
// tests/launch_plan.py compiles and loads it, tests/prune_plan.py holds its Python twin against it.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace P = pgenhip::plan::prune;
typedef const int64_t *In;
typedef uint64_t *Out;

extern "C" {

void prune_constants(In, Out out)
{
    out[0] = (uint64_t)P::kThreads, out[1] = P::kBlocksPerCu, out[2] = P::kChunkRows, out[3] = P::kHaloRows, out[4] = P::kLdsRows;
}
void prune_window(In in, Out out)   // window
{
    out[0] = P::mask_words((uint32_t)in[0]), out[1] = P::halo_rows((uint32_t)in[0]);
}
void prune_general_grid(In in, Out out)   // n_rows, num_cus, blocks
{
    out[0] = P::general_grid((uint64_t)in[0], (int)in[1], (int)in[2]);
}
void prune_block_plan(In in, Out out)   // n_rows, num_cus, blocks
{
    const P::BlockPlan p = P::block_plan((uint64_t)in[0], (int)in[1], (int)in[2]);
    out[0] = p.range_rows, out[1] = p.grid;
}
void prune_auto(In in, Out out)   // n_rows, window: 1 = BLOCK
{
    out[0] = P::auto_block((uint64_t)in[0], (uint32_t)in[1]);
}

}  // extern "C"
