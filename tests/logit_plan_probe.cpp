// logit_plan_probe.cpp — namespace plan::logit of csrc/launch_plan.h as a shared object for the tests (tests/logit_plan.py compiles and
// loads it, as tests/launch_plan.py does with plan_probe.cpp): scalars in through `in`, results out through `out`.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace L = pgenhip::plan::logit;

extern "C" {

void logit_constants(const int64_t *, uint64_t *out)
{
    out[0] = L::kThreads, out[1] = L::kWaves, out[2] = L::kMaxP, out[3] = L::kSums, out[4] = L::kBlocksPerCu;
}

void logit_shape(const int64_t *in, uint64_t *out)   // p
{
    const uint32_t b = L::bucket((uint32_t)in[0]);
    out[0] = b, out[1] = L::waves_per_row(b), out[2] = L::group_rows(b), out[3] = L::sum_fmas((uint32_t)in[0]);
}

void logit_row_part(const int64_t *in, uint64_t *out) { out[0] = L::row_part((uint32_t)in[0], (uint32_t)in[1]); }   // a, waves

void logit_grids(const int64_t *in, uint64_t *out)   // n_variants, p, num_cus, blocks
{
    out[0] = L::groups((uint64_t)in[0], L::bucket((uint32_t)in[1]));
    out[1] = L::fast_grid((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[2] = L::general_grid((uint32_t)in[0], (int)in[2], (int)in[3]);
}

}  // extern "C"
