// wide_plan_probe.cpp — namespace plan::wide of csrc/launch_plan.h as a shared object for the tests (tests/wide_plan.py compiles and
// loads it, as tests/launch_plan.py does with plan_probe.cpp): scalars in through `in`, results out through `out`.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace W = pgenhip::plan::wide;

extern "C" {

void wide_constants(const int64_t *, uint64_t *out)
{
    out[0] = W::kThreads, out[1] = W::kStorers, out[2] = W::kSpanChunks, out[3] = W::kShortLaunchBytes, out[4] = W::kWtOneSpanMaxBytes;
    out[5] = W::kFrontSteps, out[6] = W::kStoreNt, out[7] = W::kStoreWt, out[8] = W::kBurstOneMinBytes, out[9] = W::kRunsLongBytes;
}

void wide_spans_per_row(const int64_t *in, uint64_t *out) { out[0] = W::spans_per_row((uint64_t)in[0]); }   // row bytes

void wide_steps(const int64_t *in, uint64_t *out) { out[0] = W::steps((uint64_t)in[0]); }   // items

static void put(const W::Rule &r, uint64_t *out) { out[0] = r.policy, out[1] = r.burst, out[2] = r.blocks_per_cu, out[3] = r.fronts, out[4] = r.grid; }

void wide_kernel_choice(const int64_t *in, uint64_t *out)   // text bytes, spans per row, runs, forced policy, forced burst
{
    put(W::kernel_choice((uint64_t)in[0], (uint32_t)in[1], in[2] != 0, (int)in[3], (int)in[4]), out);
}

void wide_rule(const int64_t *in, uint64_t *out)   // text bytes, spans per row, runs, steps needed, occupancy, CUs, forced policy / blocks per CU / fronts / burst
{
    put(W::rule((uint64_t)in[0], (uint32_t)in[1], in[2] != 0, (uint64_t)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], (int)in[8], (int)in[9]), out);
}

}  // extern "C"
