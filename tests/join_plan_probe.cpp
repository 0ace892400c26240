// join_plan_probe.cpp — namespace plan::join of csrc/launch_plan.h (gt_join.hip's launch plans) as a shared object for the tests:
// tests/launch_plan.py compiles and loads it, tests/join_plan.py holds its Python twin against it.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace J = pgenhip::plan::join;
typedef const int64_t *In;
typedef uint64_t *Out;

extern "C" {

void join_constants(In, Out out) { out[0] = (uint64_t)J::kThreads, out[1] = J::kBlocksPerCu, out[2] = J::kChunkBytes; }
void join_chunks(In in, Out out)   // record_size
{
    out[0] = J::chunks_per_row((uint32_t)in[0]), out[1] = J::rows_per_block((uint32_t)in[0]), out[2] = J::blocks_per_row((uint32_t)in[0]);
}
void join_chunk_bytes(In in, Out out)   // record_size, mis, chunk
{
    const pgenhip::plan::RowRange r = J::chunk_bytes((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2]);
    out[0] = r.begin, out[1] = r.end;
}
void join_stream_plan(In in, Out out)   // record_size, n_variants, num_cus, blocks
{
    const J::StreamPlan p = J::stream_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.chunks, out[1] = p.total, out[2] = p.grid;
}
void join_general_grid(In in, Out out)   // n_variants, record_size, num_cus, blocks
{
    out[0] = J::general_grid((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
}
void join_auto(In in, Out out)   // record_size, n_variants, n_parts: 1 = STREAM
{
    out[0] = J::auto_stream((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2]);
}

}  // extern "C"
