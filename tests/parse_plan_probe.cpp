// parse_plan_probe.cpp — namespace plan::parse of csrc/launch_plan.h (gt_parse.hip's launch plans) as a shared object for the
// tests: tests/launch_plan.py compiles and loads it, tests/parse_plan.py holds its Python twin against it.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace P = pgenhip::plan::parse;
typedef const int64_t *In;
typedef uint64_t *Out;

extern "C" {

void parse_constants(In, Out out)
{
    out[0] = (uint64_t)P::kThreads, out[1] = P::kWaves, out[2] = P::kBlocksPerCu, out[3] = P::kPieceBytes, out[4] = P::kPieceSamples;
    out[5] = P::kPieceText, out[6] = P::kChunkLaneBytes, out[7] = P::kChunkBytes, out[8] = P::kAutoFixedFirst, out[9] = P::kLanePieces, out[10] = P::kBlockPieces;
}
void parse_pieces(In in, Out out)   // record_size
{
    out[0] = P::pieces_per_line((uint32_t)in[0]), out[1] = P::rows_per_block((uint32_t)in[0]), out[2] = P::blocks_per_row((uint32_t)in[0]);
}
void parse_piece_bytes(In in, Out out)   // record_size, piece
{
    const pgenhip::plan::RowRange r = P::piece_bytes((uint32_t)in[0], (uint32_t)in[1]);
    out[0] = r.begin, out[1] = r.end;
}
void parse_fixed_plan(In in, Out out)   // record_size, n_lines, num_cus, blocks
{
    const P::FixedPlan p = P::fixed_plan((uint32_t)in[0], (uint32_t)in[1], (int)in[2], (int)in[3]);
    out[0] = p.pieces, out[1] = p.total, out[2] = p.grid;
}
void parse_general(In in, Out out)   // n_lines, num_cus, blocks, region bytes, lead
{
    out[0] = P::general_grid((uint32_t)in[0], (int)in[1], (int)in[2]);
    out[1] = P::general_chunks((uint64_t)in[3], (uint32_t)in[4]);
}

}  // extern "C"
