// emit_plan_probe.cpp — namespace plan::emit of csrc/launch_plan.h as a shared object for the tests (tests/subset_plan.py and
// tests/line_plan.py load it through tests/launch_plan.py, as tests/wide_plan.py does with wide_plan_probe.cpp): scalars in through
// `in`, results out through `out`.  A shape is the eleven scalars of plan::emit::Shape, in the order of its fields.  No logic here.
#include "../pgen_rs_amd/csrc/launch_plan.h"

namespace E = pgenhip::plan::emit;
typedef const int64_t *In;
typedef uint64_t *Out;

static E::Shape shape(In in)
{
    E::Shape s{};
    s.N = (uint32_t)in[0], s.K = (uint32_t)in[1], s.R = (uint32_t)in[2], s.V = (uint32_t)in[3];
    s.kept_list = in[4] != 0, s.lines = in[5] != 0, s.gathered = in[6] != 0, s.records_dense = in[7] != 0, s.out_dense = in[8] != 0;
    s.max_line_bytes = (uint64_t)in[9], s.prefix_blob = in[10] != 0;
    return s;
}
constexpr int kShape = 11;   // scalars of a shape: further arguments follow them

extern "C" {

void emit_constants(In, Out out)
{
    out[0] = E::kWaves, out[1] = E::kScanSegmentSamples, out[2] = E::kCompactMaxSegCodes, out[3] = E::kCompactSliceBytes;
    out[4] = E::kRowPickMaxKept, out[5] = E::kRowPickMaxSegments, out[6] = E::kRowPickRowsPerWave;
    out[7] = E::kRunLoadBytes, out[8] = E::kRunSpanBytes, out[9] = E::kLrMaxRows, out[10] = E::kLrPfxBytes, out[11] = E::kLrTabMaxSamples;
    out[12] = E::pick_family::kMaxSamples, out[13] = E::pick_family::kStageBytes, out[14] = (uint64_t)E::pick_family::kMaxBatchRows;
    out[15] = E::pick_family::kMaxPackedRows, out[16] = E::pick_family::kPfxBytes, out[17] = E::pick_family::kMaxLinesRows;
    out[18] = E::pick_family::kMaxLinesPrefix;
}

void emit_n_segments(In in, Out out) { out[0] = E::n_segments((uint32_t)in[0]); }   // N

// ---- applicability (shape; rowpick: + CUs)
void emit_applicable(In in, Out out)
{
    const E::Shape s = shape(in);
    out[0] = E::flat(s), out[1] = E::wide(s), out[2] = E::wide_lines(s), out[3] = E::runs(s), out[4] = E::runs_preferred(s);
    out[5] = E::lineruns(s), out[6] = E::pick(s), out[7] = E::rowpick_takes(s), out[8] = E::rowpick(s, (int)in[kShape]);
    out[9] = E::run_rows(s), out[10] = E::lineruns_rows(s);
}
void emit_lineruns_seam_shift(In in, Out out) { out[0] = E::lineruns_seam_shift((uint32_t)in[0]); }   // seam bytes
void emit_prefix_copy_shift(In in, Out out) { out[0] = E::prefix_copy_shift((uint64_t)in[0]); }      // longest prefix

// ---- AUTO and forced ids
void emit_two_pass_shape(In in, Out out) { out[0] = E::two_pass_shape((uint32_t)in[0], (uint32_t)in[1]); }   // N, K
void emit_very_sparse(In in, Out out) { out[0] = E::very_sparse((uint32_t)in[0], (uint32_t)in[1]); }         // N, K
void emit_rowpick_shape(In in, Out out) { out[0] = E::rowpick_shape(shape(in), in[kShape] != 0, (int)in[kShape + 1]); }   // shape, rowpick on, CUs
void emit_two_pass(In in, Out out) { out[0] = E::two_pass(shape(in), in[kShape] != 0, (uint32_t)in[kShape + 1]); }     // shape, two-pass on, max_seg_count
void emit_choose_all_samples(In in, Out out) { out[0] = (uint64_t)E::choose_all_samples(shape(in)); }
void emit_choose_subset(In in, Out out)   // shape, rowpick on, two-pass on, max_seg_count, CUs
{
    out[0] = (uint64_t)E::choose_subset(shape(in), in[kShape] != 0, in[kShape + 1] != 0, (uint32_t)in[kShape + 2], (int)in[kShape + 3]);
}
void emit_accepts(In in, Out out)   // shape, kernel id
{
    const uint32_t kernel = (uint32_t)in[kShape];
    out[0] = E::accepts(kernel, shape(in)), out[1] = E::is_kernel_id(kernel), out[2] = (uint64_t)E::forced(kernel, in[5] != 0);
}
void emit_choices(In, Out out)   // the values of Emit, in the order tests/subset_plan.py names them
{
    out[0] = (uint64_t)E::Emit::Rows, out[1] = (uint64_t)E::Emit::Flat, out[2] = (uint64_t)E::Emit::Wide, out[3] = (uint64_t)E::Emit::Runs;
    out[4] = (uint64_t)E::Emit::LineRuns, out[5] = (uint64_t)E::Emit::Pick, out[6] = (uint64_t)E::Emit::Scan, out[7] = (uint64_t)E::Emit::RowPick;
    out[8] = (uint64_t)E::Emit::TwoPass;
}

// ---- the two passes
void emit_chunks(In in, Out out)   // shape, slice bytes, forced rows, rowpick on, rows of a round, CUs
{
    const E::Chunks c = E::chunks(shape(in), (uint64_t)in[kShape], (int)in[kShape + 1], in[kShape + 2] != 0, (uint64_t)in[kShape + 3], (int)in[kShape + 4]);
    out[0] = c.rows, out[1] = c.row_owner;
}
void emit_chunk_by_row_owner(In in, Out out) { out[0] = E::chunk_by_row_owner(E::Chunks{(uint64_t)in[0], in[1] != 0}, (uint32_t)in[2]); }   // chunk rows, row owner, n

// ---- launch plans
void emit_scan_plan(In in, Out out)   // N, K, V, compact, occupancy, forced blocks per CU, XCD map, CUs
{
    const E::ScanPlan p = E::scan_plan((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], in[3] != 0, (int)in[4], (int)in[5], in[6] != 0, (int)in[7]);
    out[0] = p.n_seg, out[1] = p.per_cu, out[2] = p.groups, out[3] = p.xcd_groups, out[4] = p.bands, out[5] = p.grid;
}
void emit_rowpick_lds_bytes(In in, Out out) { out[0] = E::rowpick_lds_bytes((uint32_t)in[0], (uint32_t)in[1]); }   // N, K
void emit_rowpick_plan(In in, Out out)   // N, V, compact, occupancy, forced blocks per CU, CUs
{
    const E::RowPickPlan p = E::rowpick_plan((uint32_t)in[0], (uint32_t)in[1], in[2] != 0, (int)in[3], (int)in[4], (int)in[5]);
    out[0] = p.per_cu, out[1] = p.max_blocks, out[2] = p.grid;
}
void emit_pick_plan(In in, Out out)   // shape, batch bytes
{
    const E::Shape s = shape(in);
    const E::PickPlan p = E::pick_plan(s, (int)in[kShape]);
    const E::PickLinesPlan l = E::pick_lines_plan(s, p);
    out[0] = p.packed, out[1] = p.pitch, out[2] = p.batch_rows, out[3] = l.taken, out[4] = (uint64_t)(int64_t)l.batch_rows, out[5] = l.cps_shift;
}
void emit_pick_lines_rows(In in, Out out) { out[0] = (uint64_t)(int64_t)E::pick_lines_rows((uint32_t)in[0], (uint64_t)in[1], (uint32_t)in[2]); }   // R, longest prefix, batch rows
void emit_pick_cps_shift(In in, Out out) { out[0] = E::pick_cps_shift((uint64_t)in[0]); }   // longest prefix

}  // extern "C"
