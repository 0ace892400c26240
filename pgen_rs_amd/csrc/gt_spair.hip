// gt_spair.hip — pairwise sample tables for gfx950 (MI355X): for every pair of kept samples (a, b) of two rank ranges the exact 4 x 4
// table T[x][y] = number of selected rows in which a has code x and b has code y (src/pfile.rs:172-183: sample s in byte s/4, bits
// 2*(s%4)).  The transpose of gt_pair.hip: pairs of samples summed over rows.  Every kernel ADDS into out (u32, modular); capi.hip
// zeroes the entries ahead of the launch unless the caller accumulates.
//
// GENERAL: a lane owns one pair, walks its row range reading the two samples' bytes and keeps the sixteen counters in registers
// (sixteen compares of the 4-bit pair code, no dynamic indexing).  The correctness baseline of the MFMA shape.
//
// MFMA: the project's first contraction.  Per sample three 0/1 int8 indicator vectors over the rows, h (code 1), d (code 2),
// m (code 3); the nine cells with x, y in {1, 2, 3} are the nine products ind_x(a)^T ind_y(b), formed by
// v_mfma_i32_16x16x64_i8 on 16 x 16 samples and 64 rows at a time, accumulating in i32.  The other seven cells follow from the
// per-sample totals of h, d, m over the same rows and the row count:
//     T[x][0] = tot_a[x] - T[x][1] - T[x][2] - T[x][3]        x = 1, 2, 3
//     T[0][y] = tot_b[y] - T[1][y] - T[2][y] - T[3][y]        y = 1, 2, 3
//     T[0][0] = n - tot_a[1] - tot_a[2] - tot_a[3] - T[0][1] - T[0][2] - T[0][3]
// A block of four waves owns a tile of 64 x 64 ranks and one contiguous range of rows (a "slice", below 2^31 rows, so an i32
// accumulator stays below its sign bit).  Per step of 64 rows it stages both operands ONCE: thread t owns rank t & 63 of operand
// (t >> 6) & 1 and the 32 rows of half t >> 7; it reads the sample's byte of each row (rank -> sample through the kept list; pad
// bits and samples >= N are never touched), gathers four rows' codes into the bytes of a word, forms the three indicator words
// with three bit operations each and counts the totals with v_bcnt, then writes 2 x 16 bytes per indicator to the LDS image
// [operand][indicator][rank][row], ranks 80 bytes apart.  That image IS the transpose: an operand fragment (one rank, 16 consecutive
// rows per lane) is one ds_read_b128.  A and B fragments are built by the same code from the same rows, so the k order inside a
// fragment, which the instruction does not document for int8, cancels in the sum over rows.  Each wave owns 32 x 32 ranks:
// 2 x 3 A fragments, 2 x 3 B fragments, 36 MFMAs per step.  The next step's bytes are loaded before the MFMAs of the current one.
// The kernel is compiled for two blocks per CU (all 144 accumulator registers in VGPRs), which measured 1.67 x ahead of one
// (profiles/r10_spair), and per row selection (stride, variant list, byte offsets), so that no byte load sits under a branch.
// Rows past the slice and ranks past the range stage zeros (code 0), which add nothing to any product or total.
// Epilogue: C/D map col = lane & 15 (the B operand's rank), row = (lane >> 4) * 4 + reg (the A operand's rank); a lane holds all
// nine products of its four pairs per 16 x 16 tile, completes the sixteen cells and adds the non-zero ones with
// global_atomic_add_u32.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::spair;               // kThreads, kTile, kStepRows, the grid caps and the launch plan
constexpr uint32_t kRankStride = 80;       // bytes between ranks in the LDS image (64 rows + 16: ds_read_b128 of 16 ranks spread over the banks)
constexpr uint32_t kIndBytes = kTile * kRankStride;
constexpr uint32_t kOperandBytes = 3u * kIndBytes;

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t sample_of(const SpairArgs &a, uint32_t rank) { return a.kept_idx != nullptr ? a.kept_idx[rank] : rank; }

__device__ __forceinline__ void add_cell(uint32_t *p, uint32_t v)
{
    if (v != 0u) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void gt_spair_general_kernel(SpairArgs a, uint64_t pairs, uint64_t pair_blocks, uint32_t grid_pairs, uint32_t slices)
{
    const uint32_t slice = blockIdx.x / grid_pairs;
    const uint64_t V = a.n_variants;
    const plan::RowRange rows = plan::slice_rows(V, slice, slices);
    const uint64_t rbeg = rows.begin, rend = rows.end;
    for (uint64_t pb = blockIdx.x % grid_pairs; pb < pair_blocks; pb += grid_pairs) {
        const uint64_t p = pb * kThreads + threadIdx.x;
        if (p >= pairs) break;
        const uint32_t i = (uint32_t)(p / a.b_count), l = (uint32_t)(p % a.b_count);
        const uint32_t sa = sample_of(a, a.a_begin + i), sb = sample_of(a, a.b_begin + l);
        const uint32_t ba = sa >> 2, bb = sb >> 2, sha = 2u * (sa & 3u), shb = 2u * (sb & 3u);
        uint32_t cnt[16];
#pragma unroll
        for (int q = 0; q < 16; q++) cnt[q] = 0u;
        for (uint64_t j = rbeg; j < rend; j++) {
            const uint8_t *rec = row_record(a, j);
            const uint32_t c = (((uint32_t)rec[ba] >> sha) & 3u) * 4u + (((uint32_t)rec[bb] >> shb) & 3u);
#pragma unroll
            for (int q = 0; q < 16; q++) cnt[q] += c == (uint32_t)q ? 1u : 0u;
        }
        uint32_t *o = a.out + 16u * p;
#pragma unroll
        for (int q = 0; q < 16; q++) add_cell(o + q, cnt[q]);
    }
}

// MODE: rows by stride (0), through variant_idx (1), through record_off (2)
template <int MODE>
__global__ __launch_bounds__(kThreads, 2) void gt_spair_mfma_kernel(SpairArgs a, uint32_t tiles_b, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[2u * kOperandBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slice = blockIdx.x / grid_tiles;
    const uint64_t V = a.n_variants;
    const plan::RowRange rows = plan::slice_rows(V, slice, slices);
    const uint64_t rbeg = rows.begin, rend = rows.end;
    const uint32_t n = (uint32_t)(rend - rbeg);                 // < 2^31 (launch plan)
    const uint32_t steps = (n + kStepRows - 1u) / kStepRows;
    // staging role: operand, rank of the tile, half of the step's rows (wave-uniform: waves 0, 1 stage rows 0-31, waves 2, 3 rows 32-63)
    const uint32_t op = (tid >> 6) & 1u, ts = tid & 63u;
    const uint32_t half = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 7));
    // MFMA role: the wave's 32 x 32 ranks of the tile
    const uint32_t wa = wave >> 1, wb = wave & 1u;

    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint32_t ta = (uint32_t)(tile / tiles_b), tb = (uint32_t)(tile % tiles_b);
        const uint64_t local = (uint64_t)(op ? tb : ta) * kTile + ts;
        const bool valid = local < (op ? a.b_count : a.a_count);
        const uint32_t sample = sample_of(a, (op ? a.b_begin : a.a_begin) + (valid ? (uint32_t)local : 0u));
        const uint32_t boff = sample >> 2, shift = 2u * (sample & 3u);

        // the codes of this thread's sample in its 32 rows of step t, four rows per word (row i in byte i % 4 of word i / 4);
        // rows past the slice and ranks past the range give code 0
        auto load = [&](uint32_t t, uint32_t (&c4)[8]) {
            const uint64_t r0 = rbeg + (uint64_t)t * kStepRows + half * 32u;
            // the rows' record offsets are wave-uniform and come first, G at a time (MODE: how the rows are selected), so that
            // no load of a sample byte sits under a branch and all 32 are in flight together
            constexpr uint32_t G = MODE == 2 ? 4u : 8u;   // 64-bit offsets from memory: fewer at a time, for ScratchSize 0
            uint32_t raw[32];
            const uint8_t *lp = a.records + boff;
#pragma unroll
            for (uint32_t g = 0; g < 32u; g += G) {
                uint64_t off[G];
#pragma unroll
                for (uint32_t i = 0; i < G; i++) {
                    const uint64_t row = r0 + g + i < rend ? r0 + g + i : rbeg;
                    off[i] = MODE == 2 ? a.record_off[row] : MODE == 1 ? (uint64_t)a.variant_idx[row] * a.record_stride : row * a.record_stride;
                }
#pragma unroll
                for (uint32_t i = 0; i < G; i++) raw[g + i] = lp[off[i]];
            }
#pragma unroll
            for (uint32_t q = 0; q < 8u; q++) {
                uint32_t w = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const uint32_t code = (raw[4u * q + i] >> shift) & 3u;
                    w |= (valid && r0 + 4u * q + i < rend ? code : 0u) << (8u * i);
                }
                c4[q] = w;
            }
        };

        v4i acc[2][2][3][3];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int x = 0; x < 3; x++)
#pragma unroll
                    for (int y = 0; y < 3; y++) acc[i][j][x][y] = v4i{0, 0, 0, 0};
        uint32_t tot[3] = {0u, 0u, 0u};

        uint32_t cur[8];
        load(0u, cur);
        for (uint32_t t = 0; t < steps; t++) {
            // codes -> the three indicator vectors (bytes of 0 / 1), their totals, the LDS image
            uint32_t ind[3][8];
#pragma unroll
            for (uint32_t q = 0; q < 8u; q++) {
                const uint32_t c = cur[q], hi = c >> 1;
                ind[0][q] = c & ~hi & 0x01010101u;
                ind[1][q] = hi & ~c & 0x01010101u;
                ind[2][q] = c & hi & 0x01010101u;
#pragma unroll
                for (int x = 0; x < 3; x++) tot[x] += (uint32_t)__builtin_popcount(ind[x][q]);
            }
            uint8_t *dst = lds + op * kOperandBytes + ts * kRankStride + half * 32u;
#pragma unroll
            for (int x = 0; x < 3; x++) {
                u32x4 *d = reinterpret_cast<u32x4 *>(dst + (uint32_t)x * kIndBytes);
                d[0] = u32x4{ind[x][0], ind[x][1], ind[x][2], ind[x][3]};
                d[1] = u32x4{ind[x][4], ind[x][5], ind[x][6], ind[x][7]};
            }
            __syncthreads();
            if (t + 1u < steps) load(t + 1u, cur);   // in flight under the MFMAs

            v4i fb[2][3];
            const uint32_t frag = (lane & 15u) * kRankStride + 16u * (lane >> 4);
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int y = 0; y < 3; y++)
                    fb[j][y] = *reinterpret_cast<const v4i *>(lds + kOperandBytes + (uint32_t)y * kIndBytes + (32u * wb + 16u * (uint32_t)j) * kRankStride + frag);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                v4i fa[3];
#pragma unroll
                for (int x = 0; x < 3; x++)
                    fa[x] = *reinterpret_cast<const v4i *>(lds + (uint32_t)x * kIndBytes + (32u * wa + 16u * (uint32_t)i) * kRankStride + frag);
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int x = 0; x < 3; x++)
#pragma unroll
                        for (int y = 0; y < 3; y++)
                            acc[i][j][x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[x], fb[j][y], acc[i][j][x][y], 0, 0, 0);
            }
            __syncthreads();   // the image is read; the next step may overwrite it
        }

        // per-sample totals of the slice through LDS: [half][operand][rank][indicator]
        uint32_t *tots = reinterpret_cast<uint32_t *>(lds);
#pragma unroll
        for (int x = 0; x < 3; x++) tots[((half * 2u + op) * kTile + ts) * 3u + (uint32_t)x] = tot[x];
        __syncthreads();

#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t bl = 32u * wb + 16u * (uint32_t)j + (lane & 15u);
            const uint64_t l = (uint64_t)tb * kTile + bl;
            uint32_t tb_[3];
#pragma unroll
            for (int y = 0; y < 3; y++) tb_[y] = tots[(kTile + bl) * 3u + (uint32_t)y] + tots[(3u * kTile + bl) * 3u + (uint32_t)y];
#pragma unroll
            for (int i = 0; i < 2; i++) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const uint32_t al = 32u * wa + 16u * (uint32_t)i + (lane >> 4) * 4u + (uint32_t)reg;
                    const uint64_t ia = (uint64_t)ta * kTile + al;
                    if (ia >= a.a_count || l >= a.b_count) continue;
                    uint32_t ta_[3];
#pragma unroll
                    for (int x = 0; x < 3; x++) ta_[x] = tots[al * 3u + (uint32_t)x] + tots[(2u * kTile + al) * 3u + (uint32_t)x];
                    uint32_t T[4][4];
#pragma unroll
                    for (int x = 0; x < 3; x++)
#pragma unroll
                        for (int y = 0; y < 3; y++) T[x + 1][y + 1] = (uint32_t)acc[i][j][x][y][reg];
#pragma unroll
                    for (int x = 1; x < 4; x++) T[x][0] = ta_[x - 1] - T[x][1] - T[x][2] - T[x][3];
#pragma unroll
                    for (int y = 1; y < 4; y++) T[0][y] = tb_[y - 1] - T[1][y] - T[2][y] - T[3][y];
                    T[0][0] = n - ta_[0] - ta_[1] - ta_[2] - T[0][1] - T[0][2] - T[0][3];
                    uint32_t *o = a.out + 16u * (ia * a.b_count + l);
#pragma unroll
                    for (int x = 0; x < 4; x++)
#pragma unroll
                        for (int y = 0; y < 4; y++) add_cell(o + 4 * x + y, T[x][y]);
                }
            }
        }
        __syncthreads();   // the totals are read; the next tile's image may overwrite them
    }
}

}  // namespace

hipError_t launch_gt_spair_general(const SpairArgs &a, int slices_per_tile, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.a_count == 0 || a.b_count == 0) return hipSuccess;
    const uint64_t pairs = (uint64_t)a.a_count * a.b_count;
    const uint32_t grid_pairs = plan::spair::grid_pairs(a.a_count, a.b_count);
    const uint32_t slices = general_slices(a.n_variants, a.a_count, a.b_count, slices_per_tile, num_cus);
    hipLaunchKernelGGL(gt_spair_general_kernel, dim3(grid_pairs * slices), dim3(kThreads), 0, stream, a, pairs, pair_blocks(a.a_count, a.b_count), grid_pairs, slices);
    return hipGetLastError();
}

hipError_t launch_gt_spair_mfma(const SpairArgs &a, int slices_per_tile, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.a_count == 0 || a.b_count == 0) return hipSuccess;
    const uint32_t tiles_b = range_tiles(a.b_count);
    const uint64_t tiles = plan::spair::tiles(a.a_count, a.b_count);
    const uint32_t grid_tiles = plan::spair::grid_tiles(a.a_count, a.b_count);
    const uint32_t slices = mfma_slices(a.n_variants, a.a_count, a.b_count, slices_per_tile, num_cus);
    const dim3 grid(grid_tiles * slices), block(kThreads);
    if (a.record_off != nullptr)
        hipLaunchKernelGGL(gt_spair_mfma_kernel<2>, grid, block, 0, stream, a, tiles_b, tiles, grid_tiles, slices);
    else if (a.variant_idx != nullptr)
        hipLaunchKernelGGL(gt_spair_mfma_kernel<1>, grid, block, 0, stream, a, tiles_b, tiles, grid_tiles, slices);
    else
        hipLaunchKernelGGL(gt_spair_mfma_kernel<0>, grid, block, 0, stream, a, tiles_b, tiles, grid_tiles, slices);
    return hipGetLastError();
}

}  // namespace pgenhip
