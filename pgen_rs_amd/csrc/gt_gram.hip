// gt_gram.hip — sample Gram matrix for gfx950 (MI355X): for every pair of kept samples (a, b) of two rank ranges the FP64 sum over the
// selected rows j of t_j[x_j(a)] * t_j[x_j(b)], where x_j(s) is the 2-bit code of sample s in row j (src/pfile.rs:172-183: sample s in
// byte s/4, bits 2*(s%4)) and t_j the row's four doubles code_values[4 j .. 4 j + 3].  The weighted member of the family whose integer
// member is gt_spair.hip: Z^T Z with Z[j][s] = t_j[x_j(s)].  A GRM, a dominance GRM, a dosage cross-product and the jointly-called
// count (table 1, 1, 1, 0) are all "four doubles per row"; the kernels do not interpret them.
//
// Arithmetic: every product and every addition is FP64, no f32 partial sums anywhere.  The order of the additions is not fixed (rows
// are dealt to slices and, inside the matrix core, to two accumulator chains; slices of one tile meet in global FP64 atomics), so
// two runs may differ in the last bits.  Sums whose every partial sum is an integer below 2^53 are exact in any order.
//
// GENERAL: a lane owns one pair and walks its row range: two byte loads, two selects from the row's table, one multiply-add.  The
// correctness baseline of the MFMA shape.
//
// MFMA: D (16 x 16) += A (16 x 4) B (4 x 16) with v_mfma_f64_16x16x4_f64: M = 16 a-ranks, N = 16 b-ranks, K = 4 rows.
//   A[m][k] = Z[row k][a-rank m] in lane (m = l & 15, k = l >> 4);   B[k][n] = Z[row k][b-rank n] in lane (k = l >> 4, n = l & 15)
//   D register i: a-rank m = (l >> 4) + 4 i, b-rank n = l & 15
// A block of four waves owns a tile of kTile x kTile ranks and one contiguous range of rows (a "slice").  Per step of kStepRows rows
// it expands both operands ONCE into an LDS image of doubles [operand][row][rank], rows kRowStride doubles apart: thread t owns
// operand t >> 7, row (t >> 2) & 31 of the step and the 16 ranks of quarter t & 3.  Without a kept list those 16 samples are at most
// five consecutive record bytes (four adjacent lanes read a row's 17 bytes; a byte index past the record is clamped, its codes
// masked); through a kept list the thread reads its 16 samples' bytes, so only the tile's samples are touched.  The thread reads its
// row's table once, selects 16 doubles from it (rows past the slice and ranks past the range give 0.0) and writes them as eight
// 16-byte LDS stores, rotated over the lanes so that neighbouring lanes fall on different banks.  Each wave then owns 32 x 32 ranks:
// per four rows two A and two B fragments (ds_read_b64, 16 consecutive doubles per row: the row pitch keeps the four rows of one
// read on different banks) feed four MFMAs, every fragment two of them, into two alternating accumulator chains (even and odd row
// groups).  The next step's record bytes and table are loaded before the MFMAs of the current one.  Compiled per row selection
// (stride, variant list, byte offsets) and per sample selection (all, kept list), so that no load sits under a branch.
// Epilogue: the two chains are added; a tile with one slice that overwrites stores its entries, everything else adds the non-zero
// ones with global_atomic_add_f64 (the target holds +0.0 or a sum, so a skipped -0.0 cannot matter).
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::gram;                // kThreads, kTile, kStepRows, kGroupRows, the grid caps and the launch plan
constexpr uint32_t kRowStride = 80;        // doubles between rows of the LDS image (64 ranks + 16: the four rows of a ds_read_b64 on different banks)
constexpr uint32_t kOperandDoubles = kStepRows * kRowStride;

typedef double gram_v4d __attribute__((ext_vector_type(4)));
typedef double gram_v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t sample_of(const GramArgs &a, uint32_t rank) { return a.kept_idx != nullptr ? a.kept_idx[rank] : rank; }

__device__ __forceinline__ double pick(const double (&t)[4], uint32_t code)
{
    const double lo = (code & 1u) ? t[1] : t[0], hi = (code & 1u) ? t[3] : t[2];
    return (code & 2u) ? hi : lo;
}

__device__ __forceinline__ void put(const GramArgs &a, double *p, double v)
{
    if (a.store) *p = v;
    else if (v != 0.0) unsafeAtomicAdd(p, v);   // global_atomic_add_f64
}

__global__ __launch_bounds__(kThreads) void gt_gram_general_kernel(GramArgs a, uint64_t pairs, uint64_t pair_blocks, uint32_t grid_pairs, uint32_t slices)
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
        double acc = 0.0;
        for (uint64_t j = rbeg; j < rend; j++) {
            const uint8_t *rec = row_record(a, j);
            const double *tj = a.code_values + 4u * j;
            const double t[4] = {tj[0], tj[1], tj[2], tj[3]};
            acc += pick(t, ((uint32_t)rec[ba] >> sha) & 3u) * pick(t, ((uint32_t)rec[bb] >> shb) & 3u);
        }
        put(a, a.out + (uint64_t)i * a.out_stride + l, acc);
    }
}

// what a staging thread holds of one step: the 16 codes of its ranks in its row, and the row's table
struct Staged {
    uint32_t codes;   // rank i of the thread's 16 at bits 2 i
    double t[4];
};

// MODE: rows by stride (0), through variant_idx (1), through record_off (2).  KEPT: ranks go through the kept list
template <int MODE, bool KEPT>
__global__ __launch_bounds__(kThreads, 2) void gt_gram_mfma_kernel(GramArgs a, uint32_t tiles_b, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    __shared__ __attribute__((aligned(16))) double lds[2u * kOperandDoubles];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slice = blockIdx.x / grid_tiles;
    const uint64_t V = a.n_variants;
    const plan::RowRange rows = plan::slice_rows(V, slice, slices);   // never empty (launch plan)
    const uint64_t rbeg = rows.begin, rend = rows.end;
    const uint64_t steps = (rend - rbeg + kStepRows - 1u) / kStepRows;
    // staging role: operand, row of the step, quarter of the tile's ranks
    const uint32_t op = tid >> 7, sr = (tid >> 2) & 31u, q = tid & 3u;
    const uint32_t rot = (q >> 1) | ((sr & 1u) << 1);   // which 16-byte piece of its 128 the thread writes first
    // MFMA role: the wave's 32 x 32 ranks of the tile; the lane's rank of a fragment and its row of a group
    const uint32_t wa = wave >> 1, wb = wave & 1u, m = lane & 15u, k4 = lane >> 4;
    const uint32_t R = a.record_size;

    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint32_t ta = (uint32_t)(tile / tiles_b), tb = (uint32_t)(tile % tiles_b);
        const uint32_t begin = op ? a.b_begin : a.a_begin, count = op ? a.b_count : a.a_count;
        const uint64_t local0 = (uint64_t)(op ? tb : ta) * kTile + 16u * q;   // the thread's first rank, relative to the range
        // which of the 16 ranks exist
        const uint32_t n_valid = local0 < count ? (uint32_t)min((uint64_t)16u, count - local0) : 0u;
        const uint32_t vmask = (1u << n_valid) - 1u;
        // all samples: the five bytes that hold the 16 samples (an index past the record is clamped: its codes are masked)
        // kept list: the byte and the shift of each sample (a rank past the range takes the range's last)
        uint32_t boff[KEPT ? 16 : 5], shifts = 0u;
        if (KEPT) {
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) {
                const uint64_t local = min(local0 + i, (uint64_t)count - 1u);
                const uint32_t s = a.kept_idx[begin + (uint32_t)local];
                boff[i] = s >> 2;
                shifts |= (s & 3u) << (2u * i);
            }
        } else {
            const uint64_t s0 = (uint64_t)begin + local0;
#pragma unroll
            for (uint32_t i = 0; i < 5u; i++) boff[i] = (uint32_t)min((s0 >> 2) + i, (uint64_t)R - 1u);
            shifts = 2u * ((uint32_t)s0 & 3u);
        }

        auto load = [&](uint64_t t, Staged &st) {
            const uint64_t j = rbeg + t * kStepRows + sr;
            const bool live = j < rend;
            const uint64_t row = live ? j : rbeg;
            const uint8_t *rec = a.records + (MODE == 2 ? a.record_off[row] : MODE == 1 ? (uint64_t)a.variant_idx[row] * a.record_stride : row * a.record_stride);
            if (KEPT) {
                uint32_t raw[16];
#pragma unroll
                for (uint32_t i = 0; i < 16u; i++) raw[i] = rec[boff[i]];
                uint32_t c = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 16u; i++) c |= ((raw[i] >> (2u * ((shifts >> (2u * i)) & 3u))) & 3u) << (2u * i);
                st.codes = c;
            } else {
                uint32_t raw[5];
#pragma unroll
                for (uint32_t i = 0; i < 5u; i++) raw[i] = rec[boff[i]];
                const uint64_t w = (uint64_t)(raw[0] | (raw[1] << 8) | (raw[2] << 16) | (raw[3] << 24)) | ((uint64_t)raw[4] << 32);
                st.codes = (uint32_t)(w >> shifts);
            }
            const double *tj = a.code_values + 4u * row;
#pragma unroll
            for (int x = 0; x < 4; x++) st.t[x] = live ? tj[x] : 0.0;   // a row past the slice stages zeros
        };

        gram_v4d acc[2][2][2];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[c][i][j] = gram_v4d{0.0, 0.0, 0.0, 0.0};

        Staged cur;
        load(0u, cur);
        for (uint64_t t = 0; t < steps; t++) {
            // codes -> doubles -> the LDS image
            double *dst = lds + op * kOperandDoubles + sr * kRowStride + 16u * q;
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t piece = (i + rot) & 7u;
                const uint32_t two = cur.codes >> (4u * piece), ok = vmask >> (2u * piece);
                const double v0 = (ok & 1u) ? pick(cur.t, two & 3u) : 0.0;
                const double v1 = (ok & 2u) ? pick(cur.t, (two >> 2) & 3u) : 0.0;
                *reinterpret_cast<gram_v2d *>(dst + 2u * piece) = gram_v2d{v0, v1};
            }
            __syncthreads();
            if (t + 1u < steps) load(t + 1u, cur);   // in flight under the MFMAs

            const double *za = lds + k4 * kRowStride + 32u * wa + m;
            const double *zb = lds + kOperandDoubles + k4 * kRowStride + 32u * wb + m;
#pragma unroll
            for (uint32_t g = 0; g < kStepRows / kGroupRows; g++) {
                const uint32_t o = g * kGroupRows * kRowStride;
                const double fa[2] = {za[o], za[o + 16u]}, fb[2] = {zb[o], zb[o + 16u]};
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) acc[g & 1u][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[g & 1u][i][j], 0, 0, 0);
            }
            __syncthreads();   // the image is read; the next step (or tile) may overwrite it
        }

#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint64_t l = (uint64_t)tb * kTile + 32u * wb + 16u * (uint32_t)j + m;
#pragma unroll
                for (uint32_t reg = 0; reg < 4u; reg++) {
                    const uint64_t ia = (uint64_t)ta * kTile + 32u * wa + 16u * (uint32_t)i + k4 + 4u * reg;
                    if (ia >= a.a_count || l >= a.b_count) continue;
                    put(a, a.out + ia * a.out_stride + l, acc[0][i][j][reg] + acc[1][i][j][reg]);
                }
            }
    }
}

template <int MODE>
void launch_mfma(const GramArgs &a, dim3 grid, uint32_t tiles_b, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream)
{
    if (a.kept_idx != nullptr)
        hipLaunchKernelGGL((gt_gram_mfma_kernel<MODE, true>), grid, dim3(kThreads), 0, stream, a, tiles_b, tiles, grid_tiles, slices);
    else
        hipLaunchKernelGGL((gt_gram_mfma_kernel<MODE, false>), grid, dim3(kThreads), 0, stream, a, tiles_b, tiles, grid_tiles, slices);
}

}  // namespace

hipError_t launch_gt_gram_general(const GramArgs &a, uint32_t slices, hipStream_t stream)
{
    if (a.n_variants == 0 || a.a_count == 0 || a.b_count == 0) return hipSuccess;
    const uint64_t pairs = (uint64_t)a.a_count * a.b_count;
    const uint32_t grid_pairs = plan::gram::grid_pairs(a.a_count, a.b_count);
    hipLaunchKernelGGL(gt_gram_general_kernel, dim3(grid_pairs * slices), dim3(kThreads), 0, stream, a, pairs, pair_blocks(a.a_count, a.b_count), grid_pairs, slices);
    return hipGetLastError();
}

hipError_t launch_gt_gram_mfma(const GramArgs &a, uint32_t slices, hipStream_t stream)
{
    if (a.n_variants == 0 || a.a_count == 0 || a.b_count == 0) return hipSuccess;
    const uint32_t tiles_b = range_tiles(a.b_count);
    const uint64_t tiles = plan::gram::tiles(a.a_count, a.b_count);
    const uint32_t grid_tiles = plan::gram::grid_tiles(a.a_count, a.b_count);
    const dim3 grid(grid_tiles * slices);
    if (a.record_off != nullptr)
        launch_mfma<2>(a, grid, tiles_b, tiles, grid_tiles, slices, stream);
    else if (a.variant_idx != nullptr)
        launch_mfma<1>(a, grid, tiles_b, tiles, grid_tiles, slices, stream);
    else
        launch_mfma<0>(a, grid, tiles_b, tiles, grid_tiles, slices, stream);
    return hipGetLastError();
}

}  // namespace pgenhip
