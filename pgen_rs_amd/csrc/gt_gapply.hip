// gt_gapply.hip — matrix-free Gram product for gfx950 (MI355X): Y = Z^T (Z Q) without Z^T Z.  Z[j][k] = t_j[x_j(k)] over the selected
// rows j and ALL kept samples k (ranks in the kept list), x_j(k) the 2-bit code of that sample in row j (src/pfile.rs:172-183: sample s
// in byte s/4, bits 2*(s%4)), t_j the row's four doubles code_values[4 j .. 4 j + 3]; Q is K x C, C <= 16.  Two passes, each one
// kernel, both reading every record once:
//   P pass:  proj[j][c] = sum over k of Z[j][k] * q[k][c]        (the variants' projections, a documented output)
//   Y pass:  out[k][c]  = sum over j of Z[j][k] * proj[j][c]
// The member of the family gt_vsum / gt_score / gt_gram (X^T w, X v, Z^T Z) that is linear in K: what an eigen-solver iterates.
//
// Arithmetic: every product and every addition is FP64, no f32 partial sums anywhere.  The order of the additions is not fixed (the
// reduction dimension is dealt to lanes or to slices and, inside the matrix core, to two accumulator chains; slices of one tile meet
// in global FP64 atomics), so two runs may differ in the last bits.  Sums whose every partial sum is an integer below 2^53 are exact.
//
// GENERAL: plain multiply-adds.  P pass: a wave per (row, column) and sample slice, lanes stride over the slice's ranks, a wave
// reduction follows.  Y pass: a lane per (rank, column) walks its row slice.  The correctness baseline of the MFMA shape.
//
// MFMA: D (16 x 16) += A (16 x 4) B (4 x 16) with v_mfma_f64_16x16x4_f64 in both passes; lane l holds
//   A[m][k] in (m = l & 15, k = l >> 4);   B[k][n] in (k = l >> 4, n = l & 15);   D register i: row (l >> 4) + 4 i, column l & 15
// P pass: M = 16 rows, N = the 16 columns, k = 4 samples.  A block of four waves owns kRowTile = 64 rows (16 per wave) and one range of
//   samples (a "slice", whole units of kStepSamples = 64).  Per step the block stages a 64 x 16 tile of Q in LDS once for its 64 rows
//   (columns >= C and ranks past the slice stage 0.0), and every lane holds its row's table and the 16 codes it expands: without a
//   kept list the 64 samples are 16 consecutive record bytes, of which lane (m, k) uses bit pair k of every byte (one 16-byte load
//   where it stays inside the record, else clamped byte loads); through a kept list 16 list entries and 16 bytes.  16 MFMAs per
//   step and wave into two alternating chains; the next step's Q and codes are loaded before them.
// Y pass: M = 16 samples, N = the 16 columns, k = 4 rows.  A block owns kSampleTile = 256 ranks (64 per wave: four M tiles that share
//   each B fragment) and one range of rows.  Per step of kStepRows = 64 rows the block stages their 64 x 16 tile of proj and their
//   tables in LDS; a lane reads, per group of four rows, its row's 16 bytes (or four bytes through the kept list) and takes Z
//   straight from the staged tables, indexed by (row, code): no select chain.  64 MFMAs per step and wave.
// A value expanded for a rank or row that does not exist meets a staged 0.0 or lands in a D entry that is not written.
// Epilogue: a pass with one slice that overwrites stores its entries; everything else adds the non-zero ones with
// global_atomic_add_f64 (the target holds +0.0 or a sum).  Compiled per row selection (stride, variant list, byte offsets) and per
// sample selection (all, kept list), so that no load sits under a divergent branch.  All offsets are 64-bit.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::gapply;   // kThreads, kWaves, kRowTile, kStepSamples, kSampleTile, kStepRows and the slices
constexpr uint32_t kCols = 16;  // columns of a staged tile (PGENHIP_GAPPLY_MAX_COLUMNS)

typedef double gapply_v4d __attribute__((ext_vector_type(4)));
typedef double gapply_v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t sample_of(const GapplyArgs &a, uint64_t rank) { return a.kept_idx != nullptr ? a.kept_idx[rank] : (uint32_t)rank; }

__device__ __forceinline__ double pick(const double (&t)[4], uint32_t code)
{
    const double lo = (code & 1u) ? t[1] : t[0], hi = (code & 1u) ? t[3] : t[2];
    return (code & 2u) ? hi : lo;
}

__device__ __forceinline__ void put(uint32_t store, double *p, double v)
{
    if (store) *p = v;
    else if (v != 0.0) unsafeAtomicAdd(p, v);   // global_atomic_add_f64
}

template <int MODE>
__device__ __forceinline__ const uint8_t *record_of(const GapplyArgs &a, uint64_t row)
{
    return a.records + (MODE == 2 ? a.record_off[row] : MODE == 1 ? (uint64_t)a.variant_idx[row] * a.record_stride : row * a.record_stride);
}

// ---- GENERAL -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gt_gapply_p_general_kernel(GapplyArgs a, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t C = a.n_columns;
    const uint64_t items = (uint64_t)a.n_variants * C;
    const plan::RowRange s = slice_samples(a.kept_count, blockIdx.x / grid_tiles, slices);
    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint64_t item = tile * kWaves + wave;
        if (item >= items) break;   // wave-uniform
        const uint64_t row = item / C;
        const uint32_t c = (uint32_t)(item % C);
        const uint8_t *rec = row_record(a, row);
        const double *tj = a.code_values + 4u * row;
        const double t[4] = {tj[0], tj[1], tj[2], tj[3]};
        double acc = 0.0;
        for (uint64_t k = s.begin + lane; k < s.end; k += 64u) {
            const uint32_t smp = sample_of(a, k);
            acc += pick(t, ((uint32_t)rec[smp >> 2] >> (2u * (smp & 3u))) & 3u) * a.q[k * a.q_stride + c];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0u) put(a.p_store, a.proj + item, acc);
    }
}

__global__ __launch_bounds__(kThreads) void gt_gapply_y_general_kernel(GapplyArgs a, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    const uint32_t C = a.n_columns;
    const uint64_t entries = (uint64_t)a.kept_count * C;
    const plan::RowRange rows = plan::slice_rows(a.n_variants, blockIdx.x / grid_tiles, slices);
    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint64_t e = tile * kThreads + threadIdx.x;
        if (e >= entries) break;
        const uint64_t k = e / C;
        const uint32_t c = (uint32_t)(e % C);
        const uint32_t smp = sample_of(a, k), byte = smp >> 2, sh = 2u * (smp & 3u);
        double acc = 0.0;
        for (uint64_t j = rows.begin; j < rows.end; j++) {
            const uint8_t *rec = row_record(a, j);
            const double *tj = a.code_values + 4u * j;
            const double t[4] = {tj[0], tj[1], tj[2], tj[3]};
            acc += pick(t, ((uint32_t)rec[byte] >> sh) & 3u) * a.proj[j * C + c];
        }
        put(a.y_store, a.out + k * a.out_stride + c, acc);
    }
}

// ---- MFMA ----------------------------------------------------------------------------------------------------------------------------
// 16 record bytes from byte b0 of a record of R bytes as four little-endian words; a byte at or past R repeats the record's last
__device__ __forceinline__ void load16(const uint8_t *rec, uint32_t b0, uint32_t R, bool inside, uint32_t (&w)[4])
{
    if (inside) {   // (wave-uniform)
        __builtin_memcpy(w, rec + b0, 16);   // any address
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) w[q] = 0u;
#pragma unroll
        for (uint32_t g = 0; g < 16u; g++) w[g >> 2] |= (uint32_t)rec[min(b0 + g, R - 1u)] << (8u * (g & 3u));
    }
}

// what a lane holds of one P-pass step: its four doubles of the Q tile and the codes of its row
struct PStaged {
    double q[4];
    uint32_t w[4];   // all samples: the step's 16 record bytes >> 2 k (code of group g at bits 8 g); kept list: w[0] holds code g at bits 2 g
};

// MODE: rows by stride (0), through variant_idx (1), through record_off (2).  KEPT: ranks go through the kept list
template <int MODE, bool KEPT>
__global__ __launch_bounds__(kThreads, 2) void gt_gapply_p_mfma_kernel(GapplyArgs a, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    __shared__ __attribute__((aligned(16))) double qt[kStepSamples * kCols];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = lane & 15u, k4 = lane >> 4;
    const uint32_t ss = tid >> 2, c0 = 4u * (tid & 3u);   // staging role: sample of the step, first of four columns
    const uint32_t C = a.n_columns, R = a.record_size;
    const uint64_t V = a.n_variants, K = a.kept_count;
    const plan::RowRange sr = slice_samples(K, blockIdx.x / grid_tiles, slices);   // never empty (launch plan)
    const uint64_t kbeg = sr.begin, kend = sr.end;
    const uint64_t steps = (kend - kbeg + kStepSamples - 1u) / kStepSamples;

    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint64_t row0 = tile * kRowTile + 16u * wave;
        const bool live = row0 + m < V;
        const uint64_t row = live ? row0 + m : V - 1u;   // a row past the end expands a real row into a D row that is not written
        const uint8_t *rec = record_of<MODE>(a, row);
        const double *tj = a.code_values + 4u * row;
        const double t[4] = {tj[0], tj[1], tj[2], tj[3]};

        auto load = [&](uint64_t step, PStaged &st) {
            const uint64_t s0 = kbeg + step * kStepSamples;   // a multiple of kStepSamples
            const uint64_t rank = s0 + ss;
            const bool ok = rank < kend;
            const double *qr = a.q + (ok ? rank : kbeg) * a.q_stride;
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t col = c0 + i;
                const double v = qr[col < C ? col : 0u];
                st.q[i] = (ok && col < C) ? v : 0.0;
            }
            if (KEPT) {
                uint32_t c = 0u;   // folded as the bytes arrive: no per-thread arrays (the compiler had put them in LDS)
#pragma unroll
                for (uint32_t g = 0; g < 16u; g++) {
                    const uint32_t s = a.kept_idx[min(s0 + 4u * g + k4, K - 1u)];
                    c |= (((uint32_t)rec[s >> 2] >> (2u * (s & 3u))) & 3u) << (2u * g);
                }
                st.w[0] = c;
            } else {
                const uint32_t b0 = (uint32_t)(s0 >> 2);
                load16(rec, b0, R, (uint64_t)b0 + 16u <= R, st.w);
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) st.w[i] >>= 2u * k4;
            }
        };

        gapply_v4d acc[2] = {gapply_v4d{0.0, 0.0, 0.0, 0.0}, gapply_v4d{0.0, 0.0, 0.0, 0.0}};
        PStaged cur;
        load(0u, cur);
        for (uint64_t step = 0; step < steps; step++) {
            double *dst = qt + ss * kCols + c0;
            *reinterpret_cast<gapply_v2d *>(dst) = gapply_v2d{cur.q[0], cur.q[1]};
            *reinterpret_cast<gapply_v2d *>(dst + 2) = gapply_v2d{cur.q[2], cur.q[3]};
            __syncthreads();
            PStaged nxt = cur;
            if (step + 1u < steps) load(step + 1u, nxt);   // in flight under the MFMAs
            const double *qb = qt + k4 * kCols + m;
#pragma unroll
            for (uint32_t g = 0; g < 16u; g++) {
                const uint32_t code = KEPT ? (cur.w[0] >> (2u * g)) & 3u : (cur.w[g >> 2] >> (8u * (g & 3u))) & 3u;
                acc[g & 1u] = __builtin_amdgcn_mfma_f64_16x16x4f64(pick(t, code), qb[g * kGroup * kCols], acc[g & 1u], 0, 0, 0);
            }
            __syncthreads();   // the tile is read; the next step (or row tile) may overwrite it
            cur = nxt;
        }

        if (m < C) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint64_t prow = row0 + k4 + 4u * i;
                if (prow < V) put(a.p_store, a.proj + prow * C + m, acc[0][i] + acc[1][i]);
            }
        }
    }
}

template <int MODE, bool KEPT>
__global__ __launch_bounds__(kThreads, 2) void gt_gapply_y_mfma_kernel(GapplyArgs a, uint64_t tiles, uint32_t grid_tiles, uint32_t slices)
{
    __shared__ __attribute__((aligned(16))) double pt[kStepRows * kCols];
    __shared__ __attribute__((aligned(16))) double tab[kStepRows * 4u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = lane & 15u, k4 = lane >> 4;
    const uint32_t srow = tid >> 2, c0 = 4u * (tid & 3u);   // staging role: row of the step, first of four columns (and the table entry tid & 3)
    const uint32_t C = a.n_columns, R = a.record_size;
    const uint64_t V = a.n_variants, K = a.kept_count;
    const plan::RowRange rows = plan::slice_rows(V, blockIdx.x / grid_tiles, slices);   // never empty (launch plan)
    const uint64_t rbeg = rows.begin, rend = rows.end;
    const uint64_t steps = (rend - rbeg + kStepRows - 1u) / kStepRows;

    for (uint64_t tile = blockIdx.x % grid_tiles; tile < tiles; tile += grid_tiles) {
        const uint64_t s0 = tile * kSampleTile + 64u * wave;   // the wave's first rank, a multiple of 64
        // all samples: the wave's 64 samples are 16 record bytes from b0, sample 16 u + m at bits 2 m of word u
        // kept list: the byte and the shift of the lane's four samples (a rank past K takes the last)
        const uint32_t b0 = (uint32_t)min(s0 >> 2, (uint64_t)R);
        const bool inside = (uint64_t)b0 + 16u <= R;
        uint32_t boff[4] = {0u, 0u, 0u, 0u}, bsh[4] = {0u, 0u, 0u, 0u};
        if (KEPT) {
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t s = a.kept_idx[min(s0 + 16u * u + m, K - 1u)];
                boff[u] = s >> 2;
                bsh[u] = 2u * (s & 3u);
            }
        }

        double sp[4], st;
        auto load = [&](uint64_t step) {
            const uint64_t j = rbeg + step * kStepRows + srow;
            const bool ok = j < rend;
            const uint64_t r = ok ? j : rbeg;
            const double *pr = a.proj + r * C;
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t col = c0 + i;
                const double v = pr[col < C ? col : 0u];
                sp[i] = (ok && col < C) ? v : 0.0;
            }
            const double tv = a.code_values[4u * r + (tid & 3u)];
            st = ok ? tv : 0.0;   // a row past the slice stages zeros
        };

        gapply_v4d acc[2][4];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int u = 0; u < 4; u++) acc[c][u] = gapply_v4d{0.0, 0.0, 0.0, 0.0};

        load(0u);
        for (uint64_t step = 0; step < steps; step++) {
            double *dst = pt + srow * kCols + c0;
            *reinterpret_cast<gapply_v2d *>(dst) = gapply_v2d{sp[0], sp[1]};
            *reinterpret_cast<gapply_v2d *>(dst + 2) = gapply_v2d{sp[2], sp[3]};
            tab[tid] = st;
            __syncthreads();
            if (step + 1u < steps) load(step + 1u);   // in flight under the MFMAs
            const uint64_t j0 = rbeg + step * kStepRows + k4;
            if (s0 < K)   // (wave-uniform) a wave whose 64 ranks all lie past K loads and multiplies nothing; it still stages and syncs
            for (uint32_t gg = 0; gg < kStepRows / kGroup; gg += 4u)
#pragma unroll
            for (uint32_t gi = 0; gi < 4u; gi++) {   // four groups' loads in flight; gi picks the accumulator chain
                const uint32_t g = gg + gi;
                const uint64_t j = j0 + kGroup * g;
                const uint8_t *rec = record_of<MODE>(a, j < rend ? j : rend - 1u);   // (its staged table and proj are zeros)
                uint32_t code[4];
                if (KEPT) {
#pragma unroll
                    for (uint32_t u = 0; u < 4u; u++) code[u] = ((uint32_t)rec[boff[u]] >> bsh[u]) & 3u;
                } else {
                    uint32_t w[4];
                    load16(rec, b0, R, inside, w);
#pragma unroll
                    for (uint32_t u = 0; u < 4u; u++) code[u] = (w[u] >> (2u * m)) & 3u;
                }
                const double b = pt[(kGroup * g + k4) * kCols + m];
                const double *tr = tab + (kGroup * g + k4) * 4u;
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++) acc[gi & 1u][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[code[u]], b, acc[gi & 1u][u], 0, 0, 0);
            }
            __syncthreads();   // the tiles are read; the next step (or sample tile) may overwrite them
        }

        if (m < C) {
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const uint64_t rank = s0 + 16u * u + k4 + 4u * i;
                    if (rank < K) put(a.y_store, a.out + rank * a.out_stride + m, acc[0][u][i] + acc[1][u][i]);
                }
        }
    }
}

template <int MODE>
void launch_mfma(const GapplyArgs &a, bool y_pass, dim3 grid, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream)
{
    if (y_pass) {
        if (a.kept_idx != nullptr)
            hipLaunchKernelGGL((gt_gapply_y_mfma_kernel<MODE, true>), grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
        else
            hipLaunchKernelGGL((gt_gapply_y_mfma_kernel<MODE, false>), grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
    } else {
        if (a.kept_idx != nullptr)
            hipLaunchKernelGGL((gt_gapply_p_mfma_kernel<MODE, true>), grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
        else
            hipLaunchKernelGGL((gt_gapply_p_mfma_kernel<MODE, false>), grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
    }
}

hipError_t launch_pass(const GapplyArgs &a, bool mfma, bool y_pass, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0 || a.n_columns == 0) return hipSuccess;
    const dim3 grid(grid_tiles * slices);
    if (!mfma) {
        if (y_pass)
            hipLaunchKernelGGL(gt_gapply_y_general_kernel, grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
        else
            hipLaunchKernelGGL(gt_gapply_p_general_kernel, grid, dim3(kThreads), 0, stream, a, tiles, grid_tiles, slices);
    } else if (a.record_off != nullptr) {
        launch_mfma<2>(a, y_pass, grid, tiles, grid_tiles, slices, stream);
    } else if (a.variant_idx != nullptr) {
        launch_mfma<1>(a, y_pass, grid, tiles, grid_tiles, slices, stream);
    } else {
        launch_mfma<0>(a, y_pass, grid, tiles, grid_tiles, slices, stream);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gt_gapply_p(const GapplyArgs &a, bool mfma, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream)
{
    return launch_pass(a, mfma, false, tiles, grid_tiles, slices, stream);
}

hipError_t launch_gt_gapply_y(const GapplyArgs &a, bool mfma, uint64_t tiles, uint32_t grid_tiles, uint32_t slices, hipStream_t stream)
{
    return launch_pass(a, mfma, true, tiles, grid_tiles, slices, stream);
}

}  // namespace pgenhip
