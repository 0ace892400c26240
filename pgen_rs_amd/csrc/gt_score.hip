// gt_score.hip — per-sample weighted dosage sums (polygenic scores) for gfx950 (MI355X): for every kept sample k and weight column
// c < C the sum over the selected rows j of (double)w[j, c] * D(j, k), D = 0, 1, 2 for codes 0, 1, 2 and (double)miss[j] for code 3
// (src/pfile.rs:172-183: sample s in byte s/4, bits 2*(s%4)).  gt_scount.hip's reduction with a weight per row: the bit-sliced
// counters of that kernel only work because every row weighs 1, so this one decodes each genotype and adds in floating point.
//
// Arithmetic: w and miss are f32; a term w * D is exact in FP64 (24 bits x {1, 2, 24 bits} fits 53), and every term goes into an
// FP64 sum through ONE v_fma_f64 (the exact product and the running sum, rounded once: the same value as forming the term and
// adding it).  No f32 partial sums anywhere.  The order of the additions is not fixed (rows are dealt to lanes by the launch plan,
// lanes meet in LDS atomics, blocks in global atomics), so two runs may differ in the last bits.
//
// A lane owns BYTES consecutive bytes of every row of its slot (4 BYTES samples) and keeps 4 BYTES x C sums in registers (at most
// 64 VGPRs: BYTES = 4 for C <= 2, 2 for C <= 4, 1 for C <= 8).  Per row it loads its bytes (any record alignment; bytes at or past
// R are never read), the row's C weights and miss value (no load sits under a lane-dependent branch), and per genotype decodes D
// ONCE (v_bfe_u32, v_lshl_add_u32 for the high word of 1.0 / 2.0, two compares and three selects) and then issues one v_fma_f64
// per column.  The loads of the next batch of rows are issued before the adds of the current one.
//
// Launch plan: G = 1 .. 64 lanes per row (the fewest that cover a row's units of BYTES bytes; 64 and column tiles of 64 units past
// that), 64 / G rows per wave side by side.  A block owns one column tile and one contiguous range of rows (a "slice"); its lanes
// add their sums into the block's LDS table ([sample of the lane][column][lane of the row]: consecutive lanes, consecutive
// doubles), which is flushed once with global FP64 atomics of consecutive output doubles (zero sums skipped; kept subsets through
// the ctx's mask and kept-before table, as gt_scount.hip).  Lanes whose samples are all dropped or past N re-read row
// bytes that other lanes read anyway, add zeros and flush nothing.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::score;   // kThreads, kWaves, lane_bytes, batch_rows, ... and the launch plan

template <int C>
struct Row {
    uint32_t bits;   // the lane's bytes of the row, little-endian; 0 where there is no row or no byte
    float w[C], m;
};

// D as a double from its 2-bit code: 0.0, 1.0 (0x3FF00000), 2.0 (0x40000000) or the row's miss value
__device__ __forceinline__ double dosage(uint32_t code, int m_hi, int m_lo)
{
    const int hi012 = code == 0u ? 0 : (int)(0x3FE00000u + (code << 20));
    return __hiloint2double(code == 3u ? m_hi : hi012, code == 3u ? m_lo : 0);
}

template <int BYTES, int C>
__global__ __launch_bounds__(kThreads) void gt_score_kernel(ScoreArgs a, uint32_t log_g, uint32_t tiles, uint32_t slices)
{
    constexpr int S = 4 * BYTES;               // samples of a lane
    constexpr uint32_t B = batch_rows(C);
    __shared__ double table[64 * S * C];       // [S][C][G] sums of the tile's samples (at most 16 KiB)
    const uint32_t G = 1u << log_g, groups = 64u >> log_g, slots = plan::score::slots(log_g);   // lanes per row, rows per wave, rows side by side in the block
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (G - 1u);
    const uint32_t slot = (threadIdx.x >> 6) * groups + (lane >> log_g);
    const uint32_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const uint32_t unit = tile * G + gl;       // this lane's row bytes [BYTES unit, BYTES unit + BYTES)
    const uint32_t N = a.sample_count, R = a.record_size;
    const uint64_t V = a.n_variants;
    const plan::RowRange rows = plan::slice_rows(V, slice, slices);
    const uint64_t rbeg = rows.begin, rend = rows.end;

    for (uint32_t i = threadIdx.x; i < G * (uint32_t)(S * C); i += kThreads) table[i] = 0.0;
    __syncthreads();

    const uint64_t b0 = (uint64_t)unit * BYTES;
    bool active = b0 < R;                      // the lane's bytes hold samples of the row
    if (active && a.kept_mask != nullptr) {    // ... and one of them is kept (the mask is record-shaped behind 16 zero bytes)
        uint32_t mk = 0u;
#pragma unroll
        for (int i = 0; i < BYTES; i++) mk |= a.kept_mask[16u + b0 + i];
        active = mk != 0u;
    }

    const uint64_t steps = (rend - rbeg + slots - 1u) / slots;   // rows per slot, rounded up (block-uniform)
    // One batch of rows per slot.  Every lane loads, with no branch that depends on the lane: a lane without a row (or without
    // samples) reads row rbeg (byte 0) and its bits are zeroed, which makes every term fma(w, 0, acc) = acc; bytes at or past R
    // are not read (the wide load is moved back to end at the record's last byte and shifted).
    const uint64_t bb = active ? b0 : 0u;
    auto load = [&](uint64_t t, Row<C> (&r)[B]) {
        uint64_t row[B], off[B];
        bool live[B];
#pragma unroll
        for (uint32_t b = 0; b < B; b++) {
            const uint64_t j = rbeg + (t + b) * slots + slot;
            live[b] = active && t + b < steps && j < rend;
            row[b] = live[b] ? j : rbeg;
        }
        if (a.record_off != nullptr) {
#pragma unroll
            for (uint32_t b = 0; b < B; b++) off[b] = a.record_off[row[b]];
        } else if (a.variant_idx != nullptr) {
#pragma unroll
            for (uint32_t b = 0; b < B; b++) off[b] = (uint64_t)a.variant_idx[row[b]] * a.record_stride;
        } else {
#pragma unroll
            for (uint32_t b = 0; b < B; b++) off[b] = row[b] * a.record_stride;
        }
#pragma unroll
        for (uint32_t b = 0; b < B; b++) {
            const uint8_t *rec = a.records + off[b];
            uint32_t bits = 0u;
            if (BYTES == 1 || R >= (uint32_t)BYTES) {   // (block-uniform)
                const uint64_t at = min(bb, (uint64_t)(R - (uint32_t)BYTES));
                __builtin_memcpy(&bits, rec + at, BYTES);   // one load of 1, 2 or 4 bytes at any address
                bits >>= 8u * (uint32_t)(bb - at);
            } else {
#pragma unroll
                for (int i = 0; i < BYTES; i++) {
                    const uint32_t x = rec[min(bb + i, (uint64_t)(R - 1u))];
                    bits |= bb + i < R ? x << (8 * i) : 0u;
                }
            }
            r[b].bits = live[b] ? bits : 0u;
            const float *w = a.weights + row[b] * a.w_stride;
#pragma unroll
            for (int c = 0; c < C; c++) r[b].w[c] = w[c];
            r[b].m = 0.f;
        }
        if (a.miss != nullptr) {
#pragma unroll
            for (uint32_t b = 0; b < B; b++) r[b].m = a.miss[row[b]];
        }
    };

    double acc[S][C];
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[i][c] = 0.0;

    Row<C> cur[B], nxt[B];
    load(0, cur);
    for (uint64_t t = 0; t < steps; t += B) {
        load(t + B, nxt);
#pragma unroll
        for (uint32_t b = 0; b < B; b++) {
            double wd[C];
#pragma unroll
            for (int c = 0; c < C; c++) wd[c] = (double)cur[b].w[c];
            const double md = (double)cur[b].m;
            const int m_hi = __double2hiint(md), m_lo = __double2loint(md);
#pragma unroll
            for (int i = 0; i < S; i++) {
                const double d = dosage((cur[b].bits >> (2 * i)) & 3u, m_hi, m_lo);
#pragma unroll
                for (int c = 0; c < C; c++) acc[i][c] = __builtin_fma(wd[c], d, acc[i][c]);
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < B; b++) cur[b] = nxt[b];
    }

    // the lanes' sums -> the block's table; samples at or past N (pad bits, bytes that were never loaded) stay out
    if (active) {
#pragma unroll
        for (int i = 0; i < S; i++) {
            if ((uint64_t)unit * S + i < N) {
#pragma unroll
                for (int c = 0; c < C; c++)
                    if (acc[i][c] != 0.0) atomicAdd(&table[(uint32_t)(i * C + c) * G + gl], acc[i][c]);
            }
        }
    }
    __syncthreads();

    // the tile's sums -> d_scores: thread e of a pass adds column e % C of tile sample e / C, so a wave covers consecutive
    // doubles of the output (all samples kept; with a subset, the kept ones among them)
    const uint32_t tile_samples = G * (uint32_t)S;
    for (uint32_t e = threadIdx.x; e < tile_samples * (uint32_t)C; e += kThreads) {
        const uint32_t ts = e / (uint32_t)C, c = e % (uint32_t)C;
        const uint64_t s64 = (uint64_t)tile * tile_samples + ts;
        if (s64 >= N) break;
        const uint32_t s = (uint32_t)s64;
        uint32_t k = s;
        if (a.kept_mask != nullptr) {   // kept_rank_of (gt_common.hip.h), written out: an unkept sample leaves before its rank is formed
            const uint32_t *mw = reinterpret_cast<const uint32_t *>(a.kept_mask + 16u + 16u * (s >> 6));
            const uint32_t j = (s >> 4) & 3u, bit = 2u * (s & 15u);
            if (((mw[j] >> bit) & 1u) == 0u) continue;
            k = a.kept_rank[s >> 6] + __builtin_popcount(mw[j] & ((1u << bit) - 1u));
            for (uint32_t i = 0; i < j; i++) k += __builtin_popcount(mw[i]);
        }
        const double v = table[((ts % (uint32_t)S) * (uint32_t)C + c) * G + ts / (uint32_t)S];
        if (v != 0.0) unsafeAtomicAdd(a.scores + (uint64_t)k * (uint32_t)C + c, v);   // global_atomic_add_f64
    }
}

template <int BYTES, int C>
void launch(const ScoreArgs &a, const Plan &p, hipStream_t stream)
{
    hipLaunchKernelGGL((gt_score_kernel<BYTES, C>), dim3(p.tiles * p.slices), dim3(kThreads), 0, stream, a, p.log_g, p.tiles, p.slices);
}

}  // namespace

hipError_t launch_gt_score(const ScoreArgs &a, int slices_per_tile, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    const Plan p = plan::score::plan(a.record_size, a.n_variants, a.n_columns, num_cus, slices_per_tile);
    switch (a.n_columns) {
        case 1u: launch<4, 1>(a, p, stream); break;
        case 2u: launch<4, 2>(a, p, stream); break;
        case 3u: launch<2, 3>(a, p, stream); break;
        case 4u: launch<2, 4>(a, p, stream); break;
        case 5u: launch<1, 5>(a, p, stream); break;
        case 6u: launch<1, 6>(a, p, stream); break;
        case 7u: launch<1, 7>(a, p, stream); break;
        case 8u: launch<1, 8>(a, p, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pgenhip
