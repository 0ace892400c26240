// gt_vsum.hip — per-variant sums of per-sample values, split by genotype code, for gfx950 (MI355X): for every selected row j, value
// column c < C and code x in {0, 1, 2, 3} the FP64 sum over the kept samples k whose code in row j is x of values[k * v_stride + c]
// (src/pfile.rs:172-183: sample s in byte s/4, bits 2*(s%4)).  The transpose of gt_score.hip: there the sums are per sample and
// rows are summed, here they are per row and samples are summed, so the partial sums of one row must meet across the lanes that hold
// its samples.
//
// Arithmetic: a term is a value itself (no product), every addition is FP64, no f32 partial sums anywhere.  The order of the
// additions is not fixed (samples are dealt to lanes, tiles of one row meet in global FP64 atomics), so two runs may differ in the
// last bits.  Unkept samples, samples at or past N and pad bits contribute exact zeros or nothing.
//
// GENERAL: one wave per (row, column), the rest by grid stride.  Lanes walk the row's bytes, pick the four code accumulators by
// select, a wave reduction follows and lane 0 stores the four doubles.  Any layout, any keep set; every output has one owner.
//
// MFMA: the FP64 matrix core does the reduction over samples.  D (16 x 16) += A (16 x 4) B (4 x 16) with v_mfma_f64_16x16x4_f64:
//   M = value column (hence at most 16 columns), K = the 4 samples of ONE record byte, N = 16 (row, code) pairs of 4 rows.
//   A[m][k] = value of column m for sample k of the byte; 0.0 for an unkept sample, a sample >= N or a column >= C
//   B[k][n] = 1.0 if sample k of row n / 4 has code n % 4, else 0.0   (v_bfe_u32, v_cmp, one v_cndmask of the high word)
// A does not depend on the row: a work item is (tile of kTileBytes record bytes, slice of rows); the block loads the tile's A once
// (through the ctx's kept mask and kept-before table, as gt_score.hip's flush) into kTileBytes registers per lane and its waves walk
// the slice's groups of 4 rows, one MFMA per record byte into two alternating accumulators.  The last tile of a row is moved back
// to END at the record's last byte (no byte at or past R is read) and the bytes it then shares with the tile before have A = 0.
// Tiles of one row meet through FP64 atomics on the sums (zeroed by a hipMemsetAsync ahead of the kernel; zero results skipped);
// when one tile covers the row every sum has one owner and is stored.  Operand and result lanes (lane l):
//   A: m = l & 15, k = l >> 4;   B: k = l >> 4, n = l & 15;   D register i: m = (l >> 4) + 4 i, n = l & 15
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::vsum;   // kThreads, kWaves, kTileBytes, kGroupRows, ... and the launch plan

typedef double vsum_v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void gt_vsum_general_kernel(VsumArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kThreads) >> 6;
    const uint32_t N = a.sample_count, R = a.record_size, C = a.n_columns;
    const uint64_t items = (uint64_t)a.n_variants * C;
    for (uint64_t item = wave; item < items; item += n_waves) {
        const uint64_t row = item / C;
        const uint32_t c = (uint32_t)(item % C);
        const uint8_t *rec = row_record(a, row);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t b = lane; b < R; b += 64u) {
            const uint32_t byte = rec[b];
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t s = 4u * b + i;
                if (s >= N) break;   // pad bits
                bool kept;
                const uint32_t k = kept_rank_of(a.kept_mask, a.kept_rank, s, kept);
                if (!kept) continue;
                const double v = a.values[(uint64_t)k * a.v_stride + c];
                const uint32_t code = (byte >> (2u * i)) & 3u;
#pragma unroll
                for (uint32_t x = 0; x < 4u; x++) acc[x] += code == x ? v : 0.0;
            }
        }
#pragma unroll
        for (uint32_t x = 0; x < 4u; x++)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[x] += __shfl_xor(acc[x], off, 64);
        if (lane == 0u) {
            double *dst = a.sums + 4ull * item;
            dst[0] = acc[0];
            dst[1] = acc[1];
            dst[2] = acc[2];
            dst[3] = acc[3];
        }
    }
}

struct RowBytes {
    uint32_t w[kTileBytes / 4u];   // the tile's bytes of the lane's row, little-endian
};

__global__ __launch_bounds__(kThreads) void gt_vsum_mfma_kernel(VsumArgs a, uint32_t tiles, uint32_t slices)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15u, k4 = lane >> 4;           // A: column, sample of the byte
    const uint32_t rg = (lane & 15u) >> 2, x = lane & 3u;    // B: row of the group, code
    const uint32_t N = a.sample_count, R = a.record_size, C = a.n_columns;
    const uint64_t V = a.n_variants;
    const uint32_t items = tiles * slices;

    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t tile = item % tiles, slice = item / tiles;
        const plan::RowRange slice_groups = plan::slice_rows(groups(V), slice, slices);
        const uint64_t gbeg = slice_groups.begin, gend = slice_groups.end;
        const uint32_t b0 = tile * kTileBytes;                                   // the tile's own bytes are [b0, b0 + kTileBytes) of the record
        const uint32_t at = R >= kTileBytes ? min(b0, R - kTileBytes) : 0u;      // ... and it reads [at, at + kTileBytes) (block-uniform)

        // the tile's A operand: one double per record byte
        double av[kTileBytes];
#pragma unroll
        for (uint32_t t = 0; t < kTileBytes; t++) {
            const uint32_t byte = at + t;
            const uint64_t s64 = 4ull * byte + k4;
            double v = 0.0;
            if (byte >= b0 && byte < R && s64 < N && m < C) {
                bool kept;
                const uint32_t k = kept_rank_of(a.kept_mask, a.kept_rank, (uint32_t)s64, kept);
                if (kept) v = a.values[(uint64_t)k * a.v_stride + m];
            }
            av[t] = v;
        }

        // the lane's row bytes of one group; a group past the slice reads the slice's first row and is not written
        auto load = [&](uint64_t g, RowBytes &rb) {
            const uint64_t j = g * kGroupRows + rg;
            const uint64_t row = g < gend && j < V ? j : gbeg * kGroupRows;
            const uint8_t *rec = row_record(a, row);
            if (R >= kTileBytes) {   // (block-uniform)
                __builtin_memcpy(rb.w, rec + at, kTileBytes);   // any address
            } else {
#pragma unroll
                for (uint32_t q = 0; q < kTileBytes / 4u; q++) rb.w[q] = 0u;
#pragma unroll
                for (uint32_t t = 0; t < kTileBytes; t++)
                    if (t < R) rb.w[t >> 2] |= (uint32_t)rec[t] << (8u * (t & 3u));
            }
        };

        RowBytes cur, nxt;
        if (gbeg + wave < gend) load(gbeg + wave, cur);
        for (uint64_t g = gbeg + wave; g < gend; g += kWaves) {
            load(g + kWaves, nxt);
            vsum_v4d d0 = {0.0, 0.0, 0.0, 0.0}, d1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (uint32_t t = 0; t < kTileBytes; t += 2u) {
                const uint32_t c0 = (cur.w[t >> 2] >> (8u * (t & 3u) + 2u * k4)) & 3u;
                const uint32_t c1 = (cur.w[(t + 1u) >> 2] >> (8u * ((t + 1u) & 3u) + 2u * k4)) & 3u;
                const double o0 = __hiloint2double(c0 == x ? 0x3FF00000 : 0, 0), o1 = __hiloint2double(c1 == x ? 0x3FF00000 : 0, 0);
                d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], o0, d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t + 1u], o1, d1, 0, 0, 0);
            }
            const uint64_t j = g * kGroupRows + rg;
            if (j < V) {
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const uint32_t col = k4 + 4u * i;
                    const double v = d0[i] + d1[i];
                    if (col < C) {
                        double *dst = a.sums + (j * C + col) * 4ull + x;
                        if (tiles == 1u) *dst = v;
                        else if (v != 0.0) unsafeAtomicAdd(dst, v);   // global_atomic_add_f64
                    }
                }
            }
            cur = nxt;
        }
    }
}

}  // namespace

hipError_t launch_gt_vsum_general(const VsumArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    hipLaunchKernelGGL(gt_vsum_general_kernel, dim3(general_grid(a.n_variants, a.n_columns, num_cus, blocks)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gt_vsum_mfma(const VsumArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    const MfmaPlan p = mfma_plan(a.record_size, a.n_variants, num_cus, blocks);
    hipLaunchKernelGGL(gt_vsum_mfma_kernel, dim3(p.grid), dim3(kThreads), 0, stream, a, p.tiles, p.slices);
    return hipGetLastError();
}

}  // namespace pgenhip
