// gt_scount.hip — per-sample genotype counts for gfx950 (MI355X): for every kept sample the number of selected rows in which it
// has code 0 (hom-ref "0/0"), 1 (het "0/1"), 2 (hom-alt "1/1") and 3 (missing "./."): the per-variant counts of gt_count.hip
// summed the other way, across rows instead of along them (src/pfile.rs:172-183: sample s in byte s/4, bits 2*(s%4)).
//
// A read-bound reduction with no horizontal popcount to lean on: a lane owns one fixed 16-byte column chunk of the rows (64
// samples) and walks rows, adding one 0/1 per sample and category per row.  Per row and chunk (dwords w0..w3, m = 0x55555555):
//   L0 = (w0 & m) | ((w1 << 1) & ~m),  H0 = ((w0 >> 1) & m) | (w1 & ~m)      (v_bfi_b32: 32 samples' low / high code bits)
//   L1, H1 alike from w2, w3;  M = L & H (missing)
// and het = #L - #M, hom-alt = #H - #M, missing = #M.  The six bit vectors go into bit-sliced (vertical) counters, eight rows at
// a time through a carry-save adder tree (Harley-Seal: 7 adders of 3 VALU each per 8 rows and vector, then the weight-8 carry
// rippled into an 8-bit batch counter), so a counter holds 2 047 rows; every 255 batches (2 040 rows) and at the end the
// counters are turned into integers and added into the block's LDS table.  Hom-ref is never counted: the block that owns row
// range 0 of a column tile adds n_variants to each hom-ref word, every block subtracts its het + hom-alt + missing (u32 modular).
//
// Rows are read as gt_count.hip reads them (aligned non-temporal 16-byte loads, any record alignment, gathers, byte offsets):
// lane g of a row's group loads aligned chunk g + 1 of the row's span, takes chunk g from the lane below (DPP wave_shr:1; the
// group's first lane loads it itself) and funnels the pair into row bytes [16g, 16g + 16) (v_alignbyte_b32).  Bytes at or past R
// belong to samples >= N, which are never flushed.
//
// Launch plan: G = 4 .. 64 lanes per row (the fewest that cover a row's column chunks; 64 and column tiles of 1 KiB past that),
// 64 / G rows per wave side by side.  A block owns one column tile and one contiguous range of rows (a "slice"); its 4 waves
// share one LDS table (3 words per sample of the tile, 65 words per 64-sample column so that the lanes of a wave hit distinct
// banks), which is flushed once with global atomics of 64 consecutive count words per wave instruction.  Slices per tile: as
// many as fill the chip's resident blocks, so each sample gets at most a few thousand partials.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::scount;   // kThreads, kBatch, kHiBits, kWindowBatches, kColWords, ... and the launch plan

// 32 samples' counts, bit-sliced: ones + 2 twos + 4 fours + 8 * hi (hi a kHiBits-bit number)
struct Slice {
    uint32_t ones, twos, fours, hi[kHiBits];
};

// full adder on 32 lanes of bits: l = a ^ b ^ c, h = majority (v_bfi_b32)
__device__ __forceinline__ void csa(uint32_t &h, uint32_t &l, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t t = a ^ b;
    l = t ^ c;
    h = (t & c) | (~t & a);
}

// eight rows' bit vectors into the counter
__device__ __forceinline__ void add8(Slice &s, const uint32_t (&x)[kBatch])
{
    uint32_t twos_a, twos_b, fours_a, fours_b, eights;
    csa(twos_a, s.ones, s.ones, x[0], x[1]);
    csa(twos_b, s.ones, s.ones, x[2], x[3]);
    csa(fours_a, s.twos, s.twos, twos_a, twos_b);
    csa(twos_a, s.ones, s.ones, x[4], x[5]);
    csa(twos_b, s.ones, s.ones, x[6], x[7]);
    csa(fours_b, s.twos, s.twos, twos_a, twos_b);
    csa(eights, s.fours, s.fours, fours_a, fours_b);
#pragma unroll
    for (int i = 0; i < kHiBits; i++) {
        const uint32_t carry = s.hi[i] & eights;
        s.hi[i] ^= eights;
        eights = carry;
    }
}

__device__ __forceinline__ void clear(Slice &s)
{
    s.ones = s.twos = s.fours = 0u;
#pragma unroll
    for (int i = 0; i < kHiBits; i++) s.hi[i] = 0u;
}

// the count of bit p; hi planes at or above n_hi are known zero (n_hi is block-uniform)
__device__ __forceinline__ uint32_t value(const Slice &s, uint32_t p, int n_hi)
{
    uint32_t v = 0u;
#pragma unroll
    for (int i = kHiBits - 1; i >= 0; i--)
        if (i < n_hi) v = (v << 1) | ((s.hi[i] >> p) & 1u);
    v = (v << 1) | ((s.fours >> p) & 1u);
    v = (v << 1) | ((s.twos >> p) & 1u);
    return (v << 1) | ((s.ones >> p) & 1u);
}

template <int G>
__global__ __launch_bounds__(kThreads) void gt_scount_kernel(ScountArgs a, uint32_t tiles, uint32_t slices, uint32_t cols)
{
    extern __shared__ uint32_t table[];   // [3][cols * kColWords]: het, hom-alt, missing of the tile's samples
    constexpr uint32_t kGroups = 64u / G;
    constexpr uint32_t kSlots = slots(G);   // rows side by side in the block
    const uint32_t lane = threadIdx.x & 63u, gl = lane % (uint32_t)G;
    const uint32_t slot = (threadIdx.x >> 6) * kGroups + lane / (uint32_t)G;
    const uint32_t tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
    const uint32_t col = tile * (uint32_t)G + gl;   // this lane's column chunk: row bytes [16 col, 16 col + 16)
    const uint32_t N = a.sample_count, R = a.record_size;
    const uint64_t V = a.n_variants;
    const plan::RowRange rows = plan::slice_rows(V, slice, slices);
    const uint64_t rbeg = rows.begin, rend = rows.end;
    const uint32_t plane = cols * kColWords;

    for (uint32_t i = threadIdx.x; i < 3u * plane; i += kThreads) table[i] = 0u;
    __syncthreads();

    const uint64_t steps = (rend - rbeg + kSlots - 1u) / kSlots;   // rows per slot, rounded up (block-uniform)
    const bool owner = 64ull * col < N;                             // the lane's chunk holds samples of the row
    for (uint64_t t0 = 0; t0 < steps; t0 += (uint64_t)kBatch * kWindowBatches) {
        Slice cnt[6];   // L0 H0 M0 L1 H1 M1
#pragma unroll
        for (int v = 0; v < 6; v++) clear(cnt[v]);
        const uint64_t t_end = min<uint64_t>(steps, t0 + (uint64_t)kBatch * kWindowBatches);
        for (uint64_t t = t0; t < t_end; t += kBatch) {
            gt_v4u hi[kBatch], lo[kBatch];
            uint32_t d[kBatch];
#pragma unroll
            for (uint32_t b = 0; b < kBatch; b++) {
                const uint64_t row = rbeg + (t + b) * kSlots + slot;
                const bool live = t + b < t_end && row < rend;
                const uint8_t *rec = live ? row_record(a, row) : a.records;
                d[b] = (uint32_t)(uintptr_t)rec & 15u;
                const uint8_t *base = rec - d[b];   // (pointer arithmetic on the argument keeps the loads global, not flat)
                const uint32_t nch = live ? (d[b] + R + 15u) >> 4 : 0u;   // aligned chunks the row's bytes touch
                hi[b] = col + 1u < nch ? load_nt16(base + 16ull * (col + 1u)) : gt_v4u{0u, 0u, 0u, 0u};
                lo[b] = gl == 0u && col < nch ? load_nt16(base + 16ull * col) : gt_v4u{0u, 0u, 0u, 0u};
            }
            uint32_t x[6][kBatch];
#pragma unroll
            for (uint32_t b = 0; b < kBatch; b++) {
                const gt_v4u lower = dpp_from_lower_lane(hi[b], lo[b]);
                const gt_v4u w = funnel16(G == 64 || gl != 0u ? lower : lo[b], hi[b], d[b]);
                constexpr uint32_t m = 0x55555555u;
                x[0][b] = (w[0] & m) | ((w[1] << 1) & ~m);
                x[1][b] = ((w[0] >> 1) & m) | (w[1] & ~m);
                x[2][b] = x[0][b] & x[1][b];
                x[3][b] = (w[2] & m) | ((w[3] << 1) & ~m);
                x[4][b] = ((w[2] >> 1) & m) | (w[3] & ~m);
                x[5][b] = x[3][b] & x[4][b];
            }
#pragma unroll
            for (int v = 0; v < 6; v++) add8(cnt[v], x[v]);
        }
        // flush the window: batches <= 255, so hi planes past the batch count's bit length are zero
        const uint32_t batches = (uint32_t)((t_end - t0 + kBatch - 1u) / kBatch);
        const int n_hi = hi_planes(batches);
        if (owner) {
            uint32_t *const het = table + gl * kColWords, *const alt = het + plane, *const miss = alt + plane;
#pragma unroll 1
            for (uint32_t p = 0; p < 32u; p++) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t cs = 16u * (2u * h + (p & 1u)) + (p >> 1);   // sample of bit p within the chunk
                    const uint32_t vl = value(cnt[3 * h], p, n_hi), vh = value(cnt[3 * h + 1], p, n_hi), vm = value(cnt[3 * h + 2], p, n_hi);
                    if (vl != vm) atomicAdd(het + cs, vl - vm);
                    if (vh != vm) atomicAdd(alt + cs, vh - vm);
                    if (vm) atomicAdd(miss + cs, vm);
                }
            }
        }
    }
    __syncthreads();

    // the tile's sums -> d_counts: thread e of a pass adds count word e & 3 of tile sample e >> 2, so 64 lanes cover 16 samples'
    // 64 consecutive words (all samples kept; with a subset, the kept ones of those 16)
    const uint32_t hom_ref_rows = slice == 0u ? a.n_variants : 0u;
    for (uint32_t e = threadIdx.x; e < 256u * cols; e += kThreads) {
        const uint32_t ts = e >> 2, c = e & 3u;
        const uint32_t s = tile * 64u * (uint32_t)G + ts;
        if (s >= N) break;
        uint32_t k = s;
        if (a.kept_mask != nullptr) {   // kept_rank_of (gt_common.hip.h), written out: an unkept sample leaves before its rank is formed
            const uint32_t *mw = reinterpret_cast<const uint32_t *>(a.kept_mask + 16u + 16u * (s >> 6));
            const uint32_t j = (s >> 4) & 3u, bit = 2u * (s & 15u);
            if (((mw[j] >> bit) & 1u) == 0u) continue;
            k = a.kept_rank[s >> 6] + __builtin_popcount(mw[j] & ((1u << bit) - 1u));
            for (uint32_t i = 0; i < j; i++) k += __builtin_popcount(mw[i]);
        }
        const uint32_t w = (ts >> 6) * kColWords + (ts & 63u);
        const uint32_t het = table[w], alt = table[plane + w], miss = table[2u * plane + w];
        const uint32_t v = c == 0u ? hom_ref_rows - het - alt - miss : c == 1u ? het : c == 2u ? alt : miss;
        if (v != 0u) atomicAdd(a.counts + 4ull * k + c, v);
    }
}

}  // namespace

hipError_t launch_gt_scount(const ScountArgs &a, int slices_per_tile, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    const Plan p = plan::scount::plan(a.record_size, a.n_variants, num_cus, slices_per_tile);
    const dim3 grid(p.tiles * p.slices), block(kThreads);
    switch (p.G) {
        case 4u: hipLaunchKernelGGL(gt_scount_kernel<4>, grid, block, p.lds_bytes, stream, a, p.tiles, p.slices, p.cols); break;
        case 8u: hipLaunchKernelGGL(gt_scount_kernel<8>, grid, block, p.lds_bytes, stream, a, p.tiles, p.slices, p.cols); break;
        case 16u: hipLaunchKernelGGL(gt_scount_kernel<16>, grid, block, p.lds_bytes, stream, a, p.tiles, p.slices, p.cols); break;
        case 32u: hipLaunchKernelGGL(gt_scount_kernel<32>, grid, block, p.lds_bytes, stream, a, p.tiles, p.slices, p.cols); break;
        default: hipLaunchKernelGGL(gt_scount_kernel<64>, grid, block, p.lds_bytes, stream, a, p.tiles, p.slices, p.cols); break;
    }
    return hipGetLastError();
}

}  // namespace pgenhip
