// gt_count.hip — per-variant genotype counts for gfx950 (MI355X): for every selected row j the number of kept samples with
// code 0 (hom-ref "0/0"), 1 (het "0/1"), 2 (hom-alt "1/1") and 3 (missing "./."), i.e. what counting the GT fields of the row's
// VCF text would give (src/pfile.rs:172-183: sample s in byte s/4, bits 2*(s%4)).
//
// A read-bound reduction: the records are read once (aligned, non-temporal 16-byte loads of each row's span) and 16 bytes per
// row are written.  Per 32-bit record word w and mask m (bit 2s set for every counted sample s of the word):
//   lo = w & m, hi = (w >> 1) & m;  het = popc(lo & ~hi), hom-alt = popc(hi & ~lo), missing = popc(lo & hi)
// and hom-ref = K - the three.  m excludes the bytes of neighbouring rows in the first / last aligned chunk of a row and the pad
// bits of the last record byte.  With a kept subset, m comes from the ctx's kept mask (2 bits per sample, 0b01 for a kept
// sample, laid out like a record of N samples behind 16 zero bytes); its chunks are aligned to the mask buffer, not to the row,
// so each lane funnel-shifts the pair (buffer chunk c, buffer chunk c+1) into line with its record chunk (v_alignbyte_b32).
// Buffer chunk c is the neighbouring lane's chunk c+1 (DPP wave_shr:1); the first lane of a row's group loads it itself.
//
// One kernel, two shape classes (the host picks by N):
//   * rows of several hundred chunks: a wave per row, four chunks per lane in flight, one wave reduction and one 16-B store;
//   * short rows: G = 4 .. 32 lanes per row (as many as three passes over the row's chunks need), 64/G rows per wave and two
//     rows per group in flight, so lanes are not idle on 75-byte records.
// Every row's counts are written by one lane: no atomics, no hand-off between blocks, no scratch.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::count;   // kThreads, kBlocksPerCu and the launch plan

// bits [0, 2n) of a word, n in [0, 16]
__device__ __forceinline__ uint32_t low_sample_bits(int32_t n) { return n >= 16 ? 0xFFFFFFFFu : ((1u << (2 * n)) - 1u); }

// mask of the samples of dword j of the aligned chunk whose first byte is row byte i0 (i0 = 16c - d, may be negative): samples
// [0, N) of the row, nothing of the neighbouring rows' bytes, no pad bits
__device__ __forceinline__ uint32_t row_mask(int64_t i0, uint32_t j, uint32_t N)
{
    const int64_t s0 = 4 * (i0 + 4 * (int64_t)j);   // sample index of bit 0 of the dword
    const int32_t lo = (int32_t)min<int64_t>(max<int64_t>(-s0, 0), 16);
    const int32_t hi = (int32_t)min<int64_t>(max<int64_t>((int64_t)N - s0, 0), 16);
    return 0x55555555u & low_sample_bits(hi) & ~low_sample_bits(lo);
}

struct Acc {
    uint32_t het = 0, alt = 0, miss = 0;
};

__device__ __forceinline__ void count16(Acc &acc, gt_v4u w, gt_v4u m)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t lo = w[j] & m[j], hi = (w[j] >> 1) & m[j];
        acc.het += __builtin_popcount(lo & ~hi);   // v_bcnt_u32_b32 adds into the accumulator
        acc.alt += __builtin_popcount(hi & ~lo);
        acc.miss += __builtin_popcount(lo & hi);
    }
}

// G lanes per row, RU rows per group in flight, U chunks per lane per pass; MASK: kept subset through the ctx's kept mask
template <int G, int RU, int U, bool MASK>
__global__ __launch_bounds__(kThreads) void gt_count_kernel(CountArgs a)
{
    constexpr uint32_t kGroups = 64u / G;                 // rows side by side in a wave
    constexpr uint32_t kRowsPerStep = rows_per_step(G, RU);
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (uint32_t)(G - 1), grp = lane / (uint32_t)G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kThreads) >> 6;
    const uint32_t R = a.record_size;
    const uint32_t n_passes = passes(R, G, U);   // over the most chunks a row can span

    for (uint64_t r0 = wave * kRowsPerStep; r0 < a.n_variants; r0 += n_waves * kRowsPerStep) {
        const uint8_t *base[RU];
        uint32_t d[RU], nch[RU];
        Acc acc[RU];
#pragma unroll
        for (int k = 0; k < RU; k++) {
            const uint64_t row = r0 + (uint64_t)k * kGroups + grp;   // groups of a wave on neighbouring rows
            const bool live = row < a.n_variants;
            const uint8_t *rec = !live ? a.records : row_record(a, row);
            const uint64_t p = (uint64_t)(uintptr_t)rec;
            d[k] = (uint32_t)p & 15u;
            base[k] = rec - d[k];   // (pointer arithmetic on the argument keeps the loads global, not flat)
            nch[k] = live && R ? (d[k] + R + 15u) >> 4 : 0u;   // aligned 16-byte chunks the row's bytes touch
        }
        for (uint32_t t = 0; t < n_passes; t++) {
            gt_v4u w[RU][U], m[RU][U];
#pragma unroll
            for (int k = 0; k < RU; k++)
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t c = (t * (uint32_t)U + (uint32_t)u) * (uint32_t)G + gl;
                    const bool on = c < nch[k];
                    w[k][u] = on ? load_nt16(base[k] + 16ull * c) : gt_v4u{0u, 0u, 0u, 0u};
                    if (MASK) m[k][u] = on ? *reinterpret_cast<const gt_v4u *>(a.kept_mask + 16ull * (c + 1u)) : gt_v4u{0u, 0u, 0u, 0u};
                }
#pragma unroll
            for (int k = 0; k < RU; k++)
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t c = (t * (uint32_t)U + (uint32_t)u) * (uint32_t)G + gl;
                    gt_v4u mm;
                    if (MASK) {
                        // buffer chunk c: the lane below holds it (same row, chunk c - 1); a group's first lane loads it
                        const bool first = gl == 0u && c < nch[k];
                        const gt_v4u own = first ? *reinterpret_cast<const gt_v4u *>(a.kept_mask + 16ull * c) : gt_v4u{0u, 0u, 0u, 0u};
                        const gt_v4u lower = dpp_from_lower_lane(m[k][u], own);
                        mm = funnel16(gl == 0u ? own : lower, m[k][u], 16u - d[k]);
                    } else {
                        const int64_t i0 = 16 * (int64_t)c - (int64_t)d[k];
                        if (c == 0u || c + 1u >= nch[k]) {   // the row's first / last chunk: neighbours' bytes and pad bits
                            mm = gt_v4u{row_mask(i0, 0, a.sample_count), row_mask(i0, 1, a.sample_count), row_mask(i0, 2, a.sample_count),
                                        row_mask(i0, 3, a.sample_count)};
                        } else {
                            mm = gt_v4u{0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u};
                        }
                    }
                    count16(acc[k], w[k][u], mm);
                }
        }
#pragma unroll
        for (int k = 0; k < RU; k++) {
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1) {
                acc[k].het += __shfl_xor(acc[k].het, off, G);
                acc[k].alt += __shfl_xor(acc[k].alt, off, G);
                acc[k].miss += __shfl_xor(acc[k].miss, off, G);
            }
            const uint64_t row = r0 + (uint64_t)k * kGroups + grp;
            if (gl == 0u && row < a.n_variants) {
                const uint32_t hom_ref = a.kept_count - acc[k].het - acc[k].alt - acc[k].miss;
                uint32_t *dst = a.counts + 4ull * row;
                if (((uintptr_t)a.counts & 15u) == 0u) {
                    *reinterpret_cast<gt_v4u *>(dst) = gt_v4u{hom_ref, acc[k].het, acc[k].alt, acc[k].miss};
                } else {
                    dst[0] = hom_ref;
                    dst[1] = acc[k].het;
                    dst[2] = acc[k].alt;
                    dst[3] = acc[k].miss;
                }
            }
        }
    }
}

template <int G, int RU, int U>
hipError_t launch_shape(const CountArgs &a, int num_cus, hipStream_t stream)
{
    static_assert(shape(0u, G == 64).RU == (uint32_t)RU && shape(0u, G == 64).U == (uint32_t)U, "an instantiation that plan::count::shape names");
    const uint32_t grid = plan::count::grid(a.n_variants, G, RU, num_cus);
    if (a.kept_mask != nullptr)
        hipLaunchKernelGGL((gt_count_kernel<G, RU, U, true>), dim3(grid), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((gt_count_kernel<G, RU, U, false>), dim3(grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gt_count(const CountArgs &a, bool wave_per_row, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0) return hipSuccess;
    switch (shape(a.record_size, wave_per_row).G) {   // (RU, U) as plan::count::shape says: 1, 4 at a wave per row, else 2, 1
        case 64u: return launch_shape<64, 1, 4>(a, num_cus, stream);
        case 4u: return launch_shape<4, 2, 1>(a, num_cus, stream);
        case 8u: return launch_shape<8, 2, 1>(a, num_cus, stream);
        case 16u: return launch_shape<16, 2, 1>(a, num_cus, stream);
        default: return launch_shape<32, 2, 1>(a, num_cus, stream);
    }
}

}  // namespace pgenhip
