// gt_pack.hip — packed K-sample records for gfx950 (MI355X): row j of the output is the mode-0x02 record of the ctx's K kept
// samples of selected row j (src/pfile.rs:172-175 read backwards: kept sample k in byte k/4, bits 2*(k%4), LSB first), each code
// sent through a four-entry 2-bit -> 2-bit map, the pad bits of the last byte zero.  Byte movers: nothing is computed but the map.
//
// The map works on bit planes.  With L = w & 0x55555555 and H = (w >> 1) & 0x55555555 the code of a sample is L + 2H at its even
// bit, and each output plane is a boolean function of (L, H) given by four masks t[c] (0x55555555 where the map's entry for code c
// has the plane's bit, else 0): two bit selects on L, one on H (v_bfi_b32), three per plane and nine instructions per 16 samples.
// The identity is instantiated separately and pays nothing.
//
// Three shapes:
//   GENERAL  one lane per output byte, four codes looked up through the kept list (or taken in place), any K, any layout.  The
//            correctness baseline.
//   DENSE    all samples kept: a record copy whose source and destination each have their own byte phase.  A lane owns one
//            16-byte-ALIGNED chunk of the destination row.  Source chunks are aligned non-temporal loads: a lane loads source chunk
//            c + 1, takes chunk c from the lane below (DPP wave_shr:1; the first lane of a row's group loads it itself) and
//            funnel-shifts the pair by the difference of the two phases.  Only source chunks that hold a byte of the record are
//            loaded.  Interior chunks are 16-byte non-temporal stores, the up to 15 bytes of a row's head and tail byte stores.
//            G = 4 .. 64 lanes per row by the row's length, 64 / G rows per wave, so 75-byte records do not cost a wave per row;
//            rows longer than one wave's four passes are cut into parts of 256 chunks (4 KiB) that separate waves take, so a call
//            with few rows of very long records still fills the chip.  Dense records into dense output with N a multiple of 4 (no
//            pad bits to clear) are one byte stream: the launcher hands runs of rows of about 64 KiB to the kernel as single rows.
//   GATHER   a kept subset, output-driven: a lane owns one output dword, the kept samples 16q .. 16q + 15 of row j.  Their indices
//            are four 16-byte loads of the kept list (64 B per lane, coalesced, the list shared by every row and resident in L2).
//            When the sixteen samples lie within 16 record bytes (dense keeps: half kept spans about eight) the lane reads them
//            with ONE 16-byte load and shifts the codes out of registers; else it reads one byte per sample (sparse keeps touch
//            only the sectors that hold a kept sample; nothing is staged, so a row's length does not matter).  Lanes are numbered
//            over the whole launch (row = lane index / dwords per row), so a row's dwords spread over as many blocks as they
//            fill and short lists do not leave lanes idle.
// Every output byte has one owner: no atomics, no scratch, no work counters.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::pack;   // kThreads, kBlocksPerCu, kPartChunks, kStreamRunBytes and the launch plans
constexpr uint32_t kEven = 0x55555555u;

// the map as plane masks: lo[c] / hi[c] = 0x55555555 where map[c] has bit 0 / bit 1
struct PlaneMap {
    uint32_t lo[4], hi[4];
    __device__ __forceinline__ explicit PlaneMap(uint32_t map8)
    {
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++) {
            lo[c] = (map8 >> (2u * c)) & 1u ? kEven : 0u;
            hi[c] = (map8 >> (2u * c + 1u)) & 1u ? kEven : 0u;
        }
    }
    // sixteen codes at once
    __device__ __forceinline__ uint32_t apply(uint32_t w) const
    {
        const uint32_t L = w & kEven, H = (w >> 1) & kEven;
        const uint32_t l0 = (lo[1] & L) | (lo[0] & ~L), l1 = (lo[3] & L) | (lo[2] & ~L);
        const uint32_t h0 = (hi[1] & L) | (hi[0] & ~L), h1 = (hi[3] & L) | (hi[2] & ~L);
        const uint32_t nl = (l1 & H) | (l0 & ~H), nh = (h1 & H) | (h0 & ~H);
        return nl | (nh << 1);
    }
};

// ---- GENERAL -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gt_pack_general_kernel(PackArgs a, uint64_t total)
{
    const uint32_t K = a.kept_count, RK = (K + 3u) >> 2;
    const bool small = total <= 0xFFFFFFFFull;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kThreads) {
        uint64_t j;
        uint32_t b;
        if (small) {
            j = (uint32_t)idx / RK;
            b = (uint32_t)idx % RK;
        } else {
            j = idx / RK;
            b = (uint32_t)(idx - j * RK);
        }
        const uint8_t *rec = row_record(a, j);
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t k = 4u * b + i;
            if (k >= K) break;
            const uint32_t s = a.kept_idx != nullptr ? a.kept_idx[k] : k;
            const uint32_t c = ((uint32_t)rec[s >> 2] >> (2u * (s & 3u))) & 3u;
            v |= ((a.map8 >> (2u * c)) & 3u) << (2u * i);
        }
        a.out[j * a.out_stride + b] = (uint8_t)v;
    }
}

// ---- DENSE ---------------------------------------------------------------------------------------------------------------------
// G lanes per row, P passes per work item; MAP: a map other than the identity
template <int G, int P, bool MAP>
__global__ __launch_bounds__(kThreads) void gt_pack_dense_kernel(PackArgs a, uint32_t parts, uint64_t items)
{
    constexpr uint32_t kGroups = 64u / G;   // rows side by side in a wave
    const PlaneMap pm(a.map8);
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (uint32_t)(G - 1), grp = lane / (uint32_t)G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kThreads) >> 6;
    const uint32_t R = a.record_size;
    const uint32_t pad_keep = a.sample_count & 3u ? (1u << (2u * (a.sample_count & 3u))) - 1u : 0xFFu;   // sample bits of the last byte

    for (uint64_t item = wave; item < items; item += n_waves) {   // wave-uniform: every lane runs every DPP below
        const uint64_t rg = parts == 1u ? item : item / parts;   // (short rows are one part: no division)
        const uint32_t part = (uint32_t)(item - rg * parts);
        const uint64_t row = rg * kGroups + grp;
        const bool live = row < a.n_variants;
        const uint8_t *rec = live ? row_record(a, row) : a.records;
        uint8_t *dst = a.out + (live ? row : 0ull) * a.out_stride;
        const int32_t Rl = live ? (int32_t)R : 0;   // a group without a row loads and stores nothing
        const uint32_t smis = (uint32_t)(uintptr_t)rec & 15u, dmis = (uint32_t)(uintptr_t)dst & 15u;
        const int32_t delta = (int32_t)smis - (int32_t)dmis;
        const uint32_t o = (uint32_t)delta & 15u;
        // source chunk i = the 16 bytes from row byte s0 + 16 i; destination chunk c = source bytes [16 c + o, 16 c + o + 16)
        const int32_t s0 = -(int32_t)smis - (delta < 0 ? 16 : 0);
        const uint8_t *sbase = rec + s0;   // (pointer arithmetic on the argument keeps the loads global, not flat)
        uint8_t *dbase = dst - dmis;
#pragma unroll
        for (int t = 0; t < P; t++) {
            const uint32_t c = (part * (uint32_t)P + (uint32_t)t) * (uint32_t)G + gl;
            const int32_t b0 = 16 * (int32_t)c - (int32_t)dmis;   // row byte under the destination chunk's first byte
            const int32_t hi_off = s0 + 16 * ((int32_t)c + 1), lo_off = hi_off - 16;
            // a source chunk is loaded only if it holds a byte of the record
            const gt_v4u hi = hi_off < Rl && hi_off + 16 > 0 ? load_nt16(sbase + 16ull * (c + 1u)) : gt_v4u{0u, 0u, 0u, 0u};
            const gt_v4u own = gl == 0u && lo_off < Rl && lo_off + 16 > 0 ? load_nt16(sbase + 16ull * c) : gt_v4u{0u, 0u, 0u, 0u};
            const gt_v4u lower = dpp_from_lower_lane(hi, own);
            gt_v4u v = funnel16(gl == 0u ? own : lower, hi, o);
            if (b0 >= Rl || b0 + 16 <= 0) continue;   // no byte of the row in this chunk (Rl = 0: no row)
            if (MAP) {
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = pm.apply(v[q]);
            }
            const int32_t last = Rl - 1 - b0;   // the row's last byte, relative to the chunk
            if (last < 16) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if ((last >> 2) == q) v[q] &= ~((~pad_keep & 0xFFu) << (8u * ((uint32_t)last & 3u)));
            }
            if (b0 >= 0 && last >= 15) {
                __builtin_nontemporal_store(v, reinterpret_cast<gt_v4u *>(dbase + 16ull * c));
            } else {   // the row's head or tail (both, on a row shorter than a chunk)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (b0 + i >= 0 && i <= last) dst[b0 + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

// ---- GATHER --------------------------------------------------------------------------------------------------------------------
template <bool MAP>
__global__ __launch_bounds__(kThreads) void gt_pack_gather_kernel(PackArgs a, uint32_t Q, uint64_t total)
{
    const PlaneMap pm(a.map8);
    const uint32_t K = a.kept_count, R = a.record_size, RK = (K + 3u) >> 2;
    const bool small = total <= 0xFFFFFFFFull;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kThreads) {
        uint64_t j;
        uint32_t q;
        if (small) {
            j = (uint32_t)idx / Q;
            q = (uint32_t)idx % Q;
        } else {
            j = idx / Q;
            q = (uint32_t)(idx - j * Q);
        }
        const uint32_t k0 = 16u * q, n = min(16u, K - k0);   // n >= 1
        uint32_t s[16];
        if (n == 16u) {
#pragma unroll
            for (int g = 0; g < 4; g++) {   // hipMalloc'ed list: 16-byte aligned at a multiple of 16 entries
                const gt_v4u x = *reinterpret_cast<const gt_v4u *>(a.kept_idx + k0 + 4 * g);
                s[4 * g] = x[0], s[4 * g + 1] = x[1], s[4 * g + 2] = x[2], s[4 * g + 3] = x[3];
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) s[i] = a.kept_idx[k0 + min(i, n - 1u)];
        }
        const uint8_t *rec = row_record(a, j);
        const uint32_t byte0 = s[0] >> 2;
        uint32_t w = 0u;
        if ((s[15] >> 2) - byte0 < 16u && byte0 + 16u <= R) {
            // the sixteen samples within 16 record bytes that lie inside the record: one load, codes shifted out of registers
            gt_v4u x;
            __builtin_memcpy(&x, rec + byte0, 16);
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) {
                const uint32_t rel = s[i] - 4u * byte0;   // 0 .. 63
                const uint32_t d = rel >> 4;
                const uint32_t xw = d == 0u ? x[0] : d == 1u ? x[1] : d == 2u ? x[2] : x[3];
                w |= ((xw >> (2u * (rel & 15u))) & 3u) << (2u * i);
            }
        } else {
            uint32_t b[16];
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) b[i] = rec[s[i] >> 2];   // all sixteen loads in flight
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) w |= ((b[i] >> (2u * (s[i] & 3u))) & 3u) << (2u * i);
        }
        if (MAP) w = pm.apply(w);
        if (n < 16u) w &= (1u << (2u * n)) - 1u;   // ranks past K: pad bits, zero whatever the map
        uint8_t *p = a.out + j * a.out_stride + 4ull * q;
        const uint32_t nb = min(4u, RK - 4u * q);
        if (nb == 4u && ((uintptr_t)p & 3u) == 0u) {
            *reinterpret_cast<uint32_t *>(p) = w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
                if (i < nb) p[i] = (uint8_t)(w >> (8u * i));
        }
    }
}

template <int G, int P>
hipError_t launch_dense(const PackArgs &a, const DensePlan &p, hipStream_t stream)
{
    const dim3 grid(p.grid), block(kThreads);
    if (a.map8 != kPackIdentityMap)
        hipLaunchKernelGGL((gt_pack_dense_kernel<G, P, true>), grid, block, 0, stream, a, p.parts, p.items);
    else
        hipLaunchKernelGGL((gt_pack_dense_kernel<G, P, false>), grid, block, 0, stream, a, p.parts, p.items);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gt_pack_general(const PackArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    const uint64_t total = (uint64_t)a.n_variants * ((a.kept_count + 3u) >> 2);
    const dim3 grid(general_grid(a.n_variants, a.kept_count, num_cus, blocks)), block(kThreads);
    hipLaunchKernelGGL(gt_pack_general_kernel, grid, block, 0, stream, a, total);
    return hipGetLastError();
}

// (G, P) as plan::pack::dense_plan says: three passes of 4 .. 32 lanes per row, from 97 chunks a wave per row, cut into parts
static hipError_t launch_dense_rows(const PackArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    const DensePlan p = dense_plan(a.record_size, a.n_variants, num_cus, blocks);
    switch (p.G) {
        case 4u: return launch_dense<4, 3>(a, p, stream);
        case 8u: return launch_dense<8, 3>(a, p, stream);
        case 16u: return launch_dense<16, 3>(a, p, stream);
        case 32u: return launch_dense<32, 3>(a, p, stream);
        default: return launch_dense<64, (int)(kPartChunks / 64u)>(a, p, stream);
    }
}

hipError_t launch_gt_pack_dense(const PackArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    // Dense records into dense output with no pad bits (N a multiple of 4) are one byte stream: runs of m rows go as ONE row of
    // m * R bytes (no heads and tails at every record, no idle lanes on 75-byte rows), the rows behind the last whole run row by row
    const uint32_t R = a.record_size;
    if (merge_runs(gathered(a), a.sample_count, R, a.record_stride, a.out_stride, a.n_variants)) {
        const uint64_t m = run_rows(R);
        PackArgs run = a, rest = a;
        run.n_variants = (uint32_t)(a.n_variants / m);
        run.record_size = (uint32_t)(m * R);
        run.sample_count = 4u * run.record_size;
        run.record_stride = run.out_stride = m * R;
        const hipError_t e = launch_dense_rows(run, blocks, num_cus, stream);
        if (e != hipSuccess) return e;
        const uint64_t done = (uint64_t)run.n_variants * m;
        rest.n_variants = (uint32_t)(a.n_variants - done);
        if (rest.n_variants == 0u) return hipSuccess;
        rest.records = a.records + done * R;
        rest.out = a.out + done * R;
        return launch_dense_rows(rest, blocks, num_cus, stream);
    }
    return launch_dense_rows(a, blocks, num_cus, stream);
}

hipError_t launch_gt_pack_gather(const PackArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    const GatherPlan p = gather_plan(a.n_variants, a.kept_count, num_cus, blocks);
    const dim3 grid(p.grid), block(kThreads);
    if (a.map8 != kPackIdentityMap)
        hipLaunchKernelGGL(gt_pack_gather_kernel<true>, grid, block, 0, stream, a, p.Q, p.total);
    else
        hipLaunchKernelGGL(gt_pack_gather_kernel<false>, grid, block, 0, stream, a, p.Q, p.total);
    return hipGetLastError();
}

}  // namespace pgenhip
