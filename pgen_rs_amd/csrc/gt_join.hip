// gt_join.hip — sample-wise join of records for gfx950 (MI355X): row j of the output is the mode-0x02 record of N_out = sum n_p
// samples, the samples of part 0 first, then part 1, ...: output sample start_p + s is sample s of part p's record for row j (code
// in byte s/4, bits 2*(s%4), LSB first, src/pfile.rs:172-175).  A part that has no record for the row (offset JOIN_ABSENT) gives code
// 3 for its n_p samples and is not read; a part whose flip byte for the row is set has codes 0 and 2 exchanged (REF and ALT the other
// way round), on bit planes w ^= (~w & 0x55555555) << 1.  The pad bits of the output's last byte are zero; the pad bits of a source
// record's last byte are never taken as samples.  The inverse of pack_records' sample selection: byte movers, nothing is computed.
//
// The part table (up to 8 entries) travels as kernel arguments.  A lane's part is divergent, and a by-value array indexed at run
// time goes to scratch; both kernels walk the table with an UNROLLED loop instead, so that every entry is read with scalar loads and
// a lane only executes the bodies of the parts its samples lie in (usually one: whole waves skip the others).
//
// Two shapes:
//   GENERAL  one lane per output byte, four codes, each looked up in its part.  Any part sizes, any alignment.  The correctness
//            baseline.
//   STREAM   output-driven.  A lane owns one 16-byte-ALIGNED chunk of an output row (64 samples; a row's first and last chunk are
//            partial).  A chunk that lies inside one part and whose source bytes lie 20 bytes deep inside that part's record takes
//            them with one 16-byte and one 4-byte load at the part's own byte offset and funnel-shifts the five dwords by the part's
//            bit phase (0 / 2 / 4 / 6 bits): one 16-byte store.  Every other chunk (seams, a record's end, the row's head and tail)
//            is built dword by dword: per part that has samples in the dword, up to 8 record bytes (one load where the record holds
//            them, else byte loads that stop at the record's last byte), shifted, masked to the part's samples and ORed in.  Chunks
//            are numbered over the whole launch (row = index / chunks per row), so short rows share a block and a long row spreads
//            over many.
// Every output byte has one owner: no atomics, no scratch, no work counters.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::join;   // kThreads, kBlocksPerCu, kChunkBytes and the launch plans
constexpr uint32_t kEven = 0x55555555u;
constexpr uint64_t kAbsent = PGENHIP_JOIN_ABSENT;

__device__ __forceinline__ uint32_t flip02(uint32_t w) { return w ^ ((~w & kEven) << 1); }

// ---- GENERAL -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gt_join_general_kernel(JoinArgs a, uint64_t total)
{
    const uint32_t N = a.sample_count, R = a.record_size;
    const bool small = total <= 0xFFFFFFFFull;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kThreads) {
        uint64_t j;
        uint32_t b;
        if (small) {
            j = (uint32_t)idx / R;
            b = (uint32_t)idx % R;
        } else {
            j = idx / R;
            b = (uint32_t)(idx - j * R);
        }
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t s = 4u * b + i;
            if (s >= N) break;
#pragma unroll
            for (uint32_t p = 0; p < PGENHIP_JOIN_MAX_PARTS; p++) {
                if (p >= a.n_parts) break;
                const JoinPart &pt = a.part[p];
                if (s - pt.start < pt.count) {   // (unsigned: start <= s < start + count)
                    const uint32_t ls = s - pt.start;
                    const uint64_t off = pt.record_off[j];
                    uint32_t c = 3u;
                    if (off != kAbsent) {
                        c = ((uint32_t)pt.base[off + (ls >> 2)] >> (2u * (ls & 3u))) & 3u;
                        if (pt.flip != nullptr && pt.flip[j] != 0u) c = flip02(c) & 3u;
                    }
                    v |= c << (2u * i);
                }
            }
        }
        a.out[j * a.out_stride + b] = (uint8_t)v;
    }
}

// ---- STREAM --------------------------------------------------------------------------------------------------------------------
// the 16 output samples s0 .. s0 + 15 of row j as a dword (s0 a multiple of 4; samples from N on are zero)
__device__ __forceinline__ uint32_t join_dword(const JoinArgs &a, uint64_t j, uint32_t s0)
{
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t p = 0; p < PGENHIP_JOIN_MAX_PARTS; p++) {
        if (p >= a.n_parts) break;
        const JoinPart &pt = a.part[p];
        const uint32_t lo = max(s0, pt.start), hi = min(s0 + 16u, pt.start + pt.count);   // (start + count <= N < 2^32)
        if (lo < hi) {
            const uint32_t ls = lo - pt.start, cnt = hi - lo;   // the part's samples ls .. ls + cnt - 1
            const uint64_t off = pt.record_off[j];
            uint32_t bits = 0xFFFFFFFFu;
            if (off != kAbsent) {
                const uint8_t *rec = pt.base + off;
                const uint32_t b0 = ls >> 2, b1 = (ls + cnt - 1u) >> 2, rp = (pt.count + 3u) >> 2;   // first and last byte needed
                uint64_t x = 0u;
                if (b0 + 8u <= rp) {
                    __builtin_memcpy(&x, rec + b0, 8);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 5u; i++)   // 16 samples at a phase of up to 6 bits: five bytes
                        if (b0 + i <= b1) x |= (uint64_t)rec[b0 + i] << (8u * i);
                }
                bits = (uint32_t)(x >> (2u * (ls & 3u)));
                if (pt.flip != nullptr && pt.flip[j] != 0u) bits = flip02(bits);
            }
            if (cnt < 16u) bits &= (1u << (2u * cnt)) - 1u;   // (drops the record's pad bits and whatever lies behind the samples)
            w |= bits << (2u * (lo - s0));
        }
    }
    return w;
}

__global__ __launch_bounds__(kThreads) void gt_join_stream_kernel(JoinArgs a, uint32_t chunks, uint64_t total)
{
    const uint32_t R = a.record_size;
    const bool small = total <= 0xFFFFFFFFull;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kThreads) {
        uint64_t j;
        uint32_t c;
        if (small) {
            j = (uint32_t)idx / chunks;
            c = (uint32_t)idx % chunks;
        } else {
            j = idx / chunks;
            c = (uint32_t)(idx - j * chunks);
        }
        uint8_t *dst = a.out + j * a.out_stride;
        const uint32_t dmis = (uint32_t)(uintptr_t)dst & 15u;
        const int32_t b0 = (int32_t)(kChunkBytes * c) - (int32_t)dmis;   // row byte under the chunk's first byte
        if (b0 >= (int32_t)R || b0 + (int32_t)kChunkBytes <= 0) continue;   // no byte of the row in this chunk
        const int32_t last = (int32_t)R - 1 - b0;                         // the row's last byte, relative to the chunk
        gt_v4u v = {0u, 0u, 0u, 0u};
        if (b0 >= 0 && last >= 15) {
            // a whole chunk: 64 samples from s0 on
            const uint32_t s0 = 4u * (uint32_t)b0;
            bool done = false;
#pragma unroll
            for (uint32_t p = 0; p < PGENHIP_JOIN_MAX_PARTS; p++) {
                if (p >= a.n_parts) break;
                const JoinPart &pt = a.part[p];
                if (s0 >= pt.start && s0 - pt.start + 64u <= pt.count) {   // all 64 in this part
                    const uint32_t ls = s0 - pt.start, sb = ls >> 2, rp = (pt.count + 3u) >> 2;
                    const uint64_t off = pt.record_off[j];
                    if (off == kAbsent) {
                        v = gt_v4u{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                        done = true;
                    } else if (sb + 20u <= rp) {
                        const uint8_t *src = pt.base + off + sb;
                        gt_v4u x;
                        uint32_t y;
                        __builtin_memcpy(&x, src, 16);
                        __builtin_memcpy(&y, src + 16, 4);
                        const uint32_t ph = 2u * (ls & 3u);   // 0, 2, 4 or 6 bits
                        v[0] = __builtin_amdgcn_alignbit(x[1], x[0], ph);
                        v[1] = __builtin_amdgcn_alignbit(x[2], x[1], ph);
                        v[2] = __builtin_amdgcn_alignbit(x[3], x[2], ph);
                        v[3] = __builtin_amdgcn_alignbit(y, x[3], ph);
                        if (pt.flip != nullptr && pt.flip[j] != 0u) {
#pragma unroll
                            for (int q = 0; q < 4; q++) v[q] = flip02(v[q]);
                        }
                        done = true;
                    }
                }
            }
            if (!done) {
#pragma unroll 1
                for (uint32_t q = 0; q < 4u; q++) {
                    const uint32_t w = join_dword(a, j, s0 + 16u * q);
                    v[0] = q == 0u ? w : v[0], v[1] = q == 1u ? w : v[1], v[2] = q == 2u ? w : v[2], v[3] = q == 3u ? w : v[3];
                }
            }
            __builtin_nontemporal_store(v, reinterpret_cast<gt_v4u *>(dst + b0));
        } else {
            // the row's head or tail (both, on a row shorter than a chunk): row bytes [first, first + n)
            const uint32_t first = (uint32_t)max(b0, 0), n = (uint32_t)min(last, 15) + 1u - (first - (uint32_t)b0);
#pragma unroll 1
            for (uint32_t q = 0; q < 4u; q++) {
                if (4u * q >= n) break;
                const uint32_t w = join_dword(a, j, 4u * first + 16u * q);
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++)
                    if (4u * q + i < n) dst[first + 4u * q + i] = (uint8_t)(w >> (8u * i));
            }
        }
    }
}

}  // namespace

hipError_t launch_gt_join_general(const JoinArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    const uint64_t total = (uint64_t)a.n_variants * a.record_size;
    const dim3 grid(general_grid(a.n_variants, a.record_size, num_cus, blocks)), block(kThreads);
    hipLaunchKernelGGL(gt_join_general_kernel, grid, block, 0, stream, a, total);
    return hipGetLastError();
}

hipError_t launch_gt_join_stream(const JoinArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.sample_count == 0) return hipSuccess;
    const StreamPlan p = stream_plan(a.record_size, a.n_variants, num_cus, blocks);
    const dim3 grid(p.grid), block(kThreads);
    hipLaunchKernelGGL(gt_join_stream_kernel, grid, block, 0, stream, a, p.chunks, p.total);
    return hipGetLastError();
}

}  // namespace pgenhip
