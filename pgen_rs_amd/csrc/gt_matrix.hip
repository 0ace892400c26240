// gt_matrix.hip — numeric genotype matrix for gfx950 (MI355X): element (j, k) = values[code of kept sample k in selected row j]
// (src/pfile.rs:172-175: sample s in byte s/4, bits 2*(s%4)), written as elements of 1, 2 or 4 bytes either variant-major
// (row j at out + j*out_stride) or sample-major (row k at out + k*out_stride).  The library does not interpret the elements:
// a dtype is a size and four bit patterns, so one kernel per element size serves int8, uint8, fp16, bf16, fp32 and int32.
//
// Table lookup.  Four 2-bit codes spread to the four bytes of a dword (v_bfe, two v_lshl_or, v_and) are a v_perm_b32 selector:
//   1-byte elements: the four patterns in one register, one v_perm_b32 per four samples;
//   2-byte elements: low and high byte planes in two registers, selector (c0, c0+4, c1, c1+4): per two samples one v_perm_b32 to
//                    duplicate the codes, one add, one v_perm_b32 over the two planes;
//   4-byte elements: the two code bits sign-extended to masks (v_bfe_i32) select among the patterns with and / xor on
//                    r0, r0^r1, r0^r2 and r0^r1^r2^r3 (v_bitop3_b32); the per-plane perm needs a 4 x 4 byte transpose behind it and
//                    came out longer, and a ternary chain is turned into a per-thread LDS table by the compiler.
//
// Three shapes:
//   GENERAL  one lane per output element, any K (kept list or all), any strides, both orientations.  The correctness baseline.
//   STREAM   variant-major, all samples kept.  A lane owns one ALIGNED 16-byte chunk of the output (16 / 8 / 4 elements), a wave 1 KiB
//            of whole 128-byte lines per store instruction.  A dense matrix (out_stride == K * elem_bytes) is one byte stream: a chunk
//            may hold the tail of row j and the head of row j + 1 (row = element index times a reciprocal, corrected), so rows of
//            2 504 or 300 bytes cost no partial stores; with a padded pitch every row is a span of its own with an element-wise head
//            and tail.  Rows of 4 KiB of output and more take a second kernel in which blockIdx.y strides over rows and blockIdx.x over
//            a row's chunks, so that no lane divides.  Records are read where they lie (unaligned 1-5 byte windows; any byte
//            phase, gathers, byte offsets).
//   TILE     sample-major, all samples kept, 16-byte-aligned rows: the 2-bit transpose.  A block stages kTileVariants rows x
//            kTileSamples samples (128 bytes of each record, one whole line) in LDS with 16-byte loads; a wave owns 128 variants x 128
//            samples; lane (g = lane % 8, q = lane / 8) reads the dword of samples 16q .. 16q+15 from rows 16g .. 16g+15, transposes
//            16 x 16 codes in registers (four butterfly stages of shift / xor / and) and writes, per sample, one 16-byte chunk of 16
//            consecutive variants: the eight lanes of one q cover 128 contiguous bytes of that sample's row, a whole line.  With 2- and
//            4-byte elements a chunk is 8 / 4 variants, so a lane's 16 rows are 2 / 4 runs of 8 / 4 rows, run h at tile row
//            128h/E + (16/E)g: every store instruction still covers whole lines (a first version wrote 32 / 64 contiguous bytes per
//            lane, half and quarter lines per instruction: 0.13 of 8 TB/s at f32 where the chunked form reaches what int8 does).
//            LDS rows are rotated by 16 bytes per run, so both halves of a ds_read_b32 hit 32 distinct banks.
//            Tiles are walked variant-tile first inside a band of kTileSamples samples, so a launch writes on as many fronts as a
//            band has rows, not on all K rows at once.  Ragged edges (V, N not multiples of the tile) write element by element.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::matrix;   // kThreads, kLongRowBytes, kTileVariants, kWaveSamples, kTileSamples, ... and the launch plans

// the four patterns as the lookup registers of one element size
template <int E>
struct Table {
    uint32_t r0, r1, r2, r3;
    __device__ __forceinline__ explicit Table(const MatrixArgs &a)
    {
        if (E == 1) {
            r0 = (a.tab[0] & 0xFFu) | (a.tab[1] & 0xFFu) << 8 | (a.tab[2] & 0xFFu) << 16 | (a.tab[3] & 0xFFu) << 24;
            r1 = r2 = r3 = 0u;
        } else if (E == 2) {
            r0 = (a.tab[0] & 0xFFu) | (a.tab[1] & 0xFFu) << 8 | (a.tab[2] & 0xFFu) << 16 | (a.tab[3] & 0xFFu) << 24;                   // low bytes
            r1 = ((a.tab[0] >> 8) & 0xFFu) | ((a.tab[1] >> 8) & 0xFFu) << 8 | ((a.tab[2] >> 8) & 0xFFu) << 16 | ((a.tab[3] >> 8) & 0xFFu) << 24;   // high bytes
            r2 = r3 = 0u;
        } else {   // pattern of code c = r0 ^ (bit 0 ? r1) ^ (bit 1 ? r2) ^ (both ? r3)
            r0 = a.tab[0], r1 = a.tab[0] ^ a.tab[1], r2 = a.tab[0] ^ a.tab[2], r3 = a.tab[0] ^ a.tab[1] ^ a.tab[2] ^ a.tab[3];
        }
    }
    // 4-byte pattern of the code at bits 2i, 2i + 1 of b
    __device__ __forceinline__ uint32_t pick4(uint32_t b, uint32_t i) const
    {
        const uint32_t m0 = (uint32_t)((int32_t)(b << (31u - 2u * i)) >> 31), m1 = (uint32_t)((int32_t)(b << (30u - 2u * i)) >> 31);
        return r0 ^ (m0 & r1) ^ (m1 & (r2 ^ (m0 & r3)));
    }
    // one element, zero-extended (edge paths)
    __device__ __forceinline__ uint32_t value(uint32_t c) const
    {
        if (E == 1) return (r0 >> (8u * c)) & 0xFFu;
        if (E == 2) return ((r0 >> (8u * c)) & 0xFFu) | ((r1 >> (8u * c)) & 0xFFu) << 8;
        return pick4(c, 0u);
    }
    // the four codes in the low byte of b -> 4 * E bytes in d[0 .. E)
    __device__ __forceinline__ void expand4(uint32_t b, uint32_t *d) const
    {
        if (E == 4) {
#pragma unroll
            for (int i = 0; i < 4; i++) d[i] = pick4(b, (uint32_t)i);
            return;
        }
        uint32_t s = (b & 0xFFu) | (b & 0xFFu) << 6;
        s = (s | s << 12) & 0x03030303u;   // code i in byte i
        if (E == 1) {
            d[0] = __builtin_amdgcn_perm(0u, r0, s);
        } else {
            d[0] = __builtin_amdgcn_perm(r1, r0, __builtin_amdgcn_perm(0u, s, 0x01010000u) + 0x04000400u);
            d[1] = __builtin_amdgcn_perm(r1, r0, __builtin_amdgcn_perm(0u, s, 0x03030202u) + 0x04000400u);
        }
    }
    // the 16 / E codes of one 16-byte chunk (code i at bits 2i) -> d[0 .. 4)
    __device__ __forceinline__ void expand_chunk(uint32_t codes, uint32_t *d) const
    {
#pragma unroll
        for (int q = 0; q < 4 / E; q++) expand4(codes >> (8 * q), d + q * E);
    }
};

template <int E>
__device__ __forceinline__ void store_elem(uint8_t *p, uint32_t v)
{
    if (E == 1) *p = (uint8_t)v;
    else if (E == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    else *reinterpret_cast<uint32_t *>(p) = v;
}

__device__ __forceinline__ void store16(uint8_t *p, const uint32_t *d)
{
    const gt_v4u v = {d[0], d[1], d[2], d[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<gt_v4u *>(p));
}

// floor(x / d) for x < 2^52, d >= 1, inv = 1.0 / d: the double product is within one of the quotient
__device__ __forceinline__ uint64_t div_recip(uint64_t x, uint32_t d, double inv, uint32_t &rem)
{
    uint64_t q = (uint64_t)((double)x * inv);
    int64_t r = (int64_t)(x - q * d);
    if (r < 0) { q--; r += d; }
    if (r >= (int64_t)d) { q++; r -= d; }
    rem = (uint32_t)r;
    return q;
}

// ---- GENERAL -------------------------------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(kThreads) void gt_matrix_general_kernel(MatrixArgs a, uint64_t total)
{
    const Table<E> tab(a);
    const uint32_t K = a.kept_count, V = a.n_variants;
    const uint32_t inner = a.sample_major ? V : K;   // elements of one output row
    const bool small = total <= 0xFFFFFFFFull;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kThreads) {
        uint64_t o;
        uint32_t i;
        if (small) {
            o = (uint32_t)idx / inner;
            i = (uint32_t)idx % inner;
        } else {
            o = idx / inner;
            i = (uint32_t)(idx - o * inner);
        }
        const uint64_t j = a.sample_major ? i : o;
        const uint32_t k = a.sample_major ? (uint32_t)o : i;
        const uint32_t s = a.kept_idx != nullptr ? a.kept_idx[k] : k;
        const uint8_t *rec = row_record(a, j);
        const uint32_t c = ((uint32_t)rec[s >> 2] >> (2u * (s & 3u))) & 3u;
        store_elem<E>(a.out + o * a.out_stride + (uint64_t)i * E, tab.value(c));
    }
}

// ---- STREAM --------------------------------------------------------------------------------------------------------------------
// n = 16 / E samples from sample k0 of a record: bytes k0/4 .. (k0 + n - 1)/4, all inside the record when k0 + n <= N
template <int E>
__device__ __forceinline__ uint32_t load_codes(const uint8_t *rec, uint32_t k0)
{
    const uint8_t *p = rec + (k0 >> 2);
    const uint32_t sh = 2u * (k0 & 3u);
    uint64_t bits;
    if (E == 1) {
        uint32_t w;
        __builtin_memcpy(&w, p, 4);
        bits = w;
        if (sh) bits |= (uint64_t)p[4] << 32;
    } else if (E == 2) {
        uint16_t h;
        __builtin_memcpy(&h, p, 2);
        bits = h;
        if (sh) bits |= (uint64_t)p[2] << 16;
    } else {
        bits = p[0];
        if (sh) bits |= (uint64_t)p[1] << 8;
    }
    return (uint32_t)(bits >> sh);
}

// One aligned 16-byte chunk at ptr whose first element is sample k0 of row j (k0 < 0: the chunk starts in front of the span).
// dense: elements at or past K belong to the following rows; else they lie outside the row's span and are not written.
template <int E>
__device__ __forceinline__ void stream_chunk(const MatrixArgs &a, const Table<E> &tab, bool dense, uint64_t j, int64_t k0, uint8_t *ptr)
{
    constexpr uint32_t n = 16u / E;
    const uint32_t K = a.kept_count;
    const uint64_t V = a.n_variants;
    uint32_t d[4];
    if (k0 >= 0 && k0 + n <= K) {
        tab.expand_chunk(load_codes<E>(row_record(a, j), (uint32_t)k0), d);
        store16(ptr, d);
        return;
    }
    // edge chunk: the span's head or tail, or (dense) a chunk that crosses rows
    uint32_t codes = 0u, valid = 0u;
    uint64_t jj = j;
    int64_t kk = k0;
#pragma unroll 1
    for (uint32_t i = 0; i < n; i++, kk++) {
        if (dense && kk >= (int64_t)K) {
            kk = 0;
            jj++;
        }
        if (kk < 0 || kk >= (int64_t)K || jj >= V) continue;
        const uint8_t *rec = row_record(a, jj);
        codes |= (((uint32_t)rec[kk >> 2] >> (2u * ((uint32_t)kk & 3u))) & 3u) << (2u * i);
        valid |= 1u << i;
    }
    if (valid == (1u << n) - 1u) {
        tab.expand_chunk(codes, d);
        store16(ptr, d);
    } else {
#pragma unroll 1
        for (uint32_t i = 0; i < n; i++)
            if ((valid >> i) & 1u) store_elem<E>(ptr + i * E, tab.value((codes >> (2u * i)) & 3u));
    }
}

// Short rows.  dense: the whole matrix is one span of V * K elements; else every row is a span of K elements and `per_row` chunk slots
template <int E>
__global__ __launch_bounds__(kThreads) void gt_matrix_stream_kernel(MatrixArgs a, bool dense, uint64_t per_row, uint64_t total, double inv)
{
    constexpr uint32_t kLog = E == 1 ? 0u : E == 2 ? 1u : 2u;
    const Table<E> tab(a);
    const uint32_t K = a.kept_count;
    const uint32_t mis0 = (uint32_t)(uintptr_t)a.out & 15u;
    for (uint64_t w = (uint64_t)blockIdx.x * kThreads + threadIdx.x; w < total; w += (uint64_t)gridDim.x * kThreads) {
        uint64_t j;
        int64_t k0;
        uint8_t *ptr;
        if (dense) {
            const int64_t e0 = ((int64_t)(w << 4) - (int64_t)mis0) >> kLog;
            ptr = a.out - mis0 + (w << 4);
            if (e0 < 0) {
                j = 0;
                k0 = e0;
            } else {
                uint32_t rem;
                j = div_recip((uint64_t)e0, K, inv, rem);
                k0 = rem;
            }
        } else {
            uint32_t c;
            j = div_recip(w, (uint32_t)per_row, inv, c);
            uint8_t *row = a.out + j * a.out_stride;
            const uint32_t mis = (uint32_t)(uintptr_t)row & 15u;
            k0 = ((int64_t)((uint64_t)c << 4) - (int64_t)mis) >> kLog;
            ptr = row - mis + ((uint64_t)c << 4);
            if (k0 >= (int64_t)K) continue;
        }
        stream_chunk<E>(a, tab, dense, j, k0, ptr);
    }
}

// Long rows (kLongRowBytes of output and more): blockIdx.y strides over the rows, blockIdx.x over a row's chunk slots, so no lane
// divides; a row's head and tail are element-wise whatever the pitch (two chunks of several hundred)
template <int E>
__global__ __launch_bounds__(kThreads) void gt_matrix_stream_rows_kernel(MatrixArgs a, uint32_t per_row)
{
    constexpr uint32_t kLog = E == 1 ? 0u : E == 2 ? 1u : 2u;
    const Table<E> tab(a);
    for (uint64_t j = blockIdx.y; j < a.n_variants; j += gridDim.y) {
        uint8_t *row = a.out + j * a.out_stride;
        const uint32_t mis = (uint32_t)(uintptr_t)row & 15u;
        for (uint32_t c = blockIdx.x * kThreads + threadIdx.x; c < per_row; c += gridDim.x * kThreads) {
            const int64_t k0 = ((int64_t)((uint64_t)c << 4) - (int64_t)mis) >> kLog;
            if (k0 >= (int64_t)a.kept_count) continue;
            stream_chunk<E>(a, tab, false, j, k0, row - mis + ((uint64_t)c << 4));
        }
    }
}

// ---- TILE ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ gt_v4u load16_unaligned(const uint8_t *p)
{
    gt_v4u v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

template <int E>
__global__ __launch_bounds__(kThreads) void gt_matrix_tile_kernel(MatrixArgs a, uint64_t v_tiles, uint64_t total)
{
    // A lane's 16 variants are E runs of n = 16 / E consecutive ones, run h at tile row 8n*h + n*g: store h of the eight lanes of one
    // sample then covers 128 contiguous bytes, a whole line, for every element size
    constexpr uint32_t n = 16u / E;
    __shared__ gt_v4u stage4[kTileVariants * 8u];   // [row][32 dwords], dword c of row v at ((c + 4 * ((v / n) % 8)) % 32)
    uint32_t *const stage = reinterpret_cast<uint32_t *>(stage4);
    const Table<E> tab(a);
    const uint32_t N = a.sample_count, R = a.record_size;
    const uint64_t V = a.n_variants;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, g = lane & 7u, q = lane >> 3;

    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const uint64_t band = tile / v_tiles, vt = tile - band * v_tiles;
        const uint64_t j0 = vt * kTileVariants;
        const uint32_t cb0 = (uint32_t)band * (kTileSamples / 4u);   // first record byte of the band
        // stage: thread t takes 16-byte chunk t % 8 of rows t / 8 + 32 i
        gt_v4u ld[4];
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t v = (t >> 3) + 32u * i, cb = cb0 + 16u * (t & 7u);
            ld[i] = gt_v4u{0u, 0u, 0u, 0u};
            if (j0 + v < V && cb < R) {
                const uint8_t *p = row_record(a, j0 + v) + cb;
                if (cb + 16u <= R) {
                    ld[i] = load16_unaligned(p);
                } else {
                    for (uint32_t b = 0; b < R - cb; b++) ld[i][b >> 2] |= (uint32_t)p[b] << (8u * (b & 3u));
                }
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t v = (t >> 3) + 32u * i;
            stage4[v * 8u + (((t & 7u) + v / n) & 7u)] = ld[i];
        }
        __syncthreads();

        // 16 rows x 16 samples of codes -> 16 samples x 16 variants
        uint32_t x[16];
#pragma unroll
        for (uint32_t r = 0; r < 16u; r++) x[r] = stage[(8u * n * (r / n) + n * g + r % n) * 32u + ((8u * wave + q + 4u * g) & 31u)];
#pragma unroll
        for (uint32_t dlog = 4u; dlog-- > 0u;) {
            const uint32_t dd = 1u << dlog;
            const uint32_t m = dd == 8u ? 0x0000FFFFu : dd == 4u ? 0x00FF00FFu : dd == 2u ? 0x0F0F0F0Fu : 0x33333333u;
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) {
                if (i & dd) continue;
                const uint32_t tt = ((x[i] >> (2u * dd)) ^ x[i + dd]) & m;
                x[i + dd] ^= tt;
                x[i] ^= tt << (2u * dd);
            }
        }
        __syncthreads();   // the stage is free for the next tile

        const uint32_t s0 = (uint32_t)band * kTileSamples + wave * kWaveSamples + 16u * q;   // this lane's 16 samples
        if (s0 >= N) continue;
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) {
            if (s0 + i >= N) break;
            uint8_t *const row = a.out + (uint64_t)(s0 + i) * a.out_stride;
#pragma unroll
            for (uint32_t h = 0; h < (uint32_t)E; h++) {
                const uint64_t jb = j0 + 8u * n * h + n * g;   // run h: variants jb .. jb + n - 1, codes at bits 2nh of x[i]
                const uint32_t codes = x[i] >> (2u * n * h);
                if (jb + n <= V) {
                    uint32_t d[4];
                    tab.expand_chunk(codes, d);
                    store16(row + jb * E, d);
                } else if (jb < V) {
#pragma unroll 1
                    for (uint32_t r = 0; r < (uint32_t)(V - jb); r++) store_elem<E>(row + (jb + r) * E, tab.value((codes >> (2u * r)) & 3u));
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_gt_matrix_general(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    const uint64_t total = (uint64_t)a.n_variants * a.kept_count;
    const dim3 grid(general_grid(a.n_variants, a.kept_count, num_cus, blocks)), block(kThreads);
    switch (a.elem_bytes) {
        case 1u: hipLaunchKernelGGL(gt_matrix_general_kernel<1>, grid, block, 0, stream, a, total); break;
        case 2u: hipLaunchKernelGGL(gt_matrix_general_kernel<2>, grid, block, 0, stream, a, total); break;
        default: hipLaunchKernelGGL(gt_matrix_general_kernel<4>, grid, block, 0, stream, a, total); break;
    }
    return hipGetLastError();
}

hipError_t launch_gt_matrix_stream(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    const StreamPlan p = stream_plan(a.n_variants, a.kept_count, a.elem_bytes, (uint32_t)((uintptr_t)a.out & 15u), a.out_stride, num_cus, blocks);
    const dim3 grid(p.grid_x, p.grid_y), block(kThreads);
    if (p.long_rows) {
        switch (a.elem_bytes) {
            case 1u: hipLaunchKernelGGL(gt_matrix_stream_rows_kernel<1>, grid, block, 0, stream, a, (uint32_t)p.per_row); break;
            case 2u: hipLaunchKernelGGL(gt_matrix_stream_rows_kernel<2>, grid, block, 0, stream, a, (uint32_t)p.per_row); break;
            default: hipLaunchKernelGGL(gt_matrix_stream_rows_kernel<4>, grid, block, 0, stream, a, (uint32_t)p.per_row); break;
        }
        return hipGetLastError();
    }
    const double inv = 1.0 / (double)(p.dense ? (uint64_t)a.kept_count : p.per_row);   // the kernel divides through a reciprocal
    switch (a.elem_bytes) {
        case 1u: hipLaunchKernelGGL(gt_matrix_stream_kernel<1>, grid, block, 0, stream, a, p.dense, p.per_row, p.total, inv); break;
        case 2u: hipLaunchKernelGGL(gt_matrix_stream_kernel<2>, grid, block, 0, stream, a, p.dense, p.per_row, p.total, inv); break;
        default: hipLaunchKernelGGL(gt_matrix_stream_kernel<4>, grid, block, 0, stream, a, p.dense, p.per_row, p.total, inv); break;
    }
    return hipGetLastError();
}

hipError_t launch_gt_matrix_tile(const MatrixArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0 || a.kept_count == 0) return hipSuccess;
    const TilePlan p = tile_plan(a.n_variants, a.sample_count, num_cus, blocks);
    const dim3 grid(p.grid), block(kThreads);
    switch (a.elem_bytes) {
        case 1u: hipLaunchKernelGGL(gt_matrix_tile_kernel<1>, grid, block, 0, stream, a, p.v_tiles, p.total); break;
        case 2u: hipLaunchKernelGGL(gt_matrix_tile_kernel<2>, grid, block, 0, stream, a, p.v_tiles, p.total); break;
        default: hipLaunchKernelGGL(gt_matrix_tile_kernel<4>, grid, block, 0, stream, a, p.v_tiles, p.total); break;
    }
    return hipGetLastError();
}

}  // namespace pgenhip
