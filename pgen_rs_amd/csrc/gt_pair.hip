// gt_pair.hip — windowed pairwise genotype tables for gfx950 (MI355X): for every pair of selected rows (i, i + d), 0 <= i < n_left,
// 1 <= d <= W, i + d < n_variants, the 4 x 4 table T[a][b] = number of kept samples with code a in row i and code b in row i + d
// (codes as everywhere: 0 hom-ref, 1 het, 2 hom-alt, 3 missing; src/pfile.rs:172-183), or the unphased genotype r^2 of that table.
//
// The first kernel here that re-uses rows: a row is read once per tile it belongs to and then meets 16 partner rows from LDS, so
// the work is ANDs and popcounts, not bytes.  Per 32 samples (record dwords w0, w1, m = 0x55555555):
//   L = (w0 & m) | ((w1 << 1) & ~m),  H = ((w0 >> 1) & m) | (w1 & ~m)          (v_bfi_b32: the low / high code bit planes)
//   c1 = L & ~H & keep,  c2 = H & ~L & keep,  c3 = L & H & keep                 (het, hom-alt, missing of the counted samples)
// `keep` is the ctx's kept mask put through the same plane split (or, with all samples kept, the samples < N), so the N tail, the
// pad bits and the unkept samples are gone before anything is counted.  A pair's nine cells with a, b in {1, 2, 3} are
// popc(c_a(i) & c_b(j)) (v_and_b32 + v_bcnt_u32_b32, which adds into its accumulator); the seven cells with a zero index follow
// from the rows' own totals of c1, c2, c3 (counted once per row and tile while staging, not once per pair) and K.
//
// Work item: a tile of 16 left x 16 right rows on the 16-row grid that meets the band 1 <= j - i <= W, i < n_left.  One wave per
// tile; lane (ty, tx) of 8 x 8 owns the 2 x 2 pairs (2 ty + {0, 1}, 2 tx + {0, 1}): 36 u32 accumulators.  The wave walks the
// samples in chunks of 512 (128 record bytes per row): lane (row slot, piece) loads 16 bytes of a row as two aligned 16-byte
// loads funnelled to the row's phase (any record alignment; bytes of neighbouring rows only reach positions the mask clears),
// splits planes and writes the three vectors of its two 32-sample words to LDS at [word][vector][row slot].  The word stride is
// 100 dwords, so the 8 pieces x 8 rows of a staging store hit 64 distinct banks, and an accumulation step's ds_read_b64 of two
// neighbouring row slots is 8 distinct addresses inside one 128-byte line (broadcast, conflict-free).  On a diagonal tile (left
// rows = right rows) the 16 rows are staged once and both operands read the same slots.
//
// Tiles are numbered (left tile) * tiles_per_left + k, right tile = left tile + k, and the grid strides over the numbers; the few
// numbers at the ragged end whose tile lies outside the band or past the last row leave at once without touching memory.  Every
// pair has exactly one owner lane: no atomics, no counters, no scratch, nothing allocated, graph-capturable.
//
// The third epilogue (pgenhip_pair_mask) keeps one bit per pair instead: the pair's r^2 above a threshold and, with
// keys, the rows' keys inside a span (which is how a window in base pairs is expressed).  A row's bits of one tile are neighbours
// in one or two mask words; the lanes that hold them combine them with shuffles and one lane per row ORs them in with an atomic
// (rows of a mask are shared between tiles), a tile without an edge writes nothing.
// Not built: splitting one pair's samples over several blocks (few rows of very long records leave CUs idle), explicit pair
// lists.
#include <math.h>

#include <type_traits>

#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::pair;                             // kThreads (one wave per tile), kTile, kChunkWords, kBlocksPerCu and the launch plan
constexpr uint32_t kPieces = kChunkWords / 2;           // 16-byte pieces of a row per chunk
constexpr uint32_t kSlots = 2 * kTile;                  // row slots: 0-15 left, 16-31 right
constexpr uint32_t kWordStride = 3 * kSlots + 4;        // dwords per staged word; 2 * 100 = 8 (mod 64): see the header comment

static_assert(kThreads == 64 && kPieces == 8 && kSlots == 32, "lane <-> (piece, row slot) and (ty, tx) maps below");

// bits [0, 2n) of a word, n in [0, 16]
__device__ __forceinline__ uint32_t low_sample_bits(int32_t n) { return n >= 16 ? 0xFFFFFFFFu : ((1u << (2 * n)) - 1u); }

// low code bits of the 32 samples of a dword pair, bit 2i = sample i of w0, bit 2i + 1 = sample i of w1; the high bits alike
__device__ __forceinline__ uint32_t plane_lo(uint32_t w0, uint32_t w1) { return (w0 & 0x55555555u) | ((w1 << 1) & 0xAAAAAAAAu); }
__device__ __forceinline__ uint32_t plane_hi(uint32_t w0, uint32_t w1) { return ((w0 >> 1) & 0x55555555u) | (w1 & 0xAAAAAAAAu); }

// r^2 of the called-in-both part of a table.  The three terms are exact 64-bit integers (K < 2^31: n * Sxy <= 4 n^2 < 2^64);
// doubles from there on, one rounding to float.
__device__ __forceinline__ float table_r2(const uint32_t (&t)[4][4])
{
    uint64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (uint32_t x = 0; x < 3u; x++)
#pragma unroll
        for (uint32_t y = 0; y < 3u; y++) {
            const uint64_t c = t[x][y];
            n += c;
            sx += x * c;
            sy += y * c;
            sxx += x * x * c;
            syy += y * y * c;
            sxy += x * y * c;
        }
    const uint64_t p = n * sxy, q = sx * sy;
    const uint64_t cov = p >= q ? p - q : q - p;   // magnitude; the sign is squared away
    const uint64_t vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
    if (vx == 0u || vy == 0u) return __builtin_nanf("");
    const double c = (double)cov;
    return (float)((c * c) / ((double)vx * (double)vy));
}

// 16 edge bits of one row and tile, bit t = the partner at b0 + t (b0 >= -16; bits below mask bit 0 are clear by construction):
// OR into the one or two mask words that hold a set bit, nothing else is touched
__device__ __forceinline__ void or_mask_bits(uint32_t *row_words, int64_t b0, uint32_t bits16)
{
    if (bits16 == 0u) return;
    uint64_t bits = bits16;
    uint64_t bit0 = 0u;
    if (b0 < 0) {
        bits >>= (uint32_t)(-b0);
    } else {
        bit0 = (uint64_t)b0;
        bits <<= (uint32_t)(bit0 & 31u);
    }
    uint32_t *w = row_words + (bit0 >> 5);
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    if (lo) atomicOr(w, lo);
    if (hi) atomicOr(w + 1, hi);
}

// Args = PairArgs: tables or r^2 (a.r2), one owner lane per entry.  Args = PairMaskArgs: the same tile, staging and accumulation, and
// an epilogue that keeps one bit per pair (the r^2 above a threshold, the keys inside a span): a row's 16 partner bits of the tile are
// ORed together across the eight lanes that hold them (three shuffles), then one lane per row ORs them into the mask.
template <class Args>
__global__ __launch_bounds__(kThreads) void gt_pair_kernel(Args a, uint64_t n_items, uint64_t tiles_per_left)
{
    constexpr bool kMask = std::is_same<Args, PairMaskArgs>::value;
    __shared__ __attribute__((aligned(16))) uint32_t vec[kChunkWords * kWordStride];
    __shared__ uint32_t marg[kSlots * 3];
    const uint32_t lane = threadIdx.x;
    const uint32_t piece = lane & 7u, srow = lane >> 3;   // staging: 16-byte piece of the chunk, row slot within a round of 8
    const uint32_t tx = lane & 7u, ty = lane >> 3;        // accumulation: right rows 2 tx + {0, 1}, left rows 2 ty + {0, 1}
    const uint32_t N = a.sample_count, R = a.record_size;
    const uint64_t V = a.n_variants, W = a.window;
    const uint32_t n_chunks = (N + 32u * kChunkWords - 1u) / (32u * kChunkWords);

    for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint64_t lt = item / tiles_per_left, rt = lt + item % tiles_per_left;
        const uint64_t i0 = lt * kTile, j0 = rt * kTile;
        const uint64_t i_last = min(i0 + kTile - 1u, (uint64_t)a.n_left - 1u);
        if (j0 >= V || j0 > i_last + W) continue;          // (block-uniform) outside the band or past the last row
        const bool diag = rt == lt;
        const uint32_t rbase = diag ? 0u : kTile;          // slot of right row 0

        const uint8_t *base[4];
        uint32_t d[4], nch[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t slot = k * 8u + srow;
            const uint64_t row = slot < kTile ? i0 + slot : j0 + (slot - kTile);
            const bool live = (k < 2u || !diag) && row < V;
            const uint8_t *rec = live ? row_record(a, row) : a.records;
            d[k] = (uint32_t)(uintptr_t)rec & 15u;
            base[k] = rec - d[k];   // (pointer arithmetic on the argument keeps the loads global, not flat)
            nch[k] = live && R ? (d[k] + R + 15u) >> 4 : 0u;   // aligned 16-byte chunks the row's bytes touch
        }

        uint32_t acc[2][2][9];
        uint32_t mg[4][3];
#pragma unroll
        for (uint32_t x = 0; x < 36u; x++) (&acc[0][0][0])[x] = 0u;
#pragma unroll
        for (uint32_t x = 0; x < 12u; x++) (&mg[0][0])[x] = 0u;

        for (uint32_t c = 0; c < n_chunks; c++) {
            // ---- stage: rows' bytes [16 ch, 16 ch + 16) -> three masked vectors of words 2 piece, 2 piece + 1
            const uint32_t ch = c * kPieces + piece;
            const bool piece_live = (uint64_t)ch * 16u < R;
            gt_v4u lo[4], hi[4], keep;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                lo[k] = gt_v4u{0u, 0u, 0u, 0u};
                hi[k] = gt_v4u{0u, 0u, 0u, 0u};
                if (k < 2u || !diag) {
                    if (ch < nch[k]) lo[k] = *reinterpret_cast<const gt_v4u *>(base[k] + 16ull * ch);
                    if (ch + 1u < nch[k]) hi[k] = *reinterpret_cast<const gt_v4u *>(base[k] + 16ull * (ch + 1u));
                }
            }
            if (a.kept_mask != nullptr) {
                keep = piece_live ? *reinterpret_cast<const gt_v4u *>(a.kept_mask + 16ull + 16ull * ch) : gt_v4u{0u, 0u, 0u, 0u};
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    const int64_t left = (int64_t)N - (64ll * ch + 16ll * q);   // samples of the row from this dword's first on
                    keep[q] = 0x55555555u & low_sample_bits((int32_t)min<int64_t>(max<int64_t>(left, 0), 16));
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                if (k < 2u || !diag) {
                    const gt_v4u w = funnel16(lo[k], hi[k], d[k]);
                    const uint32_t slot = k * 8u + srow;
#pragma unroll
                    for (uint32_t h = 0; h < 2u; h++) {
                        const uint32_t L = plane_lo(w[2 * h], w[2 * h + 1]), H = plane_hi(w[2 * h], w[2 * h + 1]);
                        const uint32_t M = plane_lo(keep[2 * h], keep[2 * h + 1]);   // 0b01 per kept sample: its low plane is the kept bit
                        const uint32_t c1 = L & ~H & M, c2 = H & ~L & M, c3 = L & H & M;
                        uint32_t *dst = vec + (2u * piece + h) * kWordStride + slot;
                        dst[0] = c1;
                        dst[kSlots] = c2;
                        dst[2 * kSlots] = c3;
                        mg[k][0] += __builtin_popcount(c1);
                        mg[k][1] += __builtin_popcount(c2);
                        mg[k][2] += __builtin_popcount(c3);
                    }
                }
            }
            __syncthreads();
            // ---- accumulate: the words of this chunk that hold samples < N
            const uint32_t left_words = (N - c * 32u * kChunkWords + 31u) / 32u;
            const uint32_t nw = left_words < kChunkWords ? left_words : kChunkWords;
            for (uint32_t wd = 0; wd < nw; wd++) {
                const uint32_t *p = vec + wd * kWordStride;
                uint2 l[3], r[3];
#pragma unroll
                for (uint32_t v = 0; v < 3u; v++) {
                    l[v] = *reinterpret_cast<const uint2 *>(p + v * kSlots + 2u * ty);
                    r[v] = *reinterpret_cast<const uint2 *>(p + v * kSlots + rbase + 2u * tx);
                }
#pragma unroll
                for (uint32_t u = 0; u < 3u; u++)
#pragma unroll
                    for (uint32_t v = 0; v < 3u; v++) {
                        acc[0][0][3 * u + v] += __builtin_popcount(l[u].x & r[v].x);
                        acc[0][1][3 * u + v] += __builtin_popcount(l[u].x & r[v].y);
                        acc[1][0][3 * u + v] += __builtin_popcount(l[u].y & r[v].x);
                        acc[1][1][3 * u + v] += __builtin_popcount(l[u].y & r[v].y);
                    }
            }
            __syncthreads();
        }

        // ---- the rows' own totals: eight pieces -> one number per row slot and vector
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
            for (uint32_t v = 0; v < 3u; v++) {
                uint32_t s = mg[k][v];
                s += __shfl_xor(s, 1, 8);
                s += __shfl_xor(s, 2, 8);
                s += __shfl_xor(s, 4, 8);
                if (piece == 0u) marg[(k * 8u + srow) * 3u + v] = s;
            }
        __syncthreads();

        // ---- epilogue: 2 x 2 pairs per lane
        [[maybe_unused]] uint32_t fwd_bits = 0u, bwd_bits = 0u;   // mask mode: this lane's edges, two 16-bit halves each
#pragma unroll
        for (uint32_t x = 0; x < 2u; x++)
#pragma unroll
            for (uint32_t y = 0; y < 2u; y++) {
                const uint64_t i = i0 + 2u * ty + x, j = j0 + 2u * tx + y;
                if (i >= a.n_left || j <= i || j - i > W || j >= V) continue;   // (no lane leaves the wave: the mask epilogue shuffles below)
                const uint32_t *mi = marg + (2u * ty + x) * 3u, *mj = marg + (rbase + 2u * tx + y) * 3u;
                uint32_t t[4][4];
                uint32_t rows_called = 0u, top = 0u;
#pragma unroll
                for (uint32_t u = 1; u < 4u; u++) {
                    uint32_t s = 0u;
#pragma unroll
                    for (uint32_t v = 1; v < 4u; v++) {
                        t[u][v] = acc[x][y][3 * (u - 1) + (v - 1)];
                        s += t[u][v];
                    }
                    t[u][0] = mi[u - 1] - s;
                    rows_called += mi[u - 1];
                }
#pragma unroll
                for (uint32_t v = 1; v < 4u; v++) {
                    t[0][v] = mj[v - 1] - t[1][v] - t[2][v] - t[3][v];
                    top += t[0][v];
                }
                t[0][0] = a.kept_count - rows_called - top;
                if constexpr (kMask) {
                    // NaN compares false; the key difference is taken mod 2^64, so a partner with a smaller key is far away
                    if (table_r2(t) > a.min_r2 && (a.key == nullptr || a.key[j] - a.key[i] <= a.max_span)) {
                        fwd_bits |= 1u << (16u * x + 2u * tx + y);             // row i's partner at j0 + (2 tx + y)
                        bwd_bits |= 1u << (16u * y + 15u - (2u * ty + x));     // row j's partner at i0 + 15 - (bit)
                    }
                } else {
                    const uint64_t p = i * W + (j - i - 1u);
                    if (a.r2) {
                        static_cast<float *>(a.out)[p] = table_r2(t);
                    } else {
                        gt_v4u *dst = reinterpret_cast<gt_v4u *>(static_cast<uint32_t *>(a.out) + 16ull * p);
#pragma unroll
                        for (uint32_t u = 0; u < 4u; u++) dst[u] = gt_v4u{t[u][0], t[u][1], t[u][2], t[u][3]};
                    }
                }
            }
        if constexpr (kMask) if (__ballot(fwd_bits != 0u) != 0ull) {   // (wave-uniform; most tiles of real data hold no edge at all)
            // forward: the lanes tx = 0 .. 7 of one ty hold the 16 partners of rows i0 + 2 ty + {0, 1}; bit t of a half = j0 + t
            fwd_bits |= __shfl_xor(fwd_bits, 1, 8);
            fwd_bits |= __shfl_xor(fwd_bits, 2, 8);
            fwd_bits |= __shfl_xor(fwd_bits, 4, 8);
            // backward: the lanes ty = 0 .. 7 of one tx hold the 16 partners of rows j0 + 2 tx + {0, 1}; bit t of a half = i0 + 15 - t
            bwd_bits |= __shfl_xor(bwd_bits, 8);
            bwd_bits |= __shfl_xor(bwd_bits, 16);
            bwd_bits |= __shfl_xor(bwd_bits, 32);
            if (tx == 0u) {
#pragma unroll
                for (uint32_t x = 0; x < 2u; x++) {
                    const uint64_t i = i0 + 2u * ty + x;   // bit b = j - i - 1 of row i: j = j0 + t
                    or_mask_bits(a.fwd + i * a.mask_stride, (int64_t)(j0 - i) - 1, (fwd_bits >> (16u * x)) & 0xFFFFu);
                }
            }
            if (ty == 0u && a.bwd != nullptr) {
#pragma unroll
                for (uint32_t y = 0; y < 2u; y++) {
                    const uint64_t j = j0 + 2u * tx + y;   // bit b = j - i - 1 of row j: i = i0 + 15 - t
                    or_mask_bits(a.bwd + j * a.mask_stride, (int64_t)(j - i0) - 16, (bwd_bits >> (16u * y)) & 0xFFFFu);
                }
            }
        }
        __syncthreads();   // marg and vec are rewritten by the next item
    }
}

}  // namespace

template <class Args>
static hipError_t launch(const Args &a, int blocks, int num_cus, hipStream_t stream)
{
    const uint64_t V = a.n_variants;
    if (a.n_left == 0 || V <= 1) return hipSuccess;
    const plan::pair::Plan p = plan::pair::plan(a.n_variants, a.n_left, a.window, num_cus, blocks);
    hipLaunchKernelGGL(gt_pair_kernel<Args>, dim3(p.grid), dim3(kThreads), 0, stream, a, p.n_items, p.tiles_per_left);
    return hipGetLastError();
}

hipError_t launch_gt_pair(const PairArgs &a, int blocks, int num_cus, hipStream_t stream) { return launch(a, blocks, num_cus, stream); }
hipError_t launch_gt_pair_mask(const PairMaskArgs &a, int blocks, int num_cus, hipStream_t stream) { return launch(a, blocks, num_cus, stream); }

}  // namespace pgenhip
