// gt_parse.hip — GT text to packed records for gfx950 (MI355X): the inverse of decode_emit.  For line j the sample fields of
// text[field_off[j], line_end[j]) become the line's mode-0x02 record (sample s in byte s/4, bits 2*(s%4), LSB first, pad bits
// zero) and a word of PGENHIP_PARSE_* flags.  The grammar is the one of include/pgen_hip.h (tests/parse_ref.py restates it):
// fields introduced by '\t', a field's GT its bytes up to the first ':', an allele [0-9]+ or '.', a GT `A` or `A [/|] B`.
//
// Two shapes:
//   GENERAL  fields of any width.  A block per line; the line goes by in chunks of plan::parse::kChunkBytes, four bytes per lane
//            (one aligned dword load inside the region, byte loads at its ends).  Tabs are counted by a block scan on top of a
//            count that runs on from chunk to chunk, so every tab knows its field's ordinal; the tab's owner parses the field
//            behind it straight from memory (a GT is a few bytes: the bytes behind a ':' are never read as a GT) and puts the code
//            into an LDS window, from which the block stores whole record bytes; up to three codes wait there for the next chunk.
//            One line is not split over blocks: a call with few very long lines uses few CUs (as pair_stats' tiles do).
//   FIXED    what this project's own emit path writes: a region of exactly 4N bytes, every field `\t[01.][/|][01.]`.  Positions
//            are known, so the launch is flat over (line, piece): a lane takes one record byte = four fields = 16 text bytes
//            (one 16-byte load at whatever alignment the text has: the piece lies inside the region; bytes on a line's last,
//            partial piece), four pieces per lane and turn with all their loads in flight together.  Short rows share a block, a long row spreads over many.  A line that is not
//            4N bytes or has a field outside the pattern is declined as a whole: its pieces may sit in different blocks, so
//            declining is an atomic OR of PGENHIP_PARSE_DECLINED into the line's flag word (PHASED and HALF_CALL travel the same
//            way: one atomic per line and wave, and none at all for a wave of unphased whole calls).
// No scratch, no work counters; the flag words are zeroed by a memset ahead of a FIXED launch.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::parse;   // kThreads, kWaves, kChunkBytes, kPieceText and the launch plans

constexpr uint32_t kTab = 0x09u;
constexpr uint32_t kFieldHomRef = 0x302F3009u;   // "\t0/0": code 0, what the fields behind a line's last one count as (pad bits)

// ---- the grammar, one field --------------------------------------------------------------------------------------------------------
// The field behind the tab at p - 1: its code in bits 0-1, its flag bits from bit 8.  `end` is the region's end and acts as a tab.
__device__ __forceinline__ uint32_t parse_field(const uint8_t *__restrict__ text, uint64_t p, uint64_t end)
{
    constexpr uint32_t kBad = 3u | (PGENHIP_PARSE_BAD_CALL << 8);
    auto at = [&](uint64_t x) -> uint32_t { return x < end ? (uint32_t)text[x] : kTab; };
    uint32_t c = at(p);
    uint32_t v[2] = {0u, 0u};   // 0, 1; 2 = '.'; 3 = a digit token other than "0" and "1"
    uint32_t n_alleles = 0u;
    bool phased = false;
    for (;;) {
        if (c == '.') {
            v[n_alleles] = 2u;
            c = at(++p);
        } else if (c - '0' < 10u) {
            const uint32_t first = c;
            uint32_t digits = 0u;
            do {
                digits++;
                c = at(++p);
            } while (c - '0' < 10u);
            v[n_alleles] = digits == 1u && first <= '1' ? first - '0' : 3u;
        } else {
            return kBad;   // an empty allele, or another byte
        }
        n_alleles++;
        if (c == kTab || c == ':') break;
        if (n_alleles == 2u || (c != '/' && c != '|')) return kBad;
        phased = c == '|';
        c = at(++p);
    }
    if (v[0] == 3u || v[1] == 3u) return 3u | (PGENHIP_PARSE_ALLELE_RANGE << 8);
    if (n_alleles == 1u) return (v[0] == 2u ? 3u : 2u * v[0]) | (PGENHIP_PARSE_HAPLOID << 8);
    const uint32_t miss = (v[0] == 2u) + (v[1] == 2u);
    const uint32_t fl = (phased ? PGENHIP_PARSE_PHASED : 0u) | (miss == 1u ? PGENHIP_PARSE_HALF_CALL : 0u);
    return (miss ? 3u : v[0] + v[1]) | (fl << 8);
}

// ---- GENERAL -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gt_parse_general_kernel(ParseArgs a, uint32_t declined_only)
{
    __shared__ uint8_t s_codes[kChunkBytes + 4u];   // the window: up to 3 codes carried over + one per tab of the chunk
    __shared__ uint32_t s_wave_tabs[kWaves];
    __shared__ uint32_t s_flags;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t N = a.sample_count;
    const uint32_t R = a.record_size;
    const uint8_t *__restrict__ text = a.text;

    // A block takes the lines blockIdx.x + k * gridDim.x.  Which of its next kThreads turns it has to take (all of them, or under
    // AUTO the declined ones) it looks up side by side, a turn per lane: a pass over millions of lines that FIXED has taken is then a
    // few rounds of parallel flag loads per block, not a chain of dependent ones.
    __shared__ uint8_t s_pick[kThreads];
    for (uint64_t k0 = 0; blockIdx.x + k0 * gridDim.x < a.n_lines; k0 += kThreads) {   // block-uniform
        const uint64_t jt = blockIdx.x + (k0 + tid) * gridDim.x;
        const bool take = jt < a.n_lines && (!declined_only || (a.line_flags[jt] & PGENHIP_PARSE_DECLINED) != 0u);
        if (!__syncthreads_or(take)) continue;
        s_pick[tid] = take;
        __syncthreads();
        for (uint32_t t = 0; t < (uint32_t)kThreads; t++) {
            if (!s_pick[t]) continue;
            const uint64_t j = blockIdx.x + (k0 + t) * gridDim.x;
            uint64_t fo = min(a.field_off[j], a.text_len);
            uint64_t le = min(a.line_end[j], a.text_len);
            if (fo > le) fo = le;
            if (fo < le && text[fo] != kTab) le = fo;   // a region that does not begin with a tab has no fields
            if (tid == 0u) s_flags = 0u;
            __syncthreads();   // (also: the line before is done with the window)
            uint8_t *const out = a.out + j * a.out_stride;
            uint32_t my_flags = 0u;
            uint64_t n_fields = 0;   // tabs in front of the chunk
            uint64_t w0 = 0;         // first sample of the window (a multiple of 4): the record bytes before it are stored
            uint32_t carry = 0;      // codes in the window
            const int64_t start = (int64_t)fo - (int64_t)((uintptr_t)(text + fo) & 3u);   // dwords of the chunks are aligned

            for (int64_t c0 = start; c0 < (int64_t)le; c0 += kChunkBytes) {
                const int64_t q = c0 + 4 * (int64_t)tid;
                uint32_t w = 0u;   // bytes outside the region read as 0: no tab
                if (q >= (int64_t)fo && q + 4 <= (int64_t)le) {
                    w = *reinterpret_cast<const uint32_t *>(text + q);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (q + i >= (int64_t)fo && q + i < (int64_t)le) w |= (uint32_t)text[q + i] << (8 * i);
                }
                uint32_t cnt = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) cnt += ((w >> (8 * i)) & 0xFFu) == kTab;
                // block scan of the tab counts
                uint32_t incl = cnt;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                    if (lane >= (uint32_t)d) incl += up;
                }
                if (lane == 63u) s_wave_tabs[wave] = incl;
                __syncthreads();
                uint32_t before = 0u, chunk_tabs = 0u;
#pragma unroll
                for (uint32_t i = 0; i < kWaves; i++) {
                    const uint32_t wt = s_wave_tabs[i];
                    before += i < wave ? wt : 0u;
                    chunk_tabs += wt;
                }
                uint32_t k = before + incl - cnt;   // tabs of the chunk in front of this lane's
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (((w >> (8 * i)) & 0xFFu) != kTab) continue;
                    if (n_fields + k < N) {   // (fields past the last sample are counted, not read)
                        const uint32_t r = parse_field(text, (uint64_t)(q + i + 1), le);
                        s_codes[carry + k] = (uint8_t)(r & 3u);   // (w0 + carry == n_fields while samples are left)
                        my_flags |= r >> 8;
                    }
                    k++;
                }
                __syncthreads();
                n_fields += chunk_tabs;
                const uint32_t avail = (uint32_t)(min(n_fields, N) - w0);   // codes in the window now
                const uint32_t n_bytes = avail >> 2, left = avail & 3u;
                if (tid < n_bytes) {
                    const uint32_t v = (uint32_t)s_codes[4u * tid] | ((uint32_t)s_codes[4u * tid + 1u] << 2) | ((uint32_t)s_codes[4u * tid + 2u] << 4) |
                                       ((uint32_t)s_codes[4u * tid + 3u] << 6);
                    out[(w0 >> 2) + tid] = (uint8_t)v;
                }
                const uint32_t keep = tid < left ? (uint32_t)s_codes[4u * n_bytes + tid] : 0u;
                __syncthreads();
                if (tid < left) s_codes[tid] = (uint8_t)keep;
                w0 += 4ull * n_bytes;
                carry = left;
            }
            __syncthreads();   // (the carried codes are in place)
            // the record bytes from the window on: carried codes, then samples without a field (3), then pad bits (0)
            const uint64_t have = min(n_fields, N);
            for (uint64_t b = (w0 >> 2) + tid; b < R; b += kThreads) {
                uint32_t v = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const uint64_t s = 4ull * b + i;
                    const uint32_t c = s < have ? (uint32_t)s_codes[(uint32_t)(s - w0)] : s < N ? 3u : 0u;
                    v |= c << (2u * i);
                }
                out[b] = (uint8_t)v;
            }
            if (my_flags) atomicOr(&s_flags, my_flags);
            __syncthreads();
            if (tid == 0u) a.line_flags[j] = s_flags | (n_fields != N ? PGENHIP_PARSE_FIELD_COUNT : 0u);
        }
        __syncthreads();   // (the round's picks are read no more)
    }
}

// ---- FIXED -------------------------------------------------------------------------------------------------------------------------
// a line's last piece when N is no multiple of 4: its n fields byte by byte, the others read as "\t0/0"
__device__ __forceinline__ gt_v4u load_partial_piece(const uint8_t *__restrict__ p, uint32_t n)
{
    gt_v4u w = {kFieldHomRef, kFieldHomRef, kFieldHomRef, kFieldHomRef};
#pragma unroll
    for (uint32_t f = 0; f < 3u; f++) {
        if (f < n) {
            const uint8_t *q = p + 4u * f;
            w[f] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        }
    }
    return w;
}

// four fields: their codes as a record byte; PHASED / HALF_CALL, or DECLINED alone for a field outside `\t[01.][/|][01.]`
__device__ __forceinline__ uint32_t decode_piece(gt_v4u w, uint32_t &fl)
{
    uint32_t code = 0u, bad = 0u;
    fl = 0u;
#pragma unroll
    for (uint32_t f = 0; f < 4u; f++) {
        const uint32_t x = w[f];
        const uint32_t ca = (x >> 8) & 0xFFu, cs = (x >> 16) & 0xFFu, cb = x >> 24;
        const uint32_t ma = ca == '.', mb = cb == '.';
        bad |= (x & 0xFFu) != kTab;
        bad |= !(ma | ((ca & 0xFEu) == '0'));
        bad |= !(mb | ((cb & 0xFEu) == '0'));
        bad |= !((cs == '/') | (cs == '|'));
        fl |= cs == '|' ? PGENHIP_PARSE_PHASED : 0u;
        fl |= ma != mb ? PGENHIP_PARSE_HALF_CALL : 0u;
        code |= ((ma | mb) ? 3u : (ca & 1u) + (cb & 1u)) << (2u * f);
    }
    if (bad) fl = PGENHIP_PARSE_DECLINED;
    return code;
}

// A lane takes kLanePieces pieces per turn, kThreads items apart (so each of its loads is coalesced with its neighbours'): the
// offsets of all of them are loaded first, then the text of all of them, so four 16-byte loads per lane are in flight instead of
// one behind a dependent pair of offset loads.
template <bool VALIDATE, bool WRITE>
__global__ __launch_bounds__(kThreads) void gt_parse_fixed_kernel(ParseArgs a, uint32_t P, uint64_t total)
{
    constexpr uint32_t U = kLanePieces;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t N = a.sample_count, R = a.record_size;
    const bool small = total <= 0xFFFFFFFFull;
    // block-uniform trip count: every lane of a wave takes part in the ballots below
    for (uint64_t i0 = (uint64_t)blockIdx.x * kBlockPieces; i0 < total; i0 += (uint64_t)gridDim.x * kBlockPieces) {
        uint64_t j[U], fo[U], le[U];
        uint32_t b[U], lf[U], fl[U];
        bool live[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint64_t at = i0 + u * (uint32_t)kThreads + tid;
            live[u] = at < total;
            const uint64_t idx = live[u] ? at : total - 1u;
            if (small) {
                j[u] = (uint32_t)idx / P;
                b[u] = (uint32_t)idx % P;
            } else {
                j[u] = idx / P;
                b[u] = (uint32_t)(idx - j[u] * P);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            fo[u] = a.field_off[j[u]];
            le[u] = a.line_end[j[u]];
            lf[u] = VALIDATE ? 0u : a.line_flags[j[u]];   // the write pass of forced FIXED: the validate pass has spoken
        }
        bool work[U], full[U];
        gt_v4u w[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            fo[u] = min(fo[u], a.text_len);
            le[u] = min(le[u], a.text_len);
            const bool len_ok = le[u] >= fo[u] && le[u] - fo[u] == 4ull * N;
            const bool declined = !len_ok || (lf[u] & PGENHIP_PARSE_DECLINED) != 0u;
            fl[u] = live[u] && !len_ok && b[u] == 0u ? PGENHIP_PARSE_DECLINED : 0u;   // one lane speaks for the line
            // a declined line says nothing else (the bit stays: the line's other lanes may still read it)
            if (!VALIDATE && live[u] && declined && b[u] == 0u) a.line_flags[j[u]] = PGENHIP_PARSE_DECLINED;
            work[u] = live[u] && !declined && b[u] < R;
            full[u] = work[u] && N - 4u * b[u] >= 4u;
            w[u] = gt_v4u{kFieldHomRef, kFieldHomRef, kFieldHomRef, kFieldHomRef};
            if (full[u]) __builtin_memcpy(&w[u], a.text + fo[u] + 16ull * b[u], 16);   // the whole piece lies in the region: any alignment
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            if (!work[u]) continue;
            if (!full[u]) w[u] = load_partial_piece(a.text + fo[u] + 16ull * b[u], N - 4u * b[u]);
            const uint32_t code = decode_piece(w[u], fl[u]);
            if (WRITE) a.out[j[u] * a.out_stride + b[u]] = (uint8_t)code;
        }
        if (VALIDATE) {
            // one atomic per line of the wave that has something to say
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                bool pending = fl[u] != 0u;
                while (const uint64_t m = __ballot(pending)) {
                    const int leader = __ffsll((unsigned long long)m) - 1;
                    const uint64_t j0 = (uint64_t)__shfl((unsigned long long)j[u], leader, 64);
                    const bool mine = pending && j[u] == j0;
                    const uint32_t bits = (__ballot(mine && (fl[u] & PGENHIP_PARSE_DECLINED)) ? PGENHIP_PARSE_DECLINED : 0u) |
                                          (__ballot(mine && (fl[u] & PGENHIP_PARSE_PHASED)) ? PGENHIP_PARSE_PHASED : 0u) |
                                          (__ballot(mine && (fl[u] & PGENHIP_PARSE_HALF_CALL)) ? PGENHIP_PARSE_HALF_CALL : 0u);
                    if ((int)lane == leader) atomicOr(&a.line_flags[j0], bits);
                    if (mine) pending = false;
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_gt_parse_general(const ParseArgs &a, bool declined_only, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_lines == 0) return hipSuccess;
    const dim3 grid(general_grid(a.n_lines, num_cus, blocks)), block(kThreads);
    hipLaunchKernelGGL(gt_parse_general_kernel, grid, block, 0, stream, a, declined_only ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_gt_parse_fixed(const ParseArgs &a, bool validate, bool write, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_lines == 0) return hipSuccess;
    const FixedPlan p = fixed_plan(a.record_size, a.n_lines, num_cus, blocks);
    const dim3 grid(p.grid), block(kThreads);
    if (validate && write)
        hipLaunchKernelGGL((gt_parse_fixed_kernel<true, true>), grid, block, 0, stream, a, p.pieces, p.total);
    else if (validate)
        hipLaunchKernelGGL((gt_parse_fixed_kernel<true, false>), grid, block, 0, stream, a, p.pieces, p.total);
    else
        hipLaunchKernelGGL((gt_parse_fixed_kernel<false, true>), grid, block, 0, stream, a, p.pieces, p.total);
    return hipGetLastError();
}

}  // namespace pgenhip
