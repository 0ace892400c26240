// gt_prune.hip — the priority-greedy independent set of a windowed pair mask for gfx950 (MI355X): the graph pgenhip_pair_mask left in
// two bit masks (row v's neighbours v + d in fwd, v - d in bwd, bit d - 1) is resolved where it lies.
//
// Row u beats v iff priority[u] > priority[v], or the two are equal (or there are no priorities) and u < v.  The answer S takes the
// rows in beating order: a row is KEPT iff none of its neighbours that beat it is KEPT.  A row can therefore be decided as soon as
// every neighbour that beats it is decided (or one of them is KEPT), whatever the order in which that is found out: a sweep decides
// all such rows, and sweeps are repeated until nothing is undecided.  States only go from 0 to their final value, so a sweep that
// reads a state another workgroup wrote during the same launch reads either 0 (the L2 of another XCD, or this CU's L1, still holds
// the old line: DESIGN.md §21) or the final value; a stale 0 costs a later sweep, never a wrong state.  No fences, no spinning.
//
// GENERAL: a lane per row, grid-stride, one sweep per launch, every state read from memory.
// BLOCK: a workgroup owns rows [b * range, (b + 1) * range) and walks them in turns of kChunkRows.  A turn stages the states of its
// rows and of halo_rows(window) rows on either side in LDS, sweeps its own rows until a sweep decides nothing, and writes back what it
// decided; a neighbour farther away than the halo (windows above kHaloRows) is read from memory.  A chain inside one turn then
// costs one launch instead of one launch per link.
// Both count the rows they leave undecided: each workgroup knows its own rows' states exactly (it is their only writer), sums them
// and adds the sum to the launch's counter with one device-scope atomic.
// Bits d - 1 >= window and neighbours outside [0, n_rows) are skipped before anything is addressed.
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::prune;   // kThreads, kChunkRows, kHaloRows, kLdsRows and the launch plans

constexpr uint8_t kUndecided = 0u, kKept = 1u, kRemoved = 2u;

__device__ __forceinline__ bool beats(const uint32_t *priority, uint64_t u, uint32_t pv, uint64_t v)
{
    if (priority == nullptr) return u < v;
    const uint32_t pu = priority[u];
    return pu > pv || (pu == pv && u < v);
}

// The state row v can be given now: KEPT, REMOVED, or UNDECIDED while a neighbour that beats it is undecided and none is KEPT.
// state_of(u): the state of row u as this sweep sees it.
template <class StateOf>
__device__ __forceinline__ uint8_t decide(const PruneArgs &a, uint64_t v, StateOf state_of)
{
    const uint32_t words = (uint32_t)mask_words(a.window);
    const uint32_t pv = a.priority ? a.priority[v] : 0u;
    bool blocked = false;
    for (uint32_t dir = 0; dir < 2u; dir++) {
        const uint32_t *row = (dir ? a.bwd : a.fwd) + v * a.mask_stride;
        for (uint32_t w = 0; w < words; w++) {
            uint32_t bits = row[w];
            const uint32_t live = a.window - 32u * w;   // bits of this word below the window
            if (live < 32u) bits &= (1u << live) - 1u;
            while (bits) {
                const uint64_t d = 32ull * w + (uint32_t)__builtin_ctz(bits) + 1u;
                bits &= bits - 1u;
                uint64_t u;
                if (dir) {
                    if (d > v) continue;
                    u = v - d;
                } else {
                    u = v + d;
                    if (u >= a.n_rows) continue;
                }
                if (!beats(a.priority, u, pv, v)) continue;
                const uint8_t s = state_of(u);
                if (s == kKept) return kRemoved;
                if (s == kUndecided) blocked = true;
            }
        }
    }
    return blocked ? kUndecided : kKept;
}

// the block's rows left undecided -> one atomic
__device__ __forceinline__ void add_undecided(const PruneArgs &a, uint32_t mine)
{
    __shared__ uint32_t total;
    if (threadIdx.x == 0u) total = 0u;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0u && total) atomicAdd(a.undecided, (unsigned long long)total);
}

__global__ __launch_bounds__(kThreads) void gt_prune_general_kernel(PruneArgs a)
{
    uint32_t mine = 0u;
    for (uint64_t v = (uint64_t)blockIdx.x * kThreads + threadIdx.x; v < a.n_rows; v += (uint64_t)gridDim.x * kThreads) {
        if (a.state[v] != kUndecided) continue;
        const uint8_t s = decide(a, v, [&](uint64_t u) { return a.state[u]; });
        if (s != kUndecided)
            a.state[v] = s;
        else
            mine++;
    }
    add_undecided(a, mine);
}

__global__ __launch_bounds__(kThreads) void gt_prune_block_kernel(PruneArgs a, uint64_t range_rows)
{
    __shared__ uint8_t st[kLdsRows];
    const uint64_t begin = (uint64_t)blockIdx.x * range_rows, end = min(begin + range_rows, a.n_rows);
    const uint32_t halo = halo_rows(a.window);
    uint32_t mine = 0u;
    for (uint64_t cb = begin; cb < end; cb += kChunkRows) {   // (block-uniform)
        const uint64_t ce = min(cb + kChunkRows, end);
        const uint64_t lo = cb > halo ? cb - halo : 0u, hi = min(ce + halo, a.n_rows);   // hi - lo <= kLdsRows
        for (uint64_t r = lo + threadIdx.x; r < hi; r += kThreads) st[r - lo] = a.state[r];
        __syncthreads();
        int changed;
        do {
            changed = 0;
            for (uint64_t v = cb + threadIdx.x; v < ce; v += kThreads) {
                if (st[v - lo] != kUndecided) continue;
                const uint8_t s = decide(a, v, [&](uint64_t u) { return u >= lo && u < hi ? st[u - lo] : a.state[u]; });
                if (s != kUndecided) {
                    st[v - lo] = s;    // seen by this sweep's later reads or by the next sweep: either is a valid order
                    a.state[v] = s;    // this block is the row's only writer
                    changed = 1;
                }
            }
            changed = __syncthreads_or(changed);
        } while (changed);
        for (uint64_t v = cb + threadIdx.x; v < ce; v += kThreads) mine += st[v - lo] == kUndecided ? 1u : 0u;
        __syncthreads();   // st is rewritten by the next turn
    }
    add_undecided(a, mine);
}

}  // namespace

hipError_t launch_gt_prune_general(const PruneArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_rows == 0u) return hipSuccess;
    hipLaunchKernelGGL(gt_prune_general_kernel, dim3(general_grid(a.n_rows, num_cus, blocks)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gt_prune_block(const PruneArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_rows == 0u) return hipSuccess;
    const BlockPlan p = block_plan(a.n_rows, num_cus, blocks);
    hipLaunchKernelGGL(gt_prune_block_kernel, dim3(p.grid), dim3(kThreads), 0, stream, a, p.range_rows);
    return hipGetLastError();
}

}  // namespace pgenhip
