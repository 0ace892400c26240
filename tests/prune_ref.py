"""References of LD pruning (pgenhip_pair_mask, pgenhip_prune_resolve; include/pgen_hip.h), on top of tests/pair_ref.py.

``edges`` is the pair mask as booleans, from the exact r^2 of every pair's table rounded once to float32 and compared in float32,
as the header defines it.  The device's r^2 is "within one ulp" of that value (tests/pair_ref.py, r2_close), so its comparison can
differ from the reference's only where the exact r^2 lies next to the threshold: ``edges`` RAISES when any existing pair's r^2 is
within 2 float32 ulps of ``min_r2`` without being exactly equal to it, and every test goes through it.  ``resolve`` is the
sequential definition of the greedy independent set S."""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Sequence

import numpy as np

import pair_ref as PR

UNDECIDED, KEPT, REMOVED = 0, 1, 2
M64 = (1 << 64) - 1


class ThresholdTooClose(ValueError):
    pass


def r2_grid(codes: np.ndarray, n_left: int, window: int):
    """(float32 (V, W) with NaN where no pair exists or r^2 is undefined, object (V, W) of the exact Fractions or None) of the
    pairs (i, i + d), i < n_left.  The slow part of ``edges``: tests compute it once for their largest V and W and slice it."""
    v = codes.shape[0]
    f = np.full((v, window), np.nan, dtype=np.float32)
    x = np.full((v, window), None, dtype=object)
    for i, d in PR.pair_list(v, n_left, window):
        q = PR.r2_exact(PR.table(codes[i], codes[i + d]))
        x[i, d - 1] = q
        if q is not None:
            f[i, d - 1] = PR.to_f32_once(q)
    return f, x


def edges(codes: np.ndarray, n_left: int, window: int, min_r2, key: Optional[Sequence[int]] = None, max_span: int = 0,
          grid=None) -> np.ndarray:
    """Boolean (V, W): entry [i, d - 1] is set iff the pair (i, i + d) exists and is an edge.  ``grid``: ``r2_grid`` of at least
    these rows and this window, of the same codes (any V' >= V rows: a pair's r^2 depends on its two rows alone)."""
    v = codes.shape[0]
    m = np.float32(min_r2)
    assert not np.isnan(m)
    f, x = grid if grid is not None else r2_grid(codes, n_left, window)
    out = np.zeros((v, window), dtype=bool)
    band = 2.0 * float(np.spacing(np.abs(m)))
    for i, d in PR.pair_list(v, n_left, window):
        q = x[i, d - 1]
        if q is None:
            continue
        if q != Fraction(float(m)) and abs(float(f[i, d - 1]) - float(m)) <= band:
            raise ThresholdTooClose(f"pair ({i}, {i + d}): r^2 {float(q)!r} lies within 2 float32 ulps of min_r2 {float(m)!r}")
        if not f[i, d - 1] > m:
            continue
        if key is not None and ((int(key[i + d]) - int(key[i])) & M64) > max_span:
            continue
        out[i, d - 1] = True
    return out


def mask_words(window: int) -> int:
    return (window + 31) // 32


def masks(e: np.ndarray, mask_stride: Optional[int] = None, fill: int = 0):
    """(fwd, bwd) uint32 (V, mask_stride) of boolean edges (V, W), ORed into words that hold ``fill``."""
    v, w = e.shape
    stride = mask_words(w) if mask_stride is None else mask_stride
    fwd = np.full((v, stride), fill, dtype=np.uint32)
    bwd = np.full((v, stride), fill, dtype=np.uint32)
    for i, b in np.argwhere(e):
        bit = np.uint32(1 << (int(b) & 31))
        fwd[i, b // 32] |= bit
        bwd[i + b + 1, b // 32] |= bit
    return fwd, bwd


def neighbours(fwd: np.ndarray, bwd: np.ndarray, window: int, v: int) -> list[int]:
    """Rows v + d (fwd bit d - 1) and v - d (bwd bit d - 1), 1 <= d <= window, inside [0, n_rows)."""
    n = fwd.shape[0]
    out = []
    for sign, m in ((1, fwd), (-1, bwd)):
        for wd in range(mask_words(window)):
            bits = int(m[v, wd])
            while bits:
                low = bits & -bits
                d = 32 * wd + low.bit_length()
                bits ^= low
                u = v + sign * d
                if d <= window and 0 <= u < n:
                    out.append(u)
    return out


def beating_order(n: int, priority: Optional[Sequence[int]]) -> list[int]:
    if priority is None:
        return list(range(n))
    return sorted(range(n), key=lambda r: (-int(priority[r]), r))


def resolve(fwd: np.ndarray, bwd: np.ndarray, window: int, priority: Optional[Sequence[int]] = None,
            state0: Optional[Sequence[int]] = None) -> np.ndarray:
    """S as uint8 (n_rows,): the rows in beating order; a pre-set row has its state; any other is KEPT iff none of its neighbours
    that beat it is KEPT."""
    n = fwd.shape[0]
    order = beating_order(n, priority)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    state = np.zeros(n, dtype=np.uint8)
    for v in order:
        if state0 is not None and int(state0[v]) in (KEPT, REMOVED):
            state[v] = state0[v]
            continue
        beaten = any(rank[u] < rank[v] and state[u] == KEPT for u in neighbours(fwd, bwd, window, v))
        state[v] = REMOVED if beaten else KEPT
    return state


def resolve_from_edge_list(n: int, edge_list: Sequence[tuple[int, int]], priority: Optional[Sequence[int]] = None,
                           state0: Optional[Sequence[int]] = None) -> np.ndarray:
    """The same S from an explicit list of undirected edges: the brute force ``resolve`` is held against."""
    adj = [set() for _ in range(n)]
    for a, b in edge_list:
        adj[a].add(b)
        adj[b].add(a)
    state = [UNDECIDED] * n
    for v in beating_order(n, priority):
        if state0 is not None and int(state0[v]) in (KEPT, REMOVED):
            state[v] = int(state0[v])
        else:
            # every neighbour that beats v came earlier in the order; the ones behind it are still undecided here
            state[v] = REMOVED if any(state[u] == KEPT for u in adj[v]) else KEPT
    return np.array(state, dtype=np.uint8)


def priority_of_counts(counts: np.ndarray) -> np.ndarray:
    """The `prune` command's priority: the minor-allele frequency among called alleles, mapped monotonically to u32."""
    out = np.zeros(len(counts), dtype=np.uint32)
    for r, (c0, c1, c2) in enumerate(np.asarray(counts)[:, :3].tolist()):
        called = c0 + c1 + c2
        if called:
            alt = c1 + 2 * c2
            maf = min(alt, 2 * called - alt) / (2 * called)
            out[r] = int(maf * 4294967294.0)
    return out


def ld_codes(rng: np.random.Generator, v: int, n: int, redraw: float = 0.15, fresh_every: int = 0, missing: float = 0.02) -> np.ndarray:
    """(V, n) codes with LD: every row is the row before it with a fraction ``redraw`` of the samples drawn anew (HWE at the row's
    own allele frequency, a few missing); every ``fresh_every``-th row (0: never) starts afresh, so that LD blocks end."""
    out = np.empty((v, n), dtype=np.int64)

    def draw(size):
        p = rng.uniform(0.1, 0.5)
        c = rng.binomial(2, p, size=size)
        c[rng.random(size) < missing] = 3
        return c

    for r in range(v):
        if r == 0 or (fresh_every and r % fresh_every == 0):
            out[r] = draw(n)
        else:
            out[r] = out[r - 1]
            pick = rng.random(n) < redraw
            out[r, pick] = draw(int(pick.sum()))
    return out


# ---- the `prune` command (pgen_rs_amd/host/prune_plan.cpp, prune.cpp) ---------------------------------------------------------------
def parse_pos(text: str):
    """A POS field: decimal digits only, below 2^32; None otherwise."""
    if not text or len(text) > 10 or any(c not in "0123456789" for c in text):
        return None
    v = int(text)
    return v if v <= 0xFFFFFFFF else None


def keys(chrom: Sequence[str], pos: Optional[Sequence[int]] = None) -> list[int]:
    """(CHROM rank by first appearance << 32) | POS; without ``pos`` POS is left out."""
    rank: dict[str, int] = {}
    return [(rank.setdefault(c, len(rank)) << 32) | (int(pos[r]) if pos is not None else 0) for r, c in enumerate(chrom)]


def window_for_span(key: Sequence[int], max_span: int, cap: int = 0) -> int:
    """The W a window in base pairs needs: the largest d with key[i + d] - key[i] <= max_span on one chromosome, scanning behind
    every row until another chromosome, the first row past the span in ascending order, or ``cap`` rows (0: no cap).  At least 1."""
    w, n = 1, len(key)
    for i in range(n):
        j = i + 1
        while j < n and (cap == 0 or j - i <= cap):
            if key[j] >> 32 != key[i] >> 32:
                break
            if (key[j] - key[i]) & M64 <= max_span:
                w = max(w, j - i)
            elif key[j] > key[i]:
                break
            j += 1
    return w


def mask_bytes(n_rows: int, window: int) -> int:
    return 2 * n_rows * mask_words(window) * 4


def counts_of_codes(codes: np.ndarray) -> np.ndarray:
    return np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1)


def prune(codes: np.ndarray, chrom: Sequence[str], pos: Sequence[int], ids: Sequence[str], min_r2, window: Optional[int] = None,
          window_kb: Optional[int] = None, grid=None):
    """The command's result on the kept rows' codes (V, K): (IDs that stay, IDs removed, edges, W).  ``grid``: ``r2_grid`` of these
    codes at a window of at least W."""
    v = codes.shape[0]
    if v < 2 or codes.shape[1] == 0:
        return list(ids), [], 0, 0
    key = keys(chrom, pos if window_kb is not None else None)
    span = 0 if window_kb is None else window_kb * 1000
    w = window if window_kb is None else window_for_span(key, span, window or 0)
    w = min(w, v - 1)
    if grid is not None:
        grid = (grid[0][:, :w], grid[1][:, :w])
    e = edges(codes, v, w, min_r2, key=key, max_span=span, grid=grid)
    fwd, bwd = masks(e)
    state = resolve(fwd, bwd, w, priority_of_counts(counts_of_codes(codes)))
    return [i for i, s in zip(ids, state) if s == KEPT], [i for i, s in zip(ids, state) if s == REMOVED], int(e.sum()), w
