"""Numpy / exact-arithmetic reference of the windowed pairwise tables and r^2 (pgenhip_pair_stats, include/pgen_hip.h).

Tables: unpack the 2-bit codes (the tests' decoder idiom), take the kept columns, bincount 4*a + b per pair.  r^2: Python integers
and fractions.Fraction, rounded ONCE to float32 (the nearest float32 of the exact rational, found by comparing fractions, not by
going through a double)."""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Sequence

import numpy as np


def rsize(n: int) -> int:
    return (2 * n + 7) // 8


def unpack(recs: np.ndarray, n: int, kept: Optional[Sequence[int]] = None) -> np.ndarray:
    """(V, R) uint8 records -> (V, K) codes of the kept samples (pad bits dropped)."""
    v = recs.shape[0]
    codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return codes.astype(np.int64)


def pair_list(v: int, n_left: int, window: int):
    """(i, d) of every pair the contract defines, in pair-index order."""
    return [(i, d) for i in range(n_left) for d in range(1, window + 1) if i + d < v]


def table(ci: np.ndarray, cj: np.ndarray) -> np.ndarray:
    """4 x 4 table of two rows' codes."""
    return np.bincount(4 * ci + cj, minlength=16).reshape(4, 4).astype(np.int64)


def pair_tables(codes: np.ndarray, n_left: int, window: int, fill: int = 0) -> np.ndarray:
    """(n_left, W, 4, 4) int64; entries of pairs that do not exist hold ``fill``."""
    v = codes.shape[0]
    out = np.full((n_left, window, 4, 4), fill, dtype=np.int64)
    for i, d in pair_list(v, n_left, window):
        out[i, d - 1] = table(codes[i], codes[i + d])
    return out


def to_f32_once(x: Fraction) -> np.float32:
    """The float32 nearest to the exact rational x >= 0 (ties to even)."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    cands = [c for c in cands if np.isfinite(c)]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))
    return np.float32(best)


def r2_exact(t: np.ndarray) -> Optional[Fraction]:
    """r^2 of the cells with a, b in {0, 1, 2} as an exact rational; None when the denominator is zero."""
    n = sx = sy = sxx = syy = sxy = 0
    for a in range(3):
        for b in range(3):
            c = int(t[a][b])
            n += c
            sx += a * c
            sy += b * c
            sxx += a * a * c
            syy += b * b * c
            sxy += a * b * c
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if vx == 0 or vy == 0:
        return None
    cov = n * sxy - sx * sy
    return Fraction(cov * cov, vx * vy)


def r2_f32(t: np.ndarray) -> np.float32:
    x = r2_exact(t)
    return np.float32(np.nan) if x is None else to_f32_once(x)


def pair_r2(tables: np.ndarray, v: int, fill=np.nan) -> np.ndarray:
    """(n_left, W) float32 from pair_tables' result; entries of pairs that do not exist hold ``fill``."""
    n_left, window = tables.shape[:2]
    out = np.full((n_left, window), fill, dtype=np.float32)
    for i, d in pair_list(v, n_left, window):
        out[i, d - 1] = r2_f32(tables[i, d - 1])
    return out


def table_brute(recs: np.ndarray, n: int, kept: Optional[Sequence[int]], i: int, j: int) -> np.ndarray:
    """The same table by a per-sample loop over the raw record bytes."""
    t = np.zeros((4, 4), dtype=np.int64)
    for s in (range(n) if kept is None else kept):
        a = (int(recs[i, s // 4]) >> (2 * (s % 4))) & 3
        b = (int(recs[j, s // 4]) >> (2 * (s % 4))) & 3
        t[a, b] += 1
    return t
