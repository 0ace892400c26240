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


# ---- how the GPU files compare an output with the reference: one rule, kept in one place ---------------------------------------------
SENT_U = 0xA5A5A5A5   # the word every output entry holds before a call (the GPU tests' sentinel frames)


def r2_close(got, want) -> bool:
    """Is ``got`` within one float32 ulp of ``want`` (the exact rational rounded once), or NaN where ``want`` is NaN?"""
    return bool(np.isnan(got)) if np.isnan(want) else abs(float(got) - float(want)) <= float(np.spacing(np.float32(want)))


def check_tables(got: np.ndarray, want_tables: np.ndarray, v: int, what: str):
    """got: (n_left, W, 16) uint32 words; want_tables: pair_tables(..., fill=-1) of at least n_left rows.  Every existing entry must
    equal the reference; entries with i + d >= V must keep the sentinel."""
    n_left, w = got.shape[:2]
    want = want_tables[:n_left].reshape(n_left, w, 16)
    exists = (np.arange(n_left)[:, None] + np.arange(1, w + 1)[None, :]) < v
    assert (got[~exists] == SENT_U).all(), f"{what}: an entry with i + d >= V was written"
    bad = np.argwhere((got.astype(np.int64) != want).any(axis=2) & exists)
    if bad.size:
        i, d = bad[0]
        raise AssertionError(f"{what}: {len(bad)} tables differ; first pair ({i}, {i + d + 1}), pair index {i * w + d}: got {got[i, d].tolist()}, "
                             f"want {want[i, d].tolist()}")


def check_r2(got_bits: np.ndarray, want_tables: np.ndarray, v: int, what: str):
    """got_bits: (n_left, W) uint32 bit patterns of the r^2 output: ``r2_close`` to pair_r2 of the reference tables wherever the pair
    exists, the sentinel elsewhere."""
    n_left, w = got_bits.shape
    got = got_bits.view(np.float32)
    exists = (np.arange(n_left)[:, None] + np.arange(1, w + 1)[None, :]) < v
    assert (got_bits[~exists] == SENT_U).all(), f"{what}: an r^2 entry with i + d >= V was written"
    want = pair_r2(want_tables[:n_left], v)
    for i, d in np.argwhere(exists):
        assert r2_close(got[i, d], want[i, d]), f"{what}: pair ({i}, {i + d + 1}) r^2 {got[i, d]!r}, want {want[i, d]!r}"
