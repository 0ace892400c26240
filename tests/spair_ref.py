"""CPU reference of pgenhip_sample_pair_stats (test-side only): unpack the 2-bit codes with numpy, form the one-hot planes E_x
(V x K, E_x[j, k] = 1 where sample k has code x in row j) and T[a, b, x, y] = (E_x^T E_y)[a, b].  The products run in float64,
where sums of 0/1 terms below 2^53 are exact, and come back as int64."""
from __future__ import annotations

from typing import Optional

import numpy as np


def rsize(n: int) -> int:
    return (2 * n + 7) // 8


def unpack(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (V, K) codes 0..3 of the kept samples (pad bits dropped)."""
    v = recs.shape[0]
    codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return codes


def pair_tables(codes_a: np.ndarray, codes_b: Optional[np.ndarray] = None) -> np.ndarray:
    """(V, A) and (V, B) codes of the same rows -> (A, B, 4, 4) int64, entry [i, l, x, y] = rows with code x in column i of
    codes_a and code y in column l of codes_b."""
    if codes_b is None:
        codes_b = codes_a
    assert codes_a.shape[0] == codes_b.shape[0] and codes_a.shape[0] < 2 ** 53
    ea = [(codes_a == x).astype(np.float64) for x in range(4)]
    eb = [(codes_b == y).astype(np.float64) for y in range(4)]
    t = np.empty((codes_a.shape[1], codes_b.shape[1], 4, 4), dtype=np.int64)
    for x in range(4):
        for y in range(4):
            t[:, :, x, y] = np.rint(ea[x].T @ eb[y]).astype(np.int64)
    return t


def ranges(codes: np.ndarray, a, b) -> np.ndarray:
    """The tables of rank ranges a = (begin, count), b = (begin, count) of the (V, K) codes."""
    return pair_tables(codes[:, a[0]:a[0] + a[1]], codes[:, b[0]:b[0] + b[1]])


def table_loop(codes: np.ndarray, a: int, b: int) -> np.ndarray:
    """One pair's table by a Python loop over the rows."""
    t = np.zeros((4, 4), dtype=np.int64)
    for j in range(codes.shape[0]):
        t[codes[j, a], codes[j, b]] += 1
    return t


def kinship(t: np.ndarray):
    """(N, HETHET, IBS0, HET1, HET2, KINSHIP) of one 4 x 4 table: the KING-robust between-family estimator over the rows called
    in both samples, in double from the integers; nan when min(HET1, HET2) == 0."""
    t = np.asarray(t, dtype=np.int64)
    n = int(t[:3, :3].sum())
    hethet = int(t[1, 1])
    ibs0 = int(t[0, 2] + t[2, 0])
    het1 = int(t[1, :3].sum())
    het2 = int(t[:3, 1].sum())
    m = min(het1, het2)
    kin = float("nan") if m == 0 else 0.5 - (float(het1 + het2 - 2 * hethet) + 4.0 * float(ibs0)) / (4.0 * float(m))
    return n, hethet, ibs0, het1, het2, kin
