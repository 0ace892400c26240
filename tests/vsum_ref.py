"""CPU reference of pgenhip_variant_sums (test-side only): unpack the 2-bit codes with numpy and sum, for every row j, value column
c and code x, the values of the kept samples whose code in row j is x with math.fsum, which is correctly rounded.  Beside the sums
it returns A[c] = sum over the kept samples of |values[k, c]|, the scale of the error bound in include/pgen_hip.h."""
from __future__ import annotations

import math

import numpy as np


def unpack_codes(recs: np.ndarray, n: int) -> np.ndarray:
    """(V, R) uint8 records -> (V, n) codes 0..3 (pad bits dropped)."""
    v = recs.shape[0]
    return np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]


def vsum_from_codes(codes: np.ndarray, values: np.ndarray):
    """(V, K) codes of the selected rows and kept samples and (K, C) or (K,) float64 values -> (S, A): S (V, C, 4) float64, A (C,)."""
    vals = np.asarray(values, dtype=np.float64)
    if vals.ndim == 1:
        vals = vals[:, None]
    v, k = codes.shape
    assert vals.shape[0] == k
    c = vals.shape[1]
    a = np.abs(vals).sum(axis=0) if k else np.zeros(c)
    s = np.zeros((v, c, 4), dtype=np.float64)
    if np.array_equal(vals, np.rint(vals)):
        # integers: every partial sum of every order is an integer below 2^53 (checked), so the FP64 matrix products are exact
        assert a.size == 0 or a.max() < 2.0 ** 53
        for x in range(4):
            s[:, :, x] = (codes == x).astype(np.float64) @ vals
        return s, a
    parts = split_on_grids(vals)
    if parts is not None and k < 2 ** 28:
        # the same correctly rounded sums without a Python loop over the samples: every value is cut into four pieces of at most
        # 24 bits on fixed grids, so that the sums of a piece are exact in FP64 in any order (24 + 28 bits), and math.fsum adds
        # the four exact piece sums of every (j, c, x)
        sums = [np.stack([(codes == x).astype(np.float64) @ p for x in range(4)], axis=2) for p in parts]
        flat = [q.reshape(-1) for q in sums]
        s = np.array([math.fsum(t) for t in zip(*flat)], dtype=np.float64).reshape(v, c, 4)
        return s, a
    for j in range(v):
        for x in range(4):
            sel = vals[codes[j] == x]
            s[j, :, x] = [math.fsum(sel[:, col]) for col in range(c)]
    return s, a


GRIDS = (2.0 ** -2, 2.0 ** -26, 2.0 ** -50, 2.0 ** -74)


def split_on_grids(vals: np.ndarray):
    """vals = the sum of four arrays, each a multiple of its grid step below 2^24 steps; None where the values do not fit
    (magnitudes of 2^22 or more, or bits below 2^-74)."""
    if vals.size and np.abs(vals).max() >= 2.0 ** 22:
        return None
    rem = vals.copy()
    parts = []
    for g in GRIDS:
        p = np.trunc(rem / g) * g   # exact: a power-of-two scale and a truncation
        rem = rem - p               # exact: the low bits of rem
        parts.append(p)
    return parts if not rem.any() else None


def vsum_ref(recs: np.ndarray, n: int, values: np.ndarray, kept=None):
    """The same from (V, R) uint8 records of n samples and an optional kept list (values: one row per KEPT sample)."""
    codes = unpack_codes(recs, n)
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return vsum_from_codes(codes, values)


def bound(k: int, a: np.ndarray) -> np.ndarray:
    """|any-order FP64 sum - exact sum| <= this, per column: (K + 1) roundings of at most 2^-53 relative to the running sum, itself
    at most A_c (1.01 covers the second-order terms)."""
    return 1.01 * (k + 1) * 2.0 ** -53 * np.asarray(a, dtype=np.float64)
