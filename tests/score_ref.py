"""CPU reference of pgenhip_sample_scores (test-side only): unpack the 2-bit codes with numpy, form every term in FP64, where it
is exact (an f32 weight times 1, 2 or an f32 miss value fits 53 bits), and sum each (k, c) with math.fsum, which is correctly
rounded.  Beside the sums it returns A[k, c] = sum |term|, the scale of the standard summation error bound."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np


def unpack_codes(recs: np.ndarray, n: int) -> np.ndarray:
    """(V, R) uint8 records -> (V, n) codes 0..3 (pad bits dropped)."""
    v = recs.shape[0]
    return np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]


def dosages(codes: np.ndarray, miss: Optional[np.ndarray] = None) -> np.ndarray:
    """(V, K) codes -> (V, K) float64: 0, 1, 2 for codes 0-2 and float64(miss[j]) (0 without miss) for code 3."""
    m = np.zeros(codes.shape[0], dtype=np.float64) if miss is None else np.asarray(miss, dtype=np.float32).astype(np.float64)
    return np.where(codes == 3, m[:, None], codes.astype(np.float64))


def score_from_codes(codes: np.ndarray, weights: np.ndarray, miss: Optional[np.ndarray] = None):
    """(V, K) codes of the selected rows and kept samples, (V, C) or (V,) float32 weights and (V,) float32 miss values (or None),
    all indexed by the row's position in the selection -> (S, A), both (K, C) float64."""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    if w.ndim == 1:
        w = w[:, None]
    d = dosages(codes, miss)
    k, c = d.shape[1], w.shape[1]
    if np.array_equal(w, np.rint(w)) and np.array_equal(d, np.rint(d)):
        # integers: every partial sum of every order is an integer below 2^53 (checked), so the FP64 product sums are exact
        a = np.abs(d).T @ np.abs(w)
        assert a.size == 0 or a.max() < 2.0 ** 53
        return d.T @ w, a
    s = np.empty((k, c), dtype=np.float64)
    a = np.empty((k, c), dtype=np.float64)
    for col in range(c):
        terms = d * w[:, col][:, None]            # exact products
        s[:, col] = [math.fsum(t) for t in terms.T]
        a[:, col] = np.abs(terms).sum(axis=0)
    return s, a


def score_ref(recs: np.ndarray, n: int, weights: np.ndarray, miss: Optional[np.ndarray] = None, kept=None):
    """The same from (V, R) uint8 records of n samples and an optional kept list."""
    codes = unpack_codes(recs, n)
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return score_from_codes(codes, weights, miss)


def bound(n_terms: int, a: np.ndarray) -> np.ndarray:
    """|any-order FP64 sum - exact sum| <= this: (n + 1) roundings of at most 2^-53 relative to the running sum, itself at most A
    (the + 1 is the initial value's add, 1.01 covers the second-order terms)."""
    return 1.01 * (n_terms + 1) * 2.0 ** -53 * a
