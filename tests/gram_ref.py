"""CPU reference of pgenhip_sample_gram (test-side only): unpack the 2-bit codes with numpy, Z[j, k] = t[j, code of sample k in row
j], G = Z[:, a]^T Z[:, b] in float64 (exact where every partial sum is an integer below 2^53).  gram_abs is the bound's A(a, b),
gram_fsum the correctly rounded sum per entry (error-free products, math.fsum).  grm_ref is the host command's arithmetic
(counts -> tables -> G / N); grm_loop is a second, independent formulation of the same GRM, pair by pair."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

import spair_ref
from spair_ref import rsize  # noqa: F401  (the record layout is the pair tables')


# The two formulations of the GRM below (grm_ref: matrix form with scaled values; grm_loop: pair loop dividing by the variance)
# differ by at most 1.18e-15 A / N on the committed fileset tests/golden/grm (10.6 units of 2^-53; measured).  The
# allowance for the reference's own error sits just above that figure.
REF_DISAGREEMENT = 1.5e-15


def unpack(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (V, K) codes 0..3 of the kept samples (pad bits dropped); V = 0 gives (0, K)."""
    if recs.shape[0] == 0:
        return np.zeros((0, n if kept is None else len(kept)), dtype=np.uint8)
    return spair_ref.unpack(recs, n, kept)


def z_matrix(codes: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """(V, K) codes and (V, 4) float64 tables -> (V, K) float64, Z[j, k] = tables[j, codes[j, k]]."""
    tables = np.asarray(tables, dtype=np.float64).reshape(-1, 4)
    assert tables.shape[0] == codes.shape[0]
    if codes.shape[0] == 0:
        return np.zeros(codes.shape, dtype=np.float64)
    return np.take_along_axis(tables, codes.astype(np.int64), axis=1)


def gram_ref(codes_a: np.ndarray, tables: np.ndarray, codes_b: Optional[np.ndarray] = None) -> np.ndarray:
    """(A, B) float64: entry [i, l] = sum over the rows of t[x(a_i)] * t[x(b_l)]."""
    za = z_matrix(codes_a, tables)
    zb = za if codes_b is None else z_matrix(codes_b, tables)
    return za.T @ zb


def gram_abs(codes_a: np.ndarray, tables: np.ndarray, codes_b: Optional[np.ndarray] = None) -> np.ndarray:
    """A(a, b) = sum over the rows of |t[x(a)] * t[x(b)]|, the scale of the documented error bound."""
    za = np.abs(z_matrix(codes_a, tables))
    zb = za if codes_b is None else np.abs(z_matrix(codes_b, tables))
    return za.T @ zb


def _two_product_err(x: np.ndarray, y: np.ndarray, p: np.ndarray) -> np.ndarray:
    """x * y - p exactly (Dekker), for magnitudes far from overflow and underflow."""
    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    xh, xl = split(x)
    yh, yl = split(y)
    return ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def gram_fsum(codes_a: np.ndarray, tables: np.ndarray, codes_b: Optional[np.ndarray] = None) -> np.ndarray:
    """The exact sum of every entry rounded once: products split into value and rounding error, summed by math.fsum."""
    za = z_matrix(codes_a, tables)
    zb = za if codes_b is None else z_matrix(codes_b, tables)
    out = np.zeros((za.shape[1], zb.shape[1]), dtype=np.float64)
    for i in range(za.shape[1]):
        for l in range(zb.shape[1]):
            p = za[:, i] * zb[:, l]
            out[i, l] = math.fsum(np.concatenate([p, _two_product_err(za[:, i], zb[:, l], p)]).tolist())
    return out


def variant_counts(codes: np.ndarray) -> np.ndarray:
    """(V, 4) int64 counts of codes 0..3 over the kept samples (what pgenhip_genotype_counts returns)."""
    return np.stack([(codes == x).sum(axis=1) for x in range(4)], axis=1).astype(np.int64)


def grm_tables(counts: np.ndarray):
    """The host command's two tables per variant from its counts: G ((0-2p)s, (1-2p)s, (2-2p)s, 0) with p = (c1 + 2 c2) / (2 called),
    s = 1 / sqrt(2p(1-p)), and N (1, 1, 1, 0); both all zero when called == 0, p == 0 or p == 1.  Also how many variants that is."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    tg = np.zeros((counts.shape[0], 4), dtype=np.float64)
    tn = np.zeros((counts.shape[0], 4), dtype=np.float64)
    skipped = 0
    for j, (c0, c1, c2, _) in enumerate(counts.tolist()):
        called = c0 + c1 + c2
        alt = c1 + 2 * c2
        if called == 0 or alt == 0 or alt == 2 * called:
            skipped += 1
            continue
        p = float(alt) / (2.0 * float(called))
        s = 1.0 / math.sqrt(2.0 * p * (1.0 - p))
        tg[j] = [(0.0 - 2.0 * p) * s, (1.0 - 2.0 * p) * s, (2.0 - 2.0 * p) * s, 0.0]
        tn[j] = [1.0, 1.0, 1.0, 0.0]
    return tg, tn, skipped


def grm_ref(codes: np.ndarray):
    """(G, N, GRM = G / N with nan where N == 0) of the (V, K) codes, by the matrix formulation."""
    tg, tn, _ = grm_tables(variant_counts(codes))
    g, n = gram_ref(codes, tg), gram_ref(codes, tn)
    with np.errstate(divide="ignore", invalid="ignore"):
        return g, n, g / n


def grm_loop(codes: np.ndarray) -> np.ndarray:
    """The same GRM pair by pair: the mean over the variants called in both samples of (x_a - 2p)(x_b - 2p) / (2p(1-p)), summed
    with math.fsum.  It divides by the variance instead of multiplying two scaled values, so it rounds differently."""
    v, k = codes.shape
    counts = variant_counts(codes)
    called = counts[:, :3].sum(axis=1)
    alt = counts[:, 1] + 2 * counts[:, 2]
    use = (called > 0) & (alt > 0) & (alt < 2 * called)
    p = np.where(use, alt / np.maximum(2.0 * called, 1.0), 0.5)
    var = 2.0 * p * (1.0 - p)
    out = np.full((k, k), np.nan)
    for a in range(k):
        for b in range(k):
            both = use & (codes[:, a] < 3) & (codes[:, b] < 3)
            n = int(both.sum())
            if n:
                xa, xb = codes[both, a].astype(np.float64), codes[both, b].astype(np.float64)
                out[a, b] = math.fsum(((xa - 2.0 * p[both]) * (xb - 2.0 * p[both]) / var[both]).tolist()) / n
    return out
