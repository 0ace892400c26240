"""CPU reference of pgenhip_gram_apply (test-side only), built on gram_ref.unpack / z_matrix: Z[j, k] = t[j, code of kept sample k in
row j], P = Z q, Y = Z^T P.  apply_ref is the float64 form, apply_int the int64 form of the exact legs (integer tables and q),
apply_bounds the two documented error bounds, apply_exact the correctly rounded results of the rounding leg: P by math.fsum over
error-free products, Y in exact integer arithmetic rounded once (a term of Y is a product of three doubles, which has no two-term
error-free form to hand to fsum)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import gram_ref
from gram_ref import rsize, unpack, z_matrix  # noqa: F401  (the record layout and Z are the Gram matrix's)


def _q2(q, k: int) -> np.ndarray:
    """q as a (K, C) float64 matrix (K == 0 included)."""
    q = np.asarray(q, dtype=np.float64)
    assert q.ndim == 2 and q.shape[0] == k
    return q


def apply_ref(codes: np.ndarray, tables: np.ndarray, q: np.ndarray):
    """(P, Y) in float64: P (V, C) = Z q, Y (K, C) = Z^T P."""
    z = z_matrix(codes, tables)
    q = _q2(q, codes.shape[1])
    p = z @ q
    return p, z.T @ p


def apply_int(codes: np.ndarray, tables: np.ndarray, q: np.ndarray):
    """(P, Y) in int64 for integer tables and integer q: what every shape must equal bit for bit."""
    tables = np.asarray(tables).reshape(-1, 4)
    q = _q2(q, codes.shape[1])
    assert np.array_equal(tables, np.rint(tables)) and np.array_equal(q, np.rint(q))
    z = z_matrix(codes, tables).astype(np.int64)
    p = z @ q.astype(np.int64)
    y = z.T @ p
    assert np.abs(y).max(initial=0) < 2 ** 52
    return p, y


def apply_loop(codes: np.ndarray, tables: np.ndarray, q: np.ndarray):
    """The same, sample by sample and row by row: a second formulation that shares no matrix product with apply_ref."""
    v, k = codes.shape
    tables = np.asarray(tables, dtype=np.float64).reshape(-1, 4)
    q = _q2(q, k)
    p = np.zeros((v, q.shape[1]))
    y = np.zeros((k, q.shape[1]))
    for j in range(v):
        for s in range(k):
            p[j] += tables[j, codes[j, s]] * q[s]
    for s in range(k):
        for j in range(v):
            y[s] += tables[j, codes[j, s]] * p[j]
    return p, y


def apply_bounds(codes: np.ndarray, tables: np.ndarray, q: np.ndarray):
    """The header's bounds: |P - exact| <= (K + 1) 2^-53 sum_k |Z q| and |Y - exact| <= (V + K + 4) 2^-53 B, B = |Z|^T (|Z| |q|)."""
    v, k = codes.shape
    za = np.abs(z_matrix(codes, tables))
    a = za @ np.abs(_q2(q, k))
    return (k + 1) * 2.0 ** -53 * a, (v + k + 4) * 2.0 ** -53 * (za.T @ a)


def _as_ints(x: np.ndarray, shift: int) -> np.ndarray:
    """x * 2^shift as exact Python integers (object array); shift is large enough for every entry."""
    out = np.empty(x.shape, dtype=object)
    for idx, val in np.ndenumerate(x):
        f = Fraction(float(val)) * (1 << shift)
        assert f.denominator == 1
        out[idx] = int(f)
    return out


def apply_exact(codes: np.ndarray, tables: np.ndarray, q: np.ndarray, shift: int = 200):
    """(P, Y) correctly rounded: P[j, c] by math.fsum over the products and their rounding errors, Y in exact integers."""
    v, k = codes.shape
    z = z_matrix(codes, tables)
    q = _q2(q, k)
    p = np.zeros((v, q.shape[1]))
    for j in range(v):
        for c in range(q.shape[1]):
            pr = z[j] * q[:, c]
            p[j, c] = math.fsum(np.concatenate([pr, gram_ref._two_product_err(z[j], q[:, c], pr)]).tolist())
    zi, qi = _as_ints(z, shift), _as_ints(q, shift)
    yi = zi.T.dot(zi.dot(qi))
    y = np.zeros((k, q.shape[1]))
    for idx, val in np.ndenumerate(yi):
        y[idx] = float(Fraction(int(val), 1 << (3 * shift)))
    return p, y
