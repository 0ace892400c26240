"""CPU reference of `pgen-hip pca` (test-side only).  m_matrix is the matrix the command decomposes, M = Z^T Z / V_used with Z from grm's
table G (a missing call at the variant's mean, variants with no call or p of 0 or 1 skipped); eigh_ref its eigen-decomposition by
numpy; twin the numpy twin of the host algorithm: randomised subspace iteration on L = min(K, P + 10) columns with Rayleigh-Ritz in
every pass and the command's stop rule.  The twin draws its Gaussian start from numpy's generator, not from the command's splitmix64
stream: the iteration, not the start, is what it mirrors."""
from __future__ import annotations

import numpy as np

import gram_ref as GR


def m_matrix(codes: np.ndarray):
    """(M, variants skipped) of (V, K) codes."""
    tg, _, skipped = GR.grm_tables(GR.variant_counts(codes))
    z = GR.z_matrix(codes, tg)
    used = codes.shape[0] - skipped
    return z.T @ z / max(used, 1), skipped


def eigh_ref(m: np.ndarray):
    """(eigenvalues descending, eigenvectors in columns) by numpy.linalg.eigh."""
    lam, vec = np.linalg.eigh(m)
    return lam[::-1].copy(), vec[:, ::-1].copy()


def twin(m: np.ndarray, pcs: int, tol: float = 1e-6, max_passes: int = 100, seed: int = 1):
    """(eigenvalues (pcs,), unit eigenvectors (K, pcs), passes, relative residual, converged)."""
    k = m.shape[0]
    l = min(k, pcs + 10)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((k, l)))
    passes = 0
    while True:
        y = m @ q
        passes += 1
        t = q.T @ y
        lam, w = np.linalg.eigh(0.5 * (t + t.T))
        lam, w = lam[::-1], w[:, ::-1]
        u = q @ w
        res = np.linalg.norm(y @ w - u * lam, axis=0)[:pcs].max()
        converged = bool(res <= tol * lam[0])
        if converged or passes >= max_passes:
            break
        q, _ = np.linalg.qr(y)
    u = u[:, :pcs] / np.linalg.norm(u[:, :pcs], axis=0)
    return lam[:pcs].copy(), u, passes, float(res / lam[0]) if lam[0] > 0 else 0.0, converged


def align(u: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """u with each column's sign turned to its reference column's."""
    return u * np.where((u * ref).sum(axis=0) < 0, -1.0, 1.0)
