"""CPU reference of `pgen-hip assoc` (test-side only), in numpy float64, twice over:

  * ``closed_form``: the formulas the host evaluates from the per-code sums (include/pgen_hip.h, pgenhip_variant_sums): Q from a QR
    of [1, covariates], residualised phenotypes, t_v = S[v][1] + 2 S[v][2] + mu S[v][3], denom = gg - sum t_q^2, ...;
  * ``lstsq_fit``: the same regression the slow way, np.linalg.lstsq on [g, 1, covariates] per variant with the mean-imputed g.

Their disagreement on a fileset measures how far two sound FP64 evaluations of one fit lie apart, which is what the CLI test's
tolerance is derived from.  P values need scipy (``p_values``); GPU tests read them from tests/golden/assoc instead."""
from __future__ import annotations

import numpy as np


def unpack_codes(recs: np.ndarray, n: int) -> np.ndarray:
    v = recs.shape[0]
    return np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """(V, N) codes -> (V, R) uint8 records, pad bits zero."""
    v, n = codes.shape
    r = (n + 3) // 4
    padded = np.zeros((v, 4 * r), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, r, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def complete_cases(kept, pheno: np.ndarray, covar: np.ndarray) -> list:
    """The kept samples (row numbers) with every phenotype and every covariate; pheno (N, P), covar (N, m - 1), NaN = missing."""
    return [k for k in kept if not (np.isnan(pheno[k]).any() or np.isnan(covar[k]).any())]


def imputed(codes: np.ndarray):
    """(V, n) codes -> (g, mu, called, c3): the dosages with a missing call at the row's mean over the called samples (0 when nobody
    is called)."""
    c1, c2, c3 = (codes == 1).sum(axis=1), (codes == 2).sum(axis=1), (codes == 3).sum(axis=1)
    called = codes.shape[1] - c3
    mu = np.where(called > 0, (c1 + 2.0 * c2) / np.maximum(called, 1), 0.0)
    g = np.where(codes == 3, mu[:, None], codes.astype(np.float64))
    return g, mu, called, c3


def closed_form(codes: np.ndarray, y: np.ndarray, x: np.ndarray):
    """codes (V, n) of the complete samples, y (n, P), x (n, m - 1) -> dict of (V, P) arrays BETA, SE, T (NaN where the CLI prints
    NA), and (V,) MISS_CT, A1_FREQ (NaN when nobody is called), plus df."""
    v, n = codes.shape
    m = 1 + x.shape[1]
    q, _ = np.linalg.qr(np.column_stack([np.ones(n), x]))
    r = y - q @ (q.T @ y)
    r = r - q @ (q.T @ r)
    rr = (r * r).sum(axis=0)
    vals = np.column_stack([q, r])
    s = np.stack([(codes == c).astype(np.float64) @ vals for c in range(4)], axis=2)   # (V, C, 4)
    g, mu, called, c3 = imputed(codes)
    c1, c2 = (codes == 1).sum(axis=1), (codes == 2).sum(axis=1)
    t = s[:, :, 1] + 2.0 * s[:, :, 2] + mu[:, None] * s[:, :, 3]
    gg = c1 + 4.0 * c2 + mu * mu * c3
    denom = gg - (t[:, :m] ** 2).sum(axis=1)
    df = n - m - 1
    with np.errstate(all="ignore"):
        b = t[:, m:]
        beta = b / denom[:, None]
        rss = rr[None, :] - b * b / denom[:, None]
        se = np.sqrt(rss / df / denom[:, None])
        bad = (called == 0)[:, None] | ~(denom > 1e-12 * gg)[:, None] | ~(rss > 0)
        beta, se = np.where(bad, np.nan, beta), np.where(bad, np.nan, se)
        tstat = beta / se
    return {"BETA": beta, "SE": se, "T": tstat, "MISS_CT": c3, "A1_FREQ": np.where(called > 0, mu / 2.0, np.nan), "df": df}


def lstsq_fit(codes: np.ndarray, y: np.ndarray, x: np.ndarray, skip=None):
    """The same fit through np.linalg.lstsq per variant: (BETA, SE, T), each (V, P); rows in ``skip`` (boolean (V,)) are NaN."""
    v, n = codes.shape
    m = 1 + x.shape[1]
    g, _, _, _ = imputed(codes)
    df = n - m - 1
    beta = np.full((v, y.shape[1]), np.nan)
    se = np.full_like(beta, np.nan)
    base = np.column_stack([np.ones(n), x])
    for j in range(v):
        if skip is not None and skip[j]:
            continue
        d = np.column_stack([g[j], base])
        coef, _, rank, _ = np.linalg.lstsq(d, y, rcond=None)
        if rank < m + 1:
            continue
        res = y - d @ coef
        rss = (res * res).sum(axis=0)
        inv00 = np.linalg.inv(d.T @ d)[0, 0]
        beta[j] = coef[0]
        se[j] = np.sqrt(rss / df * inv00)
    return beta, se, beta / se


def p_values(t: np.ndarray, df: float) -> np.ndarray:
    from scipy import stats

    return 2.0 * stats.t.sf(np.abs(t), df)
