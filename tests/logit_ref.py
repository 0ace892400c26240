"""Reference for per-variant logistic regression (pgenhip_variant_logistic, `pgen-hip assoc --logistic`): numpy FP64, twice over.

  * newton: the algorithm include/pgen_hip.h fixes, restated: start at (start, 0); per evaluation mu, grad = X^T (y - mu),
    H = X^T diag(mu (1 - mu)) X, the Cholesky factor of H (a pivot <= 0 or not finite: SINGULAR), delta = H^-1 grad; CONVERGED when
    max |delta| <= tol (this beta, SE = sqrt((H^-1)[g][g]), `it` evaluations), NOT_CONVERGED when it == max_iter, else beta += delta.
  * irls_qr: the same iteration with every step taken through a QR of sqrt(w) X instead of the normal equations: delta is the
    least-squares solution of sqrt(w) X delta = (y - mu) / sqrt(w), SE = 1 / |R[g][g]|.  An independent route to the same numbers:
    the two share neither H nor a factorisation.

Both return (beta (p,), se, status), status = evaluations | CONVERGED / NOT_CONVERGED / SINGULAR as in the header."""
import numpy as np

CONVERGED, NOT_CONVERGED, SINGULAR = 0x100, 0x200, 0x400
COMPARE_CASES = [(63, 1), (64, 2), (65, 4), (67, 3), (129, 8), (257, 15), (257, 4), (1000, 15), (2504, 8)]   # (K, n_cov)
COMPARE_V = 96


def rsize(n):
    return (n + 3) // 4


def pack_codes(codes):
    """(V, N) codes 0..3 -> (V, ceil(N / 4)) record bytes, pad bits zero (sample s in byte s / 4, bits 2 (s % 4))"""
    v, n = codes.shape
    padded = np.zeros((v, 4 * rsize(n)), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def unpack_codes(recs, n):
    b = np.asarray(recs, dtype=np.uint8)
    out = np.stack([(b >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(b.shape[0], -1)
    return out[:, :n]


def code_table(codes_row, impute):
    """t[0..3] for one row: 0, 1, 2 and, for a missing call, the mean dosage over the called samples (impute) or NaN (drop)"""
    called = codes_row != 3
    mean = float(codes_row[called].sum()) / float(called.sum()) if called.any() else 0.0
    return np.array([0.0, 1.0, 2.0, mean if impute else np.nan])


def tables(codes, impute):
    return np.stack([code_table(row, impute) for row in codes])


def logistic(eta):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-eta))


def cholesky(h):
    """The lower factor by columns, or None at a pivot that is <= 0 or not finite"""
    p = h.shape[0]
    l = np.zeros_like(h)
    for j in range(p):
        piv = h[j, j] - np.dot(l[j, :j], l[j, :j])
        if not (piv > 0.0) or not np.isfinite(piv):
            return None
        l[j, j] = np.sqrt(piv)
        l[j + 1:, j] = (h[j + 1:, j] - l[j + 1:, :j] @ l[j, :j]) / l[j, j]
    return l


def solve_lower(l, b):
    z = np.zeros_like(b)
    for i in range(len(b)):
        z[i] = (b[i] - np.dot(l[i, :i], z[:i])) / l[i, i]
    return z


def solve_upper(u, b):
    z = np.zeros_like(b)
    for i in range(len(b) - 1, -1, -1):
        z[i] = (b[i] - np.dot(u[i, i + 1:], z[i + 1:])) / u[i, i]
    return z


def newton(x, y, start, max_iter, tol):
    """x: (n, p) with the genotype last; start: (p - 1,)"""
    p = x.shape[1]
    beta = np.concatenate([np.asarray(start, dtype=np.float64), [0.0]])
    if x.shape[0] == 0:
        return beta, np.nan, SINGULAR | 1
    for it in range(1, max_iter + 1):
        mu = logistic(x @ beta)
        grad = x.T @ (y - mu)
        h = (x * (mu * (1.0 - mu))[:, None]).T @ x
        l = cholesky(h)
        if l is None:
            return beta, np.nan, SINGULAR | it
        delta = solve_upper(l.T, solve_lower(l, grad))
        if np.all(np.abs(delta) <= tol):
            return beta, 1.0 / l[p - 1, p - 1], CONVERGED | it
        if it == max_iter:
            return beta, np.nan, NOT_CONVERGED | it
        beta = beta + delta
    raise AssertionError("unreachable")


def irls_qr(x, y, start, max_iter, tol):
    p = x.shape[1]
    beta = np.concatenate([np.asarray(start, dtype=np.float64), [0.0]])
    if x.shape[0] == 0:
        return beta, np.nan, SINGULAR | 1
    for it in range(1, max_iter + 1):
        mu = logistic(x @ beta)
        sw = np.sqrt(mu * (1.0 - mu))
        ok = sw > 0
        r = np.linalg.qr(x * sw[:, None], mode="r") if x.shape[0] >= p else np.zeros((p, p))
        d = np.abs(np.diag(r)) if r.shape[0] == p else np.zeros(p)
        if not np.all(np.isfinite(d)) or d.min() <= 1e-13 * max(d.max(), 1e-300):
            return beta, np.nan, SINGULAR | it
        q, r = np.linalg.qr(x * sw[:, None])
        z = np.zeros_like(y)
        z[ok] = (y - mu)[ok] / sw[ok]
        delta = solve_upper(r, q.T @ z)
        if np.all(np.abs(delta) <= tol):
            return beta, 1.0 / abs(r[p - 1, p - 1]), CONVERGED | it
        if it == max_iter:
            return beta, np.nan, NOT_CONVERGED | it
        beta = beta + delta
    raise AssertionError("unreachable")


def null_fit(design, y, max_iter=50, tol=1e-13):
    """The null model's coefficients: Newton on the design alone from zero (the host's null fit, in the design's own basis)"""
    beta = np.zeros(design.shape[1])
    for _ in range(max_iter):
        mu = logistic(design @ beta)
        h = (design * (mu * (1.0 - mu))[:, None]).T @ design
        delta = np.linalg.solve(h, design.T @ (y - mu))
        if np.all(np.abs(delta) <= tol):
            break
        beta = beta + delta
    return beta


def fit_rows(fit, codes, table, design, y, start, max_iter, tol):
    """One fit per row of codes ((V, K): the kept samples' codes): beta (V, p), se (V,), status (V,)"""
    v, p = codes.shape[0], design.shape[1] + 1
    beta, se, status = np.zeros((v, p)), np.zeros(v), np.zeros(v, dtype=np.int64)
    for j in range(v):
        g = table[j][codes[j]]
        inc = ~np.isnan(g)
        x = np.column_stack([design[inc], g[inc]])
        beta[j], se[j], status[j] = fit(x, y[inc], start, max_iter, tol)
    return beta, se, status


def make_case(seed, k, n_cov, v=COMPARE_V, missing=0.02):
    """codes (v, k) with allele frequencies uniform in [0.2, 0.5] under Hardy-Weinberg and `missing` of the calls missing; a design
    [1, standard normal covariates] (k, n_cov); a 0/1 phenotype from a logistic model of modest effects"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.2, 0.5, size=v)
    codes = rng.binomial(2, f[:, None], size=(v, k)).astype(np.uint8)
    codes[rng.random((v, k)) < missing] = 3
    design = np.column_stack([np.ones(k), rng.standard_normal((k, n_cov - 1))])
    eff = rng.standard_normal(n_cov) * 0.5 / np.sqrt(n_cov)
    eta = design @ eff + 0.3 * (codes[0] % 3) - 0.3
    y = (rng.random(k) < logistic(eta)).astype(np.float64)
    if y.min() == y.max():
        y[0] = 1.0 - y[0]
    return codes, design, y


def reference(seed, k, n_cov, impute, max_iter=25):
    """A compare-leg case and its references: newton stopped at 1e-10 and at 1e-13, irls_qr at 1e-13"""
    codes, design, y = make_case(seed, k, n_cov)
    table = tables(codes, impute)
    start = null_fit(design, y)
    loose = fit_rows(newton, codes, table, design, y, start, max_iter, 1e-10)
    tight = fit_rows(newton, codes, table, design, y, start, max_iter, 1e-13)
    qr = fit_rows(irls_qr, codes, table, design, y, start, max_iter, 1e-13)
    return {"codes": codes, "design": design, "y": y, "table": table, "start": start, "loose": loose, "tight": tight, "qr": qr}


def measure(refs):
    """Over the references of several cases: the gap between the 1e-10-stopped and the converged answers, and the disagreement of the
    two formulations, each for beta (absolute, all coefficients) and SE (relative), on the rows where all three converged"""
    out = {"beta_gap": 0.0, "se_gap": 0.0, "beta_form": 0.0, "se_form": 0.0, "rows": 0, "max_it": 0}
    for r in refs:
        ok = ((r["loose"][2] & CONVERGED) != 0) & ((r["tight"][2] & CONVERGED) != 0) & ((r["qr"][2] & CONVERGED) != 0)
        if not ok.any():
            continue
        out["rows"] += int(ok.sum())
        out["max_it"] = max(out["max_it"], int((r["loose"][2][ok] & 0xFF).max()))
        out["beta_gap"] = max(out["beta_gap"], np.abs(r["loose"][0][ok] - r["tight"][0][ok]).max())
        out["se_gap"] = max(out["se_gap"], (np.abs(r["loose"][1][ok] - r["tight"][1][ok]) / r["tight"][1][ok]).max())
        out["beta_form"] = max(out["beta_form"], np.abs(r["tight"][0][ok] - r["qr"][0][ok]).max())
        out["se_form"] = max(out["se_form"], (np.abs(r["tight"][1][ok] - r["qr"][1][ok]) / r["tight"][1][ok]).max())
    return out


def tolerances(m):
    """Twice the reference's own stopping gap plus 100 x the formulations' disagreement: (beta absolute, SE relative)"""
    return 2.0 * m["beta_gap"] + 100.0 * m["beta_form"], 2.0 * m["se_gap"] + 100.0 * m["se_form"]
