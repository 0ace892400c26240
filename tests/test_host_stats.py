"""The host commands' arithmetic (pgen_rs_amd/host/stats.cpp and the pca steps of linalg.cpp) without a device: tests/stats_check.cpp, a
stand-alone program built from those two sources alone under ASan + UBSan, runs the cases written here and prints every result as a
hexadecimal float; each test compares the lines with an independent numpy computation.

Tolerances, each measured in its test and printed:
  * tables, mean dosage, KING: a handful of IEEE operations in a fixed order, so equality to the last bit.
  * Student t: against 1 - (2/pi) atan|t| (df = 1) and 1 - |t| / sqrt(2 + t^2) (df = 2) on 61 values of |t| from 1e-3 to 1e3.  Allowed: ten
    times the worst relative difference numpy float64 shows between that spelling and its algebraic twin ((2/pi) atan(1/|t|);
    2 / ((2 + t^2) + |t| sqrt(2 + t^2))), at least 2^-50.  Measured: the spellings differ by 1.5e-13 (df = 1) and 3.8e-11 (df = 2), at large
    |t| where the first spelling cancels, so 1.5e-12 and 3.8e-10 are allowed; the program is 1.5e-13 and 3.8e-11 from the first
    spelling and 1.1e-15 and 1.8e-15 from the twin.
  * assoc: NA rows, the counts' consequences (has_freq) and df exact; A1_FREQ 1e-11 relative; BETA, SE, T and the residual sums of
    squares 100 x the largest relative disagreement of assoc_ref.closed_form and assoc_ref.lstsq_fit on these same cases.  Measured:
    they disagree by 6.4e-13, so 6.4e-11 is allowed; the program is 9.4e-15 from closed_form at most.
  * pca: a Ritz value whose residual is at most tol lambda_1 lies within tol lambda_1 of an eigenvalue; its vector within
    2 sqrt(2) tol lambda_1 / gap of the eigenvector (Davis-Kahan, the factor 2 for the gap being measured between eigenvalues, not from
    the Ritz value; the test requires gap > 2 tol lambda_1)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import assoc_ref as AS

REPO = Path(__file__).resolve().parent.parent
HOST = REPO / "pgen_rs_amd" / "host"


@pytest.fixture(scope="module")
def stats_check(tmp_path_factory):
    """The program, and the proof of purity: it links from stats.cpp and linalg.cpp alone."""
    exe = tmp_path_factory.mktemp("stats") / "stats_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe),
           str(REPO / "tests" / "stats_check.cpp"), str(HOST / "stats.cpp"), str(HOST / "linalg.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr

    def run(text, tmp_path):
        (tmp_path / "cases.txt").write_text(text)
        p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", p.stderr
        return [ln.split() for ln in p.stdout.splitlines()]

    return run


def hexes(words):
    return np.array([float.fromhex(w) for w in words])


def floats(a):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def test_headers_include_no_project_header_but_each_other():
    for name in ("stats.h", "linalg.h", "stats.cpp", "linalg.cpp"):
        quoted = [ln.split('"')[1] for ln in (HOST / name).read_text().splitlines() if ln.startswith('#include "')]
        assert set(quoted) <= {"stats.h", "linalg.h"}, (name, quoted)


# ---- the standardised table and the mean dosage ----

TABLES = {
    "nothing called": (0, 0, 0, 9),
    "empty": (0, 0, 0, 0),
    "all hom-ref": (17, 0, 0, 3),
    "all hom-alt": (0, 0, 21, 0),
    "all missing but one het": (0, 1, 0, 40),
    "all missing but one hom-ref": (1, 0, 0, 40),
    "all missing but one hom-alt": (0, 0, 1, 40),
    "ordinary": (31, 22, 7, 4),
    "ordinary, p > 1/2": (3, 10, 50, 1),
    "hets only": (0, 13, 0, 0),
    "near 2^31": (2 ** 31 - 5, 2 ** 31 - 1, 2 ** 31 - 3, 7),
    "near 2^32": (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1),
    "one alt allele in 2^32": (2 ** 32 - 2, 1, 0, 0),
}


def test_tables_and_mean_dosage_bit_for_bit(stats_check, tmp_path):
    lines = stats_check("".join("table %d %d %d %d\n" % c for c in TABLES.values()), tmp_path)
    assert len(lines) == len(TABLES)
    for (name, (c0, c1, c2, _)), ln in zip(TABLES.items(), lines):
        called, alt = c0 + c1 + c2, c1 + 2 * c2
        used = not (called == 0 or alt == 0 or alt == 2 * called)
        g, n = np.zeros(4), np.zeros(4)
        if used:
            p = np.float64(alt) / (np.float64(2.0) * np.float64(called))
            s = np.float64(1.0) / np.sqrt(np.float64(2.0) * p * (np.float64(1.0) - p))
            g[:3] = [(np.float64(x) - np.float64(2.0) * p) * s for x in (0.0, 1.0, 2.0)]
            n[:3] = 1.0
        mean = np.float64(alt) / np.float64(called) if called else np.float64(0.0)
        got = hexes(ln[2:])
        assert ln[:2] == ["table", str(int(used))], name
        assert got[:4].tobytes() == g.tobytes() and got[4:8].tobytes() == n.tobytes() and got[8] == mean, (name, got, g, mean)


# ---- KING ----

def king_pairs():
    rng = np.random.default_rng(41)
    pairs = [(rng.choice(4, size=200, p=[0.4, 0.3, 0.2, 0.1]), rng.choice(4, size=200, p=[0.3, 0.4, 0.2, 0.1])) for _ in range(4)]
    a = rng.choice(4, size=211, p=[0.5, 0.3, 0.1, 0.1])
    pairs.append((a, a.copy()))                                                                       # a sample with itself
    pairs.append((rng.choice([0, 2, 3], size=190), rng.choice(4, size=190)))                          # no heterozygote in the first
    pairs.append((rng.choice([0, 2, 3], size=190), rng.choice([0, 2, 3], size=190)))                  # none in either
    pairs.append((np.full(50, 3), rng.choice(4, size=50)))                                            # nothing called in the first
    return pairs


def test_king_from_the_code_vectors(stats_check, tmp_path):
    pairs = king_pairs()
    text = ""
    for a, b in pairs:
        table = np.zeros((4, 4), dtype=np.int64)
        np.add.at(table, (a, b), 1)
        text += "king " + " ".join(map(str, table.ravel())) + "\n"
    lines = stats_check(text, tmp_path)
    assert len(lines) == len(pairs)
    nans = 0
    for (a, b), ln in zip(pairs, lines):
        both = (a != 3) & (b != 3)
        n, hethet = int(both.sum()), int(((a == 1) & (b == 1)).sum())
        ibs0 = int((((a == 0) & (b == 2)) | ((a == 2) & (b == 0))).sum())
        het1, het2 = int(((a == 1) & both).sum()), int(((b == 1) & both).sum())
        assert ln[0] == "king" and [int(w) for w in ln[1:6]] == [n, hethet, ibs0, het1, het2]
        kin = float.fromhex(ln[6])
        if min(het1, het2) == 0:
            nans += 1
            assert math.isnan(kin)
        else:
            assert kin == 0.5 - (float(het1 + het2 - 2 * hethet) + 4.0 * float(ibs0)) / (4.0 * float(min(het1, het2)))
    assert nans == 3
    assert float.fromhex(lines[4][6]) == 0.5   # a sample with itself


# ---- Student t ----

def test_student_t_against_the_closed_forms(stats_check, tmp_path):
    ts = np.logspace(-3, 3, 61)
    signed = np.where(np.arange(ts.size) % 2 == 0, ts, -ts)   # P is even in t
    lines = stats_check("".join(f"tp {float(t).hex()} {df}\n" for df in (1, 2) for t in signed), tmp_path)
    got = hexes([ln[1] for ln in lines]).reshape(2, ts.size)
    root = np.sqrt(2.0 + ts * ts)
    spellings = {1: (1.0 - (2.0 / np.pi) * np.arctan(ts), (2.0 / np.pi) * np.arctan(1.0 / ts)),
                 2: (1.0 - ts / root, 2.0 / ((2.0 + ts * ts) + ts * root))}
    for row, df in enumerate((1, 2)):
        first, twin = spellings[df]
        own = (np.abs(first - twin) / twin).max()
        allowed = max(10.0 * own, 2.0 ** -50)
        err_first, err_twin = (np.abs(got[row] - first) / first).max(), (np.abs(got[row] - twin) / twin).max()
        print(f"df = {df}: the spellings differ by {own:.3g}; allowed {allowed:.3g}; worst relative error {err_first:.3g} (against the twin: {err_twin:.3g})")
        assert err_first <= allowed
    edge = stats_check("tp 0 5\ntp inf 5\ntp -inf 3\ntp nan 5\ntp 1 0\ntp 1 -2\n", tmp_path)
    assert [ln[1] for ln in edge[:3]] == ["0x1p+0", "0x0p+0", "0x0p+0"] and all("nan" in ln[1] for ln in edge[3:])


# ---- assoc ----

def assoc_case(seed, n, ncov, pn, v=30):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ncov))
    codes = rng.choice(4, size=(v, n), p=[0.45, 0.3, 0.15, 0.1]).astype(np.uint8)
    codes[3] = rng.choice([0, 3], size=n, p=[0.8, 0.2])   # monomorphic, with missing calls
    codes[4] = 2                                           # monomorphic, hom-alt
    codes[5] = 3                                           # missing everywhere
    codes[6] = rng.choice([1, 3], size=n, p=[0.7, 0.3])   # hets only: the imputed dosage is constant
    y = rng.standard_normal((n, pn)) + 0.4 * AS.imputed(codes)[0][7:7 + pn].T + (x.sum(axis=1, keepdims=True) if ncov else 0.0)
    return codes, y, x


def per_code_sums(codes, y, x):
    """(V, C, 4): the sum of value column c over the samples with code g, from the definition; the columns as closed_form builds them"""
    n = codes.shape[1]
    q, _ = np.linalg.qr(np.column_stack([np.ones(n), x]))
    r = y - q @ (q.T @ y)
    r = r - q @ (q.T @ r)
    vals = np.column_stack([q, r])
    s = np.zeros((codes.shape[0], vals.shape[1], 4))
    for j in range(codes.shape[0]):
        for k in range(n):
            s[j, :, codes[j, k]] += vals[k]
    return s, (r * r).sum(axis=0)


ASSOC_SHAPES = [(n, ncov, pn) for n in (12, 40) for ncov in (0, 3) for pn in (1, 2)]


@pytest.fixture(scope="module")
def assoc_refs():
    """per shape: the case, closed_form's rows, the per-code sums, and over all shapes the disagreement with lstsq_fit"""
    cases, worst = [], 0.0
    for i, (n, ncov, pn) in enumerate(ASSOC_SHAPES):
        codes, y, x = assoc_case(100 + i, n, ncov, pn)
        cf = AS.closed_form(codes, y, x)
        bad = np.isnan(cf["BETA"]).all(axis=1)
        ls = AS.lstsq_fit(codes, y, x, skip=bad)
        for key, other in zip(("BETA", "SE", "T"), ls):
            ok = ~np.isnan(cf[key])
            assert (ok == ~np.isnan(other)).all()
            worst = max(worst, (np.abs(cf[key][ok] - other[ok]) / np.abs(other[ok])).max())
        cases.append((codes, y, x, cf, *per_code_sums(codes, y, x)))
    return cases, worst


def test_assoc_rows_against_the_two_numpy_fits(stats_check, tmp_path, assoc_refs):
    cases, disagreement = assoc_refs
    rtol = 100.0 * disagreement
    text = ""
    for codes, y, x, _, s, _ in cases:
        n, v = codes.shape[1], codes.shape[0]
        text += f"assoc {n} {x.shape[1]} {y.shape[1]} {v}\n{floats(x)}\n{floats(y)}\n"
        for j in range(v):
            text += " ".join(str(int((codes[j] == c).sum())) for c in range(4)) + " " + floats(s[j]) + "\n"
    lines = stats_check(text, tmp_path)
    assert len(lines) == len(cases)
    worst, na_rows = 0.0, 0
    for (codes, y, x, cf, _, rr), ln in zip(cases, lines):
        v, pn = codes.shape[0], y.shape[1]
        assert ln[:2] == ["assoc", "-1"] and float.fromhex(ln[2]) == cf["df"] == codes.shape[1] - x.shape[1] - 2
        got_rr = hexes(ln[3:3 + pn])
        worst = max(worst, (np.abs(got_rr - rr) / rr).max())
        rows = np.array(ln[3 + pn:]).reshape(v, pn, 7)
        for j in range(v):
            for p in range(pn):
                has_freq, a1, na = rows[j, p, 0] == "1", float.fromhex(rows[j, p, 1]), rows[j, p, 2] == "1"
                assert has_freq == (not np.isnan(cf["A1_FREQ"][j])) and na == bool(np.isnan(cf["BETA"][j, p])), (j, p, rows[j, p])
                if has_freq:
                    assert abs(a1 - cf["A1_FREQ"][j]) <= 1e-11 * cf["A1_FREQ"][j]
                na_rows += na
                if na:
                    continue
                beta, se, t, pval = hexes(rows[j, p, 3:])
                for got, key in ((beta, "BETA"), (se, "SE"), (t, "T")):
                    worst = max(worst, abs(got - cf[key][j, p]) / abs(cf[key][j, p]))
                assert 0.0 <= pval <= 1.0
        assert np.isnan(cf["BETA"][3:7]).all() and not np.isnan(cf["BETA"][7:]).any()   # the four degenerate variants, and only they
    print(f"closed_form against lstsq_fit: {disagreement:.3g}, so {rtol:.3g} allowed; the program against closed_form: {worst:.3g}; {na_rows} NA rows")
    assert na_rows == 4 * sum(pn for _, _, pn in ASSOC_SHAPES)
    assert worst <= rtol


def test_assoc_design_reports_the_collinear_covariate(stats_check, tmp_path):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((12, 3))
    x[:, 2] = x[:, 0] + x[:, 1]
    y = rng.standard_normal((12, 1))
    constant = np.column_stack([x[:, 0], np.full(12, 3.0)])   # a constant covariate is collinear with the intercept
    lines = stats_check(f"assoc 12 3 1 0\n{floats(x)}\n{floats(y)}\nassoc 12 2 1 0\n{floats(constant)}\n{floats(y)}\n", tmp_path)
    assert lines == [["assoc", "3"], ["assoc", "2"]]   # columns of [1, x]: 0 is the intercept, c is covariate c - 1


# ---- the pca iteration ----

MASK = (1 << 64) - 1


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def gaussian_start(seed, count):
    out, state = [], seed
    for _ in range(count):
        state, o1 = splitmix64(state)
        state, o2 = splitmix64(state)
        u1, u2 = float((o1 >> 11) + 1) * 2.0 ** -53, float(o2 >> 11) * 2.0 ** -53
        out.append(math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2))
    return np.array(out)


def largest_positive(vec):
    return vec * np.sign(vec[np.abs(vec).argmax(axis=0), np.arange(vec.shape[1])])


def test_pca_iteration_against_eigh(stats_check, tmp_path):
    k, l, pcs, tol, seed = 24, 8, 3, 1e-6, 1   # tol, seed, max_passes: the CLI's defaults
    z = np.random.default_rng(23).standard_normal((k, 60))
    m = z @ z.T / 60.0
    m = 0.5 * (m + m.T)
    lines = stats_check(f"start {seed} {k} {l}\nstart 12345678901234567890 3 2\npca {k} {l} {pcs} {seed} {tol!r} 100\n{floats(m)}\n", tmp_path)
    assert hexes(lines[0][1:]).tobytes() == gaussian_start(seed, k * l).tobytes()
    assert hexes(lines[1][1:]).tobytes() == gaussian_start(12345678901234567890, 6).tobytes()
    ln = lines[2]
    passes, converged = int(ln[1]), ln[2] == "1"
    lam, vec = np.linalg.eigh(m)
    lam, vec = lam[::-1], vec[:, ::-1]
    gap = min(np.abs(lam[i] - np.delete(lam, i)).min() for i in range(pcs))
    got_lam, got_vec = hexes(ln[3:3 + pcs]), hexes(ln[3 + pcs:]).reshape(k, pcs)
    print(f"{passes} passes; lambda off by {np.abs(got_lam - lam[:pcs]).max() / lam[0]:.3g} lambda_1 of {tol:.3g} allowed; gap {gap / lam[0]:.3g} lambda_1")
    assert converged and 1 < passes < 100
    assert gap > 2 * tol * lam[0]
    assert (np.abs(got_lam - lam[:pcs]) <= tol * lam[0]).all()
    assert (np.abs(np.linalg.norm(got_vec, axis=0) - 1.0) <= k * 2.0 ** -52).all()
    assert (got_vec[np.abs(got_vec).argmax(axis=0), np.arange(pcs)] > 0).all()
    assert (np.linalg.norm(got_vec - largest_positive(vec[:, :pcs]), axis=0) <= 2 * np.sqrt(2) * tol * lam[0] / gap).all()
