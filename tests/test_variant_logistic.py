"""Per-variant logistic regression and `pgen-hip assoc --logistic` — CPU leg: the C ABI's symbols, constants and header lines, NULL-ctx
refusals, the launch plan that logit_plan.py runs, the command's usage text, usage errors (exit 2), coding errors (exit 101, the
column named), `assoc --p-of-z` against math.erfc, the pure null fit (pgen_rs_amd/host/stats.cpp through the stand-alone
tests/logit_check.cpp under ASan + UBSan) against logit_ref, and the two formulations of logit_ref against each other on the cases of
the GPU compare leg.

Tolerances:
  * --p-of-z: both sides are libm's erfc of |z| / sqrt 2; 4 ulp.
  * null fit: the fitted linear predictor (the coefficients live in different bases: the program's orthonormalised one, the
    reference's raw one) within 100 x the disagreement of the reference with itself in an orthonormal basis plus the stopping gap,
    2 tol sum_c |x_kc| with tol = 1e-12.
  * formulations: statuses equal; beta and SE disagreement far below the 1e-10 stopping gap that dominates the GPU tolerance
    (measured: 1.3e-15 absolute in beta, 7.0e-15 relative in SE; asserted below 1e-12)."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import logit_plan as LP
import logit_ref as LR
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
HOST = REPO / "pgen_rs_amd" / "host"
HEADER = (REPO / "include" / "pgen_hip.h").read_text()


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


# ---- the ABI ----

def test_symbols_constants_and_header_lines():
    for name in ("pgenhip_variant_logistic", "pgenhip_variant_logistic_at"):
        assert name in _capi.PROTOTYPES and hasattr(_capi.lib, name)
        assert re.search(r"^int %s\(pgenhip_ctx \*ctx," % name, HEADER, re.M), name
    defines = dict(re.findall(r"^#define PGENHIP_LOGIT_(\w+)\s+(0x[0-9A-Fa-f]+|\d+)u", HEADER, re.M))
    want = {"MAX_COVARIATES": 15, "MAX_ITER": 64, "AUTO": 0, "GENERAL": 1, "FAST": 2, "SHAPE_MASK": 0xF, "CONVERGED": 0x100,
            "NOT_CONVERGED": 0x200, "SINGULAR": 0x400}
    assert {k: int(v, 0) for k, v in defines.items()} == want
    for k, v in want.items():
        assert getattr(_capi, "LOGIT_" + k) == v
    assert re.search(r"PGENHIP_KNOB_LOGIT_BLOCKS = 32,", HEADER) and _capi.KNOB_LOGIT_BLOCKS == 32
    assert "#define PGENHIP_ABI_VERSION 2u" in HEADER and _capi.lib.pgenhip_abi_version() == 2
    for phrase in ("One row's samples are not split over blocks", "no step\n *     halving and no Firth penalty", "not NaN", "graph-capturable"):
        assert phrase in HEADER, phrase
    assert (LR.CONVERGED, LR.NOT_CONVERGED, LR.SINGULAR) == (_capi.LOGIT_CONVERGED, _capi.LOGIT_NOT_CONVERGED, _capi.LOGIT_SINGULAR)


def test_null_ctx_is_refused():
    lib = _capi.lib
    assert lib.pgenhip_variant_logistic(None, None, 0, None, 1, None, None, 1, 1, None, None, 25, 1e-9, None, 2, None, None, 0) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_variant_logistic_at(None, None, None, 1, None, None, 1, 1, None, None, 25, 1e-9, None, 2, None, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_tune(None, _capi.KNOB_LOGIT_BLOCKS, 1) == _capi.ERR_BAD_ARG


def test_plan_mirror():
    assert (LP.THREADS, LP.WAVES, LP.MAX_P, LP.SUMS) == (256, 4, _capi.LOGIT_MAX_COVARIATES + 1, 16 * 17 // 2 + 16)
    for p in range(2, 17):
        s = LP.shape(p)
        assert s.bucket == (4 if p <= 4 else 8 if p <= 8 else 12 if p <= 12 else 16)
        assert s.waves_per_row == (2 if s.bucket > 8 else 1) and s.group_rows * s.waves_per_row == LP.WAVES
        assert s.sum_fmas == p * (p + 1) // 2 + p
        # a lane's accumulators fit 256 VGPRs: two registers each, and the design row beside them
        assert 2 * (LP.shape(s.bucket).sum_fmas // s.waves_per_row + s.bucket) <= 256 - 32
    # the two waves of a row own the same number of H's entries, and every row of H has one owner
    owned = [sum(a + 1 for a in range(16) if LP.row_part(a, 2) == part) for part in (0, 1)]
    assert owned == [68, 68] and all(LP.row_part(a, 1) == 0 for a in range(16))
    for p, rows in ((4, 4), (8, 4), (9, 2), (13, 2)):
        for v in (1, rows - 1, rows, rows + 1, 1000):
            g = LP.grids(v, p)
            assert g.groups == -(-v // rows) and g.fast == min(g.groups, 256 * LP.BLOCKS_PER_CU) and g.general == min(v, 256 * LP.BLOCKS_PER_CU)
        assert LP.grids(1000, p, blocks=3).fast == 3 and LP.grids(1000, p, blocks=3).general == 3 and LP.grids(2, p, blocks=3).fast == 1


# ---- the command line ----

def test_assoc_logistic_in_usage():
    p = run("help")
    assert p.returncode == 0
    for word in (b"assoc --logistic", b"--no-mean-imputation", b"--max-iter", b"--tol", b"--p-of-z", b"Z_STAT", b"ITER STATUS", b"log-odds per",
                 b"Wald", b"Firth", b"step halving", b"likelihood-ratio", b"interaction", b"no digit parity\n       with plink2 --glm"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [["x", "--logistic"], ["x", "--pheno", "p", "--logistic", "--max-iter", "0"], ["x", "--pheno", "p", "--logistic", "--max-iter", "65"],
                                  ["x", "--pheno", "p", "--logistic", "--max-iter", "many"], ["x", "--pheno", "p", "--logistic", "--tol", "-1"],
                                  ["x", "--pheno", "p", "--logistic", "--tol", "nan"], ["x", "--pheno", "p", "--logistic", "--tol", "1e-9x"],
                                  ["x", "--pheno", "p", "--logistic", "--tol"], ["x", "--pheno", "p", "--max-iter", "5"], ["x", "--pheno", "p", "--tol", "1e-9"],
                                  ["x", "--pheno", "p", "--no-mean-imputation"], ["--p-of-z"], ["--p-of-z", "x"], ["--p-of-z", "1", "2"]])
def test_usage_errors_exit_2(args):
    p = run("assoc", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


@pytest.fixture()
def tiny(tmp_path):
    """Five variants x eight samples behind an all-zero .pgen (the records are never read without a GPU)."""
    (tmp_path / "t.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"1\t%d\tv%d\tA\tG\n" % (10 + i, i) for i in range(5)))
    (tmp_path / "t.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"S%d\tNA\n" % i for i in range(8)))
    (tmp_path / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (5).to_bytes(4, "little") + (8).to_bytes(4, "little") + b"\x40" + bytes(10))
    return tmp_path / "t"


def pheno(values, names=("CC",)):
    head = b"#IID\t" + b"\t".join(n.encode() for n in names) + b"\n"
    return head + b"".join(b"S%d\t" % i + b"\t".join(str(v).encode() for v in row) + b"\n" for i, row in enumerate(values))


def put(tmp_path, name, text):
    (tmp_path / name).write_bytes(text)
    return str(tmp_path / name)


@pytest.mark.parametrize("column,what", [
    ([0, 1, 2, 1, 0, 1, 2, 1], b"not a case/control column"),          # 0, 1 and 2
    ([1, 2, 1.5, 2, 1, 2, 1, 2], b"not a case/control column"),        # a quantitative value
    ([-1, 1, 1, 0, 0, 1, 0, 1], b"not a case/control column"),
    ([1, 1, 1, 1, 1, 1, 1, 1], b"has no control"),                     # no 2: read as 0 / 1, all cases
    ([0, 0, 0, 0, 0, 0, 0, 0], b"has no case"),
    ([1, 1, 1, 1, 1, 1, 1, "NA"], b"has no control"),
    ([2, 1, 1, 1, 1, 1, 1, 1], None),                                  # fine by itself: kept samples decide
])
def test_coding_errors_exit_101_and_name_the_column(tiny, tmp_path, column, what):
    text = pheno([(1 + i % 2, v) for i, v in enumerate(column)], names=("FINE", "BAD"))
    args = ["assoc", str(tiny), "--logistic", "--pheno", put(tmp_path, "p.tsv", text), "--pheno-name", "BAD"]
    if what is None:   # the one case among the complete samples is dropped by the sample query: no case is left
        args += ["--include-sam", 'IID != "S0"']
        what = b"has no case"
    p = run(*args)
    assert p.returncode == 101, p.stderr
    assert what in p.stderr and b"phenotype BAD" in p.stderr and b"FINE" not in p.stderr, p.stderr


def test_too_many_covariates_exit_101(tiny, tmp_path):
    cov = b"IID\t" + b"\t".join(b"C%d" % c for c in range(15)) + b"\n" + b"".join(b"S%d\t" % i + b"\t".join(b"%d" % ((i + 1) ** c % 7) for c in range(15)) + b"\n" for i in range(8))
    p = run("assoc", str(tiny), "--logistic", "--pheno", put(tmp_path, "p.tsv", pheno([(1 + i % 2,) for i in range(8)])), "--covar", put(tmp_path, "c.tsv", cov))
    assert p.returncode == 101 and b"15 covariates" in p.stderr and b"14 at most" in p.stderr, p.stderr


def test_separating_covariate_exits_101_and_names_the_phenotype(tiny, tmp_path):
    cov = b"IID\tA\n" + b"".join(b"S%d\t%d\n" % (i, i) for i in range(8))
    p = run("assoc", str(tiny), "--logistic", "--pheno", put(tmp_path, "p.tsv", pheno([(int(i >= 4),) for i in range(8)])), "--covar", put(tmp_path, "c.tsv", cov))
    assert p.returncode == 101 and b"null model of phenotype CC" in p.stderr, p.stderr


def test_no_kept_variant_prints_the_header_alone(tiny, tmp_path):
    p = run("assoc", str(tiny), "--logistic", "--pheno", put(tmp_path, "p.tsv", pheno([(1 + i % 2,) for i in range(8)])), "--include-var", 'ID == "none"', "--stats")
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tP\tITER\tSTATUS\n"
    assert b'"converged": 0, "not_converged": 0, "singular": 0' in p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101(tiny, tmp_path):
    p = run("assoc", str(tiny), "--logistic", "--pheno", put(tmp_path, "p.tsv", pheno([(i % 2,) for i in range(8)])))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()


def ulp_distance(a, b):
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))


def test_p_of_z_against_erfc():
    zs = [0.0, 1e-300, 1e-9, 0.5, 1.0, 1.959963984540054, 2.5, 5.0, 8.2, 12.0, 20.0, 30.5, 37.5, 38.0] + [k * 38.0 / 23 for k in range(1, 23)]
    worst = 0
    for z in zs:
        for s in (z, -z):
            r = run("assoc", "--p-of-z", repr(s))
            assert r.returncode == 0, r.stderr
            got, want = float(r.stdout), math.erfc(abs(s) / math.sqrt(2.0))
            worst = max(worst, ulp_distance(got, want))
            assert ulp_distance(got, want) <= 4, (s, got, want)
    print(f"--p-of-z: worst distance {worst} ulp")
    assert float(run("assoc", "--p-of-z", "0").stdout) == 1.0 and float(run("assoc", "--p-of-z", "38").stdout) > 0.0


# ---- the pure host arithmetic, stand-alone under the sanitizers ----

@pytest.fixture(scope="module")
def logit_check(tmp_path_factory):
    """The program, and the proof of purity: it links from stats.cpp alone."""
    exe = tmp_path_factory.mktemp("logit") / "logit_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe),
           str(REPO / "tests" / "logit_check.cpp"), str(HOST / "stats.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr

    def run_cases(text, tmp_path):
        (tmp_path / "cases.txt").write_text(text)
        p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", p.stderr
        return [ln.split() for ln in p.stdout.splitlines()]

    return run_cases


def floats(a):
    return " ".join(float(v).hex() if np.isfinite(v) else "nan" for v in np.asarray(a, dtype=np.float64).ravel())


def test_codings(logit_check, tmp_path):
    nan = float("nan")
    cases = [([1, 2, 1, 2], 2), ([1, 1, 1], 1), ([0, 1, 0], 1), ([0, 0], 1), ([2, 2], 2), ([0, 1, 2], 0), ([1, 2, nan, 2], 2), ([nan, nan], 1),
             ([0.5, 1], 0), ([1, 2, 3], 0), ([-0.0, 1], 1), ([], 1)]
    lines = logit_check("".join(f"coding {len(v)} {floats(v)}\n" for v, _ in cases), tmp_path)
    assert [int(ln[1]) for ln in lines] == [want for _, want in cases]


def test_null_fit_against_reference(logit_check, tmp_path):
    tol, text, cases = 1e-12, "", []
    for i, (n, ncov) in enumerate([(30, 0), (63, 1), (200, 3), (500, 14)]):
        _, design, y = LR.make_case(300 + i, n, ncov + 1, v=1)
        cases.append((design, y))
        text += f"null {n} {ncov} 64 {tol!r}\n{floats(design[:, 1:])}\n{floats(y)}\n"
    sep = np.arange(10.0)
    text += f"null 10 1 64 {tol!r}\n{floats(sep)}\n{floats(sep >= 5)}\n"                 # separated by the covariate: never converges
    text += f"null 10 2 64 {tol!r}\n{floats(np.column_stack([sep, 2 * sep + 1]))}\n{floats(sep % 2)}\n"   # collinear covariates
    lines = logit_check(text, tmp_path)
    assert len(lines) == len(cases) + 2
    worst = 0.0
    for (design, y), ln in zip(cases, lines):
        n, m = design.shape
        assert ln[:3] == ["null", "-1", "1"] and 2 <= int(ln[3]) <= 12, ln[:4]
        vals = np.array([float.fromhex(w) for w in ln[4:]])
        eta = vals[m:]
        assert eta.shape == (n,)
        ref_a = design @ LR.null_fit(design, y, tol=tol)
        q = np.linalg.qr(design)[0] * np.sqrt(n)
        ref_b = q @ LR.null_fit(q, y, tol=tol)
        allowed = 100.0 * np.abs(ref_a - ref_b).max() + 2.0 * tol * np.abs(design).sum(axis=1).max()
        err = np.abs(eta - ref_a).max()
        worst = max(worst, err / allowed)
        print(f"n = {n}, m = {m}: the references differ by {np.abs(ref_a - ref_b).max():.3g}; allowed {allowed:.3g}; the program is off by {err:.3g}")
        assert err <= allowed
        if m == 1:   # the program's first column is the constant 1: the intercept alone is the log-odds of the case fraction
            assert abs(vals[0] - np.log(y.mean() / (1 - y.mean()))) <= 1e-12
    assert lines[-2][:3] == ["null", "-1", "0"]
    assert lines[-1] == ["null", "2"]
    assert worst <= 1.0


def test_p_values_in_the_program(logit_check, tmp_path):
    zs = [0.0, -0.0, 1.0, -1.0, 10.0, 38.0, -38.0, float("inf")]
    lines = logit_check("".join(f"pz {z!r}\n" for z in zs), tmp_path)
    for z, ln in zip(zs, lines):
        assert ulp_distance(float.fromhex(ln[1]), math.erfc(abs(z) / math.sqrt(2.0))) <= 4
    nan_line = logit_check("pz nan\n", tmp_path)
    assert "nan" in nan_line[0][1]


def test_stats_sources_stay_pure():
    for name in ("stats.h", "stats.cpp"):
        quoted = [ln.split('"')[1] for ln in (HOST / name).read_text().splitlines() if ln.startswith('#include "')]
        assert set(quoted) <= {"stats.h", "linalg.h"}, (name, quoted)


# ---- the reference against itself ----

def test_formulations_agree_on_the_compare_cases():
    refs = [LR.reference(1000 + i, k, nc, impute) for i, (k, nc) in enumerate(LR.COMPARE_CASES) for impute in (True, False)]
    for r in refs:
        for a in ("loose", "tight", "qr"):
            assert ((r[a][2] & LR.CONVERGED) != 0).all(), "the reference converges on every row of every case"
        assert ((r["tight"][2] & 0xFF) <= 8).all() and (np.abs((r["tight"][2] & 0xFF) - (r["qr"][2] & 0xFF)) <= 1).all()
        assert ((r["loose"][2] & 0xFF) <= 7).all()
    m = LR.measure(refs)
    tol_b, tol_se = LR.tolerances(m)
    print(f"beta gap {m['beta_gap']:.3g}, SE gap {m['se_gap']:.3g}; formulations: beta {m['beta_form']:.3g}, SE {m['se_form']:.3g}; "
          f"allowed on the GPU: beta {tol_b:.3g}, SE {tol_se:.3g}")
    assert m["rows"] == 2 * len(LR.COMPARE_CASES) * LR.COMPARE_V
    assert m["beta_gap"] <= 1e-10 and m["se_gap"] <= 1e-10 and m["beta_form"] <= 1e-12 and m["se_form"] <= 1e-12


def test_reference_edge_rows():
    _, design, y = LR.make_case(3, 50, 2, v=1)
    start = LR.null_fit(design, y)
    zero = np.column_stack([design, np.zeros(50)])
    for fit in (LR.newton, LR.irls_qr):
        beta, se, status = fit(zero, y, start, 25, 1e-10)
        assert status == (LR.SINGULAR | 1) and np.isnan(se) and np.array_equal(beta, np.concatenate([start, [0.0]]))
        beta, se, status = fit(zero[:0], y[:0], start, 25, 1e-10)
        assert status == (LR.SINGULAR | 1)
    sep = np.column_stack([np.ones(50), np.where(y > 0.5, 2.0, 0.0)])
    assert not LR.newton(sep, y, LR.null_fit(sep[:, :1], y), 25, 1e-10)[2] & LR.CONVERGED
    g = np.column_stack([design, np.random.default_rng(1).integers(0, 3, 50).astype(float)])
    beta, se, status = LR.newton(g, y, start, 1, 1e-10)
    assert status == (LR.NOT_CONVERGED | 1) and np.array_equal(beta[:2], start) and beta[2] == 0.0
    codes = np.array([[0, 1, 2, 3, 3, 1]], dtype=np.uint8)
    assert np.array_equal(LR.unpack_codes(LR.pack_codes(codes), 6), codes)
    assert np.array_equal(LR.code_table(codes[0], True), [0.0, 1.0, 2.0, 1.0]) and np.isnan(LR.code_table(codes[0], False)[3])
