"""GPU leg of `pgen-hip assoc --logistic`: case/control files -> coding -> complete cases -> design and null models on the host -> per
block the variant counts, the code tables and pgenhip_variant_logistic per phenotype -> BETA, SE, Z_STAT, P, ITER, STATUS per variant
and phenotype, against tests/logit_ref.py (newton run to 1e-13 on the same complete cases, covariates standardised: the genotype's
coefficient and its SE do not depend on the basis of the covariates' span).

The command runs with --tol 1e-10 --max-iter 25, the setting of the kernel's compare leg, and BETA and SE are held to that leg's
tolerances (logit_ref.tolerances over logit_ref.COMPARE_CASES, computed once here) plus the rounding of a value printed with 12
digits; Z_STAT and P to what those two propagate to (dP/dz = -2 phi(z)).  OBS_CT, MISS_CT, STATUS and the NA fields are exact, ITER
within +-1 of the reference stopped at 1e-10.  Linear `assoc` on the committed fileset must still print tests/golden/assoc/linear.tsv,
the parent commit's output, byte for byte."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import logit_ref as LR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
ASSOC = GOLDEN / "assoc"
V, N = 3000, 300
POS0 = 16050000
POS_CUT = POS0 + 7 * 400
HEADER = "#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\tZ_STAT\tP\tITER\tSTATUS"
PRINT = 5e-12   # relative rounding of %.12g


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def make_data(seed=177, v=V):
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=v)
    codes = (rng.random((v, N)) < af[:, None]).astype(np.uint8) + (rng.random((v, N)) < af[:, None]).astype(np.uint8)
    codes[rng.random((v, N)) < 0.01] = 3
    codes[5] = 0      # monomorphic: SINGULAR
    codes[9] = 3      # missing everywhere: SINGULAR, no A1_FREQ
    keep = np.arange(N) % 3 != 0
    covar = np.column_stack([rng.normal(50.0, 10.0, size=N), rng.integers(0, 2, size=N).astype(np.float64), rng.normal(size=N)])
    dos = np.where(codes == 3, 0, codes).astype(np.float64)
    eta = 0.6 * dos[20] - 0.5 * dos[51] + 0.03 * (covar[:, 0] - 50.0) + 0.4 * covar[:, 2] - 0.2
    y = (rng.random(N) < LR.logistic(eta)).astype(np.float64)
    pheno = np.column_stack([y + 1.0, y, (rng.random(N) < 0.3).astype(np.float64)])   # CC12 (1 / 2), CC01 (0 / 1), OTHER (0 / 1)
    pheno[4, 0] = pheno[4, 1] = np.nan
    pheno[100, 2] = np.nan
    covar[31, 2] = np.nan
    return codes, keep, pheno, covar


NAMES = ["CC12", "CC01", "OTHER"]


def cell(x):
    return "NA" if np.isnan(x) else repr(float(x))


def write_text_files(d, stem, codes, keep, pheno, covar, extra=None):
    iids = [f"S{k:06d}" for k in range(N)]
    head = "#CHROM\tPOS\tID\tREF\tALT" + ("\tRTYPE" if extra is not None else "") + "\n"
    (d / f"{stem}.pvar").write_text(head + "".join(f"22\t{POS0 + 7 * j}\tv{j}\tA\tG" + (f"\t{extra[j]}" if extra is not None else "") + "\n" for j in range(len(codes))))
    (d / f"{stem}.psam").write_text("#IID\tSEX\tKEEP\n" + "".join(f"{iids[k]}\tNA\t{int(keep[k])}\n" for k in range(N)))
    (d / "pheno.tsv").write_text("#IID\t" + "\t".join(NAMES) + "\n" + "".join("\t".join([iids[k]] + [cell(x) for x in pheno[k]]) + "\n" for k in range(N - 1, -1, -1) if k != 50))
    (d / "covar.tsv").write_text("IID\tAGE\tSEX\tPC1\n" + "".join("\t".join([iids[k]] + [cell(x) for x in covar[k]]) + "\n" for k in range(N)))


@pytest.fixture(scope="module")
def tolerances():
    refs = [LR.reference(1000 + i, k, nc, impute) for i, (k, nc) in enumerate(LR.COMPARE_CASES) for impute in (True, False)]
    return LR.tolerances(LR.measure(refs))


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("logistic")
    codes, keep, pheno, covar = make_data()
    (d / "s.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + LR.pack_codes(codes).tobytes())
    write_text_files(d, "s", codes, keep, pheno, covar)
    pheno = pheno.copy()
    pheno[50] = np.nan       # the sample the pheno file does not hold
    return d, codes, keep, pheno, covar


_REFS = {}


def reference(key, codes, stay, y, covar, impute):
    """newton to 1e-13 and to 1e-10 over the complete cases, cached per (fileset, sample set, phenotype, covariates, policy)"""
    if key not in _REFS:
        kc = codes[:, stay]
        cv = covar[stay]
        design = np.column_stack([np.ones(len(stay)), (cv - cv.mean(axis=0)) / cv.std(axis=0)]) if cv.shape[1] else np.ones((len(stay), 1))
        table = LR.tables(kc, impute)
        start = LR.null_fit(design, y[stay])
        _REFS[key] = (LR.fit_rows(LR.newton, kc, table, design, y[stay], start, 25, 1e-13), LR.fit_rows(LR.newton, kc, table, design, y[stay], start, 25, 1e-10), kc)
    return _REFS[key]


def check(stdout, key, codes, var_kept, sam_kept, pheno, covar, pcols, impute, tols, stderr=b""):
    tol_b, tol_se = tols
    used = pheno[:, pcols]
    stay = [k for k in sam_kept if not np.isnan(used[k]).any() and not np.isnan(covar[k]).any()]
    lines = stdout.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert len(body) == len(var_kept) * len(pcols)
    counts = {".": 0, "NOT_CONVERGED": 0, "SINGULAR": 0}
    worst = [0.0, 0.0, 0.0, 0.0]
    for c, pc in enumerate(pcols):
        y = pheno[:, pc] - (1.0 if NAMES[pc] == "CC12" else 0.0)
        tight, loose, kc = reference((key, tuple(stay), NAMES[pc][:2] + str(pc >= 2), covar.shape[1], impute), codes, stay, y, covar, impute)
        for i, j in enumerate(var_kept):
            b = body[i * len(pcols) + c]
            assert b[2] == f"v{j}" and b[5] == b[4] == "G" and b[6] == NAMES[pc]
            miss = int((kc[j] == 3).sum())
            assert int(b[8]) == miss and int(b[7]) == (len(stay) if impute else len(stay) - miss)
            called = kc[j][kc[j] != 3]
            if len(called):
                assert abs(float(b[9]) - called.mean() / 2.0) <= 1e-11
            else:
                assert b[9] == "NA"
            bits = int(loose[2][j]) & ~0xFF
            want_status = "." if bits == LR.CONVERGED else "SINGULAR" if bits == LR.SINGULAR else "NOT_CONVERGED"
            assert b[15] == want_status, (b, hex(int(loose[2][j])))
            counts[b[15]] += 1
            assert abs(int(b[14]) - (int(loose[2][j]) & 0xFF)) <= 1, b
            if b[15] != ".":
                assert b[10:14] == ["NA"] * 4
                continue
            beta, se = tight[0][j][-1], tight[1][j]
            z = beta / se
            got = [float(w) for w in b[10:14]]
            eb, es = abs(got[0] - beta), abs(got[1] - se) / se
            assert eb <= tol_b + PRINT * abs(beta) and es <= tol_se + PRINT, (b, beta, se)
            dz = tol_b / se + abs(z) * (tol_se + 2 * PRINT) + PRINT * abs(z)
            assert abs(got[2] - z) <= dz, (b, z)
            phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
            p_want = math.erfc(abs(z) / math.sqrt(2.0))
            assert abs(got[3] - p_want) <= 1.01 * 2.0 * phi * dz + PRINT * p_want, (b, p_want)
            worst = [max(worst[0], eb), max(worst[1], es), max(worst[2], abs(got[2] - z)), max(worst[3], abs(got[3] - p_want))]
    print(f"{len(body)} lines ({counts}): BETA off by {worst[0]:.3g} of {tol_b:.3g}, SE by {worst[1]:.3g} of {tol_se:.3g}, Z by {worst[2]:.3g}, P by {worst[3]:.3g}")
    if stderr:
        assert f'"samples_dropped": {len(sam_kept) - len(stay)}'.encode() in stderr, stderr
        assert f'"converged": {counts["."]}, "not_converged": {counts["NOT_CONVERGED"]}, "singular": {counts["SINGULAR"]}'.encode() in stderr, stderr
    return counts


@pytest.mark.parametrize("case", ["no_covar", "covar3", "both_codings", "kept_samples", "include_var", "shards3", "shards7", "no_mean_imputation"])
def test_synthesised_fileset_against_the_reference(synth, tolerances, case):
    d, codes, keep, pheno, covar = synth
    var_kept, sam_kept, pcols, impute = list(range(0, V)), list(range(N)), [0], True
    flags = ["--pheno-name", "CC12", "--covar", str(d / "covar.tsv")]
    cv = covar
    if case == "no_covar":
        flags, cv = ["--pheno-name", "CC12"], np.zeros((N, 0))
    if case == "both_codings":
        flags[1], pcols = "CC12,CC01,OTHER", [0, 1, 2]
    if case == "kept_samples":
        flags += ["--include-sam", 'KEEP == "1"']
        sam_kept = [k for k in range(N) if keep[k]]
    if case == "shards3":
        flags += ["--shards", "3"]
    if case == "shards7":
        flags += ["--shards", "7", "--include-sam", 'IID != "S000005"']
        sam_kept = [k for k in range(N) if k != 5]
    if case == "no_mean_imputation":
        flags += ["--no-mean-imputation"]
        impute = False
    if case != "no_covar" and case != "covar3":   # the reference is a python loop over the rows: the other cases take the leading variants
        flags += ["--include-var", f'POS < "{POS_CUT}"']
        var_kept = [j for j in range(V) if POS0 + 7 * j < POS_CUT]
        assert 9 < len(var_kept) < V
    if case == "include_var":
        assert "--include-var" in flags
    p = run("assoc", str(d / "s"), "--logistic", "--tol", "1e-10", "--max-iter", "25", "--pheno", str(d / "pheno.tsv"), *flags, "--stats")
    assert p.returncode == 0, p.stderr
    counts = check(p.stdout, "s", codes, var_kept, sam_kept, pheno, cv, pcols, impute, tolerances, p.stderr)
    assert counts["SINGULAR"] >= 2 * len(pcols) and counts["."] >= 0.95 * len(var_kept) * len(pcols)
    if case == "both_codings":   # the two codings of one phenotype print the same numbers
        body = [ln.split("\t") for ln in p.stdout.decode().split("\n")[1:-1]]
        assert all(a[7:] == b[7:] for a, b in zip(body[0::3], body[1::3]))


def test_variable_width_plain_records_go_through_at(tmp_path, tolerances):
    """A mode-0x10 file: the kept plain records are staged as they lie on disk and fitted through their byte offsets."""
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    codes, keep, pheno, covar = make_data(seed=178, v=600)
    rng = np.random.default_rng(2033)
    types = np.where(rng.random(len(codes)) < 0.8, 0, rng.integers(1, 8, size=len(codes))).tolist()
    types[0] = types[5] = types[9] = 0
    recs = writer.make_records(rng, N, types)
    packed = LR.pack_codes(codes)
    recs = [(ty, packed[j].tobytes() if ty == 0 else body) for j, (ty, body) in enumerate(recs)]
    data, _ = writer.write_vw(N, recs, 8, 2)
    (tmp_path / "vw.pgen").write_bytes(data)
    write_text_files(tmp_path, "vw", codes, keep, pheno, covar, extra=types)
    pheno = pheno.copy()
    pheno[50] = np.nan
    var_kept = [j for j in range(len(codes)) if types[j] == 0]
    for extra, sam_kept in ([], list(range(N))), (["--include-sam", 'KEEP == "1"', "--shards", "3"], [k for k in range(N) if keep[k]]):
        p = run("assoc", str(tmp_path / "vw"), "--logistic", "--tol", "1e-10", "--pheno", str(tmp_path / "pheno.tsv"), "--pheno-name", "CC01", "--covar",
                str(tmp_path / "covar.tsv"), "--include-var", 'RTYPE == "0"', *extra)
        assert p.returncode == 0, p.stderr
        check(p.stdout, "vw", codes, var_kept, sam_kept, pheno, covar, [1], True, tolerances)


def test_linear_assoc_prints_what_the_parent_commit_printed():
    p = run("assoc", str(ASSOC / "g"), "--pheno", str(ASSOC / "pheno.tsv"), "--covar", str(ASSOC / "covar.tsv"))
    assert p.returncode == 0, p.stderr
    assert p.stdout == (ASSOC / "linear.tsv").read_bytes()
