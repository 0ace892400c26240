"""GPU leg of `pgen-hip assoc`: linear regression end to end (value files -> complete cases -> Q and residuals on the host -> records
staged to HBM -> per block the variant counts and the per-code sums of every value column -> BETA, SE, T_STAT, P per variant and
phenotype) against tests/assoc_ref.py's closed form in numpy float64, and on the committed fileset against
tests/golden/assoc/expected.json field by field.

OBS_CT, MISS_CT and the NA rows must be exact.  Tolerance of BETA, SE and T_STAT (relative), measured, not assumed: the largest
relative disagreement between the two numpy formulations of the same fit (assoc_ref.closed_form against assoc_ref.lstsq_fit) is
3.55e-10 on the committed fileset (120 samples) and 5.06e-8 over the cases of the synthesised filesets below (300 samples, allele
frequencies 0.05 .. 0.5; per case 4.7e-11 without covariates, 5.5e-9 with three, 3.6e-10 on the kept subset, 5.1e-8 with twenty
phenotypes, 4.7e-9 on the mode-0x10 fileset: the largest figures belong to estimates that happen to lie near zero, where a relative
measure is at its weakest); the tests allow 100 x that, 3.6e-8 and 5.1e-6 (the floor of 1e-10 does not bind).  A1_FREQ is a quotient
of two exact counts printed with 12 digits: 1e-11.  P on the committed fileset: the same relative tolerance as T_STAT against the
golden values (scipy), for P >= 1e-300."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import assoc_ref as AR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
ASSOC = GOLDEN / "assoc"
V, N, P_ALL, N_COV = 3000, 300, 20, 3
POS0 = 16050000
POS_CUT = POS0 + 7 * 2500            # --include-var keeps the variants in front of it
RTOL_GOLDEN = 100 * 3.55e-10
RTOL_SYNTH = 100 * 5.06e-8
HEADER = "#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tP"


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def make_data(seed=77):
    """-> (codes (V, N), keep flags, pheno (N, 20), covar (N, 3)): Hardy-Weinberg codes at allele frequencies 0.05 .. 0.5 with 1 %
    missing calls, variant 5 monomorphic, variant 9 missing everywhere; a few samples with a missing value."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=V)
    codes = (rng.random((V, N)) < af[:, None]).astype(np.uint8) + (rng.random((V, N)) < af[:, None]).astype(np.uint8)
    codes[rng.random((V, N)) < 0.01] = 3
    codes[5] = 0
    codes[9] = 3
    keep = np.arange(N) % 3 != 0
    covar = np.column_stack([rng.normal(50.0, 10.0, size=N), rng.integers(0, 2, size=N).astype(np.float64), rng.normal(size=N)])
    dos = np.where(codes == 3, 0, codes).astype(np.float64)
    pheno = np.column_stack([0.5 * dos[20 + 31 * p] + 0.02 * (p % 3) * covar[:, 0] + rng.normal(scale=1.0 + p, size=N) + 10.0 * p for p in range(P_ALL)])
    pheno[4, 0] = np.nan
    pheno[8, 1] = np.nan
    pheno[100, 19] = np.nan
    covar[31, 2] = np.nan
    # the files print 17 significant digits: what is parsed back is what is written
    return codes, keep, pheno, covar


def cell(x):
    return "NA" if np.isnan(x) else repr(float(x))


def write_text_files(d: Path, stem: str, codes, keep, pheno, covar, extra_var_cols=None):
    iids = [f"S{k:06d}" for k in range(N)]
    head = "#CHROM\tPOS\tID\tREF\tALT" + ("\tRTYPE" if extra_var_cols is not None else "") + "\n"
    (d / f"{stem}.pvar").write_text(head + "".join(
        f"22\t{POS0 + 7 * j}\tv{j}\tA\tG" + (f"\t{extra_var_cols[j]}" if extra_var_cols is not None else "") + "\n" for j in range(len(codes))))
    (d / f"{stem}.psam").write_text("#IID\tSEX\tKEEP\n" + "".join(f"{iids[k]}\tNA\t{int(keep[k])}\n" for k in range(N)))
    (d / "pheno.tsv").write_text("#IID\t" + "\t".join(f"Y{p}" for p in range(P_ALL)) + "\n" +
                                 "".join("\t".join([iids[k]] + [cell(x) for x in pheno[k]]) + "\n" for k in range(N - 1, -1, -1) if k != 50))
    (d / "covar.tsv").write_text("IID\tAGE\tSEX\tPC1\n" + "".join("\t".join([iids[k]] + [cell(x) for x in covar[k]]) + "\n" for k in range(N)))


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc")
    codes, keep, pheno, covar = make_data()
    (d / "s.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + AR.pack_codes(codes).tobytes())
    write_text_files(d, "s", codes, keep, pheno, covar)
    pheno = pheno.copy()
    pheno[50] = np.nan       # the sample the pheno file does not hold
    return d, codes, keep, pheno, covar


def check(stdout: bytes, codes, var_kept, sam_kept, pheno, covar, pcols, rtol, stderr=b""):
    """The CLI's lines against the closed form over the complete cases among sam_kept."""
    ids = [f"v{j}" for j in var_kept]
    stay = AR.complete_cases(sam_kept, pheno[:, pcols], covar)
    ref = AR.closed_form(codes[np.asarray(var_kept)][:, stay], pheno[stay][:, pcols], covar[stay])
    lines = stdout.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert len(body) == len(ids) * len(pcols)
    worst = 0.0
    t_and_p = []
    for i, b in enumerate(body):
        j, c = divmod(i, len(pcols))
        assert b[2] == ids[j] and b[5] == b[4] == "G" and b[6] == f"Y{pcols[c]}"
        assert int(b[7]) == len(stay), "OBS_CT"
        assert int(b[8]) == ref["MISS_CT"][j], "MISS_CT"
        if np.isnan(ref["A1_FREQ"][j]):
            assert b[9] == "NA"
        else:
            assert abs(float(b[9]) - ref["A1_FREQ"][j]) <= 1e-11 * ref["A1_FREQ"][j]
        want = [ref["BETA"][j, c], ref["SE"][j, c], ref["T"][j, c]]
        if np.isnan(want[0]):
            assert b[10:] == ["NA"] * 4, (ids[j], b)
            continue
        for got, w in zip(b[10:13], want):
            rel = abs(float(got) - w) / abs(w)
            worst = max(worst, rel)
            assert rel <= rtol, (ids[j], b, want)
        assert 0.0 <= float(b[13]) <= 1.0
        t_and_p.append((abs(float(b[12])), float(b[13])))
    # one df for the whole run: P falls as |T_STAT| grows (both are printed with 12 digits, hence the 1e-9)
    t_and_p.sort()
    assert all(q[1] <= p[1] * (1 + 1e-9) for p, q in zip(t_and_p, t_and_p[1:])) and t_and_p[0][1] > 0.9 and t_and_p[-1][1] < 0.05
    print(f"{len(body)} lines: max relative deviation {worst:.3g} of {rtol:.3g} allowed")
    if stderr:
        assert f'"samples_dropped": {len(sam_kept) - len(stay)}'.encode() in stderr, stderr
    return ref


def test_golden_fileset_every_field():
    p = run("assoc", str(ASSOC / "g"), "--pheno", str(ASSOC / "pheno.tsv"), "--covar", str(ASSOC / "covar.tsv"), "--stats")
    assert p.returncode == 0, p.stderr
    assert b'"samples_dropped": 4' in p.stderr
    want = json.loads((ASSOC / "expected.json").read_text())
    lines = p.stdout.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == "" and len(lines) == len(want) + 2
    worst = {"BETA": 0.0, "SE": 0.0, "T_STAT": 0.0, "P": 0.0}
    n_na = 0
    for ln, w in zip(lines[1:-1], want):
        b = ln.split("\t")
        assert b[0] == "22" and b[2] == w["ID"] and b[5] == b[4] and b[6] == w["PHENO"]
        assert int(b[7]) == w["OBS_CT"] and int(b[8]) == w["MISS_CT"]
        assert (b[9] == "NA") if w["A1_FREQ"] is None else abs(float(b[9]) - w["A1_FREQ"]) <= 1e-11 * w["A1_FREQ"]
        for key, got in zip(("BETA", "SE", "T_STAT", "P"), b[10:]):
            if w[key] is None:
                assert got == "NA"
                n_na += 1
            elif key != "P" or w[key] >= 1e-300:
                rel = abs(float(got) - w[key]) / abs(w[key])
                worst[key] = max(worst[key], rel)
                assert rel <= RTOL_GOLDEN, (w, b)
    print("max relative deviation:", worst)
    assert n_na == 2 * 2 * 4   # the monomorphic and the all-missing variant, two phenotypes, four fields


@pytest.mark.parametrize("case", ["no_covar", "covar3", "kept_samples", "include_var", "shards3", "shards7", "twenty_phenotypes"])
def test_synthesised_fileset_against_the_reference(synth, case):
    d, codes, keep, pheno, covar = synth
    var_kept, sam_kept, pcols = list(range(V)), list(range(N)), [0, 1]
    flags = ["--pheno-name", "Y0,Y1", "--covar", str(d / "covar.tsv")]
    cv = covar
    if case == "no_covar":
        flags, cv = ["--pheno-name", "Y0,Y1"], np.zeros((N, 0))
    if case == "kept_samples":
        flags += ["--include-sam", 'KEEP == "1"']
        sam_kept = [k for k in range(N) if keep[k]]
    if case == "include_var":
        flags += ["--include-var", f'POS < "{POS_CUT}"']
        var_kept = [j for j in range(V) if POS0 + 7 * j < POS_CUT]
        assert 9 < len(var_kept) < V
    if case == "shards3":
        flags += ["--shards", "3"]
    if case == "shards7":    # R = 75 bytes: a 1-MiB block would hold every row, so cut the rows with shards of their own blocks
        flags += ["--shards", "7", "--include-sam", 'IID != "S000005"']
        sam_kept = [k for k in range(N) if k != 5]
    if case == "twenty_phenotypes":   # 1 + 3 + 20 value columns: two column groups
        flags, pcols = ["--covar", str(d / "covar.tsv")], list(range(P_ALL))
    p = run("assoc", str(d / "s"), "--pheno", str(d / "pheno.tsv"), *flags, "--stats")
    assert p.returncode == 0, p.stderr
    ref = check(p.stdout, codes, var_kept, sam_kept, pheno, cv, pcols, RTOL_SYNTH, p.stderr)
    na = np.isnan(ref["BETA"][:, 0])
    assert na[5] and na[9] and na.sum() == 2 and ref["MISS_CT"][9] == ref["df"] + 2 + cv.shape[1]


def test_output_file_equals_stdout(synth, tmp_path):
    d = synth[0]
    out = tmp_path / "s.assoc"
    args = ["assoc", str(d / "s"), "--pheno", str(d / "pheno.tsv"), "--pheno-name", "Y3", "--include-var", f'POS < "{POS_CUT}"']
    a, b = run(*args), run(*args, "-o", str(out))
    assert a.returncode == 0 and b.returncode == 0 and b.stdout == b"", (a.stderr, b.stderr)
    la, lb = a.stdout.split(b"\n"), out.read_bytes().split(b"\n")
    # sums in another order may differ in the last printed digit: compare the exact columns and the shape
    assert len(la) == len(lb) and [x.split(b"\t")[:9] for x in la] == [x.split(b"\t")[:9] for x in lb]


def test_variable_width_plain_records_go_through_at(tmp_path):
    """A mode-0x10 file: the kept plain records are staged as they lie on disk and summed through their byte offsets."""
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    codes, keep, pheno, covar = make_data(seed=78)
    codes = codes[:1500]
    rng = np.random.default_rng(2032)
    types = np.where(rng.random(len(codes)) < 0.8, 0, rng.integers(1, 8, size=len(codes))).tolist()
    types[0] = types[5] = types[9] = 0
    recs = writer.make_records(rng, N, types)
    packed = AR.pack_codes(codes)
    recs = [(ty, packed[j].tobytes() if ty == 0 else body) for j, (ty, body) in enumerate(recs)]
    data, _ = writer.write_vw(N, recs, 8, 2)
    (tmp_path / "vw.pgen").write_bytes(data)
    write_text_files(tmp_path, "vw", codes, keep, pheno, covar, extra_var_cols=types)
    pheno = pheno.copy()
    pheno[50] = np.nan
    var_kept = [j for j in range(len(codes)) if types[j] == 0]
    for extra, sam_kept in ([], list(range(N))), (["--include-sam", 'KEEP == "1"', "--shards", "3"], [k for k in range(N) if keep[k]]):
        p = run("assoc", str(tmp_path / "vw"), "--pheno", str(tmp_path / "pheno.tsv"), "--pheno-name", "Y2,Y7", "--covar", str(tmp_path / "covar.tsv"),
                "--include-var", 'RTYPE == "0"', *extra)
        assert p.returncode == 0, p.stderr
        check(p.stdout, codes, var_kept, sam_kept, pheno, covar, [2, 7], RTOL_SYNTH)
    p = run("assoc", str(tmp_path / "vw"), "--pheno", str(tmp_path / "pheno.tsv"))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr
