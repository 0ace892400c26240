"""Per-variant sums of per-sample values by genotype code and `pgen-hip assoc` — CPU leg: the reference (vsum_ref.py) agrees with the
committed GT text of the golden cases, the launch plan that vsum_plan.py runs has the edges the GPU tests sit on, the C ABI symbols are exported
and refuse a NULL ctx, `pgen-hip assoc` parses its flags and its value files, names the line of what it refuses, and its Student t
routine (`assoc --p-of`) agrees with the committed scipy triples."""
import ctypes as C
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import assoc_ref as AR
import vsum_plan as VP
import vsum_ref as VR
from helpers import GOLDEN, case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
SRC = REPO / "pgen_rs_amd" / "csrc" / "gt_vsum.hip"
ASSOC = GOLDEN / "assoc"

# `assoc --p-of` against tests/golden/assoc/t_triples.json: the worst relative deviation measured over the committed triples with
# p >= 1e-300 is 1.98e-11 (t = 2, df = 10^6: the continued fraction sees x = df / (df + t^2) rounded, 1e-16 / (1 - x) of relative
# error); the tolerance is 10 x that (the rule: floored at 1e-12, capped at 1e-9)
P_RTOL = 2e-10


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.mark.parametrize("name", case_names())
def test_reference_with_ones_counts_the_golden_gt_text(name):
    """A column of ones: the four sums of a row are the numbers of 0/0, 0/1, 1/1 and ./. among its GT fields."""
    v, n, recs, kept, gt = load_case(name)
    rows = bytes(gt).split(b"\n")[:v]
    k = n if kept is None else len(kept)
    want = np.zeros((v, 4))
    for j, row in enumerate(rows):
        fields = row.split(b"\t")[1:]
        assert len(fields) == k
        want[j] = [fields.count(f) for f in (b"0/0", b"0/1", b"1/1", b"./.")] if k else 0
    s, a = VR.vsum_ref(recs, n, np.ones(k), kept)
    assert s.shape == (v, 1, 4) and np.array_equal(s[:, 0, :], want) and a[0] == k


def test_reference_rounds_correctly_and_bounds():
    """fsum, not a float loop: 2^60 + 1.5 - 2^60 is 1.5; the grid-split path gives the same correctly rounded sums as plain fsum."""
    recs = np.array([[0b010101]], dtype=np.uint8)
    s, a = VR.vsum_ref(recs, 3, np.array([2.0 ** 60, 1.5, -(2.0 ** 60)]))
    assert s[0, 0, 1] == 1.5 and a[0] == 2.0 ** 61 + 1.5 and not s[0, 0, [0, 2, 3]].any()
    rng = np.random.default_rng(1)
    n, v = 301, 6
    recs = rng.integers(0, 256, size=(v, VP.record_size(n)), dtype=np.uint8)
    vals = rng.choice([-1.0, 1.0], size=(n, 3)) * rng.uniform(1, 2, size=(n, 3)) * 2.0 ** rng.integers(-20, 21, size=(n, 3))
    assert VR.split_on_grids(vals) is not None and VR.split_on_grids(vals * 2.0 ** 30) is None
    s, _ = VR.vsum_ref(recs, n, vals)
    codes = VR.unpack_codes(recs, n)
    for j in range(v):
        for x in range(4):
            for c in range(3):
                assert s[j, c, x] == math.fsum(vals[codes[j] == x, c])
    assert VR.bound(3000, np.array([1.0]))[0] == 1.01 * 3001 * 2.0 ** -53


def test_plan_mirror_matches_the_source():
    """vsum_plan.py runs gt_vsum.hip's launch plan (csrc/launch_plan.h); these are the values the GPU tests are placed around, and the
    one line of device code they rely on that only the source shows: the last tile is moved back to end at the record's last byte."""
    assert "const uint32_t at = R >= kTileBytes ? min(b0, R - kTileBytes) : 0u;" in SRC.read_text()
    assert VP.THREADS == 256 and VP.TILE_BYTES == 32 and VP.MIN_SLICE_ROWS == 256 and VP.MAX_COLUMNS == _capi.VSUM_MAX_COLUMNS == 16
    assert [VP.tiles(n) for n in (1, 128, 129, 2504, 500_000)] == [1, 1, 2, 20, 3907]
    assert [VP.slices(v, 3) for v in (1, 16, 17, 32, 33, 1000)] == [1, 1, 2, 2, 3, 3]
    assert VP.grid(2504, 1000, 3) == 3 and VP.grid(2504, 1000, 1) == 1 and VP.grid(100, 5, 3) == 1
    assert VP.edge_rows(3)[:7] == [1, 3, 4, 5, 15, 16, 17]
    assert [VP.plan(n)[3] for n in (128, 129)] == [0, 1]   # tiles of a row meet in atomics from the second tile on


def test_flag_ids_and_symbols():
    for sym in ("pgenhip_variant_sums", "pgenhip_variant_sums_at"):
        assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None and sym in _capi.PROTOTYPES
    assert (VP.AUTO, VP.GENERAL, VP.MFMA) == (_capi.VSUM_AUTO, _capi.VSUM_GENERAL, _capi.VSUM_MFMA) == (0, 1, 2)
    assert _capi.VSUM_SHAPE_MASK == 0xF and _capi.KNOB_VSUM_BLOCKS == 23
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for text in ("#define PGENHIP_VSUM_MAX_COLUMNS 16u", "#define PGENHIP_VSUM_GENERAL 1u", "#define PGENHIP_VSUM_MFMA 2u",
                 "#define PGENHIP_VSUM_SHAPE_MASK 0xFu", "PGENHIP_KNOB_VSUM_BLOCKS = 23", "PGENHIP_ABI_VERSION 2u",
                 "(K + 1) * 2^-53 * A_c", "column total minus the other three", "There is no ACCUMULATE flag",
                 "do not count against PGENHIP_LAUNCHES_IN_FLIGHT"):
        assert text in h, text


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_variant_sums(None, None, 0, None, 0, None, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_variant_sums_at(None, None, None, 0, None, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_tune(None, _capi.KNOB_VSUM_BLOCKS, 3) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()


# ---- the two numpy formulations of the fit --------------------------------------------------------------------------------------

def test_closed_form_agrees_with_lstsq_on_the_golden_fileset():
    raw = (ASSOC / "g.pgen").read_bytes()
    v, n = int.from_bytes(raw[3:7], "little"), int.from_bytes(raw[7:11], "little")
    codes = AR.unpack_codes(np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(v, -1), n)
    sys.path.insert(0, str(GOLDEN))
    import make_assoc_golden as G

    iids = [ln.split("\t")[0] for ln in (ASSOC / "g.psam").read_text().split("\n")[1:] if ln]
    names, ph = G.read_values(ASSOC / "pheno.tsv", iids)
    _, cv = G.read_values(ASSOC / "covar.tsv", iids)
    stay = AR.complete_cases(list(range(n)), ph, cv)
    assert len(stay) == n - 4                                    # S005, S017, S040 and S077
    cf = AR.closed_form(codes[:, stay], ph[stay], cv[stay])
    na = np.isnan(cf["BETA"][:, 0])
    assert na[7] and na[11] and na.sum() == 2                    # the monomorphic and the all-missing variant
    beta, se, t = AR.lstsq_fit(codes[:, stay], ph[stay], cv[stay], skip=na)
    rel = max(np.nanmax(np.abs(cf[k] - w) / np.abs(w)) for k, w in (("BETA", beta), ("SE", se), ("T", t)))
    print(f"closed form against lstsq: max relative disagreement {rel:.3g}")
    assert rel < 1e-9
    # the committed expectation is what the reference gives today
    want = json.loads((ASSOC / "expected.json").read_text())
    assert len(want) == v * 2 and want[0]["OBS_CT"] == len(stay)
    for i in (0, 2 * 7, 2 * 11 + 1, 2 * 250 + 1):
        j, c = divmod(i, 2)
        for key, arr in (("BETA", cf["BETA"]), ("SE", cf["SE"]), ("T_STAT", cf["T"])):
            assert (want[i][key] is None and np.isnan(arr[j, c])) or math.isclose(want[i][key], arr[j, c], rel_tol=1e-12)


def test_golden_p_values_are_self_consistent():
    stats = pytest.importorskip("scipy.stats")
    for t, df, p in json.loads((ASSOC / "t_triples.json").read_text()):
        assert p == float(2.0 * stats.t.sf(t, df))
    for row in json.loads((ASSOC / "expected.json").read_text()):
        if row["P"] is not None:
            assert math.isclose(row["P"], float(2.0 * stats.t.sf(abs(row["T_STAT"]), row["OBS_CT"] - 4)), rel_tol=1e-12)


# ---- the CLI without a device ------------------------------------------------------------------------------------------------

def test_p_of_against_the_committed_triples():
    triples = json.loads((ASSOC / "t_triples.json").read_text())
    assert {t[1] for t in triples} >= {1, 1_000_000} and {t[0] for t in triples} >= {0.0, 40.0}
    worst = 0.0
    for t, df, p in triples:
        r = run("assoc", "--p-of", repr(t), repr(df))
        assert r.returncode == 0, r.stderr
        got = float(r.stdout)
        if p >= 1e-300:
            worst = max(worst, abs(got - p) / p)
            assert abs(got - p) <= P_RTOL * p, (t, df, p, got)
        else:
            assert 0.0 <= got <= 1e-300, (t, df, got)
    print(f"--p-of: worst relative deviation {worst:.3g}")
    assert float(run("assoc", "--p-of", "-2.5", "10").stdout) == float(run("assoc", "--p-of", "2.5", "10").stdout)


@pytest.fixture()
def tiny(tmp_path):
    """Five variants x six samples behind an all-zero .pgen (the records are never read without a GPU)."""
    (tmp_path / "t.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"1\t%d\tv%d\tA\tG\n" % (10 + i, i) for i in range(5)))
    (tmp_path / "t.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"S%d\tNA\n" % i for i in range(6)))
    (tmp_path / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (5).to_bytes(4, "little") + (6).to_bytes(4, "little") + b"\x40" + bytes(10))
    return tmp_path / "t"


GOOD_PHENO = b"#IID\tY1\tY2\n" + b"".join(b"S%d\t%d.5\t%d\n" % (i, i * i, 7 - i) for i in range(6))


def put(tmp_path, name: str, text: bytes) -> str:
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


def test_assoc_in_usage():
    p = run("help")
    assert p.returncode == 0
    for word in (b"assoc ", b"--pheno", b"--pheno-name", b"--covar", b"--p-of", b"T_STAT", b"A1_FREQ", b"mean", b"no digit parity with plink2"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["--bogus"], ["a", "b", "--pheno", "p"], ["x"], ["x", "--pheno"], ["x", "--pheno", ""],
                                  ["x", "--pheno", "p", "-q"], ["x", "--pheno", "p", "--covar", ""], ["x", "--pheno", "p", "--pheno-name", "A,,B"],
                                  ["--p-of", "1"], ["--p-of", "1", "x"], ["--p-of", "1", "0"], ["--p-of", "1", "2", "3"]])
def test_usage_errors_exit_2(args):
    p = run("assoc", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


# the whole message behind "<path> line <n>: " for every text of the table below
WHOLE = {
    b"IID\tY1\nS0\t0.5\nS1\tabc\n": b"value 'abc' of column Y1 is not a finite number, NA or nan",
    b"#IID\tY1\tY2\nS0\t0.5\t1\n\nS1\t1\t1e999\n": b"value '1e999' of column Y2 is not a finite number, NA or nan",
    b"IID\tY1\nS0\t1\nS1\n": b"expected 2 tab-separated cells like the header's",
    b"IID\tY1\tY2\nS0\t1\t2\nS1\t1\t2\t3\n": b"expected 3 tab-separated cells like the header's",
    b"IID\tY1\nS0\t1\nS1\t1\nS0\t2\n": b"IID 'S0' occurs twice (first on line 2)",
}


@pytest.mark.parametrize("text,line,what", [
    (b"IID\tY1\nS0\t0.5\nS1\tabc\n", 3, b"not a finite number"),
    (b"#IID\tY1\tY2\nS0\t0.5\t1\n\nS1\t1\t1e999\n", 4, b"not a finite number"),      # (an empty line is skipped, and counted)
    (b"IID\tY1\nS0\t1\nS1\n", 3, b"cells"),
    (b"IID\tY1\tY2\nS0\t1\t2\nS1\t1\t2\t3\n", 3, b"cells"),
    (b"IID\tY1\nS0\t1\nS1\t1\nS0\t2\n", 4, b"occurs twice"),
])
def test_value_file_errors_exit_101_and_name_the_line(tiny, tmp_path, text, line, what):
    """The whole line of stderr: the reader under these files and score's weights file is one, and its wording per file kind is pinned here."""
    bad = put(tmp_path, "p.tsv", text)
    p = run("assoc", str(tiny), "--pheno", bad)
    assert p.returncode == 101 and what in p.stderr, p.stderr
    assert p.stderr == b"pgen-hip: %s line %d: %s\n" % (bad.encode(), line, WHOLE[text]), p.stderr
    # the same reader takes the covariates
    bad = put(tmp_path, "c.tsv", text)
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "ok.tsv", GOOD_PHENO), "--covar", bad)
    assert p.returncode == 101 and p.stderr == b"pgen-hip: %s line %d: %s\n" % (bad.encode(), line, WHOLE[text]), p.stderr


def test_unknown_pheno_name_exits_101(tiny, tmp_path):
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", GOOD_PHENO), "--pheno-name", "Y2,Y9")
    assert p.returncode == 101 and b"p.tsv line 1:" in p.stderr and b"'Y9'" in p.stderr, p.stderr


def test_collinear_covariates_exit_101_and_name_the_column(tiny, tmp_path):
    cov = b"IID\tA\tB\tC\n" + b"".join(b"S%d\t%d\t%d\t%d\n" % (i, i, i * i, 3 * i - 2) for i in range(6))   # C = 3 A - 2
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", b"IID\tY\n" + b"".join(b"S%d\t%d\n" % (i, i % 3) for i in range(6))),
            "--covar", put(tmp_path, "c.tsv", cov))
    assert p.returncode == 101 and b"collinear" in p.stderr and b"covariate C " in p.stderr, p.stderr


def test_too_few_complete_samples_exit_101(tiny, tmp_path):
    pheno = b"IID\tY\nS0\t1\nS1\tNA\nS2\t2\nS3\t\nS4\tnan\nS5\t4\n"                     # three complete samples, m = 2: n - m - 1 = 0
    cov = b"IID\tA\n" + b"".join(b"S%d\t%d\n" % (i, i * i) for i in range(6))
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", pheno), "--covar", put(tmp_path, "c.tsv", cov))
    assert p.returncode == 101 and b"too few samples" in p.stderr and b"3 complete samples" in p.stderr, p.stderr
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", GOOD_PHENO), "--include-sam", 'IID == "nobody"')
    assert p.returncode == 101 and b"no kept sample" in p.stderr, p.stderr
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", b"IID\tY\nT0\t1\nT1\t2\n"))   # nobody of the psam is in the file
    assert p.returncode == 101 and b"no kept sample" in p.stderr, p.stderr


def test_no_kept_variant_prints_the_header_alone(tiny, tmp_path):
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", GOOD_PHENO.replace(b"S5\t25.5", b"S5\tNA")), "--include-var", 'ID == "none"', "--stats")
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\tT_STAT\tP\n"
    assert b'"samples_dropped": 1' in p.stderr and b'"samples_kept": 5' in p.stderr


def test_missing_pheno_file_exits_101(tiny, tmp_path):
    p = run("assoc", str(tiny), "--pheno", str(tmp_path / "absent.tsv"))
    assert p.returncode == 101, p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101(tiny, tmp_path):
    p = run("assoc", str(tiny), "--pheno", put(tmp_path, "p.tsv", GOOD_PHENO))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
