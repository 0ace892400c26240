"""Per-sample weighted dosage sums (polygenic scores) — CPU leg: the reference (score_ref.py) agrees with the committed GT text of
the golden cases, the launch plan that score_plan.py runs has the edges the GPU tests sit on, the C ABI symbols are exported and refuse a NULL
ctx, and `pgen-hip score` parses its flags and its weights file, names the line of what it refuses, and needs no device for the
header alone."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import score_plan as SP
import score_ref as SR
from helpers import GOLDEN, case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.mark.parametrize("name", case_names())
def test_reference_agrees_with_the_golden_gt_text(name):
    """Weights 1, no miss value: a sample's score is the number of '1' characters in its GT fields."""
    v, n, recs, kept, gt = load_case(name)
    rows = bytes(gt).split(b"\n")[:v]
    k = n if kept is None else len(kept)
    want = np.zeros(k, dtype=np.int64)
    for row in rows:
        fields = row.split(b"\t")[1:]
        assert len(fields) == k
        want += np.array([f.count(b"1") for f in fields], dtype=np.int64) if k else 0
    s, a = SR.score_ref(recs, n, np.ones(v, dtype=np.float32), None, kept)
    assert s.shape == (k, 1) and np.array_equal(s[:, 0], want.astype(np.float64)) and np.array_equal(a, s)


def test_reference_rounds_correctly_and_bounds():
    """fsum, not a float loop: 2^60 + 1.5 - 2^60 (code 1 three times, exact terms) is 1.5; the bound scales with sum |term|."""
    recs = np.array([[0b01], [0b01], [0b01]], dtype=np.uint8)
    w = np.array([2.0 ** 60, 1.5, -(2.0 ** 60)], dtype=np.float32)
    s, a = SR.score_ref(recs, 1, w)
    assert s[0, 0] == 1.5 and a[0, 0] == 2.0 ** 61
    # a missing call takes the row's miss value, in f32
    m = np.array([0.1, 0.0, 0.0], dtype=np.float32)
    s, _ = SR.score_ref(np.array([[0b11], [0b10], [0b00]], dtype=np.uint8), 1, np.array([3, 5, 7], dtype=np.float32), m)
    assert s[0, 0] == 3.0 * float(np.float32(0.1)) + 10.0
    assert SR.bound(3000, np.array([1.0]))[0] == 1.01 * 3001 * 2.0 ** -53


def test_plan_mirror_matches_the_source():
    """score_plan.py runs gt_score.hip's launch plan (csrc/launch_plan.h); these are the values the GPU tests are placed around."""
    assert SP.THREADS == 256 and SP.MIN_SLICE_ROWS == 512 and SP.MAX_COLUMNS == _capi.SCORE_MAX_COLUMNS == 8
    assert [SP.lane_bytes(c) for c in range(1, 9)] == [4, 4, 2, 2, 1, 1, 1, 1]
    # the sums a lane keeps never pass 32 doubles
    assert all(4 * SP.lane_bytes(c) * c <= 32 for c in range(1, 9))
    assert [SP.lanes_per_row(n, 1) for n in (1, 16, 17, 32, 33, 1024, 1025, 500_000)] == [1, 1, 2, 2, 4, 64, 64, 64]
    assert [SP.tiles(n, 1) for n in (1024, 1025, 2504, 500_000)] == [1, 2, 3, 489]
    assert [SP.tiles(n, 8) for n in (256, 257, 2504, 500_000)] == [1, 2, 10, 1954]
    assert SP.slots(300, 1) == 8 and SP.step_rows(300, 1) == 32 and SP.step_rows(300, 8) == 8
    assert SP.slices(300, 1, 33, 3) == 2 and SP.slices(300, 1, 65, 3) == 3 and SP.slices(300, 1, 1, 3) == 1


def test_flag_ids_and_symbols():
    for sym in ("pgenhip_sample_scores", "pgenhip_sample_scores_at"):
        assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None and sym in _capi.PROTOTYPES
    assert (SP.AUTO, SP.ROWS, SP.ACCUMULATE) == (_capi.SCORE_AUTO, _capi.SCORE_ROWS, _capi.SCORE_ACCUMULATE) == (0, 1, 0x10)
    assert _capi.SCORE_ACCUMULATE & _capi.SCORE_SHAPE_MASK == 0 and _capi.KNOB_SCORE_SLICES == 21
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for text in ("#define PGENHIP_SCORE_MAX_COLUMNS 8u", "#define PGENHIP_SCORE_ROWS 1u", "#define PGENHIP_SCORE_ACCUMULATE 0x10u",
                 "PGENHIP_KNOB_SCORE_SLICES = 21", "PGENHIP_ABI_VERSION 2u", "reproducibility is NOT promised", "hipMalloc"):
        assert text in h, text
    assert re.search(r"2u is reserved for a matrix-core form", h)


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_sample_scores(None, None, 0, None, 0, None, 0, 1, None, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_scores_at(None, None, None, 0, None, 0, 1, None, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_tune(None, _capi.KNOB_SCORE_SLICES, 3) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()


# ---- the CLI without a device -----------------------------------------------------------------------------------------------

@pytest.fixture()
def tiny(tmp_path):
    """Five variants x three samples behind an all-zero .pgen (the records are never read without a GPU)."""
    (tmp_path / "t.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"1\t%d\tv%d\tA\tG\n" % (10 + i, i) for i in range(5)))
    (tmp_path / "t.psam").write_bytes(b"#IID\tSEX\nS0\tNA\nS1\tNA\nS2\tNA\n")
    (tmp_path / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (5).to_bytes(4, "little") + (3).to_bytes(4, "little") + b"\x40" + bytes(5))
    return tmp_path / "t"


def weights(tmp_path, text: bytes) -> str:
    p = tmp_path / "w.tsv"
    p.write_bytes(text)
    return str(p)


def test_score_in_usage():
    p = run("help")
    assert p.returncode == 0
    for word in (b"score ", b"--weights", b"--no-mean-imputation", b"--avg", b"ALLELE_CT", b"DENOM", b"_SUM", b"_AVG", b".sscore"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["--bogus"], ["a", "b", "--weights", "w"], ["x"], ["x", "--weights"], ["x", "--weights", ""],
                                  ["x", "--weights", "w", "-q"], ["x", "--weights", "w", "--dry-run"], ["x", "--weights", "w", "--avg=1", "--out"]])
def test_usage_errors_exit_2(args):
    p = run("score", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


# the whole message behind "<path> line <n>: " for every text of the table below
WHOLE = {
    b"ID\tA1\tS1\nv0\tG\t0.5\nv1\tG\tabc\n": b"weight 'abc' of score S1 is not a finite number",
    b"#ID\tA1\tS1\tS2\nv0\tG\t0.5\t1\n\nv1\tG\t1\tnan\n": b"weight 'nan' of score S2 is not a finite number",
    b"ID\tA1\tS1\nv0\tG\t1e39\n": b"weight '1e39' of score S1 is not a finite number",
    b"ID\tA1\tS1\nv0\tG\t\n": b"weight '' of score S1 is not a finite number",
    b"ID\tA1\tS1\nv0\tG\t1\nv1\tG\n": b"expected 3 tab-separated cells like the header's",
    b"ID\tA1\tS1\tS2\nv0\tG\t1\t2\nv1\tG\t1\t2\t3\n": b"expected 4 tab-separated cells like the header's",
    b"ID\tA1\tS1\nv0\tG\t1\nv1\tG\t1\nv0\tA\t2\n": b"variant ID 'v0' occurs twice (first on line 2)",
}


@pytest.mark.parametrize("text,line,what", [
    (b"ID\tA1\tS1\nv0\tG\t0.5\nv1\tG\tabc\n", 3, b"not a finite number"),
    (b"#ID\tA1\tS1\tS2\nv0\tG\t0.5\t1\n\nv1\tG\t1\tnan\n", 4, b"not a finite number"),      # (an empty line is skipped, and counted)
    (b"ID\tA1\tS1\nv0\tG\t1e39\n", 2, b"not a finite number"),                                   # finite in FP64, not in f32
    (b"ID\tA1\tS1\nv0\tG\t\n", 2, b"not a finite number"),
    (b"ID\tA1\tS1\nv0\tG\t1\nv1\tG\n", 3, b"cells"),
    (b"ID\tA1\tS1\tS2\nv0\tG\t1\t2\nv1\tG\t1\t2\t3\n", 3, b"cells"),
    (b"ID\tA1\tS1\nv0\tG\t1\nv1\tG\t1\nv0\tA\t2\n", 4, b"occurs twice"),
])
def test_weights_file_errors_exit_101_and_name_the_line(tiny, tmp_path, text, line, what):
    """The whole line of stderr: the reader under this file and assoc's value files is one, and its wording per file kind is pinned here."""
    w = weights(tmp_path, text)
    p = run("score", str(tiny), "--weights", w)
    assert p.returncode == 101 and what in p.stderr, p.stderr
    assert p.stderr == b"pgen-hip: %s line %d: %s\n" % (w.encode(), line, WHOLE[text]), p.stderr


def test_header_without_a_score_column_exits_101(tiny, tmp_path):
    p = run("score", str(tiny), "--weights", weights(tmp_path, b"ID\tA1\nv0\tG\n"))
    assert p.returncode == 101 and b"line 1" in p.stderr, p.stderr


def test_matched_id_twice_among_the_kept_variants_exits_101(tmp_path):
    (tmp_path / "d.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n1\t10\tv0\tA\tG\n1\t11\tdup\tA\tG\n1\t12\tdup\tA\tC\n")
    (tmp_path / "d.psam").write_bytes(b"#IID\nS0\n")
    (tmp_path / "d.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (3).to_bytes(4, "little") + (1).to_bytes(4, "little") + b"\x40" + bytes(3))
    w = weights(tmp_path, b"ID\tA1\tS1\nv0\tG\t1\ndup\tG\t2\n")
    p = run("score", str(tmp_path / "d"), "--weights", w)
    assert p.returncode == 101 and b"w.tsv line 3:" in p.stderr and b"twice among the kept variants" in p.stderr, p.stderr
    # with one of the two filtered out the ID is unique among the kept variants, and nobody is kept: the header alone
    p = run("score", str(tmp_path / "d"), "--weights", w, "--include-var", 'ALT == "G"', "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0 and p.stdout == b"#IID\tALLELE_CT\tDENOM\tS1_SUM\n", p.stderr


@pytest.mark.parametrize("text,flags", [
    (b"ID\tA1\tS1\nnope\tG\t1\nnada\tA\t2\n", []),                         # unknown IDs
    (b"ID\tA1\tS1\nv0\tT\t1\nv1\tC\t2\n", []),                              # neither allele
    (b"ID\tA1\tS1\nv0\tG\t1\n", ["--include-var", 'ID != "v0"']),           # the ID is not kept
    (b"ID\tA1\tS1\n", []),                                                  # no row at all
])
def test_zero_matches_exits_101(tiny, tmp_path, text, flags):
    p = run("score", str(tiny), "--weights", weights(tmp_path, text), *flags)
    assert p.returncode == 101 and b"names a kept variant" in p.stderr, p.stderr
    assert p.stdout == b""


def test_no_kept_sample_prints_the_header_alone(tiny, tmp_path):
    w = weights(tmp_path, b"#ID\tA1\tPRS_A\tPRS_B\nv0\tG\t0.5\t-1\nv3\tA\t2\t3\n")
    p = run("score", str(tiny), "--weights", w, "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"#IID\tALLELE_CT\tDENOM\tPRS_A_SUM\tPRS_B_SUM\n"
    p = run("score", str(tiny), "--weights", w, "--include-sam", 'IID == "nobody"', "--avg", "--no-mean-imputation", "--stats")
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"#IID\tALLELE_CT\tDENOM\tPRS_A_AVG\tPRS_B_AVG\n"
    assert b'"weights_matched": 2, "weights_flipped": 1, "weights_skipped": 0' in p.stderr


def test_missing_weights_file_exits_101(tiny, tmp_path):
    p = run("score", str(tiny), "--weights", str(tmp_path / "absent.tsv"))
    assert p.returncode == 101, p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101(tiny, tmp_path):
    p = run("score", str(tiny), "--weights", weights(tmp_path, b"ID\tA1\tS1\nv0\tG\t1\n"))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
