"""Per-sample genotype counts — CPU leg: the two C ABI symbols are exported and bound, argument errors come back as status codes,
the launch plan that scount_plan.py runs has the edges the GPU tests sit on, and `pgen-hip sample-counts` parses its flags, refuses what it
cannot do, prints zeros without a device when nothing is kept and needs a GPU for real counts."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import scount_plan as SP
from helpers import GOLDEN
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
HEADER = b"#IID\tHOM_REF_CT\tHET_CT\tHOM_ALT_CT\tMISSING_CT\n"


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.fixture()
def tiny(tmp_path):
    """basic1's metadata with a small all-zero fixed-width .pgen behind it (the records are never read without a GPU)."""
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", tmp_path / f"basic1.{ext}")
    n, v = 2504, 17784
    (tmp_path / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + bytes(v * 626))
    return tmp_path / "basic1"


@pytest.mark.parametrize("sym", ["pgenhip_sample_counts", "pgenhip_sample_counts_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_sample_counts(None, None, 0, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_counts(None, None, 1, None, 5, None, _capi.SCOUNT_ROWS | _capi.SCOUNT_ACCUMULATE) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_counts_at(None, None, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_counts_at(None, None, None, 3, None, _capi.SCOUNT_AUTO) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()


def test_flag_ids_are_distinct():
    shapes = {_capi.SCOUNT_AUTO, _capi.SCOUNT_ROWS}
    assert len(shapes) == 2 and _capi.SCOUNT_AUTO == 0
    assert all(s & ~_capi.SCOUNT_SHAPE_MASK == 0 for s in shapes)
    assert _capi.SCOUNT_ACCUMULATE & _capi.SCOUNT_SHAPE_MASK == 0
    assert (SP.AUTO, SP.ROWS, SP.ACCUMULATE) == (_capi.SCOUNT_AUTO, _capi.SCOUNT_ROWS, _capi.SCOUNT_ACCUMULATE)


def test_plan_mirror_matches_the_source():
    """scount_plan.py runs gt_scount.hip's launch plan (csrc/launch_plan.h); these are the values the GPU tests are placed around."""
    assert SP.WINDOW_BATCHES == (1 << 8) - 1 and SP.THREADS == 256 and SP.BATCH == 8
    # a flush window fits a counter, and its last batch is the first to need the top hi plane
    assert SP.HI_BITS == 8 and SP.counter_capacity() == 2047
    assert SP.BATCH * SP.WINDOW_BATCHES <= SP.counter_capacity()
    assert SP.hi_planes(SP.WINDOW_BATCHES) == SP.HI_BITS
    assert [SP.hi_planes(b) for b in (0, 1, 2, 3, 4, 127, 128, 255)] == [1, 1, 2, 2, 3, 7, 8, 8]
    assert [SP.lanes_per_row(n) for n in (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    assert [SP.tiles(n) for n in (4096, 4097, 8192, 8193, 500_000)] == [1, 2, 2, 3, 123]


def test_header_documents_the_contract():
    h = (REPO / "include" / "pgen_hip.h").read_text()
    assert re.search(r"#define PGENHIP_SCOUNT_ACCUMULATE 0x10u", h)
    assert "PGENHIP_ABI_VERSION 2u" in h
    assert "d_counts[4*k + c]" in h


def test_sample_counts_in_usage():
    p = run("help")
    assert p.returncode == 0 and b"sample-counts" in p.stdout
    for col in (b"IID", b"HOM_REF_CT", b"HET_CT", b"HOM_ALT_CT", b"MISSING_CT", b".scount"):
        assert col in p.stdout, col


@pytest.mark.parametrize("args", [[], ["--bogus"], ["a", "b"], ["--include-var"], ["x", "-q"], ["x", "--dry-run"], ["x", "--out"]])
def test_usage_errors_exit_2(args):
    p = run("sample-counts", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_zero_kept_variants_prints_zero_lines_without_gpu(tiny):
    p = run("sample-counts", str(tiny), "--include-var", 'ID == "nothing"')
    assert p.returncode == 0, p.stderr
    lines = p.stdout.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b""
    body = lines[1:-1]
    iids = [row.split(b"\t")[0] for row in (GOLDEN / "basic1" / "basic1.psam").read_bytes().split(b"\n")[1:] if row]
    assert len(body) == 2504
    assert body == [iid + b"\t0\t0\t0\t0" for iid in iids]


def test_zero_kept_samples_prints_the_header_alone(tiny):
    p = run("sample-counts", str(tiny), "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0, p.stderr
    assert p.stdout == HEADER


def test_psam_without_iid_exits_101(tmp_path):
    (tmp_path / "t.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n1\t10\tv0\tA\tG\n")
    (tmp_path / "t.psam").write_bytes(b"#FID\tSEX\nS0\tNA\n")
    (tmp_path / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + b"\x40\x00")
    p = run("sample-counts", str(tmp_path / "t"))
    assert p.returncode == 101 and b"IID not among the headers" in p.stderr, p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101(tiny):
    p = run("sample-counts", str(tiny), "--include-var", 'ALT == "G"')
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
