"""Per-variant genotype counts — CPU leg: the two C ABI symbols are exported and bound, argument errors come back as
status codes, and `pgen-hip freq` parses its flags, refuses what it cannot do and needs a GPU for the counts."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from helpers import GOLDEN
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"


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


@pytest.mark.parametrize("sym", ["pgenhip_genotype_counts", "pgenhip_genotype_counts_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_genotype_counts(None, None, 0, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_genotype_counts(None, None, 1, None, 5, None, _capi.COUNT_AUTO) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_genotype_counts_at(None, None, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_genotype_counts_at(None, None, None, 3, None, _capi.COUNT_ROWS_PER_WAVE) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()


def test_kernel_ids_are_distinct():
    assert len({_capi.COUNT_AUTO, _capi.COUNT_WAVE_PER_ROW, _capi.COUNT_ROWS_PER_WAVE}) == 3 and _capi.COUNT_AUTO == 0


def test_freq_in_usage():
    p = run("help")
    assert p.returncode == 0 and b"freq" in p.stdout and b"HOM_REF_CT" in p.stdout and b"plink2" in p.stdout


@pytest.mark.parametrize("args", [[], ["--bogus"], ["a", "b"], ["--include-var"], ["x", "-q"], ["x", "--dry-run"]])
def test_freq_usage_errors_exit_2(args):
    p = run("freq", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_freq_missing_pvar_column_exits_101_and_names_it(tmp_path):
    (tmp_path / "t.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\n1\t10\tv0\tA\n")
    (tmp_path / "t.psam").write_bytes(b"#IID\nS0\n")
    (tmp_path / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + b"\x40\x00")
    p = run("freq", str(tmp_path / "t"))
    assert p.returncode == 101 and b"ALT not among the headers" in p.stderr, p.stderr


def test_freq_zero_kept_variants_needs_no_gpu(tiny):
    p = run("freq", str(tiny), "--include-var", 'ID == "nothing"')
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"#CHROM\tPOS\tID\tREF\tALT\tHOM_REF_CT\tHET_REF_ALT_CTS\tTWO_ALT_GENO_CTS\tMISSING_CT\n"


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_freq_without_gpu_exits_101(tiny):
    p = run("freq", str(tiny), "--include-var", 'ALT == "G"')
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
