"""Pairwise sample tables — CPU leg: the reference (tests/spair_ref.py) against a per-pair Python loop and the oracle's counts, the
transpose identity, the two C ABI symbols and their NULL-ctx refusal, the constants, the kernel constants the GPU tests place
their sizes around, and `pgen-hip kinship` without a device."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import launch_plan as LP
import pgen_oracle as oracle
import spair_ref as XR
from helpers import GOLDEN
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
SRC = REPO / "pgen_rs_amd" / "csrc" / "gt_spair.hip"
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
KIN_HEADER = b"#IID1\tIID2\tN\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP\n"
KIN_HEADER_COUNTS = KIN_HEADER[:-1] + b"".join(b"\tT%d%d" % (x, y) for x in range(4) for y in range(4)) + b"\n"


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    v = int(rng.integers(0, 12))
    recs = rng.integers(0, 256, size=(v, XR.rsize(n)), dtype=np.uint8)
    kept = None if seed % 3 == 0 else sorted(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).tolist())
    return n, v, recs, kept


@pytest.mark.parametrize("seed", range(12))
def test_reference_agrees_with_a_per_pair_loop(seed):
    n, v, recs, kept = random_case(seed)
    codes = XR.unpack(recs, n, kept)
    k = codes.shape[1]
    t = XR.pair_tables(codes)
    assert t.shape == (k, k, 4, 4) and t.dtype == np.int64
    for a in range(k):
        for b in range(k):
            assert (t[a, b] == XR.table_loop(codes, a, b)).all()
        assert (t[a, a] == np.diag(np.diag(t[a, a]))).all(), "T(a, a) is diagonal"
    assert (t.sum(axis=(2, 3)) == v).all()
    # ranges, either order, overlapping
    if k >= 3:
        a, b = (1, k - 1), (0, 2)
        assert (XR.ranges(codes, a, b) == t[1:, :2]).all() and (XR.ranges(codes, b, a) == t[:2, 1:]).all()


@pytest.mark.parametrize("seed", range(12))
def test_marginals_are_the_oracles_per_sample_counts(seed):
    n, v, recs, kept = random_case(seed)
    codes = XR.unpack(recs, n, kept)
    idx = list(range(n)) if kept is None else kept
    t = XR.pair_tables(codes)
    for r, s in enumerate(idx):
        # the oracle's per-variant counts with only sample s kept, summed over the variants: that sample's counts
        per = oracle.genotype_counts(recs.reshape(-1), v, n, [s]).reshape(v, 4).sum(axis=0) if v else np.zeros(4, dtype=np.int64)
        assert (t[r, :, :, :].sum(axis=2) == per[None, :]).all(), "sums over y are a's counts"
        assert (t[:, r, :, :].sum(axis=1) == per[None, :]).all(), "sums over x are b's counts"


@pytest.mark.parametrize("seed", range(6))
def test_transpose_identity(seed):
    n, v, recs, kept = random_case(seed + 100)
    codes = XR.unpack(recs, n, kept)
    t = XR.pair_tables(codes)
    assert (t.transpose(1, 0, 3, 2) == t).all()


def test_kinship_reference_values():
    same = np.diag([50, 30, 20, 7])                                     # a sample against itself: kinship 0.5
    assert XR.kinship(same) == (100, 30, 0, 30, 30, 0.5)
    t = np.array([[40, 10, 2, 1], [8, 20, 3, 0], [1, 4, 12, 2], [3, 0, 1, 9]])
    n, hethet, ibs0, het1, het2 = 100, 20, 3, 31, 34                    # by hand from the 3 x 3 corner
    assert XR.kinship(t) == (n, hethet, ibs0, het1, het2, 0.5 - (het1 + het2 - 2 * hethet + 4 * ibs0) / (4 * het1))
    nohet = np.zeros((4, 4), dtype=np.int64)
    nohet[0, 0], nohet[0, 1], nohet[3, 1] = 5, 7, 2
    assert XR.kinship(nohet)[:5] == (12, 0, 0, 0, 7) and np.isnan(XR.kinship(nohet)[5])


@pytest.mark.parametrize("sym", ["pgenhip_sample_pair_stats", "pgenhip_sample_pair_stats_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_sample_pair_stats(None, None, 0, None, 0, 0, 0, 0, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_pair_stats(None, None, 75, None, 9, 0, 4, 2, 4, None, _capi.SPAIR_MFMA | _capi.SPAIR_ACCUMULATE) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_pair_stats_at(None, None, None, 0, 0, 0, 0, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_pair_stats_at(None, None, None, 5, 0, 2, 0, 2, None, _capi.SPAIR_GENERAL) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_SPAIR_SLICES, 3) == _capi.ERR_BAD_ARG


def test_constants_and_header():
    assert (_capi.SPAIR_AUTO, _capi.SPAIR_GENERAL, _capi.SPAIR_MFMA, _capi.SPAIR_SHAPE_MASK, _capi.SPAIR_ACCUMULATE) == (0, 1, 2, 0xF, 0x10)
    assert _capi.KNOB_SPAIR_SLICES == 22
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for text in ("#define PGENHIP_SPAIR_AUTO 0u", "#define PGENHIP_SPAIR_GENERAL 1u", "#define PGENHIP_SPAIR_MFMA 2u",
                 "#define PGENHIP_SPAIR_SHAPE_MASK 0xFu", "#define PGENHIP_SPAIR_ACCUMULATE 0x10u", "PGENHIP_KNOB_SPAIR_SLICES = 22",
                 "PGENHIP_ABI_VERSION 2u", "d_out[16 * (i * b_count + l) + 4 * x + y]", "do not count against PGENHIP_LAUNCHES_IN_FLIGHT"):
        assert text in h, text


def test_kernel_constants_the_gpu_tests_rely_on():
    """tests/test_sample_pair_stats_gpu.py places its N and V around these (csrc/launch_plan.h, run through tests/launch_plan.py)."""
    assert (LP.CONST["spair.kThreads"], LP.CONST["spair.kTile"], LP.CONST["spair.kStepRows"]) == (256, 64, 64)
    assert "__builtin_amdgcn_mfma_i32_16x16x64_i8(" in SRC.read_text()


# ---- `pgen-hip kinship` without a device ----

def run_cli(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.fixture()
def tiny(tmp_path):
    """basic1's metadata with a small all-zero fixed-width .pgen behind it (the records are never read without a GPU)."""
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", tmp_path / f"basic1.{ext}")
    n, v = 2504, 17784
    (tmp_path / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + bytes(v * 626))
    return tmp_path / "basic1"


def test_kinship_in_usage():
    p = run_cli("help")
    assert p.returncode == 0
    for word in (b"kinship ", b"--min-kinship", b"--counts", b"--sample-tile", b"IID1", b"HETHET", b"IBS0", b"KINSHIP", b"KING-robust",
                 b"out-of-core sample tiling is not built", b".kin0"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["--bogus"], ["x", "y"], ["x", "--min-kinship"], ["x", "--min-kinship", "abc"], ["x", "--min-kinship", "nan"],
                                  ["x", "--min-kinship", ""], ["x", "--sample-tile", "0"], ["x", "--sample-tile", "-4"], ["x", "--sample-tile", "t"],
                                  ["x", "--window", "5"], ["x", "--counts", "--out"], ["x", "--block-rows", "0"]])
def test_kinship_usage_errors_exit_2(args):
    p = run_cli("kinship", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_kinship_missing_prefix_exits_101(tmp_path):
    p = run_cli("kinship", str(tmp_path / "absent"))
    assert p.returncode == 101, p.stderr


def test_kinship_without_a_pair_or_a_variant_needs_no_device(tiny):
    p = run_cli("kinship", str(tiny), "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0 and p.stdout == KIN_HEADER, p.stderr
    p = run_cli("kinship", str(tiny), "--include-sam", 'IID == "HG00096"', "--counts")
    assert p.returncode == 0 and p.stdout == KIN_HEADER_COUNTS, p.stderr
    # two samples and no variant: one line of zeros, kinship nan; --min-kinship drops it
    two = 'IID == "HG00096" || IID == "HG00097"'
    p = run_cli("kinship", str(tiny), "--include-sam", two, "--include-var", 'ID == "nothing"')
    assert p.returncode == 0 and p.stdout == KIN_HEADER + b"HG00096\tHG00097\t0\t0\t0\t0\t0\tnan\n", p.stderr
    p = run_cli("kinship", str(tiny), "--include-sam", two, "--include-var", 'ID == "nothing"', "--min-kinship", "-10", "--counts")
    assert p.returncode == 0 and p.stdout == KIN_HEADER_COUNTS, p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_kinship_without_gpu_exits_101(tiny):
    p = run_cli("kinship", str(tiny), "--include-var", 'ALT == "G"')
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
