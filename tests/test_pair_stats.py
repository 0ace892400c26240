"""Windowed pairwise tables — CPU leg: the reference (tests/pair_ref.py) against a per-sample brute-force loop and the oracle's
per-variant counts, the exact r^2 and its single rounding, the two C ABI symbols, the argument errors that need no device, and
the constants the GPU tests take from gt_pair.hip."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import launch_plan as LP
import pair_ref as PR
import pgen_oracle as oracle
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 70))
    v = int(rng.integers(2, 9))
    recs = rng.integers(0, 256, size=(v, PR.rsize(n)), dtype=np.uint8)
    kept = None if seed % 3 == 0 else sorted(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).tolist())
    return n, v, recs, kept


@pytest.mark.parametrize("seed", range(12))
def test_reference_agrees_with_a_per_sample_loop(seed):
    n, v, recs, kept = random_case(seed)
    w = 1 + seed % 4
    n_left = v - seed % 2
    codes = PR.unpack(recs, n, kept)
    got = PR.pair_tables(codes, n_left, w, fill=-1)
    seen = 0
    for i in range(n_left):
        for d in range(1, w + 1):
            if i + d < v:
                assert (got[i, d - 1] == PR.table_brute(recs, n, kept, i, i + d)).all()
                seen += 1
            else:
                assert (got[i, d - 1] == -1).all()
    assert seen == len(PR.pair_list(v, n_left, w))


@pytest.mark.parametrize("seed", range(12))
def test_marginals_are_the_oracles_counts(seed):
    n, v, recs, kept = random_case(seed)
    codes = PR.unpack(recs, n, kept)
    counts = oracle.genotype_counts(recs.reshape(-1), v, n, kept)
    k = n if kept is None else len(kept)
    t = PR.pair_tables(codes, v, v)
    for i, d in PR.pair_list(v, v, v):
        assert (t[i, d - 1].sum(axis=1) == counts[i]).all()
        assert (t[i, d - 1].sum(axis=0) == counts[i + d]).all()
        assert t[i, d - 1].sum() == k


def test_r2_reference_values():
    ident = np.diag([5, 7, 3, 9])
    assert PR.r2_exact(ident) == 1 and PR.r2_f32(ident) == np.float32(1.0)
    anti = np.zeros((4, 4), dtype=np.int64)
    anti[0, 2] = anti[2, 0] = 4
    assert PR.r2_exact(anti) == 1                                      # the sign is squared away
    mono = np.zeros((4, 4), dtype=np.int64)
    mono[1, 0], mono[1, 1], mono[1, 2], mono[0, 3], mono[3, 3] = 3, 4, 5, 8, 2
    assert PR.r2_exact(mono) is None and np.isnan(PR.r2_f32(mono))      # row i monomorphic among the jointly called
    assert np.isnan(PR.r2_f32(np.zeros((4, 4), dtype=np.int64)))        # n == 0
    only_missing = np.zeros((4, 4), dtype=np.int64)
    only_missing[3, :] = 6
    assert np.isnan(PR.r2_f32(only_missing))
    t = np.array([[10, 3, 0, 1], [2, 7, 1, 0], [0, 2, 5, 2], [1, 1, 1, 9]])
    n, sx, sy, sxx, syy, sxy = 30, 24, 24, 38, 36, 33                  # by hand from the 3 x 3 corner
    assert PR.r2_exact(t) == Fraction((n * sxy - sx * sy) ** 2, (n * sxx - sx * sx) * (n * syy - sy * sy))


def test_single_rounding_to_float32():
    for x in [Fraction(1, 3), Fraction(2, 3), Fraction(1, 10), Fraction(123456789, 987654321), Fraction(1), Fraction(0)]:
        f = PR.to_f32_once(x)
        err = abs(Fraction(float(f)) - x)
        for other in (np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(2))):
            assert err <= abs(Fraction(float(other)) - x)
    # a double-rounding trap: just above the midpoint of two float32s, closer than a double resolves from the midpoint
    lo = np.float32(0.5)
    hi = np.nextafter(lo, np.float32(1))
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    assert PR.to_f32_once(mid + Fraction(1, 2 ** 80)) == hi
    assert PR.to_f32_once(mid - Fraction(1, 2 ** 80)) == lo


@pytest.mark.parametrize("sym", ["pgenhip_pair_stats", "pgenhip_pair_stats_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_pair_stats(None, None, 0, None, 0, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pair_stats(None, None, 75, None, 9, 9, 4, None, _capi.PAIR_R2) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pair_stats_at(None, None, None, 0, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pair_stats_at(None, None, None, 5, 5, 2, None, _capi.PAIR_TABLE) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_PAIR_BLOCKS, 3) == _capi.ERR_BAD_ARG


def test_header_documents_the_contract():
    h = (REPO / "include" / "pgen_hip.h").read_text()
    assert re.search(r"#define PGENHIP_PAIR_TABLE 0u", h) and re.search(r"#define PGENHIP_PAIR_R2\s+1u", h)
    assert "PGENHIP_KNOB_PAIR_BLOCKS = 19" in h and _capi.KNOB_PAIR_BLOCKS == 19
    assert (_capi.PAIR_TABLE, _capi.PAIR_R2) == (0, 1)
    assert "PGENHIP_ABI_VERSION 2u" in h
    assert "d_out[16*p + 4*a + b]" in h and "p = i * W + (d - 1)" in h


def test_kernel_constants_the_gpu_tests_rely_on():
    """tests/test_pair_stats_gpu.py places its N, V and W around these (csrc/launch_plan.h, run through tests/launch_plan.py)."""
    assert (LP.CONST["pair.kThreads"], LP.CONST["pair.kTile"], LP.CONST["pair.kChunkWords"]) == (64, 16, 16)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_device_means_no_fallback():
    ctx = C.c_void_p()
    assert _capi.lib.pgenhip_create(C.byref(ctx), 0, 100, None, 0, 0) == _capi.ERR_NO_DEVICE
    assert not ctx.value


# ---- `pgen-hip ld` without a device ----
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
LD_HEADER = b"#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tR2\n"


def run_cli(*args):
    import subprocess

    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.fixture()
def tiny(tmp_path):
    """basic1's metadata with a small all-zero fixed-width .pgen behind it (the records are never read without a GPU)."""
    import shutil

    from helpers import GOLDEN

    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", tmp_path / f"basic1.{ext}")
    n, v = 2504, 17784
    (tmp_path / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + bytes(v * 626))
    return tmp_path / "basic1"


def test_ld_in_usage():
    p = run_cli("help")
    assert p.returncode == 0
    for word in (b"ld ", b"--window", b"--min-r2", b"--counts", b"CHROM_A", b"R2", b"N_OBS"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["x"], ["x", "--window"], ["x", "--window", "0"], ["x", "--window", "-3"], ["x", "--window", "w"],
                                  ["x", "--window", "5", "--min-r2", "2"], ["x", "--window", "5", "--min-r2", "x"],
                                  ["x", "--window", "5", "--bogus"], ["x", "y", "--window", "5"], ["x", "--window", "5", "--block-rows", "0"]])
def test_ld_usage_errors_exit_2(args):
    p = run_cli("ld", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_ld_without_a_pair_prints_the_header_alone_without_gpu(tiny):
    p = run_cli("ld", str(tiny), "--window", "10", "--include-var", 'ID == "nothing"')
    assert p.returncode == 0 and p.stdout == LD_HEADER, p.stderr
    p = run_cli("ld", str(tiny), "--window", "10", "--include-var", 'ID == "rs7815"')
    assert p.returncode == 0 and p.stdout == LD_HEADER, p.stderr
    p = run_cli("ld", str(tiny), "--window", "10", "--include-sam", 'IID == "nobody"', "--counts")
    assert p.returncode == 0 and p.stdout.startswith(LD_HEADER[:-1] + b"\tN_OBS\tT00\tT01") and p.stdout.count(b"\n") == 1, p.stderr


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_ld_without_gpu_exits_101(tiny):
    p = run_cli("ld", str(tiny), "--window", "10", "--include-var", 'ALT == "G"')
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
