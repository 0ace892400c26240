"""Sample Gram matrix — CPU leg: the two C ABI symbols, constants and header lines, the NULL-ctx refusals, the kernel constants the
GPU tests place their sizes around, the reference (tests/gram_ref.py) against a per-pair loop, against counts from the oracle's GT
text and against the pair tables' reference, the committed GRM fileset with the two reference formulations side by side, and
`pgen-hip grm` without a device."""
import ctypes as C
import json
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import gram_plan as GP
import gram_ref as GR
import spair_ref as XR
from helpers import GOLDEN, case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
SRC = REPO / "pgen_rs_amd" / "csrc" / "gt_gram.hip"
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
GRM = GOLDEN / "grm"
REF_DISAGREEMENT = GR.REF_DISAGREEMENT


# ---- ABI surface ----

@pytest.mark.parametrize("sym", ["pgenhip_sample_gram", "pgenhip_sample_gram_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_sample_gram(None, None, 0, None, 0, None, 0, 0, 0, 0, None, 0, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_gram(None, None, 75, None, 9, None, 0, 4, 2, 4, None, 4, _capi.GRAM_MFMA | _capi.GRAM_ACCUMULATE) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_gram_at(None, None, None, 0, None, 0, 0, 0, 0, None, 0, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_sample_gram_at(None, None, None, 5, None, 0, 2, 0, 2, None, 2, _capi.GRAM_GENERAL) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_GRAM_SLICES, 3) == _capi.ERR_BAD_ARG


def test_constants_and_header():
    assert (_capi.GRAM_AUTO, _capi.GRAM_GENERAL, _capi.GRAM_MFMA, _capi.GRAM_SHAPE_MASK, _capi.GRAM_ACCUMULATE) == (0, 1, 2, 0xF, 0x10)
    assert _capi.KNOB_GRAM_SLICES == 25
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for text in ("#define PGENHIP_GRAM_AUTO 0u", "#define PGENHIP_GRAM_GENERAL 1u", "#define PGENHIP_GRAM_MFMA 2u",
                 "#define PGENHIP_GRAM_SHAPE_MASK 0xFu", "#define PGENHIP_GRAM_ACCUMULATE 0x10u", "PGENHIP_KNOB_GRAM_SLICES = 25",
                 "PGENHIP_ABI_VERSION 2u", "d_out[i * out_stride + l]", "(n_variants + 2) * 2^-53", "ORDINARY device memory",
                 "3u is reserved"):
        assert text in h, text


def test_kernel_constants_the_gpu_tests_rely_on():
    """tests/test_sample_gram_gpu.py places its N and V around these (tests/gram_plan.py runs csrc/launch_plan.h for them)."""
    assert (GP.THREADS, GP.TILE, GP.STEP_ROWS, GP.GROUP_ROWS, GP.MIN_SLICE_ROWS) == (256, 64, 32, 4, 256)
    assert (GP.MAX_GRID_TILES, GP.MAX_GRID_BLOCKS) == (1 << 20, 1 << 22)
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64(" in SRC.read_text()
    assert GP.mfma_slices(1000, 70, 70, forced=7) == 7 and GP.mfma_slices(33, 70, 70, forced=7) == 2 and GP.mfma_slices(5, 70, 70) == 1
    assert GP.general_slices(1000, 70, 70, forced=7) == 7 and GP.general_slices(5, 70, 70, forced=7) == 5 and GP.general_slices(75, 130, 70) == 1


# ---- the reference ----

def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    v = int(rng.integers(0, 12))
    recs = rng.integers(0, 256, size=(v, GR.rsize(n)), dtype=np.uint8)
    kept = None if seed % 3 == 0 else sorted(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).tolist())
    return n, v, recs, kept, rng.integers(-8, 9, size=(v, 4)).astype(np.float64)


def gram_loop(codes, t, a, b):
    return math.fsum(float(t[j, codes[j, a]]) * float(t[j, codes[j, b]]) for j in range(codes.shape[0]))


@pytest.mark.parametrize("seed", range(12))
def test_reference_agrees_with_a_per_pair_loop(seed):
    n, v, recs, kept, t = random_case(seed)
    codes = GR.unpack(recs, n, kept)
    k = codes.shape[1]
    g = GR.gram_ref(codes, t)
    assert g.shape == (k, k) and g.dtype == np.float64
    for a in range(k):
        for b in range(k):
            assert g[a, b] == gram_loop(codes, t, a, b)
    assert np.array_equal(g, g.T) and np.array_equal(GR.gram_fsum(codes, t), g)
    assert (GR.gram_abs(codes, t) >= np.abs(g)).all()
    if k >= 3:   # ranges, either order
        assert np.array_equal(GR.gram_ref(codes[:, 1:], t, codes[:, :2]), g[1:, :2])
        assert np.array_equal(GR.gram_ref(codes[:, :2], t, codes[:, 1:]), g[:2, 1:])


def codes_of_gt_text(gt, v, k):
    """The oracle's GT text of a golden case ("\\tA/B" per kept sample, a newline per row) -> (V, K) codes."""
    cells = gt.reshape(v, 4 * k + 1)[:, :-1].reshape(v, k, 4)
    pair = cells[:, :, 1].astype(np.int32) * 256 + cells[:, :, 3]
    lut = {ord("0") * 256 + ord("0"): 0, ord("0") * 256 + ord("1"): 1, ord("1") * 256 + ord("1"): 2, ord(".") * 256 + ord("."): 3}
    return np.vectorize(lut.__getitem__, otypes=[np.int64])(pair) if pair.size else np.zeros((v, k), dtype=np.int64)


@pytest.mark.parametrize("name", [c for c in case_names() if c != "sub_k0"])
def test_called_in_both_against_the_oracles_gt_text(name):
    """Table (1, 1, 1, 0): the number of rows called in both samples, counted from the committed GT text of the golden cases."""
    v, n, recs, kept, gt = load_case(name)
    k = n if kept is None else len(kept)
    text = codes_of_gt_text(gt, v, k)
    codes = GR.unpack(recs, n, None if kept is None else kept.tolist())
    assert np.array_equal(codes, text)
    hi = min(k, 70)   # the first ranks of the wide cases
    called = (text[:, :hi] < 3).astype(np.int64)
    got = GR.gram_ref(codes[:, :hi], np.tile([1.0, 1.0, 1.0, 0.0], (v, 1)))
    assert np.array_equal(got, (called.T @ called).astype(np.float64))


@pytest.mark.parametrize("seed", range(6))
def test_dosage_products_against_the_pair_tables_reference(seed):
    """Table (0, 1, 2, 0): sum over x, y of x * y * T[x][y] over the called cells of spair_ref's tables."""
    n, v, recs, kept, _ = random_case(seed + 50)
    codes = GR.unpack(recs, n, kept)
    tables = XR.pair_tables(codes)
    w = np.array([0, 1, 2, 0], dtype=np.int64)
    want = (tables * (w[:, None] * w[None, :])[None, None]).sum(axis=(2, 3))
    assert np.array_equal(GR.gram_ref(codes, np.tile([0.0, 1.0, 2.0, 0.0], (v, 1))), want.astype(np.float64))


def test_grm_tables_by_hand():
    tg, tn, skipped = GR.grm_tables([[6, 3, 1, 2], [10, 0, 0, 0], [0, 0, 7, 1], [0, 0, 0, 9], [0, 4, 0, 0]])
    p = 5 / 20
    s = 1 / math.sqrt(2 * p * (1 - p))
    assert tg[0].tolist() == [(0 - 2 * p) * s, (1 - 2 * p) * s, (2 - 2 * p) * s, 0.0] and tn[0].tolist() == [1, 1, 1, 0]
    assert skipped == 3 and not tg[1:4].any() and not tn[1:4].any()
    assert tg[4].tolist() == [-1 / math.sqrt(0.5), 0.0, 1 / math.sqrt(0.5), 0.0]   # p = 1/2


def golden_codes():
    raw = (GRM / "g.pgen").read_bytes()
    v, n = int.from_bytes(raw[3:7], "little"), int.from_bytes(raw[7:11], "little")
    return GR.unpack(np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(v, -1), n)


def test_committed_grm_fileset_and_the_two_formulations():
    codes = golden_codes()
    v, n = codes.shape
    assert (v, n) == (300, 40) and (codes == 3).any() and (np.delete(codes[7], 5) == 0).all() and (codes[150] == 2).all() and (codes[11] == 3).all()
    exp = json.loads((GRM / "expected.json").read_text())
    unhex = lambda m: np.array([[float.fromhex(x) for x in row] for row in m])
    g, cnt, grm = GR.grm_ref(codes)
    tg, _, skipped = GR.grm_tables(GR.variant_counts(codes))
    assert skipped == exp["skipped"] == 3 and exp["ids"] == [f"S{k:03d}" for k in range(n)]
    assert np.array_equal(cnt, np.array(exp["N"], dtype=np.float64))
    # the matrix product's order of additions is the BLAS's: allow the committed values the documented bound
    scale = GR.gram_abs(codes, tg)
    assert (np.abs(g - unhex(exp["G"])) <= (v + 2) * 2.0 ** -53 * scale).all()
    assert (np.abs(grm - unhex(exp["GRM"])) <= (v + 3) * 2.0 ** -53 * scale / cnt).all()
    loop = GR.grm_loop(codes)
    worst = (np.abs(grm - loop) / (scale / cnt)).max()
    print("the two formulations differ by at most", worst, "A / N")
    assert worst <= REF_DISAGREEMENT
    assert abs(np.diag(grm).mean() - 1.0) < 0.2 and abs(grm[~np.eye(n, dtype=bool)].mean()) < 0.1   # unrelated samples


# ---- `pgen-hip grm` without a device ----

def run_cli(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.fixture()
def tiny(tmp_path):
    for ext in ("pgen", "pvar", "psam"):
        shutil.copy(GRM / f"g.{ext}", tmp_path / f"g.{ext}")
    return tmp_path / "g"


def test_grm_in_usage():
    p = run_cli("help")
    assert p.returncode == 0
    for word in (b"  grm ", b"grm    <PFILE_PREFIX>", b"--format grm-bin|rel", b"--sample-tile", b"--block-rows", b".grm.N.bin", b".grm.id", b".rel.id",
                 b"out-of-core", b"no byte or digit parity with plink2 or GCTA"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["--bogus"], ["x"], ["x", "y", "-o", "z"], ["x", "-o"], ["x", "-o", ""], ["x", "-o", "z", "--format", "npy"],
                                  ["x", "-o", "z", "--format"], ["x", "-o", "z", "--sample-tile", "0"], ["x", "-o", "z", "--sample-tile", "-4"],
                                  ["x", "-o", "z", "--sample-tile", "t"], ["x", "-o", "z", "--block-rows", "0"], ["x", "-o", "z", "--counts"]])
def test_grm_usage_errors_exit_2(args):
    p = run_cli("grm", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_grm_missing_prefix_exits_101(tmp_path):
    p = run_cli("grm", str(tmp_path / "absent"), "-o", str(tmp_path / "out"))
    assert p.returncode == 101, p.stderr


def test_grm_without_a_sample_or_a_variant_needs_no_device(tiny, tmp_path):
    out = tmp_path / "none"
    p = run_cli("grm", str(tiny), "--include-sam", 'IID == "nobody"', "-o", str(out))
    assert p.returncode == 0, p.stderr
    assert [Path(f"{out}{ext}").read_bytes() for ext in (".grm.bin", ".grm.N.bin", ".grm.id")] == [b"", b"", b""]
    p = run_cli("grm", str(tiny), "--include-sam", 'IID == "nobody"', "--format", "rel", "-o", str(out))
    assert p.returncode == 0 and Path(f"{out}.rel").read_bytes() == b"" and Path(f"{out}.rel.id").read_bytes() == b"", p.stderr
    # two samples and no variant: N = 0 everywhere, every entry nan
    two = 'IID == "S003" || IID == "S004"'
    p = run_cli("grm", str(tiny), "--include-sam", two, "--include-var", 'ID == "nothing"', "--format", "rel", "-o", str(out), "--stats")
    assert p.returncode == 0 and b'"variants_skipped": 0' in p.stderr, p.stderr
    assert Path(f"{out}.rel").read_bytes() == b"nan\tnan\nnan\tnan\n" and Path(f"{out}.rel.id").read_bytes() == b"S003\nS004\n"
    p = run_cli("grm", str(tiny), "--include-sam", two, "--include-var", 'ID == "nothing"', "-o", str(out))
    assert p.returncode == 0, p.stderr
    assert np.isnan(np.fromfile(f"{out}.grm.bin", dtype="<f4")).all() and np.fromfile(f"{out}.grm.bin", dtype="<f4").size == 3
    assert np.array_equal(np.fromfile(f"{out}.grm.N.bin", dtype="<f4"), np.zeros(3, dtype=np.float32))
    assert Path(f"{out}.grm.id").read_bytes() == b"S003\tS003\nS004\tS004\n"


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_grm_without_gpu_exits_101(tiny, tmp_path):
    p = run_cli("grm", str(tiny), "-o", str(tmp_path / "out"))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
