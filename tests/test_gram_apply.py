"""Gram product — CPU leg: the two C ABI symbols, constants, knob ids and header lines, the NULL-ctx refusals, the plan constants the GPU
tests place their sizes around (tests/gapply_plan.py runs csrc/launch_plan.h for them), the reference (tests/gapply_ref.py) against a
per-sample loop, its int64 and exact forms, and Y against the Gram matrix's reference times Q on every golden case."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import gapply_plan as AP
import gapply_ref as AR
import gram_ref as GR
from helpers import case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
SRC = REPO / "pgen_rs_amd" / "csrc" / "gt_gapply.hip"


# ---- ABI surface ----

@pytest.mark.parametrize("sym", ["pgenhip_gram_apply", "pgenhip_gram_apply_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_gram_apply(None, None, 0, None, 0, None, None, 0, 0, None, None, 0, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_gram_apply(None, None, 75, None, 9, None, None, 4, 4, None, None, 4, _capi.GAPPLY_MFMA | _capi.GAPPLY_ACCUMULATE) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_gram_apply_at(None, None, None, 0, None, None, 0, 0, None, None, 0, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_gram_apply_at(None, None, None, 5, None, None, 2, 2, None, None, 2, _capi.GAPPLY_GENERAL) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_GAPPLY_SAMPLE_SLICES, 3) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_tune(None, _capi.KNOB_GAPPLY_ROW_SLICES, 3) == _capi.ERR_BAD_ARG


def test_constants_and_header():
    assert (_capi.GAPPLY_AUTO, _capi.GAPPLY_GENERAL, _capi.GAPPLY_MFMA, _capi.GAPPLY_SHAPE_MASK, _capi.GAPPLY_ACCUMULATE) == (0, 1, 2, 0xF, 0x10)
    assert _capi.GAPPLY_MAX_COLUMNS == 16
    assert (_capi.KNOB_GAPPLY_SAMPLE_SLICES, _capi.KNOB_GAPPLY_ROW_SLICES) == (26, 27)
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for text in ("#define PGENHIP_GAPPLY_MAX_COLUMNS 16u", "#define PGENHIP_GAPPLY_AUTO 0u", "#define PGENHIP_GAPPLY_GENERAL 1u",
                 "#define PGENHIP_GAPPLY_MFMA 2u", "#define PGENHIP_GAPPLY_SHAPE_MASK 0xFu", "#define PGENHIP_GAPPLY_ACCUMULATE 0x10u",
                 "PGENHIP_KNOB_GAPPLY_SAMPLE_SLICES = 26", "PGENHIP_KNOB_GAPPLY_ROW_SLICES = 27", "PGENHIP_ABI_VERSION 2u",
                 "d_proj[j * n_columns + c]", "d_out[k * out_stride + c]", "(K + 1) * 2^-53", "(n_variants + K + 4) * 2^-53",
                 "ORDINARY device memory"):
        assert text in h, text


def test_plan_constants_the_gpu_tests_rely_on():
    """tests/test_gram_apply_gpu.py places its N, V and slices around these."""
    assert (AP.THREADS, AP.WAVES, AP.GROUP, AP.ROW_TILE, AP.STEP_SAMPLES, AP.SAMPLE_TILE, AP.STEP_ROWS) == (256, 4, 4, 64, 64, 256, 64)
    assert (AP.MIN_SLICE_SAMPLES, AP.MIN_SLICE_ROWS, AP.MAX_GRID_TILES, AP.MAX_GRID_BLOCKS) == (4096, 256, 1 << 20, 1 << 22)
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64(" in SRC.read_text()
    # forced slices are capped at the units of the reduction dimension: no slice is empty
    p = AP.plan(1000, 300, 7, True, 7, 7)
    assert (p.p_tiles, p.y_tiles, p.sample_slices, p.row_slices) == (16, 2, 5, 7)
    assert AP.plan(33, 63, 1, True, 7, 7)[4:] == (1, 1) and AP.plan(65, 65, 1, True, 7, 7)[4:] == (2, 2)
    p = AP.plan(1000, 300, 7, False, 7, 7)
    assert (p.p_tiles, p.y_tiles, p.sample_slices, p.row_slices) == (1750, 9, 5, 7)
    assert AP.plan(5, 300, 16, False, 0, 7).row_slices == 5
    # the two regimes: many short rows fill the chip with row tiles; few long rows split the samples
    chr22, long_rows = AP.plan(1_100_000, 2504, 16, True), AP.plan(1000, 500_000, 16, True)
    assert chr22.sample_slices == 1 and chr22.row_slices > 1 and chr22.y_grid * chr22.row_slices >= 256
    assert long_rows.sample_slices > 1 and long_rows.p_grid * long_rows.sample_slices >= 256 and long_rows.row_slices == 1
    # the sample slices tile [0, K) in whole steps
    for k, s in ((1, 1), (64, 1), (65, 2), (300, 5), (70_001, 7)):
        cuts = [AP.slice_samples(k, i, s) for i in range(s)]
        assert cuts[0][0] == 0 and cuts[-1][1] == k and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert all(b < e and b % AP.STEP_SAMPLES == 0 for b, e in cuts)


# ---- the reference ----

def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    v = int(rng.integers(0, 12))
    c = int(rng.integers(1, 17))
    recs = rng.integers(0, 256, size=(v, GR.rsize(n)), dtype=np.uint8)
    kept = None if seed % 3 == 0 else sorted(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).tolist())
    k = n if kept is None else len(kept)
    return n, v, recs, kept, rng.integers(-8, 9, size=(v, 4)).astype(np.float64), rng.integers(-4, 5, size=(k, c)).astype(np.float64)


@pytest.mark.parametrize("seed", range(12))
def test_reference_agrees_with_a_per_sample_loop(seed):
    n, v, recs, kept, t, q = random_case(seed)
    codes = GR.unpack(recs, n, kept)
    p, y = AR.apply_ref(codes, t, q)
    assert p.shape == (v, q.shape[1]) and y.shape == q.shape and p.dtype == y.dtype == np.float64
    lp, ly = AR.apply_loop(codes, t, q)
    assert np.array_equal(p, lp) and np.array_equal(y, ly)
    ip, iy = AR.apply_int(codes, t, q)
    assert np.array_equal(p, ip.astype(np.float64)) and np.array_equal(y, iy.astype(np.float64))
    ep, ey = AR.apply_exact(codes, t, q)
    assert np.array_equal(p, ep) and np.array_equal(y, ey)
    bp, by = AR.apply_bounds(codes, t, q)
    assert (bp * 2.0 ** 53 >= np.abs(p)).all() and (by * 2.0 ** 53 >= np.abs(y)).all()


def test_exact_form_rounds_once_where_float64_does_not():
    """1 + 2^-60 - 1 over three samples: float64 left to right loses the small term, the exact forms keep it."""
    codes = np.zeros((1, 3), dtype=np.uint8)
    t = np.array([[1.0, 0.0, 0.0, 0.0]])
    q = np.array([[1.0], [2.0 ** -60], [-1.0]])
    p, y = AR.apply_exact(codes, t, q)
    assert p[0, 0] == 2.0 ** -60 and (y == 2.0 ** -60).all()


@pytest.mark.parametrize("name", case_names())
def test_y_is_the_gram_matrix_times_q_on_the_golden_cases(name):
    """Y == gram_ref(...) @ Q in exact integers, on the first ranks of the wide cases."""
    v, n, recs, kept, _ = load_case(name)
    codes = GR.unpack(recs, n, None if kept is None else kept.tolist())[:, :70]
    k = codes.shape[1]
    rng = np.random.default_rng(len(name))
    t = rng.integers(-8, 9, size=(v, 4)).astype(np.float64)
    q = rng.integers(-4, 5, size=(k, 5)).astype(np.float64)
    p, y = AR.apply_ref(codes, t, q)
    assert np.array_equal(y, GR.gram_ref(codes, t) @ q)
    assert np.array_equal(p, GR.z_matrix(codes, t) @ q)


# ---- the numpy twin of `pgen-hip pca` on the committed fileset ----

import json  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

import torch  # noqa: E402

import pca_ref as PR  # noqa: E402
from helpers import GOLDEN  # noqa: E402

CLI = REPO / "pgen_rs_amd" / "pgen-hip"
PCA = GOLDEN / "pca"


def pca_golden_codes():
    raw = (PCA / "p.pgen").read_bytes()
    v, n = int.from_bytes(raw[3:7], "little"), int.from_bytes(raw[7:11], "little")
    return GR.unpack(np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(v, -1), n)


def test_pca_twin_against_eigh_on_the_committed_fileset():
    codes = pca_golden_codes()
    assert codes.shape == (600, 120) and (codes == 3).any()
    exp = json.loads((PCA / "expected.json").read_text())
    m, skipped = PR.m_matrix(codes)
    lam, vec = PR.eigh_ref(m)
    want = np.array([float.fromhex(x) for x in exp["eigenvalues"]])
    assert skipped == exp["skipped"] and np.abs(lam - want).max() <= 120 * 2.0 ** -52 * want[0]   # eigh's own backward error, K ulps of the norm
    gap = min(lam[0] - lam[1], lam[1] - lam[2])
    assert gap >= 0.05 * lam[0]
    tol = 1e-9
    tl, tu, passes, res, converged = PR.twin(m, 2, tol=tol, max_passes=30)
    print(f"twin: {passes} passes, residual {res:.3g}")
    assert converged and passes <= 30
    assert (np.abs(tl - lam[:2]) <= 2 * tol * lam[0]).all()
    ref = np.array([[float.fromhex(x) for x in col] for col in exp["vectors"]]).T
    assert (np.linalg.norm(PR.align(tu, ref) - ref, axis=0) <= 2 * np.sqrt(2) * tol * lam[0] / gap).all()
    # four components reach into the bulk: three passes do not converge, and the twin says so
    assert not PR.twin(m, 4, tol=tol, max_passes=3)[4]


# ---- host linear algebra: a stand-alone program under ASan and UBSan, compared with numpy on the same inputs ----

def _spd_with_repeats(rng, l):
    lam = np.array([3.0, 3.0, 1.0, 1.0, 1.0, 0.5, 0.25, 0.25, 0.0, -1.0, -1.0, 2.0][:l])
    w, _ = np.linalg.qr(rng.standard_normal((l, l)))
    t = (w * lam) @ w.T
    return 0.5 * (t + t.T)


def test_host_linalg_under_sanitizers_against_numpy(tmp_path):
    rng = np.random.default_rng(18)
    deficient = rng.standard_normal((120, 12))
    deficient[:, 5] = deficient[:, 2] - 2.0 * deficient[:, 3]
    deficient[:, 9] = 0.0
    qr_cases = [rng.standard_normal((1, 1)), rng.standard_normal((5, 5)), rng.standard_normal((120, 12)), deficient]
    eig_cases = [np.array([[2.5]]), _spd_with_repeats(rng, 2), _spd_with_repeats(rng, 12)]
    text = ""
    for a in qr_cases:
        text += f"qr {a.shape[0]} {a.shape[1]}\n" + " ".join(repr(float(x)) for x in a.ravel()) + "\n"
    for t in eig_cases:
        text += f"eig {t.shape[0]}\n" + " ".join(repr(float(x)) for x in t.ravel()) + "\n"
    (tmp_path / "cases.txt").write_text(text)
    exe = tmp_path / "linalg_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe),
           str(REPO / "tests" / "linalg_check.cpp"), str(REPO / "pgen_rs_amd" / "host" / "linalg.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert len(lines) == len(qr_cases) + len(eig_cases)
    fro = np.linalg.norm
    for a, ln in zip(qr_cases, lines):
        k, l = a.shape
        q, r = np.linalg.qr(a)
        mine = (float(ln[3]), float(ln[4]))
        numpys = (fro(q.T @ q - np.eye(l)), fro(q @ r - a) / fro(a))
        print(f"qr {k} x {l}: |QtQ - I| = {mine[0]:.3g} (numpy {numpys[0]:.3g}), |QR - A| / |A| = {mine[1]:.3g} (numpy {numpys[1]:.3g})")
        assert ln[:3] == ["qr", str(k), str(l)] and ln[5] == "1"
        for got, ref in zip(mine, numpys):
            assert got <= max(8 * ref, l * 2.0 ** -52)
    for t, ln in zip(eig_cases, lines[len(qr_cases):]):
        l = t.shape[0]
        lam, w = np.linalg.eigh(t)
        mine = (float(ln[2]), float(ln[3]))
        numpys = (fro(w.T @ w - np.eye(l)), fro((w * lam) @ w.T - t) / fro(t))
        print(f"eig {l}: |WtW - I| = {mine[0]:.3g} (numpy {numpys[0]:.3g}), |W L Wt - T| / |T| = {mine[1]:.3g} (numpy {numpys[1]:.3g})")
        assert ln[:2] == ["eig", str(l)] and ln[4] == "1"
        for got, ref in zip(mine, numpys):
            assert got <= max(8 * ref, l * 2.0 ** -52)


# ---- `pgen-hip pca` without a device ----

def run_cli(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120)


@pytest.fixture()
def tiny_pca(tmp_path):
    for ext in ("pgen", "pvar", "psam"):
        shutil.copy(PCA / f"p.{ext}", tmp_path / f"p.{ext}")
    return tmp_path / "p"


def test_pca_in_usage():
    p = run_cli("help")
    assert p.returncode == 0
    for word in (b"  pca ", b"pca    <PFILE_PREFIX>", b"--pcs <P>", b"--tol <X>", b"--max-passes <I>", b"--seed <S>", b"--block-rows <B>", b".eigenval", b".eigenvec",
                 b"plink2 --pca's convention", b"pairwise-complete", b"No digit parity with plink2"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["--bogus"], ["x"], ["x", "y", "-o", "z"], ["x", "-o"], ["x", "-o", ""], ["x", "-o", "z", "--pcs", "0"],
                                  ["x", "-o", "z", "--pcs", "33"], ["x", "-o", "z", "--pcs", "two"], ["x", "-o", "z", "--pcs"], ["x", "-o", "z", "--tol", "-1"],
                                  ["x", "-o", "z", "--tol", "t"], ["x", "-o", "z", "--max-passes", "0"], ["x", "-o", "z", "--seed", "-3"],
                                  ["x", "-o", "z", "--block-rows", "0"], ["x", "-o", "z", "--format", "rel"]])
def test_pca_usage_errors_exit_2(args):
    p = run_cli("pca", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_pca_missing_prefix_exits_101(tmp_path):
    p = run_cli("pca", str(tmp_path / "absent"), "-o", str(tmp_path / "out"))
    assert p.returncode == 101, p.stderr


def test_pca_without_a_sample_or_a_variant_needs_no_device(tiny_pca, tmp_path):
    out = tmp_path / "none"
    p = run_cli("pca", str(tiny_pca), "--include-sam", 'IID == "nobody"', "--pcs", "3", "-o", str(out))
    assert p.returncode == 0, p.stderr
    assert Path(f"{out}.eigenval").read_bytes() == b"" and Path(f"{out}.eigenvec").read_bytes() == b"#IID\tPC1\tPC2\tPC3\n"
    p = run_cli("pca", str(tiny_pca), "--include-var", 'ID == "nothing"', "--pcs", "2", "-o", str(out), "--stats")
    assert p.returncode == 0 and b'"variants_skipped": 0, "passes": 0' in p.stderr and b'"converged": true' in p.stderr, p.stderr
    assert Path(f"{out}.eigenval").read_bytes() == b"" and Path(f"{out}.eigenvec").read_bytes() == b"#IID\tPC1\tPC2\n"


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_pca_without_gpu_exits_101(tiny_pca, tmp_path):
    p = run_cli("pca", str(tiny_pca), "--pcs", "2", "-o", str(tmp_path / "out"))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
