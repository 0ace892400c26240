"""Numeric genotype matrix — CPU leg: the numpy reference (matrix_ref.py) agrees with the GT text of every golden case, the
launch plan that matrix_plan.py runs has the edges the GPU tests sit on, the two C ABI symbols are exported,
bound and refuse a NULL ctx, and `pgen-hip matrix` parses its flags, refuses what it cannot do, writes a zero-dimension .npy
without a device and needs a GPU for a real matrix."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import matrix_plan as MP
import matrix_ref as MR
from helpers import GOLDEN, case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
SRC = REPO / "pgen_rs_amd" / "csrc" / "gt_matrix.hip"


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


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_reference_equals_the_golden_gt_text(name):
    """0/0 -> 0, 0/1 -> 1, 1/1 -> 2, ./. -> 3, field by field, kept lists and K = 0 included."""
    v, n, recs, kept, gt = load_case(name)
    k = n if kept is None else len(kept)
    codes = MR.codes(recs, n, kept)
    assert codes.shape == (v, k)
    assert (codes == MR.gt_text_codes(gt, v, k)).all()
    for dt in (np.int8, np.float16, np.float32):
        vals = MR.default_values(dt)
        m = MR.matrix(recs, n, kept, vals)
        assert m.dtype == dt and m.shape == (v, k)
        assert (MR.raw(MR.matrix(recs, n, kept, vals, sample_major=True)) == MR.raw(np.ascontiguousarray(m.T))).all()
        assert (MR.raw(m) == MR.raw(vals[codes])).all()


def test_default_values():
    assert MR.default_values(np.int8).tolist() == [0, 1, 2, -1] and MR.default_values(np.uint8).tolist() == [0, 1, 2, 255]
    f = MR.default_values(np.float32)
    assert f[:3].tolist() == [0.0, 1.0, 2.0] and np.isnan(f[3])


# ---- the plan -----------------------------------------------------------------------------------------------------------
def test_mirrored_constants_match_the_source():
    assert (MP.THREADS, MP.BLOCKS_PER_CU, MP.LONG_ROW_BYTES) == (256, 8, 4096)
    assert (MP.TILE_VARIANTS, MP.WAVE_SAMPLES, MP.TILE_SAMPLES, MP.TILE_BLOCKS_PER_CU) == (128, 128, 512, 4)
    assert MP.THREADS // 64 * MP.WAVE_SAMPLES == MP.TILE_SAMPLES and MP.TILE_SAMPLES // 4 == 128   # one line of every record
    hdr = (REPO / "include" / "pgen_hip.h").read_text()
    for name, v in (("AUTO", MP.AUTO), ("GENERAL", MP.GENERAL), ("STREAM", MP.STREAM), ("TILE", MP.TILE)):
        assert re.search(rf"#define PGENHIP_MATRIX_{name} {v}u\b", hdr), name
        assert getattr(_capi, f"MATRIX_{name}") == v
    assert "#define PGENHIP_MATRIX_SHAPE_MASK 0xFu" in hdr and "#define PGENHIP_MATRIX_SAMPLE_MAJOR 0x10u" in hdr
    assert (_capi.MATRIX_SHAPE_MASK, _capi.MATRIX_SAMPLE_MAJOR) == (MP.SHAPE_MASK, MP.SAMPLE_MAJOR)
    assert re.search(rf"PGENHIP_KNOB_MATRIX_BLOCKS = {MP.KNOB_MATRIX_BLOCKS},", hdr) and _capi.KNOB_MATRIX_BLOCKS == MP.KNOB_MATRIX_BLOCKS
    assert "PGENHIP_ABI_VERSION 2u" in hdr


def test_launch_plan_matches_the_source():
    """Device code and dispatch lines that running the plan (matrix_plan.py) cannot show."""
    src = SRC.read_text()
    for line in [
        "for (uint64_t j = blockIdx.y; j < a.n_variants; j += gridDim.y) {",
        "x[r] = stage[(8u * n * (r / n) + n * g + r % n) * 32u + ((8u * wave + q + 4u * g) & 31u)];",
        "const uint64_t band = tile / v_tiles, vt = tile - band * v_tiles;",
    ]:
        assert line in src, line
    capi = (REPO / "pgen_rs_amd" / "csrc" / "capi.hip").read_text()
    body = capi[capi.index("static int decode_matrix_core("):]
    body = body[: body.index("\n}\n")]
    assert "a.kept_idx = all_kept ? nullptr : ctx->d_kept;" in body and "const bool all_kept = !ctx->subset || ctx->identity;" in body


def test_derived_edges():
    """The edges the GPU cells sit on, as derived today (a change here means re-reading the launch code)."""
    assert MP.N_EDGES == [4, 8, 16, 128, 512, 1024, 2048, 4096] and MP.V_EDGES == [16, 128, 256]
    assert MP.stream_long_rows(4096, 1) and not MP.stream_long_rows(4095, 1) and MP.stream_long_rows(1024, 4) and not MP.stream_long_rows(2047, 2)
    assert MP.stream_rows_grid(100_000, 500_000, 1) == (123, 16) and MP.stream_rows_grid(1_103_547, 2504, 4) == (3, 682)
    assert MP.stream_rows_grid(37, 4096, 1, forced=3) == (1, 3) and MP.stream_rows_grid(2, 4096, 1) == (2, 2)
    assert MP.auto_shape(True, False, 1, 7, 300) == MP.STREAM
    assert MP.auto_shape(False, False, 0, 304, 300) == MP.GENERAL and MP.auto_shape(False, True, 0, 128, 300) == MP.GENERAL
    assert MP.auto_shape(True, True, 256, 100_000, 500_000) == MP.TILE       # configs[2], dense pitch: a multiple of 16, not of 128
    assert MP.auto_shape(True, True, 256, 1_103_547, 2504) == MP.GENERAL     # chr22, dense pitch: odd
    assert MP.auto_shape(True, True, 256, 1_103_616, 2504) == MP.TILE        # chr22, padded pitch
    assert MP.auto_shape(True, True, 272, 32, 2504) == MP.TILE and MP.auto_shape(True, True, 257, 32, 2504) == MP.GENERAL
    assert MP.auto_shape(True, True, 256, 33, 1) == MP.TILE                  # one output row: the stride is not used
    assert MP.stream_dense(1, 300, 1, 999) and MP.stream_dense(5, 300, 4, 1200) and not MP.stream_dense(5, 300, 4, 1204)
    assert MP.stream_chunks(37, 300, 1, 0, 300) == 694 and MP.stream_chunks(37, 300, 1, 1, 300) == 694 and MP.stream_chunks(37, 300, 1, 13, 300) == 695
    assert MP.stream_chunks(37, 300, 1, 0, 303) == 37 * 20
    assert MP.tile_counts(128, 512) == (1, 1) and MP.tile_counts(129, 513) == (2, 2) and MP.tile_counts(100_000, 500_000) == (782, 977)
    assert MP.tile_grid(100_000, 500_000) == 1024 and MP.tile_grid(100_000, 500_000, forced=3) == 3 and MP.tile_grid(100, 100) == 1
    assert MP.stream_grid(100_000, 500_000, 4, 0, 2_000_000) == 2048 and MP.general_grid(3, 5) == 1


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["pgenhip_decode_matrix", "pgenhip_decode_matrix_at"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_decode_matrix(None, None, 0, None, 0, None, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_decode_matrix(None, None, 1, None, 5, None, 8, 4, None, _capi.MATRIX_TILE | _capi.MATRIX_SAMPLE_MAJOR) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_decode_matrix_at(None, None, None, 0, None, 0, 1, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_decode_matrix_at(None, None, None, 3, None, 0, 2, None, _capi.MATRIX_GENERAL) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()


def test_wrapper_patterns():
    from pgen_rs_amd import GtEngine

    assert GtEngine.matrix_values(torch.int8).tolist() == [0, 1, 2, 255]
    assert GtEngine.matrix_values(torch.uint8).tolist() == [0, 1, 2, 255]
    assert GtEngine.matrix_values(torch.int16).view(np.int16).tolist() == [0, 1, 2, -1]
    assert GtEngine.matrix_values(torch.int32).view(np.int32).tolist() == [0, 1, 2, -1]
    for dt, nd in ((torch.float16, np.float16), (torch.float32, np.float32)):
        assert (GtEngine.matrix_values(dt) == MR.default_values(nd).view(np.uint8)).all()
    assert GtEngine.matrix_values(torch.bfloat16).view(np.uint16).tolist()[:3] == [0, 0x3F80, 0x4000]
    assert GtEngine.matrix_values(torch.float32, [0.0, 0.5, 1.0, -9.0]).view(np.float32).tolist() == [0.0, 0.5, 1.0, -9.0]
    with pytest.raises(ValueError):
        GtEngine.matrix_values(torch.float64)
    with pytest.raises(ValueError):
        GtEngine.matrix_values(torch.int8, [0, 1, 2])


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def test_matrix_in_usage():
    p = run("help")
    assert p.returncode == 0 and b"matrix" in p.stdout
    for word in (b"--dtype i8|f16|f32", b"--missing", b"--sample-major", b".npy.variants", b".npy.samples"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args,msg", [
    ([], b"<PFILE_PREFIX>"),
    (["-o", "x.npy"], b"<PFILE_PREFIX>"),
    (["x"], b"--out"),
    (["x", "-o", "x.npy", "--dtype", "i16"], b"invalid value 'i16' for '--dtype <DTYPE>'"),
    (["x", "-o", "x.npy", "--dtype"], b"a value is required for '--dtype'"),
    (["x", "-o", "x.npy", "--missing", "128"], b"invalid value '128' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--missing", "-129"], b"invalid value '-129' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--missing", "nan"], b"invalid value 'nan' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--missing", "1.5"], b"invalid value '1.5' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--dtype", "f16", "--missing", "70000"], b"invalid value '70000' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--dtype", "f32", "--missing", "1e39"], b"invalid value '1e39' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--dtype", "f32", "--missing", "abc"], b"invalid value 'abc' for '--missing <X>'"),
    (["x", "-o", "x.npy", "--bogus"], b"unexpected argument '--bogus'"),
    (["a", "b", "-o", "x.npy"], b"<PFILE_PREFIX>"),
])
def test_usage_errors_exit_2(args, msg, tmp_path):
    p = subprocess.run([str(CLI), "matrix", *args], capture_output=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr and msg in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())


def _ids(path, column):
    rows = [r.split(b"\t") for r in path.read_bytes().split(b"\n") if r and not r.startswith(b"##")]
    c = rows[0].index(column) if column in rows[0] else rows[0].index(b"#" + column)
    return [r[c] for r in rows[1:]]


@pytest.mark.parametrize("dtype,descr", [("i8", "|i1"), ("f16", "<f2"), ("f32", "<f4")])
@pytest.mark.parametrize("sample_major", [False, True])
def test_zero_kept_variants_writes_a_zero_dimension_without_gpu(tiny, tmp_path, dtype, descr, sample_major):
    out = tmp_path / "m.npy"
    p = run("matrix", str(tiny), "--include-var", 'ID == "nothing"', "--dtype", dtype, "-o", str(out), *(["--sample-major"] if sample_major else []))
    assert p.returncode == 0, p.stderr
    raw = out.read_bytes()
    assert raw[:8] == b"\x93NUMPY\x01\x00" and len(raw) % 64 == 0 and raw.endswith(b"\n")
    assert f"'descr': '{descr}'".encode() in raw and b"'fortran_order': False" in raw
    a = np.load(out)
    assert a.shape == ((2504, 0) if sample_major else (0, 2504)) and a.dtype == np.dtype(descr)
    assert (tmp_path / "m.npy.variants").read_bytes() == b""
    assert (tmp_path / "m.npy.samples").read_bytes().split(b"\n")[:-1] == _ids(GOLDEN / "basic1" / "basic1.psam", b"IID")


def test_zero_kept_samples_writes_a_zero_dimension_without_gpu(tiny, tmp_path):
    out = tmp_path / "m.npy"
    p = run("matrix", str(tiny), "--include-sam", 'IID == "nobody"', "--include-var", 'ALT == "G"', "-o", str(out))
    assert p.returncode == 0, p.stderr
    a = np.load(out)
    ids = (tmp_path / "m.npy.variants").read_bytes().split(b"\n")[:-1]
    assert a.shape == (len(ids), 0) and a.dtype == np.int8 and len(ids) > 0
    assert (tmp_path / "m.npy.samples").read_bytes() == b""


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101_and_leaves_no_file(tiny, tmp_path):
    out = tmp_path / "m.npy"
    p = run("matrix", str(tiny), "--include-var", 'ALT == "G"', "-o", str(out))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
    assert not list(tmp_path.glob("m.npy*"))
