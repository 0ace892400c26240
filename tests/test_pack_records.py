"""CPU leg of the packed-record export: the numpy reference (tests/pack_ref.py) against the oracle on every golden case, the ABI's
refusals without a device, and what `pgen-hip export` does without one (usage errors, the input-prefix refusal, empty selections)."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import pack_ref as PR
import pgen_oracle as oracle
from helpers import GOLDEN, case_names, load_case
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
N, V, R = 2504, 17784, 626


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=120, cwd=cwd)


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_reference_round_trips_through_the_oracle(name):
    """GT text of the packed K-sample records with all samples kept == the case's GT text of the kept samples."""
    v, n, recs, kept, gt = load_case(name)
    packed = PR.pack(recs, n, kept)
    k = n if kept is None else int(kept.size)
    assert packed.shape == (v, (k + 3) // 4)
    if k % 4:
        assert not (packed[:, -1] >> (2 * (k % 4))).any()
    assert oracle.decode_emit(packed, v, k).tobytes() == gt.tobytes()


def test_reference_map_and_pad():
    recs = oracle.synth_records(13, 5, dirty_pad=True).reshape(5, 4)
    ident = PR.pack(recs, 13)
    assert (ident[:, :3] == recs[:, :3]).all() and (ident[:, 3] == (recs[:, 3] & 0x03)).all()
    assert (PR.pack(recs, 13, code_map=(3, 3, 3, 3)) == np.array([0xFF, 0xFF, 0xFF, 0x03], dtype=np.uint8)).all()
    bed = PR.unpack(PR.pack(recs, 13, code_map=PR.BED_MAP), 13)
    assert (bed == np.array(PR.BED_MAP)[PR.unpack(recs, 13)]).all()


# ---- the ABI without a device -------------------------------------------------------------------------------------------
def test_constants_and_wrapper():
    import pgen_rs_amd.engine as E

    assert (_capi.PACK_AUTO, _capi.PACK_GENERAL, _capi.PACK_DENSE, _capi.PACK_GATHER) == (0, 1, 2, 3)
    assert _capi.KNOB_PACK_BLOCKS == 20
    assert E.BED_CODE_MAP == PR.BED_MAP
    for name in ("pack_records", "pack_records_at", "packed_record_size"):
        assert hasattr(E.GtEngine, name)


def test_null_ctx_is_refused():
    lib = _capi.lib
    assert lib.pgenhip_packed_record_size(None) == 0
    assert lib.pgenhip_pack_records(None, None, 0, None, 0, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pack_records(None, None, 1, None, 5, None, 8, None, _capi.PACK_DENSE) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pack_records_at(None, None, None, 0, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pack_records_at(None, None, None, 3, None, 0, None, _capi.PACK_GENERAL) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_PACK_BLOCKS, 2) == _capi.ERR_BAD_ARG


def test_new_kernels_stay_off_the_environment_and_the_oracle():
    for p in (REPO / "pgen_rs_amd" / "csrc" / "gt_pack.hip", REPO / "pgen_rs_amd" / "host" / "pfile.cpp", REPO / "pgen_rs_amd" / "host" / "commands.cpp", REPO / "pgen_rs_amd" / "host" / "assoc.cpp",
              REPO / "pgen_rs_amd" / "host" / "cli.cpp"):
        text = p.read_text()
        assert "getenv" not in text and "pgen_oracle" not in text and "pgo_" not in text, p


# ---- the CLI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basic1(tmp_path_factory):
    """basic1's metadata with synthetic records behind it, as tests/test_host_cli_matrix_gpu.py builds them."""
    d = tmp_path_factory.mktemp("basic1x")
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", d / f"basic1.{ext}")
    recs = oracle.synth_records(N, V)
    (d / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    return d / "basic1"


def test_export_in_usage():
    p = run("help")
    assert p.returncode == 0
    for word in (b"export", b"--format pgen|bed", b"<OUT_PREFIX>", b"no byte parity with plink2"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args,msg", [
    ([], b"<PFILE_PREFIX>"),
    (["-o", "x"], b"<PFILE_PREFIX>"),
    (["x"], b"--out <OUT_PREFIX>"),
    (["x", "--format", "bed"], b"--out <OUT_PREFIX>"),
    (["x", "-o", "y", "--format", "vcf"], b"invalid value 'vcf' for '--format <FORMAT>'"),
    (["x", "-o", "y", "--format"], b"a value is required for '--format'"),
    (["x", "-o", "y", "--bogus"], b"unexpected argument '--bogus'"),
    (["a", "b", "-o", "y"], b"<PFILE_PREFIX>"),
])
def test_usage_errors_exit_2(args, msg, tmp_path):
    p = run("export", *args, cwd=tmp_path)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr and msg in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())


def test_export_onto_the_input_prefix_is_refused(basic1, tmp_path):
    before = {p.name: p.stat().st_size for p in basic1.parent.iterdir()}
    link = tmp_path / "alias"
    os.symlink(basic1.parent, link)
    for out in (str(basic1), str(basic1.parent / "." / "basic1"), str(link / "basic1")):
        p = run("export", str(basic1), "--include-var", 'ID == "nothing"', "-o", out)
        assert p.returncode == 101 and b"overwrite its input" in p.stderr, (out, p.stderr)
    assert {p.name: p.stat().st_size for p in basic1.parent.iterdir()} == before


def _meta(path: Path):
    """-> (bytes up to and including the column-header line, the rows as lists of fields)"""
    lines = path.read_bytes().splitlines(keepends=True)
    n_head = max(i for i, l in enumerate(lines) if l.startswith(b"#")) + 1
    return b"".join(lines[:n_head]), [l.rstrip(b"\n").split(b"\t") for l in lines[n_head:]]


def test_no_kept_variant_writes_the_header_alone_without_gpu(basic1, tmp_path):
    out = tmp_path / "o"
    p = run("export", str(basic1), "--include-var", 'ID == "nothing"', "-o", str(out), "--stats")
    assert p.returncode == 0, p.stderr
    assert b'"variants_kept": 0' in p.stderr
    assert out.with_suffix(".pgen").read_bytes() == PR.pgen_file(np.zeros((0, R), dtype=np.uint8), N)
    assert out.with_suffix(".pvar").read_bytes() == _meta(basic1.with_suffix(".pvar"))[0]
    assert out.with_suffix(".psam").read_bytes() == basic1.with_suffix(".psam").read_bytes()
    p = run("export", str(basic1), "--include-var", 'ID == "nothing"', "-o", str(out), "--format", "bed")
    assert p.returncode == 0, p.stderr
    assert out.with_suffix(".bed").read_bytes() == b"\x6c\x1b\x01"
    assert out.with_suffix(".bim").read_bytes() == b""
    assert len(out.with_suffix(".fam").read_bytes().splitlines()) == N


def test_no_kept_sample_writes_empty_records_without_gpu(basic1, tmp_path):
    out = tmp_path / "o"
    p = run("export", str(basic1), "--include-sam", 'IID == "nobody"', "--include-var", 'ALT == "G"', "-o", str(out))
    assert p.returncode == 0, p.stderr
    head, rows = _meta(basic1.with_suffix(".pvar"))
    cols = head.splitlines()[-1].lstrip(b"#").split(b"\t")
    kept = [r for r in rows if r[cols.index(b"ALT")] == b"G"]
    assert 100 < len(kept) < V
    assert out.with_suffix(".pgen").read_bytes() == PR.pgen_file(np.zeros((len(kept), 0), dtype=np.uint8), 0)
    assert out.with_suffix(".pvar").read_bytes() == head + b"".join(b"\t".join(r) + b"\n" for r in kept)
    assert out.with_suffix(".psam").read_bytes() == _meta(basic1.with_suffix(".psam"))[0]
    p = run("export", str(basic1), "--include-sam", 'IID == "nobody"', "--include-var", 'ALT == "G"', "-o", str(out), "--format", "bed")
    assert p.returncode == 0, p.stderr
    assert out.with_suffix(".bed").read_bytes() == b"\x6c\x1b\x01"
    assert out.with_suffix(".fam").read_bytes() == b""
    c = {name: cols.index(name) for name in (b"CHROM", b"ID", b"POS", b"ALT", b"REF")}
    assert out.with_suffix(".bim").read_bytes() == b"".join(
        b"\t".join([r[c[b"CHROM"]], r[c[b"ID"]], b"0", r[c[b"POS"]], r[c[b"ALT"]], r[c[b"REF"]]]) + b"\n" for r in kept)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101_and_leaves_no_file(basic1, tmp_path):
    p = run("export", str(basic1), "--include-var", 'ALT == "G"', "-o", str(tmp_path / "o"))
    assert p.returncode == 101, p.stderr
    assert b"device" in p.stderr.lower()
    assert not list(tmp_path.iterdir())
