"""GPU leg of `pgen-hip matrix`: the numeric genotype matrix end to end (metadata filter -> records staged to HBM -> matrix kernels
-> .npy written with pwrite) against numpy on the file's record bytes (tests/matrix_ref.py), with the id lists beside it."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import matrix_ref as MR
import pgen_oracle as oracle
from helpers import GOLDEN
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
DT = {"i8": np.int8, "f16": np.float16, "f32": np.float32}


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def expected(prefix: Path, var_pred=None, sam_pred=None, dtype="i8", missing=None, sample_major=False):
    """-> (matrix, variant ids, sample ids)"""
    _, _, pvar_cols, pvar_rows = read_meta(prefix.with_suffix(".pvar"))
    _, _, psam_cols, psam_rows = read_meta(prefix.with_suffix(".psam"))
    raw = prefix.with_suffix(".pgen").read_bytes()
    if raw[2] == 0x02:
        n = int.from_bytes(raw[7:11], "little")
        offs = None
    else:
        rc, h = oracle.vw_parse_header(raw[:12])
        assert rc == 0
        rc, _types, _lens, offs = oracle.vw_index(h, raw)
        assert rc == 0
        n = int(h.sample_count)
    r = (2 * n + 7) // 8
    keep_v = [i for i, row in enumerate(pvar_rows) if var_pred is None or var_pred(dict(zip(pvar_cols, row)))]
    keep_s = np.array([i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))], dtype=np.int64)
    recs = np.zeros((len(keep_v), r), dtype=np.uint8)
    for j, vi in enumerate(keep_v):
        recs[j] = np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r if offs is None else int(offs[vi]))
    vals = MR.default_values(DT[dtype])
    if missing is not None:
        vals[3] = missing
    m = MR.matrix(recs, n, keep_s, vals, sample_major)
    return m, [pvar_rows[i][pvar_cols.index(b"ID")] for i in keep_v], [psam_rows[i][psam_cols.index(b"IID")] for i in keep_s]


def check(out: Path, want):
    m, vids, sids = want
    raw = out.read_bytes()
    hlen = 10 + int.from_bytes(raw[8:10], "little")
    assert raw[:8] == b"\x93NUMPY\x01\x00" and hlen % 64 == 0 and b"'fortran_order': False" in raw[:hlen]
    a = np.load(out)
    assert a.dtype == m.dtype and a.shape == m.shape
    assert len(raw) == hlen + m.size * m.itemsize
    assert (MR.raw(a) == MR.raw(m)).all()
    assert Path(str(out) + ".variants").read_bytes() == b"".join(v + b"\n" for v in vids)
    assert Path(str(out) + ".samples").read_bytes() == b"".join(s + b"\n" for s in sids)


@pytest.fixture(scope="module")
def basic1(tmp_path_factory):
    d = tmp_path_factory.mktemp("basic1m")
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", d / f"basic1.{ext}")
    n, v = 2504, 17784
    recs = oracle.synth_records(n, v)
    (d / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    return d / "basic1"


VAR = (["--include-var", 'ALT == "G"'], lambda r: r[b"ALT"] == b"G")
SAM = (["--include-sam", 'IID != "HG00097" && IID != "NA20900"'], lambda r: r[b"IID"] not in (b"HG00097", b"NA20900"))
CASES = {
    "neither": ([], None, None),
    "var": (VAR[0], VAR[1], None),
    "sam": (SAM[0], None, SAM[1]),
    "both": (VAR[0] + SAM[0], VAR[1], SAM[1]),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("sample_major", [False, True])
def test_selection_matches_the_reference(basic1, tmp_path, case, sample_major):
    flags, vp, sp = CASES[case]
    out = tmp_path / "m.npy"
    p = run("matrix", str(basic1), *flags, "-o", str(out), "--stats", *(["--sample-major"] if sample_major else []))
    assert p.returncode == 0, p.stderr
    assert b'"variants_kept"' in p.stderr
    check(out, expected(basic1, vp, sp, sample_major=sample_major))


@pytest.mark.parametrize("dtype,missing,value", [("i8", None, None), ("f16", None, None), ("f32", None, None), ("i8", "-9", -9), ("i8", "3", 3),
                                                 ("f16", "-1", -1.0), ("f32", "0.25", 0.25), ("f32", "inf", np.inf), ("f16", "nan", np.nan)])
def test_dtypes_and_missing(basic1, tmp_path, dtype, missing, value):
    out = tmp_path / "m.npy"
    flags = ["--dtype", dtype] + (["--missing=" + missing] if missing is not None else [])
    for sample_major in (False, True):
        p = run("matrix", str(basic1), *VAR[0], *flags, "-o", str(out), *(["--sample-major"] if sample_major else []))
        assert p.returncode == 0, p.stderr
        want = expected(basic1, VAR[1], None, dtype, value, sample_major)
        check(out, want)


def test_sample_major_is_the_transpose(basic1, tmp_path):
    a, b = tmp_path / "a.npy", tmp_path / "b.npy"
    assert run("matrix", str(basic1), *SAM[0], "-o", str(a)).returncode == 0
    assert run("matrix", str(basic1), *SAM[0], "-o", str(b), "--sample-major").returncode == 0
    assert (np.load(a).T == np.load(b)).all()
    assert Path(str(a) + ".variants").read_bytes() == Path(str(b) + ".variants").read_bytes()


@pytest.mark.parametrize("sample_major", [False, True])
def test_shards_and_blocks_give_identical_bytes(basic1, tmp_path, sample_major):
    sm = ["--sample-major"] if sample_major else []
    ref = tmp_path / "ref.npy"
    assert run("matrix", str(basic1), *VAR[0], *SAM[0], "--dtype", "f16", "-o", str(ref), *sm).returncode == 0
    check(ref, expected(basic1, VAR[1], SAM[1], "f16", sample_major=sample_major))
    for extra in (["--shards", "1"], ["--shards", "3"], ["--shards", "7"], ["--block-mib", "1"], ["--shards", "3", "--block-mib", "1"]):
        out = tmp_path / "o.npy"
        p = run("matrix", str(basic1), *VAR[0], *SAM[0], "--dtype", "f16", "-o", str(out), *sm, *extra)
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == ref.read_bytes(), extra


def test_more_shards_than_variants(basic1, tmp_path):
    ids = ("rs2312724", "rs7815")
    out = tmp_path / "m.npy"
    q = " || ".join(f'ID == "{i}"' for i in ids)
    for sm in ([], ["--sample-major"]):
        p = run("matrix", str(basic1), "--include-var", q, "--shards", "7", "-o", str(out), *sm)
        assert p.returncode == 0, p.stderr
        want = expected(basic1, lambda r: r[b"ID"].decode() in ids, sample_major=bool(sm))
        assert want[0].shape == ((2504, 2) if sm else (2, 2504))
        check(out, want)


def test_zero_kept_samples_and_zero_kept_variants(basic1, tmp_path):
    out = tmp_path / "m.npy"
    p = run("matrix", str(basic1), "--include-sam", 'IID == "nobody"', *VAR[0], "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(basic1, VAR[1], lambda r: False))
    assert np.load(out).shape[1] == 0 and np.load(out).shape[0] > 100
    p = run("matrix", str(basic1), "--include-var", 'ID == "nothing"', "-o", str(out), "--sample-major", "--dtype", "f32")
    assert p.returncode == 0, p.stderr
    check(out, expected(basic1, lambda r: False, None, "f32", sample_major=True))
    assert np.load(out).shape == (2504, 0)


@pytest.fixture(scope="module")
def vw_pfile(tmp_path_factory):
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    d = tmp_path_factory.mktemp("vwm")
    n, v = 2504, 3000
    rng = np.random.default_rng(2029)
    types = np.where(rng.random(v) < 0.8, 0, rng.integers(1, 8, size=v)).tolist()
    types[0] = 0
    recs = writer.make_records(rng, n, types)
    data, _ = writer.write_vw(n, recs, 8, 2)
    (d / "vw.pgen").write_bytes(data)
    with open(d / "vw.pvar", "wb") as f:
        f.write(b"#CHROM\tPOS\tID\tREF\tALT\tRTYPE\n")
        f.write(b"".join(b"7\t%d\tv%d\tC\tT\t%d\n" % (500 + 3 * i, i, t) for i, t in enumerate(types)))
    with open(d / "vw.psam", "wb") as f:
        f.write(b"#IID\tSEX\n" + b"".join(b"S%04d\tNA\n" % i for i in range(n)))
    return d / "vw"


def test_variable_width_plain_records(vw_pfile, tmp_path):
    out = tmp_path / "m.npy"
    p = run("matrix", str(vw_pfile), "--include-var", 'RTYPE == "0"', "--block-mib", "1", "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(vw_pfile, lambda r: r[b"RTYPE"] == b"0"))
    p = run("matrix", str(vw_pfile), "--include-var", 'RTYPE == "0" && ID != "v5"', "--include-sam", 'IID != "S0007"', "--shards", "3",
            "--sample-major", "--dtype", "f32", "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(vw_pfile, lambda r: r[b"RTYPE"] == b"0" and r[b"ID"] != b"v5", lambda r: r[b"IID"] != b"S0007", "f32", sample_major=True))


def test_variable_width_compressed_kept_record_exits_101(vw_pfile, tmp_path):
    p = run("matrix", str(vw_pfile), "-o", str(tmp_path / "m.npy"))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr


def test_two_gpus(basic1, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    out = tmp_path / "m.npy"
    p = run("matrix", str(basic1), *VAR[0], "--gpus", "2", "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(basic1, VAR[1]))
