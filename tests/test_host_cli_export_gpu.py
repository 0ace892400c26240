"""GPU leg of `pgen-hip export`: the selection written back as a fileset end to end (metadata filter -> records staged to HBM -> pack
kernels -> records written with pwrite) against numpy on the file's record bytes (tests/pack_ref.py), the metadata files against
the input's text, and the round trip through `filter`."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pack_ref as PR
import pgen_oracle as oracle
from helpers import GOLDEN
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def expected(prefix: Path, var_pred=None, sam_pred=None, bed=False):
    """-> the three files' bytes: (.pgen | .bed, .pvar | .bim, .psam | .fam)"""
    pvar_hdr, pvar_col_line, pvar_cols, pvar_rows = read_meta(prefix.with_suffix(".pvar"))
    psam_hdr, psam_col_line, psam_cols, psam_rows = read_meta(prefix.with_suffix(".psam"))
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
    keep_s = [i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))]
    recs = np.zeros((len(keep_v), r), dtype=np.uint8)
    for j, vi in enumerate(keep_v):
        recs[j] = np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r if offs is None else int(offs[vi]))
    packed = PR.pack(recs, n, keep_s, PR.BED_MAP if bed else None)
    if not bed:
        pvar = pvar_hdr + pvar_col_line + b"\n" + b"".join(b"\t".join(pvar_rows[i]) + b"\n" for i in keep_v)
        psam = psam_hdr + psam_col_line + b"\n" + b"".join(b"\t".join(psam_rows[i]) + b"\n" for i in keep_s)
        return PR.pgen_file(packed, len(keep_s)), pvar, psam
    c = {name: pvar_cols.index(name) for name in (b"CHROM", b"ID", b"POS", b"ALT", b"REF")}
    bim = b"".join(b"\t".join([pvar_rows[i][c[b"CHROM"]], pvar_rows[i][c[b"ID"]], b"0", pvar_rows[i][c[b"POS"]], pvar_rows[i][c[b"ALT"]],
                               pvar_rows[i][c[b"REF"]]]) + b"\n" for i in keep_v)

    def col(row, name):
        return row[psam_cols.index(name)] if name in psam_cols else b"0"

    fam = b"".join(b"\t".join([col(psam_rows[i], b"FID"), col(psam_rows[i], b"IID"), col(psam_rows[i], b"PAT"), col(psam_rows[i], b"MAT"),
                               col(psam_rows[i], b"SEX") if col(psam_rows[i], b"SEX") in (b"1", b"2") else b"0", b"-9"]) + b"\n" for i in keep_s)
    return PR.bed_file(packed), bim, fam


def check(out: Path, want, bed=False):
    exts = (".bed", ".bim", ".fam") if bed else (".pgen", ".pvar", ".psam")
    for ext, w in zip(exts, want):
        got = out.with_suffix(ext).read_bytes()
        assert len(got) == len(w) and got == w, ext


@pytest.fixture(scope="module")
def basic1(tmp_path_factory):
    d = tmp_path_factory.mktemp("basic1e")
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
def test_exported_fileset_matches_the_reference(basic1, tmp_path, case):
    flags, vp, sp = CASES[case]
    out = tmp_path / "o"
    p = run("export", str(basic1), *flags, "-o", str(out), "--stats")
    assert p.returncode == 0, p.stderr
    assert b'"variants_kept"' in p.stderr
    check(out, expected(basic1, vp, sp))


def test_shards_and_blocks_give_identical_bytes(basic1, tmp_path):
    want = expected(basic1, VAR[1], SAM[1])
    for extra in (["--shards", "3"], ["--block-mib", "1"], ["--shards", "3", "--block-mib", "1"], ["--shards", "7"]):
        out = tmp_path / "o"
        p = run("export", str(basic1), *VAR[0], *SAM[0], "-o", str(out), *extra)
        assert p.returncode == 0, p.stderr
        check(out, want)


def test_round_trip_through_filter(basic1, tmp_path):
    out = tmp_path / "o"
    assert run("export", str(basic1), *VAR[0], *SAM[0], "-o", str(out), "--shards", "3").returncode == 0
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    p = run("filter", str(out), "-o", str(a))
    assert p.returncode == 0, p.stderr
    p = run("filter", str(basic1), *VAR[0], *SAM[0], "-o", str(b))
    assert p.returncode == 0, p.stderr
    assert a.stat().st_size > 1 << 20 and a.read_bytes() == b.read_bytes()   # header included
    # and the export of an export is the export
    again = tmp_path / "again"
    assert run("export", str(out), "-o", str(again)).returncode == 0
    for ext in (".pgen", ".pvar", ".psam"):
        assert again.with_suffix(ext).read_bytes() == out.with_suffix(ext).read_bytes(), ext


@pytest.mark.parametrize("case", ["var", "both"])   # basic1 has multiallelic rows: a .bed needs a variant filter that drops them
def test_format_bed(basic1, tmp_path, case):
    flags, vp, sp = CASES[case]
    out = tmp_path / "o"
    p = run("export", str(basic1), *flags, "--format", "bed", "-o", str(out), "--block-mib", "2")
    assert p.returncode == 0, p.stderr
    check(out, expected(basic1, vp, sp, bed=True), bed=True)
    assert not out.with_suffix(".pgen").exists()


def test_format_bed_refuses_a_multiallelic_row_of_basic1(basic1, tmp_path):
    p = run("export", str(basic1), "--format", "bed", "-o", str(tmp_path / "o"))
    assert p.returncode == 101 and b"rs10426061" in p.stderr and b"A,T" in p.stderr, p.stderr
    assert not list(tmp_path.iterdir())


def test_bed_columns_and_multiallelic_refusal(tmp_path):
    n, v = 37, 5
    recs = oracle.synth_records(n, v)
    (tmp_path / "t.pgen").write_bytes(PR.pgen_file(recs.reshape(v, -1), n))
    (tmp_path / "t.pvar").write_bytes(b"##x=1\n#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"3\t%d\tv%d\tA\t%s\n" % (10 + i, i, b"C,T" if i == 3 else b"C") for i in range(v)))
    sexes = [b"1", b"2", b"NA", b"0", b"M"]
    (tmp_path / "t.psam").write_bytes(b"#FID\tIID\tPAT\tMAT\tSEX\n" + b"".join(b"F%d\tI%d\tP%d\t0\t%s\n" % (i // 2, i, i, sexes[i % 5]) for i in range(n)))
    out = tmp_path / "o"
    p = run("export", str(tmp_path / "t"), "--format", "bed", "--include-var", 'ID != "v3"', "--include-sam", 'IID != "I4"', "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(tmp_path / "t", lambda r: r[b"ID"] != b"v3", lambda r: r[b"IID"] != b"I4", bed=True), bed=True)
    assert out.with_suffix(".fam").read_bytes().startswith(b"F0\tI0\tP0\t0\t1\t-9\nF0\tI1\tP1\t0\t2\t-9\nF1\tI2\tP2\t0\t0\t-9\n")
    bad = tmp_path / "bad"
    p = run("export", str(tmp_path / "t"), "--format", "bed", "-o", str(bad))
    assert p.returncode == 101 and b"v3" in p.stderr, p.stderr
    assert not list(tmp_path.glob("bad.*"))
    p = run("export", str(tmp_path / "t"), "-o", str(bad))   # a .pgen takes the row as it is
    assert p.returncode == 0, p.stderr
    check(bad, expected(tmp_path / "t"))


@pytest.fixture(scope="module")
def vw_pfile(tmp_path_factory):
    """tests/golden/vw/all0_8bit_len2.pgen (variable-width, every record plain) with metadata made for it."""
    d = tmp_path_factory.mktemp("vwe")
    meta = json.loads((GOLDEN / "vw" / "index.json").read_text())["all0_8bit_len2"]
    shutil.copy(GOLDEN / "vw" / "all0_8bit_len2.pgen", d / "vw.pgen")
    (d / "vw.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"7\t%d\tv%d\tC\tT\n" % (500 + 3 * i, i) for i in range(meta["variant_count"])))
    (d / "vw.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"S%04d\t%d\n" % (i, 1 + i % 2) for i in range(meta["sample_count"])))
    return d / "vw"


def test_variable_width_input_gives_a_fixed_width_file(vw_pfile, tmp_path):
    out = tmp_path / "o"
    p = run("export", str(vw_pfile), "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(vw_pfile))
    assert out.with_suffix(".pgen").read_bytes()[2] == 0x02
    vp, sp = (lambda r: r[b"ID"] not in (b"v5", b"v6")), (lambda r: r[b"IID"] != b"S0007")
    p = run("export", str(vw_pfile), "--include-var", 'ID != "v5" && ID != "v6"', "--include-sam", 'IID != "S0007"', "--shards", "3", "-o", str(out))
    assert p.returncode == 0, p.stderr
    check(out, expected(vw_pfile, vp, sp))
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    assert run("filter", str(out), "-o", str(a)).returncode == 0
    assert run("filter", str(vw_pfile), "--include-var", 'ID != "v5" && ID != "v6"', "--include-sam", 'IID != "S0007"', "-o", str(b)).returncode == 0
    assert a.read_bytes() == b.read_bytes()


def test_variable_width_compressed_kept_record_exits_101(tmp_path):
    meta = json.loads((GOLDEN / "vw" / "index.json").read_text())["mixed_8bit_len2"]
    shutil.copy(GOLDEN / "vw" / "mixed_8bit_len2.pgen", tmp_path / "m.pgen")
    (tmp_path / "m.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"7\t%d\tv%d\tC\tT\n" % (5 + i, i) for i in range(meta["variant_count"])))
    (tmp_path / "m.psam").write_bytes(b"#IID\n" + b"".join(b"S%04d\n" % i for i in range(meta["sample_count"])))
    p = run("export", str(tmp_path / "m"), "-o", str(tmp_path / "o"))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr
