"""GPU leg of `pgen-hip sample-counts`: per-sample genotype counts end to end (metadata filter -> records staged to HBM -> sample count
kernel, blocks accumulated per shard -> 16 bytes per kept sample back) against the expected text built with numpy, and against
filter's VCF for the same flags, counted per column."""
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pgen_oracle as oracle
from helpers import GOLDEN
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
HEADER = b"#IID\tHOM_REF_CT\tHET_CT\tHOM_ALT_CT\tMISSING_CT\n"


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def expected(prefix: Path, var_pred=None, sam_pred=None) -> bytes:
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
    keep_s = [i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))]
    cts = np.zeros((len(keep_s), 4), dtype=np.int64)
    if keep_v and keep_s:
        recs = np.stack([np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r if offs is None else int(offs[vi])) for vi in keep_v])
        codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(keep_v), -1)[:, :n][:, keep_s]
        cts = np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1)
    iid = psam_cols.index(b"IID")
    return HEADER + b"".join(b"\t".join([psam_rows[s][iid]] + [b"%d" % x for x in cts[k]]) + b"\n" for k, s in enumerate(keep_s))


def counts_from_vcf(vcf: bytes):
    """The VCF's GT columns counted per column: [IID, hom-ref, het, hom-alt, missing] per sample."""
    ids, cols = None, None
    for ln in vcf.split(b"\n"):
        if ln.startswith(b"#CHROM"):
            f = ln.split(b"\t")
            ids = f[f.index(b"FORMAT") + 1:]
            cols = [[0, 0, 0, 0] for _ in ids]
        elif ln and not ln.startswith(b"#"):
            f = ln.split(b"\t")
            for k, g in enumerate(f[f.index(b"GT") + 1:]):
                cols[k][(b"0/0", b"0/1", b"1/1", b"./.").index(g)] += 1
    return [[i] + [b"%d" % x for x in c] for i, c in zip(ids, cols)]


@pytest.fixture(scope="module")
def basic1(tmp_path_factory):
    d = tmp_path_factory.mktemp("basic1s")
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", d / f"basic1.{ext}")
    n, v = 2504, 17784
    recs = oracle.synth_records(n, v)
    (d / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    return d / "basic1"


CASES = {
    "all": ([], None, None),
    "alt_g": (["--include-var", 'ALT == "G"'], lambda r: r[b"ALT"] == b"G", None),
    "samples": (["--include-sam", 'IID == "HG00097" || IID == "NA20900" || IID == "NA21144"'], None,
                lambda r: r[b"IID"] in (b"HG00097", b"NA20900", b"NA21144")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_basic1_matches_expected_and_filter(basic1, tmp_path, case):
    flags, vp, sp = CASES[case]
    p = run("sample-counts", str(basic1), *flags, "--stats")
    assert p.returncode == 0, p.stderr
    want = expected(basic1, vp, sp)
    assert p.stdout == want
    assert b'"variants_kept"' in p.stderr
    if case != "all":   # (every sample of every variant is 180 MB of VCF: counted in Python it would take minutes)
        vcf = tmp_path / "f.vcf"
        q = run("filter", str(basic1), *flags, "-o", str(vcf))
        assert q.returncode == 0, q.stderr
        body = [ln.split(b"\t") for ln in p.stdout.split(b"\n")[1:] if ln]
        assert body == counts_from_vcf(vcf.read_bytes())
    out = tmp_path / "s.tsv"
    assert run("sample-counts", str(basic1), *flags, "-o", str(out)).returncode == 0 and out.read_bytes() == want


@pytest.mark.parametrize("shards", [1, 3, 7])
def test_shards_and_blocks_accumulate(basic1, shards):
    p = run("sample-counts", str(basic1), "--include-var", 'ALT == "G"', "--include-sam", 'IID != "HG00097"', "--shards", str(shards), "--block-mib", "1")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(basic1, lambda r: r[b"ALT"] == b"G", lambda r: r[b"IID"] != b"HG00097")


def test_more_shards_than_variants(basic1):
    ids = ("rs2312724", "rs7815")
    p = run("sample-counts", str(basic1), "--include-var", " || ".join(f'ID == "{i}"' for i in ids), "--shards", "7")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(basic1, lambda r: r[b"ID"].decode() in ids)
    assert all(sum(int(x) for x in ln.split(b"\t")[1:]) == 2 for ln in p.stdout.split(b"\n")[1:-1])


@pytest.fixture(scope="module")
def vw_pfile(tmp_path_factory):
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    d = tmp_path_factory.mktemp("vws")
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


def test_variable_width_plain_records_are_counted(vw_pfile):
    p = run("sample-counts", str(vw_pfile), "--include-var", 'RTYPE == "0"', "--block-mib", "1")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(vw_pfile, lambda r: r[b"RTYPE"] == b"0")
    p = run("sample-counts", str(vw_pfile), "--include-var", 'RTYPE == "0" && ID != "v5"', "--include-sam", 'IID != "S0007"', "--shards", "3")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(vw_pfile, lambda r: r[b"RTYPE"] == b"0" and r[b"ID"] != b"v5", lambda r: r[b"IID"] != b"S0007")


def test_variable_width_compressed_kept_record_exits_101(vw_pfile):
    p = run("sample-counts", str(vw_pfile))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr
