"""GPU leg of `pgen-hip import`: a VCF that `filter` wrote comes back as the fileset it was written from (records with pad bits zero,
the .pvar's kept header lines and rows, the .psam's IIDs) and `filter` on the imported fileset gives the same VCF byte for byte; a
hand-written VCF against tests/parse_ref.py; and the errors that name a line and leave no file."""
import gzip
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import parse_ref
import pgen_oracle as oracle
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
N1, V1 = 2504, 17784


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def pgen_bytes(records: np.ndarray, n: int) -> bytes:
    return bytes([0x6C, 0x1B, 0x02]) + len(records).to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + records.tobytes()


@pytest.fixture(scope="module")
def basic1(tmp_path_factory):
    """basic1.{pvar,psam} are the reference's data files; basic1.pgen is synthesised at their geometry (dirty pad bits: N % 4 == 0 here,
    so there are none to mask)."""
    d = tmp_path_factory.mktemp("basic1")
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", d / f"basic1.{ext}")
    recs = oracle.synth_records(N1, V1).reshape(V1, -1)
    (d / "basic1.pgen").write_bytes(pgen_bytes(recs, N1))
    return d / "basic1", recs


def meta_lines(path: Path):
    lines = path.read_bytes().split(b"\n")
    kept = [ln for ln in lines if ln.startswith(b"##") and not ln.startswith(b"##fileformat=") and ln != b"##source=pgen-rs"]
    body = [ln for ln in lines if ln and not ln.startswith(b"##")]
    return kept, body


def test_round_trip_basic1(basic1, tmp_path):
    prefix, recs = basic1
    a = tmp_path / "a.vcf"
    assert run("filter", str(prefix), "-o", str(a)).returncode == 0
    p = run("import", str(a), "-o", str(tmp_path / "out"), "--stats")
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stderr.decode().strip().split("\n")[-1])
    assert stats["variants"] == V1 and stats["samples"] == N1 and stats["skipped_multiallelic"] == 0
    assert stats["half_call_lines"] == stats["haploid_lines"] == stats["phased_lines"] == 0 and b"warning" not in p.stderr
    assert (tmp_path / "out.pgen").read_bytes() == pgen_bytes(parse_ref.mask_pad(recs, N1), N1)
    assert meta_lines(tmp_path / "out.pvar") == meta_lines(prefix.with_suffix(".pvar"))
    iids = lambda path: [ln.split(b"\t")[0] for ln in path.read_bytes().split(b"\n") if ln]
    assert iids(tmp_path / "out.psam") == iids(prefix.with_suffix(".psam"))
    b = tmp_path / "b.vcf"
    assert run("filter", str(tmp_path / "out"), "-o", str(b)).returncode == 0
    assert b.read_bytes() == a.read_bytes()


def test_round_trip_through_bgzf_with_filters(basic1, tmp_path):
    prefix, recs = basic1
    a = tmp_path / "a.vcf.gz"
    args = ["--include-var", 'ALT == "G"', "--include-sam", 'IID != "HG00097"']
    assert run("filter", str(prefix), *args, "-o", str(a)).returncode == 0
    text = gzip.decompress(a.read_bytes())
    p = run("import", str(a), "-o", str(tmp_path / "out"), "--block-mib", "3")   # several blocks, lines cut at every block's end
    assert p.returncode == 0, p.stderr
    body = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    n = N1 - 1
    want, flags = parse_ref.parse_lines(b"".join(ln[ln.index(b"\tGT\t") + 3:] for ln in body[:50]), np.arange(50) * 4 * n, (np.arange(50) + 1) * 4 * n, n)
    raw = (tmp_path / "out.pgen").read_bytes()
    r = (n + 3) // 4
    assert raw[:12] == pgen_bytes(np.zeros((len(body), 0), dtype=np.uint8), n) and len(raw) == 12 + len(body) * r and len(body) == 4130
    assert raw[12:12 + 50 * r] == want.tobytes() and not flags.any()
    b = tmp_path / "b.vcf"
    assert run("filter", str(tmp_path / "out"), "-o", str(b)).returncode == 0
    assert b.read_bytes() == text


def test_five_column_pvar_round_trips(tmp_path):
    n, v = 13, 40
    recs = oracle.synth_records(n, v, first_variant=9).reshape(v, -1)
    (tmp_path / "t.pgen").write_bytes(pgen_bytes(recs, n))
    (tmp_path / "t.pvar").write_bytes(b"##note=five columns\n#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(b"3\t%d\tv%d\tA\tC\n" % (100 + i, i) for i in range(v)))
    (tmp_path / "t.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"s%d\tNA\n" % k for k in range(n)))
    a = tmp_path / "a.vcf"
    assert run("filter", str(tmp_path / "t"), "-o", str(a)).returncode == 0
    assert run("import", str(a), "-o", str(tmp_path / "out")).returncode == 0
    assert (tmp_path / "out.pgen").read_bytes() == pgen_bytes(parse_ref.mask_pad(recs, n), n)
    assert (tmp_path / "out.pvar").read_bytes() == (tmp_path / "t.pvar").read_bytes()
    assert (tmp_path / "out.psam").read_bytes() == (tmp_path / "t.psam").read_bytes()
    b = tmp_path / "b.vcf"
    assert run("filter", str(tmp_path / "out"), "-o", str(b)).returncode == 0 and b.read_bytes() == a.read_bytes()


HEAD = b"##fileformat=VCFv4.3\n##contig=<ID=X>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\td\te\n"
ROWS = [
    (b"X\t1\tr1\tA\tG\t.\t.\t.\tGT:DP", [b"0/1:3", b"1|1:9", b"./.:.", b"0/0:1", b"1/0:2"]),
    (b"X\t2\tr2\tA\tG\t.\t.\t.\tGT", [b"0", b"1", b".", b"0/1", b"1/1"]),
    (b"X\t3\tr3\tA\tG\t.\t.\tAC=1\tGT:GQ:PL", [b"./1:1:0,1,2", b"0/.:2:.", b"0/0:3:.", b"1/1", b"0/1:."]),
    (b"X\t4\tr4\tA\tG\t.\t.\t.\tGT", [b"0/0", b"0/0", b"0/1", b"1/1", b"./."]),
]


def vcf_of(rows, head=HEAD, eol=b"\n"):
    return head.replace(b"\n", eol) + b"".join(pre + b"".join(b"\t" + f for f in fields) + eol for pre, fields in rows)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_hand_written_vcf(tmp_path, eol):
    (tmp_path / "h.vcf").write_bytes(vcf_of(ROWS, eol=eol)[:-len(eol)])   # no final newline
    p = run("import", str(tmp_path / "h.vcf"), "-o", str(tmp_path / "out"), "--stats")
    assert p.returncode == 0, p.stderr
    want = np.stack([parse_ref.pack_codes(parse_ref.parse_region(b"".join(b"\t" + f for f in fields), 5)[0]) for _, fields in ROWS])
    assert (tmp_path / "out.pgen").read_bytes() == pgen_bytes(want, 5)
    stats = json.loads(p.stderr.decode().strip().split("\n")[-1])
    assert (stats["variants"], stats["samples"], stats["half_call_lines"], stats["haploid_lines"], stats["phased_lines"]) == (4, 5, 1, 1, 1)
    assert p.stderr.count(b"warning:") == 3
    assert (tmp_path / "out.pvar").read_bytes() == b"##contig=<ID=X>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + b"".join(
        pre[:pre.rindex(b"\t")] + b"\n" for pre, _ in ROWS)
    assert (tmp_path / "out.psam").read_bytes() == b"#IID\tSEX\na\tNA\nb\tNA\nc\tNA\nd\tNA\ne\tNA\n"


def test_multiallelic_lines(tmp_path):
    rows = list(ROWS)
    rows.insert(2, (b"X\t9\tm1\tA\tG,T\t.\t.\t.\tGT", [b"0/1", b"0/2", b"1/2", b"0/0", b"./."]))
    (tmp_path / "m.vcf").write_bytes(vcf_of(rows))
    p = run("import", str(tmp_path / "m.vcf"), "-o", str(tmp_path / "out"))
    assert p.returncode == 101 and b"line 6:" in p.stderr and b"allele" in p.stderr and not list(tmp_path.glob("out.*"))
    p = run("import", str(tmp_path / "m.vcf"), "-o", str(tmp_path / "out"), "--skip-multiallelic", "--stats")
    assert p.returncode == 0, p.stderr
    stats = json.loads(p.stderr.decode().strip().split("\n")[-1])
    assert stats["variants"] == 4 and stats["skipped_multiallelic"] == 1
    (tmp_path / "h.vcf").write_bytes(vcf_of(ROWS))
    assert run("import", str(tmp_path / "h.vcf"), "-o", str(tmp_path / "ref")).returncode == 0
    for ext in (".pgen", ".pvar", ".psam"):
        assert (tmp_path / "out").with_suffix(ext).read_bytes() == (tmp_path / "ref").with_suffix(ext).read_bytes()


@pytest.mark.parametrize("bad,what", [
    ((b"X\t5\tr5\tA\tG\t.\t.\t.\tGT", [b"0/0", b"0/1", b"0/x", b"1/1", b"./."]), b"GT"),                 # a malformed field
    ((b"X\t5\tr5\tA\tG\t.\t.\t.\tGT", [b"0/0", b"0/1", b"0/2", b"1/1", b"./."]), b"allele"),             # an allele out of range
    ((b"X\t5\tr5\tA\tG\t.\t.\t.\tGT", [b"0/0", b"0/1", b"1/1", b"./."]), b"sample fields"),             # N - 1 fields
    ((b"X\t5\tr5\tA\tG\t.\t.\t.\tGT", [b"0/0", b"0/1", b"1/1", b"./.", b"0/0", b"0/0"]), b"sample fields"),
    ((b"X\t5\tr5\tA\tG\t.\t.\t.\tDP:GT", [b"1:0/0"] * 5), b"FORMAT"),
    ((b"X\t5\tr5\tA", []), b"columns"),
])
def test_errors_name_the_line_and_leave_no_file(tmp_path, bad, what):
    rows = ROWS[:3] + [bad] + ROWS[3:]
    (tmp_path / "e.vcf").write_bytes(vcf_of(rows))
    for old in ("out.pgen", "out.pvar"):   # files from an earlier run do not survive a failed one
        (tmp_path / old).write_bytes(b"old")
    p = run("import", str(tmp_path / "e.vcf"), "-o", str(tmp_path / "out"))
    assert p.returncode == 101 and b"line 7:" in p.stderr and what in p.stderr, p.stderr
    assert not list(tmp_path.glob("out.*"))
