"""`pgen-hip import` beyond its first block (host/import.cpp): error line numbers far into the input with skipped lines in between,
a line against the block size, blocks filled with lines of the minimal width that ``max_lines`` is sized by, and VcfSource on plain
concatenated gzip members.  The expected .pgen always comes from tests/parse_ref.py; the expected .pvar / .psam are written out here.
Files are compared for equality.

Measured on the MI355X (a whole test, its CLI process included; the file runs in 8 s): the far file 0.3 s behind 0.3 s for its
shared reference, 0.3 - 0.4 s per error; a line against the block size 0.35 s per case; the #CHROM line of 1.5 MiB 0.5 s; blocks
of minimal lines 0.2 - 0.4 s per line ending behind 0.6 s for parse_ref over 75 000 lines, shared; gzip members 0.9 s (two
imports); a damaged small stream 0.01 s, a damaged far file under 0.4 s.
"""
import gzip
import json

import numpy as np
import pytest

import parse_ref
from test_host_cli_import_gpu import HEAD, ROWS, pgen_bytes, run, vcf_of

pytestmark = pytest.mark.gpu

MIB = 1 << 20
COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


def stats_of(p):
    return json.loads(p.stderr.decode().strip().split("\n")[-1])


def no_files(tmp_path, prefix="out"):
    return not list(tmp_path.glob(prefix + ".*"))


def fails(tmp_path, path, what, *args, old=True):
    """The import exits 101 with ``what`` in its message and leaves no output file; ``old``: not even one from an earlier run (an
    error that is met once the output exists; one met while the header is read leaves the directory as it was)."""
    if old:
        (tmp_path / "out.pgen").write_bytes(b"old")
    p = run("import", str(path), "-o", str(tmp_path / "out"), *args)
    assert p.returncode == 101 and what in p.stderr, (p.returncode, p.stderr[-400:])
    assert no_files(tmp_path), list(tmp_path.glob("out.*"))
    return p


def expected_pgen(regions, n):
    text = b"".join(regions)
    ends = np.cumsum([len(r) for r in regions])
    recs, flags = parse_ref.parse_lines(text, ends - [len(r) for r in regions], ends, n)
    return pgen_bytes(recs, n), flags


# ---- far line numbers ---------------------------------------------------------------------------------------------------------------
N_FAR = 50
FAR_HEAD = b"##fileformat=VCFv4.2\n##contig=<ID=7>\n##note=far lines\n" + COLS + b"\tFORMAT" + b"".join(b"\ts%d" % k for k in range(N_FAR)) + b"\n"
FAR_HEADER_LINES = 4
BAD_AT = 3000   # the data line (0-based) that the error cases replace


def far_line(i, fields, alt=b"G"):
    return b"7\t%d\tv%d\tA\t%s\t.\t.\tPAD=%s\tGT" % (100 + i, i, alt, b"x" * 700) + b"".join(b"\t" + f for f in fields) + b"\n"


@pytest.fixture(scope="module")
def far():
    """About 3.5 MiB of lines of N = 50: fixed-width lines, every 7th with fields of other widths, and a multiallelic line (ALT `G,T`,
    alleles 2) after every 40th.  -> (lines, indices of the multiallelic lines, the expected .pgen and .pvar of the others)."""
    rng = np.random.default_rng(71)
    narrow = [b"0/0", b"0/1", b"1/1", b"./.", b"1|0"]
    wide = narrow + [b"0", b"1", b".", b"./1", b"0|1"]
    lines, multi, regions, pvar = [], [], [], [b"##contig=<ID=7>", b"##note=far lines", COLS]
    i = 0
    while sum(map(len, lines)) < 7 * MIB // 2:
        pool = wide if i % 7 == 3 else narrow
        fields = [pool[k] for k in rng.integers(0, len(pool), size=N_FAR)]
        lines.append(far_line(i, fields))
        regions.append(b"".join(b"\t" + f for f in fields))
        pvar.append(lines[-1][:lines[-1].index(b"\tGT\t")])
        if i % 40 == 11:
            multi.append(len(lines))
            lines.append(far_line(i, [(b"0/2", b"1/2", b"2/2", b"0/1")[k] for k in rng.integers(0, 4, size=N_FAR)], alt=b"G,T"))
        i += 1
    pgen, flags = expected_pgen(regions, N_FAR)
    assert not (flags & (parse_ref.FIELD_COUNT | parse_ref.BAD_CALL | parse_ref.ALLELE_RANGE)).any()
    return lines, multi, pgen, b"\n".join(pvar) + b"\n", flags


def test_far_file_imports(far, tmp_path):
    """``lines_before`` and the carry across four blocks of 1 MiB with skipped multiallelic lines in every block: the records are
    parse_ref's, ``skipped_multiallelic`` is the number planted, and the line counters are the reference's."""
    lines, multi, pgen, pvar, flags = far
    body = b"".join(lines)
    assert len(body) > 3 * MIB and all(any(k * MIB < sum(map(len, lines[:m])) < (k + 1) * MIB for m in multi) for k in range(3))
    (tmp_path / "far.vcf").write_bytes(FAR_HEAD + body)
    p = run("import", str(tmp_path / "far.vcf"), "-o", str(tmp_path / "out"), "--block-mib", "1", "--skip-multiallelic", "--stats")
    assert p.returncode == 0, p.stderr
    st = stats_of(p)
    assert (st["variants"], st["samples"], st["skipped_multiallelic"]) == (len(lines) - len(multi), N_FAR, len(multi))
    assert st["haploid_lines"] == int(((flags & parse_ref.HAPLOID) != 0).sum()) and st["phased_lines"] == int(((flags & parse_ref.PHASED) != 0).sum())
    assert st["half_call_lines"] == int(((flags & parse_ref.HALF_CALL) != 0).sum())
    assert (tmp_path / "out.pgen").read_bytes() == pgen
    assert (tmp_path / "out.pvar").read_bytes() == pvar
    assert (tmp_path / "out.psam").read_bytes() == b"#IID\tSEX\n" + b"".join(b"s%d\tNA\n" % k for k in range(N_FAR))


@pytest.mark.parametrize("kind,what", [("columns", b"fewer columns"), ("format", b"GT must come first"), ("count", b"sample fields"),
                                       ("call", b"neither A nor A/B"), ("allele", b"an allele other than")])
def test_far_error_names_its_line(far, tmp_path, kind, what):
    """One bad line in the third block (behind 3 000 lines, dozens of them skipped): the reader's errors (``lines_before + i + 1``) and
    the device's (``b.line_no[j]``, with the skipped lines of every block so far counted) name exactly that 1-based input line."""
    lines = list(far[0])
    assert sum(map(len, lines[:BAD_AT])) + len(FAR_HEAD) > 2 * MIB and BAD_AT not in far[1]   # the third block or later
    fields = [b"0/1"] * N_FAR
    if kind == "columns":
        bad = b"7\t5\tx\tA\n"
    elif kind == "format":
        bad = far_line(0, [b"1:0/0"] * N_FAR).replace(b"\tGT\t", b"\tDP:GT\t")
    elif kind == "count":
        bad = far_line(0, fields[:-1])
    elif kind == "call":
        bad = far_line(0, fields[:30] + [b"0/x"] + fields[31:])
    else:
        bad = far_line(0, fields[:30] + [b"0/2"] + fields[31:])
    lines[BAD_AT] = bad
    (tmp_path / "e.vcf").write_bytes(FAR_HEAD + b"".join(lines))
    p = fails(tmp_path, tmp_path / "e.vcf", what, "--block-mib", "1", "--skip-multiallelic")
    assert b"line %d:" % (FAR_HEADER_LINES + BAD_AT + 1) in p.stderr, p.stderr[-400:]


# ---- a line against the block size ------------------------------------------------------------------------------------------------------
N_BLOCK = 1000
BLOCK_HEAD = b"##fileformat=VCFv4.2\n" + COLS + b"\tFORMAT" + b"".join(b"\tq%d" % k for k in range(N_BLOCK)) + b"\n"


def sized_line(i, size, rng):
    """A data line of N = 1000 that is exactly ``size`` bytes with its newline (the INFO column takes up the slack)."""
    fields = [(b"0/0", b"0/1", b"1/1", b"./.")[k] for k in rng.integers(0, 4, size=N_BLOCK)]
    region = b"".join(b"\t" + f for f in fields)
    pre = b"2\t%d\tb%d\tC\tT\t.\t.\t" % (i, i)
    pad = size - len(pre) - len(b"\tGT") - len(region) - 1
    assert pad >= 1
    line = pre + b"i" * pad + b"\tGT" + region + b"\n"
    assert len(line) == size
    return line, region


@pytest.mark.parametrize("position", ["first_in_its_block", "behind_a_short_line"])
@pytest.mark.parametrize("extra", [0, 1], ids=["exactly_a_block", "a_block_and_a_byte"])
def test_a_line_against_the_block_size(tmp_path, position, extra):
    """At --block-mib 1 a data line of exactly 2^20 bytes (newline included) imports, as the first line of its block and directly behind
    a short line (then it arrives half by the carry); one of 2^20 + 1 bytes is "a line is longer than a block" (``n == 0 && len ==
    cap``: the only one of the two such errors a command line can reach, since the carry behind the header is below 1 MiB and a block
    is at least that), exit 101, no files."""
    rng = np.random.default_rng(73)
    big, big_region = sized_line(1, MIB + extra, rng)
    small, small_region = sized_line(2, 5000, rng)
    order = [(big, big_region), (small, small_region)] if position == "first_in_its_block" else [(small, small_region), (big, big_region)]
    (tmp_path / "b.vcf").write_bytes(BLOCK_HEAD + b"".join(line for line, _ in order))
    if extra:
        fails(tmp_path, tmp_path / "b.vcf", b"a line is longer than a block", "--block-mib", "1")
        return
    p = run("import", str(tmp_path / "b.vcf"), "-o", str(tmp_path / "out"), "--block-mib", "1", "--stats")
    assert p.returncode == 0, p.stderr
    assert stats_of(p)["variants"] == 2
    assert (tmp_path / "out.pgen").read_bytes() == expected_pgen([r for _, r in order], N_BLOCK)[0]
    assert (tmp_path / "out.pvar").read_bytes() == COLS + b"\n" + b"".join(line[:line.index(b"\tGT\t")] + b"\n" for line, _ in order)


def test_a_chrom_line_longer_than_a_mib(tmp_path):
    """The header loop's carry over several 1-MiB reads: a #CHROM line of N = 200 000 sample names (1.5 MiB) and one data line, at
    --block-mib 2."""
    n = 200_000
    names = [b"sample%d" % k for k in range(n)]
    chrom = COLS + b"\tFORMAT\t" + b"\t".join(names) + b"\n"
    assert len(chrom) > MIB
    rng = np.random.default_rng(74)
    region = b"".join(b"\t" + (b"0/0", b"0/1", b"1/1", b"./.", b"1|1")[k] for k in rng.integers(0, 5, size=n))
    (tmp_path / "c.vcf").write_bytes(b"##fileformat=VCFv4.2\n" + chrom + b"3\t9\tw\tG\tA\t.\t.\t.\tGT" + region + b"\n")
    p = run("import", str(tmp_path / "c.vcf"), "-o", str(tmp_path / "out"), "--block-mib", "2", "--stats")
    assert p.returncode == 0, p.stderr
    assert (stats_of(p)["variants"], stats_of(p)["samples"]) == (1, n)
    assert (tmp_path / "out.pgen").read_bytes() == expected_pgen([region], n)[0]
    assert (tmp_path / "out.pvar").read_bytes() == COLS + b"\n3\t9\tw\tG\tA\t.\t.\t.\n"
    assert (tmp_path / "out.psam").read_bytes() == b"#IID\tSEX\n" + b"".join(name + b"\tNA\n" for name in names)


# ---- max_lines filled -------------------------------------------------------------------------------------------------------------------
N_MIN, V_MIN = 5, 75_000


@pytest.fixture(scope="module")
def minimal():
    rng = np.random.default_rng(75)
    picks = rng.integers(0, 3, size=(V_MIN, N_MIN))
    regions = [b"".join(b"\t" + (b"0", b"1", b".")[k] for k in row) for row in picks]
    pgen, flags = expected_pgen(regions, N_MIN)
    assert (flags == parse_ref.HAPLOID).all()
    return regions, pgen


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_blocks_of_minimal_lines(minimal, tmp_path, eol):
    """``max_lines = cap / (2 N + 2 format_col + 3) + 1``: one-character columns, FORMAT `GT` and haploid one-character fields make every
    line exactly 2 N + 2 format_col + 3 = 29 bytes, the narrowest line that passes the reader's checks, so each full block of 1 MiB
    holds as many lines as any block can (36 157; max_lines is 36 158) and the offset, record and flag buffers sized by max_lines
    are used up to their last slot but one; three blocks, no final newline.  Again with CRLF (30 bytes a line)."""
    regions, pgen = minimal
    prefix = b"1\t2\t.\tA\tC\t.\t.\t."
    lines = [prefix + b"\tGT" + r + b"\n" for r in regions]
    assert all(len(ln) == 2 * N_MIN + 2 * 8 + 3 for ln in lines) and len(lines) * 29 > 2 * MIB
    assert MIB // 29 + 1 == 36_158 and MIB // 29 == 36_157
    head = b"##fileformat=VCFv4.2\n" + COLS + b"\tFORMAT\ta\tb\tc\td\te\n"
    (tmp_path / "m.vcf").write_bytes((head + b"".join(lines)).replace(b"\n", eol)[:-len(eol)])
    p = run("import", str(tmp_path / "m.vcf"), "-o", str(tmp_path / "out"), "--block-mib", "1", "--stats")
    assert p.returncode == 0, p.stderr
    st = stats_of(p)
    assert (st["variants"], st["samples"], st["haploid_lines"], st["phased_lines"], st["half_call_lines"]) == (V_MIN, N_MIN, V_MIN, 0, 0)
    assert (tmp_path / "out.pgen").read_bytes() == pgen
    assert (tmp_path / "out.pvar").read_bytes() == COLS + b"\n" + (prefix + b"\n") * V_MIN
    assert (tmp_path / "out.psam").read_bytes() == b"#IID\tSEX\na\tNA\nb\tNA\nc\tNA\nd\tNA\ne\tNA\n"


# ---- gzip members -----------------------------------------------------------------------------------------------------------------------
def members(data: bytes, cuts, empties=()):
    """``data`` cut at ``cuts`` and compressed as plain gzip members; an empty member in front of each part index in ``empties``
    (len(cuts) + 1: at the end)."""
    parts = [data[a:b] for a, b in zip((0, *cuts), (*cuts, len(data)))]
    out = []
    for k, part in enumerate(parts):
        if k in empties:
            out.append(gzip.compress(b""))
        out.append(gzip.compress(part))
    if len(parts) in empties:
        out.append(gzip.compress(b""))
    return out


HAND = vcf_of(ROWS)
CUT_HEADER, CUT_LINE = 30, len(HEAD) + 20   # inside the second ## line; inside the first data line
assert 0 < CUT_HEADER < HEAD.index(b"#CHROM") and HAND[CUT_LINE - 20 - 1:CUT_LINE - 20] == b"\n" and b"\n" not in HAND[CUT_LINE - 19:CUT_LINE + 1]


def test_plain_gzip_members(tmp_path):
    """VcfSource's ``inflateReset`` at Z_STREAM_END: three plain gzip members with seams inside a header line and inside a data line,
    an empty member between the first two and one at the end.  The fileset is the plain file's, byte for byte."""
    (tmp_path / "h.vcf").write_bytes(HAND)
    assert run("import", str(tmp_path / "h.vcf"), "-o", str(tmp_path / "ref")).returncode == 0
    stream = b"".join(members(HAND, (CUT_HEADER, CUT_LINE), empties=(1, 3)))
    assert gzip.decompress(stream) == HAND and stream.count(b"\x1f\x8b\x08") >= 5
    (tmp_path / "h.vcf.gz").write_bytes(stream)
    p = run("import", str(tmp_path / "h.vcf.gz"), "-o", str(tmp_path / "out"))
    assert p.returncode == 0, p.stderr
    for ext in (".pgen", ".pvar", ".psam"):
        assert (tmp_path / "out").with_suffix(ext).read_bytes() == (tmp_path / "ref").with_suffix(ext).read_bytes(), ext
    want = np.stack([parse_ref.pack_codes(parse_ref.parse_region(b"".join(b"\t" + f for f in fields), 5)[0]) for _, fields in ROWS])
    assert (tmp_path / "out.pgen").read_bytes() == pgen_bytes(want, 5)


@pytest.mark.parametrize("where", ["header", "body"])
def test_a_stream_that_ends_inside_a_member(tmp_path, where):
    """``mid_member_`` at the end of the file: the stream above cut inside its first member (the header's) and inside its last
    data member.  (The header loop's first read inflates all of so small a stream: both are met before the output exists.)"""
    ms = members(HAND, (CUT_HEADER, CUT_LINE), empties=(1, 3))
    k = 0 if where == "header" else 3
    stream = b"".join(ms[:k]) + ms[k][:len(ms[k]) - 9]   # the member loses its trailer and the last byte of its data
    (tmp_path / "t.vcf.gz").write_bytes(stream)
    fails(tmp_path, tmp_path / "t.vcf.gz", b"ends inside a member", old=False)


@pytest.mark.parametrize("where", ["header", "body"])
def test_bytes_that_are_not_gzip(tmp_path, where):
    """The branch behind ``inflate`` that is neither Z_OK nor Z_STREAM_END: the second of three members overwritten, when it holds the
    rest of the header and when it holds body bytes only."""
    cuts = (CUT_HEADER, CUT_LINE) if where == "header" else (CUT_LINE, CUT_LINE + 40)
    ms = members(HAND, cuts)
    ms[1] = bytes(len(ms[1]))
    (tmp_path / "g.vcf.gz").write_bytes(b"".join(ms))
    fails(tmp_path, tmp_path / "g.vcf.gz", b"not a gzip stream", old=False)


@pytest.mark.parametrize("damage", ["truncated", "overwritten"])
def test_a_damaged_member_behind_written_blocks(far, tmp_path, damage):
    """The same two errors met by the reader thread, behind blocks that are already written: the far file as five members cut inside
    lines, the fourth one damaged.  The output files that exist by then do not stay."""
    data = FAR_HEAD + b"".join(far[0])
    cuts = (MIB // 2 + 17, MIB + 333, 5 * MIB // 2 + 1, 3 * MIB + 77)
    ms = members(data, cuts)
    if damage == "truncated":
        stream, what = b"".join(ms[:3]) + ms[3][:len(ms[3]) // 2], b"ends inside a member"
    else:
        ms[3] = bytes(len(ms[3]))
        stream, what = b"".join(ms), b"not a gzip stream"
    (tmp_path / "d.vcf.gz").write_bytes(stream)
    fails(tmp_path, tmp_path / "d.vcf.gz", what, "--block-mib", "1", "--skip-multiallelic")
