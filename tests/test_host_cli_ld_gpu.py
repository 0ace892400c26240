"""GPU leg of `pgen-hip ld`: windowed pairwise r^2 end to end (metadata filter -> a block's rows and the window's halo staged to HBM
-> pair kernel -> entries back -> TSV) against tests/pair_ref.py: the line set and its order exactly, r^2 through the %.6g round
trip; shard and block seams; and `freq` / `sample-counts` on the same fileset against numpy (the block loop they share with `ld`
grew a halo parameter)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pair_ref as PR
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
HEADER = b"#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tR2\n"
HEADER_COUNTS = HEADER[:-1] + b"\tN_OBS" + b"".join(b"\tT%d%d" % (a, b) for a in range(4) for b in range(4)) + b"\n"
V, N, SPLIT = 331, 300, 190          # variants, samples, first variant of the second chromosome


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def pfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("ld")
    prefix = d / "syn"
    p = run("synth", str(prefix), "--variants", str(V), "--samples", str(N), "--keep-modulus", "3")
    assert p.returncode == 0, p.stderr
    pvar = prefix.with_suffix(".pvar")
    out, row = [], 0
    for ln in pvar.read_bytes().split(b"\n"):
        if ln and not ln.startswith(b"#"):
            f = ln.split(b"\t")
            f[0] = b"21" if row < SPLIT else b"22"
            ln = b"\t".join(f)
            row += 1
        out.append(ln)
    pvar.write_bytes(b"\n".join(out))
    assert row == V
    return prefix


def selection(prefix, var_pred, sam_pred):
    _, _, pvar_cols, pvar_rows = read_meta(prefix.with_suffix(".pvar"))
    _, _, psam_cols, psam_rows = read_meta(prefix.with_suffix(".psam"))
    raw = prefix.with_suffix(".pgen").read_bytes()
    assert raw[2] == 0x02 and int.from_bytes(raw[7:11], "little") == N
    r = PR.rsize(N)
    keep_v = [i for i, row in enumerate(pvar_rows) if var_pred is None or var_pred(dict(zip(pvar_cols, row)))]
    keep_s = [i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))]
    recs = np.stack([np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r) for vi in keep_v]) if keep_v else np.zeros((0, r), np.uint8)
    meta = [[pvar_rows[i][pvar_cols.index(c)] for c in (b"CHROM", b"POS", b"ID")] for i in keep_v]
    return recs, keep_v, keep_s, meta, (pvar_cols, pvar_rows, psam_cols, psam_rows)


_REF = {}


def reference(prefix, key, var_pred, sam_pred, w):
    """[(fields of the six leading columns, r^2 float32, table)] of every pair `ld --min-r2 0` prints, in order; computed once
    per selection."""
    if key not in _REF:
        recs, keep_v, keep_s, meta, _ = selection(prefix, var_pred, sam_pred)
        codes = PR.unpack(recs, N, keep_s)
        rows = []
        for i, d in PR.pair_list(len(keep_v), len(keep_v), w):
            if meta[i][0] != meta[i + d][0]:
                continue
            t = PR.table(codes[i], codes[i + d])
            r2 = PR.r2_f32(t)
            if not np.isnan(r2):
                rows.append((meta[i] + meta[i + d], r2, t))
        _REF[key] = rows
    return _REF[key]


def r2_texts(x):
    """What %.6g may print for an r^2 within one float32 ulp of x (the kernel's contract)."""
    return {b"%.6g" % float(c) for c in (x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2)))}


def check_lines(stdout, rows, counts=False):
    head = HEADER_COUNTS if counts else HEADER
    assert stdout.startswith(head)
    lines = stdout[len(head):].split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]
    assert len(lines) == len(rows), f"{len(lines)} lines, reference {len(rows)}"
    for ln, (lead, r2, t) in zip(lines, rows):
        f = ln.split(b"\t")
        assert f[:6] == lead, (f[:6], lead)
        assert f[6] in r2_texts(r2), (lead, f[6], r2)
        if counts:
            assert f[7:] == [b"%d" % int(t[:3, :3].sum())] + [b"%d" % int(x) for x in t.reshape(-1)], lead
        else:
            assert len(f) == 7


KEEP3 = (["--include-sam", 'KEEP == "1"'], lambda r: r[b"KEEP"] == b"1")
ODD = (["--include-var", 'ID != "snp7" && ID != "snp200" && ID != "snp201"'], lambda r: r[b"ID"] not in (b"snp7", b"snp200", b"snp201"))


def test_window_10_all_pairs_and_counts(pfile):
    rows = reference(pfile, "all", None, None, 10)
    assert len(rows) > 2000 and all(lead[0] == lead[3] for lead, _, _ in rows)
    assert any(lead[0] == b"21" for lead, _, _ in rows) and any(lead[0] == b"22" for lead, _, _ in rows)
    p = run("ld", str(pfile), "--window", "10", "--min-r2", "0", "--stats")
    assert p.returncode == 0, p.stderr
    check_lines(p.stdout, rows)
    assert b'"variants_kept"' in p.stderr
    p = run("ld", str(pfile), "--window", "10", "--min-r2", "0", "--counts")
    assert p.returncode == 0, p.stderr
    check_lines(p.stdout, rows, counts=True)


def test_sample_and_variant_filters(pfile, tmp_path):
    rows = reference(pfile, "keep3", None, KEEP3[1], 10)
    p = run("ld", str(pfile), "--window", "10", "--min-r2", "0", *KEEP3[0])
    assert p.returncode == 0, p.stderr
    check_lines(p.stdout, rows)
    rows = reference(pfile, "odd", ODD[1], KEEP3[1], 10)
    out = tmp_path / "ld.tsv"
    p = run("ld", str(pfile), "--window", "10", "--min-r2", "0", "--counts", *ODD[0], *KEEP3[0], "-o", str(out))
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    check_lines(out.read_bytes(), rows, counts=True)


@pytest.mark.parametrize("flags", [["--shards", "3"], ["--block-rows", "7"], ["--block-rows", "16", "--shards", "2"], ["--block-rows", "1"]])
def test_seams_neither_lose_nor_repeat_a_pair(pfile, flags):
    """Shards own ranges of first variants, blocks overlap by the window: the bytes are those of one block."""
    for extra in ([], ["--counts"]):
        one = run("ld", str(pfile), "--window", "10", "--min-r2", "0", *extra)
        p = run("ld", str(pfile), "--window", "10", "--min-r2", "0", *extra, *flags)
        assert one.returncode == 0 and p.returncode == 0, p.stderr
        assert p.stdout == one.stdout
    check_lines(one.stdout, reference(pfile, "all", None, None, 10), counts=True)


def test_default_threshold_and_wide_window(pfile):
    all_pairs = run("ld", str(pfile), "--window", "10", "--min-r2", "0").stdout.split(b"\n")[1:-1]
    p = run("ld", str(pfile), "--window", "10")
    assert p.returncode == 0, p.stderr
    kept = p.stdout.split(b"\n")[1:-1]
    assert [ln for ln in all_pairs if float(ln.split(b"\t")[6]) >= 0.2001] == [ln for ln in kept if float(ln.split(b"\t")[6]) >= 0.2001]
    assert all(float(ln.split(b"\t")[6]) >= 0.1999 for ln in kept) and set(kept) <= set(all_pairs)
    # a window wider than the file: every pair of a chromosome
    rows = reference(pfile, "wide", lambda r: int(r[b"ID"][3:]) % 9 == 0, None, 5000)
    ids = [b"snp%d" % i for i in range(0, V, 9)]
    p = run("ld", str(pfile), "--window", "5000", "--min-r2", "0", "--include-var", " || ".join('ID == "%s"' % i.decode() for i in ids))
    assert p.returncode == 0, p.stderr
    check_lines(p.stdout, rows)


def test_fewer_than_two_variants_or_no_sample_is_the_header_alone(pfile):
    p = run("ld", str(pfile), "--window", "10", "--include-var", 'ID == "snp5"')
    assert p.returncode == 0 and p.stdout == HEADER, p.stderr
    p = run("ld", str(pfile), "--window", "10", "--include-var", 'ID == "nothing"', "--counts")
    assert p.returncode == 0 and p.stdout == HEADER_COUNTS, p.stderr
    p = run("ld", str(pfile), "--window", "10", "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0 and p.stdout == HEADER, p.stderr


@pytest.mark.parametrize("args", [[], ["x"], ["x", "--window"], ["x", "--window", "0"], ["x", "--window", "-3"], ["x", "--window", "w"],
                                  ["x", "--window", "5", "--min-r2", "2"], ["x", "--window", "5", "--min-r2", "x"],
                                  ["x", "--window", "5", "--bogus"], ["x", "y", "--window", "5"], ["x", "--window", "5", "--block-rows", "0"]])
def test_usage_errors_exit_2(args):
    p = run("ld", *args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def test_freq_and_sample_counts_on_the_same_fileset(pfile):
    """The block loop `ld` shares with them, with no halo: their bytes from numpy, not from the code under test."""
    recs, keep_v, keep_s, _, (pvar_cols, pvar_rows, psam_cols, psam_rows) = selection(pfile, ODD[1], KEEP3[1])
    codes = PR.unpack(recs, N, keep_s)
    cols = [pvar_cols.index(c) for c in (b"CHROM", b"POS", b"ID", b"REF", b"ALT")]
    want = b"#CHROM\tPOS\tID\tREF\tALT\tHOM_REF_CT\tHET_REF_ALT_CTS\tTWO_ALT_GENO_CTS\tMISSING_CT\n" + b"".join(
        b"\t".join([pvar_rows[vi][c] for c in cols] + [b"%d" % int((codes[j] == g).sum()) for g in range(4)]) + b"\n"
        for j, vi in enumerate(keep_v))
    for flags in ([], ["--shards", "3"]):
        p = run("freq", str(pfile), *ODD[0], *KEEP3[0], *flags)
        assert p.returncode == 0, p.stderr
        assert p.stdout == want
    iid = psam_cols.index(b"IID")
    want = b"#IID\tHOM_REF_CT\tHET_CT\tHOM_ALT_CT\tMISSING_CT\n" + b"".join(
        b"\t".join([psam_rows[s][iid]] + [b"%d" % int((codes[:, k] == g).sum()) for g in range(4)]) + b"\n" for k, s in enumerate(keep_s))
    for flags in ([], ["--shards", "3"]):
        p = run("sample-counts", str(pfile), *ODD[0], *KEEP3[0], *flags)
        assert p.returncode == 0, p.stderr
        assert p.stdout == want


def test_variable_width_plain_records_give_the_fixed_width_bytes(tmp_path):
    """Mode-0x10 records go to the pair kernel through their staged offsets (the `_at` entry): blocks, halo rows and a shard seam
    over 60 plain records give the bytes of the fixed-width file of the same records."""
    from helpers import plain_record_filesets

    vw, fixed = plain_record_filesets(tmp_path)
    flags = ["--window", "5", "--block-rows", "7", "--shards", "2", "--counts", "--min-r2", "0", "--include-var", 'RTYPE == "0"']
    a, b = run("ld", str(vw), *flags), run("ld", str(fixed), *flags)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout == b.stdout and a.stdout.count(b"\n") > 200
    one = run("ld", str(fixed), "--window", "5", "--counts", "--min-r2", "0")
    assert one.returncode == 0 and one.stdout == b.stdout, one.stderr
