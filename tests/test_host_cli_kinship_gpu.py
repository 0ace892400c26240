"""GPU leg of `pgen-hip kinship`: end to end (metadata filter -> blocks of variants staged to HBM -> sample-pair tables accumulated
per pair of rank tiles -> tables back -> TSV) against tests/spair_ref.py: the line set and its order exactly, the integer columns
exactly, KINSHIP through the %.6g text of the same double arithmetic; --counts, --min-kinship; sample tiles, variant blocks and
shards give the bytes of one tile, one block, one shard.  The fileset is the synthetic one `ld`'s test uses (the golden prefixes
carry no .pgen)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spair_ref as XR
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
HEADER = b"#IID1\tIID2\tN\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP\n"
HEADER_COUNTS = HEADER[:-1] + b"".join(b"\tT%d%d" % (x, y) for x in range(4) for y in range(4)) + b"\n"
V, N = 331, 300

KEEP3 = (["--include-sam", 'KEEP == "1"'], lambda r: r[b"KEEP"] == b"1")
ODD = (["--include-var", 'ID != "snp7" && ID != "snp200" && ID != "snp201"'], lambda r: r[b"ID"] not in (b"snp7", b"snp200", b"snp201"))


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def pfile(tmp_path_factory):
    prefix = tmp_path_factory.mktemp("kinship") / "syn"
    p = run("synth", str(prefix), "--variants", str(V), "--samples", str(N), "--keep-modulus", "3")
    assert p.returncode == 0, p.stderr
    return prefix


_REF = {}


def reference(prefix, key, var_pred, sam_pred):
    """(IIDs of the kept samples, (K, K, 4, 4) tables over the kept variants); computed once per selection."""
    if key not in _REF:
        _, _, pvar_cols, pvar_rows = read_meta(prefix.with_suffix(".pvar"))
        _, _, psam_cols, psam_rows = read_meta(prefix.with_suffix(".psam"))
        raw = prefix.with_suffix(".pgen").read_bytes()
        assert raw[2] == 0x02 and int.from_bytes(raw[7:11], "little") == N
        r = XR.rsize(N)
        keep_v = [i for i, row in enumerate(pvar_rows) if var_pred is None or var_pred(dict(zip(pvar_cols, row)))]
        keep_s = [i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))]
        recs = np.stack([np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r) for vi in keep_v])
        iids = [psam_rows[s][psam_cols.index(b"IID")] for s in keep_s]
        _REF[key] = (iids, XR.pair_tables(XR.unpack(recs, N, keep_s)))
    return _REF[key]


def expected(iids, t, counts=False, min_kinship=None):
    out = [HEADER_COUNTS if counts else HEADER]
    for a in range(len(iids)):
        for b in range(a + 1, len(iids)):
            n, hethet, ibs0, het1, het2, kin = XR.kinship(t[a, b])
            if min_kinship is not None and not kin >= min_kinship:
                continue
            f = [iids[a], iids[b]] + [b"%d" % x for x in (n, hethet, ibs0, het1, het2)] + [b"nan" if np.isnan(kin) else b"%.6g" % kin]
            if counts:
                f += [b"%d" % int(x) for x in t[a, b].reshape(-1)]
            out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def test_all_pairs_and_counts(pfile):
    iids, t = reference(pfile, "all", None, None)
    assert len(iids) == N and (t.sum(axis=(2, 3)) == V).all()
    p = run("kinship", str(pfile), "--stats")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(iids, t)
    assert p.stdout.count(b"\n") == 1 + N * (N - 1) // 2 and b'"variants_kept"' in p.stderr
    p = run("kinship", str(pfile), "--counts")
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(iids, t, counts=True)


def test_sample_and_variant_filters_and_min_kinship(pfile, tmp_path):
    iids, t = reference(pfile, "odd", ODD[1], KEEP3[1])
    assert len(iids) == N // 3 and (t.sum(axis=(2, 3)) == V - 3).all()
    out = tmp_path / "kin.tsv"
    p = run("kinship", str(pfile), "--counts", *ODD[0], *KEEP3[0], "-o", str(out))
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    assert out.read_bytes() == expected(iids, t, counts=True)
    kins = sorted(XR.kinship(t[a, b])[5] for a in range(len(iids)) for b in range(a + 1, len(iids)))
    floor = kins[len(kins) // 2] + 1e-9          # between two values: about half of the lines stay
    p = run("kinship", str(pfile), *ODD[0], *KEEP3[0], "--min-kinship", repr(floor))
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(iids, t, min_kinship=floor)
    assert 1 < p.stdout.count(b"\n") < 1 + len(kins)


@pytest.mark.parametrize("flags", [["--sample-tile", "64"], ["--sample-tile", "37", "--block-rows", "50"], ["--block-rows", "1", "--shards", "2"], ["--shards", "2"], ["--shards", "3", "--sample-tile", "128"]])
def test_tiles_blocks_and_shards_give_the_same_bytes(pfile, flags):
    """Two device shards on one device, several rank tiles: the host adds u32 tables, so the bytes are those of one shard, one tile."""
    iids, t = reference(pfile, "all", None, None)
    p = run("kinship", str(pfile), "--counts", *flags)
    assert p.returncode == 0, p.stderr
    assert p.stdout == expected(iids, t, counts=True)


def test_one_sample_is_the_header_alone(pfile):
    p = run("kinship", str(pfile), "--include-sam", 'IID == "nobody"')
    assert p.returncode == 0 and p.stdout == HEADER, p.stderr


def test_variable_width_plain_records_give_the_fixed_width_bytes(tmp_path):
    """Mode-0x10 records go to the sample-pair kernel through their staged offsets (the `_at` entry): tiles, blocks and a shard
    seam over 60 plain records give the bytes of the fixed-width file of the same records."""
    from helpers import plain_record_filesets

    vw, fixed = plain_record_filesets(tmp_path)
    flags = ["--sample-tile", "16", "--block-rows", "9", "--shards", "2", "--counts", "--include-var", 'RTYPE == "0"']
    a, b = run("kinship", str(vw), *flags), run("kinship", str(fixed), *flags)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout == b.stdout and a.stdout.count(b"\n") == 1 + 40 * 39 // 2
    one = run("kinship", str(fixed), "--counts")
    assert one.returncode == 0 and one.stdout == b.stdout, one.stderr
