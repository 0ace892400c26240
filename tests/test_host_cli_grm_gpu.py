"""GPU leg of `pgen-hip grm`: end to end (metadata filter -> blocks of variants staged to HBM -> counts back -> tables -> two FP64 Gram
matrices accumulated per pair of rank tiles -> G / N -> files) against tests/gram_ref.py, entry for entry.

Allowance per entry, in units of A / N (A = sum over the variants of |t[x_a] t[x_b]|, N the variants called in both samples):
1.01 (V + 64) 2^-53 for the device sums and the host's division, plus the two reference formulations' own disagreement
(gram_ref.REF_DISAGREEMENT); grm-bin adds 2^-23 |value| for the f32 store.  Rank tiles, variant blocks and shards cut
the sums differently (the kernel's slice plan depends on the size of the tile pair), so every cut is held to the same allowance, not
to identical bytes; N is an exact integer in every cut."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gram_ref as GR
from helpers import GOLDEN
from ref_vcf import read_meta

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
GRM = GOLDEN / "grm"
V, N = 3000, 300

KEEP3 = (["--include-sam", 'KEEP == "1"'], lambda r: r[b"KEEP"] == b"1")
ODD = (["--include-var", 'ID != "snp7" && ID != "snp200" && ID != "snp201"'], lambda r: r[b"ID"] not in (b"snp7", b"snp200", b"snp201"))


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def allowance(v, scale, cnt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.01 * (v + 64) * 2.0 ** -53 + GR.REF_DISAGREEMENT) * scale / cnt


def reference_of(codes):
    """(GRM, N, allowance) of (V, K) codes."""
    _, cnt, grm = GR.grm_ref(codes)
    tg, _, skipped = GR.grm_tables(GR.variant_counts(codes))
    return grm, cnt, allowance(codes.shape[0], GR.gram_abs(codes, tg), cnt), skipped


def check_rel(prefix, ids, grm, tol):
    k = len(ids)
    assert Path(f"{prefix}.rel.id").read_bytes() == b"".join(i + b"\n" for i in ids)
    got = np.loadtxt(f"{prefix}.rel", delimiter="\t", ndmin=2)
    assert got.shape == (k, k) and np.array_equal(np.isnan(got), np.isnan(grm))
    ok = ~np.isnan(grm)
    worst = (np.abs(got - grm)[ok] / tol[ok]).max()
    print("rel: worst error / allowance =", worst)
    assert worst <= 1.0
    assert np.array_equal(got[ok], got.T[ok]), "the square is written from one triangle"


def check_bin(prefix, ids, grm, cnt, tol):
    k = len(ids)
    assert Path(f"{prefix}.grm.id").read_bytes() == b"".join(i + b"\t" + i + b"\n" for i in ids)
    g = np.fromfile(f"{prefix}.grm.bin", dtype="<f4").astype(np.float64)
    n = np.fromfile(f"{prefix}.grm.N.bin", dtype="<f4").astype(np.float64)
    lower = np.tril_indices(k)   # row a, then b = 0 .. a
    assert g.size == n.size == k * (k + 1) // 2
    assert np.array_equal(n, cnt[lower]), "N is an exact integer"
    want, t = grm[lower], tol[lower]
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(g), ~ok)
    worst = (np.abs(g - want)[ok] / (t[ok] + 2.0 ** -23 * np.abs(want[ok]))).max()
    print("grm-bin: worst error / allowance =", worst)
    assert worst <= 1.0


# ---- the committed fileset ----

def test_committed_fileset_both_formats(tmp_path):
    exp = json.loads((GRM / "expected.json").read_text())
    unhex = lambda m: np.array([[float.fromhex(x) for x in row] for row in m])
    grm, cnt = unhex(exp["GRM"]), np.array(exp["N"], dtype=np.float64)
    ids = [i.encode() for i in exp["ids"]]
    raw = (GRM / "g.pgen").read_bytes()
    codes = GR.unpack(np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(300, -1), 40)
    tg, _, _ = GR.grm_tables(GR.variant_counts(codes))
    tol = allowance(300, GR.gram_abs(codes, tg), cnt)
    p = run("grm", str(GRM / "g"), "--format", "rel", "-o", str(tmp_path / "g"), "--stats")
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    assert b'"variants_skipped": 3' in p.stderr and b'"variants_kept"' in p.stderr
    check_rel(tmp_path / "g", ids, grm, tol)
    p = run("grm", str(GRM / "g"), "-o", str(tmp_path / "g"))
    assert p.returncode == 0, p.stderr
    check_bin(tmp_path / "g", ids, grm, cnt, tol)
    p = run("grm", str(GRM / "g"), "--format", "rel", "--sample-tile", "16", "--block-rows", "70", "--shards", "2", "-o", str(tmp_path / "cut"))
    assert p.returncode == 0, p.stderr
    check_rel(tmp_path / "cut", ids, grm, tol)


# ---- a synthesised fileset ----

@pytest.fixture(scope="module")
def pfile(tmp_path_factory):
    prefix = tmp_path_factory.mktemp("grm") / "syn"
    p = run("synth", str(prefix), "--variants", str(V), "--samples", str(N), "--keep-modulus", "3")
    assert p.returncode == 0, p.stderr
    return prefix


_REF = {}


def reference(prefix, key, var_pred, sam_pred):
    """(IIDs of the kept samples, GRM, N, allowance, skipped variants); computed once per selection."""
    if key not in _REF:
        _, _, pvar_cols, pvar_rows = read_meta(prefix.with_suffix(".pvar"))
        _, _, psam_cols, psam_rows = read_meta(prefix.with_suffix(".psam"))
        raw = prefix.with_suffix(".pgen").read_bytes()
        assert raw[2] == 0x02 and int.from_bytes(raw[7:11], "little") == N
        r = GR.rsize(N)
        keep_v = [i for i, row in enumerate(pvar_rows) if var_pred is None or var_pred(dict(zip(pvar_cols, row)))]
        keep_s = [i for i, row in enumerate(psam_rows) if sam_pred is None or sam_pred(dict(zip(psam_cols, row)))]
        recs = np.stack([np.frombuffer(raw, dtype=np.uint8, count=r, offset=12 + vi * r) for vi in keep_v])
        iids = [psam_rows[s][psam_cols.index(b"IID")] for s in keep_s]
        _REF[key] = (iids,) + reference_of(GR.unpack(recs, N, keep_s))
    return _REF[key]


def test_all_samples_both_formats(pfile, tmp_path):
    iids, grm, cnt, tol, skipped = reference(pfile, "all", None, None)
    assert len(iids) == N
    p = run("grm", str(pfile), "--format", "rel", "-o", str(tmp_path / "a"), "--stats")
    assert p.returncode == 0, p.stderr
    assert b'"variants_skipped": %d' % skipped in p.stderr
    check_rel(tmp_path / "a", iids, grm, tol)
    p = run("grm", str(pfile), "-o", str(tmp_path / "a"))
    assert p.returncode == 0, p.stderr
    check_bin(tmp_path / "a", iids, grm, cnt, tol)


def test_sample_and_variant_filters(pfile, tmp_path):
    iids, grm, cnt, tol, _ = reference(pfile, "odd", ODD[1], KEEP3[1])
    assert len(iids) == N // 3
    p = run("grm", str(pfile), *ODD[0], *KEEP3[0], "-o", str(tmp_path / "f"))
    assert p.returncode == 0, p.stderr
    check_bin(tmp_path / "f", iids, grm, cnt, tol)


@pytest.mark.parametrize("flags", [["--sample-tile", "64"], ["--sample-tile", "37", "--block-rows", "500"], ["--block-rows", "129", "--shards", "2"],
                                   ["--shards", "2"], ["--shards", "3", "--sample-tile", "128"]])
def test_tiles_blocks_and_shards_stay_inside_the_allowance(pfile, tmp_path, flags):
    iids, grm, cnt, tol, _ = reference(pfile, "all", None, None)
    p = run("grm", str(pfile), "--format", "rel", *flags, "-o", str(tmp_path / "t"))
    assert p.returncode == 0, p.stderr
    check_rel(tmp_path / "t", iids, grm, tol)


def test_variable_width_plain_records_go_through_at(tmp_path):
    """A mode-0x10 file: the kept plain records are staged as they lie on disk and summed through their byte offsets."""
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer
    from make_grm_golden import pack_codes

    n, v = 120, 900
    rng = np.random.default_rng(2033)
    af = rng.uniform(0.05, 0.5, size=(v, 1))
    codes = (rng.random((v, n)) < af).astype(np.uint8) + (rng.random((v, n)) < af).astype(np.uint8)
    codes[rng.random((v, n)) < 0.01] = 3
    types = np.where(rng.random(v) < 0.8, 0, rng.integers(1, 8, size=v)).tolist()
    types[0] = 0
    recs = writer.make_records(rng, n, types)
    packed = pack_codes(codes)
    recs = [(ty, packed[j].tobytes() if ty == 0 else body) for j, (ty, body) in enumerate(recs)]
    data, _ = writer.write_vw(n, recs, 8, 2)
    (tmp_path / "vw.pgen").write_bytes(data)
    (tmp_path / "vw.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\tRTYPE\n" + "".join(f"22\t{1000 + j}\tv{j}\tA\tG\t{types[j]}\n" for j in range(v)))
    iids = [b"S%03d" % k for k in range(n)]
    (tmp_path / "vw.psam").write_bytes(b"#IID\tSEX\n" + b"".join(i + b"\tNA\n" for i in iids))
    grm, cnt, tol, _ = reference_of(codes[[j for j in range(v) if types[j] == 0]])
    for extra in [], ["--shards", "3", "--sample-tile", "50"]:
        p = run("grm", str(tmp_path / "vw"), "--include-var", 'RTYPE == "0"', "--format", "rel", *extra, "-o", str(tmp_path / "vw_out"))
        assert p.returncode == 0, p.stderr
        check_rel(tmp_path / "vw_out", iids, grm, tol)
    p = run("grm", str(tmp_path / "vw"), "-o", str(tmp_path / "vw_out"))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr
