"""GPU leg of `pgen-hip pca`: end to end (metadata filter -> a pass of genotype counts -> tables -> passes of Gram products over blocks
of variants and shards -> Rayleigh-Ritz on the host -> files) against numpy's eigh of the same matrix (tests/pca_ref.py).

Allowances, from the stop rule |r_i| <= tol lambda_1 (r_i the residual of Ritz pair i):
  eigenvalues   |lambda_i - ref_i| <= 2 tol lambda_1: a Ritz value lies within its residual of an eigenvalue; the factor 2 covers the
                residual being evaluated in rounded arithmetic (the kernel's own rounding, (V + K + 4) 2^-53 relative, is about 1e-13
                here, four orders below tol = 1e-9);
  eigenvectors  sign-aligned, |u_i - ref_i|_2 <= 2 sqrt(2) tol lambda_1 / gap_i, gap_i the distance to the nearest other reference
                eigenvalue (Davis-Kahan, the same factor 2);
  unit norms and mutual orthogonality to the eigenvectors' allowance (the larger of the two vectors').
Every case prints its worst fraction of each allowance."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gram_ref as GR
import pca_ref as PR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
PCA = GOLDEN / "pca"
TOL = 1e-9


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def golden_codes():
    raw = (PCA / "p.pgen").read_bytes()
    v, n = int.from_bytes(raw[3:7], "little"), int.from_bytes(raw[7:11], "little")
    return GR.unpack(np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(v, -1), n)


def read_out(prefix, pcs):
    lam = np.loadtxt(f"{prefix}.eigenval", ndmin=1)
    lines = Path(f"{prefix}.eigenvec").read_text().splitlines()
    assert lines[0] == "#IID\t" + "\t".join(f"PC{i + 1}" for i in range(pcs))
    ids = [ln.split("\t")[0] for ln in lines[1:]]
    vec = np.array([[float(x) for x in ln.split("\t")[1:]] for ln in lines[1:]]).reshape(len(ids), pcs)
    assert lam.shape == (pcs,)
    return lam, ids, vec


def stats_of(p):
    line = [ln for ln in p.stderr.decode().splitlines() if ln.startswith('{"variants_skipped"')]
    assert len(line) == 1, p.stderr
    return json.loads(line[0])


def check(prefix, ids, codes, pcs, tol, compare=None, what=""):
    """The files under `prefix` against eigh of the (V, K) codes' matrix; compare: how many leading components (default: all written)."""
    m, skipped = PR.m_matrix(codes)
    ref_lam, ref_vec = PR.eigh_ref(m)
    lam, got_ids, vec = read_out(prefix, pcs)
    assert got_ids == ids
    n = pcs if compare is None else compare
    gaps = np.array([min(abs(ref_lam[i] - ref_lam[j]) for j in range(len(ref_lam)) if j != i) for i in range(n)])
    assert (gaps >= 0.05 * ref_lam[0]).all(), "the compared components are not separated"
    f_val = (np.abs(lam[:n] - ref_lam[:n]) / (2 * tol * ref_lam[0])).max()
    allow = 2 * np.sqrt(2) * tol * ref_lam[0] / gaps
    u = PR.align(vec[:, :n], ref_vec[:, :n])
    f_vec = (np.linalg.norm(u - ref_vec[:, :n], axis=0) / allow).max()
    gram = vec[:, :n].T @ vec[:, :n] - np.eye(n)
    f_orth = (np.abs(gram) / np.maximum(allow[:, None], allow[None, :])).max()
    print(f"pca {what}: worst fraction of the allowance: eigenvalues {f_val:.3g}, eigenvectors {f_vec:.3g}, norms and orthogonality {f_orth:.3g}")
    assert f_val <= 1.0 and f_vec <= 1.0 and f_orth <= 1.0
    assert (np.abs(vec).max(axis=0) == vec.max(axis=0)).all(), "the largest-magnitude entry of every vector is positive"
    return skipped


def test_committed_fileset(tmp_path):
    exp = json.loads((PCA / "expected.json").read_text())
    codes = golden_codes()
    p = run("pca", str(PCA / "p"), "--pcs", "2", "--tol", "1e-9", "-o", str(tmp_path / "p"), "--stats")
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    skipped = check(tmp_path / "p", exp["ids"], codes, 2, TOL, what="committed fileset")
    st = stats_of(p)
    assert st["variants_skipped"] == skipped == exp["skipped"] and st["converged"] is True and 1 <= st["passes"] <= 30 and st["residual"] <= TOL
    assert b'"variants_kept": 600' in p.stderr
    # the committed eigenvalues and vectors themselves
    lam, _, vec = read_out(tmp_path / "p", 2)
    want = np.array([float.fromhex(x) for x in exp["eigenvalues"]])
    ref = np.array([[float.fromhex(x) for x in col] for col in exp["vectors"]]).T
    assert (np.abs(lam - want[:2]) <= 2 * TOL * want[0]).all()
    gap = min(want[0] - want[1], want[1] - want[2])
    assert (np.linalg.norm(PR.align(vec, ref) - ref, axis=0) <= 2 * np.sqrt(2) * TOL * want[0] / gap).all()


def test_sample_and_variant_filters(tmp_path):
    codes = golden_codes()
    drop_s, drop_v = [5, 50, 100, 119], [7, 200, 201]
    sam = " && ".join(f'IID != "S{k:03d}"' for k in drop_s)
    var = " && ".join(f'ID != "v{j}"' for j in drop_v)
    keep_s = [k for k in range(120) if k not in drop_s]
    keep_v = [j for j in range(600) if j not in drop_v]
    p = run("pca", str(PCA / "p"), "--include-sam", sam, "--include-var", var, "--pcs", "2", "--tol", "1e-9", "-o", str(tmp_path / "f"))
    assert p.returncode == 0, p.stderr
    check(tmp_path / "f", [f"S{k:03d}" for k in keep_s], codes[keep_v][:, keep_s], 2, TOL, what="filters")


@pytest.mark.parametrize("flags", [["--block-rows", "70"], ["--shards", "2"], ["--shards", "3", "--block-rows", "129"]])
def test_blocks_and_shards_stay_inside_the_allowance(tmp_path, flags):
    ids = json.loads((PCA / "expected.json").read_text())["ids"]
    p = run("pca", str(PCA / "p"), "--pcs", "2", "--tol", "1e-9", *flags, "-o", str(tmp_path / "c"))
    assert p.returncode == 0, p.stderr
    check(tmp_path / "c", ids, golden_codes(), 2, TOL, what=" ".join(flags))


def test_two_seeds_agree_within_the_allowances(tmp_path):
    ids = json.loads((PCA / "expected.json").read_text())["ids"]
    outs = []
    for seed in ("1", "20261019"):
        p = run("pca", str(PCA / "p"), "--pcs", "2", "--tol", "1e-9", "--seed", seed, "-o", str(tmp_path / f"s{seed}"))
        assert p.returncode == 0, p.stderr
        check(tmp_path / f"s{seed}", ids, golden_codes(), 2, TOL, what=f"seed {seed}")
        outs.append(read_out(tmp_path / f"s{seed}", 2))
    assert not np.array_equal(outs[0][2], outs[1][2]), "the seed does not reach the start matrix"


def test_not_converged_is_reported_and_written(tmp_path):
    """Four components reach into the bulk (gaps of 0.003 lambda_1): three passes cannot reach tol."""
    p = run("pca", str(PCA / "p"), "--pcs", "4", "--tol", "1e-9", "--max-passes", "3", "-o", str(tmp_path / "n"), "--stats")
    assert p.returncode == 0 and b"warning" in p.stderr, p.stderr
    st = stats_of(p)
    assert st["converged"] is False and st["passes"] == 3 and st["residual"] > TOL
    lam, ids, vec = read_out(tmp_path / "n", 4)
    assert len(ids) == 120 and np.isfinite(lam).all() and (np.diff(lam) <= 0).all()
    assert np.allclose(np.linalg.norm(vec, axis=0), 1.0, atol=1e-12)


def test_variable_width_plain_records_go_through_at(tmp_path):
    """A mode-0x10 file: the kept plain records are staged as they lie on disk and multiplied through their byte offsets."""
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer
    from make_grm_golden import pack_codes

    codes = golden_codes()
    v, n = codes.shape
    rng = np.random.default_rng(2034)
    types = np.where(rng.random(v) < 0.8, 0, rng.integers(1, 8, size=v)).tolist()
    types[0] = 0
    recs = writer.make_records(rng, n, types)
    packed = pack_codes(codes)
    recs = [(ty, packed[j].tobytes() if ty == 0 else body) for j, (ty, body) in enumerate(recs)]
    data, _ = writer.write_vw(n, recs, 8, 2)
    (tmp_path / "vw.pgen").write_bytes(data)
    (tmp_path / "vw.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\tRTYPE\n" + "".join(f"22\t{1000 + j}\tv{j}\tA\tG\t{types[j]}\n" for j in range(v)))
    ids = [f"S{k:03d}" for k in range(n)]
    (tmp_path / "vw.psam").write_text("#IID\tSEX\n" + "".join(f"{i}\tNA\n" for i in ids))
    plain = codes[[j for j in range(v) if types[j] == 0]]
    for extra in [], ["--shards", "3"]:
        p = run("pca", str(tmp_path / "vw"), "--include-var", 'RTYPE == "0"', "--pcs", "2", "--tol", "1e-9", *extra, "-o", str(tmp_path / "vw_out"))
        assert p.returncode == 0, p.stderr
        check(tmp_path / "vw_out", ids, plain, 2, TOL, what="mode 0x10 " + " ".join(extra))


def test_planted_3000_by_300_spans_two_column_groups(tmp_path):
    """3 populations of 100 over 3 000 variants at F_ST = 0.05: --pcs 8 gives L = 18 columns, two Gram products per block.  Six of the
    eight components lie in the bulk, so the iteration runs at --tol 1e-3 (39 passes in the numpy twin) and only the two separated
    components are compared, to that tolerance's allowances."""
    from make_grm_golden import pack_codes

    v, pops, per, fst = 3000, 3, 100, 0.05
    n = pops * per
    rng = np.random.default_rng(7)
    anc = rng.uniform(0.1, 0.9, size=v)
    freq = rng.beta((anc * (1 - fst) / fst)[:, None], ((1 - anc) * (1 - fst) / fst)[:, None], size=(v, pops))
    af = np.repeat(freq, per, axis=1)
    codes = (rng.random((v, n)) < af).astype(np.uint8) + (rng.random((v, n)) < af).astype(np.uint8)
    codes[rng.random((v, n)) < 0.01] = 3
    recs = pack_codes(codes)
    (tmp_path / "s.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    (tmp_path / "s.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\n" + "".join(f"22\t{1000 + j}\tv{j}\tA\tG\n" for j in range(v)))
    ids = [f"S{k:03d}" for k in range(n)]
    (tmp_path / "s.psam").write_text("#IID\tSEX\n" + "".join(f"{i}\tNA\n" for i in ids))
    p = run("pca", str(tmp_path / "s"), "--pcs", "8", "--tol", "1e-3", "--block-rows", "1000", "-o", str(tmp_path / "s_out"), "--stats")
    assert p.returncode == 0, p.stderr
    st = stats_of(p)
    assert st["converged"] is True and st["passes"] <= 100, st
    check(tmp_path / "s_out", ids, codes, 8, 1e-3, compare=2, what="planted 3000 x 300, L = 18")
