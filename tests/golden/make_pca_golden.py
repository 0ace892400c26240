"""Writes tests/golden/pca: a small fileset with population structure for `pgen-hip pca`, and its expected decomposition.

Run from the repository root:  python tests/golden/make_pca_golden.py   (numpy only)

  p.pgen / p.pvar / p.psam   600 variants x 120 samples: 3 populations of 40 (psam column POP), allele frequencies by Balding-Nichols
                             with F_ST = 0.1 around ancestral p ~ U(0.1, 0.9), Hardy-Weinberg codes, 1 % missing calls
  expected.json              {"ids", "skipped", "eigenvalues": all K by numpy's eigh of M (tests/pca_ref.py), "vectors": the first two
                             eigenvectors}, as hex floats

The generator asserts what the CLI tests rely on: the two leading eigenvalues are separated from each other and from the bulk by
a relative gap of at least 0.05 lambda_1, and the numpy twin of the host algorithm reaches tol = 1e-9 within 30 passes."""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import gram_ref as GR  # noqa: E402
import pca_ref as PR  # noqa: E402
from make_grm_golden import pack_codes  # noqa: E402

OUT = HERE / "pca"
V, POPS, PER = 600, 3, 40
N = POPS * PER
FST = 0.1


def main():
    rng = np.random.default_rng(20261019)
    OUT.mkdir(exist_ok=True)
    anc = rng.uniform(0.1, 0.9, size=V)
    a = anc * (1 - FST) / FST
    b = (1 - anc) * (1 - FST) / FST
    freq = rng.beta(a[:, None], b[:, None], size=(V, POPS))          # Balding-Nichols
    af = np.repeat(freq, PER, axis=1)
    codes = (rng.random((V, N)) < af).astype(np.uint8) + (rng.random((V, N)) < af).astype(np.uint8)
    codes[rng.random((V, N)) < 0.01] = 3
    recs = pack_codes(codes)
    assert np.array_equal(GR.unpack(recs, N), codes)
    (OUT / "p.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    (OUT / "p.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\n" + "".join(f"22\t{16050000 + 37 * j}\tv{j}\t{'ACGT'[j % 4]}\t{'CGTA'[j % 4]}\n" for j in range(V)))
    iids = [f"S{k:03d}" for k in range(N)]
    (OUT / "p.psam").write_text("#IID\tSEX\tPOP\n" + "".join(f"{i}\tNA\t{k // PER}\n" for k, i in enumerate(iids)))
    m, skipped = PR.m_matrix(codes)
    lam, vec = PR.eigh_ref(m)
    gaps = [lam[0] - lam[1], lam[1] - lam[2]]
    assert min(gaps) >= 0.05 * lam[0], (lam[:4], gaps)
    tl, tu, passes, res, converged = PR.twin(m, 2, tol=1e-9, max_passes=30)
    assert converged and passes <= 30, (passes, res)
    dev_val = np.abs(tl - lam[:2]).max() / lam[0]
    dev_vec = np.linalg.norm(PR.align(tu, vec[:, :2]) - vec[:, :2], axis=0).max()
    print(f"lambda = {lam[:4]}, relative gaps = {[g / lam[0] for g in gaps]}, skipped = {skipped}")
    print(f"twin: {passes} passes, eigenvalue deviation {dev_val:.3g} lambda_1, eigenvector deviation {dev_vec:.3g}")
    (OUT / "expected.json").write_text(json.dumps({"ids": iids, "skipped": skipped, "eigenvalues": [float(x).hex() for x in lam],
                                                   "vectors": [[float(x).hex() for x in vec[:, i]] for i in range(2)]}) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
