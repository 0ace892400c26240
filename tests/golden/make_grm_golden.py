"""Writes tests/golden/grm: a small fileset for `pgen-hip grm` with its expected matrices.

Run from the repository root:  python tests/golden/make_grm_golden.py

  g.pgen / g.pvar / g.psam   300 variants x 40 samples, Hardy-Weinberg codes at allele frequencies 0.05 .. 0.5 from a seed, 2 % missing
                             calls; variants 7 and 150 are monomorphic (hom-ref and hom-alt in every called sample), variant 11 is missing in every
                             sample, sample 5 misses the first 60 variants
  expected.json              {"ids": [...], "skipped": 3, "G": K x K, "N": K x K, "GRM": K x K} from tests/gram_ref.py's grm_ref
                             (counts -> tables -> Z^T Z in float64 -> G / N); G and GRM as hex floats, so that nothing is lost
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import gram_ref as GR  # noqa: E402

OUT = HERE / "grm"
V, N = 300, 40


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """(V, N) codes 0..3 -> (V, R) uint8 records: sample s in byte s / 4, bits 2 * (s % 4); pad bits zero."""
    v, n = codes.shape
    padded = np.zeros((v, 4 * GR.rsize(n)), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | q[:, :, 1] << 2 | q[:, :, 2] << 4 | q[:, :, 3] << 6).astype(np.uint8)


def main():
    rng = np.random.default_rng(20261019)
    OUT.mkdir(exist_ok=True)
    af = rng.uniform(0.05, 0.5, size=V)
    codes = (rng.random((V, N)) < af[:, None]).astype(np.uint8) + (rng.random((V, N)) < af[:, None]).astype(np.uint8)
    codes[rng.random((V, N)) < 0.02] = 3
    codes[7] = 0
    codes[150] = 2
    codes[11] = 3
    codes[:60, 5] = 3
    recs = pack_codes(codes)
    assert np.array_equal(GR.unpack(recs, N), codes)
    (OUT / "g.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    (OUT / "g.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\n" + "".join(f"22\t{16050000 + 37 * j}\tv{j}\t{'ACGT'[j % 4]}\t{'CGTA'[j % 4]}\n" for j in range(V)))
    iids = [f"S{k:03d}" for k in range(N)]
    (OUT / "g.psam").write_text("#IID\tSEX\n" + "".join(f"{i}\tNA\n" for i in iids))
    g, n, grm = GR.grm_ref(codes)
    skipped = GR.grm_tables(GR.variant_counts(codes))[2]
    assert skipped == 3 and not np.isnan(grm).any()
    hexed = lambda m: [[float(x).hex() for x in row] for row in m]
    (OUT / "expected.json").write_text(json.dumps({"ids": iids, "skipped": skipped, "G": hexed(g), "N": n.astype(np.int64).tolist(), "GRM": hexed(grm)}) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
