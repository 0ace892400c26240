"""Writes tests/golden/assoc: a small fileset for `pgen-hip assoc` with its expected output, and Student t triples.

Needs scipy (the P values are scipy.stats.t.sf's); GPU machines may lack it, so the tests read P from the files written here.
Run from the repository root:  python tests/golden/make_assoc_golden.py

  g.pgen / g.pvar / g.psam   400 variants x 120 samples, Hardy-Weinberg codes at allele frequencies 0.05 .. 0.5, 1 % missing calls;
                             variant 7 is monomorphic and variant 11 is missing in every sample
  pheno.tsv, covar.tsv       two phenotypes, two covariates; a few samples with NA / nan / empty cells, one sample in neither file
  expected.json              per (variant, phenotype): OBS_CT, MISS_CT, A1_FREQ, BETA, SE, T_STAT, P (null where the CLI prints NA)
                             from tests/assoc_ref.py's closed form, P from scipy
  t_triples.json             [t, df, p] with p = 2 * scipy.stats.t.sf(t, df), df 1 .. 10^6, t 0 .. 40
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import assoc_ref as AR  # noqa: E402

OUT = HERE / "assoc"
V, N = 400, 120
T_LIST = [0.0, 1e-3, 0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 12.0, 20.0, 40.0]
DF_LIST = [1, 2, 3, 4, 5, 10, 30, 100, 117, 1000, 10_000, 100_000, 1_000_000]


def cell(x):
    return "NA" if np.isnan(x) else repr(float(x))


def read_values(path: Path, iids):
    """-> (names, (N, C) array in psam order; NaN for NA / nan / empty and for a sample the file does not hold)."""
    lines = path.read_text().split("\n")
    names = lines[0].lstrip("#").split("\t")[1:]
    out = np.full((len(iids), len(names)), np.nan)
    row = {iid: k for k, iid in enumerate(iids)}
    for ln in lines[1:]:
        if ln:
            cells = ln.split("\t")
            out[row[cells[0]]] = [np.nan if c in ("NA", "nan", "") else float(c) for c in cells[1:]]
    return names, out


def expected(codes, iids, kept, pheno, covar, names):
    stay = AR.complete_cases(kept, pheno, covar)
    ref = AR.closed_form(codes[:, stay], pheno[stay], covar[stay])
    p = AR.p_values(ref["T"], ref["df"])
    num = lambda x: None if np.isnan(x) else float(x)
    rows = []
    for j in range(codes.shape[0]):
        for c, name in enumerate(names):
            rows.append({"ID": f"v{j}", "PHENO": name, "OBS_CT": len(stay), "MISS_CT": int(ref["MISS_CT"][j]), "A1_FREQ": num(ref["A1_FREQ"][j]),
                         "BETA": num(ref["BETA"][j, c]), "SE": num(ref["SE"][j, c]), "T_STAT": num(ref["T"][j, c]), "P": num(p[j, c])})
    return rows


def main():
    from scipy import stats

    rng = np.random.default_rng(20240611)
    OUT.mkdir(exist_ok=True)
    af = rng.uniform(0.05, 0.5, size=V)
    codes = (rng.random((V, N)) < af[:, None]).astype(np.uint8) + (rng.random((V, N)) < af[:, None]).astype(np.uint8)
    codes[rng.random((V, N)) < 0.01] = 3
    codes[7] = 0
    codes[11] = 3
    recs = AR.pack_codes(codes)
    (OUT / "g.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + recs.tobytes())
    (OUT / "g.pvar").write_text("#CHROM\tPOS\tID\tREF\tALT\n" + "".join(f"22\t{16050000 + 37 * j}\tv{j}\t{'ACGT'[j % 4]}\t{'CGTA'[j % 4]}\n" for j in range(V)))
    iids = [f"S{k:03d}" for k in range(N)]
    (OUT / "g.psam").write_text("#IID\tSEX\n" + "".join(f"{i}\tNA\n" for i in iids))
    covar = np.column_stack([rng.normal(50.0, 10.0, size=N), rng.integers(0, 2, size=N).astype(np.float64)])
    dos = np.where(codes == 3, 0, codes).astype(np.float64)
    pheno = np.column_stack([0.6 * dos[3] - 0.4 * dos[100] + 0.03 * covar[:, 0] + rng.normal(size=N),
                             170.0 + 4.0 * covar[:, 1] + 1.5 * dos[250] + rng.normal(scale=6.0, size=N)])
    pheno[5, 0] = np.nan
    pheno[17, 1] = np.nan
    covar[40, 1] = np.nan
    order = rng.permutation(N)   # the files' order is not the .psam's
    lines = ["#IID\tY1\tY2"]
    for k in order:
        if k == 77:
            continue             # a sample the pheno file does not hold
        cells = [cell(pheno[k, 0]), cell(pheno[k, 1])]
        if k == 17:
            cells[1] = ""        # an empty cell is missing
        if k == 5:
            cells[0] = "nan"
        lines.append("\t".join([iids[k]] + cells))
    (OUT / "pheno.tsv").write_text("\n".join(lines) + "\n")
    (OUT / "covar.tsv").write_text("IID\tAGE\tSEX\n" + "".join("\t".join([iids[k], cell(covar[k, 0]), cell(covar[k, 1])]) + "\n" for k in order[::-1]))
    # what the files hold is what the CLI reads: parse them back so that the expectation sees the printed digits
    names, ph = read_values(OUT / "pheno.tsv", iids)
    _, cv = read_values(OUT / "covar.tsv", iids)
    (OUT / "expected.json").write_text(json.dumps(expected(codes, iids, list(range(N)), ph, cv, names), indent=0) + "\n")
    triples = [[t, df, float(2.0 * stats.t.sf(t, df))] for df in DF_LIST for t in T_LIST]
    (OUT / "t_triples.json").write_text(json.dumps(triples) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
