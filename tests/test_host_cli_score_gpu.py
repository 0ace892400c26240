"""GPU leg of `pgen-hip score`: polygenic scores end to end (weights file -> ID match among the kept variants -> matched records
staged to HBM -> per block the mean dosages from the variant counts, the score kernel and the sample counts -> K x C doubles back
per shard) against tests/score_ref.py fed the same f32 weights and the same f32 mean-dosage formula.

ALLELE_CT and DENOM must be exact.  A sum S may differ from the correctly rounded reference by
    1.01 (M + 64) 2^-53 A  +  5e-12 |S|
: the bound of any summation order of the M exact terms (score_ref.bound) with slack for the additions of blocks, shards and the
host's constant, and the rounding of the printed %.12g."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pgen_oracle as oracle
import score_ref as SR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
V, N = 3000, 300
POS_CUT = 16050000 + 7 * 2500        # --include-var keeps the variants in front of it


def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, timeout=300)


def make_weights(path: Path, ids, ref, alt, n_scores, seed):
    """A weights file over `ids`: ~40 % of the variants, a third of them naming REF, a few naming neither allele, some unknown IDs.
    -> {id: (allele, [f32 weights])} of every row."""
    rng = np.random.default_rng(seed)
    rows = {}
    lines = ["#ID\tA1\t" + "\t".join(f"PRS{c}" for c in range(n_scores))]
    picks = sorted(rng.choice(len(ids), size=len(ids) * 2 // 5, replace=False).tolist())
    entries = [(ids[i], (ref[i] if rng.random() < 0.33 else alt[i]) if rng.random() > 0.02 else "T") for i in picks]
    entries += [(f"unknown{i}", "G") for i in range(20)]
    order = rng.permutation(len(entries))    # the file's order is not the .pvar's
    for e in order:
        vid, allele = entries[e]
        cells = ["%.7g" % (rng.normal() * 10.0 ** rng.integers(-3, 3)) for _ in range(n_scores)]
        rows[vid] = (allele, [np.float32(float(c)) for c in cells])
        lines.append("\t".join([vid, allele] + cells))
    path.write_text("\n".join(lines) + "\n")
    return rows


def read_plain(prefix: Path):
    """-> (ids, ref, alt, iids, keep flags or None, records (V, R), N) of a fileset whose kept records are plain."""
    def table(p):
        rows = [ln.split("\t") for ln in p.read_text().split("\n") if ln and not ln.startswith("##")]
        return [c.lstrip("#") for c in rows[0]], rows[1:]
    vc, vr = table(prefix.with_suffix(".pvar"))
    sc, sr = table(prefix.with_suffix(".psam"))
    raw = prefix.with_suffix(".pgen").read_bytes()
    if raw[2] == 0x02:
        n = int.from_bytes(raw[7:11], "little")
        r = (2 * n + 7) // 8
        recs = np.frombuffer(raw, dtype=np.uint8, offset=12).reshape(len(vr), r)
        plain = np.ones(len(vr), dtype=bool)
    else:
        rc, h = oracle.vw_parse_header(raw[:12])
        assert rc == 0
        rc, types, lens, offs = oracle.vw_index(h, raw)
        assert rc == 0
        n = int(h.sample_count)
        r = (2 * n + 7) // 8
        plain = (np.asarray(types) == 0) & (np.asarray(lens) == r)
        recs = np.stack([np.frombuffer(raw, dtype=np.uint8, count=r, offset=int(offs[i])) if plain[i] else np.zeros(r, np.uint8) for i in range(len(vr))])
    col = lambda cols, rows, name: [row[cols.index(name)] for row in rows]
    keep = [k == "1" for k in col(sc, sr, "KEEP")] if "KEEP" in sc else None
    return col(vc, vr, "ID"), col(vc, vr, "REF"), col(vc, vr, "ALT"), col(sc, sr, "IID"), keep, recs, n, plain, col(vc, vr, "POS")


def expected(meta, rows, n_scores, var_kept, sam_kept, impute):
    """-> (iids, ALLELE_CT, DENOM, S, A) of the kept samples by the issue's definition: the matched variants in .pvar order, -w for
    REF-effect rows plus the constant sum of 2w, miss[j] = f32((c1 + 2 c2) / (c0 + c1 + c2)) over the kept samples."""
    ids, ref, alt, iids, _, recs, n, _, _ = meta
    sel, w, const = [], [], np.zeros(n_scores)
    for i in var_kept:
        if ids[i] in rows and rows[ids[i]][0] in (ref[i], alt[i]):
            allele, ws = rows[ids[i]]
            flip = allele != alt[i]
            sel.append(i)
            w.append([-x if flip else x for x in ws])
            if flip:
                const += 2.0 * np.array(ws, dtype=np.float64)
    m = len(sel)
    codes = SR.unpack_codes(recs[sel], n)[:, sam_kept]
    miss = None
    if impute:
        c1, c2, called = (codes == 1).sum(axis=1), (codes == 2).sum(axis=1), (codes != 3).sum(axis=1)
        miss = np.where(called > 0, (c1 + 2 * c2) / np.maximum(called, 1), 0.0).astype(np.float32)
    s, a = SR.score_from_codes(codes, np.array(w, dtype=np.float32), miss)
    allele_ct = 2 * (m - (codes == 3).sum(axis=0))
    denom = np.full(len(sam_kept), 2 * m) if impute else allele_ct
    return [iids[k] for k in sam_kept], allele_ct, denom, s + const, a + np.abs(const), m


def check(stdout: bytes, want, n_scores, avg=False):
    iids, allele_ct, denom, s, a, m = want
    lines = stdout.decode().split("\n")
    assert lines[-1] == "" and lines[0] == "#IID\tALLELE_CT\tDENOM\t" + "\t".join(f"PRS{c}_{'AVG' if avg else 'SUM'}" for c in range(n_scores))
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert [b[0] for b in body] == iids
    assert [int(b[1]) for b in body] == allele_ct.tolist(), "ALLELE_CT"
    assert [int(b[2]) for b in body] == denom.tolist(), "DENOM"
    got = np.array([[float(x) for x in b[3:]] for b in body]).reshape(len(iids), n_scores)
    d = denom[:, None].astype(np.float64)
    ref = s / d if avg else s
    lim = SR.bound(m + 63, a) / (d if avg else 1.0) + 5e-12 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"M = {m}: max |got - ref| / bound = {np.max(err / np.maximum(lim, 1e-300)):.3g}")
    assert (err <= lim).all()
    return m


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("score")
    p = run("synth", str(d / "s"), "--variants", str(V), "--samples", str(N), "--keep-modulus", "3")
    assert p.returncode == 0, p.stderr
    meta = read_plain(d / "s")
    rows3 = make_weights(d / "w3.tsv", meta[0], meta[1], meta[2], 3, 1)
    rows9 = make_weights(d / "w9.tsv", meta[0], meta[1], meta[2], 9, 2)
    return d, meta, rows3, rows9


VAR_FLAGS = ["--include-var", f'POS < "{POS_CUT}"']


@pytest.mark.parametrize("case", ["default", "no_imputation", "avg", "avg_no_imputation", "kept_samples", "shards", "blocks", "nine_scores"])
def test_scores_match_the_reference(synth, case):
    d, meta, rows3, rows9 = synth
    pos, keep = meta[8], meta[4]
    var_kept = [i for i in range(V) if int(pos[i]) < POS_CUT]
    assert 0 < len(var_kept) < V
    sam_kept = list(range(N))
    flags, impute, avg, rows, wfile, c = list(VAR_FLAGS), True, False, rows3, "w3.tsv", 3
    if case in ("no_imputation", "avg_no_imputation"):
        flags.append("--no-mean-imputation")
        impute = False
    if case in ("avg", "avg_no_imputation"):
        flags.append("--avg")
        avg = True
    if case == "kept_samples":
        flags += ["--include-sam", 'KEEP == "1"']
        sam_kept = [k for k in range(N) if keep[k]]
        assert 0 < len(sam_kept) < N
    if case == "shards":
        flags += ["--shards", "3"]
    if case == "blocks":      # R = 75 bytes: a 1-MiB block would hold every row, so cut the rows with shards of their own blocks
        flags += ["--shards", "7", "--include-sam", 'IID != "S000005"']
        sam_kept = [k for k in range(N) if k != 5]
    if case == "nine_scores":  # two column groups: 8 + 1
        rows, wfile, c = rows9, "w9.tsv", 9
    p = run("score", str(d / "s"), "--weights", str(d / wfile), *flags, "--stats")
    assert p.returncode == 0, p.stderr
    want = expected(meta, rows, c, var_kept, sam_kept, impute)
    m = check(p.stdout, want, c, avg)
    stats = p.stderr.decode()
    flipped = sum(1 for i in var_kept if meta[0][i] in rows and rows[meta[0][i]][0] == meta[1][i])
    assert f'"weights_matched": {m}, "weights_flipped": {flipped}, "weights_skipped": {len(rows) - m}' in stats, stats
    assert 0 < flipped < m < len(rows) - 20


def test_output_file_equals_stdout(synth, tmp_path):
    d = synth[0]
    out = tmp_path / "s.sscore"
    a = run("score", str(d / "s"), "--weights", str(d / "w3.tsv"), "--include-sam", 'KEEP == "1"', "--no-mean-imputation")
    b = run("score", str(d / "s"), "--weights", str(d / "w3.tsv"), "--include-sam", 'KEEP == "1"', "--no-mean-imputation", "-o", str(out))
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    # integer-free sums in another order may differ in the last printed digit: compare the exact columns and the shape
    la, lb = a.stdout.split(b"\n"), out.read_bytes().split(b"\n")
    assert len(la) == len(lb) and [x.split(b"\t")[:3] for x in la] == [x.split(b"\t")[:3] for x in lb]


@pytest.fixture(scope="module")
def vw_pfile(tmp_path_factory):
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    d = tmp_path_factory.mktemp("vwscore")
    n, v = 2504, 1500
    rng = np.random.default_rng(2031)
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


def test_variable_width_plain_records_go_through_at(vw_pfile):
    """A mode-0x10 file: the matched plain records are staged as they lie on disk and scored through their byte offsets."""
    meta = read_plain(vw_pfile)
    ids, ref, alt, plain = meta[0], meta[1], meta[2], meta[7]
    rng = np.random.default_rng(9)
    rows = {}
    lines = ["ID\tA1\tPRS0\tPRS1"]
    for i in range(len(ids)):
        if plain[i] and rng.random() < 0.5:
            allele = ref[i] if rng.random() < 0.3 else alt[i]
            cells = ["%.7g" % rng.normal() for _ in range(2)]
            rows[ids[i]] = (allele, [np.float32(float(c)) for c in cells])
            lines.append("\t".join([ids[i], allele] + cells))
    wfile = vw_pfile.parent / "w.tsv"
    wfile.write_text("\n".join(lines) + "\n")
    var_kept = [i for i in range(len(ids)) if plain[i]]
    for extra, sam_kept in ([], list(range(meta[6]))), (["--include-sam", 'IID != "S0007"', "--shards", "3"], [k for k in range(meta[6]) if k != 7]):
        p = run("score", str(vw_pfile), "--weights", str(wfile), "--include-var", 'RTYPE == "0"', *extra)
        assert p.returncode == 0, p.stderr
        check(p.stdout, expected(meta, rows, 2, var_kept, sam_kept, True), 2)
    # a matched record that is stored compressed is refused like everywhere else
    cid = next(ids[i] for i in range(len(ids)) if not plain[i])
    wfile.write_text(f"ID\tA1\tPRS0\n{cid}\tT\t1\n")
    p = run("score", str(vw_pfile), "--weights", str(wfile))
    assert p.returncode == 101 and b"stored compressed" in p.stderr, p.stderr
