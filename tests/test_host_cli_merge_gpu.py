"""GPU leg of `pgen-hip merge`: filesets joined end to end (metadata matched on the host -> each input's records staged to HBM -> join
kernel -> rows written with pwrite), the three output files byte-equal to tests/merge_ref.py + tests/join_ref.py on the inputs' files,
and read back through `filter` and `freq`."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import join_ref as JR
import merge_ref as MR
import pack_ref as PR
import pgen_oracle as oracle
from helpers import GOLDEN, plain_record_filesets
from ref_vcf import expected_vcf

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"


def run(*args):
    return subprocess.run([str(CLI), *map(str, args)], capture_output=True, timeout=300)


def ext(prefix, e):
    return Path(str(prefix) + e)


def load(prefix):
    """A fileset as the references take it."""
    out = {"prefix": prefix}
    for kind in ("pvar", "psam"):
        lines = ext(prefix, "." + kind).read_text().split("\n")
        if lines[-1] == "":
            lines.pop()
        n_head = next((i for i, ln in enumerate(lines) if not ln.startswith("#")), len(lines))
        out[kind] = {"head": "".join(ln + "\n" for ln in lines[:n_head]), "col": lines[n_head - 1], "rows": lines[n_head:], "first_line": n_head + 1}
    raw = ext(prefix, ".pgen").read_bytes()
    out["raw"] = np.frombuffer(raw, dtype=np.uint8)
    if raw[2] == 0x02:
        out["n"] = int.from_bytes(raw[7:11], "little")
        r = (out["n"] + 3) // 4
        out["offs"] = [12 + i * r for i in range(int.from_bytes(raw[3:7], "little"))]
    else:
        rc, h = oracle.vw_parse_header(raw[:12])
        assert rc == 0
        rc, _types, _lens, offs = oracle.vw_index(h, raw)
        assert rc == 0
        out["n"], out["offs"] = int(h.sample_count), [int(o) for o in offs]
    return out


def expected(prefixes, union=False):
    """-> (the three files' bytes, the matching)"""
    sets = [load(p) for p in prefixes]
    tables = [(str(ext(s["prefix"], ".pvar")), s["pvar"]["col"], s["pvar"]["rows"]) for s in sets]
    MR.check_samples([(str(ext(s["prefix"], ".psam")), s["psam"]["col"], s["psam"]["rows"]) for s in sets])
    m = MR.match(tables, union=union)
    v = len(m["rows"])
    parts = [(s["raw"], [s["offs"][r] if r >= 0 else JR.ABSENT for r in m["src"][p]], s["n"], np.array(m["flip"][p], dtype=np.uint8))
             for p, s in enumerate(sets)]
    n = sum(s["n"] for s in sets)
    pgen = PR.pgen_file(JR.join(parts, v), n)
    pvar = sets[0]["pvar"]["head"] + "".join(sets[fi]["pvar"]["rows"][fr] + "\n" for fi, fr in m["rows"])
    psam = sets[0]["psam"]["head"] + "".join(row + "\n" for s in sets for row in s["psam"]["rows"])
    return (pgen, pvar.encode(), psam.encode()), m, n


def check(out, want):
    for e, w in zip((".pgen", ".pvar", ".psam"), want):
        got = ext(out, e).read_bytes()
        assert len(got) == len(w) and got == w, e


def write_fileset(prefix, pvar_head, pvar_rows, psam_head, psam_rows, codes):
    ext(prefix, ".pgen").write_bytes(PR.pgen_file(PR.pack_codes(codes), codes.shape[1]))
    ext(prefix, ".pvar").write_text(pvar_head + "".join(r + "\n" for r in pvar_rows))
    ext(prefix, ".psam").write_text(psam_head + "".join(r + "\n" for r in psam_rows))
    return prefix


V, N, CUT = 3000, 2504, 1001


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """The synthetic 3 000 x 2 504 fileset on golden basic1 metadata, and its codes."""
    d = tmp_path_factory.mktemp("merge")
    lines = (GOLDEN / "basic1" / "basic1.pvar").read_text().split("\n")
    n_head = next(i for i, ln in enumerate(lines) if not ln.startswith("#"))
    sam = (GOLDEN / "basic1" / "basic1.psam").read_text().split("\n")
    recs = oracle.synth_records(N, V).reshape(V, (N + 3) // 4)
    codes = PR.unpack(recs, N)
    meta = {"pvar_head": "".join(ln + "\n" for ln in lines[:n_head]), "pvar_rows": lines[n_head:n_head + V], "psam_head": sam[0] + "\n",
            "psam_rows": sam[1:1 + N], "codes": codes, "dir": d}
    meta["prefix"] = write_fileset(d / "whole", meta["pvar_head"], meta["pvar_rows"], meta["psam_head"], meta["psam_rows"], codes)
    meta["a"] = write_fileset(d / "half_a", meta["pvar_head"], meta["pvar_rows"], meta["psam_head"], meta["psam_rows"][:CUT], codes[:, :CUT])
    meta["b"] = write_fileset(d / "half_b", meta["pvar_head"], meta["pvar_rows"], meta["psam_head"], meta["psam_rows"][CUT:], codes[:, CUT:])
    return meta


def test_round_trip_of_the_halves(whole, tmp_path):
    want = tuple(ext(whole["prefix"], e).read_bytes() for e in (".pgen", ".pvar", ".psam"))
    out = tmp_path / "o"
    p = run("merge", whole["a"], whole["b"], "-o", out, "--stats")
    assert p.returncode == 0, p.stderr
    check(out, want)
    stats = json.loads(p.stderr.decode().strip().splitlines()[-1])
    ref, m, n = expected([whole["a"], whole["b"]])
    assert ref == want
    assert {k: stats[k] for k in MR.counts_json(m, n)} == MR.counts_json(m, n) and stats["seconds_kernel"] > 0
    # several blocks give the same bytes
    out2 = tmp_path / "o2"
    p = run("merge", whole["a"], whole["b"], "-o", out2, "--block-mib", "1", "--read-threads", "2")
    assert p.returncode == 0, p.stderr
    check(out2, want)
    # the halves as `export --include-sam` writes them
    pivot = whole["psam_rows"][CUT].split("\t")[0]
    ea, eb = tmp_path / "ea", tmp_path / "eb"
    assert run("export", whole["prefix"], "--include-sam", f'IID < "{pivot}"', "-o", ea).returncode == 0
    assert run("export", whole["prefix"], "--include-sam", f'IID >= "{pivot}"', "-o", eb).returncode == 0
    assert ext(ea, ".psam").read_bytes() == ext(whole["a"], ".psam").read_bytes()
    out3 = tmp_path / "o3"
    p = run("merge", ea, eb, "-o", out3)
    assert p.returncode == 0, p.stderr
    check(out3, want)


@pytest.fixture(scope="module")
def shuffled(whole):
    """A second fileset of 37 other samples: a subset of the variants in another order, every third of its rows with REF and ALT
    exchanged (its records are random codes: the join must exchange 0 and 2 in exactly those rows), some IDs changed, and a few
    variants of its own."""
    rng = np.random.default_rng(5)
    d = whole["dir"]
    pick = rng.permutation(V)[:1700]
    n2 = 37
    codes = rng.integers(0, 4, size=(len(pick) + 5, n2), dtype=np.uint8)
    rows = []
    for k, i in enumerate(pick):
        f = whole["pvar_rows"][i].split("\t")
        if k % 3 == 0:
            f[3], f[4] = f[4], f[3]
        if k % 50 == 0:
            f[2] = f"renamed{k}"
        rows.append("\t".join(f))
    rows += [f"{c}\t{1000 + k}\town{k}\tA\tC\t100\tPASS\t." for k, c in enumerate((19, 19, "X", 19, "X"))]
    psam_rows = [f"T{k:04d}\tNA" for k in range(n2)]
    return write_fileset(d / "shuffled", whole["pvar_head"], rows, whole["psam_head"], psam_rows, codes)


def test_intersection_with_differing_row_orders_and_flips(whole, shuffled, tmp_path):
    for order in ((whole["a"], shuffled), (shuffled, whole["a"])):
        want, m, n = expected(order)
        assert len(m["rows"]) == 1700 and sum(m["flipped"]) == 567 and m["id_conflicts"] == 34
        out = tmp_path / "o"
        p = run("merge", *order, "-o", out, "--stats", "--block-mib", "1")
        assert p.returncode == 0, p.stderr
        check(out, want)
        stats = json.loads(p.stderr.decode().strip().splitlines()[-1])
        assert {k: stats[k] for k in MR.counts_json(m, n)} == MR.counts_json(m, n)


def test_union_marks_the_missing_side(whole, shuffled, tmp_path):
    want, m, n = expected((shuffled, whole["b"]), union=True)
    assert len(m["rows"]) == V + 5 and m["absent"] == [V - 1700, 5]
    out = tmp_path / "o"
    p = run("merge", shuffled, whole["b"], "-o", out, "--union", "--stats")
    assert p.returncode == 0, p.stderr
    check(out, want)
    stats = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert stats["absent"] == m["absent"] and stats["variants"] == V + 5
    # the absent samples are code 3
    recs = np.frombuffer(want[0][12:], dtype=np.uint8).reshape(V + 5, -1)
    codes = PR.unpack(recs, n)
    for p_, (lo, hi) in enumerate(((0, 37), (37, n))):
        gone = np.array(m["src"][p_]) < 0
        assert gone.any() and (codes[gone, lo:hi] == 3).all()
    # read back: filter gives the VCF the oracle writes for the expected fileset, and freq runs
    exp = tmp_path / "exp"
    for e, w in zip((".pgen", ".pvar", ".psam"), want):
        ext(exp, e).write_bytes(w)
    vcf = tmp_path / "o.vcf"
    p = run("filter", out, "-o", vcf)
    assert p.returncode == 0, p.stderr
    assert vcf.read_bytes() == expected_vcf(exp)
    p = run("freq", out, "-o", tmp_path / "o.freq")
    assert p.returncode == 0, p.stderr
    assert len((tmp_path / "o.freq").read_bytes().splitlines()) == V + 5 + 1


def test_three_inputs_one_of_them_variable_width(tmp_path):
    vw, fixed = plain_record_filesets(tmp_path)
    a = load(fixed)
    rng = np.random.default_rng(9)
    others = []
    for k, n in enumerate((7, 130)):
        rows = a["pvar"]["rows"][::-1] if k else a["pvar"]["rows"][3:]
        codes = rng.integers(0, 4, size=(len(rows), n), dtype=np.uint8)
        others.append(write_fileset(tmp_path / f"other{k}", a["pvar"]["head"], rows, a["psam"]["head"], [f"U{k}_{i}\tNA" for i in range(n)], codes))
    for order, union in (((others[0], vw, others[1]), False), ((vw, others[0], others[1]), True)):
        if union:   # the variable-width file's compressed rows are variants of the union: their records cannot be read
            p = run("merge", *order, "-o", tmp_path / "u", "--union")
            assert p.returncode == 101 and b"stored compressed" in p.stderr and not list(tmp_path.glob("u.*"))
            continue
        want, m, n = expected(order, union=union)
        assert len(m["rows"]) == 57 and n == 40 + 137
        out = tmp_path / "o"
        p = run("merge", *order, "-o", out)
        assert p.returncode == 0, p.stderr
        check(out, want)
        # and equal to the merge with the fixed-width twin of the variable-width fileset, its .psam apart from nothing
        out2 = tmp_path / "o2"
        assert run("merge", order[0], fixed, order[2], "-o", out2).returncode == 0
        check(out2, want)
