"""`merge` without a device: the matching rules (pgen_rs_amd/host/merge_match.cpp) through tests/merge_check.cpp, a stand-alone program
built from that source alone under ASan + UBSan, against tests/merge_ref.py, an independent Python restatement; then
`pgen-hip merge --dry-run` on small filesets: its counts, its errors and exit codes, and that it creates no file."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import merge_ref as MR
import pack_ref as PR

REPO = Path(__file__).resolve().parent.parent
HOST = REPO / "pgen_rs_amd" / "host"
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
PVAR_COLS = "#CHROM\tPOS\tID\tREF\tALT"
PSAM_COLS = "#IID\tSEX"


@pytest.fixture(scope="module")
def merge_check(tmp_path_factory):
    """The program, and the proof of purity: it links from merge_match.cpp alone."""
    d = tmp_path_factory.mktemp("merge")
    exe = d / "merge_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe),
           str(REPO / "tests" / "merge_check.cpp"), str(HOST / "merge_match.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    count = [0]

    def run(mode, tables):
        """tables: [(column_line, rows)] -> (the program's lines, the tables as merge_ref takes them)"""
        count[0] += 1
        named = []
        for i, (col, rows) in enumerate(tables):
            path = d / f"case{count[0]}_{chr(97 + i)}.txt"
            path.write_text("".join(line + "\n" for line in [col] + list(rows)))
            named.append((str(path), col, list(rows)))
        p = subprocess.run([str(exe), mode] + [t[0] for t in named], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", p.stderr
        return p.stdout.splitlines(), named

    return run


def test_merge_match_includes_no_project_header_but_its_own():
    for name in ("merge_match.h", "merge_match.cpp"):
        quoted = [ln.split('"')[1] for ln in (HOST / name).read_text().splitlines() if ln.startswith('#include "')]
        assert set(quoted) <= {"merge_match.h"}, (name, quoted)


def rows_of(*specs):
    return ["\t".join(map(str, s)) for s in specs]


def as_lines(m):
    out = []
    for j, (fi, fr) in enumerate(m["rows"]):
        out.append(" ".join(["row", str(fi), str(fr)] + [f"{m['src'][p][j]} {m['flip'][p][j]}" for p in range(len(m["src"]))]))
    for k in ("flipped", "absent", "dropped"):
        out.append(" ".join([k] + [str(x) for x in m[k]]))
    out.append(f"id_conflicts {m['id_conflicts']}")
    return out


def agree(merge_check, mode, tables):
    got, named = merge_check(mode, tables)
    want = MR.match(named, union=mode == "union")
    assert got == as_lines(want)
    return want


A = rows_of((1, 100, "a", "A", "G"), (1, 200, "b", "C", "T"), (2, 50, "c", "G", "GA"), (1, 300, "d", "T", "C"), (2, 70, "e", "A", "C"))


def test_intersection_in_the_first_inputs_order(merge_check):
    b = rows_of((2, 70, "e", "A", "C"), (1, 300, "d", "T", "C"), (9, 1, "x", "A", "C"), (1, 100, "a", "A", "G"))
    c = rows_of((1, 300, "d", "T", "C"), (1, 100, "a", "A", "G"), (2, 70, "e", "A", "C"), (2, 50, "c", "G", "GA"))
    m = agree(merge_check, "variants", [(PVAR_COLS, A), (PVAR_COLS, b), (PVAR_COLS, c)])
    assert m["rows"] == [(0, 0), (0, 3), (0, 4)] and m["src"][1] == [3, 1, 0] and m["src"][2] == [1, 0, 2]
    assert m["dropped"] == [2, 1, 1] and m["absent"] == [0, 0, 0] and m["flipped"] == [0, 0, 0]


def test_union_order_across_interleaved_chromosomes(merge_check):
    a = rows_of((2, 50, "a1", "A", "G"), (1, 300, "a2", "A", "G"), (2, 10, "a3", "A", "G"))
    b = rows_of((1, 100, "b1", "A", "G"), (3, 5, "b2", "A", "G"), (2, 50, "b3", "A", "G"), (2, 10, "b4", "C", "T"), (1, 300, "b5", "A", "G"))
    m = agree(merge_check, "union", [(PVAR_COLS, a), (PVAR_COLS, b)])
    # CHROM ranks by first appearance: 2, 1, 3; POS numeric (10 before 50); at 2:10 the first-seen variant first
    assert m["rows"] == [(0, 2), (1, 3), (0, 0), (1, 0), (0, 1), (1, 1)]
    assert m["absent"] == [3, 1] and m["dropped"] == [0, 0] and m["id_conflicts"] == 2
    agree(merge_check, "union", [(PVAR_COLS, rows_of((1, 9, "p", "A", "C"), (1, 10, "q", "A", "C"), (1, 9, "r", "A", "G")))])   # 9 before 10: numbers, not strings


def test_swapped_alleles_flip_and_other_alleles_are_another_variant(merge_check):
    b = rows_of((1, 100, "a", "G", "A"), (1, 200, "b", "C", "T"), (1, 200, "b2", "C", "G"), (2, 50, "c", "GA", "G"))
    m = agree(merge_check, "variants", [(PVAR_COLS, A), (PVAR_COLS, b)])
    assert m["rows"] == [(0, 0), (0, 1), (0, 2)] and m["flip"] == [[0, 0, 0], [1, 0, 1]] and m["flipped"] == [0, 2] and m["dropped"] == [2, 1]
    m = agree(merge_check, "union", [(PVAR_COLS, A), (PVAR_COLS, b)])
    assert len(m["rows"]) == 6 and m["absent"] == [1, 2]   # 1:200 C/T and 1:200 C/G are two variants
    agree(merge_check, "union", [(PVAR_COLS, b), (PVAR_COLS, A)])   # the first holder fixes the orientation: now A is the flipped one


def test_id_conflict_is_counted(merge_check):
    b = rows_of((1, 100, "other", "A", "G"), (1, 200, "b", "T", "C"), (7, 7, "only_b", "A", "C"))
    m = agree(merge_check, "variants", [(PVAR_COLS, A), (PVAR_COLS, b), (PVAR_COLS, rows_of((1, 200, "B", "C", "T"), (1, 100, "a", "A", "G")))])
    assert m["id_conflicts"] == 2 and m["rows"] == [(0, 0), (0, 1)]


def test_named_errors(merge_check):
    def error(mode, tables):
        got, named = merge_check(mode, tables)
        assert len(got) == 1 and got[0].startswith("error "), got
        with pytest.raises(MR.MergeError) as ei:
            (MR.check_samples if mode == "samples" else MR.match)(named, **({} if mode == "samples" else {"union": mode == "union"}))
        return got[0], ei.value, named

    dup = A + rows_of((1, 200, "again", "T", "C"))   # the same key with the alleles the other way round
    msg, e, named = error("variants", [(PVAR_COLS, A), (PVAR_COLS, dup)])
    assert e.kind == "duplicate" and e.where == (named[1][0], 3, 7) and f"{named[1][0]}: lines 3 and 7 hold the same variant" in msg
    bad = rows_of((1, 100, "a", "A", "G"), (1, "1e3", "f", "A", "G"))
    msg, e, named = error("union", [(PVAR_COLS, A), (PVAR_COLS, bad)])
    assert e.kind == "pos" and e.where == (named[1][0], 3, "1e3") and f"{named[1][0]}: line 3: POS '1e3' is not an unsigned integer" in msg
    for pos in ("", "-5", "+5", " 5", "5 ", "0x10"):
        msg, e, _ = error("union", [(PVAR_COLS, rows_of((1, pos, "f", "A", "G")))])
        assert e.kind == "pos"
    agree(merge_check, "variants", [(PVAR_COLS, A), (PVAR_COLS, bad)])   # the intersection compares POS as a string only
    msg, e, named = error("variants", [(PVAR_COLS, A), (PVAR_COLS + "\tQUAL", [r + "\t." for r in A])])
    assert e.kind == "columns" and e.where == (named[0][0], named[1][0]) and f"column lines of {named[0][0]} and {named[1][0]} differ" in msg
    sa, sb = rows_of(("s1", "NA"), ("s2", "NA")), rows_of(("s3", "NA"), ("s1", "NA"))
    msg, e, named = error("samples", [(PSAM_COLS, sa), (PSAM_COLS, sb)])
    assert e.kind == "iid" and e.where == ("s1", named[0][0], named[1][0]) and f"IID 's1' occurs twice: in {named[0][0]} and in {named[1][0]}" in msg
    msg, e, named = error("samples", [(PSAM_COLS, sa + rows_of(("s2", "1")))])
    assert e.where == ("s2", named[0][0], named[0][0])
    msg, e, named = error("samples", [(PSAM_COLS, sa), ("#IID\tSEX\tPOP", rows_of(("s9", "NA", "x")))])
    assert e.kind == "columns" and f".psam column lines of {named[0][0]} and {named[1][0]} differ" in msg
    got, _ = merge_check("samples", [(PSAM_COLS, sa), (PSAM_COLS, rows_of(("s3", "NA")))])
    assert got == ["ok"]


def test_empty_inputs(merge_check):
    for mode in ("variants", "union"):
        m = agree(merge_check, mode, [(PVAR_COLS, []), (PVAR_COLS, [])])
        assert m["rows"] == []
        m = agree(merge_check, mode, [(PVAR_COLS, A), (PVAR_COLS, [])])
        assert len(m["rows"]) == (5 if mode == "union" else 0) and m["dropped"] == [0 if mode == "union" else 5, 0]
        agree(merge_check, mode, [(PVAR_COLS, []), (PVAR_COLS, A)])
    got, _ = merge_check("samples", [(PSAM_COLS, []), (PSAM_COLS, [])])
    assert got == ["ok"]


# ---- the command, up to the device ----

def write_fileset(prefix, pvar_rows, n_samples, first_sample=0, pvar_cols=PVAR_COLS, psam_cols=PSAM_COLS, iids=None, seed=1):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(len(pvar_rows), n_samples), dtype=np.uint8)
    Path(str(prefix) + ".pgen").write_bytes(PR.pgen_file(PR.pack_codes(codes), n_samples))
    Path(str(prefix) + ".pvar").write_text("##source=test\n" + "".join(r + "\n" for r in [pvar_cols] + list(pvar_rows)))
    iids = iids if iids is not None else [f"S{first_sample + i}" for i in range(n_samples)]
    Path(str(prefix) + ".psam").write_text("".join(r + "\n" for r in [psam_cols] + [f"{i}\tNA" for i in iids]))
    return (str(prefix) + ".pvar", pvar_cols, list(pvar_rows))


def cli(*args):
    return subprocess.run([str(CLI), "merge", *map(str, args)], capture_output=True, text=True, timeout=120)


def test_dry_run_counts_errors_and_exit_codes(tmp_path):
    b_rows = rows_of((2, 70, "e", "A", "C"), (1, 300, "d", "C", "T"), (9, 1, "x", "A", "C"), (1, 100, "A", "A", "G"))
    ta = write_fileset(tmp_path / "a", A, 5)
    tb = write_fileset(tmp_path / "b", b_rows, 3, first_sample=5, seed=2)
    tc = write_fileset(tmp_path / "c", A[::-1], 0, seed=3)
    before = sorted(p.name for p in tmp_path.iterdir())
    out = tmp_path / "out"
    for extra, union, tables in (((), False, [ta, tb]), (("--union",), True, [ta, tb]), (("--union",), True, [tb, tc, ta]), ((), False, [tc, tb, ta])):
        p = cli(*[t[0][:-5] for t in tables], "-o", out, "--dry-run", *extra)
        assert p.returncode == 0, p.stderr
        n = sum({ta[0]: 5, tb[0]: 3, tc[0]: 0}[t[0]] for t in tables)
        assert json.loads(p.stdout) == MR.counts_json(MR.match(tables, union=union, first_line=3), n)
    # errors: exit code 101 and the message
    td = write_fileset(tmp_path / "d", A + rows_of((1, 200, "again", "T", "C")), 2, first_sample=20)
    te = write_fileset(tmp_path / "e", rows_of((1, "x7", "f", "A", "G")), 2, first_sample=30)
    write_fileset(tmp_path / "f", A, 2, first_sample=4)                       # S4 and S5: S4 is in a too
    write_fileset(tmp_path / "g", A, 2, first_sample=40, pvar_cols=PVAR_COLS + "\tQUAL")
    write_fileset(tmp_path / "h", A, 2, first_sample=50, psam_cols="#IID\tPOP")
    before = sorted(p.name for p in tmp_path.iterdir())
    for args, message in (
        ((tmp_path / "a", tmp_path / "d"), f"{td[0]}: lines 4 and 8 hold the same variant (1:200 T/C)"),
        ((tmp_path / "a", tmp_path / "e", "--union"), f"{te[0]}: line 3: POS 'x7' is not an unsigned integer"),
        ((tmp_path / "a", tmp_path / "f"), f"sample IID 'S4' occurs twice: in {tmp_path / 'a'}.psam and in {tmp_path / 'f'}.psam"),
        ((tmp_path / "a", tmp_path / "g"), f"the .pvar column lines of {tmp_path / 'a'}.pvar and {tmp_path / 'g'}.pvar differ"),
        ((tmp_path / "a", tmp_path / "h"), f"the .psam column lines of {tmp_path / 'a'}.psam and {tmp_path / 'h'}.psam differ"),
        ((tmp_path / "a", tmp_path / "nowhere"), f"open {tmp_path / 'nowhere'}.pgen"),
    ):
        p = cli(*args, "-o", out, "--dry-run")
        assert p.returncode == 101 and message in p.stderr, (p.returncode, p.stderr)
    # an output that names an input, by another spelling too
    for o in (tmp_path / "b", tmp_path / "x" / ".." / "b"):
        p = cli(tmp_path / "a", tmp_path / "b", "-o", o, "--dry-run")
        assert p.returncode == 101 and "merge would overwrite an input" in p.stderr
    # usage errors: exit code 2
    p = cli(tmp_path / "a", "-o", out, "--dry-run")
    assert p.returncode == 2 and "at least two" in p.stderr
    p = cli(*[tmp_path / "a"] * 9, "-o", out, "--dry-run")
    assert p.returncode == 2 and "merge in stages" in p.stderr
    p = cli(tmp_path / "a", tmp_path / "b", "--dry-run")
    assert p.returncode == 2 and "--out" in p.stderr
    assert cli(tmp_path / "a", tmp_path / "b", "-o", out, "--include-var", "POS > 1").returncode == 2
    assert sorted(p.name for p in tmp_path.iterdir()) == before   # no file was created


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_device_is_a_loud_failure_that_leaves_no_file(tmp_path):
    write_fileset(tmp_path / "a", A, 5)
    write_fileset(tmp_path / "b", A, 3, first_sample=5)
    p = cli(tmp_path / "a", tmp_path / "b", "-o", tmp_path / "out")
    assert p.returncode == 101 and "device" in p.stderr   # the library's own words where the runtime finds none, else merge's
    assert not list(tmp_path.glob("out.*"))
