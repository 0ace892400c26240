"""GPU leg of `pgen-hip prune`: the two ID lists end to end (metadata filter -> records staged to HBM -> counts and pair masks per
block -> resolve loop -> state bytes) against tests/prune_ref.py on a synthesised fileset with LD blocks on three chromosomes, for
windows in variants, in base pairs and both, with sample and variant filters, blocks that cut through LD blocks and a mode-0x10
fileset; the two guarantees the README states, checked from the pairs' r^2 alone; --export's files byte for byte; the JSON line."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pack_ref
import prune_ref as R
from helpers import GOLDEN
from test_host_cli_export_gpu import check as check_files
from test_host_cli_export_gpu import expected as expected_files

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
V, N = 600, 200
MIN_R2 = 0.21337
WMAX = 40


def run(*args):
    return subprocess.run([str(CLI), *map(str, args)], capture_output=True, timeout=300)


class Data:
    pass


def build_data(directory: Path):
    """600 variants x 200 samples, chromosomes 1 / 2 / X, LD blocks of 37 rows, a few monomorphic and all-missing rows; as a
    fixed-width fileset and as a mode-0x10 one with a compressed record behind every fifth plain one.  Plain numpy and file writes:
    tests/test_prune_host.py builds it on the CPU and runs every case's reference through the guard of prune_ref.edges."""
    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    d = Data()
    d.dir = directory
    rng = np.random.default_rng(2026)
    d.codes = R.ld_codes(rng, V, N, redraw=0.1, fresh_every=37)
    d.codes[100] = 0              # monomorphic: no r^2, kept
    d.codes[101] = 3              # uncalled: priority 0, no r^2, kept
    d.codes[300] = d.codes[299]   # identical neighbours: r^2 = 1, equal priority, the earlier one stays
    d.chrom = ["1"] * 250 + ["2"] * 200 + ["X"] * 150
    d.pos = []
    for c in ("1", "2", "X"):
        d.pos += np.cumsum(rng.integers(50, 3000, size=d.chrom.count(c))).tolist()
    d.ids = [f"v{i}" for i in range(V)]
    d.flag = [int(x) for x in rng.random(V) < 0.8]
    d.pop = ["a" if s % 3 else "b" for s in range(N)]
    recs = pack_ref.pack_codes(d.codes.astype(np.uint8))
    row = lambda i, t: b"%s\t%d\t%s\tC\tT\t%d\t%d\n" % (d.chrom[i].encode(), d.pos[i], d.ids[i].encode(), d.flag[i], t)
    vw_recs, vw_rows = [], []
    for i in range(V):
        vw_recs.append((0, recs[i].tobytes()))
        vw_rows.append(row(i, 0))
        if i % 5 == 4:
            vw_recs.append((1, bytes(3 if i % 10 == 4 else 4 * recs.shape[1])))
            vw_rows.append(b"%s\t%d\tc%d\tC\tT\t1\t1\n" % (d.chrom[i].encode(), d.pos[i], i))
    vw, _ = writer.write_vw(N, vw_recs, 8, 2)
    fixed = bytes([0x6C, 0x1B, 0x02]) + V.to_bytes(4, "little") + N.to_bytes(4, "little") + b"\x40" + recs.tobytes()
    for name, pgen, rows in (("vw", vw, vw_rows), ("fixed", fixed, [row(i, 0) for i in range(V)])):
        (d.dir / f"{name}.pgen").write_bytes(pgen)
        (d.dir / f"{name}.pvar").write_bytes(b"##source=test\n#CHROM\tPOS\tID\tREF\tALT\tFLAG\tRTYPE\n" + b"".join(rows))
        (d.dir / f"{name}.psam").write_bytes(b"#IID\tSEX\tPOP\n" + b"".join(b"S%04d\tNA\t%s\n" % (k, d.pop[k].encode()) for k in range(N)))
    d.grids = {}
    return d


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return build_data(tmp_path_factory.mktemp("prune"))


def reference(d, rows, cols, **window):
    """prune_ref.prune on the kept rows and samples; the r^2 grid of a (rows, samples) choice is computed once."""
    key = (tuple(rows[:3]), len(rows), len(cols))
    codes = d.codes[np.asarray(rows)][:, np.asarray(cols)]
    if key not in d.grids:
        d.grids[key] = R.r2_grid(codes, len(rows), WMAX)
    chrom, pos, ids = [d.chrom[i] for i in rows], [d.pos[i] for i in rows], [d.ids[i] for i in rows]
    kept, removed, edges, w = R.prune(codes, chrom, pos, ids, MIN_R2, grid=d.grids[key], **window)
    assert w <= WMAX
    return dict(kept=kept, removed=removed, edges=edges, w=w, codes=codes, chrom=chrom, pos=pos, ids=ids, grid=d.grids[key], window=window)


def check_guarantees(ref):
    """From the pairs' r^2 alone: no two kept variants inside a window are linked; every removed one is linked to a kept variant inside
    its window that is more common, or equally common and earlier."""
    f = ref["grid"][0]
    n, w = len(ref["ids"]), ref["w"]
    span = ref["window"].get("window_kb")
    prio = R.priority_of_counts(R.counts_of_codes(ref["codes"]))
    kept = set(ref["kept"])
    linked = [[] for _ in range(n)]
    for i in range(n):
        for dd in range(1, w + 1):
            j = i + dd
            if j >= n or ref["chrom"][i] != ref["chrom"][j]:
                continue
            if span is not None and not 0 <= ref["pos"][j] - ref["pos"][i] <= 1000 * span:
                continue
            if f[i, dd - 1] > np.float32(MIN_R2):
                linked[i].append(j)
                linked[j].append(i)
    for i in range(n):
        mine = ref["ids"][i] in kept
        if mine:
            assert not any(ref["ids"][j] in kept for j in linked[i]), f"{ref['ids'][i]} and a linked variant both stay"
        else:
            assert any(ref["ids"][j] in kept and (prio[j] > prio[i] or (prio[j] == prio[i] and j < i)) for j in linked[i]), \
                f"{ref['ids'][i]} was removed without a kept, more common linked variant"


def check_run(p, out: Path, ref):
    assert p.returncode == 0, p.stderr
    assert out.with_suffix(".prune.in").read_text().split() == ref["kept"]
    assert out.with_suffix(".prune.out").read_text().split() == ref["removed"]
    j = json.loads(p.stdout.splitlines()[0])
    assert j["kept"] + j["removed"] == len(ref["ids"]) and j["kept"] == len(ref["kept"])
    assert j["edges"] == ref["edges"] and j["window"] == ref["w"] and j["resolve_calls"] >= 1
    assert j["mask_bytes"] == R.mask_bytes(len(ref["ids"]), ref["w"])


ALL_ROWS, ALL_COLS = list(range(V)), list(range(N))
FILTERED = dict(window_kb=15, window=20)      # test_filters_export_and_freq's windows, on the FLAG == 1 rows and the POP a samples


def filtered_choice(d):
    return [i for i in range(V) if d.flag[i]], [s for s in range(N) if d.pop[s] == "a"]


def reference_cases(d):
    """Every (rows, samples, windows) this file holds the command against."""
    return [(ALL_ROWS, ALL_COLS, w) for _, w in WINDOWS.values()] + [(*filtered_choice(d), FILTERED)]


WINDOWS = {
    "variants": (["--window", "12"], dict(window=12)),
    "kb": (["--window-kb", "10"], dict(window_kb=10)),
    "both": (["--window-kb", "40", "--window", "8"], dict(window_kb=40, window=8)),
    "kb0": (["--window-kb", "0"], dict(window_kb=0)),
}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_lists_match_the_reference_and_keep_the_guarantees(data, tmp_path, name):
    flags, window = WINDOWS[name]
    ref = reference(data, ALL_ROWS, ALL_COLS, **window)
    if name != "kb0":
        assert len(ref["removed"]) > 100 and len(ref["kept"]) > 50 and "v100" in ref["kept"] and "v101" in ref["kept"]
        assert "v299" in ref["kept"] or "v300" in ref["removed"]
    if name == "both":
        assert ref["w"] == 8
    check_guarantees(ref)
    want_in = None
    for extra in ([], ["--block-rows", "50"], ["--block-rows", "7", "--stats"]):      # blocks cut through the LD blocks of 37 rows
        out = tmp_path / "o"
        p = run("prune", data.dir / "fixed", *flags, "--r2", MIN_R2, "-o", out, *extra)
        check_run(p, out, ref)
        if "--stats" in extra:
            assert b'"variants_kept"' in p.stderr
        want_in = want_in or out.with_suffix(".prune.in").read_bytes()
        assert out.with_suffix(".prune.in").read_bytes() == want_in


def test_filters_export_and_freq(data, tmp_path):
    rows, cols = filtered_choice(data)
    ref = reference(data, rows, cols, **FILTERED)
    check_guarantees(ref)
    out = tmp_path / "o"
    p = run("prune", data.dir / "fixed", "--window-kb", "15", "--window", "20", "--r2", MIN_R2, "--include-var", 'FLAG == "1"', "--include-sam",
            'POP == "a"', "--block-rows", "64", "--export", "-o", out)
    check_run(p, out, ref)
    kept = {i.encode() for i in ref["kept"]}
    check_files(out, expected_files(data.dir / "fixed", lambda r: r[b"ID"] in kept, lambda r: r[b"POP"] == b"a"))
    q = run("freq", out)
    assert q.returncode == 0 and q.stdout.count(b"\n") == len(ref["kept"]) + 1, q.stderr
    # the pruned fileset prunes to itself
    p = run("prune", out, "--window-kb", "15", "--window", "20", "--r2", MIN_R2, "-o", tmp_path / "again")
    assert p.returncode == 0 and json.loads(p.stdout.splitlines()[0])["removed"] == 0, p.stderr


def test_variable_width_fileset_through_the_offset_entry_points(data, tmp_path):
    ref = reference(data, ALL_ROWS, ALL_COLS, window=12)
    for extra in ([], ["--block-rows", "33"]):
        out = tmp_path / "o"
        p = run("prune", data.dir / "vw", "--window", "12", "--r2", MIN_R2, "--include-var", 'RTYPE == "0"', "-o", out, *extra)
        check_run(p, out, ref)


def test_device_memory_is_what_the_mask_check_reads():
    import ctypes as C

    import pgen_rs_amd
    from pgen_rs_amd import _capi

    with pgen_rs_amd.GtEngine(8, device=0) as eng:
        free, total = C.c_uint64(), C.c_uint64()
        assert _capi.lib.pgenhip_device_memory(eng._ctx, C.byref(free), C.byref(total)) == _capi.OK
        assert 0 < free.value <= total.value and total.value > 1 << 30
        only = C.c_uint64()
        assert _capi.lib.pgenhip_device_memory(eng._ctx, None, C.byref(only)) == _capi.OK and only.value == total.value
        assert _capi.lib.pgenhip_device_memory(eng._ctx, None, None) == _capi.ERR_BAD_ARG
