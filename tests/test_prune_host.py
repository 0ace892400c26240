"""`prune` without a device: host/prune_plan.cpp (keys, the window a span needs, priorities, the mask bytes, the sequential greedy set)
through tests/prune_check.cpp, a stand-alone program built from that source alone under ASan + UBSan, against tests/prune_ref.py; then
`pgen-hip prune` in the usage text, its usage errors (exit 2), its file errors (exit 101, no output file) and the runs that keep
every variant without touching a device."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import prune_ref as R
from helpers import GOLDEN

REPO = Path(__file__).resolve().parent.parent
HOST = REPO / "pgen_rs_amd" / "host"
CLI = REPO / "pgen_rs_amd" / "pgen-hip"


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The program, and the proof of purity: it links from prune_plan.cpp alone."""
    exe = tmp_path_factory.mktemp("prune") / "prune_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe),
           str(REPO / "tests" / "prune_check.cpp"), str(HOST / "prune_plan.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr

    def run(mode, *tokens):
        p = subprocess.run([str(exe), mode], input=" ".join(str(t) for t in tokens) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == "", p.stderr
        return p.stdout.split()

    return run


def random_variants(seed, n):
    rng = np.random.default_rng(seed)
    names = ["1", "2", "X", "chr7", "MT"]
    chrom, pos, c, p = [], [], 0, 0
    for _ in range(n):
        if rng.random() < 0.08:
            c, p = int(rng.integers(0, len(names))), 0      # a chromosome may come back: its rank is its first appearance's
        p = max(0, p + int(rng.integers(-30, 400)))            # mostly ascending, sometimes not
        chrom.append(names[c])
        pos.append(p)
    return chrom, pos


@pytest.mark.parametrize("seed", range(6))
def test_keys_and_window(check, seed):
    n = [0, 1, 2, 40, 200, 333][seed]
    chrom, pos = random_variants(seed, n)
    flat = [x for cp in zip(chrom, pos) for x in cp]
    for with_pos in (1, 0):
        want = R.keys(chrom, pos if with_pos else None)
        assert [int(k) for k in check("keys", with_pos, n, *flat)] == want
        for span in (0, 1, 399, 1000, 5000, 10**6, 2**40):
            for cap in (0, 1, 3, 50):
                assert int(check("window", span, cap, n, *want)[0]) == R.window_for_span(want, span, cap), (with_pos, span, cap)
    if n == 40:
        assert len({k >> 32 for k in R.keys(chrom, pos)}) >= 2


def test_window_by_hand(check):
    key = R.keys(["a"] * 5 + ["b"] * 3, [100, 200, 300, 1300, 1400, 5, 1005, 9005])
    assert key[5] == (1 << 32) | 5
    for span, want in ((0, 1), (99, 1), (100, 1), (200, 2), (1199, 2), (1200, 3), (1300, 4), (10**9, 4)):
        assert R.window_for_span(key, span) == want == int(check("window", span, 0, len(key), *key)[0]), span
    assert R.window_for_span(key, 10**9, 2) == 2 == int(check("window", 10**9, 2, len(key), *key)[0])
    # a smaller key behind row i is far away (mod 2^64) and skipped; the equal key behind it is inside the span
    assert int(check("window", 5, 0, 3, R.M64, R.M64 - 1, R.M64)[0]) == R.window_for_span([R.M64, R.M64 - 1, R.M64], 5) == 2


def test_priority_pos_and_mask_bytes(check):
    rng = np.random.default_rng(4)
    counts = np.concatenate([rng.integers(0, 3000, size=(200, 3)), [[0, 0, 0], [5, 0, 0], [0, 0, 5], [0, 7, 0], [1, 0, 1], [2**31 - 1, 2**31 - 1, 2**31 - 1],
                                                                    [0, 0, 2**32 - 1], [2**32 - 1, 0, 0]]])
    got = [int(x) for x in check("priority", len(counts), *counts.reshape(-1).tolist())]
    assert got == R.priority_of_counts(counts).tolist()
    assert got[200:205] == [0, 0, 0, 2147483647, 2147483647]
    texts = ["0", "1", "007", "4294967295", "4294967296", "99999999999", "-5", "+5", "5x", "0x10", "-", "1e3", "12 "[:2]]
    out = check("pos", len(texts), *texts)
    for k, t in enumerate(texts):
        want = R.parse_pos("" if t == "-" else t)
        assert (out[2 * k] == "1") == (want is not None) and (want is None or int(out[2 * k + 1]) == want), t
    for n, w, free in ((0, 1, 0), (1000, 1, 8000), (1000, 33, 31999), (1000, 33, 32000), (2**32 - 1, 2**32 - 1, 2**63)):
        mb, fits = check("masks", n, w, free)
        assert int(mb) == R.mask_bytes(n, w) and (fits == "1") == (R.mask_bytes(n, w) <= free // 2)


@pytest.mark.parametrize("seed", range(8))
def test_sequential_greedy_set(check, seed):
    rng = np.random.default_rng(50 + seed)
    n = int(rng.integers(0, 80))
    m = int(rng.integers(0, 3 * n + 1)) if n > 1 else 0
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, max(n, 1), size=(m, 2)) if a != b]
    prio = None if seed % 3 == 0 else rng.integers(0, 4 if seed % 3 == 1 else 2**32, size=n, dtype=np.uint64)
    state0 = np.zeros(n, dtype=np.uint8) if seed % 2 else rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=n)
    flat = [x for p in pairs for x in p]
    got = check("resolve", n, len(pairs), 0 if prio is None else 1, *flat, *([] if prio is None else prio.tolist()), *state0.tolist())
    assert [int(s) for s in got] == R.resolve_from_edge_list(n, pairs, prio, state0).tolist()


def test_cli_gpu_cases_keep_clear_of_the_threshold(tmp_path):
    """The fileset of tests/test_host_cli_prune_gpu.py, built here, and the reference of every case that file runs: none trips the
    guard of prune_ref.edges, and the two guarantees hold on each."""
    import test_host_cli_prune_gpu as G

    d = G.build_data(tmp_path)
    cases = G.reference_cases(d)
    assert len(cases) == len(G.WINDOWS) + 1
    for rows, cols, window in cases:
        ref = G.reference(d, rows, cols, **window)
        G.check_guarantees(ref)
        assert len(ref["kept"]) + len(ref["removed"]) == len(rows)


def test_device_memory_needs_a_ctx():
    from pgen_rs_amd import _capi

    assert _capi.lib.pgenhip_device_memory(None, None, None) == _capi.ERR_BAD_ARG
    assert b"ctx" in _capi.lib.pgenhip_last_error_detail()


# ---- the command ---------------------------------------------------------------------------------------------------------------------
def cli(*args):
    return subprocess.run([str(CLI), "prune", *map(str, args)], capture_output=True, timeout=120)


def test_prune_in_usage():
    p = subprocess.run([str(CLI), "help"], capture_output=True, timeout=120)
    assert p.returncode == 0
    for word in (b"prune ", b"--window <W>", b"--window-kb <KB>", b"--r2 <X>", b"--export", b".prune.in", b".prune.out", b"monomorphic",
                 b"more common", b"plink2 --indep-pairwise"):
        assert word in p.stdout, word


@pytest.mark.parametrize("args", [[], ["x"], ["x", "--window", "5", "--r2", "0.2"], ["x", "--r2", "0.2", "-o", "o"], ["x", "--window", "5", "-o", "o"],
                                  ["x", "--window", "0", "--r2", "0.2", "-o", "o"], ["x", "--window", "w", "--r2", "0.2", "-o", "o"],
                                  ["x", "--window-kb", "-1", "--r2", "0.2", "-o", "o"], ["x", "--window-kb", "k", "--r2", "0.2", "-o", "o"],
                                  ["x", "--window", "5", "--r2", "2", "-o", "o"], ["x", "--window", "5", "--r2", "nan", "-o", "o"],
                                  ["x", "--window", "5", "--r2", "0.2", "-o", ""], ["x", "--window", "5", "--r2", "0.2", "-o", "o", "--bogus"],
                                  ["x", "y", "--window", "5", "--r2", "0.2", "-o", "o"], ["x", "--window", "5", "--r2", "0.2", "-o", "o", "--block-rows", "0"]])
def test_usage_errors_exit_2(args):
    p = cli(*args)
    assert p.returncode == 2, (args, p.stderr)
    assert b"error:" in p.stderr


def fileset(d: Path, column_line: bytes, rows: list[bytes], n=8):
    v = len(rows)
    (d / "t.pvar").write_bytes(column_line + b"".join(rows))
    (d / "t.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"S%d\tNA\n" % k for k in range(n)))
    (d / "t.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + bytes(v * ((n + 3) // 4)))
    return d / "t"


def no_output(d: Path):
    return not any(p.name.startswith("o.") for p in d.iterdir())


def test_file_errors_exit_101_and_leave_no_file(tmp_path):
    rows = [b"1\t%d\tv%d\tA\tG\n" % (100 + k, k) for k in range(4)]
    for line, drop in ((b"#CHROM\tPOS\tREF\tALT\n", 2), (b"#POS\tID\tREF\tALT\n", 0), (b"#CHROM\tID\tREF\tALT\n", 1)):   # no ID, no CHROM, no POS
        cut = [b"\t".join(f for c, f in enumerate(r.split(b"\t")) if c != drop) for r in rows]
        p = cli(fileset(tmp_path, line, cut), "--window", "3", "--r2", "0.2", "-o", tmp_path / "o")
        assert p.returncode == 101 and b"not among the headers" in p.stderr, p.stderr
        assert no_output(tmp_path)
    bad = list(rows)
    bad[2] = b"1\t1e3\tv2\tA\tG\n"
    p = cli(fileset(tmp_path, b"#CHROM\tPOS\tID\tREF\tALT\n", bad), "--window-kb", "1", "--r2", "0.2", "-o", tmp_path / "o")
    assert p.returncode == 101 and b"POS '1e3'" in p.stderr and b"line 3" in p.stderr, p.stderr
    assert no_output(tmp_path)
    p = cli(tmp_path / "missing", "--window", "3", "--r2", "0.2", "-o", tmp_path / "o")
    assert p.returncode == 101 and no_output(tmp_path)
    p = cli(fileset(tmp_path, b"#CHROM\tPOS\tID\tREF\tALT\n", rows), "--window", "3", "--r2", "0.2", "--export", "-o", tmp_path / "t")
    assert p.returncode == 101 and b"overwrite its input" in p.stderr, p.stderr


def test_fewer_than_two_variants_or_no_sample_keeps_everything_without_a_device(tmp_path):
    rows = [b"1\t%d\tv%d\tA\tG\n" % (100 + k, k) for k in range(4)]
    pre = fileset(tmp_path, b"#CHROM\tPOS\tID\tREF\tALT\n", rows)
    for flags, ids in ((["--include-var", 'ID == "v2"'], b"v2\n"), (["--include-var", 'ID == "none"'], b""),
                       (["--include-sam", 'IID == "nobody"'], b"v0\nv1\nv2\nv3\n")):
        p = cli(pre, "--window-kb", "5", "--r2", "0.2", "-o", tmp_path / "o", *flags)
        assert p.returncode == 0, p.stderr
        j = json.loads(p.stdout)
        assert j == {"kept": ids.count(b"\n"), "removed": 0, "edges": 0, "window": 0, "resolve_calls": 0, "mask_bytes": 0}
        assert (tmp_path / "o.prune.in").read_bytes() == ids and (tmp_path / "o.prune.out").read_bytes() == b""
        (tmp_path / "o.prune.in").unlink()
        (tmp_path / "o.prune.out").unlink()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_without_gpu_exits_101_and_leaves_no_file(tmp_path):
    for ext in ("pvar", "psam"):
        shutil.copy(GOLDEN / "basic1" / f"basic1.{ext}", tmp_path / f"basic1.{ext}")
    n, v = 2504, 17784
    (tmp_path / "basic1.pgen").write_bytes(bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + n.to_bytes(4, "little") + b"\x40" + bytes(v * 626))
    p = cli(tmp_path / "basic1", "--window", "10", "--r2", "0.2", "-o", tmp_path / "o", "--export")
    assert p.returncode == 101 and b"device" in p.stderr.lower(), p.stderr
    assert no_output(tmp_path)
