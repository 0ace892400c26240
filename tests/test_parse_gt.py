"""GT text to records — CPU leg: the Python restatement of the grammar (tests/parse_ref.py) against a per-byte state machine and
the committed .gt / .pgen pairs, ``pgenhip_vcf_index_lines`` against a numpy restatement and under a sanitized fuzzer, the new
constants and prototypes, the plan twin (tests/parse_plan.py) against the plan header, and the ``import`` command up to the device."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import parse_plan
import parse_ref
from helpers import GOLDEN, load_case
from pgen_rs_amd import _capi, vcf_index_lines

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "pgen_rs_amd" / "pgen-hip"
U64_MAX = 2**64 - 1


# ---- parse_ref -----------------------------------------------------------------------------------------------------------------------
def naive_field(field: bytes):
    """One field, a byte at a time: states A (an allele starts), D (inside a digit token), E (an allele has ended)."""
    alleles, seps = [], []
    state, token = "A", b""
    for ch in field + b"\t":   # a tab ends the last field
        c = bytes([ch])
        if state == "D":
            if c.isdigit():
                token += c
                continue
            alleles.append(token)
            state = "E"
        if state == "A":
            if c == b".":
                alleles.append(c)
                state = "E"
            elif c.isdigit():
                token, state = c, "D"
            else:
                return 3, parse_ref.BAD_CALL
        elif state == "E":
            if c in (b"\t", b":"):
                break
            if c not in (b"/", b"|") or len(alleles) == 2:
                return 3, parse_ref.BAD_CALL
            seps.append(c)
            state = "A"
    if any(a not in (b"0", b"1", b".") for a in alleles):
        return 3, parse_ref.ALLELE_RANGE
    if len(alleles) == 1:
        return (3 if alleles[0] == b"." else 2 * int(alleles[0])), parse_ref.HAPLOID
    flags = parse_ref.PHASED if seps[0] == b"|" else 0
    n_missing = sum(a == b"." for a in alleles)
    if n_missing:
        return 3, flags | (parse_ref.HALF_CALL if n_missing == 1 else 0)
    return int(alleles[0]) + int(alleles[1]), flags


def test_parse_ref_form_table():
    for field, code, flags in parse_ref.FORMS:
        assert parse_ref.parse_field(field) == (code, flags), field
        assert naive_field(field) == (code, flags), field


def test_parse_ref_random_fields_match_the_state_machine():
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"0011..//||:2 9a", dtype=np.uint8)
    for _ in range(20000):
        field = alphabet[rng.integers(0, alphabet.size, size=rng.integers(0, 7))].tobytes()
        assert parse_ref.parse_field(field) == naive_field(field), field


def test_parse_ref_random_lines():
    rng = np.random.default_rng(8)
    forms = parse_ref.FORMS
    for n in (0, 1, 3, 4, 5, 9):
        for _ in range(50):
            k = int(rng.integers(0, n + 3))
            picks = [forms[i] for i in rng.integers(0, len(forms), size=k)]
            region = b"".join(b"\t" + f for f, _, _ in picks)
            codes, flags = parse_ref.parse_region(region, n)
            want_flags = parse_ref.FIELD_COUNT if k != n else 0
            for _, _, fl in picks[:n]:
                want_flags |= fl
            assert codes == [c for _, c, _ in picks[:n]] + [3] * max(0, n - k) and flags == want_flags
    assert parse_ref.parse_region(b"0/0\t0/1", 2) == ([3, 3], parse_ref.FIELD_COUNT)   # no leading tab: no fields
    assert parse_ref.parse_region(b"", 0) == ([], 0)


def gt_case_names():
    return sorted(p.stem for p in (GOLDEN / "cases").glob("all_*.gt")) + ["wide_all"]


def case_lines(name):
    """(n, text, field_off, line_end, records with pad bits masked) of a committed all-samples case."""
    v, n, recs, kept, gt = load_case(name)
    assert kept is None
    text = gt.tobytes()
    assert len(text) == v * (4 * n + 1)
    field_off = np.arange(v, dtype=np.uint64) * (4 * n + 1)
    return n, text, field_off, field_off + 4 * n, parse_ref.mask_pad(recs, n)


@pytest.mark.parametrize("name", gt_case_names())
def test_parse_ref_on_committed_cases(name):
    n, text, field_off, line_end, want = case_lines(name)
    recs, flags = parse_ref.parse_lines(text, field_off, line_end, n)
    assert np.array_equal(recs, want) and not flags.any()
    assert all(parse_ref.fixed_takes(text[int(a):int(b)], n) for a, b in zip(field_off, line_end))


# ---- pgenhip_vcf_index_lines -----------------------------------------------------------------------------------------------------------
def index_lines_ref(data: bytes, format_col: int, last_block: bool, max_lines=None):
    a = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    stops = list(nl)
    if last_block and (len(a) > (nl[-1] + 1 if nl.size else 0)):
        stops.append(len(a))
    if max_lines is not None:
        stops = stops[:max_lines]
    rows, pos = [], 0
    for stop in stops:
        end = stop - 1 if stop < len(a) and stop > pos and a[stop - 1] == 13 else stop
        tabs = pos + np.flatnonzero(a[pos:end] == 9)
        if tabs.size < format_col:
            fmt = fo = U64_MAX
        else:
            fmt = pos if format_col == 0 else int(tabs[format_col - 1]) + 1
            fo = int(tabs[format_col]) if tabs.size > format_col else end
        rows.append((pos, fmt, fo, end))
        pos = min(stop + 1, len(a))
    return rows, pos


INDEX_TEXTS = [
    b"", b"\n", b"\n\n", b"a", b"a\n", b"a\tb\tc\n", b"a\tb\tc", b"a\tb\tc\r\n", b"a\tb\tc\r\nd\te\tf\r\n", b"\r\n", b"\r", b"x\r",
    b"1\t2\t3\t4\t5\t6\t7\t8\tGT\t0/0\t0/1\n1\t2\t3\t4\t5\t6\t7\t8\tGT\n1\t2\t3\n\t\t\t\t\t\t\t\t\t\n1\t2\t3\t4\t5\t6\t7\t8\tGT:DP\t0/0:1",
    b"a\tb\n\nc\td\r\n\r\ne",
]


@pytest.mark.parametrize("format_col", [0, 1, 2, 8])
@pytest.mark.parametrize("last_block", [True, False])
def test_vcf_index_lines_matches_numpy(format_col, last_block):
    for data in INDEX_TEXTS:
        for max_lines in (None, 0, 1, 2, 3):
            *arrs, consumed = vcf_index_lines(data, format_col, last_block, max_lines=max_lines)
            rows, pos = index_lines_ref(data, format_col, last_block, max_lines)
            got = list(zip(*[[int(x) for x in a] for a in arrs]))
            assert got == rows and consumed == pos, (data, format_col, last_block, max_lines)


def test_vcf_index_lines_random_and_refusals():
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"\t\t\n\r01/", dtype=np.uint8)
    for _ in range(300):
        data = alphabet[rng.integers(0, alphabet.size, size=rng.integers(0, 60))].tobytes()
        for format_col in (0, 2):
            for last_block in (True, False):
                *arrs, consumed = vcf_index_lines(data, format_col, last_block)
                rows, pos = index_lines_ref(data, format_col, last_block)
                assert list(zip(*[[int(x) for x in a] for a in arrs])) == rows and consumed == pos, (data, format_col, last_block)
    n, c = C.c_uint64(), C.c_uint64()
    buf = (C.c_uint64 * 4)()
    lib = _capi.lib
    assert lib.pgenhip_vcf_index_lines(b"a\n", 2, 0, 4, 0, buf, buf, buf, buf, None, C.byref(c)) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_vcf_index_lines(b"a\n", 2, 0, 4, 0, buf, buf, None, buf, C.byref(n), C.byref(c)) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_vcf_index_lines(None, 2, 0, 4, 0, buf, buf, buf, buf, C.byref(n), C.byref(c)) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_vcf_index_lines(b"a\n", 2, 0, 4, 2, buf, buf, buf, buf, C.byref(n), C.byref(c)) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_vcf_index_lines(None, 0, 0, 0, 0, None, None, None, None, C.byref(n), C.byref(c)) == _capi.OK and n.value == 0 and c.value == 0


def test_vcf_index_lines_fuzzed_under_asan_ubsan(tmp_path):
    """host_pure.cpp (the same source libpgen_hip.so is built from) with ASan + UBSan and tests/fuzz_vcf.cpp: random byte soups of
    tabs, newlines and digits in exactly-sized allocations, every result held against a naive walk."""
    exe = tmp_path / "fuzz_vcf"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(REPO / "include"),
           "-o", str(exe), str(REPO / "tests" / "fuzz_vcf.cpp"), str(REPO / "pgen_rs_amd" / "csrc" / "host_pure.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), "30000", "2031"], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "fuzz_vcf: 30000 iterations" in p.stdout


# ---- constants and prototypes -----------------------------------------------------------------------------------------------------------
def test_constants_and_header_lines():
    header = (REPO / "include" / "pgen_hip.h").read_text()
    for name, value in [("PARSE_AUTO", 0), ("PARSE_GENERAL", 1), ("PARSE_FIXED", 2), ("PARSE_SHAPE_MASK", 0xF), ("PARSE_FIELD_COUNT", 1),
                        ("PARSE_BAD_CALL", 2), ("PARSE_ALLELE_RANGE", 4), ("PARSE_HALF_CALL", 8), ("PARSE_HAPLOID", 0x10), ("PARSE_PHASED", 0x20),
                        ("PARSE_DECLINED", 0x40), ("VCF_LAST_BLOCK", 1)]:
        assert getattr(_capi, name) == value
        m = re.search(rf"#define PGENHIP_{name}\s+(0x[0-9A-Fa-f]+|\d+)u", header)
        assert m and int(m.group(1), 0) == value, name
    assert _capi.KNOB_PARSE_BLOCKS == 29 and re.search(r"PGENHIP_KNOB_PARSE_BLOCKS = 29,", header)
    assert (parse_ref.FIELD_COUNT, parse_ref.BAD_CALL, parse_ref.ALLELE_RANGE, parse_ref.HALF_CALL, parse_ref.HAPLOID, parse_ref.PHASED,
            parse_ref.DECLINED) == (_capi.PARSE_FIELD_COUNT, _capi.PARSE_BAD_CALL, _capi.PARSE_ALLELE_RANGE, _capi.PARSE_HALF_CALL,
                                    _capi.PARSE_HAPLOID, _capi.PARSE_PHASED, _capi.PARSE_DECLINED)
    for sym in ("pgenhip_parse_gt", "pgenhip_vcf_index_lines"):
        assert sym in _capi.PROTOTYPES and getattr(_capi.lib, sym) is not None
        assert re.search(rf"^int {sym}\(", header, flags=re.M)
    assert "#define PGENHIP_ABI_VERSION 2" in header.replace("2u", "2")


def test_null_ctx_is_refused():
    assert _capi.lib.pgenhip_parse_gt(None, None, 0, None, None, 0, None, 0, None, 0) == _capi.ERR_BAD_ARG
    assert _capi.lib.pgenhip_tune(None, _capi.KNOB_PARSE_BLOCKS, 1) == _capi.ERR_BAD_ARG


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_twin_matches_the_header():
    assert parse_plan.PIECE_SAMPLES == 4 * parse_plan.PIECE_BYTES and parse_plan.PIECE_TEXT == 4 * parse_plan.PIECE_SAMPLES
    assert parse_plan.CHUNK_BYTES == parse_plan.THREADS * parse_plan.CHUNK_LANE_BYTES and parse_plan.WAVES * 64 == parse_plan.THREADS
    assert parse_plan.BLOCK_PIECES == parse_plan.THREADS * parse_plan.LANE_PIECES
    sizes = list(range(0, 70)) + [255, 256, 257, 511, 512, 513, 626, 1024, 125000, 2**29]
    for r in sizes:
        assert parse_plan.probe("parse_pieces", 3, r) == (parse_plan.pieces_per_line(r), parse_plan.rows_per_block(r), parse_plan.blocks_per_row(r))
        for piece in (0, 1, parse_plan.pieces_per_line(r) - 1, parse_plan.pieces_per_line(r)):
            assert parse_plan.probe("parse_piece_bytes", 2, r, piece) == parse_plan.piece_bytes(r, piece)
        for n_lines in (1, 2, 70, 100_000, 2**32 - 1):
            for num_cus, blocks in ((256, 0), (0, 0), (304, 0), (256, 1), (256, 7)):
                assert parse_plan.probe("parse_fixed_plan", 3, r, n_lines, num_cus, blocks) == parse_plan.fixed_plan(r, n_lines, num_cus, blocks)
                for region, lead in ((0, 0), (1, 3), (parse_plan.CHUNK_BYTES, 0), (parse_plan.CHUNK_BYTES, 1), (4 * r, 2)):
                    assert parse_plan.probe("parse_general", 2, n_lines, num_cus, blocks, region, lead) == (
                        parse_plan.general_grid(n_lines, num_cus, blocks), parse_plan.general_chunks(region, lead))


def test_fixed_items_tile_every_line_once():
    for r in list(range(0, 40)) + [255, 256, 257, 1023, 1024, 1025, 17501]:
        pieces, total, _ = parse_plan.fixed_plan(r, 3)
        assert total == 3 * pieces
        covered = np.zeros(r, dtype=np.int32)
        for p in range(pieces):
            b, e = parse_plan.probe("parse_piece_bytes", 2, r, p)
            assert b <= e <= r and e - b <= parse_plan.PIECE_BYTES
            covered[b:e] += 1
        assert (covered == 1).all(), r
    assert parse_plan.edge_sample_counts() == sorted(set(parse_plan.edge_sample_counts())) and len(parse_plan.edge_sample_counts()) >= 3


def test_plans_at_the_far_end_of_the_item_range():
    """The launches of tests/test_long_rows_parse_gpu.py on both sides of 2^32 items, and the most lines of the longest rows: ``total``
    is not truncated and the grids equal their caps."""
    cap = 256 * parse_plan.BLOCKS_PER_CU
    for r, n_lines, total in ((1025, 4_190_208, 4_294_963_200), (1025, 4_190_211, 2**32 - 1021), (1025, 4_190_213, 4_294_968_325),
                              (2**29, 2**32 - 1, 2**61 - 2**29)):
        for blocks in (0, 7):
            want = (r, total, blocks or cap)
            assert parse_plan.fixed_plan(r, n_lines, 256, blocks) == want
            assert parse_plan.probe("parse_fixed_plan", 3, r, n_lines, 256, blocks) == want
    for num_cus, blocks in ((256, 0), (0, 0), (304, 0), (256, 3)):
        want = blocks or (num_cus or 256) * parse_plan.BLOCKS_PER_CU
        assert parse_plan.general_grid(2**32 - 1, num_cus, blocks) == want
        assert parse_plan.probe("parse_general", 2, 2**32 - 1, num_cus, blocks, 0, 0)[0] == want


def test_fixed_items_tile_every_line_once_around_2_32():
    """The tiling property on a window of items around 2^32: item i is piece i % P of line i // P.  A host loop as the FIXED kernel's
    (blocks of BLOCK_PIECES items by grid stride, LANE_PIECES items per lane, THREADS apart) over the last two turns of the launch
    only: every item of the window is taken once, none at or past ``total``, and the items of the lines that lie wholly inside the
    window are every piece of that line once, with the piece's record bytes from the header."""
    r = 1025
    for n_lines in (4_190_208, 4_190_211, 4_190_213):
        pieces, total, grid = parse_plan.fixed_plan(r, n_lines)
        bp, threads = parse_plan.BLOCK_PIECES, parse_plan.THREADS
        turn = grid * bp
        first_turn = max(0, -(-total // turn) - 2)
        lane_items = (np.arange(parse_plan.LANE_PIECES, dtype=np.int64)[:, None] * threads + np.arange(threads, dtype=np.int64)[None, :]).reshape(-1)
        taken, masked_off = [], 0
        for block in range(grid):
            for i0 in range(block * bp + first_turn * turn, total, turn):
                at = i0 + lane_items
                taken.append(at[at < total])
                masked_off += int((at >= total).sum())
        taken = np.sort(np.concatenate(taken))
        lo = first_turn * turn
        assert lo < 2**32 - bp and np.array_equal(taken, np.arange(lo, total, dtype=np.int64))   # every item once, none at or past total
        assert masked_off == -total % bp and (int(taken[-1]) >= 2**32) == (n_lines == 4_190_213)
        j0 = -(-lo // pieces)   # the lines wholly inside the window: every piece once, in order
        inside = taken[taken >= j0 * pieces]
        assert np.array_equal(inside // pieces, np.repeat(np.arange(j0, n_lines, dtype=np.int64), pieces))
        assert np.array_equal(inside % pieces, np.tile(np.arange(pieces, dtype=np.int64), n_lines - j0))
        j = n_lines - 1
        assert [parse_plan.probe("parse_piece_bytes", 2, r, i % pieces) for i in (j * pieces, (j + 1) * pieces - 1)] == [(0, 1), (r - 1, r)]


# ---- the import command, up to the device -----------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([str(CLI), *args], capture_output=True)


VCF = (b"##fileformat=VCFv4.2\n##source=pgen-rs\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts0\ts1\ts2\n"
       b"1\t10\tr1\tA\tG\t.\t.\t.\tGT\t0/0\t0/1\t1/1\n")


def test_import_usage_and_input_errors(tmp_path):
    usage = run("--help")
    assert b"import" in usage.stdout + usage.stderr
    assert run("import").returncode == 2                                       # no input
    assert run("import", str(tmp_path / "a.vcf")).returncode == 2               # no -o
    assert run("import", str(tmp_path / "a.vcf"), "-o", str(tmp_path / "o"), "--frobnicate").returncode == 2
    p = run("import", str(tmp_path / "missing.vcf"), "-o", str(tmp_path / "o"))
    assert p.returncode == 101 and p.stderr
    for body, what in ((VCF.replace(b"\tFORMAT", b"\tFMT"), b"FORMAT"), (VCF.replace(b"\ts0\ts1\ts2", b""), b"sample"),
                       (b"##fileformat=VCFv4.2\n", b"#CHROM")):
        (tmp_path / "bad.vcf").write_bytes(body)
        p = run("import", str(tmp_path / "bad.vcf"), "-o", str(tmp_path / "o"))
        assert p.returncode == 101 and what in p.stderr, p.stderr
        assert not list(tmp_path.glob("o.*"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_import_without_a_device_exits_101_and_leaves_no_file(tmp_path):
    (tmp_path / "a.vcf").write_bytes(VCF)
    p = run("import", str(tmp_path / "a.vcf"), "-o", str(tmp_path / "o"))
    assert p.returncode == 101 and b"no" in p.stderr.lower()
    assert not list(tmp_path.glob("o.*"))
