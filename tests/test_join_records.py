"""Sample-wise join of records — CPU leg: the numpy reference (tests/join_ref.py) against hand-written cases, the ABI's constants
and prototype, and the plan twin (tests/join_plan.py) against the plan header over every plan edge."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

import join_plan
import join_ref as JR
import pack_ref as PR
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent


def rec(codes):
    return PR.pack_codes(np.array([codes], dtype=np.uint8))[0]


def test_reference_two_parts_with_a_flip():
    # part 0: 3 samples (one byte, dirty pad bits), part 1: 5 samples (two bytes, dirty pad bits), two rows; part 1 flipped in row 1
    a0, a1 = rec([0, 1, 2]) | 0xC0, rec([3, 2, 1]) | 0xC0
    b0, b1 = rec([2, 2, 0, 1, 3]), rec([0, 2, 1, 3, 0])
    b0[1] |= 0xFC
    b1[1] |= 0xFC
    base_a = np.concatenate([[0xFF], a0, [0xFF], a1]).astype(np.uint8)            # records at bytes 1 and 3
    base_b = np.concatenate([[0xFF], b1, [0xFF, 0xFF], b0]).astype(np.uint8)      # row 0 at byte 5, row 1 at byte 1
    got = JR.join([(base_a, [1, 3], 3, None), (base_b, [5, 1], 5, np.array([0, 1], dtype=np.uint8))], 2)
    # row 0: 0 1 2 | 2 2 0 1 3            row 1: 3 2 1 | flip(0 2 1 3 0) = 2 0 1 3 2
    want = np.array([[0 | 1 << 2 | 2 << 4 | 2 << 6, 2 | 0 << 2 | 1 << 4 | 3 << 6],
                     [3 | 2 << 2 | 1 << 4 | 2 << 6, 0 | 1 << 2 | 3 << 4 | 2 << 6]], dtype=np.uint8)
    assert got.dtype == np.uint8 and (got == want).all()


def test_reference_absent_row_and_empty_part():
    a = rec([1, 1, 1])
    b = rec([0, 2, 0, 2, 1])
    parts = [(a, [0, JR.ABSENT], 3, np.array([1, 1], dtype=np.uint8)), (np.zeros(0, np.uint8), [0, 0], 0, None), (b, [JR.ABSENT, 0], 5, None)]
    got = JR.join(parts, 2)
    # row 0: 1 1 1 | 3 3 3 3 3 (the flip leaves code 1)      row 1: 3 3 3 | 0 2 0 2 1; N_out = 8: no pad bits
    assert got.tolist() == [[1 | 1 << 2 | 1 << 4 | 3 << 6, 0xFF], [3 | 3 << 2 | 3 << 4 | 0 << 6, 2 | 0 << 2 | 2 << 4 | 1 << 6]]
    # nine samples: the last byte holds one code and six zero pad bits
    got = JR.join([(a, [0], 3, None), (b, [0], 5, None), (rec([3]), [JR.ABSENT], 1, None)], 1)
    assert got.shape == (1, 3) and got[0, 2] == 3


def test_constants_and_prototype():
    assert (_capi.JOIN_AUTO, _capi.JOIN_GENERAL, _capi.JOIN_STREAM, _capi.JOIN_MAX_PARTS, _capi.KNOB_JOIN_BLOCKS) == (0, 1, 2, 8, 30)
    assert _capi.JOIN_ABSENT == 2**64 - 1 and np.array([JR.ABSENT], dtype=np.int64).view(np.uint64)[0] == _capi.JOIN_ABSENT
    text = (REPO / "include" / "pgen_hip.h").read_text()
    for name, value in (("PGENHIP_JOIN_MAX_PARTS", "8u"), ("PGENHIP_JOIN_ABSENT", "UINT64_MAX"), ("PGENHIP_JOIN_AUTO", "0u"),
                        ("PGENHIP_JOIN_GENERAL", "1u"), ("PGENHIP_JOIN_STREAM", "2u")):
        assert f"#define {name} {value}" in text
    assert "PGENHIP_KNOB_JOIN_BLOCKS = 30," in text
    assert C.sizeof(_capi.JoinPart) == 32 and _capi.JoinPart.sample_count.offset == 24 and _capi.JoinPart.reserved.offset == 28
    assert _capi.lib.pgenhip_join_records(None, None, 0, 0, None, 0, 0) == _capi.ERR_BAD_ARG   # a NULL ctx is refused, not dereferenced
    assert _capi.lib.pgenhip_abi_version() == 2


def test_capi_symbols_still_pass():
    proc = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", str(REPO / "tests" / "test_capi_symbols.py")],
                          capture_output=True, text=True, cwd=REPO)
    assert proc.returncode == 0, proc.stdout + proc.stderr


def test_plan_twin_matches_header():
    assert (join_plan.THREADS, join_plan.CHUNK_BYTES) == (256, 16) and join_plan.THREADS % 64 == 0
    sizes = sorted(set(list(range(1, 70)) + join_plan.edge_record_sizes() + [626, 17501, 125000, 2**29]))
    for r in sizes:
        chunks = join_plan.chunks_per_row(r)
        assert join_plan.probe("join_chunks", 3, r) == (chunks, join_plan.rows_per_block(r), join_plan.blocks_per_row(r))
        for mis in (0, 1, 15):
            for c in (0, 1, chunks - 1, chunks):
                assert join_plan.probe("join_chunk_bytes", 2, r, mis, c) == join_plan.chunk_bytes(r, mis, c)
        for v in (1, 2, 257, 100_000, 2**32 - 1):
            for num_cus, blocks in ((256, 0), (0, 0), (304, 0), (256, 1), (256, 3)):
                assert join_plan.probe("join_stream_plan", 3, r, v, num_cus, blocks) == join_plan.stream_plan(r, v, num_cus, blocks)
                assert join_plan.probe("join_general_grid", 1, v, r, num_cus, blocks)[0] == join_plan.general_grid(v, r, num_cus, blocks)
            for n_parts in (1, 2, 8):
                assert bool(join_plan.probe("join_auto", 1, r, v, n_parts)[0]) == join_plan.auto_stream(r, v, n_parts)


def test_stream_paths_classifier_by_hand():
    # R = 101 bytes at phase 0: chunks 0..5 whole, chunk 6 the tail.  Part 1 (100 bytes) starts at sample 1: ls & 3 == 3 in all its chunks
    got = join_plan.stream_paths((1, 400), 0)
    assert got[0] == ("dword", None, None, None) and got[-1] == ("edge", None, None, None) and len(got) == 7
    assert got[1] == ("fast", 1, 3, 100 - 15) and got[5] == ("fast", 1, 3, 100 - 79)
    assert join_plan.stream_paths((1, 400), 1)[:2] == [("edge", None, None, None), ("fast", 1, 3, 100 - 14)]
    assert join_plan.stream_paths((3,), 5) == [("edge", None, None, None)]
    # one part, 80 samples = 20 bytes: the only whole chunk is byte 0's, exactly 20 bytes deep; one byte less and it is not
    assert join_plan.stream_paths((80,), 0) == [("fast", 0, 0, 20), ("edge", None, None, None)]
    assert join_plan.stream_paths((76,), 0) == [("dword", 0, 0, 19), ("edge", None, None, None)]


def test_gpu_size_lists_reach_every_stream_path():
    """The size lists of tests/test_join_records_gpu.py, at all 16 address phases of an output row, reach: the fast path at every bit
    phase; a whole chunk inside one part 19, 20 and 21 bytes from the record's end (the last that misses the fast path and the first
    two that take it) at every bit phase; the fast path in the first, a middle and the last part of an eight-part table."""
    import test_join_records_gpu as G

    fast, depth, eight = set(), set(), set()
    for sizes in G.SIZES + [G.PHASE_SIZES]:
        for dmis in range(16):
            for kind, p, phase, deep in join_plan.stream_paths(sizes, dmis):
                if p is None:
                    continue
                assert kind == ("fast" if deep >= 20 else "dword")
                if kind == "fast":
                    fast.add(phase)
                    if len(sizes) == 8:
                        eight.add(p)
                if deep in (19, 20, 21):
                    depth.add((phase, deep))
    assert fast == {0, 1, 2, 3}, f"fast path only at ls & 3 in {sorted(fast)}"
    assert depth == {(ph, d) for ph in range(4) for d in (19, 20, 21)}, f"rp - sb reached: {sorted(depth)}"
    assert 0 in eight and 7 in eight and eight & set(range(1, 7)), f"fast path in parts {sorted(eight)} of eight"


def test_stream_chunks_tile_every_row_once():
    """Whatever the row's address, the chunks of the plan cover each of its bytes once, in order, 16 at the most each."""
    for r in sorted(set(list(range(1, 50)) + join_plan.edge_record_sizes() + [17501])):
        chunks = join_plan.chunks_per_row(r)
        for mis in range(16):
            covered = np.zeros(r, dtype=np.int32)
            for c in range(chunks):
                b, e = join_plan.probe("join_chunk_bytes", 2, r, mis, c)
                assert b <= e <= r and e - b <= join_plan.CHUNK_BYTES
                covered[b:e] += 1
            assert (covered == 1).all(), (r, mis)
        assert join_plan.probe("join_chunk_bytes", 2, r, 15, chunks) == (r, r)   # nothing behind the last chunk


def test_plans_at_the_far_end_of_the_item_range():
    cap = 256 * join_plan.BLOCKS_PER_CU
    for r, v in ((2**29, 2**32 - 1), (125000, 2**32 - 1)):
        chunks = join_plan.chunks_per_row(r)
        for blocks in (0, 3):
            want = (chunks, v * chunks, blocks or cap)
            assert join_plan.stream_plan(r, v, 256, blocks) == want == join_plan.probe("join_stream_plan", 3, r, v, 256, blocks)
            assert join_plan.probe("join_general_grid", 1, v, r, 256, blocks)[0] == (blocks or cap)
