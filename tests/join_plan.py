"""The launch plan of gt_join.hip (csrc/launch_plan.h, namespace plan::join) as a Python twin, for the tests that are placed around
its constants.  ``probe`` is the header itself, run through tests/join_plan_probe.cpp (built and loaded by tests/launch_plan.py, as
every probe is); tests/test_join_records.py holds every function below against it."""
from __future__ import annotations

import functools

import launch_plan

probe = functools.partial(launch_plan.call_into, launch_plan.load("join_plan_probe"))

# the constants are read, not restated: the twin is the arithmetic on top of them
THREADS, BLOCKS_PER_CU, CHUNK_BYTES = probe("join_constants", 3)


def grid_blocks(work: int, per_cu: int, num_cus: int, forced: int) -> int:
    cap = forced if forced > 0 else (num_cus if num_cus > 0 else 256) * per_cu
    return max(1, min(work, cap))


def general_grid(n_variants: int, record_size: int, num_cus: int = 256, blocks: int = 0) -> int:
    """GENERAL: a lane per output byte."""
    return grid_blocks(-(-n_variants * record_size // THREADS), BLOCKS_PER_CU, num_cus, blocks)


def chunks_per_row(record_size: int) -> int:
    """STREAM: the most aligned chunks a row can touch, whatever its address."""
    return (record_size + 2 * CHUNK_BYTES - 2) // CHUNK_BYTES


def chunk_bytes(record_size: int, mis: int, chunk: int) -> tuple[int, int]:
    """Row bytes [begin, end) under one chunk of a row that starts ``mis`` bytes behind a chunk boundary."""
    b0 = CHUNK_BYTES * chunk - mis
    lo = min(max(b0, 0), record_size)
    return lo, max(lo, min(b0 + CHUNK_BYTES, record_size))


def stream_paths(sizes, dmis: int) -> list[tuple]:
    """The class of every chunk of one output row of parts ``sizes`` (all present) that starts ``dmis`` bytes behind a chunk boundary,
    as gt_join_stream_kernel sorts them (gt_join.hip; the conditions are the kernel's, in its order):
      ("edge", None, None, None)      `b0 >= 0 && last >= 15` fails: the row's head or tail, bytes through join_dword
      ("dword", p, phase, depth)      a whole chunk built by four join_dword calls; p, phase and depth are None where the 64 samples
                                      span parts (`s0 >= pt.start && s0 - pt.start + 64u <= pt.count` holds for no part), else the
                                      part's index, `ls & 3` and `rp - sb` (< 20: `sb + 20u <= rp` fails)
      ("fast", p, phase, depth)       the 16 + 4-byte load, funnel-shifted by ph = 2 * (ls & 3): phase = `ls & 3`, depth = `rp - sb`
    Chunks with no byte of the row (`b0 >= R || b0 + kChunkBytes <= 0`) are left out."""
    starts = [sum(sizes[:p]) for p in range(len(sizes))]
    r = (sum(sizes) + 3) // 4
    out = []
    for c in range(chunks_per_row(r)):
        b0 = CHUNK_BYTES * c - dmis
        if b0 >= r or b0 + CHUNK_BYTES <= 0:
            continue
        last = r - 1 - b0
        if not (b0 >= 0 and last >= CHUNK_BYTES - 1):
            out.append(("edge", None, None, None))
            continue
        s0 = 4 * b0
        kind = ("dword", None, None, None)
        for p, (start, count) in enumerate(zip(starts, sizes)):
            if s0 >= start and s0 - start + 64 <= count:
                ls = s0 - start
                sb, rp = ls >> 2, (count + 3) >> 2
                kind = ("fast" if sb + 20 <= rp else "dword", p, ls & 3, rp - sb)
        out.append(kind)
    return out


def rows_per_block(record_size: int) -> int:
    """STREAM: whole rows of short records that share a block."""
    return max(1, THREADS // chunks_per_row(record_size))


def blocks_per_row(record_size: int) -> int:
    """STREAM: blocks a long row spreads over."""
    return -(-chunks_per_row(record_size) // THREADS)


def stream_plan(record_size: int, n_variants: int, num_cus: int = 256, blocks: int = 0) -> tuple[int, int, int]:
    """(chunks per row, items, grid) of a STREAM launch."""
    chunks = chunks_per_row(record_size)
    total = n_variants * chunks
    return chunks, total, grid_blocks(-(-total // THREADS), BLOCKS_PER_CU, num_cus, blocks)


def auto_stream(record_size: int, n_variants: int, n_parts: int) -> bool:
    """AUTO's rule: STREAM on every shape."""
    return True


def edge_record_sizes() -> list[int]:
    """Record sizes R at which a plan quantity steps: one chunk and two, the rows-per-block step 2 -> 1, a row that fills one
    block's turn and one chunk more."""
    c, t = CHUNK_BYTES, THREADS
    return sorted({1, 2, c, c + 1, c + 2, (t // 2 - 1) * c + 2, (t // 2) * c + 2, (t - 1) * c + 2, (t - 1) * c + 3, t * c + 2, t * c + 3})
