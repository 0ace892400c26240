"""The launch plan of gt_parse.hip (csrc/launch_plan.h, namespace plan::parse) as a Python twin, for the tests that are placed
around its constants.  ``probe`` is the header itself, run through tests/parse_plan_probe.cpp (built and loaded by
tests/launch_plan.py, as every probe is); tests/test_parse_gt.py holds every function below against it."""
from __future__ import annotations

import functools

import launch_plan

probe = functools.partial(launch_plan.call_into, launch_plan.load("parse_plan_probe"))

# the constants are read, not restated: the twin is the arithmetic on top of them
(THREADS, WAVES, BLOCKS_PER_CU, PIECE_BYTES, PIECE_SAMPLES, PIECE_TEXT, CHUNK_LANE_BYTES, CHUNK_BYTES, AUTO_FIXED_FIRST, LANE_PIECES,
 BLOCK_PIECES) = probe("parse_constants", 11)


def pieces_per_line(record_size: int) -> int:
    """FIXED: work items of a line; a line of no samples has one, which only checks that the region is empty."""
    return 1 if record_size == 0 else -(-record_size // PIECE_BYTES)


def piece_bytes(record_size: int, piece: int) -> tuple[int, int]:
    """Record bytes [begin, end) of one piece."""
    return min(piece * PIECE_BYTES, record_size), min((piece + 1) * PIECE_BYTES, record_size)


def rows_per_block(record_size: int) -> int:
    """FIXED: whole lines of short rows that share a block."""
    return max(1, BLOCK_PIECES // pieces_per_line(record_size))


def blocks_per_row(record_size: int) -> int:
    """FIXED: blocks a long row spreads over."""
    return -(-pieces_per_line(record_size) // BLOCK_PIECES)


def grid_blocks(work: int, per_cu: int, num_cus: int, forced: int) -> int:
    cap = forced if forced > 0 else (num_cus if num_cus > 0 else 256) * per_cu
    return max(1, min(work, cap))


def fixed_plan(record_size: int, n_lines: int, num_cus: int = 256, blocks: int = 0) -> tuple[int, int, int]:
    """(pieces per line, items, grid) of a FIXED launch."""
    pieces = pieces_per_line(record_size)
    total = n_lines * pieces
    return pieces, total, grid_blocks(-(-total // BLOCK_PIECES), BLOCKS_PER_CU, num_cus, blocks)


def general_grid(n_lines: int, num_cus: int = 256, blocks: int = 0) -> int:
    """GENERAL: a block per line, the rest by grid stride."""
    return grid_blocks(n_lines, BLOCKS_PER_CU, num_cus, blocks)


def general_chunks(region_bytes: int, lead: int) -> int:
    """GENERAL: chunks of a region that starts ``lead`` bytes behind a 4-byte boundary."""
    return -(-(region_bytes + lead) // CHUNK_BYTES)


def edge_sample_counts() -> list[int]:
    """Sample counts N at which a plan quantity steps, for fixed-width text (4 N bytes per line): a GENERAL chunk (and two, and
    one more lane's worth of lead), a FIXED row that fills one step of a block's lanes, one block's turn and two, and the
    rows-per-block step 2 -> 1."""
    edges = {CHUNK_BYTES // 4, 2 * CHUNK_BYTES // 4, 4 * PIECE_BYTES * THREADS, 4 * PIECE_BYTES * BLOCK_PIECES, 8 * PIECE_BYTES * BLOCK_PIECES,
             4 * PIECE_BYTES * (BLOCK_PIECES // 2)}
    return sorted(edges)
