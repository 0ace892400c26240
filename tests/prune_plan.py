"""The launch plan of gt_prune.hip (csrc/launch_plan.h, namespace plan::prune) as a Python twin, for the tests that are placed around
its constants.  ``probe`` is the header itself, run through tests/prune_plan_probe.cpp (built and loaded by tests/launch_plan.py, as
every probe is); tests/test_prune.py holds every function below against it."""
from __future__ import annotations

import functools

import launch_plan

probe = functools.partial(launch_plan.call_into, launch_plan.load("prune_plan_probe"))

# the constants are read, not restated: the twin is the arithmetic on top of them
THREADS, BLOCKS_PER_CU, CHUNK_ROWS, HALO_ROWS, LDS_ROWS = probe("prune_constants", 5)


def grid_blocks(work: int, per_cu: int, num_cus: int, forced: int) -> int:
    cap = forced if forced > 0 else (num_cus if num_cus > 0 else 256) * per_cu
    return max(1, min(work, cap))


def mask_words(window: int) -> int:
    return (window + 31) // 32


def halo_rows(window: int) -> int:
    """BLOCK: rows on either side of a turn whose states are staged in LDS."""
    return min(window, HALO_ROWS)


def general_grid(n_rows: int, num_cus: int = 256, blocks: int = 0) -> int:
    """GENERAL: a lane per row."""
    return grid_blocks(-(-n_rows // THREADS), BLOCKS_PER_CU, num_cus, blocks)


def block_plan(n_rows: int, num_cus: int = 256, blocks: int = 0) -> tuple[int, int]:
    """BLOCK: (rows of a workgroup's range, grid).  Block b owns [b * range, min((b + 1) * range, n_rows)), in turns of CHUNK_ROWS."""
    rows = max(n_rows, 1)
    want = min(blocks, rows) if blocks > 0 else grid_blocks(-(-rows // CHUNK_ROWS), BLOCKS_PER_CU, num_cus, 0)
    range_rows = -(-rows // want)
    return range_rows, -(-rows // range_rows)


def turn_edges(n_rows: int, num_cus: int = 256, blocks: int = 0) -> list[int]:
    """First rows of every turn of every block: where a BLOCK launch stages anew."""
    range_rows, grid = block_plan(n_rows, num_cus, blocks)
    return [r for b in range(grid) for r in range(b * range_rows, min((b + 1) * range_rows, n_rows), CHUNK_ROWS)]


def auto_block(n_rows: int, window: int) -> bool:
    """AUTO's rule: BLOCK on every shape."""
    return True
