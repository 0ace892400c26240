"""The launch plan of the per-sample count kernel, restated from csrc/gt_scount.hip so that the tests can place their cells on
both sides of every edge it has: the lanes-per-row ladder (one column tile up to 64 chunks), the column tiles past it, the
8-row carry-save batch, the 255-batch flush window of a slot and the row ranges (slices) a tile is cut into.

Mirrors (keep in step; test_sample_counts.py checks them against the source):
  * ``kThreads``, ``kBatch``, ``kHiBits`` / ``kWindowBatches``, and ``n_hi``, the hi planes a flush reads;
  * the ladder of ``plan`` (``C <= 4 ? 4 : ...``) and its tiles;
  * the rows of a block, ``rbeg = V * slice / slices``.
"""
from __future__ import annotations

THREADS = 256
WAVES = THREADS // 64
BATCH = 8               # kBatch
HI_BITS = 8             # kHiBits: planes of a counter's batch count
WINDOW_BATCHES = 255    # kWindowBatches = 2^kHiBits - 1

AUTO, ROWS = 0, 2       # PGENHIP_SCOUNT_* (include/pgen_hip.h)
ACCUMULATE = 0x10


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def columns(n: int) -> int:
    """Column chunks of a row: 16 record bytes = 64 samples each."""
    return (record_size(n) + 15) // 16


def lanes_per_row(n: int) -> int:
    c = columns(n)
    for g in (4, 8, 16, 32):
        if c <= g:
            return g
    return 64


def tiles(n: int) -> int:
    g = lanes_per_row(n)
    return (columns(n) + g - 1) // g


def slots(n: int) -> int:
    """Rows a block has side by side (4 waves x 64 / G groups)."""
    return WAVES * (64 // lanes_per_row(n))


def window_rows(n: int, slices: int) -> int:
    """Rows of a launch that fill every slot of every slice's first flush window exactly (one row more opens a second)."""
    return slices * slots(n) * BATCH * WINDOW_BATCHES


def counter_capacity() -> int:
    """The most rows a bit-sliced counter holds: every hi plane set, and ones + 2 twos + 4 fours = 7 on top."""
    return BATCH * ((1 << HI_BITS) - 1) + BATCH - 1


def hi_planes(batches: int) -> int:
    """The hi planes a flush reads after ``batches`` batches (``n_hi``): a counter is then at most 8 * batches."""
    return max(batches, 1).bit_length()


# N at the ladder's edges: the last N of a lanes-per-row class and the first of the next; then the first two-tile N
CLASS_EDGES = [256, 512, 1024, 2048, 4096, 8192]
