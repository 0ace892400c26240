"""The launch plan of the per-sample count kernel, RUN from csrc/launch_plan.h (namespace plan::scount) through tests/launch_plan.py
rather than restated, so that the tests can place their cells on both sides of every edge it has: the lanes-per-row ladder (one
column tile up to 64 chunks), the column tiles past it, the 8-row carry-save batch, the 255-batch flush window of a slot and the
row ranges (slices) a tile is cut into.  Only the helpers that lay out test sizes (``window_rows``, ``counter_capacity``,
``CLASS_EDGES``) are Python, on top of probed values.
"""
from __future__ import annotations

import launch_plan as L

THREADS = L.CONST["scount.kThreads"]
WAVES = L.CONST["scount.kWaves"]
BATCH = L.CONST["scount.kBatch"]                    # rows per carry-save batch
HI_BITS = L.CONST["scount.kHiBits"]                 # planes of a counter's batch count
WINDOW_BATCHES = L.CONST["scount.kWindowBatches"]   # batches between flushes

AUTO, ROWS = 0, 2       # PGENHIP_SCOUNT_* (include/pgen_hip.h)
ACCUMULATE = 0x10


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def plan(n: int, v: int = 1, forced: int = 0, num_cus: int = 256):
    """(G, tiles, cols, slices, lds_bytes, slots) of a launch over V rows of N samples."""
    return L.call("scount_plan", 6, record_size(n), v, num_cus, forced)


def columns(n: int) -> int:
    """Column chunks of a row: 16 record bytes = 64 samples each."""
    return (record_size(n) + 15) // 16


def lanes_per_row(n: int) -> int:
    return plan(n)[0]


def tiles(n: int) -> int:
    return plan(n)[1]


def slices(n: int, v: int, forced: int = 0, num_cus: int = 256) -> int:
    return plan(n, v, forced, num_cus)[3]


def slots(n: int) -> int:
    """Rows a block has side by side (4 waves x 64 / G groups)."""
    return plan(n)[5]


def window_rows(n: int, slices: int) -> int:
    """Rows of a launch that fill every slot of every slice's first flush window exactly (one row more opens a second)."""
    return slices * slots(n) * BATCH * WINDOW_BATCHES


def counter_capacity() -> int:
    """The most rows a bit-sliced counter holds: every hi plane set, and ones + 2 twos + 4 fours = 7 on top."""
    return BATCH * ((1 << HI_BITS) - 1) + BATCH - 1


def hi_planes(batches: int) -> int:
    """The hi planes a flush reads after ``batches`` batches (``n_hi``): a counter is then at most 8 * batches."""
    return L.call("scount_hi_planes", 1, batches)[0]


# N at the ladder's edges: the last N of a lanes-per-row class and the first of the next; then the first two-tile N
CLASS_EDGES = [256, 512, 1024, 2048, 4096, 8192]
