"""The launch plan of the per-sample score kernel, restated from csrc/gt_score.hip so that the tests can place their row counts on
both sides of every edge it has: the bytes a lane owns (by the number of columns), the lanes-per-row ladder and the column tiles
past 64 lanes, the rows a block has side by side, the batch of rows whose loads are issued together, and the row ranges (slices)
a tile is cut into.

Mirrors (keep in step; test_sample_scores.py checks them against the source):
  * ``lane_bytes`` and ``batch_rows``;
  * ``plan``: units, ``log_g``, tiles, the cap of the slices at one batch of every slot;
  * the rows of a block, ``rbeg = V * slice / slices``.
"""
from __future__ import annotations

THREADS = 256
WAVES = THREADS // 64
MIN_SLICE_ROWS = 512    # kMinSliceRows (only when the slices are not forced)

AUTO, ROWS = 0, 1       # PGENHIP_SCORE_* (include/pgen_hip.h)
ACCUMULATE = 0x10
MAX_COLUMNS = 8


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def lane_bytes(c: int) -> int:
    return 4 if c <= 2 else 2 if c <= 4 else 1


def batch_rows(c: int) -> int:
    return 4 if c <= 4 else 2


def units(n: int, c: int) -> int:
    b = lane_bytes(c)
    return (record_size(n) + b - 1) // b


def lanes_per_row(n: int, c: int) -> int:
    g = 1
    while g < 64 and g < units(n, c):
        g *= 2
    return g


def tiles(n: int, c: int) -> int:
    g = lanes_per_row(n, c)
    return (units(n, c) + g - 1) // g


def slots(n: int, c: int) -> int:
    """Rows a block has side by side (4 waves x 64 / G groups)."""
    return WAVES * (64 // lanes_per_row(n, c))


def step_rows(n: int, c: int) -> int:
    """Rows of one batch of every slot of a block: a launch has at most ceil(V / step_rows) slices."""
    return slots(n, c) * batch_rows(c)


def slices(n: int, c: int, v: int, forced: int) -> int:
    return max(1, min(forced, (v + step_rows(n, c) - 1) // step_rows(n, c)))


def edge_rows(n: int, c: int, forced: int) -> list[int]:
    """Row counts on both sides of every edge: one slot row, one batch, the cap of the forced slices, a second batch per slice."""
    s, st = slots(n, c), step_rows(n, c)
    vs = {1, s - 1, s, s + 1, st - 1, st, st + 1, forced * st - 1, forced * st, forced * st + 1, 2 * forced * st + forced + 1}
    return sorted(v for v in vs if v >= 1)
