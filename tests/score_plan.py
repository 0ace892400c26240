"""The launch plan of the per-sample score kernel, RUN from csrc/launch_plan.h (namespace plan::score) through tests/launch_plan.py
rather than restated, so that the tests can place their row counts on both sides of every edge it has: the bytes a lane owns (by
the number of columns), the lanes-per-row ladder and the column tiles past 64 lanes, the rows a block has side by side, the batch
of rows whose loads are issued together, and the row ranges (slices) a tile is cut into.  Only ``edge_rows``, which lays out test
sizes, is Python, on top of probed values.
"""
from __future__ import annotations

import launch_plan as L

THREADS = L.CONST["score.kThreads"]
WAVES = L.CONST["score.kWaves"]
MIN_SLICE_ROWS = L.CONST["score.kMinSliceRows"]    # only when the slices are not forced

AUTO, ROWS = 0, 1       # PGENHIP_SCORE_* (include/pgen_hip.h)
ACCUMULATE = 0x10
MAX_COLUMNS = 8


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def plan(n: int, c: int, v: int = 1, forced: int = 0, num_cus: int = 256):
    """(lane_bytes, batch_rows, log_g, tiles, slices, slots) of a launch over V rows of N samples with C columns."""
    return L.call("score_plan", 6, record_size(n), v, c, num_cus, forced)


def lane_bytes(c: int) -> int:
    return plan(1, c)[0]


def batch_rows(c: int) -> int:
    return plan(1, c)[1]


def lanes_per_row(n: int, c: int) -> int:
    return 1 << plan(n, c)[2]


def tiles(n: int, c: int) -> int:
    return plan(n, c)[3]


def slots(n: int, c: int) -> int:
    """Rows a block has side by side (4 waves x 64 / G groups)."""
    return plan(n, c)[5]


def step_rows(n: int, c: int) -> int:
    """Rows of one batch of every slot of a block: a launch has at most ceil(V / step_rows) slices."""
    return slots(n, c) * batch_rows(c)


def slices(n: int, c: int, v: int, forced: int = 0, num_cus: int = 256) -> int:
    return plan(n, c, v, forced, num_cus)[4]


def edge_rows(n: int, c: int, forced: int) -> list[int]:
    """Row counts on both sides of every edge: one slot row, one batch, the cap of the forced slices, a second batch per slice."""
    s, st = slots(n, c), step_rows(n, c)
    vs = {1, s - 1, s, s + 1, st - 1, st, st + 1, forced * st - 1, forced * st, forced * st + 1, 2 * forced * st + forced + 1}
    return sorted(v for v in vs if v >= 1)
