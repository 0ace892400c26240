"""The launch plan of the genotype-count kernel, RUN from csrc/launch_plan.h (namespace plan::count) through tests/launch_plan.py
rather than restated, so that the count tests can place their cells on both sides of every shape class and of every grid-stride
boundary (the rows one grid covers, past which ``gt_count_kernel`` runs its ``r0 += n_waves * kRowsPerStep`` loop again).
Only the helpers that lay out test sizes (``rows_per_grid``, ``CLASS_EDGES``) are Python, on top of probed values.
"""
from __future__ import annotations

import launch_plan as L

THREADS = L.CONST["count.kThreads"]
BLOCKS_PER_CU = L.CONST["count.kBlocksPerCu"]
WAVE = 64

AUTO, WAVE_PER_ROW, ROWS_PER_WAVE = 0, 1, 2   # PGENHIP_COUNT_* (include/pgen_hip.h)


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def max_chunks(r: int) -> int:
    """The most aligned 16-byte chunks a row of R bytes can touch."""
    return L.call("count_lanes_per_row", 2, r)[1]


def lanes_per_row(r: int) -> int:
    return L.call("count_lanes_per_row", 2, r)[0]


def shape(n: int, kernel: int = AUTO):
    """(G, RU, U) that launch_gt_count runs for N samples under ``kernel``."""
    return L.call("count_shape", 4, record_size(n), kernel == WAVE_PER_ROW, kernel == ROWS_PER_WAVE)[1:]


def rows_per_step(g: int, ru: int) -> int:
    """Rows one wave takes per iteration of the row loop (kRowsPerStep)."""
    return L.call("count_grid", 3, 1, g, ru, 0)[0]


def rows_per_block(g: int, ru: int) -> int:
    return L.call("count_grid", 3, 1, g, ru, 0)[1]


def grid(n_variants: int, g: int, ru: int, num_cus: int) -> int:
    return L.call("count_grid", 3, n_variants, g, ru, num_cus)[2]


def rows_per_grid(g: int, ru: int, num_cus: int) -> int:
    """Rows one full grid covers (S): rows past S are reached only through the grid-stride loop."""
    return L.cu_count(num_cus) * BLOCKS_PER_CU * rows_per_block(g, ru)


def passes(r: int, g: int, u: int) -> int:
    return L.call("count_passes", 1, r, g, u)[0]


def _last_n_of_class():
    out = []
    prev = lanes_per_row(record_size(1))
    for n in range(2, 20_000):
        g = lanes_per_row(record_size(n))
        if g != prev:
            out.append(n - 1)
            prev = g
    return out


CLASS_EDGES = _last_n_of_class()   # the last N of the 4 / 8 / 16 / 32 lanes-per-row classes: [708, 1476, 3012, 6084]
# lanes per row -> the (G, RU, U) instantiation of that class under AUTO; 64 is the wave-per-row one
SHAPES = {lanes_per_row(record_size(n)): shape(n) for n in CLASS_EDGES + [CLASS_EDGES[-1] + 1]}
