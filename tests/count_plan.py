"""The launch plan of the genotype-count kernel, restated from csrc/gt_count.hip so that the count tests can place their cells
on both sides of every shape class and of every grid-stride boundary (the rows one grid covers, past which
``gt_count_kernel`` runs its ``r0 += n_waves * kRowsPerStep`` loop again).

Mirrors (keep in step; test_count_plan.py checks them against the source):
  * ``kThreads``, ``kBlocksPerCu``;
  * the chunk bound ``(R + 30) / 16`` and the lanes-per-row ladder of ``gt_count_lanes_per_row``;
  * the ``<G, RU, U>`` instantiations ``launch_gt_count`` picks, forced kernels included;
  * ``rows_per_block`` and the grid cap of ``launch_shape``.
"""
from __future__ import annotations

THREADS = 256          # kThreads
BLOCKS_PER_CU = 8      # kBlocksPerCu
WAVE = 64

AUTO, WAVE_PER_ROW, ROWS_PER_WAVE = 0, 1, 2   # PGENHIP_COUNT_* (include/pgen_hip.h)

# lanes per row -> (G, RU, U) of launch_gt_count's switch; 64 is the wave-per-row instantiation
SHAPES = {4: (4, 2, 1), 8: (8, 2, 1), 16: (16, 2, 1), 32: (32, 2, 1), 64: (64, 1, 4)}
LADDER = [(12, 4), (24, 8), (48, 16), (96, 32)]   # chunks <= bound -> lanes per row; above the last: 64


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def max_chunks(r: int) -> int:
    """The most aligned 16-byte chunks a row of R bytes can touch."""
    return (r + 30) // 16


def lanes_per_row(r: int) -> int:
    c = max_chunks(r)
    for bound, g in LADDER:
        if c <= bound:
            return g
    return 64


def shape(n: int, kernel: int = AUTO):
    """(G, RU, U) that launch_gt_count runs for N samples under ``kernel``."""
    g = lanes_per_row(record_size(n))
    if kernel == WAVE_PER_ROW or (kernel == AUTO and g == 64):
        return SHAPES[64]
    return SHAPES[min(g, 32)]   # forced ROWS_PER_WAVE on long rows: G = 32, more passes per row


def rows_per_step(g: int, ru: int) -> int:
    """Rows one wave takes per iteration of the row loop (kRowsPerStep)."""
    return (WAVE // g) * ru


def rows_per_block(g: int, ru: int) -> int:
    return (THREADS // WAVE) * rows_per_step(g, ru)


def grid(n_variants: int, g: int, ru: int, num_cus: int) -> int:
    blocks = -(-n_variants // rows_per_block(g, ru))
    return min(blocks, (num_cus if num_cus > 0 else 256) * BLOCKS_PER_CU)


def rows_per_grid(g: int, ru: int, num_cus: int) -> int:
    """Rows one full grid covers (S): rows past S are reached only through the grid-stride loop."""
    return (num_cus if num_cus > 0 else 256) * BLOCKS_PER_CU * rows_per_block(g, ru)


def passes(r: int, g: int, u: int) -> int:
    return (max_chunks(r) + g * u - 1) // (g * u)


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
