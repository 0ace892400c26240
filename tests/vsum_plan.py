"""The launch plan of the matrix-core shape of the per-variant sums kernel, RUN from csrc/launch_plan.h (namespace plan::vsum) through
tests/launch_plan.py rather than restated, so that the tests can place their row and sample counts on both sides of every edge it
has: the record bytes of a tile (one tile: every sum has one owner and is stored; more: tiles meet in FP64 atomics), the rows of one
MFMA, the groups the waves of a block take in turn, and the row ranges (slices) a tile is cut into, which the grid-size knob forces.
Only ``edge_rows`` and ``edge_samples``, which lay out test sizes, are Python, on top of probed values.
"""
from __future__ import annotations

import launch_plan as L

THREADS = L.CONST["vsum.kThreads"]
WAVES = L.CONST["vsum.kWaves"]
TILE_BYTES = L.CONST["vsum.kTileBytes"]
TILE_SAMPLES = 4 * TILE_BYTES
GROUP_ROWS = L.CONST["vsum.kGroupRows"]
MIN_SLICE_ROWS = L.CONST["vsum.kMinSliceRows"]    # only when the grid is not forced

AUTO, GENERAL, MFMA = 0, 1, 2   # PGENHIP_VSUM_* (include/pgen_hip.h)
MAX_COLUMNS = 16


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def plan(n: int, v: int = 1, forced: int = 0, num_cus: int = 256):
    """(tiles, slices, grid, atomic, groups) of an MFMA launch over V rows of N samples."""
    return L.call("vsum_mfma_plan", 5, record_size(n), v, num_cus, forced)


def tiles(n: int) -> int:
    return plan(n)[0]


def groups(v: int) -> int:
    return plan(1, v)[4]


def slices(v: int, forced: int = 0, n: int = 1, num_cus: int = 256) -> int:
    """Row ranges per tile (``forced``: the grid forced to that many blocks; at most one slice per WAVES groups)."""
    return plan(n, v, forced, num_cus)[1]


def grid(n: int, v: int, forced: int = 0, num_cus: int = 256) -> int:
    return plan(n, v, forced, num_cus)[2]


def edge_rows(forced: int) -> list[int]:
    """Row counts on both sides of every edge: one group, one group per wave, the cap of the forced slices, a second round of
    groups per slice."""
    g, w = GROUP_ROWS, GROUP_ROWS * WAVES
    vs = {1, g - 1, g, g + 1, w - 1, w, w + 1, forced * w - 1, forced * w, forced * w + 1, 2 * forced * w + forced + 1}
    return sorted(v for v in vs if v >= 1)


def edge_samples() -> list[int]:
    """Sample counts on both sides of the tile edges: one tile exactly, a second tile of one byte (moved back over the first), a last
    tile one byte short of whole, three tiles."""
    t = TILE_SAMPLES
    return [t - 1, t, t + 1, t + 4, t + 5, 2 * t - 4, 2 * t - 3, 2 * t, 2 * t + 1, 3 * t + 2]
