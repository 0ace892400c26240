"""The launch plan of the matrix-core shape of the per-variant sums kernel, restated from csrc/gt_vsum.hip so that the tests can
place their row and sample counts on both sides of every edge it has: the record bytes of a tile (one tile: every sum has one
owner and is stored; more: tiles meet in FP64 atomics), the rows of one MFMA, the groups the waves of a block take in turn, and the
row ranges (slices) a tile is cut into, which the grid-size knob forces.

Mirrors (keep in step; test_variant_sums.py checks them against the source):
  * ``kTileBytes``, ``kGroupRows``, ``kMinSliceRows``;
  * ``plan``: tiles, the cap of the slices at one group per wave, the grid;
  * the groups of a slice, ``gbeg = groups * slice / slices``.
"""
from __future__ import annotations

THREADS = 256
WAVES = THREADS // 64
TILE_BYTES = 32         # kTileBytes
TILE_SAMPLES = 4 * TILE_BYTES
GROUP_ROWS = 4          # kGroupRows
MIN_SLICE_ROWS = 256    # kMinSliceRows (only when the grid is not forced)

AUTO, GENERAL, MFMA = 0, 1, 2   # PGENHIP_VSUM_* (include/pgen_hip.h)
MAX_COLUMNS = 16


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def tiles(n: int) -> int:
    return (record_size(n) + TILE_BYTES - 1) // TILE_BYTES


def groups(v: int) -> int:
    return (v + GROUP_ROWS - 1) // GROUP_ROWS


def slices(v: int, forced: int) -> int:
    """Row ranges per tile with the grid forced to ``forced`` blocks: at most one per WAVES groups."""
    return max(1, min(forced, (groups(v) + WAVES - 1) // WAVES))


def grid(n: int, v: int, forced: int) -> int:
    return min(tiles(n) * slices(v, forced), forced)


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
