"""The launch plan of the genotype-matrix kernels, RUN from csrc/launch_plan.h (namespace plan::matrix, which csrc/gt_matrix.hip and
the dispatch in csrc/capi.hip call) through tests/launch_plan.py rather than restated, so that the tests can place their cells on
both sides of every edge: the 16-byte chunk of the STREAM shape (16 / 8 / 4 elements), its dense and per-row forms, the 128-variant x
512-sample block tile and 128-sample wave tile of the TILE shape, the grids one launch covers and the shape AUTO takes.  Only
``N_EDGES`` and ``V_EDGES``, which lay out test sizes, are Python, on top of probed values.
"""
from __future__ import annotations

import launch_plan as L

THREADS = L.CONST["matrix.kThreads"]
BLOCKS_PER_CU = L.CONST["matrix.kBlocksPerCu"]
TILE_VARIANTS = L.CONST["matrix.kTileVariants"]
WAVE_SAMPLES = L.CONST["matrix.kWaveSamples"]
TILE_SAMPLES = L.CONST["matrix.kTileSamples"]
TILE_BLOCKS_PER_CU = L.CONST["matrix.kTileBlocksPerCu"]
CHUNK = 16
LONG_ROW_BYTES = L.CONST["matrix.kLongRowBytes"]    # STREAM rows from this many output bytes take the rows kernel

AUTO = 0                                            # PGENHIP_MATRIX_* (include/pgen_hip.h)
GENERAL, STREAM, TILE = L.CONST["matrix.kGeneral"], L.CONST["matrix.kStream"], L.CONST["matrix.kTile"]
SHAPE_MASK = 0xF
SAMPLE_MAJOR = 0x10
KNOB_MATRIX_BLOCKS = 18


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def auto_shape(all_kept: bool, sample_major: bool, out_addr: int, out_stride: int, k: int) -> int:
    """What PGENHIP_MATRIX_AUTO launches."""
    return L.call("matrix_auto_shape", 3, all_kept, sample_major, out_addr % 16, out_stride, k)[0]


def stream_plan(v, k, elem, out_addr, out_stride, cus=256, forced=0):
    """(dense, long_rows, per_row, total, grid_x, grid_y) of a STREAM launch."""
    return L.call("matrix_stream_plan", 6, v, k, elem, out_addr % 16, out_stride, cus, forced)


def stream_dense(v: int, k: int, elem: int, out_stride: int) -> bool:
    return bool(stream_plan(v, k, elem, 0, out_stride)[0])


def stream_chunks(v: int, k: int, elem: int, out_addr: int, out_stride: int) -> int:
    """Work items (one lane each) of a STREAM launch."""
    return stream_plan(v, k, elem, out_addr, out_stride)[3]


def stream_long_rows(k: int, elem: int) -> bool:
    return bool(stream_plan(1, k, elem, 0, k * elem)[1])


def stream_rows_grid(v: int, k: int, elem: int, cus: int = 256, forced: int = 0) -> tuple[int, int]:
    """(blocks along a row's chunks, blocks along the rows) of the long-row STREAM kernel."""
    assert stream_long_rows(k, elem)
    return stream_plan(v, k, elem, 0, k * elem, cus, forced)[4:]


def stream_grid(v, k, elem, out_addr, out_stride, cus=256, forced=0) -> int:
    """Blocks of the short-row STREAM kernel over the launch's chunks (rows below LONG_ROW_BYTES launch exactly this)."""
    return L.grid_blocks((stream_chunks(v, k, elem, out_addr, out_stride) + THREADS - 1) // THREADS, BLOCKS_PER_CU, cus, forced)


def general_grid(v, k, cus=256, forced=0) -> int:
    return L.call("matrix_general_grid", 1, v, k, cus, forced)[0]


def tile_counts(v: int, n: int) -> tuple[int, int]:
    """(variant tiles, sample bands); a launch walks bands x variant tiles, variant tile fastest."""
    return L.call("matrix_tile_plan", 4, v, n, 256, 0)[:2]


def tile_grid(v, n, cus=256, forced=0) -> int:
    return L.call("matrix_tile_plan", 4, v, n, cus, forced)[3]


# sample counts at the edges of the plan: the 16-sample lane piece and the 128-sample wave piece of TILE, its 512-sample band
# (one, two bands), the STREAM chunk sizes (4, 8, 16 elements) and its long-row threshold at 4-, 2- and 1-byte elements
N_EDGES = [4, 8, 16, WAVE_SAMPLES, TILE_SAMPLES, 2 * TILE_SAMPLES, LONG_ROW_BYTES // 2, LONG_ROW_BYTES]
# variant counts at the edges: a lane's 16 variants, the tile, two tiles
V_EDGES = [16, TILE_VARIANTS, 2 * TILE_VARIANTS]
