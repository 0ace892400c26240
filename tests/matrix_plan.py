"""The launch plan of the genotype-matrix kernels, restated from csrc/gt_matrix.hip and the dispatch in csrc/capi.hip so that the
tests can place their cells on both sides of every edge: the 16-byte chunk of the STREAM shape (16 / 8 / 4 elements), its dense and
per-row forms, the 128-variant x 512-sample block tile and 128-sample wave tile of the TILE shape, the grids one launch covers and
the shape AUTO takes.

Mirrors (keep in step; test_decode_matrix.py checks them against the source):
  * ``kThreads``, ``kBlocksPerCu``, ``kTileVariants``, ``kWaveSamples``, ``kTileSamples``, ``kTileBlocksPerCu``;
  * ``launch_gt_matrix_stream``: ``dense``, ``per_row``, ``total``, ``kLongRowBytes`` and the rows kernel's grid;
  * ``launch_gt_matrix_tile``: ``v_tiles``, ``bands``;
  * ``gt_matrix_stream_applicable`` / ``gt_matrix_tile_applicable`` and the order AUTO asks them in.
"""
from __future__ import annotations

THREADS = 256
BLOCKS_PER_CU = 8
TILE_VARIANTS = 128
WAVE_SAMPLES = 128
TILE_SAMPLES = 512
TILE_BLOCKS_PER_CU = 4
CHUNK = 16
LONG_ROW_BYTES = 4096    # kLongRowBytes: STREAM rows from this many output bytes take the rows kernel

AUTO, GENERAL, STREAM, TILE = 0, 1, 2, 3     # PGENHIP_MATRIX_* (include/pgen_hip.h)
SHAPE_MASK = 0xF
SAMPLE_MAJOR = 0x10
KNOB_MATRIX_BLOCKS = 18


def record_size(n: int) -> int:
    return (2 * n + 7) // 8


def auto_shape(all_kept: bool, sample_major: bool, out_addr: int, out_stride: int, k: int) -> int:
    """What PGENHIP_MATRIX_AUTO launches."""
    if all_kept and not sample_major:
        return STREAM
    if all_kept and sample_major and out_addr % 16 == 0 and (out_stride % 16 == 0 or k <= 1):
        return TILE
    return GENERAL


def stream_dense(v: int, k: int, elem: int, out_stride: int) -> bool:
    return v == 1 or out_stride == k * elem


def stream_chunks(v: int, k: int, elem: int, out_addr: int, out_stride: int) -> int:
    """Work items (one lane each) of a STREAM launch."""
    row_bytes = k * elem
    if stream_dense(v, k, elem, out_stride):
        return (out_addr % 16 + row_bytes * v + 15) // 16
    return ((row_bytes + 15) // 16 + 1) * v


def stream_long_rows(k: int, elem: int) -> bool:
    return k * elem >= LONG_ROW_BYTES


def stream_rows_grid(v: int, k: int, elem: int, cus: int = 256, forced: int = 0) -> tuple[int, int]:
    """(blocks along a row's chunks, blocks along the rows) of the long-row STREAM kernel."""
    per_row = (k * elem + 15) // 16 + 1
    gx = grid((per_row + THREADS - 1) // THREADS, BLOCKS_PER_CU, cus, 1 if forced > 0 else 0)
    cap = forced if forced > 0 else cus * BLOCKS_PER_CU
    return gx, min(v, max(1, cap // gx), 65535)


def grid(work_blocks: int, per_cu: int, cus: int = 256, forced: int = 0) -> int:
    cap = forced if forced > 0 else cus * per_cu
    return max(1, min(work_blocks, cap))


def stream_grid(v, k, elem, out_addr, out_stride, cus=256, forced=0) -> int:
    return grid((stream_chunks(v, k, elem, out_addr, out_stride) + THREADS - 1) // THREADS, BLOCKS_PER_CU, cus, forced)


def general_grid(v, k, cus=256, forced=0) -> int:
    return grid((v * k + THREADS - 1) // THREADS, BLOCKS_PER_CU, cus, forced)


def tile_counts(v: int, n: int) -> tuple[int, int]:
    """(variant tiles, sample bands); a launch walks bands x variant tiles, variant tile fastest."""
    return (v + TILE_VARIANTS - 1) // TILE_VARIANTS, (n + TILE_SAMPLES - 1) // TILE_SAMPLES


def tile_grid(v, n, cus=256, forced=0) -> int:
    vt, bands = tile_counts(v, n)
    return grid(vt * bands, TILE_BLOCKS_PER_CU, cus, forced)


# sample counts at the edges of the plan: the 16-sample lane piece and the 128-sample wave piece of TILE, its 512-sample band
# (one, two bands), the STREAM chunk sizes (4, 8, 16 elements) and its long-row threshold at 4-, 2- and 1-byte elements
N_EDGES = [4, 8, 16, WAVE_SAMPLES, TILE_SAMPLES, 2 * TILE_SAMPLES, LONG_ROW_BYTES // 2, LONG_ROW_BYTES]
# variant counts at the edges: a lane's 16 variants, the tile, two tiles
V_EDGES = [16, TILE_VARIANTS, 2 * TILE_VARIANTS]
