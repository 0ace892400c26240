"""The planning arithmetic of the full-line kernels, RUN from csrc/launch_plan.h (namespace plan::emit, through the probe that
tests/subset_plan.py loads) so that the prefix-edge tests can place their cells on both sides of every limit a kernel derives from
``max_prefix_bytes`` (P below: the longest prefix, or the stated bound).

What the header decides and this module only asks for:
  * line-run kernel: ``lineruns_rows``, ``lineruns`` and ``lineruns_seam_shift``
  * pick family, full lines: ``pick_plan``, ``pick_lines_rows`` and ``pick_cps_shift``
  * prefix copy of the stream / segment / row-owner / pick row-by-row kernels: ``prefix_copy_shift``
  * row-owner kernel: ``rowpick_lds_bytes``, ``kRowPickMaxKept``
The edges below are found by running those functions over P, not by restating them.
"""
from __future__ import annotations

from subset_plan import (LR_MAX_ROWS, LR_PFX_BYTES, PICK_MAX_PACKED_ROWS, PICK_MAX_SAMPLES, PICK_PFX_BYTES, PICK_STAGE_BYTES,  # noqa: F401
                         ROWPICK_MAX_KEPT, SEG_SAMPLES, _call, record_size, rowpick_lds_bytes, shape)
from subset_plan import RUN_LOAD_BYTES as LR_LOAD_BYTES  # noqa: F401  one wide load of a run's records (+ 1 byte): 1040 // R rows
from subset_plan import RUN_SPAN_BYTES as SPAN_BYTES     # noqa: F401  a run's chunks (+ lead) fit one 1 024-chunk span

PICK_BATCH_BYTES = 32768    # default text bytes per batch (PGENHIP_KNOB_PICK_BATCH_BYTES)


def _signed(x: int) -> int:
    return x - (1 << 64) if x >= 1 << 63 else x


def lineruns_rows(n: int, k: int, subset: bool, p: int) -> int:
    """Lines per work item of the line-run kernel (0/1: it refuses the shape)."""
    return _call("emit_applicable", 11, *shape(n, k, kept_list=subset, lines=True, bound=p), 256)[10]


def lineruns_accepts(n: int, k: int, subset: bool, p: int) -> bool:
    """plan::emit::lineruns for dense records without a gather."""
    return bool(_call("emit_applicable", 11, *shape(n, k, kept_list=subset, lines=True, bound=p), 256)[5])


def lineruns_seam_shift(p: int) -> int:
    """log2 of the lanes per seam in phase B of the line-run kernel (by P + 1: the prefix and the '\\n' in front of it)."""
    return _call("emit_lineruns_seam_shift", 1, p + 1)[0]


def pick_batch_rows(n: int, k: int) -> int:
    """Rows per batch of the pick family on dense records (before the full-line plan)."""
    return _call("emit_pick_plan", 6, *shape(n, k, kept_list=k != n, lines=True), PICK_BATCH_BYTES)[2]


def pick_lines_rows(n: int, k: int, p: int) -> int:
    """Batch rows of gt_pick_lines_kernel (interiors + seams) on dense records; < 2 (or P > 993): the row-by-row kernel instead."""
    return _signed(_call("emit_pick_lines_rows", 1, record_size(n), p, pick_batch_rows(n, k))[0])


def pick_cps_shift(p: int) -> int:
    """log2 of the chunk slots (lanes) per seam of gt_pick_lines_kernel: a seam is at most P + 31 bytes."""
    return _call("emit_pick_cps_shift", 1, p)[0]


def prefix_copy_shift(p: int) -> int:
    return _call("emit_prefix_copy_shift", 1, p)[0]


# ---- the edges, found by running the functions above (each is the LAST P before the planned value changes) --------------------
def _last_before_change(f, lo: int, hi: int):
    out = []
    prev = f(lo)
    for p in range(lo + 1, hi + 1):
        v = f(p)
        if v != prev:
            out.append(p - 1)
            prev = v
    return out


LR_SEAM_EDGES = _last_before_change(lineruns_seam_shift, 0, 400)                      # [15, 31, 63, 127]
# rows of 8 samples: only the prefix area bounds a run
LR_ROWS_7_6 = max(p for p in range(1, 800) if lineruns_rows(8, 8, False, p) >= 7)      # 94: B = 7 -> 6 at 95
LR_ROWS_2_1 = max(p for p in range(1, 800) if lineruns_rows(8, 8, False, p) >= 2)      # 250: B = 2 -> 1 at 251
# rows of 1 900 samples (two records per load): only the span bounds a run — 4K + 1 + P for two lines per span
LR_LINE_LIMIT = 4 * 1900 + 1 + max(p for p in range(0, 200) if lineruns_rows(1900, 1900, False, p) >= 2)   # 7664
PICK_SEAM_EDGES = _last_before_change(pick_cps_shift, 0, 1200)                          # [48, 112, 240, 496]
# records of 16 bytes: only the prefix stage bounds a batch
PICK_ROWS_FALLBACK = max(p for p in range(1, 2048) if pick_lines_rows(61, 61, p) >= 2)   # 677: row by row from 678
COPY_SHIFT_EDGE = _last_before_change(prefix_copy_shift, 0, 200)[0]                      # 48


def pick_cross_edge(n: int, k: int) -> int:
    """The last P at which the records, not the prefix stage, bound pick-lines' batch rows (N = 4 096, 10 % kept: 290)."""
    base = pick_lines_rows(n, k, 0)
    return max(p for p in range(1, 2048) if pick_lines_rows(n, k, p) == base)
