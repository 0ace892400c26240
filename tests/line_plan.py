"""The planning arithmetic of the full-line kernels, restated from csrc/ so that the prefix-edge tests can place their cells on
both sides of every limit a kernel derives from ``max_prefix_bytes`` (P below: the longest prefix, or the stated bound).

Mirrors (keep in step; test_line_plan.py checks the constants against the sources):
  * line-run kernel: ``lineruns_rows_for`` (gt_wide.hip, "runs of full LINES") and ``seam_shift`` in ``emit_lines_run``
  * pick family, full lines: the ``gt_pick_lines_kernel`` plan at the end of ``launch_gt_pick`` (gt_pick.hip)
  * prefix copy of the stream / segment / row-owner / pick row-by-row kernels: ``prefix_copy_shift`` (gt_common.hip.h)
  * row-owner kernel: ``table_bytes`` / ``rank_bytes`` / ``codes_bytes`` and ``plan`` (gt_rowpick.hip), ``kRowPickMaxKept`` (kernels.h)
  * AUTO's choice between them: ``choose_all_samples`` and ``choose_subset`` (capi.hip)
"""
from __future__ import annotations

from subset_plan import ROWPICK_MAX_KEPT, SEG_SAMPLES, record_size, rowpick_lds_bytes  # noqa: F401  (kernels.h, gt_rowpick.hip)

# gt_wide.hip
LR_PFX_BYTES = 768          # kLrPfxBytes: LDS area of the prefixes of B + 1 lines
LR_MAX_ROWS = 30            # kLrMaxRows
LR_LOAD_BYTES = 1040        # one wide load of a run's records (+ 1 byte): 1040 // R rows
SPAN_BYTES = 15328          # a run's chunks (+ lead) fit one 1 024-chunk span
# gt_pick.hip
PICK_PFX_BYTES = 2048       # kPfxBytes: prefix stage of a pick-lines batch (+ the row behind it)
PICK_STAGE_BYTES = 8192     # kStageBytes: record stage of a batch
PICK_MAX_PACKED_ROWS = 64   # kMaxPackedRows
PICK_MAX_SAMPLES = 4096     # kMaxSamples
PICK_BATCH_BYTES = 32768    # default text bytes per batch (PGENHIP_KNOB_PICK_BATCH_BYTES)


def lineruns_rows(n: int, k: int, subset: bool, p: int) -> int:
    """Lines per work item of the line-run kernel (0/1: it refuses the shape); gt_wide.hip lineruns_rows_for."""
    r = record_size(n)
    line = p + 4 * k + 1
    if r == 0 or line > SPAN_BYTES:
        return 0
    b = LR_LOAD_BYTES // r
    if subset and b:
        b -= 1                                   # the whole record behind the run comes along
    b = min(b, SPAN_BYTES // line, LR_MAX_ROWS)
    if p:
        q = (LR_PFX_BYTES - 16) // p
        b = min(b, q - (1 if q else 0))          # prefixes of B + 1 lines in kLrPfxBytes - 16
    return b


def lineruns_accepts(n: int, k: int, subset: bool, p: int) -> bool:
    """gt_lineruns_applicable for dense records without a gather."""
    ok = n >= 8 if not subset else (n <= 4096 and k >= 8)
    return ok and lineruns_rows(n, k, subset, p) >= 2


def lineruns_seam_shift(p: int) -> int:
    """log2 of the lanes per seam in phase B of the line-run kernel (by P + 1: the prefix and the '\\n' in front of it)."""
    s = p + 1
    return 2 if s <= 16 else 3 if s <= 32 else 4 if s <= 64 else 5 if s <= 128 else 6


def pick_batch_rows(n: int, k: int) -> int:
    """Rows per batch of the pick family on dense records (before the full-line plan)."""
    r = record_size(n)
    b = max(1, -(-PICK_BATCH_BYTES // (4 * k + 1)))
    return min(b, PICK_MAX_PACKED_ROWS, (PICK_STAGE_BYTES - 16) // r)


def pick_lines_rows(n: int, k: int, p: int) -> int:
    """Batch rows of gt_pick_lines_kernel (interiors + seams) on dense records; < 2 (or P > 993): the row-by-row kernel instead."""
    r = record_size(n)
    bl = min(pick_batch_rows(n, k), 62)
    if 15 + (bl + 1) * r > PICK_STAGE_BYTES:
        bl = (PICK_STAGE_BYTES - 15) // r - 1   # the row behind the batch comes along
    if p and (bl + 1) * p > PICK_PFX_BYTES - 16:
        bl = (PICK_PFX_BYTES - 16) // p - 1     # and its prefix
    return bl


def pick_cps_shift(p: int) -> int:
    """log2 of the chunk slots (lanes) per seam of gt_pick_lines_kernel: a seam is at most P + 31 bytes."""
    c = (p + 31) // 16
    return 2 if c <= 4 else 3 if c <= 8 else 4 if c <= 16 else 5 if c <= 32 else 6


def prefix_copy_shift(p: int) -> int:
    return 3 if p <= 48 else 4


# ---- the edges, derived from the functions above (each is the LAST P before the planned value changes) ------------------------
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
LR_ROWS_7_6 = max(p for p in range(1, 800) if (LR_PFX_BYTES - 16) // p - 1 >= 7)       # 94: B = 7 -> 6 at 95
LR_ROWS_2_1 = max(p for p in range(1, 800) if (LR_PFX_BYTES - 16) // p - 1 >= 2)       # 250: B = 2 -> 1 at 251
LR_LINE_LIMIT = SPAN_BYTES // 2                                                         # 7664: 4K + 1 + P for two lines per span
PICK_SEAM_EDGES = _last_before_change(pick_cps_shift, 0, 1200)                          # [48, 112, 240, 496]
PICK_ROWS_FALLBACK = max(p for p in range(1, 2048) if (PICK_PFX_BYTES - 16) // p - 1 >= 2)   # 677: row by row from 678
COPY_SHIFT_EDGE = _last_before_change(prefix_copy_shift, 0, 200)[0]                      # 48


def pick_cross_edge(n: int, k: int) -> int:
    """The last P at which the records, not the prefix stage, bound pick-lines' batch rows (N = 4 096, 10 % kept: 290)."""
    base = pick_lines_rows(n, k, 0)
    return max(p for p in range(1, 2048) if pick_lines_rows(n, k, p) == base)
