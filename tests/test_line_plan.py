"""CPU guard of tests/line_plan.py: the constants it restates must still read the same in csrc/.  A changed constant fails here and
points at the edge table of test_emit_lines_prefixes_gpu.py, instead of silently moving an edge away from the cells that test it."""
import re
from pathlib import Path

import line_plan as LP

CSRC = Path(__file__).resolve().parent.parent / "pgen_rs_amd" / "csrc"


def _const(file, name):
    m = re.findall(rf"constexpr\s+(?:uint32_t|int|size_t)\s+{name}\s*=\s*(\d+)u?\s*;", (CSRC / file).read_text())
    assert len(m) == 1, f"{name} in {file}: {m}"
    return int(m[0])


def test_mirrored_constants_match_the_sources():
    assert _const("gt_wide.hip", "kLrPfxBytes") == LP.LR_PFX_BYTES
    assert _const("gt_wide.hip", "kLrMaxRows") == LP.LR_MAX_ROWS
    assert _const("gt_pick.hip", "kPfxBytes") == LP.PICK_PFX_BYTES
    assert _const("gt_pick.hip", "kStageBytes") == LP.PICK_STAGE_BYTES
    assert _const("gt_pick.hip", "kMaxPackedRows") == LP.PICK_MAX_PACKED_ROWS
    assert _const("gt_pick.hip", "kMaxSamples") == LP.PICK_MAX_SAMPLES
    assert _const("kernels.h", "kRowPickMaxKept") == LP.ROWPICK_MAX_KEPT


def test_mirrored_plan_expressions_match_the_sources():
    """The literals of the plans (the span limit, the record load, the seam-lane ladders, the pick-lines clamps) as the sources spell them."""
    wide = (CSRC / "gt_wide.hip").read_text()
    body = wide[wide.index("static uint32_t lineruns_rows_for"):]
    body = body[: body.index("\n}\n")]
    assert f"a.max_line_bytes > {LP.SPAN_BYTES}ull" in body and f"{LP.SPAN_BYTES}u / (uint32_t)a.max_line_bytes" in body
    assert f"{LP.LR_LOAD_BYTES}u / a.record_size" in body
    assert "(kLrPfxBytes - 16u) / max_prefix - (((kLrPfxBytes - 16u) / max_prefix) ? 1u : 0u)" in body
    assert ("seam_bytes <= 16u ? 2u : (seam_bytes <= 32u ? 3u : (seam_bytes <= 64u ? 4u : (seam_bytes <= 128u ? 5u : 6u)))" in wide)
    pick = (CSRC / "gt_pick.hip").read_text()
    assert "bl = (uint32_t)((kPfxBytes - 16u) / max_prefix) - 1u" in pick
    assert "(max_prefix + 31ull) / 16ull" in pick
    assert "seam_chunks <= 4u ? 2u : (seam_chunks <= 8u ? 3u : (seam_chunks <= 16u ? 4u : (seam_chunks <= 32u ? 5u : 6u)))" in pick
    assert "max_prefix <= 993ull && (int32_t)bl >= 2 && bl <= 62u" in pick
    common = (CSRC / "gt_common.hip.h").read_text()
    assert "<= 48ull ? 3u : 4u" in common


def test_derived_edges():
    """The edges the GPU matrix places its cells around, as derived today (a change here means re-reading the planning code)."""
    assert LP.LR_SEAM_EDGES == [15, 31, 63, 127]
    assert (LP.LR_ROWS_7_6, LP.LR_ROWS_2_1, LP.LR_LINE_LIMIT) == (94, 250, 7664)
    assert LP.PICK_SEAM_EDGES == [48, 112, 240, 496]
    assert LP.PICK_ROWS_FALLBACK == 677 and LP.COPY_SHIFT_EDGE == 48
    assert LP.pick_lines_rows(4096, 409, 0) == 6 and LP.pick_cross_edge(4096, 409) == 290
    assert LP.rowpick_lds_bytes(20_000, 16_384) == 65_632 and LP.rowpick_lds_bytes(65_536, 16_384) == 65_648
    assert [LP.lineruns_rows(1900, 1900, False, p) for p in (63, 64)] == [2, 1]
