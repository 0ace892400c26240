"""CPU pins of tests/count_plan.py, which runs csrc/launch_plan.h: the edges that the cells of test_genotype_counts_gpu.py /
test_genotype_counts_stride_gpu.py sit on, as numbers, so that a changed constant, ladder or instantiation fails here instead of
silently moving a class edge or a grid-stride boundary away from them.  The flag values are checked against the header, and the
one thing of the kernel that only its text shows (its row loop strides by the plan's step) against gt_count.hip."""
import re
from pathlib import Path

import count_plan as CP

REPO = Path(__file__).resolve().parent.parent


def test_derived_edges():
    """The edges the GPU cells sit on, as derived today (a change here means re-reading the launch code)."""
    assert (CP.THREADS, CP.BLOCKS_PER_CU) == (256, 8)
    assert CP.CLASS_EDGES == [708, 1476, 3012, 6084]
    assert [CP.lanes_per_row(CP.record_size(n)) for n in (708, 709, 1476, 1477, 3012, 3013, 6084, 6085)] == [4, 8, 8, 16, 16, 32, 32, 64]
    assert CP.shape(6085) == (64, 1, 4) and CP.shape(6085, CP.ROWS_PER_WAVE) == (32, 2, 1) and CP.shape(708, CP.WAVE_PER_ROW) == (64, 1, 4)
    assert CP.shape(708) == (4, 2, 1) and CP.shape(6084) == (32, 2, 1) and CP.shape(500_000, CP.ROWS_PER_WAVE) == (32, 2, 1)
    # on 256 CUs one grid covers 8 192 rows with a wave per row, 32 768 / 65 536 / 131 072 / 262 144 at G = 32 / 16 / 8 / 4
    assert [CP.rows_per_grid(*CP.SHAPES[g][:2], 256) for g in (64, 32, 16, 8, 4)] == [8192, 32768, 65536, 131072, 262144]
    assert CP.grid(8193, 64, 1, 256) == 2048 and CP.grid(8192, 64, 1, 256) == 2048 and CP.grid(8188, 64, 1, 256) == 2047
    assert CP.passes(CP.record_size(6085), 32, 1) == 4 and CP.passes(CP.record_size(6084), 32, 1) == 3
    hdr = (REPO / "include" / "pgen_hip.h").read_text()
    for name, v in (("AUTO", CP.AUTO), ("WAVE_PER_ROW", CP.WAVE_PER_ROW), ("ROWS_PER_WAVE", CP.ROWS_PER_WAVE)):
        assert re.search(rf"#define PGENHIP_COUNT_{name} {v}u\b", hdr), name
    # device code: a wave's row loop strides by the step the plan states
    kern = (REPO / "pgen_rs_amd" / "csrc" / "gt_count.hip").read_text()
    assert "constexpr uint32_t kRowsPerStep = rows_per_step(G, RU);" in kern
    assert "r0 = wave * kRowsPerStep; r0 < a.n_variants; r0 += n_waves * kRowsPerStep" in kern
