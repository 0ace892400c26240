"""CPU guard of tests/count_plan.py: what it restates must still read the same in csrc/gt_count.hip (and the flag values in the
header).  A changed constant, ladder or instantiation fails here instead of silently moving a class edge or a grid-stride
boundary away from the cells of test_genotype_counts_gpu.py / test_genotype_counts_stride_gpu.py that test it."""
import re
from pathlib import Path

import count_plan as CP

REPO = Path(__file__).resolve().parent.parent
SRC = (REPO / "pgen_rs_amd" / "csrc" / "gt_count.hip").read_text()


def _const(name):
    m = re.findall(rf"constexpr\s+(?:uint32_t|int)\s+{name}\s*=\s*(\d+)u?\s*;", SRC)
    assert len(m) == 1, f"{name}: {m}"
    return int(m[0])


def _body(signature):
    b = SRC[SRC.index(signature):]
    return b[: b.index("\n}\n")]


def test_mirrored_constants_match_the_source():
    assert _const("kThreads") == CP.THREADS
    assert _const("kBlocksPerCu") == CP.BLOCKS_PER_CU
    hdr = (REPO / "include" / "pgen_hip.h").read_text()
    for name, v in (("AUTO", CP.AUTO), ("WAVE_PER_ROW", CP.WAVE_PER_ROW), ("ROWS_PER_WAVE", CP.ROWS_PER_WAVE)):
        assert re.search(rf"#define PGENHIP_COUNT_{name} {v}u\b", hdr), name


def test_lanes_per_row_ladder_matches_the_source():
    body = _body("uint32_t gt_count_lanes_per_row(uint32_t record_size)")
    assert "const uint32_t chunks = (record_size + 30u) / 16u;" in body
    ladder = " : ".join(f"chunks <= {b}u ? {g}u" for b, g in CP.LADDER) + " : 64u;"
    assert ladder in body, body
    # the kernel's pass count uses the same chunk bound
    assert "((R + 30u) / 16u + (uint32_t)(G * U) - 1u) / (uint32_t)(G * U)" in SRC


def test_instantiations_match_the_source():
    body = _body("hipError_t launch_gt_count(")
    assert "if (wave_per_row) return launch_shape<%d, %d, %d>(a, num_cus, stream);" % CP.SHAPES[64] in body
    for g in (4, 8, 16):
        assert "case %du: return launch_shape<%d, %d, %d>(a, num_cus, stream);" % ((g,) + CP.SHAPES[g]) in body
    assert "default: return launch_shape<%d, %d, %d>(a, num_cus, stream);" % CP.SHAPES[32] in body
    # AUTO takes a wave per row exactly where the ladder says 64 lanes
    capi = (REPO / "pgen_rs_amd" / "csrc" / "capi.hip").read_text()
    assert ("flags == PGENHIP_COUNT_WAVE_PER_ROW || (flags == PGENHIP_COUNT_AUTO && gt_count_lanes_per_row(ctx->record_size) == 64u)"
            in capi)


def test_launch_shape_matches_the_source():
    body = _body("hipError_t launch_shape(")
    assert "const uint64_t rows_per_block = (uint64_t)(kThreads / 64) * (64u / G) * RU;" in body
    assert "const uint64_t blocks = (a.n_variants + rows_per_block - 1) / rows_per_block;" in body
    assert "const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * kBlocksPerCu;" in body
    assert "const uint32_t grid = (uint32_t)(blocks < cap ? blocks : cap);" in body
    kern = _body("__global__ __launch_bounds__(kThreads) void gt_count_kernel(")
    assert "constexpr uint32_t kRowsPerStep = kGroups * RU;" in kern and "constexpr uint32_t kGroups = 64u / G;" in kern
    assert "r0 = wave * kRowsPerStep; r0 < a.n_variants; r0 += n_waves * kRowsPerStep" in kern


def test_derived_edges():
    """The edges the GPU cells sit on, as derived today (a change here means re-reading the launch code)."""
    assert CP.CLASS_EDGES == [708, 1476, 3012, 6084]
    assert [CP.lanes_per_row(CP.record_size(n)) for n in (708, 709, 1476, 1477, 3012, 3013, 6084, 6085)] == [4, 8, 8, 16, 16, 32, 32, 64]
    assert CP.shape(6085) == (64, 1, 4) and CP.shape(6085, CP.ROWS_PER_WAVE) == (32, 2, 1) and CP.shape(708, CP.WAVE_PER_ROW) == (64, 1, 4)
    assert CP.shape(708) == (4, 2, 1) and CP.shape(6084) == (32, 2, 1) and CP.shape(500_000, CP.ROWS_PER_WAVE) == (32, 2, 1)
    # on 256 CUs one grid covers 8 192 rows with a wave per row, 32 768 / 65 536 / 131 072 / 262 144 at G = 32 / 16 / 8 / 4
    assert [CP.rows_per_grid(*CP.SHAPES[g][:2], 256) for g in (64, 32, 16, 8, 4)] == [8192, 32768, 65536, 131072, 262144]
    assert CP.grid(8193, 64, 1, 256) == 2048 and CP.grid(8192, 64, 1, 256) == 2048 and CP.grid(8188, 64, 1, 256) == 2047
    assert CP.passes(CP.record_size(6085), 32, 1) == 4 and CP.passes(CP.record_size(6084), 32, 1) == 3
