"""The launch plan of gt_gram.hip, RUN from csrc/launch_plan.h (namespace plan::gram) through tests/launch_plan.py rather than
restated, for the tests that are placed around its constants and its slices."""
import launch_plan as L

TILE = L.CONST["gram.kTile"]                       # ranks of a block tile, per operand
STEP_ROWS = L.CONST["gram.kStepRows"]              # rows expanded into LDS per step
GROUP_ROWS = L.CONST["gram.kGroupRows"]            # rows of one v_mfma_f64_16x16x4_f64
MIN_SLICE_ROWS = L.CONST["gram.kMinSliceRows"]     # rows a slice takes at least when the plan is not forced
THREADS = L.CONST["gram.kThreads"]                 # lanes of a block; GENERAL owns one pair per lane
MAX_GRID_TILES = L.CONST["gram.kMaxGridTiles"]     # tiles (MFMA) or pair blocks (GENERAL) side by side in the grid; a block strides over the rest
MAX_GRID_BLOCKS = L.CONST["gram.kMaxGridBlocks"]   # blocks of a launch, slices included


def mfma_slices(n_variants: int, a_count: int, b_count: int, forced: int = 0, num_cus: int = 256) -> int:
    """Row ranges per tile of an MFMA launch."""
    return L.call("gram_slices", 2, n_variants, a_count, b_count, forced, num_cus)[1]


def mfma_tiles(a_count: int, b_count: int) -> int:
    """Tiles of an MFMA launch; past MAX_GRID_TILES the blocks stride."""
    return L.call("sample_pair_tiles", 4, a_count, b_count)[0]


def general_pair_blocks(a_count: int, b_count: int) -> int:
    """Blocks of THREADS pairs of a GENERAL launch; past MAX_GRID_TILES the blocks stride."""
    return L.call("sample_pair_tiles", 4, a_count, b_count)[2]


def general_slices(n_variants: int, a_count: int, b_count: int, forced: int = 0, num_cus: int = 256) -> int:
    """Row ranges per pair block of a GENERAL launch (eight blocks per CU, units of one row)."""
    return L.call("gram_slices", 2, n_variants, a_count, b_count, forced, num_cus)[0]
