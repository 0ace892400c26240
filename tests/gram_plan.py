"""The launch-plan constants of gt_gram.hip, mirrored for the tests that are placed around them (test_sample_gram.py checks that the
kernel source still holds these values)."""
TILE = 64             # ranks of a block tile, per operand (kTile)
STEP_ROWS = 32        # rows expanded into LDS per step (kStepRows)
GROUP_ROWS = 4        # rows of one v_mfma_f64_16x16x4_f64 (kGroupRows)
MIN_SLICE_ROWS = 256  # rows a slice takes at least when the plan is not forced (kMinSliceRows)
THREADS = 256         # lanes of a block; GENERAL owns one pair per lane (kThreads)
MAX_GRID_TILES = 1 << 20    # tiles (MFMA) or pair blocks (GENERAL) side by side in the grid; a block strides over the rest (kMaxGridTiles)
MAX_GRID_BLOCKS = 1 << 22   # blocks of a launch, slices included (kMaxGridBlocks)


def mfma_slices(n_variants: int, a_count: int, b_count: int, forced: int = 0, num_cus: int = 256) -> int:
    """Row ranges per tile of an MFMA launch (plan_slices of gt_gram.hip)."""
    grid_tiles = min(mfma_tiles(a_count, b_count), MAX_GRID_TILES)
    s = forced if forced > 0 else min(max(1, num_cus * 2 // grid_tiles), max(1, n_variants // MIN_SLICE_ROWS))
    s = min(s, -(-n_variants // STEP_ROWS), MAX_GRID_BLOCKS // grid_tiles)
    return max(s, 1)


def mfma_tiles(a_count: int, b_count: int) -> int:
    """Tiles of an MFMA launch; past MAX_GRID_TILES the blocks stride."""
    return -(-a_count // TILE) * -(-b_count // TILE)


def general_pair_blocks(a_count: int, b_count: int) -> int:
    """Blocks of THREADS pairs of a GENERAL launch; past MAX_GRID_TILES the blocks stride."""
    return -(-(a_count * b_count) // THREADS)


def general_slices(n_variants: int, a_count: int, b_count: int, forced: int = 0, num_cus: int = 256) -> int:
    """Row ranges per pair block of a GENERAL launch (plan_slices of gt_gram.hip: eight blocks per CU, units of one row)."""
    grid_pairs = min(general_pair_blocks(a_count, b_count), MAX_GRID_TILES)
    s = forced if forced > 0 else min(max(1, num_cus * 8 // grid_pairs), max(1, n_variants // MIN_SLICE_ROWS))
    s = min(s, n_variants, MAX_GRID_BLOCKS // grid_pairs)
    return max(s, 1)
