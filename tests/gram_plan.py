"""The launch-plan constants of gt_gram.hip, mirrored for the tests that are placed around them (test_sample_gram.py checks that the
kernel source still holds these values)."""
TILE = 64             # ranks of a block tile, per operand (kTile)
STEP_ROWS = 32        # rows expanded into LDS per step (kStepRows)
GROUP_ROWS = 4        # rows of one v_mfma_f64_16x16x4_f64 (kGroupRows)
MIN_SLICE_ROWS = 256  # rows a slice takes at least when the plan is not forced (kMinSliceRows)
THREADS = 256         # lanes of a block; GENERAL owns one pair per lane (kThreads)


def mfma_slices(n_variants: int, a_count: int, b_count: int, forced: int = 0, num_cus: int = 256) -> int:
    """Row ranges per tile of an MFMA launch (plan_slices of gt_gram.hip)."""
    tiles = -(-a_count // TILE) * -(-b_count // TILE)
    grid_tiles = min(tiles, 1 << 20)
    s = forced if forced > 0 else min(max(1, num_cus * 2 // grid_tiles), max(1, n_variants // MIN_SLICE_ROWS))
    s = min(s, -(-n_variants // STEP_ROWS), (1 << 22) // grid_tiles)
    return max(s, 1)
