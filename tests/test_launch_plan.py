"""Properties of the launch plans (csrc/launch_plan.h, run through tests/launch_plan.py) that hold for EVERY shape, which pinning
single values cannot state: the slices of a launch tile its rows in order without gaps and none is empty, grids stay inside their
caps and the 32-bit block index, and a forced value is honoured up to the documented caps.  A few hundred shapes per family: the
edge sizes the ``*_plan.py`` modules list plus seeded random ones, forced in {0, 1, 3, 7}, num_cus in {0, 1, 256, 304}.  No GPU."""
import itertools
import random

import count_plan as CP
import gram_plan as GP
import launch_plan as L
import matrix_plan as MP
import score_plan as RP
import scount_plan as SP
import vsum_plan as VP

FORCED = (0, 1, 3, 7)
CUS = (0, 1, 256, 304)
I31 = 0x7FFFFFFF          # tiles * slices is cast to the 32-bit grid size below this
U32 = 0xFFFFFFFF


def shapes(seed, edges_n, edges_v, count=300, max_n_log2=20, max_v_log2=24):
    """(N, V, forced, num_cus): every edge size once at least, then random sizes (log-uniform), knobs cycled."""
    rng = random.Random(seed)
    knobs = itertools.cycle(itertools.product(FORCED, CUS))
    ns = sorted({max(1, n + d) for n in edges_n for d in (-1, 0, 1)})
    vs = sorted({max(1, v + d) for v in edges_v for d in (-1, 0, 1)})
    out = [(n, rng.choice(vs), *next(knobs)) for n in ns] + [(rng.choice(ns), v, *next(knobs)) for v in vs]
    while len(out) < count:
        out.append((int(2 ** rng.uniform(0, max_n_log2)), int(2 ** rng.uniform(0, max_v_log2)), *next(knobs)))
    return out


def check_slices(rows, slices, never_empty=True):
    """The slices of slice_rows tile [0, rows) in order without gaps (all of them up to 64, else both ends and the middle)."""
    assert slices >= 1
    idx = range(slices) if slices <= 64 else [0, 1, slices // 2 - 1, slices // 2, slices - 2, slices - 1]
    prev_end = None
    for i in idx:
        b, e = L.slice_rows(rows, i, slices)
        assert b <= e and (not never_empty or b < e), (rows, i, slices)
        if prev_end is not None and i == prev_i + 1:
            assert b == prev_end
        prev_end, prev_i = e, i
    assert L.slice_rows(rows, 0, slices)[0] == 0 and L.slice_rows(rows, slices - 1, slices)[1] == rows


def cap(per_cu, cus, forced):
    return forced if forced > 0 else L.cu_count(cus) * per_cu


def test_shared_helpers():
    assert [L.cu_count(c) for c in (-1, 0, 1, 256, 304)] == [256, 256, 1, 256, 304]
    assert L.grid_blocks(0, 8) == 1 and L.grid_blocks(5, 8) == 5 and L.grid_blocks(10 ** 9, 8) == 2048 and L.grid_blocks(10 ** 9, 8, 304, 3) == 3
    for rows, slices in ((1, 1), (7, 7), (10, 3), (U32, 7), (U32, 1 << 22), (1 << 30, 556)):
        check_slices(rows, slices)
    assert L.slice_rows(10, 1, 3) == (3, 6) and L.slice_rows(2, 0, 3) == (0, 0)   # more slices than rows: empty ones


def test_count():
    for n, v, _, cus in shapes(1, CP.CLASS_EDGES + [4, 300, 2504, 500_000], [1, 8192, 32768, 262144]):
        r = CP.record_size(n)
        assert CP.lanes_per_row(r) in (4, 8, 16, 32, 64)
        for kernel in (CP.AUTO, CP.WAVE_PER_ROW, CP.ROWS_PER_WAVE):
            g, ru, u = CP.shape(n, kernel)
            assert (g, ru, u) in CP.SHAPES.values()
            assert (g == 64) == (kernel == CP.WAVE_PER_ROW or (kernel == CP.AUTO and CP.lanes_per_row(r) == 64))
            assert CP.passes(r, g, u) * g * u >= CP.max_chunks(r) > (CP.passes(r, g, u) - 1) * g * u   # the passes cover the row, none spare
            assert kernel == CP.ROWS_PER_WAVE or CP.passes(r, g, u) <= 3 or g == 64                # three passes at most unless forced
            grid = CP.grid(v, g, ru, cus)
            assert 1 <= grid <= cap(CP.BLOCKS_PER_CU, cus, 0)
            assert grid * CP.rows_per_block(g, ru) >= min(v, CP.rows_per_grid(g, ru, cus))        # short launches: a row per slot, no stride


def test_scount():
    for n, v, forced, cus in shapes(2, SP.CLASS_EDGES + [300, 2504, 500_000], [1, 8, 32, 2040 * 4, SP.window_rows(300, 3)]):
        g, tiles, cols, slices, lds_bytes, slots = SP.plan(n, v, forced, cus)
        c = SP.columns(n)
        assert g in (4, 8, 16, 32, 64) and tiles * g >= c > (tiles - 1) * g and slots * g == SP.THREADS
        assert cols == (c if tiles == 1 else g) and lds_bytes == 3 * cols * 65 * 4 <= 64 * 1024
        assert 1 <= tiles * slices <= I31
        check_slices(v, slices)                              # one batch of every slot at least: never empty
        step = slots * SP.BATCH
        if forced:
            assert slices <= forced and (slices == forced or slices == -(-v // step))
        else:
            assert slices <= max(1, L.cu_count(cus) * 4 // tiles)


def test_score():
    for n, v, forced, cus in shapes(3, [16, 32, 64, 128, 256, 1024, 2504, 500_000], [1, 8, 32, 512, 1024, 512 * 7]):
        for c in (1, 2, 3, 4, 5, 8):
            lane_bytes, batch, log_g, tiles, slices, slots = RP.plan(n, c, v, forced, cus)
            units = -(-RP.record_size(n) // lane_bytes)
            assert 4 * lane_bytes * c <= 32 and log_g <= 6 and tiles * (1 << log_g) >= units > (tiles - 1) * (1 << log_g)
            assert log_g == 0 or (1 << (log_g - 1)) < units  # the fewest lanes that cover a row
            assert 1 <= tiles * slices <= I31
            check_slices(v, slices)
            step = slots * batch
            if forced:
                assert slices <= forced and (slices == forced or slices == -(-v // step))
            else:
                assert slices <= max(1, L.cu_count(cus) * 4 // tiles) and (slices == 1 or v // slices >= RP.MIN_SLICE_ROWS)


def test_vsum():
    for n, v, forced, cus in shapes(4, VP.edge_samples() + [2504, 500_000], VP.edge_rows(3) + VP.edge_rows(7) + [256, 512, 256 * 7]):
        tiles, slices, grid, atomic, groups = VP.plan(n, v, forced, cus)
        assert tiles == -(-VP.record_size(n) // VP.TILE_BYTES) and atomic == (tiles > 1) and groups == -(-v // VP.GROUP_ROWS)
        assert 1 <= tiles * slices <= I31 and 1 <= grid <= min(tiles * slices, cap(8, cus, forced))
        check_slices(groups, slices)                         # at least one group per wave: never empty
        assert slices <= -(-groups // VP.WAVES)
        if forced:
            assert slices <= forced and (slices == forced or slices == -(-groups // VP.WAVES))
        else:
            assert slices == 1 or v // slices >= VP.MIN_SLICE_ROWS
        for c in (1, 16):
            assert 1 <= L.call("vsum_general_grid", 1, v, c, cus, forced)[0] <= min(-(-v * c // VP.WAVES), cap(8, cus, forced))


def test_matrix():
    rng = random.Random(5)
    for k, v, forced, cus in shapes(5, MP.N_EDGES + [300, 2504, 500_000], MP.V_EDGES + [1, 2, 37], max_v_log2=20):
        for elem in (1, 2, 4):
            addr, pad = rng.choice([0, elem, 13 * elem, 16]), rng.choice([0, 0, elem, 16])
            stride = k * elem + pad
            dense, long_rows, per_row, total, gx, gy = MP.stream_plan(v, k, elem, addr, stride, cus, forced)
            assert dense == (v == 1 or pad == 0) and long_rows == (k * elem >= MP.LONG_ROW_BYTES) and per_row == -(-k * elem // 16) + 1
            assert total * 16 >= k * elem * v and total <= per_row * v        # a lane per chunk that holds a byte, no more than every row's own
            c = cap(MP.BLOCKS_PER_CU, cus, forced)
            if long_rows:
                assert 1 <= gx <= max(1, -(-per_row // MP.THREADS)) and 1 <= gy <= min(v, 65535) and (gy == 1 or gx * gy <= c)
                assert gx == 1 or not forced                                  # a forced grid goes along the rows
            else:
                assert gy == 1 and 1 <= gx <= min(max(1, -(-total // MP.THREADS)), c)
            assert 1 <= MP.general_grid(v, k, cus, forced) <= min(-(-v * k // MP.THREADS), c)
        vt, bands = MP.tile_counts(v, k)
        assert vt == -(-v // MP.TILE_VARIANTS) and bands == -(-k // MP.TILE_SAMPLES)
        assert 1 <= MP.tile_grid(v, k, cus, forced) <= min(vt * bands, cap(MP.TILE_BLOCKS_PER_CU, cus, forced))
        # AUTO asks STREAM first, then TILE, else GENERAL; the forced-shape predicates agree with it
        for all_kept, sample_major in itertools.product((False, True), repeat=2):
            stride = rng.choice([16 * rng.randint(1, 10 ** 5), v + 1, 33])
            shape, stream_ok, tile_ok = L.call("matrix_auto_shape", 3, all_kept, sample_major, addr % 16, stride, k)
            assert shape == (MP.STREAM if stream_ok else MP.TILE if tile_ok else MP.GENERAL) and not (stream_ok and tile_ok)
            assert stream_ok == (all_kept and not sample_major)
            assert tile_ok == (all_kept and sample_major and addr % 16 == 0 and (stride % 16 == 0 or k <= 1))


def test_pair():
    tile, per_cu = L.CONST["pair.kTile"], L.CONST["pair.kBlocksPerCu"]
    for w, v, forced, cus in shapes(6, [1, tile, 2 * tile, 1000], [2, tile, 2 * tile, 3 * tile + 2], max_n_log2=24):
        v = max(v, 2)
        for n_left in {1, max(1, v // 2), v - 1, v}:
            w_eff, tiles_per_left, n_items, grid = L.call("pair_plan", 4, v, n_left, w, cus, forced)
            assert w_eff == min(w, v - 1) and 1 <= tiles_per_left <= -(-v // tile)
            # the right tiles that hold a partner of the last row of any left tile, the diagonal tile included
            assert tiles_per_left == min((tile - 1 + w_eff) // tile + 1, -(-v // tile))
            assert n_items == -(-n_left // tile) * tiles_per_left
            assert grid == forced if forced else 1 <= grid <= min(n_items, L.cu_count(cus) * per_cu)


def test_pack():
    part = L.CONST["pack.kPartChunks"]
    for n, v, forced, cus in shapes(7, CP.CLASS_EDGES + [4, 300, 2504, 500_000], [1, 2, 16, 64, 873, 874, 1746, 1747]):
        r, c = CP.record_size(n), cap(L.CONST["pack.kBlocksPerCu"], cus, forced)
        g, p, parts, items, grid = L.call("pack_dense_plan", 5, r, v, cus, forced)
        chunks = (r + 30) // 16
        assert g == CP.lanes_per_row(r) and p == (part // 64 if g == 64 else 3)      # the ladder of the count kernel
        assert parts * g * p >= chunks > (parts - 1) * g * p and (parts == 1 or g == 64)
        assert items == -(-v // (64 // g)) * parts and 1 <= grid <= min(-(-items // 4), c)
        q, total, ggrid = L.call("pack_gather_plan", 3, v, n, cus, forced)
        assert q == -(-n // 16) and total == v * q and 1 <= ggrid <= min(-(-total // 256), c)
        assert 1 <= L.call("pack_general_grid", 1, v, n, cus, forced)[0] <= min(-(-v * -(-n // 4) // 256), c)
        # runs of rows go as one row only from two whole runs on, of dense records without pad bits into dense output
        merge, m = L.call("pack_merge_runs", 2, 0, n, r, r, r, v)
        assert m == L.CONST["pack.kStreamRunBytes"] // r and merge == (n % 4 == 0 and m >= 2 and v >= 2 * m)
        assert L.call("pack_merge_runs", 2, 1, n, r, r, r, v)[0] == 0 and L.call("pack_merge_runs", 2, 0, n, r, r + 1, r, v)[0] == 0
        assert L.call("pack_merge_runs", 2, 0, n, r, r, r + 1, v)[0] == 0
    assert L.call("pack_applicable", 2, 0, 300, 300) == (1, 0) and L.call("pack_applicable", 2, 1, 300, 300) == (0, 1)
    assert L.call("pack_applicable", 2, 0, 299, 300) == (0, 0) and L.call("pack_applicable", 2, 1, 0, 300) == (0, 0)


def check_sample_pairs(family, step_rows, min_slices):
    tile, max_tiles, max_blocks = GP.TILE, GP.MAX_GRID_TILES, GP.MAX_GRID_BLOCKS
    edges_v = [1, step_rows, 256, 512, 7 * step_rows, 7 * 256, 1 << 30, 1 << 31, U32]
    for a, v, forced, cus in shapes(8, [1, tile, 2 * tile, 2504], edges_v, max_n_log2=17, max_v_log2=32):
        v = min(v, U32)
        for b in {1, a, 70, 100_000}:
            tiles, grid_tiles, pair_blocks, grid_pairs = L.call("sample_pair_tiles", 4, a, b)
            assert tiles == -(-a // tile) * -(-b // tile) and grid_tiles == min(tiles, max_tiles)
            assert pair_blocks == -(-a * b // GP.THREADS) and grid_pairs == min(pair_blocks, max_tiles)
            general, mfma = L.call(family, 2, v, a, b, forced, cus)
            for slices, items, unit in ((general, grid_pairs, 1), (mfma, grid_tiles, step_rows)):
                assert 1 <= items * slices <= max_blocks       # the grid, cast to 32 bits below this
                check_slices(v, slices)                         # never empty: at most one slice per unit of rows
                assert slices >= min_slices(v) and slices <= max(min_slices(v), -(-v // unit))
                assert max(e - b_ for b_, e in (L.slice_rows(v, i, slices) for i in {0, slices // 2, slices - 1})) < 1 << 31 or min_slices(v) == 1
                if forced:
                    assert slices <= max(forced, min_slices(v))
                    assert slices == forced or slices in (-(-v // unit), max_blocks // items, min_slices(v))
                else:
                    assert slices <= max(min_slices(v), 1, L.cu_count(cus) * 8 // items) and (slices <= min_slices(v) or v // slices >= GP.MIN_SLICE_ROWS)


def test_spair():
    """pair_slices with spair's lower clamp: a slice stays below 2^31 rows, so an i32 accumulator stays below its sign bit."""
    assert L.CONST["spair.kMaxGridTiles"] == GP.MAX_GRID_TILES and L.CONST["spair.kMaxGridBlocks"] == GP.MAX_GRID_BLOCKS
    check_sample_pairs("spair_slices", L.CONST["spair.kStepRows"], lambda v: (v >> 30) + 1)
    assert L.call("spair_slices", 2, U32, 64, 64, 1, 256) == (4, 4) and L.call("spair_slices", 2, (1 << 30) - 1, 64, 64, 1, 256) == (1, 1)


def test_gram():
    """pair_slices with gram's lower clamp of 1: one slice means every entry has one owner and is stored."""
    check_sample_pairs("gram_slices", GP.STEP_ROWS, lambda v: 1)
    assert L.call("gram_slices", 2, U32, 64, 64, 1, 256) == (1, 1)
    # the two families differ in that clamp alone
    assert L.call("pair_slices", 1, 5000, 4, 0, 256, 2, 32, 1) == L.call("pair_slices", 1, 5000, 4, 0, 256, 2, 32, 0) == (19,)
