"""LD pruning — CPU leg: the references (tests/prune_ref.py) against brute force and hand cases, the guard that keeps every test's
r^2 away from its threshold (run here on the GPU files' own data), the plan twin (tests/prune_plan.py) against the plan header,
the three C ABI symbols, their constants and the status codes that need no device."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import pair_ref as PR
import prune_plan as PP
import prune_ref as R
from pgen_rs_amd import _capi

REPO = Path(__file__).resolve().parent.parent


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_edges_against_a_per_pair_loop(seed):
    rng = np.random.default_rng(seed)
    v, n, w = int(rng.integers(2, 12)), int(rng.integers(5, 80)), int(rng.integers(1, 6))
    n_left = v - seed % 2
    codes = R.ld_codes(rng, v, n, redraw=0.3)
    key = None if seed % 2 else [int(x) for x in np.cumsum(rng.integers(0, 40, size=v))]
    m = 0.2345
    got = R.edges(codes, n_left, w, m, key=key, max_span=50)
    assert got.shape == (v, w)
    for i in range(v):
        for d in range(1, w + 1):
            want = False
            if i < n_left and i + d < v:
                x = PR.r2_exact(PR.table(codes[i], codes[i + d]))
                want = x is not None and x > Fraction(float(np.float32(m))) and (key is None or key[i + d] - key[i] <= 50)
            assert bool(got[i, d - 1]) == want, (i, d)


def test_edges_keys_are_taken_mod_2_64():
    codes = np.array([[0, 1, 2, 0, 1, 2, 0, 0]] * 3)
    assert R.edges(codes, 3, 2, 0.5).tolist() == [[True, True], [True, False], [False, False]]    # identical rows: r^2 = 1 where a pair exists
    assert not R.edges(codes, 3, 2, 0.5, key=[5, 4, 3], max_span=1 << 63).any()          # out of order: the difference wraps
    assert R.edges(codes, 3, 2, 0.5, key=[R.M64, 0, 1], max_span=1)[0, 0]                # 0 - (2^64 - 1) = 1
    assert not R.edges(codes, 3, 2, 0.5, key=[R.M64, 0, 1], max_span=1)[0, 1]            # 1 - (2^64 - 1) = 2


def test_guard_fires_next_to_the_threshold_and_not_on_it():
    codes = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 1, 0, 0, 0]])
    assert PR.r2_exact(PR.table(codes[0], codes[1])) == Fraction(1, 4)
    assert not R.edges(codes, 2, 1, 0.25).any()                                          # equal: not above, and not "too close"
    for steps in (1, 2):
        for toward in (0.0, 1.0):
            m = np.float32(0.25)
            for _ in range(steps):
                m = np.nextafter(m, np.float32(toward))
            with pytest.raises(R.ThresholdTooClose):
                R.edges(codes, 2, 1, m)
    m = np.float32(0.25)
    for _ in range(3):
        m = np.nextafter(m, np.float32(0))
    assert R.edges(codes, 2, 1, m)[0, 0]                                                 # three ulps away: decided
    assert not R.edges(np.zeros((2, 8), dtype=np.int64), 2, 1, 0.0).any()                # NaN is never an edge


def test_masks_layout():
    e = np.zeros((40, 40), dtype=bool)
    e[0, 0] = e[0, 31] = e[0, 32] = e[3, 35] = True
    fwd, bwd = R.masks(e, 3, fill=0)
    assert fwd.shape == (40, 3) and fwd[0].tolist() == [0x80000001, 1, 0] and fwd[3].tolist() == [0, 8, 0]
    assert bwd[1, 0] == 1 and bwd[32, 0] == 0x80000000 and bwd[33, 1] == 1 and bwd[39, 1] == 8
    assert int(fwd.sum()) == int(bwd.sum())
    assert sorted(R.neighbours(fwd, bwd, 40, 0)) == [1, 32, 33] and R.neighbours(fwd, bwd, 40, 39) == [3]
    assert R.neighbours(fwd, bwd, 32, 0) == [1, 32]                                      # bits >= window do not count


# ---- the greedy set -----------------------------------------------------------------------------------------------------------------
def from_edges(n, pairs):
    w = max([b - a for a, b in pairs], default=1)
    e = np.zeros((n, w), dtype=bool)
    for a, b in pairs:
        e[a, b - a - 1] = True
    return R.masks(e) + (w,)


def test_hand_cases():
    K, X = R.KEPT, R.REMOVED
    chain = [(i, i + 1) for i in range(5)]
    f, b, w = from_edges(6, chain)
    assert R.resolve(f, b, w).tolist() == [K, X, K, X, K, X]
    assert R.resolve(f, b, w, priority=[1, 2, 3, 4, 5, 6]).tolist() == [X, K, X, K, X, K]
    assert R.resolve(f, b, w, priority=[5, 9, 1, 1, 9, 5]).tolist() == [X, K, X, X, K, X]
    clique = [(a, c) for a in range(4) for c in range(a + 1, 4)]
    f, b, w = from_edges(4, clique)
    assert R.resolve(f, b, w).tolist() == [K, X, X, X]
    assert R.resolve(f, b, w, priority=[3, 3, 7, 7]).tolist() == [X, X, K, X]            # the tie goes to the earlier row
    star = [(0, i) for i in range(1, 6)]
    f, b, w = from_edges(6, star)
    assert R.resolve(f, b, w).tolist() == [K, X, X, X, X, X]
    assert R.resolve(f, b, w, priority=[0, 1, 1, 1, 1, 1]).tolist() == [X, K, K, K, K, K]
    # pre-set states: a removed centre frees the leaves; a kept leaf removes the centre even though the centre beats it
    assert R.resolve(f, b, w, state0=[X, 0, 0, 0, 0, 0]).tolist() == [X, K, K, K, K, K]
    assert R.resolve(f, b, w, state0=[0, 0, 0, K, 0, 0]).tolist() == [K, X, X, K, X, X]  # row 0 has no beater: kept beside a pre-set leaf
    assert R.resolve(f, b, w, priority=[0, 1, 1, 1, 1, 1], state0=[0, X, X, X, X, X]).tolist() == [K, X, X, X, X, X]
    f, b, w = from_edges(3, [])
    assert R.resolve(f, b, w).tolist() == [K, K, K]


@pytest.mark.parametrize("seed", range(10))
def test_resolve_against_edge_lists(seed):
    rng = np.random.default_rng(100 + seed)
    n, w = int(rng.integers(1, 60)), int(rng.integers(1, 40))
    e = rng.random((n, w)) < 0.15
    e &= (np.arange(n)[:, None] + np.arange(1, w + 1)[None, :]) < n
    fwd, bwd = R.masks(e)
    pairs = [(int(i), int(i + d + 1)) for i, d in np.argwhere(e)]
    prio = [None, rng.integers(0, 4, size=n), rng.integers(0, 1 << 32, size=n, dtype=np.uint64)][seed % 3]
    state0 = None if seed % 2 else rng.choice([0, 0, 1, 2], size=n)
    got = R.resolve(fwd, bwd, w, prio, state0)
    assert (got == R.resolve_from_edge_list(n, pairs, prio, state0)).all()
    assert set(got.tolist()) <= {R.KEPT, R.REMOVED}
    if state0 is None:
        kept = set(np.flatnonzero(got == R.KEPT).tolist())
        assert not any(a in kept and c in kept for a, c in pairs)                         # independent
        for r in np.flatnonzero(got == R.REMOVED):                                        # and every removed row has a kept beater
            assert any((a == r and c in kept) or (c == r and a in kept) for a, c in pairs)


def test_priority_of_counts():
    p = R.priority_of_counts(np.array([[10, 0, 0, 0], [0, 0, 0, 9], [5, 0, 5, 1], [8, 2, 0, 0], [0, 2, 8, 3], [4, 2, 4, 0]]))
    assert p[0] == 0 and p[1] == 0 and p[2] == 2147483647 and p[3] == p[4] == int(0.1 * 4294967294.0) and p[5] == p[2]


# ---- the GPU files' data never trips the guard ----------------------------------------------------------------------------------------
def test_gpu_cases_keep_clear_of_the_threshold():
    import test_pair_mask_gpu as G

    for n in G.N_LIST:
        for keep in G.KEEPS:
            G.layout_case(n, keep)
    codes, _, grid = G.grid_case()
    e = R.edges(codes, 100, 100, G.MIN_R2, grid=grid)
    exists = (np.arange(100)[:, None] + np.arange(1, 101)[None, :]) < 100
    assert e.sum() > 50 and (~e & exists).sum() > 50
    codes, _, _, _ = G.key_case()
    grid = R.r2_grid(codes, 40, 12)
    sums = {int(R.edges(codes, 40, 12, G.MIN_R2, key=k, max_span=s, grid=grid).sum()) for _, k, s in G.key_variants()}
    assert len(sums) >= 5
    for n in (5, 301, 2503):
        R.edges(G.ld_records(n, 35, n, redraw=0.15)[0], 35, 17, G.MIN_R2)
    R.edges(G.ld_records(77, 50, 300, redraw=0.1)[0][:, list(range(0, 300, 7))], 50, 33, G.MIN_R2)
    c = G.ld_records(5, 180, 2504, redraw=0.1)[0][:, list(range(0, 2504, 3))]
    for i in range(3):
        R.edges(c[60 * i: 60 * i + 60], 60, 32, G.MIN_R2)


def test_far_range_cases_are_what_prune_ref_gives_row_by_row():
    """The builders of tests/test_long_rows_prune_gpu.py, at sizes small enough to go through prune_ref row by row: the periodic rows
    never trip the guard and their tiled masks are prune_ref.masks of prune_ref.edges of all rows; the S of a graph of disjoint
    segments (strays and truncated last segment included) is the S of one segment, tiled."""
    import test_long_rows_prune_gpu as G

    _, fwd, bwd, codes = G.periodic_mask_case()
    assert fwd.shape == bwd.shape == (G.V_FAR, 2) and fwd[:, 1].any() and bwd[:, 1].any()
    for v in (50, 200):
        _, f, b, _ = G.periodic_mask_case(v)
        rf, rb = R.masks(R.edges(codes[np.arange(v) % G.P], v, G.W_FAR, G.MIN_R2))
        assert (f == rf).all() and (b == rb).all(), v
        assert (f == fwd[:v]).sum() > f.size // 2 and (b == bwd[:v]).all()    # the long case's first rows, but for the clipping
    v = 2 * G.SEGMENT_TURNS + 517
    f, b, p, s_whole, s_tail = G.many_turns_case(v)
    assert len(s_tail) == 517 and set(p.tolist()) == {0, 1, 2}
    assert (R.resolve(f, b, G.W_TURNS, p) == np.concatenate([s_whole, s_whole, s_tail])).all()
    for prio_values in (0, 1 << 32):
        v = 3 * 90 + 63
        f90, b90, p90, s_whole, s_tail = G.segment_graph(90, 90, 32, 0.1, v, prio_values)
        rows = np.arange(v) % 90
        got = R.resolve(f90[rows], b90[rows], 32, None if p90 is None else p90[rows])
        assert (got == np.concatenate([s_whole] * 3 + [s_tail])).all()
        assert any(R.neighbours(f90[:63], b90[:63], 32, r) != R.neighbours(f90, b90, 32, r) for r in range(63))   # strays exist


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_twin_matches_header():
    assert (PP.THREADS, PP.CHUNK_ROWS, PP.HALO_ROWS, PP.LDS_ROWS) == (256, 1024, 512, 2048) and PP.LDS_ROWS == PP.CHUNK_ROWS + 2 * PP.HALO_ROWS
    for w in (1, 31, 32, 33, 64, 65, 511, 512, 513, 2**32 - 1):
        assert PP.probe("prune_window", 2, w) == (PP.mask_words(w), PP.halo_rows(w))
    c = PP.CHUNK_ROWS
    rows = sorted({0, 1, 2, 255, 256, 257, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 1, 2048 * c, 2048 * c + 1, 10**7, 2**40})
    for n in rows:
        for num_cus, blocks in ((256, 0), (0, 0), (304, 0), (256, 1), (256, 2), (256, 3), (256, 5000)):
            assert PP.probe("prune_general_grid", 1, n, num_cus, blocks)[0] == PP.general_grid(n, num_cus, blocks)
            range_rows, grid = PP.block_plan(n, num_cus, blocks)
            assert PP.probe("prune_block_plan", 2, n, num_cus, blocks) == (range_rows, grid)
            # the ranges tile the rows, none is empty, and a forced grid is never exceeded
            assert grid >= 1 and range_rows * (grid - 1) < max(n, 1) <= range_rows * grid
            assert blocks == 0 or grid <= blocks
        for w in (1, 200, 5000):
            assert bool(PP.probe("prune_auto", 1, n, w)[0]) == PP.auto_block(n, w)
    assert PP.turn_edges(2 * c + 1, 256, 2) == [0, c, c + 1]           # ranges of c + 1 and c rows: two turns, then one
    assert PP.turn_edges(2 * c + 3, 256, 2) == [0, c, c + 2, 2 * c + 2]
    assert PP.turn_edges(c + 1, 256, 1) == [0, c]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["pgenhip_pair_mask", "pgenhip_pair_mask_at", "pgenhip_prune_resolve"])
def test_symbols_exported_and_bound(sym):
    assert getattr(C.CDLL(str(_capi.LIB_PATH)), sym) is not None
    assert sym in _capi.PROTOTYPES


def test_constants_and_header():
    h = (REPO / "include" / "pgen_hip.h").read_text()
    for name, value in (("UNDECIDED", 0), ("KEPT", 1), ("REMOVED", 2), ("AUTO", 0), ("GENERAL", 1), ("BLOCK", 2)):
        assert re.search(rf"#define PGENHIP_PRUNE_{name}\s+{value}u", h) and getattr(_capi, f"PRUNE_{name}") == value
    assert "PGENHIP_KNOB_PRUNE_BLOCKS = 31" in h and _capi.KNOB_PRUNE_BLOCKS == 31
    assert "PGENHIP_ABI_VERSION 2u" in h and _capi.lib.pgenhip_abi_version() == 2
    assert (R.UNDECIDED, R.KEPT, R.REMOVED) == (_capi.PRUNE_UNDECIDED, _capi.PRUNE_KEPT, _capi.PRUNE_REMOVED)
    for phrase in ("d_fwd[i * mask_stride + b / 32]", "never an edge", "mod 2^64 <= max_span", "not the\n * transpose of d_fwd",
                   "without any out-of-bounds access"):
        assert phrase in h, phrase


def test_null_ctx_is_bad_arg():
    lib = _capi.lib
    assert lib.pgenhip_pair_mask(None, None, 0, None, 0, 0, 1, 0.2, None, 0, None, None, 0, 0) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_pair_mask(None, None, 75, None, 9, 9, 4, 0.2, None, 0, None, None, 1, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pair_mask_at(None, None, None, 0, 0, 1, 0.2, None, 0, None, None, 0, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_pair_mask_at(None, None, None, 5, 5, 2, 0.2, None, 0, None, None, 1, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_prune_resolve(None, None, None, 1, 1, 0, None, None, None, 0) == _capi.ERR_BAD_ARG
    assert lib.pgenhip_prune_resolve(None, None, None, 1, 4, 9, None, None, None, _capi.PRUNE_BLOCK) == _capi.ERR_BAD_ARG
    assert b"ctx" in lib.pgenhip_last_error_detail()
    assert lib.pgenhip_tune(None, _capi.KNOB_PRUNE_BLOCKS, 3) == _capi.ERR_BAD_ARG


def test_kernel_sources_are_built():
    from pgen_rs_amd import build

    assert "gt_prune.hip" in build.HIP_SOURCES and (build.CSRC / "gt_prune.hip").exists()
