"""One bit per pair — GPU leg (pgenhip_pair_mask / _at through GtEngine): the forward and backward masks against the exact
reference (tests/prune_ref.py, whose guard keeps every r^2 away from the threshold) at every N, keep set, layout, V, W, n_left and
grid where gt_pair.hip takes another path; framing, OR-only writes, block-wise calls, keys, exact equality with the threshold,
streams, a captured graph and the refusals.  The data builders are plain numpy: tests/test_prune.py runs them on the CPU to show
that no case trips the guard."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_ref
import pair_ref as PR
import prune_ref as R
import pgen_rs_amd
from pgen_rs_amd import _capi
from test_pair_stats_gpu import KEEPS, keep_set

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_U = 0xA5A5A5A5
MIN_R2 = 0.21337          # no small rational sits next to its float32 (the guard of prune_ref.edges holds for every case below)

N_LIST = [1, 31, 32, 33, 511, 512, 513, 2504]
V_LIST = [2, 17, 33, 100]
W_LIST = [1, 16, 31, 32, 33, 64, 65, 100]


# ---- data (numpy only) ---------------------------------------------------------------------------------------------------------------
def ld_records(seed, v, n, **kw):
    """(codes (v, n), records (v, R) with dirty pad bits) of rows with LD."""
    rng = np.random.default_rng(seed)
    codes = R.ld_codes(rng, v, n, **kw)
    recs = pack_ref.pack_codes(codes.astype(np.uint8))
    if n % 4:
        recs[:, -1] |= ((rng.integers(0, 256, size=v).astype(np.uint16) << (2 * (n % 4))) & 0xFF).astype(np.uint8)
    return codes, recs


def layout_case(n, keep):
    """The N x keep-set case: 21 LD rows, their gather list and the two references (plain rows, gathered rows)."""
    v, w = 21, 5
    kept = keep_set(keep, n)
    codes, recs = ld_records(n * 43 + len(keep), v, n, redraw=0.2)
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3), [4, 4, 4]]).astype(np.int32)
    kc = codes if kept is None else codes[:, np.asarray(kept, dtype=np.int64)]
    return dict(n=n, v=v, w=w, kept=kept, recs=recs, gather=gather,
                plain=R.edges(kc, v, w, MIN_R2), gathered=R.edges(kc[gather], len(gather), w, MIN_R2))


def grid_case():
    """100 LD rows of 300 samples and the r^2 of all their pairs up to d = 100, computed once."""
    codes, _ = ld_records(7, 100, 300, redraw=0.12, fresh_every=23)
    rng = np.random.default_rng(8)
    for r, back in [(r, 35) for r in range(36, 100, 3)] + [(r, 67) for r in range(68, 100, 5)] + [(99, 99), (98, 96)]:
        pick = rng.random(300) < 0.05          # a near copy of a row far behind: edges in the second, third and fourth mask word
        codes[r] = np.where(pick, rng.integers(0, 3, size=300), codes[r - back])
    recs = pack_ref.pack_codes(codes.astype(np.uint8))
    return codes, recs, R.r2_grid(codes, 100, 100)


def key_case():
    """40 LD rows on three chromosomes: (codes, records, chromosome ranks, positions)."""
    codes, recs = ld_records(19, 40, 200, redraw=0.08)
    chrom = np.array([0] * 17 + [1] * 13 + [2] * 10, dtype=np.uint64)
    pos = np.concatenate([1000 + 100 * np.arange(17), 500 + 70 * np.arange(13), 90 + 10 * np.arange(10)]).astype(np.uint64)
    return codes, recs, chrom, pos


def key_variants():
    """(name, keys as Python ints, max_span) of every key leg."""
    _, _, chrom, pos = key_case()
    keys = [(int(c) << 32) | int(p) for c, p in zip(chrom, pos)]
    swapped = list(keys)
    swapped[5], swapped[6] = swapped[6], swapped[5]                    # out of order inside a chromosome
    high = [(k + (0xFFFFFFFE << 32)) & R.M64 for k in keys]            # the last chromosome's keys wrap past 2^64
    return [("span 300", keys, 300), ("span 299", keys, 299), ("span 100", keys, 100), ("span 99", keys, 99),
            ("chromosomes only", [int(c) << 32 for c in chrom], 0), ("out of order", swapped, 250),
            ("keys >= 2^63", [(k + (1 << 63)) & R.M64 for k in keys], 300), ("keys that wrap", high, 300),
            ("everything inside", keys, R.M64)]


# ---- launches ------------------------------------------------------------------------------------------------------------------------
def run_mask(eng, v, n_left, w, want, what, *, min_r2=MIN_R2, key=None, max_span=0, pad=0, bwd=True, init=None, **rows):
    """One call into framed masks: rows of ceil(W / 32) + pad words at a 4-byte boundary that is not an 8-byte one.  Mask words start
    as zeros (or ``init``'s words), pad words and the frames as the sentinel; afterwards every word must be what it was, ORed with
    the reference's bits ``want`` (boolean (>= v, >= w)).  Returns the words of both masks."""
    words = R.mask_words(w)
    stride = words + pad
    start = np.zeros((v, stride), dtype=np.uint32)
    start[:, words:] = SENT_U
    if init is not None:
        start[:, :words] = init
    got = []
    raws = []
    for _ in range(2 if bwd else 1):
        raw = np.full(1 + v * stride + 8, SENT_U, dtype=np.uint32)
        raw[1: 1 + v * stride] = start.reshape(-1)
        raws.append(torch.from_numpy(raw.view(np.int32)).to(DEV))
    views = [r[1:] for r in raws]
    d_key = None if key is None else torch.from_numpy(np.array(key, dtype=np.uint64).view(np.int64)).to(DEV)
    kw = dict(n_left=n_left, window=w, min_r2=min_r2, key=d_key, max_span=max_span, fwd=views[0], bwd=views[1] if bwd else None,
              want_bwd=False, mask_stride=stride)
    if "base" in rows:
        res = eng.pair_mask_at(rows["base"], rows["record_off"], v, **kw)
    else:
        res = eng.pair_mask(n_variants=v, **rows, **kw)
    eng.wait()
    assert res[0] is views[0] and (res[1] is views[1] if bwd else res[1] is None)
    e = np.zeros((v, w), dtype=bool)
    e[:min(v, want.shape[0])] = want[:v, :w]
    e[n_left:] = False
    e &= (np.arange(v)[:, None] + np.arange(1, w + 1)[None, :]) < v
    ref = R.masks(e, stride)
    for raw, r, name in zip(raws, ref, ("fwd", "bwd")):
        h = raw.cpu().numpy().view(np.uint32)
        assert h[0] == SENT_U and (h[1 + v * stride:] == SENT_U).all(), f"{what}: {name} wrote outside its rows"
        body = h[1: 1 + v * stride].reshape(v, stride)
        bad = np.argwhere(body != (start | r))
        assert not bad.size, (f"{what}: {name} differs in {len(bad)} words; first row {bad[0][0]} word {bad[0][1]}: got "
                              f"{body[tuple(bad[0])]:#010x}, want {(start | r)[tuple(bad[0])]:#010x}")
        got.append(body)
    return got


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", KEEPS)
def test_layouts_and_keep_sets(n, keep):
    c = layout_case(n, keep)
    v, w, recs, gather = c["v"], c["w"], c["recs"], c["gather"]
    r = recs.shape[1]
    stride = r + 5
    raw = np.random.default_rng(n).integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    for i in range(v):
        raw[3 + i * stride: 3 + i * stride + r] = recs[i]
    d_raw = torch.from_numpy(raw).to(DEV)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + int(i) * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    aligned = torch.from_numpy(recs.reshape(-1).copy()).to(DEV)
    vg = len(gather)
    with pgen_rs_amd.GtEngine(n, kept_idx=c["kept"], device=0) as eng:
        run_mask(eng, v, v, w, c["plain"], "padded stride", pad=1, records=d_raw, record_stride=stride, records_offset=3)
        run_mask(eng, v, v, w, c["plain"], "dense from an odd base", records=dense, records_offset=1)
        run_mask(eng, v, v - 3, w, c["plain"], "dense, aligned", pad=2, records=aligned)
        run_mask(eng, vg, vg, w, c["gathered"], "gathered", records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather)
        run_mask(eng, vg, vg, w, c["gathered"], "_at with gaps", pad=1, base=d_raw, record_off=d_offs)
        run_mask(eng, 1, 1, w, c["plain"], "one row", records=aligned)


@pytest.fixture(scope="module")
def grid300():
    codes, recs, grid = grid_case()
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        yield eng, torch.from_numpy(recs.reshape(-1).copy()).to(DEV), codes, grid


@pytest.mark.parametrize("v", V_LIST)
@pytest.mark.parametrize("w", W_LIST)
def test_v_w_n_left_and_forced_grids(grid300, v, w):
    """V, n_left and W around the tile (16) and the mask word (32), on grids of 1, 2 and 3 blocks and the grid by shape."""
    eng, d, codes, grid = grid300
    want = R.edges(codes[:v], v, w, MIN_R2, grid=(grid[0][:v, :w], grid[1][:v, :w]))
    try:
        for blocks in (1, 2, 3, 0):
            eng.tune(_capi.KNOB_PAIR_BLOCKS, blocks)
            for n_left in sorted({1, v // 2, max(v - w, 1), v - 1} - {0}):
                run_mask(eng, v, n_left, w, want, f"V {v} W {w} n_left {n_left} blocks {blocks}", pad=blocks % 2, records=d)
    finally:
        eng.tune(_capi.KNOB_PAIR_BLOCKS, 0)


def test_ld_rows_have_edges_and_non_edges(grid300):
    eng, d, codes, grid = grid300
    v, w = 100, 100
    want = R.edges(codes, v, w, MIN_R2, grid=grid)
    exists = (np.arange(v)[:, None] + np.arange(1, w + 1)[None, :]) < v
    assert want.sum() > 50 and (~want & exists).sum() > 50
    assert want[:, 32:64].any() and want[:, 64:96].any() and want[:, 96:].any()          # edges in every mask word
    assert (~want[:, :3] & exists[:, :3]).any()                                          # and near non-edges
    fwd, bwd = run_mask(eng, v, v, w, want, "LD rows", records=d)
    assert sum(bin(int(x)).count("1") for x in fwd.reshape(-1)) == want.sum() == sum(bin(int(x)).count("1") for x in bwd.reshape(-1))


def test_or_only_and_no_backward_mask(grid300):
    eng, d, codes, grid = grid300
    v, w = 70, 40
    want = R.edges(codes[:v], v, w, MIN_R2, grid=(grid[0][:v, :w], grid[1][:v, :w]))
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 1 << 32, size=(v, 2), dtype=np.uint64).astype(np.uint32) & rng.integers(0, 1 << 32, size=(v, 2), dtype=np.uint64).astype(np.uint32)
    run_mask(eng, v, v, w, want, "pre-set bits", init=pre, pad=1, records=d)
    run_mask(eng, v, v, w, want, "no backward mask", bwd=False, pad=1, records=d)
    # the wrapper's own masks: zeros, (V, stride), both
    fwd, bwd = eng.pair_mask(d, n_variants=v, window=w, min_r2=MIN_R2)
    eng.wait()
    rf, rb = R.masks(want)
    assert fwd.shape == bwd.shape == (v, 2) and fwd.dtype == torch.int32
    assert (fwd.cpu().numpy().view(np.uint32) == rf).all() and (bwd.cpu().numpy().view(np.uint32) == rb).all()
    with pytest.raises(ValueError):
        eng.pair_mask(d, n_variants=v, window=0, min_r2=MIN_R2)
    with pytest.raises(ValueError):
        eng.pair_mask(d, n_variants=v, window=w, min_r2=MIN_R2, mask_stride=1)


@pytest.mark.parametrize("rows", [37, 16, 5])
def test_block_wise_calls_with_halo_equal_one_call(grid300, rows):
    eng, d, codes, grid = grid300
    v, w = 100, 20
    want = R.edges(codes, v, w, MIN_R2, grid=(grid[0][:, :w], grid[1][:, :w]))
    rf, rb = R.masks(want)
    fwd = torch.zeros((v, 1), dtype=torch.int32, device=DEV)
    bwd = torch.zeros((v, 1), dtype=torch.int32, device=DEV)
    r = eng.record_size
    for r0 in range(0, v, rows):
        own = min(rows, v - r0)
        eng.pair_mask(d, n_variants=min(own + w, v - r0), n_left=own, window=w, min_r2=MIN_R2, fwd=fwd[r0:], bwd=bwd[r0:], records_offset=r0 * r)
    eng.wait()
    assert (fwd.cpu().numpy().view(np.uint32) == rf).all() and (bwd.cpu().numpy().view(np.uint32) == rb).all()


def test_exact_equality_with_the_threshold():
    """r^2 = 64 / 256 = 0.25 and r^2 = 1 exactly (the device's doubles hold both quotients exactly): clear at the threshold itself,
    set with the threshold one float32 below."""
    n = 8
    codes = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 1, 0, 0, 0], [0, 1, 2, 0, 1, 2, 0, 0], [0, 1, 2, 0, 1, 2, 0, 0]])
    assert PR.r2_exact(PR.table(codes[0], codes[1])) == R.Fraction(1, 4) and PR.r2_exact(PR.table(codes[2], codes[3])) == 1
    d = torch.from_numpy(pack_ref.pack_codes(codes.astype(np.uint8)).reshape(-1).copy()).to(DEV)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for m, pair, rows in ((np.float32(0.25), (0, 1), slice(0, 2)), (np.float32(1.0), (2, 3), slice(2, 4))):
            want = R.edges(codes[rows], 2, 1, m)                      # through the guard: equality is not "too close"
            assert not want.any()
            run_mask(eng, 2, 2, 1, want, f"r^2 == {m}", min_r2=float(m), records=d, records_offset=2 * rows.start)
            below = float(np.nextafter(m, np.float32(0)))
            # (the guard would refuse this threshold, rightly: what makes the outcome certain is that the quotient is exact)
            run_mask(eng, 2, 2, 1, np.ones((2, 1), dtype=bool), f"r^2 == {m}, threshold one float32 below", min_r2=below, records=d,
                     records_offset=2 * rows.start)


def test_keys_spans_and_chromosome_ends():
    codes, recs, chrom, pos = key_case()
    v, w = 40, 12
    d = torch.from_numpy(recs.reshape(-1).copy()).to(DEV)
    grid = R.r2_grid(codes, v, w)
    free = R.edges(codes, v, w, MIN_R2, grid=grid)
    seen = set()
    with pgen_rs_amd.GtEngine(200, device=0) as eng:
        for name, keys, span in key_variants():
            want = R.edges(codes, v, w, MIN_R2, key=keys, max_span=span, grid=grid)
            seen.add(int(want.sum()))
            run_mask(eng, v, v, w, want, name, key=keys, max_span=span, records=d)
            if name == "everything inside":
                assert (want == free).all()
            else:
                assert want.sum() < free.sum() and not want[16, :].any()       # row 16 is its chromosome's last
    assert len(seen) >= 5                                                       # the spans cut on both sides of real distances


@pytest.mark.parametrize("n", [5, 301, 2503])
def test_dirty_pad_bits_are_not_counted(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v, w = 35, 17
        codes, recs = ld_records(n, v, n, redraw=0.15)
        recs[:, -1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)
        d = torch.from_numpy(recs.reshape(-1).copy()).to(DEV)
        run_mask(eng, v, v, w, R.edges(codes, v, w, MIN_R2), "dirty pad", records=d)


def test_overlapping_launches_on_three_streams():
    n, v, w = 2504, 60, 32
    kept = list(range(0, n, 3))
    codes, recs = ld_records(5, 3 * v, n, redraw=0.1)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = torch.from_numpy(recs.reshape(-1).copy()).to(DEV)
        r = eng.record_size
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [(torch.zeros((v, 1), dtype=torch.int32, device=DEV), torch.zeros((v, 1), dtype=torch.int32, device=DEV)) for _ in range(3)]
        torch.cuda.synchronize()
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.pair_mask(d, n_variants=v, window=w, min_r2=MIN_R2, records_offset=i * v * r, fwd=outs[i][0], bwd=outs[i][1])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            rf, rb = R.masks(R.edges(codes[i * v:(i + 1) * v][:, kept], v, w, MIN_R2))
            assert (outs[i][0].cpu().numpy().view(np.uint32) == rf).all() and (outs[i][1].cpu().numpy().view(np.uint32) == rb).all(), i


def test_hip_graph_capture_and_two_replays():
    n, v, w = 300, 50, 33
    codes, recs = ld_records(77, v, n, redraw=0.1)
    kept = keep_set("every7", n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d_recs = torch.zeros(recs.size, dtype=torch.uint8, device=DEV)
        fwd = torch.zeros((v, 2), dtype=torch.int32, device=DEV)
        bwd = torch.zeros((v, 2), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.pair_mask(d_recs, n_variants=v, window=w, min_r2=MIN_R2, fwd=fwd, bwd=bwd)      # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.pair_mask(d_recs, n_variants=v, window=w, min_r2=MIN_R2, fwd=fwd, bwd=bwd)
        d_recs.copy_(torch.from_numpy(recs.reshape(-1).copy()))
        fwd.zero_()
        bwd.zero_()
        rf, rb = R.masks(R.edges(codes[:, kept], v, w, MIN_R2))
        assert rf.any()
        for replay in range(2):                                     # the second replay ORs the same bits in: nothing changes
            g.replay()
            torch.cuda.synchronize()
            assert (fwd.cpu().numpy().view(np.uint32) == rf).all() and (bwd.cpu().numpy().view(np.uint32) == rb).all(), replay
        eng.use_torch_stream()


def test_refusals_write_nothing():
    lib = _capi.lib
    f = C.c_float
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 8, dtype=torch.uint8, device=DEV)
        buf = torch.full((64,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)
        keys = torch.zeros(9, dtype=torch.int64, device=DEV)
        offs = torch.zeros(8, dtype=torch.int64, device=DEV)
        ctx, rp, fp, bp, kp = eng._ctx, recs.data_ptr(), buf.data_ptr(), buf.data_ptr() + 128, keys.data_ptr()
        B, T = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call = lib.pgenhip_pair_mask
        assert call(ctx, rp, 75, None, 8, 8, 0, f(0.2), None, 0, fp, bp, 1, 0) == B              # window == 0
        assert call(ctx, rp, 75, None, 8, 9, 4, f(0.2), None, 0, fp, bp, 1, 0) == B              # n_left > n_variants
        assert call(ctx, rp, 75, None, 8, 8, 4, f(float("nan")), None, 0, fp, bp, 1, 0) == B     # NaN threshold
        assert b"NaN" in lib.pgenhip_last_error_detail()
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), None, 0, None, bp, 1, 0) == B            # NULL d_fwd with pairs
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), None, 0, fp + 2, bp, 1, 0) == B          # masks need 4 bytes
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), None, 0, fp, bp + 1, 1, 0) == B
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), kp + 4, 0, fp, bp, 1, 0) == B            # keys need 8 bytes
        assert call(ctx, rp, 75, None, 0, 0, 4, f(0.2), kp + 4, 0, fp, bp, 1, 0) == B            # ... pairs or not
        assert call(ctx, rp, 75, None, 8, 8, 33, f(0.2), None, 0, fp, bp, 1, 0) == B             # mask_stride < ceil(W / 32)
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), None, 0, fp, bp, 0, 0) == B
        assert call(ctx, rp, 75, None, 8, 8, 4, f(0.2), None, 0, fp, bp, 1, 1) == B              # unknown flags
        assert call(ctx, None, 75, None, 8, 8, 4, f(0.2), None, 0, fp, bp, 1, 0) == B            # NULL records
        assert call(ctx, rp, 74, None, 8, 8, 4, f(0.2), None, 0, fp, bp, 1, 0) == B              # stride < R
        assert lib.pgenhip_pair_mask_at(ctx, rp, None, 8, 8, 4, f(0.2), None, 0, fp, bp, 1, 0) == B
        assert lib.pgenhip_pair_mask_at(ctx, rp, offs.data_ptr(), 8, 8, 4, f(0.2), None, 0, fp + 2, bp, 1, 0) == B
        assert call(ctx, rp, 75, None, 1 << 20, 8, 4, f(0.2), None, 0, fp, bp, 1 << 30, 0) == T  # n_variants * mask_stride * 4 = 2^52
        assert b"2^52" in lib.pgenhip_last_error_detail()
        # no pair exists: OK whatever the masks; one left row and no backward mask: one mask row, any stride
        assert call(ctx, rp, 75, None, 8, 0, 4, f(0.2), None, 0, None, None, 0, 0) == _capi.OK
        assert call(ctx, rp, 75, None, 1, 1, 4, f(0.2), None, 0, None, None, 0, 0) == _capi.OK
        eng.wait()
        assert (buf.cpu().numpy() == -0x5A5A5A5B).all(), "a refused call wrote"
