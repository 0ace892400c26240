"""The far end of the ABI's index ranges for LD pruning: pgenhip_pair_mask / _at (the PairMaskArgs instance of gt_pair.hip) on rows of
up to 2^31 - 1 samples and into mask rows whose addresses lie past 4 GiB, and pgenhip_prune_resolve (gt_prune.hip) on those mask
strides, on many turns per block at the natural grid and on more than 2^32 rows.  The levels, keep sets and records are
test_long_rows_gpu.py's; the threshold is test_pair_mask_gpu.py's.

References: the long rows' r^2 is longrow_ref's (pair_table -> r2_of_table, exact integers rounded once) compared with the threshold
in float32; the periodic masks are prune_ref.edges / masks of one period, tiled; S is prune_ref.resolve, the sequential definition,
of the whole graph where that takes a second and of one segment of a graph made of disjoint segments where it would take minutes.
Every comparison is bit-exact.  The only tolerance is a condition on the inputs: every reference r^2 lies farther from the
threshold than the guard of prune_ref.edges (2 float32 ulps), asserted in each test, so that the device's r^2 ("within one ulp")
cannot fall on the other side.  Every mask and state array sits in a sentinel frame, mask rows have sentinel pad words, and both
must come back untouched.  A case is skipped only when the card has less free memory than the case states.
"""
import functools

import numpy as np
import pytest
import torch

import longrow_ref as LR
import pack_ref
import prune_plan as PP
import prune_ref as R
import pgen_rs_amd
from pgen_rs_amd import _capi
from longrow_ref import frame_ok, need_gib
from test_long_rows_gpu import N_MAX, N_MID, Records, kept_of
from test_pair_mask_gpu import MIN_R2
from test_prune_resolve_gpu import random_masks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_I32 = 0xA5A5A5A5 - (1 << 32)
KEEPS = ["all", "sparse", "every22"]
SHAPES = {"general": _capi.PRUNE_GENERAL, "block": _capi.PRUNE_BLOCK, "auto": _capi.PRUNE_AUTO}
CH = PP.CHUNK_ROWS
GUARD = 2.0 * float(np.spacing(np.float32(MIN_R2)))   # the band of prune_ref.edges


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def framed_words(words: int):
    """-> (sentinel buffer, front, the int32 view of ``words`` words at a 4-byte boundary)"""
    buf, front = LR.framed(4 * words, DEV, align=4)
    return buf, front, buf[front: front + 4 * words].view(torch.int32)


def framed_masks(v: int, stride: int, live: int):
    """Two framed masks of ``v`` rows of ``stride`` words: zeros in the first ``live`` words of a row, the sentinel in its pad words."""
    out = []
    for _ in range(2):
        buf, front, m = framed_words(v * stride)
        m.view(v, stride)[:, :live] = 0
        out.append((buf, front, m))
    return out


def check_masks(framed, v, stride, live, want, what, slab_rows=4096):
    """``want``: (fwd, bwd) uint32 (v, live) on the host.  Live words equal, pad words and frames still the sentinel."""
    for (buf, front, m), ref, name in zip(framed, want, ("fwd", "bwd")):
        assert frame_ok(buf, front, 4 * v * stride), f"{what}: {name} wrote outside its rows"
        rows = m.view(v, stride)
        d_ref = as_i32(ref)
        i = LR._first_diff(rows[:, :live], d_ref)
        if i is not None:
            row, word = i // live, i % live
            raise AssertionError(f"{what}: {name} row {row} word {word} (mask word {row * stride + word:#x}, byte {4 * (row * stride + word):#x}): "
                                 f"got {int(rows[row, word]) & 0xFFFFFFFF:#010x}, want {int(ref[row, word]):#010x}")
        if stride > live:
            for a in range(0, v, slab_rows):
                assert bool((rows[a: a + slab_rows, live:] == SENT_I32).all()), f"{what}: {name} pad words of rows {a}.. were written"


# ---- a. long rows in the pair-mask instantiation ---------------------------------------------------------------------------------
def near_copy(dst: torch.Tensor, src: torch.Tensor):
    """``dst`` = ``src`` with every 64th byte left as it was (random): r^2 near 1"""
    keep = dst[::64].clone()
    dst.copy_(src)
    dst[::64] = keep


def long_row_case(n, v, w, copies, keep, seed):
    """-> (records, kept list, boolean edges (v, w)): random rows, ``copies`` = {row: the row it is a near copy of}.  The r^2 of every
    pair is the exact one of longrow_ref; near copies must lie well above the threshold, random pairs well below."""
    kept = kept_of(n, keep)
    recs = Records(n, v, seed)
    for dst, src in copies.items():
        near_copy(recs.rec(dst), recs.rec(src))
    d_kept = LR.as_kept(kept, DEV)
    e = np.zeros((v, w), dtype=bool)
    m = np.float32(MIN_R2)
    for i in range(v):
        for d in range(1, w + 1):
            if i + d < v:
                r2 = LR.r2_of_table(LR.pair_table(recs.rec(i), recs.rec(i + d), n, d_kept))
                assert abs(float(r2) - float(m)) > GUARD, f"pair ({i}, {i + d}): r^2 {r2!r} is within the guard of {m!r}"
                assert (r2 > 0.8) if copies.get(i + d) == i else (r2 < 0.01), f"pair ({i}, {i + d}): r^2 {r2!r}"
                e[i, d - 1] = r2 > m
    assert e.sum() == len(copies)
    return recs, kept, e


def run_long_rows(n, v, w, copies, keep, seed, entries=("pair_mask", "pair_mask_at")):
    recs, kept, e = long_row_case(n, v, w, copies, keep, seed)
    words = R.mask_words(w)
    stride = words + 1
    want = R.masks(e)
    offs = torch.tensor([recs.off(j) for j in range(v)], dtype=torch.int64, device=DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for entry in entries:
            fm = framed_masks(v, stride, words)
            kw = dict(window=w, min_r2=MIN_R2, fwd=fm[0][2], bwd=fm[1][2], mask_stride=stride)
            if entry == "pair_mask":
                eng.pair_mask(recs.buf, recs.stride, n_variants=v, records_offset=1, **kw)
            else:
                eng.pair_mask_at(recs.buf, offs, v, **kw)
            eng.wait()
            check_masks(fm, v, stride, words, want, f"{entry} N={n} V={v} W={w} {keep}")
            del fm
    del recs


@pytest.mark.parametrize("keep", KEEPS)
def test_pair_mask_n_mid(keep):
    """N_MID, V = 6, W = 5 (all fifteen pairs), pair_mask and pair_mask_at: rows 3 and 5 are near copies of rows 0 and 4, so two bits of
    each mask are set and thirteen pairs are not edges.  Needs 1 GiB."""
    need_gib(1)
    run_long_rows(N_MID, 6, 5, {3: 0, 5: 4}, keep, 400 + len(keep))


def test_pair_mask_n_max():
    """N_MAX, all samples, V = 3, W = 2: row 2 is a near copy of row 0.  A launch walks a pair's 2^31 samples in a single wave and
    takes about 16 s whatever V is, as in test_long_rows_tables_gpu.py's test_pair_stats: one launch, through pair_mask (the two
    entries differ in where a row's address comes from, which N_MID covers).  Needs 2 GiB."""
    need_gib(2)
    run_long_rows(N_MAX, 3, 2, {2: 0}, "all", 410, entries=("pair_mask",))


# ---- b. mask rows past 4 GiB -------------------------------------------------------------------------------------------------------
P = LR.PERIOD
V_FAR, W_FAR, N_FAR = 65_539, 33, 300
# words per mask row: with 16 385, row 65 536 of a mask starts past byte 2^32; with 65 537 its word index passes 2^32 as well
STRIDES = {"bytes-past-2^32": 16_385, "words-past-2^32": 65_537}
GIB_FAR = {"bytes-past-2^32": 9, "words-past-2^32": 34}


@functools.lru_cache(maxsize=2)
def periodic_mask_case(v: int = V_FAR):
    """numpy only (tests/test_prune.py runs it: the guard holds, and at a small ``v`` the tiling equals prune_ref on all rows): 45 LD
    rows of 300 samples, three of them near copies of the row 33 places before, so that bit 32 (the second word) is set in some
    rows; selected row j is pool row j mod 45.  -> (pool records (45, R), expected fwd and bwd live words (v, 2) uint32, all three
    read-only, the pool's codes (45, 300)); the words are prune_ref.edges and masks of 45 + 33 periodic rows, tiled (forward rows by j mod 45, backward rows from row 33 on likewise), the
    last 33 forward rows clipped to the pairs that exist."""
    w = W_FAR
    rng = np.random.default_rng(451)
    codes = R.ld_codes(rng, P, N_FAR, redraw=0.12, fresh_every=11)
    for r in (7, 9, 11):
        pick = rng.random(N_FAR) < 0.05
        codes[r + w] = np.where(pick, rng.integers(0, 3, size=N_FAR), codes[r])
    codes78 = codes[np.arange(P + w) % P]
    e = R.edges(codes78, P + w, w, MIN_R2)                      # (raises where an r^2 is within the guard of the threshold)
    exists = (np.arange(P + w)[:, None] + np.arange(1, w + 1)[None, :]) < P + w
    assert e[:P].sum() > 100 and (~e & exists)[:P].sum() > 100 and e[:P, 32].sum() >= 3
    f78, b78 = R.masks(e)
    rows = np.arange(v)
    fwd = f78[rows % P]                                          # rows 0 .. 44 of the 78 have all their 33 partners
    bwd = np.where((rows < w)[:, None], b78[np.minimum(rows, w)], b78[w + (rows - w) % P])
    for i in range(max(v - w, 0), v):                            # bit d - 1 exists iff i + d < v
        live = (1 << (v - 1 - i)) - 1
        fwd[i, 0] &= np.uint32(live & 0xFFFFFFFF)
        fwd[i, 1] &= np.uint32(live >> 32)
    recs = pack_ref.pack_codes(codes.astype(np.uint8))
    for a in (recs, fwd, bwd):
        a.setflags(write=False)
    return recs, fwd, bwd, codes


@functools.lru_cache(maxsize=1)
def far_priorities_and_states():
    """-> (priorities of period 45 x 7, prune_ref.resolve of the V_FAR rows of periodic_mask_case under them)"""
    _, fwd, bwd, _ = periodic_mask_case()
    prio = np.random.default_rng(315).integers(0, 1 << 32, size=P * 7, dtype=np.uint64).astype(np.uint32)[np.arange(V_FAR) % (P * 7)]
    return prio, R.resolve(fwd, bwd, W_FAR, prio)


def pool_on_device(recs: np.ndarray, v: int):
    """-> (base, int64 offsets of the v selected rows): pool row k at byte 3 + k * (R + 2)"""
    p, r = recs.shape
    base = np.full(3 + p * (r + 2) + 16, 0xFF, dtype=np.uint8)
    for k in range(p):
        base[3 + k * (r + 2): 3 + k * (r + 2) + r] = recs[k]
    offs = torch.from_numpy(3 + np.arange(p, dtype=np.int64) * (r + 2)).to(DEV)
    return torch.from_numpy(base).to(DEV), offs[torch.arange(v, device=DEV) % p].contiguous()


@pytest.mark.parametrize("calls", ["whole", "two-calls"])
@pytest.mark.parametrize("stride", list(STRIDES), ids=list(STRIDES))
def test_pair_mask_rows_past_4_gib(stride, calls):
    """pair_mask_at on V = 65 539 rows of N = 300, W = 33 (two live words), mask_stride = 16 385 words (row 65 536 of each mask starts
    past 4 GiB) and 65 537 words (its word index i * mask_stride passes 2^32 too).  Whole, and as two calls whose n_left blocks meet
    at row 65 536 - 7 (the first takes the rows behind its block as partners, all 10 of them; both only OR bits in).  Live words against the tiled
    reference on the device; every pad word and both frames must still be the sentinel.  Needs 9 GiB / 34 GiB."""
    need_gib(GIB_FAR[stride])
    key, stride = stride, STRIDES[stride]
    v, w = V_FAR, W_FAR
    assert 4 * 65_536 * stride > 1 << 32 and (key != "words-past-2^32" or 65_536 * stride > 1 << 32)
    recs, fwd, bwd, _ = periodic_mask_case()
    base, offs = pool_on_device(recs, v)
    fm = framed_masks(v, stride, 2)
    f, b = fm[0][2].view(v, stride), fm[1][2].view(v, stride)
    with pgen_rs_amd.GtEngine(N_FAR, device=0) as eng:
        kw = dict(window=w, min_r2=MIN_R2, mask_stride=stride)
        if calls == "whole":
            eng.pair_mask_at(base, offs, v, fwd=f, bwd=b, **kw)
        else:
            s = 65_536 - 7
            eng.pair_mask_at(base, offs, min(s + w, v), n_left=s, fwd=f, bwd=b, **kw)
            eng.pair_mask_at(base, offs[s:], v - s, fwd=f[s:], bwd=b[s:], **kw)
        eng.wait()
    check_masks(fm, v, stride, 2, (fwd, bwd), f"pair_mask_at V={v} W={w} stride {stride} {calls}")
    del fm


# ---- the host loop of prune_resolve, every call watched on the device ------------------------------------------------------------------
def count_zero(state: torch.Tensor, slab: int = 1 << 30) -> int:
    return sum(int((state[a: a + slab] == 0).sum()) for a in range(0, state.numel(), slab))


def resolve_watched(eng, d_f, d_b, stride, w, n_rows, d_prio, d_want, shape, max_calls, what, blocks=0):
    """Runs the host loop on zeroed, framed states.  After every call: the counter equals the number of zero bytes, and (with
    ``d_want``, the expected states on the device) no decided state changed and no state other than S was written; every call but
    the last decides something.  ``blocks``: a forced grid (PGENHIP_KNOB_PRUNE_BLOCKS).  -> (framed buffer, the states, calls)"""
    buf, front = LR.framed(n_rows, DEV)
    state = buf[front: front + n_rows]
    state.zero_()
    seen = {"prev": state.clone() if d_want is not None else None, "left": n_rows}

    def watch(calls, left):
        assert frame_ok(buf, front, n_rows), f"{what} call {calls}: a byte outside the states was written"
        zeros = count_zero(state)
        assert left == zeros, f"{what} call {calls}: counter {left}, undecided bytes {zeros}"
        assert left < seen["left"] or left == 0, f"{what} call {calls} decided nothing"
        seen["left"] = left
        if d_want is not None:
            prev = seen["prev"]
            assert not bool(((prev != 0) & (state != prev)).any()), f"{what} call {calls} changed a decided state"
            wrong = (state != 0) & (state != d_want)
            if bool(wrong.any()):
                row = int(torch.nonzero(wrong)[0, 0])
                raise AssertionError(f"{what} call {calls}: row {row} = {row:#x} got state {int(state[row])}, S has {int(d_want[row])}")
            prev.copy_(state)

    eng.tune(_capi.KNOB_PRUNE_BLOCKS, blocks)
    try:
        got, calls = eng.prune_resolve(d_f, d_b, w, priority=d_prio, state=state, shape=SHAPES[shape], max_calls=max_calls, n_rows=n_rows,
                                       mask_stride=stride, on_call=watch)
    finally:
        eng.tune(_capi.KNOB_PRUNE_BLOCKS, 0)
    assert got is state
    return buf, state, calls


def as_i32(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to(DEV)   # (a copy: the cached cases are read-only)


# ---- c. prune resolve on those strides ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", list(STRIDES), ids=list(STRIDES))
def test_prune_resolve_on_far_mask_rows(stride):
    """GENERAL, BLOCK and AUTO at the natural grid on the masks (b) must produce (the reference's words, written at the same stride
    into framed masks with sentinel pad words), priorities of period 45 x 7, against prune_ref.resolve of all 65 539 rows.  `row = mask + v * a.mask_stride` in
    gt_prune.hip's decide reaches byte addresses past 2^32 with 16 385 words per row and word indices past 2^32 with 65 537.
    Needs 9 GiB / 34 GiB."""
    need_gib(GIB_FAR[stride])
    stride = STRIDES[stride]
    v, w = V_FAR, W_FAR
    _, fwd, bwd, _ = periodic_mask_case()
    fm = framed_masks(v, stride, 2)
    for (_, _, m), ref in zip(fm, (fwd, bwd)):
        m.view(v, stride)[:, :2] = as_i32(ref)
    prio, want = far_priorities_and_states()
    assert (want == R.KEPT).sum() > 1000 and (want == R.REMOVED).sum() > 1000
    d_want, d_prio = torch.from_numpy(want).to(DEV), as_i32(prio)
    with pgen_rs_amd.GtEngine(8, device=0) as eng:
        for shape in SHAPES:
            what = f"prune_resolve V={v} W={w} stride {stride} {shape}"
            buf, state, _ = resolve_watched(eng, fm[0][2], fm[1][2], stride, w, v, d_prio, d_want, shape, v, what)
            assert bool((state == d_want).all()), what
            del buf, state
    check_masks(fm, v, stride, 2, (fwd, bwd), "prune_resolve left the masks as they were")
    del fm


# ---- segments: graphs whose S is the S of one segment, tiled ---------------------------------------------------------------------------
def segment_graph(seed, length, w, density, v, prio_values):
    """A graph of ``v`` rows made of disjoint copies of one random segment of ``length`` rows (edges up to distance ``w`` inside the
    segment only); the last v % length rows are a truncated segment whose forward bits past the end stay in as strays.  Priorities
    (``prio_values`` > 0: random below it, of period ``length``; 0: none) repeat with the segment, so S does too.
    -> (fwd, bwd of one segment (length, words) uint32, priorities of one segment or None, S of a whole segment, S of the truncated one)"""
    fwd, bwd = random_masks(seed, length, w, density, stray=False)
    rng = np.random.default_rng(seed + 1)
    prio = rng.integers(0, prio_values, size=length).astype(np.uint32) if prio_values else None
    tail = v % length
    s_whole = R.resolve(fwd, bwd, w, prio)
    s_tail = R.resolve(fwd[:tail], bwd[:tail], w, None if prio is None else prio[:tail]) if tail else np.zeros(0, np.uint8)
    assert (s_whole == R.KEPT).sum() > length // 8 and (s_whole == R.REMOVED).sum() > length // 8
    return fwd, bwd, prio, s_whole, s_tail


def check_tiled_states(state, s_whole, s_tail, what, slab=1 << 23):
    length = len(s_whole)
    whole = state.numel() // length
    d_s = torch.from_numpy(s_whole).to(DEV)
    got = state[: whole * length].view(whole, length)
    for a in range(0, whole, slab):
        i = LR._first_diff(got[a: a + slab], d_s[None, :].expand(min(slab, whole - a), length))
        if i is not None:
            row = a * length + i
            raise AssertionError(f"{what}: row {row} = {row:#x} (row {row % length} of its segment) got state {int(state[row])}, "
                                 f"S has {int(s_whole[row % length])}")
    i = LR._first_diff(state[whole * length:], torch.from_numpy(s_tail).to(DEV))
    assert i is None, f"{what}: row {whole * length + i} (row {i} of the truncated segment) got state {int(state[whole * length + i])}, S has {int(s_tail[i])}"


# ---- d. many turns per block ------------------------------------------------------------------------------------------------------------
W_TURNS, SEGMENT_TURNS = 40, 1543


def many_turns_case(v: int):
    """numpy only (tests/test_prune.py resolves a small ``v`` of it row by row).  -> (fwd, bwd (v, 2) uint32, priorities, S of a whole
    segment, S of the truncated one): segment_graph at window 40 and density 8 / W with priorities in [0, 3), plus the strays."""
    w, length = W_TURNS, SEGMENT_TURNS
    fwd, bwd, prio, s_whole, s_tail = segment_graph(40, length, w, 8.0 / w, v, 3)
    rng = np.random.default_rng(41)
    rows = np.arange(v) % length
    f, b, p = fwd[rows], bwd[rows], prio[rows]
    high = np.uint32((0xFFFFFFFF << (w % 32)) & 0xFFFFFFFF)
    pick = rng.random(v) < 0.3
    f[pick, 1] |= high
    b[pick, 1] |= high
    for r in range(w):                                           # the strays at both ends, half of the bits each
        for d in range(r + 1, w + 1):                            # row r - d and row v - 1 - r + d do not exist
            if rng.random() < 0.5:
                b[r, (d - 1) // 32] |= np.uint32(1 << ((d - 1) % 32))
            if rng.random() < 0.5:
                f[v - 1 - r, (d - 1) // 32] |= np.uint32(1 << ((d - 1) % 32))
    return f, b, p, s_whole, s_tail


@pytest.mark.parametrize("shape", list(SHAPES))
def test_prune_resolve_many_turns_per_block(shape):
    """V = 8 * num_cus * CHUNK_ROWS * 3 + 517 rows at the natural grid of 8 * num_cus blocks: every block owns three full turns and a
    short one, the last block is short.  Window 40, density 8 / W, priorities in [0, 3), stray bits as test_prune_resolve_gpu's
    random_masks plants them (bits >= W in the last word on a third of the rows, backward bits of the first rows that point in
    front of row 0, forward bits of the last rows that point past the end).  The sequential reference takes minutes on 6.3 million
    random rows, so the graph is disjoint copies of one random 1 543-row segment (1 543 is prime: the segments straddle every turn
    and range boundary at another row) and S is prune_ref.resolve of one segment, tiled; every call is checked against it.
    Needs 1 GiB."""
    need_gib(1)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    w, length = W_TURNS, SEGMENT_TURNS
    v = PP.BLOCKS_PER_CU * num_cus * CH * 3 + 517
    range_rows, grid = PP.block_plan(v, num_cus, 0)
    assert grid == PP.BLOCKS_PER_CU * num_cus and 3 * CH < range_rows <= 4 * CH and 0 < v - (grid - 1) * range_rows < range_rows
    f, b, p, s_whole, s_tail = many_turns_case(v)
    d_want = torch.from_numpy(np.concatenate([np.tile(s_whole, v // length), s_tail])).to(DEV)
    with pgen_rs_amd.GtEngine(8, device=0) as eng:
        what = f"prune_resolve V={v} W={w} {shape}"
        buf, state, calls = resolve_watched(eng, as_i32(f), as_i32(b), 2, w, v, as_i32(p), d_want, shape, length, what)
        check_tiled_states(state, s_whole, s_tail, what)
    del buf, state


# ---- e. row indices past 2^32 -------------------------------------------------------------------------------------------------------------
ROWS_PAST = [("general", "by-index", 0), ("general", "priorities", 0), ("block", "by-index", 0), ("block", "priorities", 0),
             ("block", "by-index", 65_537)]


@pytest.mark.parametrize("shape,priorities,blocks", ROWS_PAST, ids=[f"{s}-{p}" + (f"-{b}-blocks" if b else "") for s, p, b in ROWS_PAST])
def test_prune_resolve_rows_past_2_32(shape, priorities, blocks):
    """n_rows = 2^32 + 77, window 32, mask_stride 1: disjoint copies of a random 90-row segment (density 0.1; 90 does not divide 1 024
    or a block's range, so segments straddle turn and range boundaries, and 2^32 = 76 mod 90, so a row index cut to 32 bits lands on
    another row of the segment); the last 63 rows are a truncated segment with its forward bits left in.  Without priorities and
    with priorities of period 90.  At the natural grid (8 blocks per CU: BLOCK's ranges are of about 2^21 rows, so the last block's
    turns and rows pass 2^32 but its first row, `begin` = blockIdx.x * range_rows, does not), and BLOCK once more on a grid forced to
    65 537 blocks: ranges of 65 536 rows, so the last block begins at row 2^32 exactly and owns the 77 rows behind it (a `begin`
    cut to 32 bits sends it to rows 0 .. 65 535 and leaves the 77 undecided).  The counter is checked against the zero bytes after
    every call, the final states against prune_ref.resolve of one segment, tiled, as a (-1, 90) view on the device.
    Needs 38 GiB, 54 GiB with priorities."""
    need_gib(54 if priorities == "priorities" else 38)
    n_rows, w, length = (1 << 32) + 77, 32, 90
    if blocks:
        num_cus = torch.cuda.get_device_properties(0).multi_processor_count
        range_rows, grid = PP.block_plan(n_rows, num_cus, blocks)
        assert (range_rows, grid) == (65_536, 65_537) and (grid - 1) * range_rows == 1 << 32
    fwd, bwd, prio, s_whole, s_tail = segment_graph(90, length, w, 0.1, n_rows, (1 << 32) if priorities == "priorities" else 0)
    assert len(s_tail) == n_rows % length == 63 and (1 << 32) % length == 76
    d_f = torch.empty(n_rows, dtype=torch.int32, device=DEV)
    d_b = torch.empty(n_rows, dtype=torch.int32, device=DEV)
    LR.fill_periodic(d_f, as_i32(fwd[:, 0]))
    LR.fill_periodic(d_b, as_i32(bwd[:, 0]))
    d_p = None
    if prio is not None:
        d_p = torch.empty(n_rows, dtype=torch.int32, device=DEV)
        LR.fill_periodic(d_p, as_i32(prio))
    with pgen_rs_amd.GtEngine(8, device=0) as eng:
        what = f"prune_resolve n_rows=2^32+77 {shape} {priorities}" + (f" {blocks} blocks" if blocks else "")
        buf, state, calls = resolve_watched(eng, d_f, d_b, 1, w, n_rows, d_p, None, shape, 90, what, blocks)
        check_tiled_states(state, s_whole, s_tail, what)
    del buf, state, d_f, d_b, d_p
