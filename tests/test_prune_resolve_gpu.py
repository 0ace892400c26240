"""Greedy independent set of a pair mask — GPU leg (pgenhip_prune_resolve through GtEngine.prune_resolve), masks fed directly:
GENERAL, BLOCK and AUTO against the sequential definition (tests/prune_ref.py) on random masks at every edge of plan::prune's
ranges and turns, with every kind of priority, pre-set states and bits that point outside the rows; what every single call
guarantees (the exact undecided count, no state ever changed or wrong); chains; framing and the refusals."""
import numpy as np
import pytest
import torch

import prune_plan as PP
import prune_ref as R
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [_capi.PRUNE_GENERAL, _capi.PRUNE_BLOCK, _capi.PRUNE_AUTO]
CH = PP.CHUNK_ROWS


def random_masks(seed, v, w, density, stray=True):
    """(fwd, bwd) of a random graph with edges up to distance w, plus (``stray``) bits that no row answers: fwd bits of the last
    rows that point past the end, bwd bits of the first rows that point before row 0, bits >= w in the last word."""
    rng = np.random.default_rng(seed)
    e = rng.random((v, w)) < density
    e &= (np.arange(v)[:, None] + np.arange(1, w + 1)[None, :]) < v
    fwd, bwd = R.masks(e)
    if stray:
        words = R.mask_words(w)
        tail = np.uint32((0xFFFFFFFF << (w % 32)) & 0xFFFFFFFF) if w % 32 else np.uint32(0)
        for r in range(v):
            if r + w >= v:     # bit d - 1 with r + d >= v
                for d in range(max(v - r, 1), w + 1):
                    if rng.random() < 0.5:
                        fwd[r, (d - 1) // 32] |= np.uint32(1 << ((d - 1) % 32))
            if r < w:          # bit d - 1 with r - d < 0
                for d in range(r + 1, w + 1):
                    if rng.random() < 0.5:
                        bwd[r, (d - 1) // 32] |= np.uint32(1 << ((d - 1) % 32))
            if rng.random() < 0.3:
                fwd[r, words - 1] |= tail
                bwd[r, words - 1] |= tail
    return fwd, bwd


def chain_masks(v):
    e = np.zeros((v, 1), dtype=bool)
    e[: v - 1, 0] = True
    return R.masks(e)


def run(eng, fwd, bwd, w, priority, state0, shape, blocks=0, max_calls=None):
    """The host loop with every call watched: returns (final state, calls).  The state bytes sit between sentinel bytes."""
    v = fwd.shape[0]
    want = R.resolve(fwd, bwd, w, priority, state0)
    d_f = torch.from_numpy(fwd.view(np.int32).copy()).to(DEV)
    d_b = torch.from_numpy(bwd.view(np.int32).copy()).to(DEV)
    d_p = None if priority is None else torch.from_numpy(np.asarray(priority, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    raw = torch.full((v + 19,), 0xA5, dtype=torch.uint8, device=DEV)
    state = raw[3: 3 + v]
    state.copy_(torch.from_numpy(np.zeros(v, np.uint8) if state0 is None else np.asarray(state0, dtype=np.uint8)))
    seen = {"prev": state.cpu().numpy().copy(), "left": None}

    def watch(calls, left):
        h = raw.cpu().numpy()
        assert (h[:3] == 0xA5).all() and (h[3 + v:] == 0xA5).all(), "a byte outside the states was written"
        s = h[3: 3 + v]
        assert left == int((s == 0).sum()), f"call {calls}: counter {left}, undecided bytes {int((s == 0).sum())}"
        prev = seen["prev"]
        assert (s[prev != 0] == prev[prev != 0]).all(), f"call {calls} changed a decided state"
        assert (s[s != 0] == want[s != 0]).all(), f"call {calls} wrote a state that is not S"
        assert left < int((prev == 0).sum()) or left == 0, f"call {calls} decided nothing"
        seen["prev"] = s.copy()

    eng.tune(_capi.KNOB_PRUNE_BLOCKS, blocks)
    try:
        got, calls = eng.prune_resolve(d_f, d_b, w, priority=d_p, state=state, shape=shape, max_calls=max_calls or max(v, 1), on_call=watch)
    finally:
        eng.tune(_capi.KNOB_PRUNE_BLOCKS, 0)
    assert got is state and (seen["prev"] == want).all()
    return seen["prev"], calls


@pytest.fixture(scope="module")
def eng():
    with pgen_rs_amd.GtEngine(8, device=0) as e:
        yield e


# V on both sides of every first row of a turn (tests/prune_plan.py, turn_edges) with the grid forced to 1, 2 and 3, and V = 1
SIZES = [(1, 0)] + [(g * CH + dv, g) for g in (1, 2, 3) for dv in (-1, 0, 1)]


@pytest.mark.parametrize("v,blocks", SIZES)
@pytest.mark.parametrize("w", [1, 32, 33, 200])
def test_random_masks_at_every_range_edge(eng, v, blocks, w):
    if blocks:
        assert PP.block_plan(v, 256, blocks)[0] in (CH - 1, CH, CH + 1)
    seed = v * 7 + w
    density = (0.02, 0.3)[seed % 2] * min(1.0, 8.0 / w) if w > 33 else (0.05, 0.6)[seed % 2]
    fwd, bwd = random_masks(seed, v, w, density)
    rng = np.random.default_rng(seed)
    priority = [None, rng.integers(0, 1 << 32, size=v, dtype=np.uint64).astype(np.uint32), rng.integers(0, 3, size=v).astype(np.uint32),
                np.full(v, 7, dtype=np.uint32)][seed % 4]
    finals = [run(eng, fwd, bwd, w, priority, None, shape, blocks)[0] for shape in SHAPES]
    assert (finals[0] == finals[1]).all() and (finals[0] == finals[2]).all()
    if v > 1 and w <= 33:
        assert (finals[0] == R.KEPT).any() and (finals[0] == R.REMOVED).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_window_wider_than_a_range_and_than_the_halo(eng, shape):
    fwd, bwd = random_masks(11, 50, 40, 0.1)
    run(eng, fwd, bwd, 40, None, None, shape, blocks=3)                        # ranges of 17 rows, neighbours 40 rows away
    w = PP.HALO_ROWS + 90
    fwd, bwd = random_masks(12, CH + 700, w, 0.004)
    prio = np.random.default_rng(12).integers(0, 1 << 20, size=CH + 700).astype(np.uint32)
    run(eng, fwd, bwd, w, prio, None, shape, blocks=1)                         # neighbours beyond the staged halo, two turns
    run(eng, fwd, bwd, w, prio, None, shape, blocks=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_pre_set_states_stay_and_count(eng, shape):
    v, w = 700, 9
    fwd, bwd = random_masks(21, v, w, 0.25)
    rng = np.random.default_rng(21)
    state0 = rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), size=v)
    prio = rng.integers(0, 50, size=v).astype(np.uint32)
    got, _ = run(eng, fwd, bwd, w, prio, state0, shape, blocks=2)
    assert (got[state0 != 0] == state0[state0 != 0]).all()
    done = R.resolve(fwd, bwd, w, prio, None)
    _, calls = run(eng, fwd, bwd, w, prio, done, shape)                        # nothing undecided: one call, counter 0
    assert calls == 1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("order", ["descending", "ascending", "index"])
def test_chain_across_three_ranges(eng, shape, order):
    """A fully connected chain: every row waits for its neighbour.  S alternates from the end that beats."""
    v = 300
    fwd, bwd = chain_masks(v)
    prio = {"descending": np.arange(v, 0, -1), "ascending": np.arange(1, v + 1), "index": None}[order]
    prio = None if prio is None else prio.astype(np.uint32)
    got, calls = run(eng, fwd, bwd, 1, prio, None, shape, blocks=3)
    first = np.arange(v) % 2 == 0 if order != "ascending" else (v - 1 - np.arange(v)) % 2 == 0
    assert (got == np.where(first, R.KEPT, R.REMOVED)).all()
    assert calls <= v
    if shape == _capi.PRUNE_BLOCK:
        assert calls <= 3          # call k finishes range k: what beats its rows from outside was decided by the call before


def test_chain_inside_one_range_ends_within_two_block_calls(eng):
    v = 500
    fwd, bwd = chain_masks(v)
    for prio in (None, np.arange(v, 0, -1).astype(np.uint32), np.arange(1, v + 1).astype(np.uint32)):
        _, calls = run(eng, fwd, bwd, 1, prio, None, _capi.PRUNE_BLOCK, blocks=1)
        assert calls <= 2


def test_wrapper_defaults_and_max_calls(eng):
    fwd, bwd = chain_masks(40)
    d_f, d_b = torch.from_numpy(fwd.view(np.int32).copy()).to(DEV), torch.from_numpy(bwd.view(np.int32).copy()).to(DEV)
    state, calls = eng.prune_resolve(d_f, d_b, 1)
    assert state.dtype == torch.uint8 and state.shape == (40,) and calls >= 1
    assert (state.cpu().numpy() == R.resolve(fwd, bwd, 1)).all()
    with pytest.raises(RuntimeError):
        eng.prune_resolve(d_f, d_b, 1, shape=_capi.PRUNE_GENERAL, max_calls=1)      # a chain of 40 links is not one GENERAL sweep
    empty = torch.zeros((0, 1), dtype=torch.int32, device=DEV)
    state, calls = eng.prune_resolve(empty, empty, 1)
    assert state.numel() == 0 and calls == 1


def test_refusals_write_nothing(eng):
    lib = _capi.lib
    B, T = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
    buf = torch.full((64,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)
    ctx, fp, bp, pp, sp, cp = eng._ctx, buf.data_ptr(), buf.data_ptr() + 64, buf.data_ptr() + 128, buf.data_ptr() + 192, buf.data_ptr() + 224
    call = lib.pgenhip_prune_resolve
    assert call(ctx, fp, bp, 1, 0, 8, pp, sp, cp, 0) == B               # window == 0
    assert call(ctx, None, bp, 1, 4, 8, pp, sp, cp, 0) == B             # NULL pointers with rows
    assert call(ctx, fp, None, 1, 4, 8, pp, sp, cp, 0) == B
    assert call(ctx, fp, bp, 1, 4, 8, pp, None, cp, 0) == B
    assert call(ctx, fp, bp, 1, 4, 8, pp, sp, None, 0) == B
    assert call(ctx, fp + 2, bp, 1, 4, 8, pp, sp, cp, 0) == B           # alignment: masks 4, priorities 4, counter 8
    assert call(ctx, fp, bp + 1, 1, 4, 8, pp, sp, cp, 0) == B
    assert call(ctx, fp, bp, 1, 4, 8, pp + 2, sp, cp, 0) == B
    assert call(ctx, fp, bp, 1, 4, 8, pp, sp, cp + 4, 0) == B
    assert call(ctx, fp, bp, 1, 33, 8, pp, sp, cp, 0) == B              # mask_stride < ceil(window / 32)
    assert call(ctx, fp, bp, 0, 4, 2, pp, sp, cp, 0) == B
    assert call(ctx, fp, bp, 1, 4, 8, pp, sp, cp, 3) == B               # unknown shape
    assert call(ctx, fp, bp, 1, 4, 8, pp, sp, cp, 0x10) == B
    assert call(ctx, fp, bp, 1 << 30, 4, 1 << 20, pp, sp, cp, 0) == T   # n_rows * mask_stride * 4 = 2^52
    assert call(ctx, fp, bp, 1, 4, 1 << 50, pp, sp, cp, 0) == T
    eng.wait()
    assert (buf.cpu().numpy() == -0x5A5A5A5B).all(), "a refused call wrote"
    # no rows: the counter becomes 0, nothing else is touched, NULL everywhere else is fine
    assert call(ctx, None, None, 0, 4, 0, None, None, cp, 0) == _capi.OK
    eng.wait()
    h = buf.cpu().numpy()
    assert (h[56:58] == 0).all() and (np.delete(h, [56, 57]) == -0x5A5A5A5B).all()
