"""Per-sample genotype counts — GPU leg on data that fills the bit-sliced counters of gt_scount.hip.  A counter holds 2 047 rows
in planes ones / twos / fours and eight hi planes, is flushed every 255 batches of 8 rows, and the flush reads only the hi
planes the batch count can have set (scount_plan.py: counter_capacity, hi_planes).  HWE and uniform records never come near a
full counter, so these rows do: one row repeated, constant rows, one hot slot, a staircase of exact counts.  Every input is
valid data; the reference is numpy on the host records (np_scounts), compared for integer equality."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import scount_plan as SP
from pgen_rs_amd import _capi
from test_sample_counts_gpu import DEV, KERNELS, SENT, host, kept_sets, np_scounts, rsize, run_scounts

pytestmark = pytest.mark.gpu

# one N per lanes-per-row class that changes how a window fills: N -> rows a block has side by side (slots)
SHAPES = {33: 64, 300: 32, 2504: 4, 5000: 4}   # G = 4; G = 8; G = 64 in one tile with cols < G; two column tiles
KEEPS = ["all", "p50"]
# hi == b after step * b rows of one category: both sides of every step of n_hi, and the last two batches of a window
PLANE_EDGES = [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 254, 255]
FILLS = {0x55: 1, 0xAA: 2, 0xFF: 3, 0x00: 0}   # a record byte repeated -> the one code every sample has


def test_shapes_cover_the_classes():
    assert {n: SP.slots(n) for n in SHAPES} == SHAPES
    assert [SP.lanes_per_row(n) for n in SHAPES] == [4, 8, 64, 64]
    assert [SP.tiles(n) for n in SHAPES] == [1, 1, 1, 2] and SP.columns(2504) < 64
    assert SP.BATCH * max(PLANE_EDGES) == SP.BATCH * SP.WINDOW_BATCHES <= SP.counter_capacity()
    assert sorted({SP.hi_planes(b) for b in PLANE_EDGES}) == list(range(1, SP.HI_BITS + 1))


def step_rows(n, slices):
    """Rows that give every slot of every slice one batch."""
    return slices * SP.slots(n) * SP.BATCH


def one_row(n, rng):
    """A random record at byte 3 of a random buffer, its pad bits set; (buffer, the record)."""
    r = rsize(n)
    raw = rng.integers(0, 256, size=3 + r + 16, dtype=np.uint8)
    if n % 4:
        raw[3 + r - 1] |= (0xFF << (2 * (n % 4))) & 0xFF
    row = raw[3: 3 + r].copy()
    # every category has a sample, so the L, H and M counters of some lane each take every row
    assert (np_scounts(row[None, :], n).sum(axis=0) > 0).all()
    return raw, row


def closed_form(k, v, code):
    want = np.zeros((k, 4), dtype=np.int64)
    want[:, code] = v
    return want


def pack(codes, pad_code=3):
    """(V, N) codes -> (V, R) records; the pad samples of the last byte get ``pad_code``."""
    v, n = codes.shape
    c = np.full((v, 4 * rsize(n)), pad_code, dtype=np.uint8)
    c[:, :n] = codes
    c = c.reshape(v, -1, 4)
    return c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)


# a. one row repeated V times through variant_idx and through byte offsets: every sample gets V hits in one category
@pytest.mark.parametrize("n", list(SHAPES))
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("slices", [1, 3])
def test_plane_edges_on_one_repeated_row(n, keep, slices):
    rng = np.random.default_rng(1000 * n + 10 * slices + len(keep))
    kept = kept_sets(n, rng)[keep]
    raw, row = one_row(n, rng)
    w, step = SP.window_rows(n, slices), step_rows(n, slices)
    assert step * SP.WINDOW_BATCHES == w
    vs = sorted({step * b for b in PLANE_EDGES} | {w - 1, w, w + 1, w + step, 2 * w, 2 * w + slices, 3 * w + 5})
    base = np_scounts(row[None, :], n, kept)
    assert set(np.unique(base)) == {0, 1} and (base.sum(axis=1) == 1).all()
    d_raw = torch.from_numpy(raw).to(DEV)
    d_idx = torch.zeros(vs[-1], dtype=torch.int32, device=DEV)
    d_off = torch.full((vs[-1],), 3, dtype=torch.int64, device=DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, slices)
        for v in vs:
            for kern in KERNELS:
                got = run_scounts(eng, kern, records=d_raw, records_offset=3, variant_idx=d_idx, n_variants=v)
                assert (got == base * v).all(), f"variant_idx, V = {v}, shape {kern}"
                got = run_scounts(eng, kern, base=d_raw, record_off=d_off, n_variants=v)
                assert (got == base * v).all(), f"_at, V = {v}, shape {kern}"


# b. real rows, every byte the same: a full window, one batch more and a ragged tail (one slice, so the rows stay under 10 MB)
@pytest.mark.parametrize("n", list(SHAPES))
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("fill", list(FILLS))
def test_dense_constant_rows(n, keep, fill):
    rng = np.random.default_rng(2000 * n + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    v = SP.window_rows(n, 1) + step_rows(n, 1) + 3
    recs = np.full((v, r), fill, dtype=np.uint8)
    want = np_scounts(recs, n, kept)
    k = n if kept is None else len(kept)
    assert (want == closed_form(k, v, FILLS[fill])).all()   # (with 0xFF the pad bits are set: not counted)
    # the same rows at stride R + 5 from byte 3, the bytes between them the opposite pattern
    stride = r + 5
    raw = np.full(3 + v * stride, fill ^ 0xFF, dtype=np.uint8)
    raw[3:].reshape(v, stride)[:, :r] = fill
    d_recs = torch.from_numpy(recs.reshape(-1)).to(DEV)
    d_raw = torch.from_numpy(raw).to(DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, 1)
        for kern in KERNELS:
            got = run_scounts(eng, kern, records=d_recs, n_variants=v)
            assert (got == want).all(), f"dense, shape {kern}"
            got = run_scounts(eng, kern, records=d_raw, record_stride=stride, records_offset=3, n_variants=v)
            assert (got == want).all(), f"strided, shape {kern}"


# c. the rows of one slot all missing, the others hom-ref: one slot's counters fill (L == H == M, so the het and hom-alt adds are
# skipped and M's upper planes carry the result), the other slots' stay empty
@pytest.mark.parametrize("n", list(SHAPES))
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("last_slot", [False, True])
def test_one_hot_slot(n, keep, last_slot):
    rng = np.random.default_rng(3000 * n + len(keep))
    kept = kept_sets(n, rng)[keep]
    r, slots = rsize(n), SP.slots(n)
    s = slots - 1 if last_slot else 0
    v = SP.window_rows(n, 1) + step_rows(n, 1)
    recs = np.zeros((v, r), dtype=np.uint8)
    recs[s::slots] = 0xFF
    want = np_scounts(recs, n, kept)
    assert (want[:, 3] == v // slots).all() and (want[:, 0] == v - v // slots).all()
    assert v // slots == SP.BATCH * (SP.WINDOW_BATCHES + 1)   # the slot's first window is full
    d_recs = torch.from_numpy(recs.reshape(-1)).to(DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, 1)
        for kern in KERNELS:
            got = run_scounts(eng, kern, records=d_recs, n_variants=v)
            assert (got == want).all(), f"slot {s}, shape {kern}"


# d. sample s missing in rows [0, t_s), het in [t_s, u_s), hom-ref after: a different exact count per sample, full and empty
# counters in neighbouring bits of one plane word
@pytest.mark.parametrize("n", list(SHAPES))
@pytest.mark.parametrize("keep", KEEPS)
def test_staircase(n, keep):
    rng = np.random.default_rng(4000 * n + len(keep))
    kept = kept_sets(n, rng)[keep]
    v = SP.window_rows(n, 1) + step_rows(n, 1)
    ramp = np.round(np.linspace(0, v, n)).astype(np.int64)
    t = ramp[rng.permutation(n)]
    u = np.minimum(v, t + ramp[rng.permutation(n)])
    rows = np.arange(v, dtype=np.int64)[:, None]
    codes = (rows < u[None, :]).astype(np.uint8) + 2 * (rows < t[None, :]).astype(np.uint8)   # t <= u: 3, then 1, then 0
    recs = pack(codes)
    want = np_scounts(recs, n, kept)
    full = np_scounts(recs, n)
    assert (full[:, 3] == t).all() and (full[:, 1] == u - t).all()
    assert len(set(t.tolist())) == n and t.min() == 0 and t.max() == v
    d_recs = torch.from_numpy(recs.reshape(-1)).to(DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, 1)
        for kern in KERNELS:
            got = run_scounts(eng, kern, records=d_recs, n_variants=v)
            assert (got == want).all(), f"shape {kern}"


def run_accumulating(eng, kern, prefill, plain_first, **kw):
    """run_scounts for ACCUMULATE: the counts start at ``prefill`` (or at what a plain call of the same rows leaves) inside the
    sentinel-guarded buffer, then one accumulating call adds to them."""
    k = eng.kept_count
    got = None
    for lead in (1, 4):
        buf = torch.full((lead + 4 * k + 8,), SENT, dtype=torch.int32, device=DEV)
        out = buf[lead:]
        if plain_first:
            eng.sample_counts(out=out, kernel=kern, **kw)
        else:
            buf[lead: lead + 4 * k] = prefill - (1 << 32) if prefill >= 1 << 31 else prefill
        res = eng.sample_counts(out=out, kernel=kern, accumulate=True, **kw)
        eng.wait()
        h = buf.cpu().numpy()
        assert (h[:lead] == SENT).all() and (h[lead + 4 * k:] == SENT).all(), f"shape {kern} wrote outside its counts"
        assert res.shape == (k, 4) and res.dtype == torch.int32
        g = host(res)
        assert got is None or (g == got).all()
        got = g
    return got


# e. ACCUMULATE adds u32 modular sums to what the buffer holds
@pytest.mark.parametrize("n", list(SHAPES))
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("slices", [1, 3])
def test_accumulate_is_modular(n, keep, slices):
    rng = np.random.default_rng(5000 * n + 10 * slices + len(keep))
    kept = kept_sets(n, rng)[keep]
    raw, row = one_row(n, rng)
    w = SP.window_rows(n, slices)
    want = np_scounts(row[None, :], n, kept) * w
    d_raw = torch.from_numpy(raw).to(DEV)
    d_idx = torch.zeros(w, dtype=torch.int32, device=DEV)
    rows = dict(records=d_raw, records_offset=3, variant_idx=d_idx, n_variants=w)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, slices)
        for kern in KERNELS:
            got = run_accumulating(eng, kern, 0xFFFFFFF0, False, **rows)
            assert (got == (0xFFFFFFF0 + want) % (1 << 32)).all(), f"onto 0xFFFFFFF0, shape {kern}"
            assert (got[want > 0] == w - 16).all() and (got[want == 0] == 0xFFFFFFF0).all()
            got = run_accumulating(eng, kern, 0, True, **rows)
            assert (got == 2 * want).all() and (got.max(axis=1) == 2 * w).all(), f"plain then accumulate, shape {kern}"
