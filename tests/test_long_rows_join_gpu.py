"""The far end of the ABI's index ranges for pgenhip_join_records (gt_join.hip): rows of up to 2^31 - 1 samples (STREAM's row-relative
int32 arithmetic meets R = 2^29), launches on both sides of 2^32 work items (where both kernels change from a 32-bit to a 64-bit
item decomposition), and source and output addresses past 4 GiB, against the slab-wise torch reference of longrow_ref.py
(check_joined, held against join_ref.join by test_longrow_ref.py) and, for the 2^32-item launches, against a 45-row pattern built
with join_ref.join.  The levels are test_long_rows_gpu.py's.

Source records are random bytes (dirty pad bits) at odd addresses; every output sits in a sentinel frame, at a byte phase, with a
padded pitch, and the frame and the padding must come back untouched.  Every comparison is bit-exact.  A case is skipped only
when the card has less free memory than the case states.
"""
import numpy as np
import pytest
import torch

import join_ref as JR
import longrow_ref as LR
import pgen_rs_amd
from pgen_rs_amd import _capi
from longrow_ref import GIB, SENT, frame_ok, need_gib
from test_long_rows_gpu import N_MAX, N_MID

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = {"general": _capi.JOIN_GENERAL, "stream": _capi.JOIN_STREAM, "auto": _capi.JOIN_AUTO}


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def framed_at(nbytes: int, phase: int):
    """-> (buffer of sentinel bytes, offset of the payload: at least LR.FRONT, at byte ``phase`` of a 16-byte line)"""
    buf, front = LR.framed(nbytes + 16, DEV)
    front += (phase - front) % 16
    assert (buf.data_ptr() + front) % 16 == phase
    return buf, front


class Part:
    """``v`` random records of ``count`` samples: row j at byte 1 + j * pitch of ``buf``, the pitch even, so every row starts at an
    odd address; the pad bits of a record's last byte are whatever the random bytes hold."""

    def __init__(self, count: int, v: int, seed: int):
        self.count, self.r = count, LR.rsize(count)
        self.pitch = self.r + 1 + (self.r + 1) % 2
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        self.buf = torch.randint(0, 256, (1 + v * self.pitch + 15,), dtype=torch.uint8, device=DEV, generator=g)
        self.offs = [1 + j * self.pitch for j in range(v)]

    def rec(self, j: int) -> torch.Tensor:
        return self.buf[self.offs[j]: self.offs[j] + self.r]


def two_counts(n: int, first: int):
    assert first % 2 == 1 and 0 < first < n
    return [first, n - first]


def eight_counts(n: int):
    """Eight parts of ``n`` samples whose starts have every residue mod 4 and, mod 64 (a chunk's samples), fall into each of the chunk's
    four dwords; the part in the middle has fewer samples than a chunk."""
    base = n // 8 // 64 * 64
    counts = [base + 1, base + 1, base + 1, 37, base + 17, base + 30, base + 31]
    counts.append(n - sum(counts))
    starts = [sum(counts[:p]) for p in range(8)]
    assert counts[7] > 64 and {s % 4 for s in starts} == {0, 1, 2, 3} and {s % 64 // 16 for s in starts} == {0, 1, 2, 3}
    assert len({s % 64 for s in starts}) == 8
    return counts


def run_join(n, v, counts, shapes, phases, flipped, absent, seed, pad=13):
    """One table, every shape of ``shapes`` at every output phase of ``phases``.  ``flipped``: {row: parts flipped in it}; ``absent``:
    {row: the part absent in it}.  Every row is checked whole."""
    starts = [sum(counts[:p]) for p in range(len(counts))]
    parts = [Part(c, v, seed + p) for p, c in enumerate(counts)]
    dparts = []
    for p, part in enumerate(parts):
        offs = [JR.ABSENT if absent.get(j) == p else part.offs[j] for j in range(v)]
        flip = None
        if any(p in ps for ps in flipped.values()):
            flip = torch.tensor([0x80 if p in flipped.get(j, ()) else 0 for j in range(v)], dtype=torch.uint8, device=DEV)
        dparts.append((part.buf, torch.tensor(offs, dtype=torch.int64, device=DEV), part.count, flip))
    r = LR.rsize(n)
    pitch = r + pad
    total = (v - 1) * pitch + r
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        assert eng.record_size == r
        for shape in shapes:
            for phase in phases:
                buf, front = framed_at(total, phase)
                eng.join_records(dparts, v, out=buf, out_offset=front, out_stride=pitch, shape=SHAPES[shape])
                eng.wait()
                what = f"join N={n} V={v} parts={counts} {shape} phase {phase}"
                assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
                out = buf[front: front + total]
                assert LR.padding_untouched(out, v, r, pitch, SENT), f"{what}: padding between rows was written"
                for j in range(v):
                    bad = LR.check_joined(out[j * pitch: j * pitch + r], [part.rec(j) for part in parts], starts, counts,
                                          [p in flipped.get(j, ()) for p in range(len(counts))],
                                          [absent.get(j) == p for p in range(len(counts))], n)
                    assert bad is None, (f"{what}: row {j} differs first at sample {bad[0]} = {bad[0]:#x} (row byte {bad[0] >> 2:#x}, chunk "
                                         f"{((bad[0] >> 2) + phase) >> 4:#x}): got {bad[1]}, want {bad[2]}")
                del buf, out
    del parts, dparts


# ---- a. long rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["two", "eight"])
def test_join_n_mid(table):
    """N_MID, V = 3, GENERAL, STREAM and AUTO, rows at byte phases 1 and 15 with a pitch of R + 13: two parts, the first of odd size
    (every fast-path chunk of the second at a bit phase of 2), and eight parts (eight_counts).  Row 1 is flipped in the odd parts, one
    part is absent in row 2.  Needs 1 GiB."""
    need_gib(1)
    n = N_MID
    counts = two_counts(n, (1 << 23) + 3) if table == "two" else eight_counts(n)
    odd = tuple(range(1, len(counts), 2))
    run_join(n, 3, counts, ("general", "stream", "auto"), (1, 15), {1: odd}, {2: len(counts) // 2}, seed=300)


JOIN_MAX = [("stream", "two"), ("stream", "eight"), ("general", "two")]


@pytest.mark.parametrize("shape,table", JOIN_MAX, ids=[f"{s}-{t}" for s, t in JOIN_MAX])
def test_join_n_max(shape, table):
    """N_MAX (R = 2^29: STREAM's b0, last and (int32_t)R are row-relative int32, its sample index s0 = 4 b0 passes 2^31), V = 2:
    STREAM with two parts split at sample 2^30 + 1 and with eight parts (the last absent in row 0), GENERAL with two parts.  Row 1 is
    flipped in the odd parts.  Needs 4 GiB."""
    need_gib(4)
    n = N_MAX
    counts = two_counts(n, (1 << 30) + 1) if table == "two" else eight_counts(n)
    odd = tuple(range(1, len(counts), 2))
    run_join(n, 2, counts, (shape,), (15,), {1: odd}, {0: 7} if table == "eight" else {}, seed=310)


# ---- b. both sides of 2^32 work items ------------------------------------------------------------------------------------------------
P = LR.PERIOD


@pytest.mark.parametrize("shape", ["general", "stream"])
@pytest.mark.parametrize("v", [(1 << 31) - 1, 1 << 31, (1 << 31) + 23], ids=["below-2^32-items", "2^32-items", "past-2^32-items"])
def test_join_both_sides_of_2_32_items(v, shape):
    """N = 7 as parts (3, 4): R = 2 and two chunks per row, so both kernels have total = 2 V items.  V = 2^31 - 1 is the largest launch
    of the 32-bit item decomposition (2^32 - 2 items), V = 2^31 the first of the 64-bit one (2^32 items: the last index, 2^32 - 1, still
    fits 32 bits, so this launch runs the 64-bit division but would not show a narrowed index), V = 2^31 + 23 the one in which item
    indices pass 2^32 (rows 2^31 onwards, 23 of them: an index cut to 32 bits writes rows 0 .. 22 twice and these never).  Both parts share one offset tensor of
    period 45 (entry 44 absent, the others into a 44-row pool per part); part 0 has a flip tensor of period 45.  The output pitch is 3,
    so rows meet all 16 address phases and every third byte must stay the sentinel.  Compared on the device as (V // 45, 135) against
    one pattern row built with join_ref.join, plus the tail rows.  At the natural grid.  Needs 26 GiB."""
    need_gib(26)
    counts = (3, 4)
    rng = np.random.default_rng(45)
    pools = [rng.integers(0, 256, size=1 + 2 * (P - 1) + 16, dtype=np.uint8) for _ in counts]   # row k at byte 1 + 2 k: odd addresses
    offs = np.array([1 + 2 * k for k in range(P - 1)] + [JR.ABSENT], dtype=np.int64)
    flip = (rng.integers(0, 2, size=P) * 0x41).astype(np.uint8)
    assert flip.any() and not flip.all()
    pattern = JR.join([(pools[0], offs, 3, flip), (pools[1], offs, 4, None)], P)                 # (45, 2)
    assert (pattern[P - 1] == [0xFF, 0x3F]).all() and len({bytes(r) for r in pattern}) > 30
    row3 = np.full((P, 3), SENT, dtype=np.uint8)
    row3[:, :2] = pattern
    d_pattern = torch.from_numpy(row3.reshape(-1)).to(DEV)

    d_offs = torch.empty(v, dtype=torch.int64, device=DEV)
    LR.fill_periodic(d_offs, torch.from_numpy(offs).to(DEV))
    d_flip = torch.empty(v, dtype=torch.uint8, device=DEV)
    LR.fill_periodic(d_flip, torch.from_numpy(flip).to(DEV))
    dparts = [(torch.from_numpy(pools[0]).to(DEV), d_offs, 3, d_flip), (torch.from_numpy(pools[1]).to(DEV), d_offs, 4, None)]
    total = 3 * v                                        # the last row's third byte included: it must stay the sentinel too
    buf, front = LR.framed(total, DEV)
    with pgen_rs_amd.GtEngine(7, device=0) as eng:
        assert eng.record_size == 2
        eng.join_records(dparts, v, out=buf, out_offset=front, out_stride=3, shape=SHAPES[shape])
        eng.wait()
    what = f"join N=7 V={v} ({2 * v:#x} items) {shape}"
    assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
    out = buf[front: front + total]
    whole = v // P
    got = out[: whole * 3 * P].view(whole, 3 * P)
    slab = 1 << 20
    for a in range(0, whole + 1, slab):
        b = min(whole, a + slab)
        if a < whole:
            i = LR._first_diff(got[a:b], d_pattern[None, :].expand(b - a, 3 * P))
            at = None if i is None else 3 * P * a + i
        else:
            tail = out[whole * 3 * P:]
            i = LR._first_diff(tail, d_pattern[: tail.numel()])
            at = None if i is None else whole * 3 * P + i
        if at is not None:
            j, byte = at // 3, at % 3
            raise AssertionError(f"{what}: row {j} = {j:#x} byte {byte} (output byte {at:#x}, item {2 * j + (byte > 0):#x}): got "
                                 f"{int(out[at]):#04x}, want {int(d_pattern[at % (3 * P)]):#04x} "
                                 "(an item index cut to 32 bits sends item 2^32 + x to item x)")
    del buf, out, got, d_offs, d_flip


# ---- c. addresses past 4 GiB ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["general", "stream"])
def test_join_addresses_past_4_gib(shape):
    """N = 70 001 + 3, V = 5.  One source buffer of 4 GiB + 64 KiB holds both parts' records, rows 0, 2 and 4 in its last 64 KiB and
    rows 1 and 3 in its first (int64 offsets past 2^32); the output pitch is 2^30 + 3, so row 4 starts past 4 GiB.  The bytes
    between the rows are checked with padding_untouched.  Needs 10 GiB."""
    need_gib(10)
    counts = [70_001, 3]
    n, v = sum(counts), 5
    r, r0 = LR.rsize(n), LR.rsize(counts[0])
    size = 4 * GIB + (1 << 16)
    src = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(320)
    for a in (0, 4 * GIB):
        src[a: a + (1 << 16)] = torch.randint(0, 256, (1 << 16,), dtype=torch.uint8, device=DEV, generator=g)
    step = r0 + 3 + (r0 + 3) % 2                          # even: odd addresses stay odd; at least three bytes between records
    offs0 = [(4 * GIB if j % 2 == 0 else 0) + 1 + (j // 2) * step for j in range(v)]
    offs1 = [o + r0 + 1 for o in offs0[::-1]]             # the small part's byte, in the gap behind another row's record
    assert r0 % 2 == 1 and all(o % 2 for o in offs0 + offs1) and max(offs0) > 1 << 32 and max(offs1) > 1 << 32
    assert all((o % (4 * GIB)) + step <= 1 << 16 for o in offs0)   # every record and its gap inside the two random 64-KiB ends
    dparts = [(src, torch.tensor(offs0, dtype=torch.int64, device=DEV), counts[0], torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8, device=DEV)),
              (src, torch.tensor(offs1, dtype=torch.int64, device=DEV), counts[1], None)]
    pitch = GIB + 3
    total = (v - 1) * pitch + r
    assert (v - 1) * pitch > 1 << 32
    buf, front = framed_at(total, 5)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.join_records(dparts, v, out=buf, out_offset=front, out_stride=pitch, shape=SHAPES[shape])
        eng.wait()
    what = f"join N={n} V={v} pitch {pitch:#x} {shape}"
    assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
    out = buf[front: front + total]
    assert LR.padding_untouched(out, v, r, pitch, SENT, slab_rows=1), f"{what}: bytes between the rows were written"
    for j in range(v):
        rows = [src[offs0[j]: offs0[j] + r0], src[offs1[j]: offs1[j] + 1]]
        bad = LR.check_joined(out[j * pitch: j * pitch + r], rows, [0, counts[0]], counts, [j in (1, 4), False], [False, False], n)
        assert bad is None, (f"{what}: row {j} (output byte {j * pitch:#x}, sources at {offs0[j]:#x} and {offs1[j]:#x}) differs first at "
                             f"sample {bad[0]}: got {bad[1]}, want {bad[2]}")
    del buf, out, src
