"""The far end of the ABI's index ranges for the Gram product: pgenhip_gram_apply / _at (gt_gapply.hip) with more tiles than the grid
holds side by side in each of its four kernels, the grid-block clamp of the launch plan, tables, projections, Q and Y at byte offsets
past 2^32, the two zeroing calls at a wide pitch and past 4 GiB, and rows of up to 2^31 - 1 samples.  The levels, the three keep sets
(all samples, 4 099 spread over the range, every 22nd) and the records (random bytes, row 0 at byte 1, stride R + 1) are
test_long_rows_gpu.py's.  Every threshold is stated as an assert on the launch plan (gapply_plan.py runs csrc/launch_plan.h), so a
changed plan constant fails the assert instead of emptying the case.

Every comparison is exact: tables are integers in [-8, 8] and Q is an integer in [-4, 4], so |P| <= 32 K <= 2^36 and
|Y| <= 8 V max|P|, and every partial sum in any order is an integer below 2^52 (asserted per case by `exact`, and again by
longrow_ref.py from the values themselves).  Long rows are checked by longrow_ref.apply_proj / check_apply_out (int64, slab by slab,
held against gapply_ref.py by test_longrow_ref.py); many short rows by FP64 matrix products of those small integers, which are exact
for the same reason.  Every output sits in a sentinel frame that must come back untouched; a case is skipped only when the card has
less free memory than the case states.
"""
import time

import numpy as np
import pytest
import torch

import gapply_plan as AP
import longrow_ref as LR
import pgen_rs_amd
from pgen_rs_amd import _capi
from longrow_ref import SENT, frame_ok, need_gib
from test_gram_apply_gpu import int_tables
from test_long_rows_gpu import N_MAX, N_MID, Records, kept_of, select

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = {"general": _capi.GAPPLY_GENERAL, "mfma": _capi.GAPPLY_MFMA, "auto": _capi.GAPPLY_AUTO}
N_28 = (1 << 28) + 257   # 2^20 + 2 sample tiles of the MFMA Y pass, and as many entry blocks of GENERAL's at C = 1


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def exact(v: int, k: int, calls: int = 1):
    """The case's sums are exact in float64 in any order: |P| <= K * 8 * 4 and |Y| <= calls * V * 8 * max|P| stay below 2^52."""
    assert calls * v * 8 * (k * 8 * 4) < 2 ** 52


def doubles(count: int):
    """-> (framed buffer, front, payload bytes, the payload as ``count`` doubles)."""
    buf, front = LR.framed(8 * count, DEV, align=8)
    return buf, front, 8 * count, buf[front: front + 8 * count].view(torch.float64)


def device_q(k: int, width: int, seed: int) -> torch.Tensor:
    """(k, width) float64 integers in [-4, 4] drawn on the device (what int_q draws on the host, for K too large to draw there)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(-4, 5, (k, width), dtype=torch.int8, device=DEV, generator=g).to(torch.float64)


def apply_call(eng, kw, at, v, d_t, q, proj, out, out_stride, kernel, accumulate, what):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if at is None:
        eng.gram_apply(kw["records"], d_t, q, record_stride=kw["record_stride"], variant_idx=kw.get("variant_idx"), n_variants=v, proj=proj,
                       out=out, out_stride=out_stride, accumulate=accumulate, kernel=KERNELS[kernel], records_offset=kw["records_offset"])
    else:
        eng.gram_apply_at(at[0], at[1], d_t, q, n_variants=v, proj=proj, out=out, out_stride=out_stride, accumulate=accumulate,
                          kernel=KERNELS[kernel])
    eng.wait()
    print(f"{what}: the call took {time.perf_counter() - t0:.2f} s")


def check_rows(got: torch.Tensor, want: torch.Tensor, what: str, slab: int = 1 << 22):
    """``got`` and ``want``: (rows, C) float64 on the device, compared slab by slab; the first differing entry is named with its byte
    offset (an offset cut to 32 bits sends byte 2^32 + x to byte x; a tile that no block strides to keeps the prefill)."""
    rows, c = want.shape
    assert tuple(got.shape) == (rows, c)
    for lo in range(0, rows, slab):
        i = LR._first_diff(got[lo: lo + slab], want[lo: lo + slab])
        if i is not None:
            j, l = lo + i // c, i % c
            raise AssertionError(f"{what}: entry ({j}, {l}), byte {8 * (j * got.stride(0) + l):#x}: got {float(got[j, l])!r}, want {float(want[j, l])!r}")


# ---- a, b. many short rows gathered from 64 records: far rows, far tables, far proj, the grid-block clamp ------------------------------
class Gathered:
    """V rows gathered through d_variant_idx from 64 distinct random records of n samples (the last row is record 63), int8 tables
    drawn on the device and widened, a (n, C) integer Q, and the exact P = Z Q (V x C) and Y = Z^T P (n x C) as float64: FP64
    products of small integers over slabs of ``slab`` rows, Y as a batch of 1 024-row products (one product of 2^22 x n is a single
    slow tile)."""

    def __init__(self, n: int, v: int, c: int, seed: int, slab: int):
        self.n, self.v, self.c, distinct = n, v, c, 64
        exact(v, n, 2)
        self.recs = Records(n, distinct, seed)
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        self.idx = torch.randint(0, distinct, (v,), dtype=torch.int32, device=DEV, generator=g)
        self.idx[-1] = distinct - 1
        t8 = torch.randint(-8, 9, (v, 4), dtype=torch.int8, device=DEV, generator=g)
        self.d_t = t8.to(torch.float64)
        self.q = device_q(n, c, seed + 1)
        codes = torch.stack([LR.codes(self.recs.rec(j), 0, n) for j in range(distinct)]).to(torch.int64)   # (64, n)
        self.want_p = torch.empty((v, c), dtype=torch.float64, device=DEV)
        self.want_y = torch.zeros((n, c), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lo in range(0, v, slab):
            hi = min(v, lo + slab)
            z = torch.gather(t8[lo:hi].to(torch.int64), 1, codes[self.idx[lo:hi].long()]).to(torch.float64)   # Z[j, s] = t_j[code of sample s in row j]
            p = z @ self.q
            self.want_p[lo:hi] = p
            if (hi - lo) % 1024 == 0:
                self.want_y += torch.bmm(z.view(-1, 1024, n).transpose(1, 2), p.view(-1, 1024, c)).sum(dim=0)
            else:
                self.want_y += z.T @ p
            del z, p
        torch.cuda.synchronize()
        print(f"gathered N={n} V={v} C={c}: the reference took {time.perf_counter() - t0:.2f} s")
        assert float(self.want_y.abs().max()) < 2.0 ** 52 and float(self.want_p.abs().max()) <= 32 * n
        del t8

    def call(self, eng, c, proj, out, out_stride, kernel, accumulate, what):
        """The first ``c`` columns of Q (a view of the wider rows when c < C)."""
        kw = dict(records=self.recs.buf, record_stride=self.recs.stride, records_offset=1, variant_idx=self.idx)
        apply_call(eng, kw, None, self.v, self.d_t, self.q[:, :c], proj, out, out_stride, kernel, accumulate, what)


def check_gathered(g: Gathered, c, pbuf, pfront, pbytes, proj, obuf, ofront, obytes, out, out_stride, scale, what):
    assert frame_ok(pbuf, pfront, pbytes), f"{what}: bytes outside d_proj were written"
    assert frame_ok(obuf, ofront, obytes), f"{what}: bytes outside d_out were written"
    assert LR.padding_untouched(obuf[ofront: ofront + obytes], g.n, 8 * c, 8 * out_stride, SENT), f"{what}: padding between the rows of d_out was written"
    check_rows(proj.view(g.v, c), g.want_p[:, :c], what + " P")
    check_rows(torch.as_strided(out, (g.n, c), (out_stride, 1)), g.want_y[:, :c] * scale, what + " Y")


def test_far_rows_far_tables_far_proj():
    """N = 4, all samples, C = 5, V = 2^27 + 77 rows gathered from 64 records: 4.3 GB of tables (row 2^27's table is 2^32 bytes from
    d_code_values) and 5.4 GB of d_proj (byte offsets past 2^32 in both passes).  MFMA: 2^21 + 2 row tiles over the grid's 2^20 (the
    P pass strides: a block re-enters the LDS staging after the closing barrier), one sample tile cut into 512 row slices.  GENERAL:
    2^27.3 blocks of (row, column) waves over 2^20, 2 048 row slices.  All of d_proj and Y are compared on the device.  Needs 18 GiB
    (4.3 GB tables, 5.4 GB d_proj, 5.4 GB expected P, 1 GB of row numbers and int8 tables, the reference's slabs)."""
    need_gib(18)
    n, c, v = 4, 5, (1 << 27) + 77
    assert 4 * (1 << 27) * 8 == 1 << 32 and v * c * 8 > 1 << 32
    pm, pg = AP.plan(v, n, c, True), AP.plan(v, n, c, False)
    assert pm.p_tiles > AP.MAX_GRID_TILES == pm.p_grid and pm.y_tiles == 1 and pm.row_slices > 1 and v * (pm.row_slices - 1) > 1 << 32
    assert pg.p_tiles > AP.MAX_GRID_TILES == pg.p_grid and pg.y_tiles == 1 and pg.row_slices > 1 and v * (pg.row_slices - 1) > 1 << 32
    g = Gathered(n, v, c, 190, 1 << 22)
    assert g.d_t.numel() * 8 > 1 << 32
    stride = c + 3
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for kernel in ("general", "mfma"):
            pbuf, pfront, pbytes, proj = doubles(v * c)
            obuf, ofront, obytes, out = doubles((n - 1) * stride + c)
            what = f"gram_apply far rows {kernel}"
            g.call(eng, c, proj, out, stride, kernel, False, what)
            check_gathered(g, c, pbuf, pfront, pbytes, proj, obuf, ofront, obytes, out, stride, 1, what)
            del pbuf, proj, obuf, out
    del g


def test_grid_block_clamp_and_memset_past_4_gib():
    """N = 300, all samples, V = 2^26 + 65 rows gathered from 64 records, PGENHIP_KNOB_GAPPLY_SAMPLE_SLICES = 7: the P pass has more
    tiles than the grid's 2^20, so the 7 slices (5 by the row's 64-sample units) are clamped to 4 and the kernel's
    blockIdx.x / grid_tiles must agree.  MFMA, C = 8: d_proj is 4.3 GB, zeroed by one hipMemsetAsync and then filled by atomics from
    four slices across the tile stride.  GENERAL, C = 1 (a view of the 8-wide Q): 2^24 + 17 blocks of waves.  d_proj and d_out are
    pre-filled with 0x01 bytes, so that an entry nobody wrote shows.  Then ACCUMULATE on top: Y doubles, P is the same (d_proj is
    overwritten per call).  Needs 16 GiB (2.1 GB tables, 4.3 GB d_proj, 4.3 GB expected P, the reference's slabs of 2^19 rows)."""
    need_gib(16)
    n, v = 300, (1 << 26) + 65
    cols = {"general": 1, "mfma": 8}
    for kernel, c in cols.items():
        p = AP.plan(v, n, c, kernel == "mfma", 7, 0)
        assert p.p_tiles > p.p_grid == AP.MAX_GRID_TILES and p.sample_slices == 4 == AP.MAX_GRID_BLOCKS // p.p_grid
        assert AP.plan(1000, n, c, kernel == "mfma", 7, 0).sample_slices == 5   # (the knob and the row's units alone do not give 4)
    assert v * cols["mfma"] * 8 > 1 << 32
    g = Gathered(n, v, 8, 191, 1 << 19)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_GAPPLY_SAMPLE_SLICES, 7)
        for kernel, c in cols.items():
            stride = c + 3
            pbuf, pfront, pbytes, proj = doubles(v * c)
            obuf, ofront, obytes, out = doubles((n - 1) * stride + c)
            proj.view(torch.int64).fill_(0x0101010101010101)
            torch.as_strided(out.view(torch.int64), (n, c), (stride, 1)).fill_(0x0101010101010101)
            for accumulate in (False, True):
                what = f"gram_apply clamp {kernel} C={c} accumulate={accumulate}"
                g.call(eng, c, proj, out, stride, kernel, accumulate, what)
                check_gathered(g, c, pbuf, pfront, pbytes, proj, obuf, ofront, obytes, out, stride, 2 if accumulate else 1, what)
            del pbuf, proj, obuf, out
    del g


# ---- c. wide pitches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["general", "mfma", "auto"])
@pytest.mark.parametrize("keep", ["all", "two-of-three"])
def test_wide_pitches(keep, kernel):
    """N = 200, V = 75, C = 13, q_stride = out_stride = 2^22 + 3 doubles: the last ranks of Q and of d_out start past byte 2^32, with
    all samples and with a kept list of K = 133.  Three calls into one framed d_out: the default plan (one row slice: stores);
    PGENHIP_KNOB_GAPPLY_ROW_SLICES = 2 (hipMemset2DAsync at a 32-MiB pitch, which must clear 13 doubles per row and not one more,
    then atomics); ACCUMULATE on top (twice the sums).  The padding of Q and of d_out holds the sentinel and must come back
    untouched.  Needs 14 GiB."""
    need_gib(14)
    n, v, c = 200, 75, 13
    stride = (1 << 22) + 3
    kept = None if keep == "all" else np.array([s for s in range(n) if s % 3 != 1], dtype=np.uint32)
    k = LR.kept_count(n, kept)
    assert k >= 130 and (k - 1) * stride * 8 > 1 << 32
    exact(v, k, 2)
    mfma = kernel != "general"
    assert AP.plan(v, k, c, mfma).row_slices == 1 and AP.plan(v, k, c, mfma, 0, 2).row_slices == 2
    recs = Records(n, v, 192)
    order, kw, at = select(recs, "stride")
    rows = [recs.rec(j) for j in order]
    t = int_tables(v, 192)
    d_t = torch.from_numpy(t).to(DEV)
    d_kept = LR.as_kept(kept, DEV)
    count = (k - 1) * stride + c
    qbuf, qfront, qbytes, qflat = doubles(count)
    q = torch.as_strided(qflat, (k, c), (stride, 1))
    q.copy_(device_q(k, c, 193))
    t0 = time.perf_counter()
    want_p = LR.apply_proj(rows, n, d_kept, t, q)
    print(f"gram_apply wide pitches {keep}: the reference of P took {time.perf_counter() - t0:.2f} s")
    obuf, ofront, obytes, oflat = doubles(count)
    out = torch.as_strided(oflat, (k, c), (stride, 1))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        for step, knob, accumulate, scale in (("default plan", 0, False, 1), ("two row slices", 2, False, 1), ("two row slices, ACCUMULATE", 2, True, 2)):
            eng.tune(_capi.KNOB_GAPPLY_ROW_SLICES, knob)
            pbuf, pfront, pbytes, proj = doubles(v * c)
            what = f"gram_apply wide pitches {keep} {kernel}, {step}"
            apply_call(eng, kw, at, v, d_t, q, proj, oflat, stride, kernel, accumulate, what)
            assert frame_ok(pbuf, pfront, pbytes), f"{what}: bytes outside d_proj were written"
            assert frame_ok(obuf, ofront, obytes), f"{what}: bytes outside d_out were written"
            assert LR.padding_untouched(obuf[ofront: ofront + obytes], k, 8 * c, 8 * stride, SENT, slab_rows=8), f"{what}: padding between the rows of d_out was written"
            check_rows(proj.view(v, c), want_p.to(torch.float64), what + " P")
            bad = LR.check_apply_out(out, rows, n, d_kept, t, want_p * scale)
            assert bad is None, f"{what}: Y rank {bad[0]} column {bad[1]}, byte {8 * (bad[0] * stride + bad[1]):#x}: got {bad[2]!r}, want {bad[3]}"
    assert frame_ok(qbuf, qfront, qbytes) and LR.padding_untouched(qbuf[qfront: qfront + qbytes], k, 8 * c, 8 * stride, SENT, slab_rows=8), "Q's padding was written"
    del qbuf, qflat, q, obuf, oflat, out, recs


# ---- d. long rows ----------------------------------------------------------------------------------------------------------------------------
def run_long(n, v, keep, sources, cols, seed, pad=0, knobs=(), tag=""):
    """pgenhip_gram_apply / _at on V rows of n samples: for every row source and every (kernel, C) of ``cols``, P and Y into framed
    buffers (d_out's rows ``pad`` doubles wider than they hold), against longrow_ref.  Q is drawn once at the widest C; a narrower
    C reads a view of its rows (q_stride > C)."""
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    exact(v, k)
    width = max(cols.values())
    q = device_q(k, width, seed + 1)
    recs = Records(n, v, seed)
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        for knob, value in knobs:
            eng.tune(knob, value)
        for source in sources:
            order, kw, at = select(recs, source)
            rows = [recs.rec(j) for j in order]
            t = int_tables(len(order), seed)   # by position in the selection
            d_t = torch.from_numpy(t).to(DEV)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want_p = LR.apply_proj(rows, n, d_kept, t, q)
            torch.cuda.synchronize()
            print(f"gram_apply N={n} {keep} {source}: the reference of P took {time.perf_counter() - t0:.2f} s")
            for kernel, c in cols.items():
                stride = c + pad
                pbuf, pfront, pbytes, proj = doubles(len(order) * c)
                obuf, ofront, obytes, oflat = doubles((k - 1) * stride + c)
                what = f"gram_apply N={n} V={len(order)} C={c} {keep} {source} {kernel}{tag}"
                apply_call(eng, kw, at, len(order), d_t, q[:, :c], proj, oflat, stride, kernel, False, what)
                assert frame_ok(pbuf, pfront, pbytes), f"{what}: bytes outside d_proj were written"
                assert frame_ok(obuf, ofront, obytes), f"{what}: bytes outside d_out were written"
                assert LR.padding_untouched(obuf[ofront: ofront + obytes], k, 8 * c, 8 * stride, SENT), f"{what}: padding between the rows of d_out was written"
                check_rows(proj.view(len(order), c), want_p[:, :c].to(torch.float64), what + " P")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bad = LR.check_apply_out(torch.as_strided(oflat, (k, c), (stride, 1)), rows, n, d_kept, t, want_p[:, :c])
                print(f"{what}: the reference of Y took {time.perf_counter() - t0:.2f} s")
                assert bad is None, f"{what}: Y rank {bad[0]} column {bad[1]}, byte {8 * (bad[0] * stride + bad[1]):#x}: got {bad[2]!r}, want {bad[3]}"
                del pbuf, proj, obuf, oflat
    del recs, q, d_kept


@pytest.mark.parametrize("keep", ["all", "sparse", "every22"])
def test_gram_apply_n_mid(keep):
    """N_MID, V = 5, C = 16, every row source (the gather names a row twice, _at reverses the rows), GENERAL and MFMA, d_out's rows 3
    doubles wider than they hold.  With all samples GENERAL's Y pass has 2^20 + 1 entry blocks over the grid's 2^20: its stride
    loop runs for exactly one tile more; the default plan cuts the samples of the P pass into more than 100 slices, which meet in
    atomics; R = 2^22 + 1, so the last step of the MFMA passes takes its record bytes one at a time, clamped at the last.
    Needs 6 GiB."""
    need_gib(6)
    n, v, c = N_MID, 5, 16
    if keep == "all":
        pg, pm = AP.plan(v, n, c, False), AP.plan(v, n, c, True)
        assert pg.y_tiles == AP.MAX_GRID_TILES + 1 == pg.y_grid + 1
        assert pg.sample_slices > 100 and pm.sample_slices > 100 and pg.row_slices == pm.row_slices == 1
    run_long(n, v, keep, ("stride", "gather", "at"), {"general": c, "mfma": c}, 194, pad=3)


def test_gram_apply_n_2_28():
    """N = 2^28 + 257, all samples, V = 3, C = 2 for MFMA and C = 1 for GENERAL (a view of the 2-wide Q): 2^20 + 2 sample tiles and
    as many entry blocks, so the Y pass of both strides over the grid's 2^20; with C = 2 the last ranks of Q and of d_out lie past
    byte 2^32; 512 and 2 048 sample slices meet in atomics; R = 2^26 + 65, so the last steps hang past a long record and take its
    bytes one at a time, clamped at the last.  Needs 14 GiB."""
    need_gib(14)
    n, v = N_28, 3
    pg, pm = AP.plan(v, n, 1, False), AP.plan(v, n, 2, True)
    assert pg.y_tiles == pm.y_tiles == AP.MAX_GRID_TILES + 2 and pg.y_grid == pm.y_grid == AP.MAX_GRID_TILES
    assert (pg.sample_slices, pm.sample_slices) == (2048, 512) and (n - 1) * 2 * 8 > 1 << 32
    run_long(n, v, "all", ("stride",), {"general": 1, "mfma": 2}, 195)


def test_gram_apply_n_2_28_one_sample_slice():
    """The same rows with PGENHIP_KNOB_GAPPLY_SAMPLE_SLICES = 1, GENERAL, C = 1: one wave per row walks all 2^28 + 257 ranks, 2^22
    turns of its lane loop, and stores.  Measured on an MI355X: 1.8 s.  (The MFMA shape's one block per row tile takes 2^22 staged
    steps and 7.9 s for the same call, too long for this suite; its step arithmetic at the far end of a row is
    test_gram_apply_n_max's.)  Needs 8 GiB."""
    need_gib(8)
    n, v = N_28, 3
    assert AP.plan(v, n, 1, False, 1, 0).sample_slices == 1 and -(-n // 64) > 1 << 22
    run_long(n, v, "all", ("stride",), {"general": 1}, 195, knobs=((_capi.KNOB_GAPPLY_SAMPLE_SLICES, 1),), tag=", one sample slice")


@pytest.mark.parametrize("keep", ["all", "every22", "sparse"])
def test_gram_apply_n_max(keep):
    """N_MAX = 2^31 - 1 (the ABI's limit), V = 3, C = 1, GENERAL and MFMA: R = 2^29, first byte of a step up to 2^29 - 16 (the last
    step's 16 bytes end on the record's last byte, whose fourth bit pair is dirty padding and meets a staged 0.0; the steps that hang
    past a long record and are read byte by byte are test_gram_apply_n_mid's and test_gram_apply_n_2_28's), slices of 2^22 samples =
    2^16 steps, 2^23 sample tiles over the grid's 2^20; through the lists, entries up to sample 2^31 - 2.  All samples: Q and d_out
    are 16 GiB each (needs 40 GiB); every 22nd sample needs 8 GiB, the sparse list 4 GiB."""
    need_gib({"all": 40, "every22": 8, "sparse": 4}[keep])
    n, v = N_MAX, 3
    if keep == "all":
        pm = AP.plan(v, n, 1, True)
        assert pm.y_tiles == 1 << 23 > pm.y_grid and AP.slice_samples(n, pm.sample_slices - 1, pm.sample_slices) == (n - (1 << 22) + 1, n)
    run_long(n, v, keep, ("stride",), {"general": 1, "mfma": 1}, 196)
