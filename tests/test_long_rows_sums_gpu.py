"""The far end of the ABI's index ranges for the two FP64 sum entry points: pgenhip_sample_gram and pgenhip_variant_sums on rows of up to
2^31 - 1 samples, into Gram outputs whose byte offsets and entry indices pass 2^32, over more tiles and pair blocks than the grid
holds side by side, and with tables 2^32 bytes and more from d_code_values.  The levels, the three keep sets (all samples, 4 099
spread over the range, every 22nd) and the records (random bytes, row 0 at byte 1, stride R + 1) are test_long_rows_gpu.py's.

Every comparison is exact: tables and values are integers in [-8, 8], so every partial sum in any order is an integer far below
2^53 (the largest here is 64 * 2^27 = 2^33), and the expected sums are formed in int64 by longrow_ref.py (held against gram_ref.py and
vsum_ref.py by test_longrow_ref.py).  Where a whole matrix is compared on the device, Z^T Z is an FP64 matrix product of those small
integers, which is exact for the same reason.  Every output sits in a sentinel frame that must come back untouched; a case is
skipped only when the card has less free memory than the case states.
"""
import time

import numpy as np
import pytest
import torch

import gram_plan as GP
import longrow_ref as LR
import pgen_rs_amd
import vsum_plan as VP
from pgen_rs_amd import _capi
from longrow_ref import SENT, frame_ok, need_gib
from test_long_rows_gpu import N_MAX, N_MID, Records, kept_of, select
from test_sample_gram_gpu import int_tables
from test_variant_sums_gpu import int_values

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEEPS = ["all", "sparse", "every22"]
SOURCES = ("stride", "gather", "at")
GRAM = {"general": _capi.GRAM_GENERAL, "mfma": _capi.GRAM_MFMA}
VSUM = {"general": _capi.VSUM_GENERAL, "mfma": _capi.VSUM_MFMA}


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


# ---- a. Gram matrix on long rows ------------------------------------------------------------------------------------------------------
def gram_out(a, b, stride):
    """-> (framed buffer, front, payload bytes, the payload as doubles): a_count rows of b_count doubles, ``stride`` doubles apart."""
    nbytes = 8 * ((a[1] - 1) * stride + b[1])
    buf, front = LR.framed(nbytes, DEV, align=8)
    return buf, front, nbytes, buf[front: front + nbytes].view(torch.float64)


def gram_call(eng, kw, at, v, d_t, a, b, out, stride, kernel, accumulate):
    if at is None:
        eng.sample_gram(kw["records"], kw["record_stride"], kw.get("variant_idx"), v, code_values=d_t, a=a, b=b, out=out, out_stride=stride,
                        accumulate=accumulate, kernel=kernel, records_offset=kw["records_offset"])
    else:
        eng.sample_gram_at(at[0], at[1], d_t, v, a=a, b=b, out=out, out_stride=stride, accumulate=accumulate, kernel=kernel)
    eng.wait()


def check_gram_out(buf, front, nbytes, out, stride, a, b, want, what, slab_rows=1 << 24):
    assert frame_ok(buf, front, nbytes), f"{what}: bytes outside the output were written"
    assert LR.padding_untouched(buf[front: front + nbytes], a[1], 8 * b[1], 8 * stride, SENT, slab_rows), f"{what}: padding between rows was written"
    bad = LR.check_gram(torch.as_strided(out, (a[1], b[1]), (stride, 1)), want)
    assert bad is None, (f"{what}: entry ({bad[0]}, {bad[1]}) = a rank {a[0] + bad[0]}, b rank {b[0] + bad[1]}, byte "
                         f"{8 * (bad[0] * stride + bad[1]):#x} of the output: got {bad[2]!r}, want {bad[3]}")


def run_gram(n, v, keep, source, kernels, ranges, seed, twice):
    """Every range pair of ``ranges(K)`` through every kernel into a framed output whose rows are 3 doubles wider than they hold:
    an overwrite, then (``twice``) ACCUMULATE on top, which must give twice the sums."""
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    recs = Records(n, v, seed)
    order, kw, at = select(recs, source)
    rows = [recs.rec(j) for j in order]
    t = int_tables(len(order), seed)   # by position in the selection
    d_t = torch.from_numpy(t).to(DEV)
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        for a, b in ranges(k):
            want = LR.gram_ranges(rows, n, d_kept, t, a, b)
            for kernel in kernels:
                stride = b[1] + 3
                buf, front, nbytes, out = gram_out(a, b, stride)
                for accumulate in (False, True) if twice else (False,):
                    gram_call(eng, kw, at, len(order), d_t, a, b, out, stride, GRAM[kernel], accumulate)
                    check_gram_out(buf, front, nbytes, out, stride, a, b, want * (2 if accumulate else 1),
                                   f"gram N={n} V={len(order)} {keep} {source} a={a} b={b} {kernel} accumulate={accumulate}")
                del buf, out
    del recs, rows, d_kept


@pytest.mark.parametrize("keep", KEEPS)
def test_gram_n_mid(keep):
    """N_MID, V = 9, every row source (the gather names a row twice, _at reverses the rows), GENERAL and MFMA: a = the first 70 ranks
    and b = the last 67, the two swapped, and the last 67 squared.  The second tile of the last 67 ranks hangs past the range, which
    with all samples is the row's true end: the clamped byte index and the rank mask at byte R - 1.  Needs 1 GiB."""
    need_gib(1)
    for source in SOURCES:
        run_gram(N_MID, 9, keep, source, ("general", "mfma"),
                 lambda k: [((0, 70), (k - 67, 67)), ((k - 67, 67), (0, 70)), ((k - 67, 67), (k - 67, 67))], 140, False)


GRAM_MAX = ["all-first-last", "all-last-first", "every22-last-last", "sparse-all-all"]


@pytest.mark.parametrize("kernel", ["general", "mfma"])
@pytest.mark.parametrize("case", GRAM_MAX)
def test_gram_n_max(case, kernel):
    """N_MAX, V = 9: all samples with a = the first 70 and b = the last 70 ranks (by stride) and the two swapped (through _at, rows
    reversed); every 22nd sample with both ranges the last 70 ranks; the sparse list with both ranges all 4 099 ranks.  Sample bytes
    up to R - 1 = 2^29 - 1 of every row.  Overwrite, then ACCUMULATE on top: twice the sums.  Only the tiles' bytes are read; the cost
    is filling 4.8 GB of records.  Needs 8 GiB."""
    need_gib(8)
    keep, ra, rb = case.split("-")

    def ranges(k):
        rng_of = {"first": (0, 70), "last": (k - 70, 70), "all": (0, k)}
        return [(rng_of[ra], rng_of[rb])]

    run_gram(N_MAX, 9, keep, "at" if case == "all-last-first" else "stride", (kernel,), ranges, 141, True)


# ---- b. per-variant sums on long rows ----------------------------------------------------------------------------------------------------
def device_values(k: int, width: int, seed: int):
    """-> ((k, width) int64 values in [-8, 8] made on the device, the same as float64): what int_values draws on the host, for K too
    large to draw there."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    vi = torch.randint(-8, 9, (k, width), dtype=torch.int64, device=DEV, generator=g)
    return vi, vi.to(torch.float64)


def sums_call(eng, kw, at, v, vals, c, kernel, what):
    """One pgenhip_variant_sums / _at call into a framed buffer -> the V * C * 4 sums (a device tensor); the frame must survive."""
    nbytes = 8 * v * c * 4
    buf, front = LR.framed(nbytes, DEV, align=8)
    out = buf[front: front + nbytes].view(torch.float64)
    if at is None:
        eng.variant_sums(kw["records"], vals, record_stride=kw["record_stride"], variant_idx=kw.get("variant_idx"), out=out, flags=kernel,
                         n_variants=v, records_offset=kw["records_offset"])
    else:
        eng.variant_sums_at(at[0], at[1], vals, out=out, flags=kernel, n_variants=v)
    eng.wait()
    assert frame_ok(buf, front, nbytes), f"{what}: bytes outside the sums were written"
    return out


def columns_of(vi: torch.Tensor, vf: torch.Tensor, c: int):
    """The first c columns of the int64 values (for the reference) and of the float64 values (for the call): C = 1 as a 1-D tensor;
    fewer columns than the rows are wide as a view of the wider rows (v_stride > C)."""
    if c == 1:
        return vi[:, :1], vf[:, 0].contiguous()
    return vi[:, :c], vf[:, :c]


def check_sums(out, rows, n, d_kept, vi_c, what):
    bad = LR.check_variant_sums(out, rows, n, d_kept, vi_c)
    assert bad is None, f"{what}: row {bad[0]} column {bad[1]} code {bad[2]}: got {bad[3]!r}, want {bad[4]}"


@pytest.mark.parametrize("keep", KEEPS)
def test_variant_sums_n_mid(keep):
    """N_MID, V = 5, every row source, C = 1, 16 and 3 (a view of the 16-wide value rows), GENERAL and MFMA.  R = 2^22 + 1: the
    matrix-core shape's last tile holds one byte and is moved back over the 31 before it, whose values must count once.
    Needs 4 GiB."""
    n, v = N_MID, 5
    need_gib(4)
    assert VP.record_size(n) % VP.TILE_BYTES == 1
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    vf = torch.from_numpy(int_values(np.random.default_rng(150), k)).to(DEV)
    vi = vf.to(torch.int64)
    recs = Records(n, v, 150)
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for source in SOURCES:
            order, kw, at = select(recs, source)
            rows = [recs.rec(j) for j in order]
            for c in (1, 16, 3):
                vi_c, vals = columns_of(vi, vf, c)
                assert c != 3 or vals.stride(0) == 16
                for kernel in ("general", "mfma"):
                    what = f"variant_sums N_MID {keep} {source} C={c} {kernel}"
                    check_sums(sums_call(eng, kw, at, len(order), vals, c, VSUM[kernel], what), rows, n, d_kept, vi_c, what)
    del recs, vi, vf, d_kept


def run_sums_n_max(keep, c, v, kernel, seed):
    n = N_MAX
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    vi, vf = device_values(k, 4 if c == 3 else c, seed)   # C = 3: a view of 4-wide rows
    vi_c, vals = columns_of(vi, vf, c)
    recs = Records(n, v, seed)
    order, kw, at = select(recs, "stride")
    rows = [recs.rec(j) for j in order]
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        what = f"variant_sums N_MAX {keep} C={c} V={v} {kernel}"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sums_call(eng, kw, at, v, vals, c, VSUM[kernel], what)
        print(f"{what}: the call took {time.perf_counter() - t0:.2f} s")
        check_sums(out, rows, n, d_kept, vi_c, what)
    del recs, rows, vi, vf, vi_c, vals, d_kept


SUMS_MAX = [("all", 1, 40), ("every22", 3, 12), ("sparse", 16, 6)]


@pytest.mark.parametrize("keep,c,gib", SUMS_MAX, ids=[f"{k}-C{c}" for k, c, _ in SUMS_MAX])
def test_variant_sums_n_max_mfma(keep, c, gib):
    """N_MAX, V = 5, the matrix-core shape: 2^24 tiles strided over by the grid's 2 048 blocks, the kept-rank lookup up to sample
    2^31 - 2.  All samples with C = 1 (16 GiB of values and 16 GiB for the reference's int64 copy: needs 40 GiB); every 22nd sample
    with C = 3 (a view of 4-wide rows; needs 12 GiB); the sparse list with C = 16 (needs 6 GiB).  (R = 2^29 is a multiple of the
    tile, so no tile is moved back here; test_variant_sums_n_mid has that.)"""
    need_gib(gib)
    assert VP.tiles(N_MAX) == 1 << 24
    run_sums_n_max(keep, c, 5, "mfma", 151)


SUMS_MAX_GENERAL = [("every22", 3, 2, 12), ("sparse", 16, 2, 6), ("all", 1, 1, 40)]


@pytest.mark.parametrize("keep,c,v,gib", SUMS_MAX_GENERAL, ids=[f"{k}-C{c}-V{v}" for k, c, v, _ in SUMS_MAX_GENERAL])
def test_variant_sums_n_max_general(keep, c, v, gib):
    """N_MAX, GENERAL: every 22nd sample (C = 3) and the sparse list (C = 16) with V = 2, and all samples once with V = 1 and C = 1.
    GENERAL gives a (row, column) to one wave, which walks the row's 2^29 bytes whatever the keep set is, so each call is bound by
    that one walk's latency, as test_long_rows_tables_gpu.py::test_pair_stats is at N_MAX.  Measured on an MI355X (two runs): the
    all-samples call takes 9.1 s; the calls with a list look every sample up in the kept mask and take 17.4 - 17.9 s (every 22nd) and
    12.6 - 12.8 s (sparse).
    Needs 40 GiB with all samples, else 12 and 6 GiB."""
    need_gib(gib)
    run_sums_n_max(keep, c, v, "general", 152)


# ---- c. far Gram outputs, grid strides, far tables -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_gram_wide_pitch(kernel):
    """N = 300, a = (3, 130), b = (80, 70), V = 75, out_stride = 2^22 + 3 doubles: the last output row starts at byte
    129 * (2^22 + 3) * 8 > 2^32 (a byte offset cut to 32 bits shows here; the entry index stays near 2^29, and an index cut to 32
    bits shows in test_gram_full_square_past_2_32_entries).  Three calls into one buffer: the default plan (one slice: stores); PGENHIP_KNOB_GRAM_SLICES = 2
    (hipMemset2DAsync at a 32-MiB pitch, which must clear 70 doubles per row and not one more, then atomics); ACCUMULATE on top
    (twice the sums).  Needs 5 GiB."""
    need_gib(5)
    n, v, a, b = 300, 75, (3, 130), (80, 70)
    stride = (1 << 22) + 3
    assert (a[1] - 1) * stride * 8 > 1 << 32
    slices = GP.general_slices if kernel == "general" else GP.mfma_slices
    assert slices(v, a[1], b[1]) == 1 and slices(v, a[1], b[1], forced=2) == 2
    recs = Records(n, v, 160)
    order, kw, at = select(recs, "stride")
    t = int_tables(v, 160)
    d_t = torch.from_numpy(t).to(DEV)
    want = LR.gram_ranges([recs.rec(j) for j in order], n, None, t, a, b)
    buf, front, nbytes, out = gram_out(a, b, stride)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for step, knob, accumulate, scale in (("default plan", 0, False, 1), ("two slices", 2, False, 1), ("two slices, ACCUMULATE", 2, True, 2)):
            eng.tune(_capi.KNOB_GRAM_SLICES, knob)
            gram_call(eng, kw, at, v, d_t, a, b, out, stride, GRAM[kernel], accumulate)
            check_gram_out(buf, front, nbytes, out, stride, a, b, want * scale, f"gram wide pitch {kernel}, {step}", slab_rows=8)
    del buf, out, recs


def check_full_square(out, z, scale, what):
    """``out``: the (K, K) float64 matrix; ``z``: (V, K) float64 table values (small integers).  Every entry, 512 a-ranks at a time,
    against ``scale`` times Z^T Z (exact: every partial sum is an integer below 2^53)."""
    k = z.shape[1]
    tiles_b = -(-k // GP.TILE)
    for a0 in range(0, k, 512):
        a1 = min(k, a0 + 512)
        want = (z[:, a0:a1].T @ z) * scale
        i = LR._first_diff(out[a0:a1], want)
        if i is not None:
            entry = a0 * k + i
            ia, l = entry // k, entry % k
            raise AssertionError(f"{what}: entry {entry} = {entry:#x} (byte {8 * entry:#x}; a rank {ia}, b rank {l}, tile "
                                 f"{(ia // GP.TILE) * tiles_b + l // GP.TILE}): got {float(out.reshape(-1)[entry])!r}, want "
                                 f"{float(want.reshape(-1)[i])!r} (an index cut to 32 bits sends entry 2^32 + x to entry x; a tile or "
                                 "pair block that no block strides to keeps the prefill)")


@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_gram_full_square_past_2_32_entries(kernel):
    """N = K = 65 600, all samples, the full square, V = 33: 34.4 GB of output, pre-filled with 0x01 bytes, entry indices past 2^32,
    1 025^2 tiles and 2^24 pair blocks over the grid's 2^20: both grid-stride loops run.  GENERAL: one overwrite.  MFMA: an overwrite
    at the default plan (one slice: stores across the tile stride), an overwrite with the slices forced to 2 (a 34-GB memset, then
    atomics from 2^21 blocks), ACCUMULATE on top (twice the sums).  Every entry is compared on the device.  Needs 40 GiB."""
    need_gib(40)
    n, v = 65_600, 33
    k = n
    assert k * k > 1 << 32
    assert GP.mfma_tiles(k, k) == 1025 ** 2 > GP.MAX_GRID_TILES and GP.general_pair_blocks(k, k) > GP.MAX_GRID_TILES
    assert GP.mfma_slices(v, k, k) == 1 and GP.mfma_slices(v, k, k, forced=2) == 2 and GP.general_slices(v, k, k) == 1
    recs = Records(n, v, 170)
    t = int_tables(v, 170)
    d_t = torch.from_numpy(t).to(DEV)
    z = torch.stack([d_t[j][LR.codes(recs.rec(j), 0, n).to(torch.int64)] for j in range(v)])   # (V, K)
    nbytes = 8 * k * k
    buf, front = LR.framed(nbytes, DEV, align=8)
    buf[front: front + nbytes].fill_(0x01)
    out = buf[front: front + nbytes].view(torch.float64)
    order, kw, at = select(recs, "stride")
    steps = (("default plan", 0, False, 1),) if kernel == "general" else \
        (("default plan", 0, False, 1), ("two slices", 2, False, 1), ("two slices, ACCUMULATE", 2, True, 2))
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for step, knob, accumulate, scale in steps:
            eng.tune(_capi.KNOB_GRAM_SLICES, knob)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gram_call(eng, kw, at, v, d_t, (0, k), (0, k), out, k, GRAM[kernel], accumulate)
            what = f"gram K = {k} {kernel}, {step}"
            print(f"{what}: the call took {time.perf_counter() - t0:.2f} s")
            assert frame_ok(buf, front, nbytes), f"{what}: bytes outside the matrix were written"
            check_full_square(out.view(k, k), z, scale, what)
    del buf, out, recs, z


def test_gram_far_tables():
    """N = 70, all samples, V = 2^27 + 5 rows gathered through d_variant_idx from 64 distinct random records (the last row is record
    63), 4.3 GB of code_values: the tables of rows past 2^27 are 4 GiB and more from d_code_values, and with the default plan's
    slices (128 for MFMA, 102 for GENERAL) V * slice passes 2^32.  GENERAL and MFMA.  Expected: int64 sums over slabs of 2^22 rows of
    Z^T Z, Z = the row's table looked up by codes[idx].  Needs 12 GiB."""
    need_gib(12)
    n, distinct, v = 70, 64, (1 << 27) + 5
    a = b = (0, n)
    assert 4 * (v - 1) * 8 > 1 << 32
    for slices in (GP.mfma_slices(v, n, n), GP.general_slices(v, n, n)):
        assert slices > 32 and v * (slices - 1) > 1 << 32
    recs = Records(n, distinct, 180)
    g = torch.Generator(device=DEV)
    g.manual_seed(180)
    idx = torch.randint(0, distinct, (v,), dtype=torch.int32, device=DEV, generator=g)
    idx[-1] = distinct - 1
    t8 = torch.randint(-8, 9, (v, 4), dtype=torch.int8, device=DEV, generator=g)
    d_t = t8.to(torch.float64)
    assert d_t.numel() * 8 > 1 << 32
    codes = torch.stack([LR.codes(recs.rec(j), 0, n) for j in range(distinct)]).to(torch.int64)   # (64, N)
    want = torch.zeros((n, n), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo in range(0, v, 1 << 22):
        hi = min(v, lo + (1 << 22))
        c = codes[idx[lo:hi].long()]                                    # (slab, N)
        z = torch.gather(t8[lo:hi].to(torch.int64), 1, c)               # Z[j, s] = t_j[code of sample s in row j]
        del c
        zf = z.to(torch.float64)
        del z
        if (hi - lo) % 1024 == 0:   # Z^T Z as a batch of 1 024-row products (one product of 2^22 x 70 is a single slow tile)
            zb = zf.view(-1, 1024, n)
            want += torch.bmm(zb.transpose(1, 2), zb).to(torch.int64).sum(dim=0)   # exact: at most 64 * 2^10 per product
        else:
            want += (zf.T @ zf).to(torch.int64)
        del zf
    torch.cuda.synchronize()
    print(f"gram far tables: the reference took {time.perf_counter() - t0:.2f} s")
    stride = n + 3
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for kernel in ("general", "mfma"):
            buf, front, nbytes, out = gram_out(a, b, stride)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.sample_gram(recs.buf, recs.stride, idx, v, code_values=d_t, a=a, b=b, out=out, out_stride=stride, kernel=GRAM[kernel], records_offset=1)
            eng.wait()
            what = f"gram far tables {kernel}"
            print(f"{what}: the call took {time.perf_counter() - t0:.2f} s")
            check_gram_out(buf, front, nbytes, out, stride, a, b, want, what)
            del buf, out
    del recs, idx, t8, d_t
