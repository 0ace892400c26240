"""The far end of the ABI's index ranges for the four table-shaped entry points: pgenhip_pack_records, pgenhip_sample_scores,
pgenhip_pair_stats and pgenhip_sample_pair_stats on rows of up to 2^31 - 1 samples, on launches of more than 2^32 work items and
into outputs of more than 4 GiB (pair indices past 2^28 and 2^32, score indices past 2^32), against the slab-wise torch reference
of longrow_ref.py (held against the numpy references by test_longrow_ref.py).  The levels, the three keep sets (all samples, 4 099
spread over the range, every 22nd) and the records (random bytes, row 0 at byte 1, stride R + 1) are test_long_rows_gpu.py's.

Every output sits in a sentinel frame that must come back untouched; a case is skipped only when the card has less free memory
than the case states.  Scores use small integer weights and miss values, so every sum is an integer and the comparison is exact.
The outputs past 4 GiB are compared entry for entry on the device: the sample-pair square against a one-hot sum over its three
rows, the windowed pair tables against the closed form of periodic rows (selected row j = record j mod 45; longrow_ref.PERIOD).
"""
import numpy as np
import pytest
import torch

import longrow_ref as LR
import pair_ref as PR
import pgen_rs_amd
from pgen_rs_amd import _capi
from longrow_ref import GIB, SENT, frame_ok, need_gib
from test_long_rows_gpu import N_HALF, N_MAX, N_MID, Records, kept_of, select

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEVELS = {"N_MID": N_MID, "N_MAX": N_MAX}
KEEPS = ["all", "sparse", "every22"]
SENT_I32 = 0xA5A5A5A5 - (1 << 32)
REVERSED = (3, 2, 1, 0)


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def framed(nbytes: int, align: int = 1):
    return LR.framed(nbytes, DEV, align)


# ---- a. packed records ----------------------------------------------------------------------------------------------------------------
PACK = {"auto": _capi.PACK_AUTO, "general": _capi.PACK_GENERAL, "dense": _capi.PACK_DENSE, "gather": _capi.PACK_GATHER}


def pack_call(eng, kw, at, v, buf, front, pitch, shape, code_map):
    if at is None:
        eng.pack_records(out=buf, out_offset=front, out_stride=pitch, code_map=code_map, shape=PACK[shape], n_variants=v, **kw)
    else:
        eng.pack_records_at(at[0], at[1], out=buf, out_offset=front, out_stride=pitch, code_map=code_map, shape=PACK[shape], n_variants=v)
    eng.wait()


def check_pack(buf, front, pitch, rk, rows_sel, check_rows, n, d_kept, code_map, what):
    v = len(rows_sel)
    total = (v - 1) * pitch + rk
    assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
    out = buf[front: front + total]
    assert LR.padding_untouched(out, v, rk, pitch, SENT), f"{what}: padding between rows was written"
    for j in check_rows:
        bad = LR.check_packed(out[j * pitch: j * pitch + rk], rows_sel[j], n, d_kept, code_map)
        assert bad is None, (f"{what}: row {j} differs first at rank {bad[0]} = row byte {bad[0] >> 2} ({bad[0] >> 2:#x}), output byte "
                             f"{j * pitch + (bad[0] >> 2):#x}, work item {j * rk + (bad[0] >> 2):#x}: got {bad[1]}, want {bad[2]}")


def run_pack(n, v, keep, shapes_maps, source="stride", seed=80, pad=13, check_rows=None):
    kept = kept_of(n, keep)
    recs = Records(n, v, seed)
    order, kw, at = select(recs, source)
    rows_sel = [recs.rec(j) for j in order]
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        rk = eng.packed_record_size
        assert rk == (LR.kept_count(n, kept) + 3) // 4
        pitch = rk + pad
        for shape, code_map in shapes_maps:
            buf, front = framed((len(order) - 1) * pitch + rk)
            pack_call(eng, kw, at, len(order), buf, front, pitch, shape, code_map)
            check_pack(buf, front, pitch, rk, rows_sel, range(len(order)) if check_rows is None else check_rows, n, d_kept, code_map,
                       f"pack N={n} V={len(order)} {keep} {source} {shape} map {code_map}")
            del buf
    del recs, rows_sel, d_kept


def pack_shapes(keep):
    return ("auto", "general", "dense") if keep == "all" else ("auto", "general", "gather")


@pytest.mark.parametrize("source", ["stride", "gather", "at"])
@pytest.mark.parametrize("keep", KEEPS)
def test_pack_records_n_mid(keep, source):
    """N_MID, V = 5, every row source: AUTO, GENERAL and DENSE (all samples) or GATHER (the two lists), each with the identity map and
    with [3, 2, 1, 0]; rows at an odd address with a pitch of R_K + 13.  Needs 1 GiB."""
    need_gib(1)
    run_pack(N_MID, 5, keep, [(s, m) for s in pack_shapes(keep) for m in (None, REVERSED)], source)


PACK_MAX = [("all", "dense", None), ("all", "general", REVERSED), ("every22", "gather", REVERSED), ("every22", "general", None),
            ("sparse", "auto", REVERSED)]


@pytest.mark.parametrize("keep,shape,code_map", PACK_MAX, ids=[f"{k}-{s}" for k, s, _ in PACK_MAX])
def test_pack_records_n_max(keep, shape, code_map):
    """N_MAX, V = 3: DENSE and GENERAL with all samples (rows of 2^29 bytes: DENSE cuts each into 131 073 parts of 256 chunks, and its
    row-relative int32 arithmetic meets R = 2^29), GATHER and GENERAL with every 22nd sample, AUTO with the sparse list.  Needs 5 GiB."""
    need_gib(5)
    run_pack(N_MAX, 3, keep, [(shape, code_map)], "stride", seed=81)


@pytest.mark.parametrize("shape", ["general", "dense"])
def test_pack_records_past_2_32_items_all_samples(shape):
    """N_MAX, all samples, V = 9: 4.8 GB in, 4.8 GB out, V x R_K = 9 x 2^29 output bytes: GENERAL's `total` is above 2^32 and it divides in
    64 bits.  Work item 2^32 is byte 0 of row 8, the last row: rows 0, 7 and 8 are checked whole (row 9 does not exist).
    Needs 12 GiB."""
    need_gib(12)
    n, v = N_MAX, 9
    rk = (n + 3) // 4
    j = (1 << 32) // rk
    assert v * rk > 1 << 32 and j == v - 1
    run_pack(n, v, "all", [(shape, None)], "stride", seed=82, pad=0 if shape == "dense" else 13, check_rows=sorted({0, j - 1, j, v - 2, v - 1}))


def test_pack_records_past_2_32_items_gather():
    """GATHER at N = 2^30 + 6 with every other sample kept (K = 2^29 + 3, Q = 2^25 + 1 output dwords per row) and V = 129: V x Q is above
    2^32, so the kernel divides in 64 bits.  34.6 GB of dense synthetic records, 17.3 GB out.  Work item 2^32 is in row 127: rows 0,
    126, 127 and 128 (the last two) are checked whole.  Needs 60 GiB."""
    need_gib(60)
    n, v = N_HALF, 129
    kept = np.arange(0, n, 2, dtype=np.uint32)
    k = int(kept.size)
    q, rk, r = (k + 15) // 16, (k + 3) // 4, LR.rsize(n)
    assert k == (1 << 29) + 3 and q == (1 << 25) + 1 and v * q > 1 << 32
    j = (1 << 32) // q
    assert j == 127
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        del kept
        assert eng.packed_record_size == rk
        recs = eng.synth_records(v, dirty_pad=True)
        buf, front = framed(v * rk)
        eng.pack_records(recs, n_variants=v, out=buf, out_offset=front, shape=_capi.PACK_GATHER)
        eng.wait()
        rows_sel = [recs[i * r: (i + 1) * r] for i in range(v)]
        check_pack(buf, front, rk, rk, rows_sel, sorted({0, j - 1, j, j + 1, v - 2, v - 1}), n, d_kept, None, "pack GATHER past 2^32 items")
    del buf, recs, rows_sel, d_kept


# ---- b. per-sample scores -------------------------------------------------------------------------------------------------------------
def run_scores(n, v, keep, c, accumulate, source="stride", seed=90):
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    recs = Records(n, v, seed)
    order, kw, at = select(recs, source)
    rows_sel = [recs.rec(j) for j in order]
    rng = np.random.default_rng(seed + c)
    weights = rng.integers(-8, 9, size=(len(order), c))
    miss = rng.integers(0, 4, size=len(order))
    d_w = torch.from_numpy(weights.astype(np.float32)).to(DEV)
    d_m = torch.from_numpy(miss.astype(np.float32)).to(DEV)
    prefill = -1000 if accumulate else 0
    buf, front = framed(8 * k * c, align=8)
    out = buf[front: front + 8 * k * c].view(torch.float64)
    if accumulate:
        out.fill_(float(prefill))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        if at is None:
            eng.sample_scores(kw["records"], d_w, record_stride=kw["record_stride"], variant_idx=kw.get("variant_idx"), miss=d_m, out=out,
                              accumulate=accumulate, n_variants=len(order), records_offset=kw["records_offset"])
        else:
            eng.sample_scores_at(at[0], at[1], d_w, miss=d_m, out=out, accumulate=accumulate, n_variants=len(order))
        eng.wait()
    what = f"scores N={n} V={len(order)} {keep} {source} C={c} accumulate={accumulate}"
    assert frame_ok(buf, front, 8 * k * c), f"{what}: bytes outside the scores were written"
    bad = LR.check_scores(out, rows_sel, n, LR.as_kept(kept, DEV), weights, miss, prefill, slab=1 << 25)
    assert bad is None, (f"{what}: rank {bad[0]} column {bad[1]} (score index {bad[0] * c + bad[1]} = {bad[0] * c + bad[1]:#x}): "
                         f"got {bad[2]!r}, want {bad[3]!r}")
    del buf, out, recs, rows_sel


@pytest.mark.parametrize("c", [1, 4, 8])
@pytest.mark.parametrize("keep", KEEPS)
def test_sample_scores_n_mid(keep, c):
    """N_MID, V = 5, C = 1, 4, 8 (4, 2 and 1 record bytes per lane), every row source; the gathered call accumulates onto -1000.
    Needs 2 GiB."""
    need_gib(2)
    for source in ("stride", "gather", "at"):
        run_scores(N_MID, 5, keep, c, source == "gather", source)


SCORES_MAX = [("all", 1, False), ("all", 2, True), ("every22", 3, False), ("every22", 8, False), ("sparse", 8, False)]


@pytest.mark.parametrize("keep,c,accumulate", SCORES_MAX, ids=[f"{k}-C{c}" for k, c, _ in SCORES_MAX])
def test_sample_scores_n_max(keep, c, accumulate):
    """N_MAX, V = 5.  All samples: C = 1 (16 GiB of scores) and C = 2 (32 GiB: the score index k * C + c passes 2^32; ACCUMULATE onto
    -1000); every 22nd sample with C = 3 and C = 8 and the sparse list with C = 8 walk the mask and kept-before tables up to sample
    2^31 - 2.  Needs 16 GiB x C + 8 with all samples, else 12 GiB."""
    n = N_MAX
    need_gib(16 * c + 8 if keep == "all" else 12)
    run_scores(n, 5, keep, c, accumulate, "stride", seed=91)


# ---- c. windowed pair tables and r^2 --------------------------------------------------------------------------------------------------
def pair_out(mode, n_left, w):
    """-> (framed buffer, front, the output tensor): 16-byte aligned tables or 4-byte aligned r^2, every entry the sentinel."""
    nbytes = (64 if mode == "table" else 4) * n_left * w
    buf, front = framed(nbytes, align=16)
    return buf, front, buf[front: front + nbytes].view(torch.int32 if mode == "table" else torch.float32)


def put_code(rec: torch.Tensor, sample: int, code: int):
    byte = rec[sample >> 2: (sample >> 2) + 1]
    sh = 2 * (sample & 3)
    byte.copy_((byte & (0xFF ^ (3 << sh))) | (code << sh))


@pytest.mark.parametrize("mode", ["table", "r2"])
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("level", ["N_MID", "N_MAX"])
def test_pair_stats(level, keep, mode):
    """V = 5, W = 4 (all ten pairs) at N_MID and N_MAX: row 1 all het and row 3 all missing, so cells reach K (2^31 - 1 with all
    samples: a signed or 16-bit partial sum shows); rows 0, 2 and 4 random.  Tables exact, r^2 within one ulp of r2_of_table.
    One launch at N_MAX walks a pair's 2^31 samples in a single wave and takes about 16 s whatever V is.  Needs 6 GiB."""
    n = LEVELS[level]
    need_gib(6)
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    v, w = 5, 4
    recs = Records(n, v, 100 + len(keep))
    recs.rec(1).fill_(0x55)
    recs.rec(3).fill_(0xFF)
    d_kept = LR.as_kept(kept, DEV)
    want = {(i, j): LR.pair_table(recs.rec(i), recs.rec(j), n, d_kept) for i in range(v) for j in range(i + 1, v)}
    assert want[(1, 3)][1][3] == k and all(sum(map(sum, t)) == k for t in want.values())
    buf, front, out = pair_out(mode, v, w)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        fn = eng.pair_tables if mode == "table" else eng.pair_r2
        fn(recs.buf, recs.stride, n_variants=v, window=w, out=out, records_offset=1)
        eng.wait()
    what = f"pair_stats {level} {keep} {mode}"
    assert frame_ok(buf, front, out.numel() * 4), f"{what}: bytes outside the entries were written"
    got = out.cpu().numpy().reshape((v, w, 16) if mode == "table" else (v, w))
    for i in range(v):
        for d in range(1, w + 1):
            if i + d >= v:
                assert (got[i, d - 1].view(np.uint32) == 0xA5A5A5A5).all(), f"{what}: entry ({i}, {i + d}) does not exist and was written"
            elif mode == "table":
                t = [x for row in want[(i, i + d)] for x in row]
                assert got[i, d - 1].view(np.uint32).tolist() == t, f"{what}: pair ({i}, {i + d}): got {got[i, d - 1].view(np.uint32).tolist()}, want {t}"
            else:
                x = LR.r2_of_table(want[(i, i + d)])
                assert PR.r2_close(got[i, d - 1], x), f"{what}: pair ({i}, {i + d}) r^2 {got[i, d - 1]!r}, want {x!r} from {want[(i, i + d)]}"
    del buf, out, recs, d_kept


def test_pair_r2_terms_near_2_64():
    """The targeted r^2 case: N_MAX, all samples, V = 2, W = 1, two rows that are hom-alt everywhere except one het call in row 0 and
    two het and two hom-ref calls in row 1.  n * Sxx and Sx^2 are both within 2^35 of 2^64 (which leaves room for one het call in row
    0 and no more) and differ by 2^31 - 2, so a term that wraps, or goes through a double too early, changes the result.  Expected:
    r2_of_table on the exact integers.  Needs 3 GiB."""
    n = N_MAX
    need_gib(3)
    recs = Records(n, 2, 110)
    recs.buf.fill_(0xAA)   # hom-alt, pad bits of the last byte dirty
    put_code(recs.rec(0), 5, 1)
    for sample, code in ((5, 1), (1000, 1), (1 << 30, 0), (n - 1, 0)):
        put_code(recs.rec(1), sample, code)
    table = LR.pair_table(recs.rec(0), recs.rec(1), n)
    assert table == [[0, 0, 0, 0], [0, 1, 0, 0], [2, 1, n - 4, 0], [0, 0, 0, 0]]
    sx, sxx = 2 * (n - 1) + 1, 4 * (n - 1) + 1
    assert 0 < (1 << 64) - n * sxx < 1 << 35 and 0 < (1 << 64) - sx * sx < 1 << 35 and n * sxx - sx * sx == n - 1
    want = LR.r2_of_table(table)
    assert 0.0 < want < 1.0
    buf, front, out = pair_out("r2", 1, 1)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.pair_r2(recs.buf, recs.stride, n_variants=2, n_left=1, window=1, out=out, records_offset=1)
        eng.wait()
    assert frame_ok(buf, front, 4), "bytes outside the entry were written"
    got = out.cpu().numpy()[0]
    assert PR.r2_close(got, want), f"r^2 {got!r}, want {want!r} (n = {n}, Sx = {sx}, Sxx = {sxx}: n Sxx = {n * sxx:#x}, Sx^2 = {sx * sx:#x})"
    del buf, out, recs


def periodic_case():
    """-> (d_records, stride, offset, the (P, P, 16) int64 tables of its P = 45 distinct rows, N, the kept list): N = 11 with 7 kept."""
    n, p = 11, LR.PERIOD
    kept = np.array([0, 1, 3, 4, 6, 9, 10], dtype=np.uint32)
    r = LR.rsize(n)
    recs = np.random.default_rng(45).integers(0, 256, size=(p, r), dtype=np.uint8)
    codes_p = PR.unpack(recs, n, kept)
    assert len({c.tobytes() for c in codes_p}) == p
    buf = np.zeros(1 + p * (r + 2) + 16, dtype=np.uint8)
    for j in range(p):
        buf[1 + j * (r + 2): 1 + j * (r + 2) + r] = recs[j]
    return torch.from_numpy(buf).to(DEV), r + 2, 1, LR.periodic_tables(codes_p), n, kept


PAIR_BIG = [("table", 16_400), ("r2", 65_600)]


@pytest.mark.parametrize("grid", ["default-grid", "256-blocks"])
@pytest.mark.parametrize("mode,v", PAIR_BIG, ids=[m for m, _ in PAIR_BIG])
def test_pair_stats_output_past_4_gib(mode, v, grid):
    """V = n_left = W = 16 400 as tables (the last pair index is above 2^28: table word indices and byte offsets past 2^32) and
    V = n_left = W = 65 600 as r^2 (the last pair index is above 2^32); 17.2 GB of output each.  N = 11 with 7 kept; selected row j is
    record j mod 45 through d_variant_idx, so every written entry has the closed form tab[i % 45][(i + d) % 45] and is compared on
    the device, slab by slab; entries with i + d >= V must keep the sentinel (pgen_hip.h: not touched).  Once at the default grid, once
    with PGENHIP_KNOB_PAIR_BLOCKS = 256 (each block strides over thousands of tiles).  Needs 20 GiB."""
    need_gib(20)
    w = v
    per = 16 if mode == "table" else 1
    assert (v - 1) * w * per > 1 << 32 and (mode == "table" or (v - 2) * w > 1 << 32) and (v - 2) * w > 1 << 28
    d_recs, stride, off, tab, n, kept = periodic_case()
    vidx = (torch.arange(v, device=DEV) % LR.PERIOD).to(torch.int32)
    buf, front, out = pair_out(mode, v, w)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        if grid != "default-grid":
            eng.tune(_capi.KNOB_PAIR_BLOCKS, 256)
        fn = eng.pair_tables if mode == "table" else eng.pair_r2
        fn(d_recs, stride, vidx, v, n_left=v, window=w, out=out, records_offset=off)
        eng.wait()
    what = f"pair_stats {mode} V = W = {v} {grid}"
    assert frame_ok(buf, front, out.numel() * 4), f"{what}: bytes outside the entries were written"
    rows = 512 if mode == "table" else 1024
    if mode == "table":
        d_tab = torch.from_numpy(tab.astype(np.int32)).to(DEV)
        got = out.view(v, w, 16)
    else:
        r2 = np.array([[LR.r2_of_table(t.reshape(4, 4)) for t in row] for row in tab], dtype=np.float32)
        d_val = torch.from_numpy(r2.view(np.int32).copy()).to(DEV)
        d_ulp = torch.from_numpy(np.where(np.isnan(r2), 0, np.spacing(r2)).astype(np.float32)).to(DEV)
        got = out.view(v, w)
    for i0 in range(0, v, rows):
        i1 = min(v, i0 + rows)
        if mode == "table":
            ok = (got[i0:i1] == LR.periodic_expected(d_tab, i0, i1, w, v, SENT_I32)).all(dim=2)
        else:
            want_bits = LR.periodic_expected(d_val, i0, i1, w, v, SENT_I32)
            want = want_bits.view(torch.float32)
            g = got[i0:i1]
            ok = (g.view(torch.int32) == want_bits) | (torch.isnan(g) & torch.isnan(want)) | \
                ((g - want).abs() <= LR.periodic_expected(d_ulp, i0, i1, w, v, 0.0))
        if not bool(ok.all()):
            i, d = (int(x) for x in torch.nonzero(~ok)[0])
            i += i0
            p = i * w + d
            raise AssertionError(f"{what}: pair ({i}, {i + d + 1}), pair index {p} = {p:#x} (word {per * p:#x}, byte {4 * per * p:#x}): got "
                                 f"{got[i, d].tolist()}, want {'the sentinel' if i + d + 1 >= v else 'tab[%d][%d]' % (i % 45, (i + d + 1) % 45)} "
                                 "(an index cut to 32 bits sends pair 2^32 + x to pair x, an offset cut to 32 bits byte 2^32 + x to byte x)")
    del buf, out, got


# ---- d. sample-pair tables -------------------------------------------------------------------------------------------------------------
SPAIR = {"general": _capi.SPAIR_GENERAL, "mfma": _capi.SPAIR_MFMA}
SPAIR_MAX = ["all-first-last", "all-last-first", "every22-last-last"]


@pytest.mark.parametrize("kernel", ["general", "mfma"])
@pytest.mark.parametrize("case", SPAIR_MAX)
def test_sample_pair_stats_n_max(case, kernel):
    """N_MAX, V = 9, GENERAL and MFMA: all samples with a = the first 70 and b = the last 70 ranks (by stride) and the two swapped
    (through _at, rows reversed); every 22nd sample with both ranges the last 70 ranks.  Sample bytes up to R - 1 = 2^29 - 1 of every
    row.  Overwrite, then ACCUMULATE on top: twice the tables.  Needs 8 GiB."""
    n, v = N_MAX, 9
    need_gib(8)
    keep, ra, rb = case.split("-")
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    rng_of = {"first": (0, 70), "last": (k - 70, 70)}
    a, b = rng_of[ra], rng_of[rb]
    recs = Records(n, v, 120)
    order, kw, at = select(recs, "at" if case == "all-last-first" else "stride")
    want = LR.sample_pair_tables([recs.rec(j) for j in order], n, LR.as_kept(kept, DEV), a, b).reshape(-1)
    assert int(want.sum()) == v * 70 * 70
    nbytes = 64 * 70 * 70
    buf, front = framed(nbytes, align=16)
    out = buf[front: front + nbytes].view(torch.int32)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for accumulate in (False, True):
            if at is None:
                eng.sample_pair_tables(kw["records"], kw["record_stride"], n_variants=v, a=a, b=b, out=out, accumulate=accumulate,
                                       kernel=SPAIR[kernel], records_offset=kw["records_offset"])
            else:
                eng.sample_pair_tables_at(at[0], at[1], v, a=a, b=b, out=out, accumulate=accumulate, kernel=SPAIR[kernel])
            eng.wait()
            what = f"sample_pair_stats N_MAX {case} {kernel} accumulate={accumulate}"
            assert frame_ok(buf, front, nbytes), f"{what}: bytes outside the tables were written"
            word = LR._first_diff(out.to(torch.int64), want * (2 if accumulate else 1))
            assert word is None, (f"{what}: word {word} (a rank {a[0] + word // 16 // 70}, b rank {b[0] + word // 16 % 70}, cell {word % 16}): "
                                  f"got {int(out[word])}, want {int(want[word]) * (2 if accumulate else 1)}")
    del buf, out, recs


def check_square(out, codes, scale, what):
    """``out``: the (K, K, 16) int32 tables of a full square; ``codes``: (V, K) int64 on the device.  Every entry, 512 a-ranks at a time:
    expected = ``scale`` times the sum over the rows of the one-hot of 4 * c[a] + c[b]."""
    k = codes.shape[1]
    cells = torch.arange(16, device=codes.device)
    for a0 in range(0, k, 512):
        a1 = min(k, a0 + 512)
        want = torch.zeros((a1 - a0, k, 16), dtype=torch.int32, device=codes.device)
        for c in codes:
            want += (4 * c[a0:a1, None] + c[None, :])[:, :, None] == cells
        i = LR._first_diff(out[a0:a1], want * scale)
        if i is not None:
            word = 16 * a0 * k + i
            raise AssertionError(f"{what}: word {word} = {word:#x} (byte {4 * word:#x}; a rank {word // 16 // k}, b rank {word // 16 % k}, cell "
                                 f"{word % 16}): got {int(out.reshape(-1)[word])}, want {int((want * scale).reshape(-1)[i])} "
                                 "(an offset cut to 32 bits adds the table at word 2^32 + x into word x)")


@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_sample_pair_stats_output_past_4_gib(kernel):
    """N = K = 16 400, the full square, V = 3 random rows: 17.2 GB of tables, pre-filled with 0x01010101, table word indices past 2^32.
    GENERAL without ACCUMULATE: the memset must clear all of it, and 2^20 + 2 336 pair blocks stride over the 2^20 grid cap.  MFMA
    without ACCUMULATE, then with it on top: twice the tables.  Every entry is compared on the device.  Needs 20 GiB."""
    need_gib(20)
    n, v = 16_400, 3
    recs = Records(n, v, 130)
    codes = torch.stack([LR.codes(recs.rec(j), 0, n) for j in range(v)]).to(torch.int64)
    nbytes = 64 * n * n
    assert nbytes > 4 * GIB and 16 * (n * n - 1) > 1 << 32 and (n * n + 255) // 256 > 1 << 20
    buf, front = framed(nbytes, align=16)
    out = buf[front: front + nbytes].view(torch.int32)
    out.fill_(0x01010101)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for accumulate in (False, True) if kernel == "mfma" else (False,):
            eng.sample_pair_tables(recs.buf, recs.stride, n_variants=v, out=out, accumulate=accumulate, kernel=SPAIR[kernel], records_offset=1)
            eng.wait()
            what = f"sample_pair_stats K = {n} {kernel} accumulate={accumulate}"
            assert frame_ok(buf, front, nbytes), f"{what}: bytes outside the tables were written"
            check_square(out.view(n, n, 16), codes, 2 if accumulate else 1, what)
    del buf, out, recs, codes
