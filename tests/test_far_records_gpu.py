"""Records whose byte offset from d_records / d_base is 2^32 or more, through every entry point that selects rows and every kernel
that takes the shape (the per-variant counts have test_genotype_counts_gpu.py::test_row_past_4_gib).

One shared buffer of 2^32 + 4 099 + 8 * R_max + 64 bytes: random bytes in its first MiB (the near rows, and the place every far
offset lands on when it is cut to 32 bits: a wrong record, read in bounds) and from 64 bytes before FAR to its end (the far rows).
Each call mixes near and far rows through (i) d_variant_idx with record_stride = FAR, (ii) a small stride with d_variant_idx values
near FAR / stride, (iii) d_record_off; the packed-record, score, pair-table and sample-pair-table entry points also take (iv) two
rows by stride alone, FAR bytes apart.  Expected bytes: the CPU oracle and the numpy references on the few records involved.  The Gram
matrix, the per-variant sums and the Gram product take integer tables, values and Q, so their FP64 results are compared exactly.
test_sample_scores_far_weights does the same for the other pointer a kernel offsets by a row number: d_weights.

The kernels that cannot gather (RUNS, the pick family's packed path, the line-run kernel) get dense records that cross 2^32
themselves, 70 GB of text each, checked as test_gt_parity_gpu.py::test_gt_segments_past_4_gib checks: a line feed at the end of
every row (on the device), sentinels behind the last row, windows of 100 rows against the oracle at the start, around the row whose
record holds byte 2^32, at the end and at six seeded places.  pgenhip_pack_records DENSE gets the same 4.32 GB in and out.
"""
import numpy as np
import pytest
import torch

import gapply_ref as AR
import gram_ref as GR
import longrow_ref as LR
import matrix_ref as MR
import pack_ref as PK
import pair_ref as PR
import pgen_oracle as oracle
import pgen_rs_amd
import score_ref as SCR
import spair_ref as SPR
import subset_plan as SP
import vsum_ref as VR
from pgen_rs_amd import _capi
from test_gram_apply_gpu import int_q
from test_sample_gram_gpu import int_tables
from test_variant_sums_gpu import int_values

pytestmark = pytest.mark.gpu

from longrow_ref import BACK, GIB, SENT, need_gib

DEV = "cuda:0"
FAR = (1 << 32) + 4099
R_MAX = MR.rsize(20_000)
NEAR_BYTES = 1 << 20
FAR_LO = FAR - 64
BUF_BYTES = FAR + 8 * R_MAX + 64


class FarBuffer:
    def __init__(self):
        g = torch.Generator(device=DEV)
        g.manual_seed(4099)
        self.dev = torch.empty(BUF_BYTES, dtype=torch.uint8, device=DEV)
        self.dev[:NEAR_BYTES] = torch.randint(0, 256, (NEAR_BYTES,), dtype=torch.uint8, device=DEV, generator=g)
        self.dev[FAR_LO:] = torch.randint(0, 256, (BUF_BYTES - FAR_LO,), dtype=torch.uint8, device=DEV, generator=g)
        self.near = self.dev[:NEAR_BYTES].cpu().numpy()
        self.far = self.dev[FAR_LO:].cpu().numpy()

    def record(self, off: int, r: int) -> np.ndarray:
        """The r bytes at byte `off` of the buffer (host copy)."""
        if off + r <= NEAR_BYTES:
            return self.near[off: off + r]
        assert off >= FAR_LO and off + r <= BUF_BYTES
        return self.far[off - FAR_LO: off - FAR_LO + r]

    def records(self, offs, r: int) -> np.ndarray:
        """(V, r) records at the byte offsets; every far record differs from what its offset cut to 32 bits would read."""
        for o in offs:
            if o >= 1 << 32:
                assert not np.array_equal(self.record(o, r), self.record(o - (1 << 32), r))
        return np.stack([self.record(int(o), r) for o in offs])


@pytest.fixture(scope="module")
def far():
    need_gib(BUF_BYTES / GIB + 1)   # 5 GiB
    fb = FarBuffer()
    yield fb
    del fb
    torch.cuda.empty_cache()


def sources(n: int, plain: bool = False):
    """-> [(name, byte offsets of the rows, kwargs of a stride / gather call or None, record_off tensor or None)]: near and far rows mixed.
    ``plain`` adds two rows by stride alone (no list): bytes 3 and 3 + FAR, the only way to put a far row in front of the
    `row * record_stride` arm of a kernel."""
    r = MR.rsize(n)
    out = []
    if plain:
        out.append(("plain stride FAR", [3, 3 + FAR], dict(record_stride=FAR, records_offset=3, variant_idx=None), None))
    vidx = [0, 1, 1, 0, 1]
    out.append(("idx x FAR", [3 + i * FAR for i in vidx], dict(record_stride=FAR, records_offset=3, variant_idx=vidx), None))
    stride = r + 5
    q = -(-FAR // stride)
    vidx = [q + 1, 0, q, 1, q + 3, q + 2]
    offs = [3 + i * stride for i in vidx]
    assert max(offs) + r <= BUF_BYTES and min(o for o in offs if o > NEAR_BYTES) >= FAR
    out.append(("far idx x stride", offs, dict(record_stride=stride, records_offset=3, variant_idx=vidx), None))
    offs = [FAR + 7, 3, FAR + 9 + r, 4 + r, FAR + 6 + 3 * r]
    out.append(("record_off", offs, None, offs))
    return out


def tensors(kw, offs_at):
    if kw is not None and kw["variant_idx"] is not None:
        kw = dict(kw, variant_idx=torch.tensor(kw["variant_idx"], dtype=torch.int64, device=DEV).to(torch.int32))
    at = None if offs_at is None else torch.tensor(offs_at, dtype=torch.int64, device=DEV)
    return kw, at


def framed(nbytes: int, align: int = 1):
    return LR.framed(nbytes, DEV, align)


def payload(buf, front, nbytes, what) -> np.ndarray:
    h = buf.cpu().numpy()
    assert (h[:front] == SENT).all() and (h[front + nbytes:] == SENT).all(), f"{what}: bytes outside the output were written"
    return h[front: front + nbytes]


def first_diff(got: np.ndarray, want: np.ndarray, what: str):
    if got.shape == want.shape and (got == want).all():
        return
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    raise AssertionError(f"{what}: {bad.size} of {want.size} bytes differ, first at byte {int(bad[0])}: got {int(got.reshape(-1)[bad[0]])}, "
                         f"want {int(want.reshape(-1)[bad[0]])}")


# (N, kept samples or None, the kernels the shape must reach: plan::emit::accepts of csrc/launch_plan.h, through tests/subset_plan.py `accepts`)
EMIT_SHAPES = [(40, None, ("rows", "flat")), (300, None, ("pick", "flat", "rows")), (300, 30, ("pick", "rows")),
               (2504, None, ("wide", "pick", "rows")), (2504, 1252, ("pick", "scan", "rows")), (20_000, 2000, ("scan", "rowpick", "rows"))]


def kept_for(n: int, k):
    return None if k is None else np.sort(np.random.default_rng(n + k).choice(n, size=k, replace=False)).astype(np.uint32)


@pytest.mark.parametrize("n,k,must", EMIT_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k, _ in EMIT_SHAPES])
def test_emit_far_records(far, n, k, must):
    """pgenhip_decode_emit, pgenhip_decode_emit_at and pgenhip_emit_lines (10-byte prefixes), AUTO and every forced kernel id that takes the
    shape with gathered rows.  Needs 5 GiB (the shared buffer)."""
    kept = kept_for(n, k)
    kk = n if kept is None else k
    r, row = MR.rsize(n), 4 * kk + 1
    rng = np.random.default_rng(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for mode in ("segments", "lines"):
            ids = [(name, kid) for name, kid in SP.KERNEL_IDS.items()
                   if SP.accepts(kid, n, kk, kept is not None, bound=10, gather=True, mode=mode)]
            names = {name for name, _ in ids}
            assert "auto" in names and set(must) - {"flat"} <= names and (mode == "lines" or set(must) <= names), (mode, names)
            for sname, offs, kw, offs_at in sources(n):
                if mode == "lines" and kw is None:
                    continue   # (pgenhip_emit_lines has no byte-offset form)
                v = len(offs)
                recs = far.records(offs, r)
                want_gt = oracle.decode_emit(recs.reshape(-1), v, n, kept_idx=kept).reshape(v, row)
                kw_t, at_t = tensors(kw, offs_at)
                if mode == "lines":
                    blob = rng.integers(33, 127, size=10 * v, dtype=np.uint8)
                    poff = np.arange(v + 1, dtype=np.int64) * 10
                    loff = np.arange(v + 1, dtype=np.int64) * (10 + row)
                    want = np.concatenate([blob.reshape(v, 10), want_gt], axis=1).reshape(-1)
                    d_blob, d_poff, d_loff = (torch.from_numpy(x).to(DEV) for x in (blob, poff, loff))
                else:
                    want = want_gt.reshape(-1)
                for name, kid in ids:
                    buf, front = framed(want.size)
                    if mode == "lines":
                        eng.emit_lines(far.dev, v, d_blob, d_poff, d_loff, 10, buf[front:], record_stride=kw_t["record_stride"],
                                       variant_idx=kw_t["variant_idx"], kernel=kid, records_offset=kw_t["records_offset"])
                    elif at_t is None:
                        eng.decode_emit(far.dev, v, out=buf, out_offset=front, kernel=kid, **kw_t)
                    else:
                        eng.decode_emit_at(far.dev, at_t, v, out=buf[front:], kernel=kid)
                    eng.wait()
                    what = f"N={n} K={kk} {mode} {sname} kernel {name}"
                    first_diff(payload(buf, front, want.size, what), want, what)


COUNT_SHAPES = [(40, None), (300, 30), (2504, None), (2504, 1252), (20_000, 2000)]


@pytest.mark.parametrize("n,k", COUNT_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k in COUNT_SHAPES])
def test_sample_counts_far_records(far, n, k):
    """pgenhip_sample_counts and pgenhip_sample_counts_at: AUTO and ROWS, with and without ACCUMULATE (onto 0xFFFFFFF0).  Needs 5 GiB."""
    kept = kept_for(n, k)
    kk = n if kept is None else k
    r = MR.rsize(n)
    prefill = 0xFFFFFFF0
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n):
            codes = MR.codes(far.records(offs, r), n, kept)
            counts = np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1).astype(np.int64)
            kw_t, at_t = tensors(kw, offs_at)
            for kern in (_capi.SCOUNT_AUTO, _capi.SCOUNT_ROWS):
                for accumulate in (False, True):
                    buf, front = framed(16 * kk, align=4)
                    out = buf[front: front + 16 * kk].view(torch.int32)
                    if accumulate:
                        out.fill_(prefill - (1 << 32))
                    if at_t is None:
                        eng.sample_counts(far.dev, out=out, n_variants=len(offs), kernel=kern, accumulate=accumulate, **kw_t)
                    else:
                        eng.sample_counts_at(far.dev, at_t, len(offs), out=out, kernel=kern, accumulate=accumulate)
                    eng.wait()
                    what = f"N={n} K={kk} {sname} kernel {kern} accumulate={accumulate}"
                    got = payload(buf, front, 16 * kk, what).view(np.uint32).astype(np.int64).reshape(kk, 4)
                    want = (counts + (prefill if accumulate else 0)) & 0xFFFFFFFF
                    assert (got == want).all(), f"{what}: first differing rank {int(np.flatnonzero((got != want).any(axis=1))[0])}"


PAD = 0x5A   # fills the matrix rows and their padding before the call
MATRIX_SHAPES = [(40, None), (300, 30), (2504, None), (20_000, 2000)]


@pytest.mark.parametrize("dtype", [torch.int8, torch.float32], ids=["int8", "f32"])
@pytest.mark.parametrize("n,k", MATRIX_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k in MATRIX_SHAPES])
def test_decode_matrix_far_records(far, n, k, dtype):
    """pgenhip_decode_matrix and pgenhip_decode_matrix_at: GENERAL in both orientations, STREAM and TILE (all samples kept), AUTO; int8 and
    f32, compared as bytes.  Needs 5 GiB."""
    kept = kept_for(n, k)
    r = MR.rsize(n)
    np_dtype = np.int8 if dtype == torch.int8 else np.float32
    vals = MR.default_values(np_dtype)
    shapes = [(_capi.MATRIX_GENERAL, False), (_capi.MATRIX_GENERAL, True), (_capi.MATRIX_AUTO, False), (_capi.MATRIX_AUTO, True)]
    if kept is None:
        shapes += [(_capi.MATRIX_STREAM, False), (_capi.MATRIX_TILE, True)]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n):
            recs = far.records(offs, r)
            kw_t, at_t = tensors(kw, offs_at)
            for shape, sample_major in shapes:
                want = MR.raw(MR.matrix(recs, n, kept, vals, sample_major))
                # the output: a framed buffer, rows at a pitch of 16 bytes more than they hold, rounded up to 16 (what TILE needs)
                rows, row_bytes = want.shape
                eb = vals.itemsize
                pitch = -(-(row_bytes + 16) // 16) * 16
                buf, front = framed(rows * pitch, align=16)
                buf[front: front + rows * pitch] = PAD
                out = buf[front: front + rows * pitch].view(dtype).view(rows, pitch // eb)[:, : row_bytes // eb]
                if at_t is None:
                    eng.decode_matrix(far.dev, len(offs), sample_major=sample_major, kernel=shape, out=out, **kw_t)
                else:
                    eng.decode_matrix_at(far.dev, at_t, len(offs), sample_major=sample_major, kernel=shape, out=out)
                eng.wait()
                what = f"N={n} {'all' if k is None else k} {sname} shape {shape} sample_major={sample_major} {np_dtype.__name__}"
                h = payload(buf, front, rows * pitch, what).reshape(rows, pitch)
                assert (h[:, row_bytes:] == PAD).all(), f"{what}: row padding was written"
                got = h[:, :row_bytes]
                first_diff(got, want, what)


# ---- packed records, scores, pair tables, sample-pair tables ------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", COUNT_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k in COUNT_SHAPES])
def test_pack_records_far_records(far, n, k):
    """pgenhip_pack_records and pgenhip_pack_records_at: AUTO, GENERAL and DENSE (all samples) or GATHER (a list), the identity map and
    [3, 2, 1, 0], rows at an odd address with a pitch of R_K + 5; the padding must come back untouched.  Needs 5 GiB."""
    kept = kept_for(n, k)
    kk = n if kept is None else k
    r, rk = MR.rsize(n), (kk + 3) // 4
    pitch = rk + 5
    shapes = [_capi.PACK_AUTO, _capi.PACK_GENERAL, _capi.PACK_DENSE if kept is None else _capi.PACK_GATHER]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            recs = far.records(offs, r)
            kw_t, at_t = tensors(kw, offs_at)
            total = (v - 1) * pitch + rk
            for code_map in (None, [3, 2, 1, 0]):
                want = PK.pack(recs, n, kept, code_map)
                for shape in shapes:
                    buf, front = framed(total)
                    assert (buf.data_ptr() + front) % 2 == 1
                    if at_t is None:
                        eng.pack_records(far.dev, out=buf, out_offset=front, out_stride=pitch, code_map=code_map, shape=shape, n_variants=v, **kw_t)
                    else:
                        eng.pack_records_at(far.dev, at_t, out=buf, out_offset=front, out_stride=pitch, code_map=code_map, shape=shape, n_variants=v)
                    eng.wait()
                    what = f"N={n} K={kk} {sname} shape {shape} map {code_map}"
                    h = np.concatenate([payload(buf, front, total, what), np.full(pitch - rk, SENT, dtype=np.uint8)]).reshape(v, pitch)
                    assert (h[:, rk:] == SENT).all(), f"{what}: row padding was written"
                    first_diff(h[:, :rk], want, what)


@pytest.mark.parametrize("c", [1, 3, 8])
@pytest.mark.parametrize("n,k", COUNT_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k in COUNT_SHAPES])
def test_sample_scores_far_records(far, n, k, c):
    """pgenhip_sample_scores and pgenhip_sample_scores_at with C = 1, 3, 8 (4, 2 and 1 record bytes per lane): integer weights in
    [-8, 8] and miss values in {0..3} by position in the selection, overwrite and ACCUMULATE onto an integer prefill; every sum is an
    integer, so the scores are exact.  Needs 5 GiB."""
    kept = kept_for(n, k)
    kk = n if kept is None else k
    r = MR.rsize(n)
    rng = np.random.default_rng(n + c)
    prefill = -1000.0
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            weights = rng.integers(-8, 9, size=(v, c)).astype(np.float32)
            miss = rng.integers(0, 4, size=v).astype(np.float32)
            want, _ = SCR.score_ref(far.records(offs, r), n, weights, miss, kept)
            kw_t, at_t = tensors(kw, offs_at)
            d_w, d_m = torch.from_numpy(weights).to(DEV), torch.from_numpy(miss).to(DEV)
            for accumulate in (False, True):
                buf, front = framed(8 * kk * c, align=8)
                out = buf[front: front + 8 * kk * c].view(torch.float64)
                if accumulate:
                    out.fill_(prefill)
                if at_t is None:
                    eng.sample_scores(far.dev, d_w, miss=d_m, out=out, accumulate=accumulate, n_variants=v, **kw_t)
                else:
                    eng.sample_scores_at(far.dev, at_t, d_w, miss=d_m, out=out, accumulate=accumulate, n_variants=v)
                eng.wait()
                what = f"N={n} K={kk} C={c} {sname} accumulate={accumulate}"
                got = payload(buf, front, 8 * kk * c, what).view(np.float64).reshape(kk, c)
                exp = want + (prefill if accumulate else 0.0)
                if not np.array_equal(got, exp):
                    rank, col = np.argwhere(got != exp)[0]
                    raise AssertionError(f"{what}: rank {rank} column {col}: got {got[rank, col]!r}, want {exp[rank, col]!r}")


def test_sample_scores_far_weights():
    """Weight rows (1 << 30) + 3 floats apart, five rows: row 1's weights are 2^32 + 12 BYTES into d_weights and row 4's are 2^32 + 12
    FLOATS in.  Only the touched floats are set.  An offset cut to 32 bits lands on the first 64 floats, which hold 100, 101, ...
    (row 0's own three among them): weights no other row has.  C = 3, N = 300, near records.  Needs 24 GiB (17.2 GB of weights)."""
    need_gib(24)
    n, c, v = 300, 3, 5
    w_stride = (1 << 30) + 3
    r = MR.rsize(n)
    rng = np.random.default_rng(30)
    recs = rng.integers(0, 256, size=(v, r), dtype=np.uint8)
    weights = rng.integers(-8, 9, size=(v, c)).astype(np.float32)
    weights[0] = [100, 101, 102]
    miss = rng.integers(0, 4, size=v).astype(np.float32)
    want, _ = SCR.score_ref(recs, n, weights, miss)
    d_recs = torch.from_numpy(recs.reshape(-1).copy()).to(DEV)
    big = torch.empty((v - 1) * w_stride + c, dtype=torch.float32, device=DEV)
    assert 1 * w_stride * 4 == (1 << 32) + 12   # row 1, in bytes
    assert 4 * w_stride == (1 << 32) + 12       # row 4, in floats
    big[:64] = torch.arange(100, 164, dtype=torch.float32, device=DEV)
    d_w = torch.as_strided(big, (v, c), (w_stride, 1))
    d_w.copy_(torch.from_numpy(weights).to(DEV))
    assert d_w.stride(0) == w_stride and float(big[4 * w_stride + 2]) == weights[4, 2] and float(big[12]) == 112.0
    d_m = torch.from_numpy(miss).to(DEV)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for accumulate in (False, True):
            buf, front = framed(8 * n * c, align=8)
            out = buf[front: front + 8 * n * c].view(torch.float64)
            if accumulate:
                out.fill_(7.0)
            eng.sample_scores(d_recs, d_w, miss=d_m, out=out, accumulate=accumulate, n_variants=v)
            eng.wait()
            what = f"far weights, accumulate={accumulate}"
            got = payload(buf, front, 8 * n * c, what).view(np.float64).reshape(n, c)
            exp = want + (7.0 if accumulate else 0.0)
            if not np.array_equal(got, exp):
                rank, col = np.argwhere(got != exp)[0]
                raise AssertionError(f"{what}: rank {rank} column {col}: got {got[rank, col]!r}, want {exp[rank, col]!r} (weights of rows 1..4 are "
                                     f"{4 * w_stride:#x} bytes .. {4 * w_stride:#x} floats into d_weights)")
    del big, d_w
    torch.cuda.empty_cache()


def pair_call(eng, mode, v, n_left, w, kw_t, at_t, base, what):
    """One pgenhip_pair_stats / _at call into a framed buffer (16-byte aligned) -> the n_left * W entries as uint32 words."""
    per = 16 if mode == "table" else 1
    nbytes = 4 * per * n_left * w
    buf, front = framed(nbytes, align=16)
    out = buf[front: front + nbytes].view(torch.int32 if mode == "table" else torch.float32)
    if at_t is None:
        fn = eng.pair_tables if mode == "table" else eng.pair_r2
        fn(base, n_variants=v, n_left=n_left, window=w, out=out, **kw_t)
    else:
        fn = eng.pair_tables_at if mode == "table" else eng.pair_r2_at
        fn(base, at_t, v, n_left=n_left, window=w, out=out)
    eng.wait()
    words = payload(buf, front, nbytes, what).view(np.uint32)
    return words.reshape(n_left, w, 16) if mode == "table" else words.reshape(n_left, w)


@pytest.mark.parametrize("n,k", MATRIX_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k in MATRIX_SHAPES])
def test_pair_stats_far_records(far, n, k):
    """pgenhip_pair_stats and pgenhip_pair_stats_at, tables and r^2, n_left = V - 1, W = 1 and W = V - 1.  Needs 5 GiB."""
    kept = kept_for(n, k)
    r = MR.rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            codes = PR.unpack(far.records(offs, r), n, kept)
            kw_t, at_t = tensors(kw, offs_at)
            for w in sorted({1, v - 1}):
                want = PR.pair_tables(codes, v - 1, w, fill=-1)
                what = f"N={n} {'all' if k is None else k} {sname} W={w}"
                PR.check_tables(pair_call(eng, "table", v, v - 1, w, kw_t, at_t, far.dev, what), want, v, what + " tables")
                PR.check_r2(pair_call(eng, "r2", v, v - 1, w, kw_t, at_t, far.dev, what), want, v, what + " r^2")


SPAIR_SHAPES = [(300, 30, (0, 30), (0, 30)), (2504, None, (0, 70), (2400, 104)), (20_000, 2000, (1930, 70), (0, 65))]


@pytest.mark.parametrize("kernel", ["general", "mfma", "auto"])
@pytest.mark.parametrize("n,k,a,b", SPAIR_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k, _, _ in SPAIR_SHAPES])
def test_sample_pair_stats_far_records(far, n, k, a, b, kernel):
    """pgenhip_sample_pair_stats and pgenhip_sample_pair_stats_at: GENERAL, MFMA and AUTO over all four row sources (the MFMA kernel's
    stride, variant_idx and record_off instantiations each read a far row), overwrite and ACCUMULATE onto 0xFFFFFFF0.  Needs 5 GiB."""
    kept = kept_for(n, k)
    r = MR.rsize(n)
    kid = {"general": _capi.SPAIR_GENERAL, "mfma": _capi.SPAIR_MFMA, "auto": _capi.SPAIR_AUTO}[kernel]
    prefill = 0xFFFFFFF0
    nbytes = 64 * a[1] * b[1]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            want = SPR.ranges(SPR.unpack(far.records(offs, r), n, kept), a, b).reshape(-1)
            kw_t, at_t = tensors(kw, offs_at)
            for accumulate in (False, True):
                buf, front = framed(nbytes, align=16)
                out = buf[front: front + nbytes].view(torch.int32)
                if accumulate:
                    out.fill_(prefill - (1 << 32))
                if at_t is None:
                    eng.sample_pair_tables(far.dev, n_variants=v, a=a, b=b, out=out, accumulate=accumulate, kernel=kid, **kw_t)
                else:
                    eng.sample_pair_tables_at(far.dev, at_t, v, a=a, b=b, out=out, accumulate=accumulate, kernel=kid)
                eng.wait()
                what = f"N={n} {'all' if k is None else k} a={a} b={b} {sname} kernel {kernel} accumulate={accumulate}"
                got = payload(buf, front, nbytes, what).view(np.uint32).astype(np.int64)
                exp = (want + (prefill if accumulate else 0)) & 0xFFFFFFFF
                if not (got == exp).all():
                    word = int(np.flatnonzero(got != exp)[0])
                    raise AssertionError(f"{what}: word {word} (pair {word // 16}, cell {word % 16}): got {got[word]}, want {exp[word]}")


# ---- Gram matrix and per-variant sums: integer tables and values, exact --------------------------------------------------------------
GRAM = {"general": _capi.GRAM_GENERAL, "mfma": _capi.GRAM_MFMA, "auto": _capi.GRAM_AUTO}
VSUM = {"general": _capi.VSUM_GENERAL, "mfma": _capi.VSUM_MFMA, "auto": _capi.VSUM_AUTO}


@pytest.mark.parametrize("kernel", ["general", "mfma", "auto"])
@pytest.mark.parametrize("n,k,a,b", SPAIR_SHAPES, ids=[f"N{n}-{'all' if k is None else k}" for n, k, _, _ in SPAIR_SHAPES])
def test_sample_gram_far_records(far, n, k, a, b, kernel):
    """pgenhip_sample_gram and pgenhip_sample_gram_at: GENERAL, MFMA and AUTO over all four row sources (the MFMA kernel has its own row
    address, compiled per source: its stride, variant_idx and record_off instantiations, with and without a kept list, each read a
    far row), integer tables by position in the selection, overwrite and ACCUMULATE onto an integer prefill.  Exact.  Needs 5 GiB."""
    kept = kept_for(n, k)
    r = MR.rsize(n)
    prefill = -1000.0
    nbytes = 8 * a[1] * b[1]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            t = int_tables(v, n + v)
            codes = GR.unpack(far.records(offs, r), n, kept)
            want = GR.gram_ref(codes[:, a[0]:a[0] + a[1]], t, codes[:, b[0]:b[0] + b[1]])
            d_t = torch.from_numpy(t).to(DEV)
            kw_t, at_t = tensors(kw, offs_at)
            for accumulate in (False, True):
                buf, front = framed(nbytes, align=8)
                out = buf[front: front + nbytes].view(torch.float64)
                if accumulate:
                    out.fill_(prefill)
                if at_t is None:
                    eng.sample_gram(far.dev, n_variants=v, code_values=d_t, a=a, b=b, out=out, accumulate=accumulate, kernel=GRAM[kernel], **kw_t)
                else:
                    eng.sample_gram_at(far.dev, at_t, d_t, v, a=a, b=b, out=out, accumulate=accumulate, kernel=GRAM[kernel])
                eng.wait()
                what = f"N={n} {'all' if k is None else k} a={a} b={b} {sname} kernel {kernel} accumulate={accumulate}"
                got = payload(buf, front, nbytes, what).view(np.float64).reshape(a[1], b[1])
                exp = want + (prefill if accumulate else 0.0)
                if not np.array_equal(got, exp):
                    i, l = np.argwhere(got != exp)[0]
                    raise AssertionError(f"{what}: entry ({i}, {l}): got {got[i, l]!r}, want {exp[i, l]!r}")


@pytest.mark.parametrize("kernel", ["general", "mfma", "auto"])
@pytest.mark.parametrize("c", [1, 16])
@pytest.mark.parametrize("n,k", [(n, k) for n, k, _, _ in SPAIR_SHAPES], ids=[f"N{n}-{'all' if k is None else k}" for n, k, _, _ in SPAIR_SHAPES])
def test_variant_sums_far_records(far, n, k, c, kernel):
    """pgenhip_variant_sums and pgenhip_variant_sums_at with C = 1 and C = 16: GENERAL, MFMA and AUTO over all four row sources, integer
    values in [-8, 8].  Exact.  Needs 5 GiB."""
    kept = kept_for(n, k)
    kk = n if kept is None else k
    r = MR.rsize(n)
    v16 = int_values(np.random.default_rng(n + c), kk)
    d_v16 = torch.from_numpy(v16).to(DEV)
    vals = d_v16[:, 0].contiguous() if c == 1 else d_v16
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            want, _ = VR.vsum_ref(far.records(offs, r), n, v16[:, :c], kept)
            kw_t, at_t = tensors(kw, offs_at)
            nbytes = 8 * v * c * 4
            buf, front = framed(nbytes, align=8)
            out = buf[front: front + nbytes].view(torch.float64)
            if at_t is None:
                eng.variant_sums(far.dev, vals, out=out, flags=VSUM[kernel], n_variants=v, **kw_t)
            else:
                eng.variant_sums_at(far.dev, at_t, vals, out=out, flags=VSUM[kernel], n_variants=v)
            eng.wait()
            what = f"N={n} K={kk} C={c} {sname} kernel {kernel}"
            got = payload(buf, front, nbytes, what).view(np.float64).reshape(v, c, 4)
            if not np.array_equal(got, want):
                row, col, code = np.argwhere(got != want)[0]
                raise AssertionError(f"{what}: row {row} (record at byte {offs[row]:#x}) column {col} code {code}: got {got[row, col, code]!r}, "
                                     f"want {want[row, col, code]!r}")


GAPPLY = {"general": _capi.GAPPLY_GENERAL, "mfma": _capi.GAPPLY_MFMA, "auto": _capi.GAPPLY_AUTO}


@pytest.mark.parametrize("kernel", ["general", "mfma", "auto"])
@pytest.mark.parametrize("keep", ["all", "every7"])
def test_gram_apply_far_records(far, keep, kernel):
    """pgenhip_gram_apply and pgenhip_gram_apply_at with N = 299 and C = 13, all samples and every 7th: GENERAL, MFMA and AUTO over
    all four row sources (both passes of the MFMA shape have their own row address, compiled per source: the stride, variant_idx and
    record_off instantiations, with and without a kept list, each read a far row), integer tables by position in the selection and
    an integer Q, P and Y into sentinel frames.  Exact.  Needs 5 GiB."""
    n, c = 299, 13
    kept = None if keep == "all" else np.arange(0, n, 7, dtype=np.uint32)
    r = MR.rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        kk = eng.kept_count
        q = int_q(kk, c, n)
        d_q = torch.from_numpy(q).to(DEV)
        for sname, offs, kw, offs_at in sources(n, plain=True):
            v = len(offs)
            t = int_tables(v, n + v)
            wp, wy = AR.apply_int(GR.unpack(far.records(offs, r), n, kept), t, q)
            d_t = torch.from_numpy(t).to(DEV)
            kw_t, at_t = tensors(kw, offs_at)
            pbuf, pfront = framed(8 * v * c, align=8)
            obuf, ofront = framed(8 * kk * c, align=8)
            proj = pbuf[pfront: pfront + 8 * v * c].view(torch.float64)
            out = obuf[ofront: ofront + 8 * kk * c].view(torch.float64)
            if at_t is None:
                eng.gram_apply(far.dev, d_t, d_q, n_variants=v, proj=proj, out=out, kernel=GAPPLY[kernel], **kw_t)
            else:
                eng.gram_apply_at(far.dev, at_t, d_t, d_q, n_variants=v, proj=proj, out=out, kernel=GAPPLY[kernel])
            eng.wait()
            what = f"N={n} {keep} C={c} {sname} kernel {kernel}"
            for name, got, want, offs_of in (("P", payload(pbuf, pfront, 8 * v * c, what + " P").view(np.float64).reshape(v, c), wp, offs),
                                            ("Y", payload(obuf, ofront, 8 * kk * c, what + " Y").view(np.float64).reshape(kk, c), wy, None)):
                exp = want.astype(np.float64)
                if not np.array_equal(got, exp):
                    i, l = np.argwhere(got != exp)[0]
                    at = f" (row {i}: record at byte {offs_of[i]:#x})" if offs_of else ""
                    raise AssertionError(f"{what}: {name} entry ({i}, {l}){at}: got {float(got[i, l])!r}, want {float(exp[i, l])!r}")


# ---- dense records that cross 2^32 themselves ---------------------------------------------------------------------------------------
DENSE = [("runs", 1900, 9_100_000, _capi.KERNEL_RUNS, False), ("pick-packed", 2504, 6_900_000, _capi.KERNEL_PICK, False),
         ("line-runs", 900, 19_200_000, _capi.KERNEL_RUNS, True)]


@pytest.mark.parametrize("name,n,v,kernel,lines", DENSE, ids=[d[0] for d in DENSE])
def test_dense_records_past_4_gib(name, n, v, kernel, lines):
    """RUNS (N = 1 900), the pick family's packed path (N = 2 504, all samples) and the line-run kernel (N = 900, 12-byte prefixes)
    on 4.32 GB of dense records: V x R > 2^32, about 70 GB of text.  Needs 80 GiB."""
    need_gib(80)
    r = MR.rsize(n)
    plen = 12 if lines else 0
    row = plen + 4 * n + 1
    total = v * row
    assert v * r > (1 << 32) + (1 << 24) and total < 75 * 10**9
    assert SP.accepts(kernel, n, n, False, bound=plen, gather=False, mode="lines" if lines else "segments")
    rng = np.random.default_rng(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        recs = eng.synth_records(v, dirty_pad=True)
        out = torch.full((total + BACK,), SENT, dtype=torch.uint8, device=DEV)
        if lines:
            g = torch.Generator(device=DEV)
            g.manual_seed(n)
            blob = torch.randint(33, 127, (plen * v,), dtype=torch.uint8, device=DEV, generator=g)
            poff = torch.arange(v + 1, dtype=torch.int64, device=DEV) * plen
            loff = torch.arange(v + 1, dtype=torch.int64, device=DEV) * row
            eng.emit_lines(recs, v, blob, poff, loff, plen, out, kernel=kernel)
        else:
            eng.decode_emit(recs, v, out=out, kernel=kernel)
        eng.wait()
        assert bool((out[total:] == SENT).all()), "bytes behind the last row were written"
        rows2d = out[:total].view(v, row)
        assert bool((rows2d[:, row - 1] == 10).all()), "a row does not end in LF"
        j_4g = (1 << 32) // r
        starts = [0, j_4g - 50, v - 100] + [int(q) for q in rng.integers(0, v - 100, size=6)]
        for j0 in starts:
            j1 = j0 + 100
            h_recs = recs[j0 * r: j1 * r].cpu().numpy()
            want = oracle.decode_emit(h_recs, 100, n).reshape(100, 4 * n + 1)
            got = rows2d[j0:j1].cpu().numpy()
            if lines:
                first_diff(got[:, :plen], blob[j0 * plen: j1 * plen].cpu().numpy().reshape(100, plen), f"{name}: prefixes of rows {j0}..{j1}")
            first_diff(got[:, plen:], want, f"{name}: rows {j0}..{j1} (records at bytes {j0 * r:#x}..)")
        del out, rows2d, recs
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [2504, 2503], ids=["N2504-one-stream", "N2503-row-by-row"])
def test_pack_dense_records_past_4_gib(n):
    """pgenhip_pack_records DENSE on 4.32 GB of dense records into dense output, V x R > 2^32: N = 2 504 (a multiple of 4: the launcher
    hands runs of rows to the kernel as one byte stream) and N = 2 503 (row by row, the pad bits of every row cleared).  Sentinels
    around the output; windows of 100 rows against pack_ref at the start, around the row that holds byte 2^32, at the end and at six
    seeded places.  Needs 10 GiB."""
    need_gib(10)
    v = 6_900_000
    r = MR.rsize(n)
    assert v * r > (1 << 32) + (1 << 24)
    rng = np.random.default_rng(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        assert eng.packed_record_size == r
        recs = eng.synth_records(v, dirty_pad=True)
        buf, front = framed(v * r)
        eng.pack_records(recs, n_variants=v, out=buf, out_offset=front, shape=_capi.PACK_DENSE)
        eng.wait()
        assert LR.frame_ok(buf, front, v * r), "bytes outside the output were written"
        rows2d = buf[front: front + v * r].view(v, r)
        j_4g = (1 << 32) // r
        starts = [0, j_4g - 50, v - 100] + [int(q) for q in rng.integers(0, v - 100, size=6)]
        for j0 in starts:
            h_recs = recs[j0 * r: (j0 + 100) * r].cpu().numpy().reshape(100, r)
            if n % 4:
                assert (h_recs[:, -1] >> (2 * (n % 4))).any(), "the input's pad bits are clean: nothing to clear"
            first_diff(rows2d[j0: j0 + 100].cpu().numpy(), PK.pack(h_recs, n), f"pack N={n}: rows {j0}..{j0 + 100} (records at bytes {j0 * r:#x}..)")
        del buf, rows2d, recs
    torch.cuda.empty_cache()
