"""Pairwise sample tables — GPU leg (pgenhip_sample_pair_stats / _at through GtEngine).  Every table is compared bit for bit with
the numpy reference (tests/spair_ref.py) for BOTH forced shapes (GENERAL, MFMA) and for AUTO: sample counts around 4 / 16 / 64 and
the 64 x 64 block tile, row counts around the 64-row MFMA step and the slice edges (knob 22), rank ranges, keep sets, row layouts,
value coverage (constant rows, counts past 2^16, asymmetric HWE data: the check of the MFMA operand maps), framing, ACCUMULATE,
the far end of a long row, streams, a captured graph and every refusal."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import spair_ref as XR
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x5EC0DE5
KERNELS = {"general": _capi.SPAIR_GENERAL, "mfma": _capi.SPAIR_MFMA, "auto": _capi.SPAIR_AUTO}


def kept_sets(n, rng):
    """The seven keep sets of test_sample_counts_gpu.py / test_sample_scores_gpu.py."""
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def run_tables(eng, a=None, b=None, at=None, **kw):
    """Tables into a buffer that starts dirty, at the minimum alignment (16 bytes past a 256-byte boundary), with four sentinel
    words on either side: without ACCUMULATE the call overwrites its entries, and nothing else may change."""
    k = eng.kept_count
    a = (0, k) if a is None else a
    b = (0, k) if b is None else b
    need = 16 * a[1] * b[1]
    buf = torch.full((4 + need + 4,), SENT, dtype=torch.int32, device=DEV)
    out = buf[4:]
    assert out.data_ptr() % 16 == 0 and out.data_ptr() % 32 != 0
    if at is not None:
        res = eng.sample_pair_tables_at(at[0], at[1], a=a, b=b, out=out, **kw)
    else:
        res = eng.sample_pair_tables(a=a, b=b, out=out, **kw)
    eng.wait()
    assert (buf[:4] == SENT).all() and (buf[4 + need:] == SENT).all(), "wrote outside its entries"
    assert res.shape == (a[1], b[1], 4, 4) and res.dtype == torch.int32
    return res


def check_all(eng, want, a=None, b=None, at=None, what="", **kw):
    """All three shapes against the (A, B, 4, 4) int64 reference."""
    d_want = torch.from_numpy(want.astype(np.int32)).to(DEV)
    for name, kernel in KERNELS.items():
        got = run_tables(eng, a, b, at=at, kernel=kernel, **kw)
        assert torch.equal(got, d_want), f"{name} {what}"


N_LIST = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 129, 257, 2504]


@pytest.mark.parametrize("n", N_LIST)
def test_sample_count_edges_full_square(n):
    v = 67
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=2, hwe=True)
        codes = XR.unpack(d.cpu().numpy()[: v * eng.record_size].reshape(v, -1), n)
        check_all(eng, XR.pair_tables(codes), records=d, n_variants=v)


V_LIST = [0, 1, 15, 16, 17, 63, 64, 65, 127, 129, 1000]


@pytest.mark.parametrize("slices", [1, 2, 7])
def test_row_count_edges_at_forced_slices(slices):
    n = 70
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_SPAIR_SLICES, slices)
        d = eng.synth_records(V_LIST[-1], first_variant=5, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(V_LIST[-1], -1), n)
        for v in V_LIST:
            check_all(eng, XR.pair_tables(codes[:v]), records=d, n_variants=v, what=f"V = {v}")


def test_default_plan_cuts_many_slices():
    n, v = 130, 5000
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(v, -1), n)
        check_all(eng, XR.pair_tables(codes), records=d)


RANGES = [((0, 150), (0, 150)), ((7, 1), (0, 150)), ((0, 150), (149, 1)), ((3, 70), (3, 70)), ((5, 66), (37, 90)), ((1, 30), (81, 69)),
          ((100, 50), (2, 47)), ((86, 64), (86, 64)), ((13, 17), (13, 17)), ((0, 0), (0, 150)), ((10, 5), (150, 0))]


def test_rank_ranges():
    n, v = 150, 131
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=1, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(v, -1), n)
        full = XR.pair_tables(codes)
        for a, b in RANGES:
            want = full[a[0]:a[0] + a[1], b[0]:b[0] + b[1]]
            check_all(eng, np.ascontiguousarray(want), a, b, records=d, what=f"a = {a}, b = {b}")
        # defaults: both ranges all K
        assert torch.equal(eng.sample_pair_tables(d), torch.from_numpy(full.astype(np.int32)).to(DEV))


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_keep_sets_and_layouts(n, keep):
    rng = np.random.default_rng(n * 43 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = XR.rsize(n)
    v = 75
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    codes = XR.unpack(recs, n, kept)
    k = codes.shape[1]
    d_raw = torch.from_numpy(raw).to(DEV)
    # descending with repeats: each appearance counts
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + i * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    want, want_g, want_1 = XR.pair_tables(codes), XR.pair_tables(codes[gather]), XR.pair_tables(codes[-1:])
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        check_all(eng, want, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, what="strided")
        check_all(eng, want_g, records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather, what="gathered")
        check_all(eng, want_g, at=(d_raw, d_offs), what="_at")
        check_all(eng, want, records=dense, records_offset=1, what="dense from an odd base")
        check_all(eng, want_1, records=dense, records_offset=1 + r * (v - 1), n_variants=1, what="one row")
        if k >= 2:
            a, b = (k // 3, k - k // 3), (0, (k + 1) // 2)   # the first ends at K
            check_all(eng, np.ascontiguousarray(want[a[0]:, :b[1]]), a, b, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, what="ranges")


@pytest.mark.parametrize("n", [5, 299, 2503])
def test_dirty_pad_bits_do_not_count(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 67
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        lo = max(0, n - 70)
        want = XR.pair_tables(XR.unpack(recs, n)[:, lo:])
        check_all(eng, want, (lo, n - lo), (lo, n - lo), records=d, n_variants=v)


@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_constant_rows_fill_one_cell(code):
    n, v = 67, 130
    recs = np.full((v, XR.rsize(n)), code * 0x55, dtype=np.uint8)
    want = np.zeros((n, n, 4, 4), dtype=np.int64)
    want[:, :, code, code] = v
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        check_all(eng, want, records=torch.from_numpy(recs.reshape(-1)).to(DEV))


def test_counts_pass_2_to_the_16():
    """V = 70 000 all-het rows on 17 samples: a partial sum kept in 16 bits (or an int8 / int16 accumulator) cannot hold 70 000."""
    n, v = 17, 70_000
    recs = torch.full((v * XR.rsize(n),), 0x55, dtype=torch.uint8, device=DEV)
    want = np.zeros((n, n, 4, 4), dtype=np.int64)
    want[:, :, 1, 1] = v
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        check_all(eng, want, records=recs)
        eng.tune(_capi.KNOB_SPAIR_SLICES, 1)
        check_all(eng, want, records=recs, what="one slice")


def test_hwe_tables_are_asymmetric():
    """T(a, b) != T(a, b)^T on HWE data, so an MFMA kernel with its operands or its C/D map transposed cannot pass."""
    n, v = 96, 700
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=11, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(v, -1), n)
        want = XR.pair_tables(codes)
        off = [(a, b) for a in range(n) for b in range(n) if a != b]
        assert all((want[a, b] != want[a, b].T).any() for a, b in off), "the data do not tell T from its transpose"
        assert all((want[a, b] != want[b, a]).any() for a, b in off), "the data do not tell (a, b) from (b, a)"
        assert all(len({int(want[a, b, x, y]) for x in range(1, 4) for y in range(1, 4)}) > 3 for a, b in off[:50])
        check_all(eng, want, records=d)
        a, b = (3, 40), (50, 46)
        check_all(eng, np.ascontiguousarray(want[3:43, 50:96]), a, b, records=d, what="disjoint ranges")


@pytest.mark.parametrize("n,keep", [(70, "all"), (300, "p50")])
def test_accumulate_and_overwrite(n, keep):
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        v, half = 301, 123
        d = eng.synth_records(v, hwe=True)
        r, k = eng.record_size, eng.kept_count
        for name, kernel in KERNELS.items():
            whole = eng.sample_pair_tables(d, kernel=kernel).clone()
            out = torch.full((16 * k * k,), 7, dtype=torch.int32, device=DEV)
            eng.sample_pair_tables(d, n_variants=half, out=out, kernel=kernel)                                       # overwrites the 7s
            eng.sample_pair_tables(d, n_variants=v - half, out=out, accumulate=True, records_offset=half * r, kernel=kernel)
            eng.wait()
            assert torch.equal(out.view(k, k, 4, 4), whole), f"{name}: two row blocks summed in place != one call over both"
            eng.sample_pair_tables(d, n_variants=0, out=out, accumulate=True, kernel=kernel)                          # a no-op
            eng.wait()
            assert torch.equal(out.view(k, k, 4, 4), whole), name
            eng.sample_pair_tables(d, n_variants=0, out=out, kernel=kernel)                                           # overwrite with nothing
            eng.wait()
            assert not out.any(), name
        assert int(whole.sum()) == v * k * k


def test_far_end_of_a_long_row():
    n, v = 500_000, 130
    a, b = (5, 40), (n - 40, 40)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=3, hwe=True)
        recs = d.cpu().numpy().reshape(v, -1)
        codes_a = XR.unpack(recs[:, : 16], 64)[:, a[0]:a[0] + a[1]]
        tail = recs[:, (n - 40) // 4:]
        codes_b = XR.unpack(tail, tail.shape[1] * 4)[:, (n - 40) % 4:][:, :40]
        check_all(eng, XR.pair_tables(codes_a, codes_b), a, b, records=d)
        check_all(eng, XR.pair_tables(codes_b, codes_a), b, a, records=d, what="b before a")


def test_overlapping_launches_on_three_streams():
    n, v = 300, 2000
    kept = list(range(0, n, 3))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(3 * v, -1), n, kept)
        r, k = eng.record_size, eng.kept_count
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((16 * k * k,), SENT, dtype=torch.int32, device=DEV) for _ in range(3)]
        kernels = [_capi.SPAIR_MFMA, _capi.SPAIR_GENERAL, _capi.SPAIR_AUTO]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.sample_pair_tables(d, n_variants=v, records_offset=i * v * r, out=outs[i], kernel=kernels[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            want = XR.pair_tables(codes[i * v:(i + 1) * v]).astype(np.int32)
            assert np.array_equal(outs[i].view(k, k, 4, 4).cpu().numpy(), want), f"stream {i}"


@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_hip_graph_replayed_twice(kernel):
    """A capture on one stream of an overwriting call (memset + kernel) and of an ACCUMULATE call (the kernel alone), replayed
    twice onto new records: the overwrite gives the tables once, the accumulate adds them twice."""
    n, v = 130, 257
    rng = np.random.default_rng(5)
    r = XR.rsize(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        out = torch.zeros(16 * n * n, dtype=torch.int32, device=DEV)
        acc = torch.zeros(16 * n * n, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.sample_pair_tables(d_recs, out=out, kernel=KERNELS[kernel])   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.sample_pair_tables(d_recs, out=out, kernel=KERNELS[kernel])
            eng.sample_pair_tables(d_recs, out=acc, accumulate=True, kernel=KERNELS[kernel])
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        d_recs.copy_(torch.from_numpy(recs))
        out.fill_(9)
        acc.zero_()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        want = XR.pair_tables(XR.unpack(recs.reshape(v, r), n)).astype(np.int32)
        assert np.array_equal(out.view(n, n, 4, 4).cpu().numpy(), want)
        assert np.array_equal(acc.view(n, n, 4, 4).cpu().numpy(), 2 * want)
        eng.use_torch_stream()


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        buf = torch.full((16 * 20 * 20 + 8,), SENT, dtype=torch.int32, device=DEV)
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctx, rp, op, fp = eng._ctx, recs.data_ptr(), buf.data_ptr(), offs.data_ptr()
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call, call_at = lib.pgenhip_sample_pair_stats, lib.pgenhip_sample_pair_stats_at
        assert call(None, rp, 75, None, 4, 0, 20, 0, 20, op, 0) == bad                  # NULL ctx
        assert call(ctx, rp, 75, None, 4, 281, 20, 0, 20, op, 0) == bad                 # a range past K
        assert call(ctx, rp, 75, None, 4, 0, 20, 300, 1, op, 0) == bad                  # b range past K
        assert call(ctx, rp, 75, None, 4, 0xFFFFFFFF, 2, 0, 20, op, 0) == bad           # begin + count wraps in 32 bits
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, None, 0) == bad                 # NULL out
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, op + 4, 0) == bad               # out not 16-byte aligned
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, op + 8, 0) == bad
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, op, 0x20) == bad                # unknown flag bit
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, op, 3) == bad                   # unknown shape
        assert call(ctx, rp, 75, None, 4, 0, 20, 0, 20, op, 0xF | _capi.SPAIR_ACCUMULATE) == bad
        assert call(ctx, None, 75, None, 4, 0, 20, 0, 20, op, 0) == bad                 # NULL records
        assert call(ctx, rp, 74, None, 4, 0, 20, 0, 20, op, 0) == bad                   # stride < R
        assert call_at(None, rp, fp, 4, 0, 20, 0, 20, op, 0) == bad
        assert call_at(ctx, rp, None, 4, 0, 20, 0, 20, op, 0) == bad                    # NULL offsets
        assert call_at(ctx, rp, fp, 4, 0, 20, 0, 20, op + 4, 0) == bad
        assert call_at(ctx, rp, fp, 4, 0, 301, 0, 20, op, 0) == bad
        assert call(ctx, rp, 1 << 51, None, 2, 0, 20, 0, 20, op, 0) == big              # record_stride * n_variants >= 2^52
        assert call(ctx, rp, 1 << 52, fp, 2, 0, 20, 0, 20, op, 0) == big                # with a variant list the stride alone
        eng.wait()
        assert (buf == SENT).all(), "a refused call wrote"
        # an empty range writes nothing, whatever the output pointer; a single row needs no stride
        assert call(ctx, rp, 75, None, 4, 0, 0, 0, 20, None, 0) == _capi.OK
        assert call(ctx, rp, 75, None, 4, 300, 0, 0, 20, op + 4, _capi.SPAIR_MFMA) == _capi.OK
        assert call(ctx, rp, 0, None, 1, 0, 20, 0, 20, op, 0) == _capi.OK
        eng.wait()
        assert (buf[16 * 20 * 20:] == SENT).all()
    # a_count * b_count * 64 >= 2^52 needs K >= 2^23: refused before any launch or memset
    with pgen_rs_amd.GtEngine(1 << 24, device=0) as eng:
        recs = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
        small = torch.full((64,), SENT, dtype=torch.int32, device=DEV)
        assert lib.pgenhip_sample_pair_stats(eng._ctx, recs.data_ptr(), 1 << 22, None, 1, 0, 1 << 23, 0, 1 << 23, small.data_ptr(), 0) == _capi.ERR_TOO_LARGE
        eng.wait()
        assert (small == SENT).all()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0: OK, nothing written, whatever the pointers
        assert lib.pgenhip_sample_pair_stats(eng._ctx, None, 75, None, 4, 0, 0, 0, 0, None, 0) == _capi.OK
        assert lib.pgenhip_sample_pair_stats(eng._ctx, None, 75, None, 4, 0, 1, 0, 0, None, 0) == _capi.ERR_BAD_ARG
        assert eng.sample_pair_tables(recs).shape == (0, 0, 4, 4)
    with pgen_rs_amd.GtEngine(300, kept_idx=[299], device=0) as eng:   # K == 1
        d = eng.synth_records(9, hwe=True)
        codes = XR.unpack(d.cpu().numpy().reshape(9, -1), 300, [299])
        check_all(eng, XR.pair_tables(codes), records=d)
