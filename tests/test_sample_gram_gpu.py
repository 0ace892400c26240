"""Sample Gram matrix — GPU leg (pgenhip_sample_gram / _at through GtEngine), GENERAL, MFMA and AUTO.
Exact leg: integer tables in [-8, 8] drawn per row make every partial sum an integer far below 2^53, so every shape must equal the
numpy reference (tests/gram_ref.py) bit for bit: sample counts around the 64-rank tile, row counts around the 32-row step at forced
slices (knob 25), the two ends of a 2 504-sample row, keep sets x row layouts inside sentinel doubles with padded rows, dirty pads.
Map leg: data whose Gram matrix is nowhere symmetric between disjoint ranges of unequal size, so a transposed operand or C/D map
cannot pass.  Cross-checks against sample_pair_tables and sample_counts.  Rounding leg: random FP64 tables across 2^+-20 against the
correctly rounded sum, inside the header's bound.  ACCUMULATE, streams, a captured graph, every refusal."""
import numpy as np
import pytest
import torch

import gram_plan as GP
import gram_ref as GR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -12345.678
KERNELS = {"general": _capi.GRAM_GENERAL, "mfma": _capi.GRAM_MFMA, "auto": _capi.GRAM_AUTO}
T, S = GP.TILE, GP.STEP_ROWS


def int_tables(v, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(v, 4)).astype(np.float64)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gram(eng, tables, a=None, b=None, at=None, pad=3, **kw):
    """The matrix into a dirty buffer with `pad` sentinel doubles behind every row and four on either side: without ACCUMULATE the
    call overwrites its entries, and nothing else may change."""
    k = eng.kept_count
    a = (0, k) if a is None else a
    b = (0, k) if b is None else b
    stride = b[1] + pad
    buf = torch.full((4 + max(a[1], 1) * stride + 4,), SENT, dtype=torch.float64, device=DEV)
    out = buf[4:]
    d_t = dev(tables.reshape(-1, 4))
    if at is not None:
        res = eng.sample_gram_at(at[0], at[1], d_t, a=a, b=b, out=out, out_stride=stride, **kw)
    else:
        res = eng.sample_gram(code_values=d_t, a=a, b=b, out=out, out_stride=stride, **kw)
    eng.wait()
    assert res.shape == (a[1], b[1]) and res.dtype == torch.float64
    frame = buf.cpu().numpy().copy()
    body = frame[4:4 + max(a[1], 1) * stride].reshape(-1, stride)
    got = body[:a[1], :b[1]].copy()
    body[:a[1], :b[1]] = SENT
    assert (frame == SENT).all(), "wrote outside its entries"
    return got


def check_all(eng, want, tables, a=None, b=None, at=None, what="", **kw):
    for name, kernel in KERNELS.items():
        got = run_gram(eng, tables, a, b, at=at, kernel=kernel, **kw)
        assert got.shape == want.shape and np.array_equal(got, want), f"{name} {what}"


N_LIST = [1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 300]


@pytest.mark.parametrize("n", N_LIST)
def test_sample_count_edges_full_square(n):
    v = 67
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=2, hwe=True)
        codes = GR.unpack(d.cpu().numpy()[: v * eng.record_size].reshape(v, -1), n)
        t = int_tables(v, n)
        check_all(eng, GR.gram_ref(codes, t), t, records=d, n_variants=v)


V_LIST = [0, 1, 3, 4, 5, S - 1, S, S + 1, 1000]


@pytest.mark.parametrize("slices", [1, 2, 7])
def test_row_count_edges_at_forced_slices(slices):
    n = 70
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_GRAM_SLICES, slices)
        d = eng.synth_records(V_LIST[-1], first_variant=5, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(V_LIST[-1], -1), n)
        t = int_tables(V_LIST[-1], slices)
        for v in V_LIST:
            check_all(eng, GR.gram_ref(codes[:v], t[:v]), t[:v], records=d, n_variants=v, what=f"V = {v}")


def test_default_plan_cuts_many_slices():
    n, v = 130, 5000
    assert GP.mfma_slices(v, n, n) > 7
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(v, -1), n)
        t = int_tables(v, 3)
        check_all(eng, GR.gram_ref(codes, t), t, records=d)


def test_two_ends_of_a_2504_sample_row():
    n, v = 2504, 131
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=3, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(v, -1), n)
        t = int_tables(v, 9)
        a, b = (1, 70), (n - 67, 67)
        ca, cb = codes[:, a[0]:a[0] + a[1]], codes[:, b[0]:]
        check_all(eng, GR.gram_ref(ca, t, cb), t, a, b, records=d)
        check_all(eng, GR.gram_ref(cb, t, ca), t, b, a, records=d, what="b before a")
        check_all(eng, GR.gram_ref(cb, t), t, b, b, records=d, what="the last ranks squared")


def kept_sets(n, rng):
    return {"all": None, "identity": list(range(n)), "first": [0], "last": [n - 1], "every7": list(range(0, n, 7)),
            "cluster": list(range(n // 2 - 40, n // 2 + 41)),
            "holes": sorted(set(range(n)) - set(rng.choice(n, size=n // 5, replace=False).tolist()))}


@pytest.mark.parametrize("keep", ["all", "identity", "first", "last", "every7", "cluster", "holes"])
def test_keep_sets_and_layouts(keep):
    n = 300
    rng = np.random.default_rng(43 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = GR.rsize(n)
    v = 75
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    codes = GR.unpack(recs, n, kept)
    k = codes.shape[1]
    d_raw = dev(raw)
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)   # descending, with repeats
    d_gather = dev(gather)
    d_offs = dev(np.array([3 + i * stride for i in gather], dtype=np.int64))   # odd and even byte offsets
    dense = dev(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)]))
    t = int_tables(v, 7)
    tg = int_tables(len(gather), 8)   # tables go with the position in the selection, not with the row number
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        check_all(eng, GR.gram_ref(codes, t), t, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, what="strided")
        check_all(eng, GR.gram_ref(codes[gather], tg), tg, records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather, what="gathered")
        check_all(eng, GR.gram_ref(codes[gather], tg), tg, at=(d_raw, d_offs), what="_at")
        check_all(eng, GR.gram_ref(codes, t), t, records=dense, records_offset=1, what="dense from an odd base")
        check_all(eng, GR.gram_ref(codes[-1:], t[:1]), t[:1], records=dense, records_offset=1 + r * (v - 1), n_variants=1, what="one row")
        if k >= 2:
            a, b = (k // 3, k - k // 3), (0, (k + 1) // 2)   # the first ends at K
            check_all(eng, GR.gram_ref(codes[:, a[0]:], t, codes[:, :b[1]]), t, a, b, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, what="ranges")


@pytest.mark.parametrize("n", [5, 299])
def test_dirty_pad_bits_are_not_samples(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 67
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        lo = max(0, n - 70)
        t = int_tables(v, n)
        check_all(eng, GR.gram_ref(GR.unpack(recs, n)[:, lo:], t), t, (lo, n - lo), (lo, n - lo), records=d, n_variants=v)


MAP_SEED = 2   # a seed for which the 37 x 37 corner of the disjoint block differs from its transpose everywhere
RANGES = [((3, 70), (80, 37)), ((80, 37), (3, 70)), ((3, 70), (3, 70)), ((5, 66), (37, 90)), ((100, 50), (2, 47)), ((7, 1), (0, 150)),
          ((0, 150), (149, 1)), ((0, 0), (0, 150)), ((10, 5), (150, 0))]


def hwe_records(n, v, seed):
    """(V, R) records of Hardy-Weinberg genotypes with 1 % missing calls, drawn on the host, and their (V, n) codes."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(v, 1))
    codes = (rng.random((v, n)) < p).astype(np.uint8) + (rng.random((v, n)) < p).astype(np.uint8)
    codes[rng.random((v, n)) < 0.01] = 3
    padded = np.zeros((v, 4 * GR.rsize(n)), dtype=np.uint8)
    padded[:, :n] = codes
    quads = padded.reshape(v, -1, 4)
    return (quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6).astype(np.uint8), codes


def test_map_leg_asymmetric_data_in_every_range_relation():
    """G[i, l] != G[l, i] between two different rank ranges, so transposed operands or a transposed C/D map cannot pass; with equal
    ranges the matrix is symmetric and would hide both."""
    n, v = 150, 1000
    recs, codes = hwe_records(n, v, MAP_SEED)
    assert np.array_equal(GR.unpack(recs, n), codes)
    t = int_tables(v, 21)
    full = GR.gram_ref(codes, t)
    a, b = RANGES[0]
    blk = full[a[0]:a[0] + 37, b[0]:b[0] + 37]
    assert (blk != blk.T)[~np.eye(37, dtype=bool)].all(), "the data do not tell G from its transpose"
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = dev(recs.reshape(-1))
        for a, b in RANGES:
            want = np.ascontiguousarray(full[a[0]:a[0] + a[1], b[0]:b[0] + b[1]])
            check_all(eng, want, t, a, b, records=d, what=f"a = {a}, b = {b}")
        a, b = RANGES[0]
        for kernel in KERNELS.values():
            ab = run_gram(eng, t, a, b, records=d, kernel=kernel)
            ba = run_gram(eng, t, b, a, records=d, kernel=kernel)
            assert np.array_equal(ab, ba.T)
        # defaults: both ranges all K, a result allocated by the wrapper
        assert np.array_equal(eng.sample_gram(d, code_values=dev(t)).cpu().numpy(), full)


def test_cross_checks_against_pair_tables_and_sample_counts():
    n, v = 131, 400
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=4, hwe=True)
        tables = eng.sample_pair_tables(d).cpu().numpy().astype(np.int64)
        counts = eng.sample_counts(d).cpu().numpy().astype(np.int64).reshape(n, 4)
        called = np.tile([1.0, 1.0, 1.0, 0.0], (v, 1))
        dosage = np.tile([0.0, 1.0, 2.0, 0.0], (v, 1))
        for name, kernel in KERNELS.items():
            got_n = run_gram(eng, called, records=d, kernel=kernel)
            assert np.array_equal(got_n, tables[:, :, :3, :3].sum(axis=(2, 3)).astype(np.float64)), name
            got_d = run_gram(eng, dosage, records=d, kernel=kernel)
            assert np.array_equal(np.diag(got_d), (counts[:, 1] + 4 * counts[:, 2]).astype(np.float64)), name


@pytest.mark.parametrize("v", [64, 1000])
def test_rounding_leg_inside_the_documented_bound(v):
    """Random FP64 tables across 2^-20 .. 2^20: every entry within 1.01 (V + 2) 2^-53 A(a, b) of the correctly rounded sum."""
    n = 100
    rng = np.random.default_rng(v)
    t = rng.standard_normal((v, 4)) * np.exp2(rng.uniform(-20, 20, size=(v, 4)))
    a, b = (2, 40), (61, 37)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=8, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(v, -1), n)
        ca, cb = codes[:, a[0]:a[0] + a[1]], codes[:, b[0]:b[0] + b[1]]
        want, scale = GR.gram_fsum(ca, t, cb), GR.gram_abs(ca, t, cb)
        bound = 1.01 * (v + 2) * 2.0 ** -53 * scale
        for slices in (0, 1):
            eng.tune(_capi.KNOB_GRAM_SLICES, slices)
            for name, kernel in KERNELS.items():
                got = run_gram(eng, t, a, b, records=d, kernel=kernel)
                err = np.abs(got - want)
                print(f"rounding V={v} {name} slices={slices}: worst error / bound = {(err / bound).max():.4f}")
                assert (err <= bound).all(), f"{name}: worst error / bound = {(err / bound).max()}"


@pytest.mark.parametrize("n,keep", [(70, "all"), (300, "holes")])
def test_accumulate_and_overwrite(n, keep):
    kept = kept_sets(n, np.random.default_rng(n))[keep]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        v, half = 301, 123
        d = eng.synth_records(v, hwe=True)
        r, k = eng.record_size, eng.kept_count
        codes = GR.unpack(d.cpu().numpy().reshape(v, -1), n, kept)
        t = int_tables(v, 5)
        whole, d_t = GR.gram_ref(codes, t), dev(t)
        for name, kernel in KERNELS.items():
            out = torch.full((k * k,), 7.0, dtype=torch.float64, device=DEV)
            eng.sample_gram(d, n_variants=half, code_values=d_t, out=out, kernel=kernel)                                # overwrites the 7s
            eng.sample_gram(d, n_variants=v - half, code_values=d_t[half:].contiguous(), out=out, accumulate=True, records_offset=half * r, kernel=kernel)
            eng.wait()
            assert np.array_equal(out.view(k, k).cpu().numpy(), whole), f"{name}: two row blocks summed in place != one call over both"
            eng.sample_gram(d, n_variants=0, code_values=d_t, out=out, accumulate=True, kernel=kernel)                  # a no-op
            eng.wait()
            assert np.array_equal(out.view(k, k).cpu().numpy(), whole), name
            eng.sample_gram(d, n_variants=0, code_values=d_t, out=out, kernel=kernel)                                   # overwrite with nothing
            eng.wait()
            assert not out.any(), name


def test_overlapping_launches_on_three_streams():
    n, v = 300, 2000
    kept = list(range(0, n, 3))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(3 * v, -1), n, kept)
        r, k = eng.record_size, eng.kept_count
        t = int_tables(3 * v, 6)
        d_ts = [dev(t[i * v:(i + 1) * v]) for i in range(3)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((k * k,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        kernels = [_capi.GRAM_MFMA, _capi.GRAM_GENERAL, _capi.GRAM_AUTO]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.sample_gram(d, n_variants=v, records_offset=i * v * r, code_values=d_ts[i], out=outs[i], kernel=kernels[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            assert np.array_equal(outs[i].view(k, k).cpu().numpy(), GR.gram_ref(codes[i * v:(i + 1) * v], t[i * v:(i + 1) * v])), f"stream {i}"


@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_hip_graph_replayed_twice(kernel):
    """A capture on one stream of an overwriting call (zeroing + kernel) and of an ACCUMULATE call (the kernel alone), replayed twice
    onto new records and tables: the overwrite gives the matrix once, the accumulate adds it twice."""
    n, v = 130, 257
    rng = np.random.default_rng(5)
    r = GR.rsize(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        d_t = torch.zeros((v, 4), dtype=torch.float64, device=DEV)
        out = torch.zeros(n * n, dtype=torch.float64, device=DEV)
        acc = torch.zeros(n * n, dtype=torch.float64, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.sample_gram(d_recs, code_values=d_t, out=out, kernel=KERNELS[kernel])   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.sample_gram(d_recs, code_values=d_t, out=out, kernel=KERNELS[kernel])
            eng.sample_gram(d_recs, code_values=d_t, out=acc, accumulate=True, kernel=KERNELS[kernel])
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        t = int_tables(v, 12)
        d_recs.copy_(torch.from_numpy(recs))
        d_t.copy_(torch.from_numpy(t))
        out.fill_(9.0)
        acc.zero_()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        want = GR.gram_ref(GR.unpack(recs.reshape(v, r), n), t)
        assert np.array_equal(out.view(n, n).cpu().numpy(), want)
        assert np.array_equal(acc.view(n, n).cpu().numpy(), 2 * want)
        eng.use_torch_stream()


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        tabs = torch.ones(4 * 4 + 1, dtype=torch.float64, device=DEV)
        buf = torch.full((20 * 20 + 8,), SENT, dtype=torch.float64, device=DEV)
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctx, rp, tp, op, fp = eng._ctx, recs.data_ptr(), tabs.data_ptr(), buf.data_ptr(), offs.data_ptr()
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call, call_at = lib.pgenhip_sample_gram, lib.pgenhip_sample_gram_at
        assert call(None, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 20, 0) == bad                  # NULL ctx
        assert call(ctx, rp, 75, None, 4, tp, 281, 20, 0, 20, op, 20, 0) == bad                 # a range past K
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 300, 1, op, 20, 0) == bad                  # b range past K
        assert call(ctx, rp, 75, None, 4, tp, 0xFFFFFFFF, 2, 0, 20, op, 20, 0) == bad           # begin + count wraps in 32 bits
        assert call(ctx, rp, 75, None, 4, None, 0, 20, 0, 20, op, 20, 0) == bad                 # NULL tables with rows
        assert call(ctx, rp, 75, None, 4, tp + 4, 0, 20, 0, 20, op, 20, 0) == bad               # tables not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, None, 20, 0) == bad                 # NULL out
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op + 4, 20, 0) == bad               # out not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 19, 0) == bad                   # out_stride < b_count
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 20, 0x20) == bad                # unknown flag bit
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 20, 3) == bad                   # the reserved f32-operand shape
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 20, 0xF | _capi.GRAM_ACCUMULATE) == bad
        assert call(ctx, None, 75, None, 4, tp, 0, 20, 0, 20, op, 20, 0) == bad                 # NULL records
        assert call(ctx, rp, 74, None, 4, tp, 0, 20, 0, 20, op, 20, 0) == bad                   # stride < R
        assert call_at(None, rp, fp, 4, tp, 0, 20, 0, 20, op, 20, 0) == bad
        assert call_at(ctx, rp, None, 4, tp, 0, 20, 0, 20, op, 20, 0) == bad                    # NULL offsets
        assert call_at(ctx, rp, fp, 4, tp, 0, 20, 0, 20, op + 4, 20, 0) == bad
        assert call_at(ctx, rp, fp, 4, tp, 0, 301, 0, 20, op, 20, 0) == bad
        assert call(ctx, rp, 1 << 51, None, 2, tp, 0, 20, 0, 20, op, 20, 0) == big              # record_stride * n_variants >= 2^52
        assert call(ctx, rp, 1 << 52, fp, 2, tp, 0, 20, 0, 20, op, 20, 0) == big                # with a variant list the stride alone
        assert call(ctx, rp, 75, None, 4, tp, 0, 20, 0, 20, op, 1 << 45, 0) == big              # a_count * out_stride * 8 >= 2^52
        eng.wait()
        assert (buf == SENT).all(), "a refused call wrote"
        # an empty range writes nothing, whatever the pointers; a single output row needs no stride; no rows need no tables
        assert call(ctx, rp, 75, None, 4, tp, 0, 0, 0, 20, None, 0, 0) == _capi.OK
        assert call(ctx, rp, 75, None, 4, tp, 300, 0, 0, 20, op + 4, 0, _capi.GRAM_MFMA) == _capi.OK
        eng.wait()
        assert (buf == SENT).all()
        assert call(ctx, rp, 75, None, 4, tp, 5, 1, 0, 20, op, 0, 0) == _capi.OK
        assert call(ctx, rp, 75, None, 0, None, 0, 2, 0, 3, op + 8 * 30, 5, 0) == _capi.OK      # zeros into 2 x 3 at stride 5
        eng.wait()
        got = buf.cpu().numpy()
        assert (got[:20] == 4.0).all() and (got[20:30] == SENT).all()   # four rows of 1 * 1
        assert not got[30:33].any() and (got[33:35] == SENT).all() and not got[35:38].any() and (got[38:] == SENT).all()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0: OK, nothing written, whatever the pointers
        assert lib.pgenhip_sample_gram(eng._ctx, None, 75, None, 4, tp, 0, 0, 0, 0, None, 0, 0) == _capi.OK
        assert lib.pgenhip_sample_gram(eng._ctx, None, 75, None, 4, tp, 0, 1, 0, 0, None, 0, 0) == _capi.ERR_BAD_ARG
    with pgen_rs_amd.GtEngine(300, kept_idx=[299], device=0) as eng:   # K == 1
        d = eng.synth_records(9, hwe=True)
        codes = GR.unpack(d.cpu().numpy().reshape(9, -1), 300, [299])
        t = int_tables(9, 2)
        check_all(eng, GR.gram_ref(codes, t), t, records=d)
