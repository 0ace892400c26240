"""Per-sample weighted dosage sums (polygenic scores) — GPU leg (pgenhip_sample_scores / _at through GtEngine).

Exact leg: integer weights in [-8, 8] and integer miss values in {0, 1, 2, 3} make every partial sum of every summation order an
integer below 2^53, so the kernel must equal the reference (tests/score_ref.py) bit for bit whatever its plan does: every sample
count class, keep set, column count, row layout and plan edge (tests/score_plan.py).  Rounding leg: random f32 weights across
2^+-20 against math.fsum within the bound of any-order summation of exact terms.  Cross-checks against sample_counts and
decode_matrix."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import score_plan as SP
import score_ref as SR
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1.2345e300
COLUMNS = [1, 2, 3, 8]


def rsize(n):
    return (2 * n + 7) // 8


def kept_sets(n, rng):
    """The seven keep sets of test_sample_counts_gpu.py."""
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def int_weights(rng, v, c=8):
    return rng.integers(-8, 9, size=(v, c)).astype(np.float32)


def int_miss(rng, v):
    return rng.integers(0, 4, size=v).astype(np.float32)


def weight_tensor(w8: torch.Tensor, c: int) -> torch.Tensor:
    """The first c columns of the (V, 8) device weights: a 1-D tensor for c = 1, a contiguous copy for 2 and 8, and for c = 3 a
    view of the 8-wide rows (w_stride 8 > C)."""
    if c == 1:
        return w8[:, 0].contiguous()
    if c == 3:
        return w8[:, :3]
    return w8[:, :c].contiguous()


def run_scores(eng, c, at=None, **kw):
    """scores into a sentinel-guarded buffer that starts dirty: without ACCUMULATE the call overwrites its K * C doubles, and
    nothing else may change."""
    k = eng.kept_count
    lead = 3
    buf = torch.full((lead + k * c + 8,), SENT, dtype=torch.float64, device=DEV)
    out = buf[lead:]
    if at is not None:
        res = eng.sample_scores_at(at[0], at[1], out=out, **kw)
    else:
        res = eng.sample_scores(out=out, **kw)
    eng.wait()
    h = buf.cpu().numpy()
    assert (h[:lead] == SENT).all() and (h[lead + k * c:] == SENT).all(), "wrote outside its scores"
    assert res.shape == (k, c) and res.dtype == torch.float64
    return res.cpu().numpy()


N_LIST = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 257, 300, 2504, 16383, 16384, 16385, 500_000]


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_exact_layouts_against_reference(n, keep):
    rng = np.random.default_rng(n * 41 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    v = 40 if n >= 100_000 else 41
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    codes = SR.unpack_codes(recs, n)
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    d_raw = torch.from_numpy(raw).to(DEV)
    # descending with repeats: each appearance adds; weights and miss go by the position in the selection
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)
    g = len(gather)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + i * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    w8, miss = int_weights(rng, v), int_miss(rng, v)
    d_w8, d_miss = torch.from_numpy(w8).to(DEV), torch.from_numpy(miss).to(DEV)
    want, _ = SR.score_from_codes(codes, w8, miss)
    want_g, _ = SR.score_from_codes(codes[gather], w8[:g], miss[:g])
    want_1, _ = SR.score_from_codes(codes[-1:], w8[:1], miss[:1])
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for c in COLUMNS:
            w, wg = weight_tensor(d_w8, c), weight_tensor(d_w8[:g], c)
            got = run_scores(eng, c, records=d_raw, weights=w, miss=d_miss, record_stride=stride, records_offset=3)
            assert np.array_equal(got, want[:, :c]), f"strided, C = {c}"
            got = run_scores(eng, c, records=d_raw, weights=wg, miss=d_miss[:g], record_stride=stride, records_offset=3, variant_idx=d_gather)
            assert np.array_equal(got, want_g[:, :c]), f"gathered, C = {c}"
            got = run_scores(eng, c, at=(d_raw, d_offs), weights=wg, miss=d_miss[:g])
            assert np.array_equal(got, want_g[:, :c]), f"_at, C = {c}"
            got = run_scores(eng, c, records=dense, weights=w, miss=d_miss, records_offset=1, flags=_capi.SCORE_ROWS)
            assert np.array_equal(got, want[:, :c]), f"dense from an odd base, C = {c}"
            got = run_scores(eng, c, records=dense, weights=weight_tensor(d_w8[:1], c), miss=d_miss[:1], records_offset=1 + r * (v - 1), n_variants=1)
            assert np.array_equal(got, want_1[:, :c]), f"one row, C = {c}"


# rows on both sides of every edge of the plan (tests/score_plan.py), with the slices forced (PGENHIP_KNOB_SCORE_SLICES)
@pytest.mark.parametrize("n,c,keep", [(300, 1, "all"), (300, 8, "p50"), (2504, 2, "all"), (2504, 8, "p1"), (5000, 4, "all"), (33, 3, "all"), (13, 1, "all")])
@pytest.mark.parametrize("slices", [1, 3])
def test_plan_edges(n, c, keep, slices):
    rng = np.random.default_rng(n + 7 * slices + c)
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    vs = SP.edge_rows(n, c, slices)
    vmax = vs[-1]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCORE_SLICES, slices)
        d = eng.synth_records(vmax, first_variant=3, hwe=True, dirty_pad=False)
        codes = SR.unpack_codes(d[: vmax * r].cpu().numpy().reshape(vmax, r), n)
        if kept is not None:
            codes = codes[:, np.asarray(kept, dtype=np.int64)]
        w, miss = int_weights(rng, vmax, c), int_miss(rng, vmax)
        d_w, d_miss = torch.from_numpy(w).to(DEV), torch.from_numpy(miss).to(DEV)
        for v in vs:
            want, _ = SR.score_from_codes(codes[:v], w[:v], miss[:v])
            got = run_scores(eng, c, records=d, weights=d_w[:v], miss=d_miss[:v], n_variants=v)
            assert np.array_equal(got, want), f"V = {v}"


def test_default_plan_cuts_many_slices():
    """Without the knob a launch of many rows is cut into slices of at least SP.MIN_SLICE_ROWS rows, which meet in global atomics."""
    n, v, c = 300, 8 * SP.MIN_SLICE_ROWS + 77, 2
    rng = np.random.default_rng(8)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        codes = SR.unpack_codes(d.cpu().numpy().reshape(v, -1), n)
        w, miss = int_weights(rng, v, c), int_miss(rng, v)
        want, _ = SR.score_from_codes(codes, w, miss)
        got = run_scores(eng, c, records=d, weights=torch.from_numpy(w).to(DEV), miss=torch.from_numpy(miss).to(DEV))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [300, 2503, 70_001])
def test_dirty_pad_bits_do_not_count(n):
    rng = np.random.default_rng(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 67
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        if n % 4:
            assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        w, miss = int_weights(rng, v), int_miss(rng, v)
        want, _ = SR.score_ref(recs, n, w, miss)
        for c in COLUMNS:
            got = run_scores(eng, c, records=d, weights=weight_tensor(torch.from_numpy(w).to(DEV), c), miss=torch.from_numpy(miss).to(DEV), n_variants=v)
            assert np.array_equal(got, want[:, :c])


@pytest.mark.parametrize("n,keep,c", [(300, "all", 1), (2504, "p50", 3), (20_000, "p1", 8)])
def test_accumulate_overwrite_and_null_miss(n, keep, c):
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        v, half = 301, 123
        d = eng.synth_records(v, hwe=True)
        r, k = eng.record_size, eng.kept_count
        d_w = torch.from_numpy(int_weights(rng, v, c)).to(DEV)
        d_miss = torch.from_numpy(int_miss(rng, v)).to(DEV)
        whole = eng.sample_scores(d, d_w, miss=d_miss).clone()
        out = torch.full((k * c,), 7.0, dtype=torch.float64, device=DEV)
        eng.sample_scores(d, d_w[:half], miss=d_miss[:half], out=out)                                 # overwrites the 7s
        eng.sample_scores(d, d_w[half:], miss=d_miss[half:], out=out, accumulate=True, records_offset=half * r)
        eng.wait()
        assert torch.equal(out.view(k, c), whole), "two halves summed in place != one launch over both"
        eng.sample_scores(d, d_w[:0], out=out, accumulate=True, n_variants=0)                          # a no-op
        eng.wait()
        assert torch.equal(out.view(k, c), whole)
        eng.sample_scores(d, d_w[:0], out=out, n_variants=0)                                           # overwrite with nothing: zeros
        eng.wait()
        assert (out.cpu().numpy() == 0).all()
        # d_miss NULL is a zero array
        a = eng.sample_scores(d, d_w).clone()
        b = eng.sample_scores(d, d_w, miss=torch.zeros(v, dtype=torch.float32, device=DEV))
        eng.wait()
        assert torch.equal(a, b)


def test_overlapping_launches_on_three_streams():
    n, v, c = 2504, 4000, 3
    kept = list(range(0, n, 3))
    rng = np.random.default_rng(3)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        codes = SR.unpack_codes(d.cpu().numpy().reshape(3 * v, -1), n)[:, kept]
        w, miss = int_weights(rng, 3 * v, c), int_miss(rng, 3 * v)
        d_w, d_miss = torch.from_numpy(w).to(DEV), torch.from_numpy(miss).to(DEV)
        r = eng.record_size
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((eng.kept_count * c,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.sample_scores(d, d_w[i * v:(i + 1) * v], miss=d_miss[i * v:(i + 1) * v], records_offset=i * v * r, out=outs[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            want, _ = SR.score_from_codes(codes[i * v:(i + 1) * v], w[i * v:(i + 1) * v], miss[i * v:(i + 1) * v])
            assert np.array_equal(outs[i].view(-1, c).cpu().numpy(), want), f"stream {i}"


@pytest.mark.parametrize("n,keep,c", [(300, "all", 2), (2504, "p50", 8), (9000, "p1", 1)])
def test_hip_graph_replayed_twice_accumulates(n, keep, c):
    """A linear capture on one stream of an ACCUMULATE call (one kernel, no memset), replayed twice onto zeros: twice the sums."""
    rng = np.random.default_rng(5 + n)
    kept = kept_sets(n, rng)[keep]
    v = 257
    r = rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        w, miss = int_weights(rng, v, c), int_miss(rng, v)
        d_w, d_miss = torch.from_numpy(w).to(DEV), torch.from_numpy(miss).to(DEV)
        out = torch.zeros(eng.kept_count * c, dtype=torch.float64, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.sample_scores(d_recs, d_w, miss=d_miss, out=out, accumulate=True)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.sample_scores(d_recs, d_w, miss=d_miss, out=out, accumulate=True)
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        d_recs.copy_(torch.from_numpy(recs))
        out.zero_()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        want, _ = SR.score_ref(recs.reshape(v, r), n, w, miss, kept)
        assert np.array_equal(out.view(-1, c).cpu().numpy(), 2.0 * want)
        eng.use_torch_stream()


@pytest.mark.parametrize("n,keep", [(7, "all"), (300, "p50"), (2504, "last"), (30_000, "p1")])
def test_unit_weights_equal_the_counts_and_the_matrix(n, keep):
    """w = 1, no miss: het + 2 hom-alt of sample_counts; miss = 3: the column sums of decode_matrix's raw codes."""
    rng = np.random.default_rng(11 * n)
    kept = kept_sets(n, rng)[keep]
    v = 777
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        ones = torch.ones(v, dtype=torch.float32, device=DEV)
        got = eng.sample_scores(d, ones).cpu().numpy()
        cts = eng.sample_counts(d, n_variants=v).cpu().numpy().view(np.uint32).astype(np.int64)
        assert got.shape == (eng.kept_count, 1)
        assert np.array_equal(got[:, 0], (cts[:, 1] + 2 * cts[:, 2]).astype(np.float64))
        got3 = eng.sample_scores(d, ones, miss=torch.full((v,), 3.0, dtype=torch.float32, device=DEV)).cpu().numpy()
        mat = eng.decode_matrix(d, v, dtype=torch.int32, values=(0, 1, 2, 3)).cpu().numpy().astype(np.int64)
        assert np.array_equal(got3[:, 0], mat.sum(axis=0).astype(np.float64))


@pytest.mark.parametrize("n", [300, 2504])
def test_rounding_stays_inside_the_any_order_bound(n):
    """Random f32 weights of mixed sign across 2^+-20 and f32 miss values in [0, 2], V = 3 000: |got - fsum| <= 1.01 (V + 1) 2^-53
    A[k, c], the bound of ANY summation order of exact terms (derived, not tuned: an f32 accumulator misses it by six orders of
    magnitude)."""
    rng = np.random.default_rng(n + 1)
    v, c = 3000, 3
    w = (rng.choice([-1.0, 1.0], size=(v, c)) * rng.uniform(1.0, 2.0, size=(v, c)) * 2.0 ** rng.uniform(-20.0, 20.0, size=(v, c))).astype(np.float32)
    miss = rng.uniform(0.0, 2.0, size=v).astype(np.float32)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        recs = d.cpu().numpy().reshape(v, -1)
        got = run_scores(eng, c, records=d, weights=torch.from_numpy(w).to(DEV), miss=torch.from_numpy(miss).to(DEV))
    want, a = SR.score_ref(recs, n, w, miss)
    err, lim = np.abs(got - want), SR.bound(v, a)
    print(f"N = {n}: max |got - fsum| / bound = {np.max(err / np.maximum(lim, 1e-300)):.3g}")
    assert (err <= lim).all()
    assert (a > 0).all() and np.abs(want).max() > 0


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        wts = torch.ones(4 * 8 + 1, dtype=torch.float32, device=DEV)
        mis = torch.zeros(5, dtype=torch.float32, device=DEV)
        buf = torch.full((300 * 8 + 8,), SENT, dtype=torch.float64, device=DEV)
        ctx, rp, wp, mp, sp = eng._ctx, recs.data_ptr(), wts.data_ptr(), mis.data_ptr(), buf.data_ptr()
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call = lib.pgenhip_sample_scores
        assert call(None, rp, 75, None, 4, wp, 8, 8, mp, sp, 0) == bad                # NULL ctx
        assert call(ctx, rp, 75, None, 4, wp, 8, 0, mp, sp, 0) == bad                 # no column
        assert call(ctx, rp, 75, None, 4, wp, 9, 9, mp, sp, 0) == bad                 # more than PGENHIP_SCORE_MAX_COLUMNS
        assert call(ctx, rp, 75, None, 4, wp, 7, 8, mp, sp, 0) == bad                 # w_stride < n_columns
        assert call(ctx, rp, 75, None, 4, None, 8, 8, mp, sp, 0) == bad               # NULL weights
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp, None, 0) == bad               # NULL scores
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp, sp + 4, 0) == bad             # scores not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, wp + 2, 8, 8, mp, sp, 0) == bad             # weights not 4-byte aligned
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp + 1, sp, 0) == bad             # miss not 4-byte aligned
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp, sp, 0x20) == bad              # unknown flag bit
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp, sp, 2) == bad                 # the reserved matrix-core shape
        assert call(ctx, rp, 75, None, 4, wp, 8, 8, mp, sp, 3) == bad                 # unknown shape
        assert call(ctx, None, 75, None, 4, wp, 8, 8, mp, sp, 0) == bad               # NULL records
        assert call(ctx, rp, 74, None, 4, wp, 8, 8, mp, sp, 0) == bad                 # stride < R
        assert lib.pgenhip_sample_scores_at(None, rp, offs.data_ptr(), 4, wp, 8, 8, mp, sp, 0) == bad
        assert lib.pgenhip_sample_scores_at(ctx, rp, None, 4, wp, 8, 8, mp, sp, 0) == bad           # NULL offsets
        assert lib.pgenhip_sample_scores_at(ctx, rp, offs.data_ptr(), 4, wp, 8, 8, mp, sp + 4, 0) == bad
        assert call(ctx, rp, 75, None, 2, wp, 1 << 50, 8, mp, sp, 0) == big           # w_stride * n_variants * 4 >= 2^52
        assert call(ctx, rp, 1 << 51, None, 2, wp, 8, 8, mp, sp, 0) == big            # record_stride * n_variants >= 2^52
        assert call(ctx, rp, 1 << 52, offs.data_ptr(), 2, wp, 8, 8, mp, sp, 0) == big  # with a variant list the stride alone
        assert lib.pgenhip_sample_scores_at(ctx, rp, offs.data_ptr(), 2, wp, 1 << 50, 8, mp, sp, 0) == big
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
        # a single row needs no strides
        assert call(ctx, rp, 0, None, 1, wp, 0, 8, mp, sp, 0) == _capi.OK
        eng.wait()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0 writes nothing, whatever the pointers
        assert _capi.lib.pgenhip_sample_scores(eng._ctx, None, 75, None, 4, wts.data_ptr(), 8, 8, None, None, 0) == _capi.OK
        assert eng.sample_scores(recs, wts[:32].view(4, 8)).shape == (0, 8)
