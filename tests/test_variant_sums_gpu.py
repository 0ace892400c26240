"""Per-variant sums of per-sample values by genotype code — GPU leg (pgenhip_variant_sums / _at through GtEngine).

Exact leg: integer values in [-8, 8] make every partial sum of every summation order an integer below 2^53, so GENERAL, the
matrix-core shape and AUTO must equal the reference (tests/vsum_ref.py) bit for bit whatever their plans do: every sample count
class, keep set, column count, row layout and plan edge (tests/vsum_plan.py).  Rounding leg: random FP64 values across 2^+-20
against math.fsum within the bound of any-order summation, (K + 1) 2^-53 A_c.  Cross-checks against genotype_counts and
sample_scores."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import vsum_plan as VP
import vsum_ref as VR
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1.2345e300
COLUMNS = [1, 3, 8, 16]
SHAPES = [_capi.VSUM_GENERAL, _capi.VSUM_MFMA, _capi.VSUM_AUTO]


def rsize(n):
    return (2 * n + 7) // 8


def kept_sets(n, rng):
    """The seven keep sets of test_sample_scores_gpu.py."""
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def int_values(rng, k, c=16):
    return rng.integers(-8, 9, size=(k, c)).astype(np.float64)


def value_tensor(v16: torch.Tensor, c: int) -> torch.Tensor:
    """The first c columns of the (K, 16) device values: a 1-D tensor for c = 1, a contiguous copy for 8 and 16, and for c = 3 a
    view of the 16-wide rows (v_stride 16 > C)."""
    if c == 1:
        return v16[:, 0].contiguous()
    if c == 3:
        return v16[:, :3]
    return v16[:, :c].contiguous()


def run_sums(eng, v, c, at=None, **kw):
    """sums into a sentinel-guarded buffer that starts dirty: the call overwrites its 4 * C * V doubles, and nothing else may change."""
    lead = 3
    buf = torch.full((lead + v * c * 4 + 8,), SENT, dtype=torch.float64, device=DEV)
    out = buf[lead:]
    if at is not None:
        res = eng.variant_sums_at(at[0], at[1], out=out, **kw)
    else:
        res = eng.variant_sums(out=out, **kw)
    eng.wait()
    h = buf.cpu().numpy()
    assert (h[:lead] == SENT).all() and (h[lead + v * c * 4:] == SENT).all(), "wrote outside its sums"
    assert res.shape == (v, c, 4) and res.dtype == torch.float64
    return res.cpu().numpy()


def shapes_for(eng):
    """The forced matrix-core shape needs a kept sample; without one it is refused."""
    return SHAPES if eng.kept_count else [_capi.VSUM_GENERAL, _capi.VSUM_AUTO]


N_LIST = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 257, 300, 2504, 16383, 16384, 16385, 500_000]


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_exact_layouts_against_reference(n, keep):
    rng = np.random.default_rng(n * 43 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    v = 40 if n >= 100_000 else 41
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    codes = VR.unpack_codes(recs, n)
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    k = codes.shape[1]
    d_raw = torch.from_numpy(raw).to(DEV)
    # descending with repeats: each appearance is written
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)
    g = len(gather)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + i * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    v16 = int_values(rng, k)
    d_v16 = torch.from_numpy(v16).to(DEV)
    want, _ = VR.vsum_from_codes(codes, v16)
    want_g = want[gather]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        if not eng.kept_count:
            with pytest.raises(pgen_rs_amd.PgenHipError):
                eng.variant_sums(d_raw, d_v16, record_stride=stride, records_offset=3, n_variants=v, flags=_capi.VSUM_MFMA)
        for c in COLUMNS:
            vals = value_tensor(d_v16, c)
            for shape in shapes_for(eng):
                what = f"C = {c}, shape {shape}"
                got = run_sums(eng, v, c, records=d_raw, values=vals, record_stride=stride, records_offset=3, n_variants=v, flags=shape)
                assert np.array_equal(got, want[:, :c]), f"strided, {what}"
                got = run_sums(eng, g, c, records=d_raw, values=vals, record_stride=stride, records_offset=3, variant_idx=d_gather, flags=shape)
                assert np.array_equal(got, want_g[:, :c]), f"gathered, {what}"
                got = run_sums(eng, g, c, at=(d_raw, d_offs), values=vals, flags=shape)
                assert np.array_equal(got, want_g[:, :c]), f"_at, {what}"
                got = run_sums(eng, v, c, records=dense, values=vals, records_offset=1, flags=shape)
                assert np.array_equal(got, want[:, :c]), f"dense from an odd base, {what}"
                got = run_sums(eng, 1, c, records=dense, values=vals, records_offset=1 + r * (v - 1), n_variants=1, flags=shape)
                assert np.array_equal(got, want[-1:, :c]), f"one row, {what}"


# rows and samples on both sides of every edge of the plan (tests/vsum_plan.py), with the grid forced (PGENHIP_KNOB_VSUM_BLOCKS):
# 1 block walks every tile of every row itself, a small grid makes tiles and slices of one row meet across blocks
@pytest.mark.parametrize("n,c,keep", [(VP.TILE_SAMPLES, 16, "all"), (VP.TILE_SAMPLES + 1, 3, "p50"), (300, 1, "all"), (300, 8, "p50"),
                                      (2504, 16, "p1"), (2504, 3, "all"), (5000, 8, "all")])
@pytest.mark.parametrize("blocks", [1, 3])
def test_plan_edges_rows(n, c, keep, blocks):
    rng = np.random.default_rng(n + 7 * blocks + c)
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    vs = VP.edge_rows(blocks)
    vmax = vs[-1]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_VSUM_BLOCKS, blocks)
        d = eng.synth_records(vmax, first_variant=3, hwe=True, dirty_pad=False)
        codes = VR.unpack_codes(d[: vmax * r].cpu().numpy().reshape(vmax, r), n)
        if kept is not None:
            codes = codes[:, np.asarray(kept, dtype=np.int64)]
        vals = int_values(rng, eng.kept_count, c)
        d_vals = torch.from_numpy(vals).to(DEV)
        want, _ = VR.vsum_from_codes(codes, vals)
        for v in vs:
            for shape in SHAPES:
                got = run_sums(eng, v, c, records=d, values=d_vals, n_variants=v, flags=shape)
                assert np.array_equal(got, want[:v]), f"V = {v}, shape {shape}"


@pytest.mark.parametrize("n", VP.edge_samples())
@pytest.mark.parametrize("blocks", [0, 1, 2])
def test_plan_edges_samples(n, blocks):
    """Sample counts on both sides of the tile edges (a last tile moved back over the one before), all samples and every other one."""
    rng = np.random.default_rng(n + blocks)
    v, c = 37, 5
    for kept in (None, list(range(1, n, 2))):
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            eng.tune(_capi.KNOB_VSUM_BLOCKS, blocks)
            d = eng.synth_records(v, first_variant=1, dirty_pad=True)
            vals = int_values(rng, eng.kept_count, c)
            want, _ = VR.vsum_ref(d.cpu().numpy()[: v * eng.record_size].reshape(v, -1), n, vals, kept)
            for shape in SHAPES:
                got = run_sums(eng, v, c, records=d, values=torch.from_numpy(vals).to(DEV), n_variants=v, flags=shape)
                assert np.array_equal(got, want), f"shape {shape}, kept {'all' if kept is None else 'odd'}"


def test_default_plan_cuts_many_slices():
    """Without the knob a launch of many rows is cut into slices of at least VP.MIN_SLICE_ROWS rows."""
    n, v, c = 300, 8 * VP.MIN_SLICE_ROWS + 77, 2
    rng = np.random.default_rng(8)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        vals = int_values(rng, n, c)
        want, _ = VR.vsum_ref(d.cpu().numpy().reshape(v, -1), n, vals)
        got = run_sums(eng, v, c, records=d, values=torch.from_numpy(vals).to(DEV))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n,keep", [(7, "all"), (300, "p50"), (2504, "last"), (30_000, "p1")])
def test_ones_equal_the_counts_and_the_column_total(n, keep):
    """A column of ones is genotype_counts, exactly; the four sums of a column add up to the kept column total."""
    rng = np.random.default_rng(11 * n)
    kept = kept_sets(n, rng)[keep]
    v = 777
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        vals = int_values(rng, eng.kept_count, 2)
        vals[:, 0] = 1.0
        for shape in SHAPES:
            got = eng.variant_sums(d, torch.from_numpy(vals).to(DEV), flags=shape).cpu().numpy()
            cts = eng.genotype_counts(d, n_variants=v).cpu().numpy().view(np.uint32).astype(np.float64)
            assert np.array_equal(got[:, 0, :], cts.reshape(v, 4))
            assert np.array_equal(got[:, 1, :].sum(axis=1), np.full(v, vals[:, 1].sum()))


@pytest.mark.parametrize("n,keep", [(300, "all"), (2504, "p50")])
def test_weighted_dosage_total_equals_sample_scores(n, keep):
    """sum_j w_j (S[j, c, 1] + 2 S[j, c, 2]) = sum_k values[k, c] * score[k] on integer data, exactly."""
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    v, c = 500, 3
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        vals = int_values(rng, eng.kept_count, c)
        w = rng.integers(-8, 9, size=v).astype(np.float32)
        s = eng.variant_sums(d, torch.from_numpy(vals).to(DEV)).cpu().numpy()
        score = eng.sample_scores(d, torch.from_numpy(w).to(DEV)).cpu().numpy()[:, 0]
        lhs = (w.astype(np.float64)[:, None] * (s[:, :, 1] + 2.0 * s[:, :, 2])).sum(axis=0)
        assert np.array_equal(lhs, vals.T @ score)


@pytest.mark.parametrize("n", [2504, 500_000])
def test_rounding_stays_inside_the_any_order_bound(n):
    """Random FP64 values of mixed sign across 2^+-20, V = 64: |got - fsum| <= 1.01 (K + 1) 2^-53 A_c for both shapes (derived, not
    tuned).  The matrix core adds the four products of a step and the accumulator in an order and with roundings of its own; this
    is where that shows."""
    rng = np.random.default_rng(n + 1)
    v, c = 64, 16
    vals = rng.choice([-1.0, 1.0], size=(n, c)) * rng.uniform(1.0, 2.0, size=(n, c)) * 2.0 ** rng.integers(-20, 21, size=(n, c))
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        recs = d.cpu().numpy().reshape(v, -1)
        want, a = VR.vsum_ref(recs, n, vals)
        lim = VR.bound(n, a)[None, :, None]
        assert (a > 0).all() and np.abs(want).max() > 0
        for shape in (_capi.VSUM_GENERAL, _capi.VSUM_MFMA):
            got = run_sums(eng, v, c, records=d, values=torch.from_numpy(vals).to(DEV), flags=shape)
            err = np.abs(got - want)
            print(f"N = {n}, shape {shape}: max |got - fsum| / bound = {np.max(err / lim):.3g}")
            assert (err <= lim).all()


def test_overlapping_launches_on_three_streams():
    n, v, c = 2504, 4000, 3
    kept = list(range(0, n, 3))
    rng = np.random.default_rng(3)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        codes = VR.unpack_codes(d.cpu().numpy().reshape(3 * v, -1), n)[:, kept]
        vals = int_values(rng, len(kept), c)
        d_vals = torch.from_numpy(vals).to(DEV)
        want, _ = VR.vsum_from_codes(codes, vals)
        r = eng.record_size
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((v * c * 4,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.variant_sums(d, d_vals, records_offset=i * v * r, n_variants=v, out=outs[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            assert np.array_equal(outs[i].view(v, c, 4).cpu().numpy(), want[i * v:(i + 1) * v]), f"stream {i}"


@pytest.mark.parametrize("n,keep,c", [(100, "all", 2), (2504, "p50", 16), (9000, "p1", 1)])
def test_hip_graph_replayed_twice(n, keep, c):
    """A linear capture on one stream (the memset where tiles meet, then the kernel), replayed twice over a dirty buffer: the sums
    of the records the buffer holds at replay, once (the call overwrites)."""
    rng = np.random.default_rng(5 + n)
    kept = kept_sets(n, rng)[keep]
    v = 257
    r = rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        vals = int_values(rng, eng.kept_count, c)
        d_vals = torch.from_numpy(vals).to(DEV)
        out = torch.zeros(v * c * 4, dtype=torch.float64, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.variant_sums(d_recs, d_vals, out=out)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.variant_sums(d_recs, d_vals, out=out)
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        d_recs.copy_(torch.from_numpy(recs))
        out.fill_(SENT)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        want, _ = VR.vsum_ref(recs.reshape(v, r), n, vals, kept)
        assert np.array_equal(out.view(v, c, 4).cpu().numpy(), want)
        eng.use_torch_stream()


def test_far_sums_and_values_past_4_gib():
    """C = 16.  Sums: 2^23 + 5 gathered rows of a 5-sample fileset, 32 * 16 bytes each (4 GiB and a little), compared on the device
    with the sums of the 64 distinct records.  Values: 500 000 kept samples at a row stride of 1 100 doubles (4.4 GB)."""
    rng = np.random.default_rng(99)
    c = 16
    n, distinct, v = 5, 64, (1 << 23) + 5
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        recs = rng.integers(0, 256, size=(distinct, 2), dtype=np.uint8)
        vals = int_values(rng, n)
        want, _ = VR.vsum_ref(recs, n, vals)
        idx = torch.randint(0, distinct, (v,), dtype=torch.int32, device=DEV)
        idx[-1] = distinct - 1
        got = eng.variant_sums(torch.from_numpy(recs.reshape(-1)).to(DEV), torch.from_numpy(vals).to(DEV), variant_idx=idx)
        eng.wait()
        d_want = torch.from_numpy(want).to(DEV)
        assert got.numel() * 8 > 1 << 32
        for lo in range(0, v, 1 << 21):
            hi = min(v, lo + (1 << 21))
            assert torch.equal(got[lo:hi], d_want[idx[lo:hi].long()]), f"rows {lo} .. {hi}"
        del got
    n, v, stride = 500_000, 8, 1100
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        vals = int_values(rng, n)
        big = torch.zeros(n * stride, dtype=torch.float64, device=DEV)
        view = big.view(n, stride)[:, 7:7 + c]
        view.copy_(torch.from_numpy(vals).to(DEV))
        assert (n - 1) * stride * 8 > 1 << 32
        want, _ = VR.vsum_ref(d.cpu().numpy().reshape(v, -1), n, vals)
        for shape in (_capi.VSUM_GENERAL, _capi.VSUM_MFMA):
            got = run_sums(eng, v, c, records=d, values=view, flags=shape)
            assert np.array_equal(got, want), f"shape {shape}"


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        vals = torch.ones(300 * 16 + 1, dtype=torch.float64, device=DEV)
        buf = torch.full((4 * 16 * 4 + 8,), SENT, dtype=torch.float64, device=DEV)
        ctx, rp, vp, sp = eng._ctx, recs.data_ptr(), vals.data_ptr(), buf.data_ptr()
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call = lib.pgenhip_variant_sums
        assert call(None, rp, 75, None, 4, vp, 16, 16, sp, 0) == bad                 # NULL ctx
        assert call(ctx, rp, 75, None, 4, vp, 16, 0, sp, 0) == bad                   # no column
        assert call(ctx, rp, 75, None, 4, vp, 17, 17, sp, 0) == bad                  # more than PGENHIP_VSUM_MAX_COLUMNS
        assert call(ctx, rp, 75, None, 4, vp, 15, 16, sp, 0) == bad                  # v_stride < n_columns
        assert call(ctx, rp, 75, None, 4, None, 16, 16, sp, 0) == bad                # NULL values
        assert call(ctx, rp, 75, None, 4, vp, 16, 16, None, 0) == bad                # NULL sums
        assert call(ctx, rp, 75, None, 4, vp, 16, 16, sp + 4, 0) == bad              # sums not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, vp + 4, 16, 16, sp, 0) == bad              # values not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, vp, 16, 16, sp, 0x10) == bad               # unknown flag bit
        assert call(ctx, rp, 75, None, 4, vp, 16, 16, sp, 3) == bad                  # unknown shape
        assert call(ctx, None, 75, None, 4, vp, 16, 16, sp, 0) == bad                # NULL records
        assert call(ctx, rp, 74, None, 4, vp, 16, 16, sp, 0) == bad                  # stride < R
        assert lib.pgenhip_variant_sums_at(None, rp, offs.data_ptr(), 4, vp, 16, 16, sp, 0) == bad
        assert lib.pgenhip_variant_sums_at(ctx, rp, None, 4, vp, 16, 16, sp, 0) == bad           # NULL offsets
        assert lib.pgenhip_variant_sums_at(ctx, rp, offs.data_ptr(), 4, vp, 16, 16, sp + 4, 0) == bad
        assert call(ctx, rp, 75, None, 2, vp, 1 << 50, 16, sp, 0) == big             # v_stride * K * 8 >= 2^52
        assert call(ctx, rp, 1 << 51, None, 2, vp, 16, 16, sp, 0) == big             # record_stride * n_variants >= 2^52
        assert call(ctx, rp, 1 << 52, offs.data_ptr(), 2, vp, 16, 16, sp, 0) == big  # with a variant list the stride alone
        assert lib.pgenhip_variant_sums_at(ctx, rp, offs.data_ptr(), 2, vp, 1 << 50, 16, sp, 0) == big
        assert call(ctx, rp, 75, None, 0, vp, 16, 16, sp, 0) == _capi.OK             # no row: a no-op
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
        # a single row needs no record stride
        assert call(ctx, rp, 0, None, 1, vp, 16, 16, sp, 0) == _capi.OK
        eng.wait()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0: zeros, whatever the values pointer; the forced MFMA shape is refused
        ctx = eng._ctx
        buf.fill_(SENT)
        assert lib.pgenhip_variant_sums(ctx, rp, 75, None, 4, None, 0, 16, sp, _capi.VSUM_MFMA) == _capi.ERR_BAD_ARG
        assert b"MFMA" in lib.pgenhip_last_error_detail()
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
        assert lib.pgenhip_variant_sums(ctx, rp, 75, None, 4, None, 0, 16, sp, 0) == _capi.OK
        eng.wait()
        h = buf.cpu().numpy()
        assert (h[: 4 * 16 * 4] == 0).all() and (h[4 * 16 * 4:] == SENT).all()
    with pgen_rs_amd.GtEngine(1, device=0) as eng:   # K == 1 needs no value stride
        one = torch.zeros(1, dtype=torch.uint8, device=DEV)
        assert lib.pgenhip_variant_sums(eng._ctx, one.data_ptr(), 1, None, 1, vp, 0, 16, sp, 0) == _capi.OK
        eng.wait()
