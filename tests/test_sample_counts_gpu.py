"""Per-sample genotype counts — GPU leg (pgenhip_sample_counts / _at through GtEngine): every forced shape and AUTO against
numpy (unpack the 2-bit codes, take the kept columns, count along the rows), at every edge of the launch plan
(tests/scount_plan.py), and against the GT text of decode_emit and the per-variant counts."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import scount_plan as SP
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = [_capi.SCOUNT_AUTO, _capi.SCOUNT_ROWS]
SENT = -0x5A5A5A5B   # 0xA5A5A5A5 as int32


def rsize(n):
    return (2 * n + 7) // 8


def np_scounts(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (K, 4) counts of codes 0..3 per kept sample over the rows (pad bits ignored)."""
    v = recs.shape[0]
    codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1).astype(np.int64)


def kept_sets(n, rng):
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def run_scounts(eng, kern, **kw):
    """counts into a sentinel-guarded buffer at a 4-byte-but-not-16-byte offset and at an aligned one; nothing else may change.
    The counts buffer starts dirty: without ACCUMULATE the call overwrites it."""
    k = eng.kept_count
    got = None
    for lead in (1, 4):
        buf = torch.full((lead + 4 * k + 8,), SENT, dtype=torch.int32, device=DEV)
        out = buf[lead:]
        if "base" in kw:
            res = eng.sample_counts_at(kw["base"], kw["record_off"], kw.get("n_variants"), out=out, kernel=kern)
        else:
            res = eng.sample_counts(out=out, kernel=kern, **kw)
        eng.wait()
        h = buf.cpu().numpy()
        assert (h[:lead] == SENT).all() and (h[lead + 4 * k:] == SENT).all(), f"shape {kern} wrote outside its counts"
        assert res.shape == (k, 4) and res.dtype == torch.int32
        g = host(res)
        assert got is None or (g == got).all()
        got = g
    return got


# every edge of the ladder (tests/scount_plan.py, pinned to gt_scount.hip by test_sample_counts.py) +- 1
N_LIST = sorted({1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 257, 300, 2504, 16383, 16384, 16385, 500_000}
                | {n + d for n in SP.CLASS_EDGES for d in (0, 1)})


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_seeded_layouts_against_numpy(n, keep):
    rng = np.random.default_rng(n * 37 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    v = 9 if n >= 100_000 else 41
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    d_raw = torch.from_numpy(raw).to(DEV)
    # descending with repeats: each appearance counts
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + i * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        want = np_scounts(recs, n, kept)
        want_g = np_scounts(recs[gather], n, kept)
        for kern in KERNELS:
            got = run_scounts(eng, kern, records=d_raw, record_stride=stride, records_offset=3, n_variants=v)
            assert (got == want).all(), f"strided, shape {kern}"
            got = run_scounts(eng, kern, records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather)
            assert (got == want_g).all(), f"gathered, shape {kern}"
            got = run_scounts(eng, kern, base=d_raw, record_off=d_offs)
            assert (got == want_g).all(), f"_at, shape {kern}"
            got = run_scounts(eng, kern, records=dense, records_offset=1, n_variants=v)
            assert (got == want).all(), f"dense from an odd base, shape {kern}"
            got = run_scounts(eng, kern, records=dense, records_offset=1 + r * (v - 1), n_variants=1)
            assert (got == np_scounts(recs[-1:], n, kept)).all(), f"one row, shape {kern}"


# rows on both sides of the 8-row batch, of a slot's 255-batch flush window and of the slices' row ranges, with the slices forced
# (PGENHIP_KNOB_SCOUNT_SLICES) so that a window fills with few rows
@pytest.mark.parametrize("n,keep", [(300, "all"), (300, "p50"), (2504, "all"), (2504, "p1"), (5000, "all"), (33, "all")])
@pytest.mark.parametrize("slices", [1, 3])
def test_window_and_slice_edges(n, keep, slices):
    rng = np.random.default_rng(n + 7 * slices)
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    w = SP.window_rows(n, slices)
    vs = sorted({1, slices * SP.slots(n) * SP.BATCH - 1, slices * SP.slots(n) * SP.BATCH + 1, w - 1, w, w + 1, 2 * w + slices})
    vmax = vs[-1]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_SCOUNT_SLICES, slices)
        d = eng.synth_records(vmax, first_variant=3, hwe=True, dirty_pad=False)
        recs = d[: vmax * r].cpu().numpy().reshape(vmax, r)
        for v in vs:
            want = np_scounts(recs[:v], n, kept)
            for kern in KERNELS:
                got = run_scounts(eng, kern, records=d, n_variants=v)
                assert (got == want).all(), f"V = {v}, shape {kern}"


@pytest.mark.parametrize("n", [300, 2504, 70_000])
def test_dirty_pad_bits_are_not_counted(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 67
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        if n % 4:
            assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        for kern in KERNELS:
            got = run_scounts(eng, kern, records=d, n_variants=v)
            assert (got == np_scounts(recs, n)).all()
            assert (got.sum(axis=1) == v).all()


@pytest.mark.parametrize("n,keep", [(300, "all"), (2504, "p50"), (20_000, "p1")])
def test_accumulate_and_overwrite(n, keep):
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        v = 301
        d = eng.synth_records(v, hwe=True)
        r = eng.record_size
        k = eng.kept_count
        whole = eng.sample_counts(d, n_variants=v).clone()
        out = torch.full((4 * k,), 7, dtype=torch.int32, device=DEV)
        eng.sample_counts(d, n_variants=123, out=out)                                  # overwrites the 7s
        eng.sample_counts(d, n_variants=v - 123, out=out, accumulate=True, records_offset=123 * r)
        eng.wait()
        assert (host(out.view(k, 4)) == host(whole)).all(), "two blocks summed in place != one launch over both"
        eng.sample_counts(d, n_variants=0, out=out, accumulate=True)                    # a no-op
        eng.wait()
        assert (host(out.view(k, 4)) == host(whole)).all()
        eng.sample_counts(d, n_variants=0, out=out)                                     # overwrite with nothing: zeros
        eng.wait()
        assert (out.cpu().numpy() == 0).all()


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        buf = torch.full((4 * 300 + 8,), SENT, dtype=torch.int32, device=DEV)
        ctx, rp, cp = eng._ctx, recs.data_ptr(), buf.data_ptr()
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        assert lib.pgenhip_sample_counts(ctx, rp, 75, None, 4, cp, 0x20) == _capi.ERR_BAD_ARG       # unknown flag bit
        assert lib.pgenhip_sample_counts(ctx, rp, 75, None, 4, cp, 3) == _capi.ERR_BAD_ARG          # unknown shape
        assert lib.pgenhip_sample_counts(ctx, rp, 75, None, 4, cp, 1) == _capi.ERR_BAD_ARG          # the unbuilt stream shape
        assert lib.pgenhip_sample_counts(ctx, None, 75, None, 4, cp, 0) == _capi.ERR_BAD_ARG        # NULL records
        assert lib.pgenhip_sample_counts(ctx, rp, 75, None, 4, None, 0) == _capi.ERR_BAD_ARG        # NULL counts
        assert lib.pgenhip_sample_counts(ctx, rp, 74, None, 4, cp, 0) == _capi.ERR_BAD_ARG          # stride < R
        assert lib.pgenhip_sample_counts(ctx, rp, 75, None, 4, cp + 2, 0) == _capi.ERR_BAD_ARG      # counts not 4-byte aligned
        assert lib.pgenhip_sample_counts_at(ctx, rp, None, 4, cp, 0) == _capi.ERR_BAD_ARG           # NULL offsets
        assert lib.pgenhip_sample_counts_at(ctx, rp, offs.data_ptr(), 4, cp + 1, 0) == _capi.ERR_BAD_ARG
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0 writes nothing, whatever the pointer
        assert _capi.lib.pgenhip_sample_counts(eng._ctx, None, 75, None, 4, None, 0) == _capi.OK
        assert eng.sample_counts(recs, n_variants=4).shape == (0, 4)


def test_overlapping_launches_on_three_streams():
    n, v = 2504, 4000
    with pgen_rs_amd.GtEngine(n, kept_idx=list(range(0, n, 3)), device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        recs = d.cpu().numpy().reshape(3 * v, -1)
        r = eng.record_size
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((4 * eng.kept_count,), SENT, dtype=torch.int32, device=DEV) for _ in range(3)]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.sample_counts(d, n_variants=v, records_offset=i * v * r, out=outs[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        kept = list(range(0, n, 3))
        for i in range(3):
            assert (host(outs[i].view(-1, 4)) == np_scounts(recs[i * v:(i + 1) * v], n, kept)).all(), f"stream {i}"


@pytest.mark.parametrize("n,keep", [(300, "all"), (2504, "p50"), (9000, "p1")])
def test_hip_graph_capture_and_replay(n, keep):
    """A linear capture on one stream: the overwrite's memset and the kernel, replayed once on the ctx's stream."""
    rng = np.random.default_rng(5 + n)
    kept = kept_sets(n, rng)[keep]
    v = 257
    r = rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        out = torch.full((4 * eng.kept_count,), SENT, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.sample_counts(d_recs, n_variants=v, out=out)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.sample_counts(d_recs, n_variants=v, out=out)
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        d_recs.copy_(torch.from_numpy(recs))
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert (host(out.view(-1, 4)) == np_scounts(recs.reshape(v, r), n, kept)).all()
        eng.use_torch_stream()


@pytest.mark.parametrize("n,keep", [(7, "all"), (300, "p50"), (2504, "last")])
def test_column_sums_of_gt_text(n, keep):
    """The counts equal decode_emit's GT text counted per column."""
    rng = np.random.default_rng(11 * n)
    kept = kept_sets(n, rng)[keep]
    v = 53
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        gt = eng.decode_emit(d, v)
        got = host(eng.sample_counts(d, n_variants=v))
        eng.wait()
        rows = bytes(gt.cpu().numpy()).split(b"\n")[:v]
        fields = np.array([row.split(b"\t")[1:] for row in rows], dtype=object)
        want = np.stack([(fields == code).sum(axis=0) for code in (b"0/0", b"0/1", b"1/1", b"./.")], axis=1)
        assert (got == want.astype(np.int64)).all()


@pytest.mark.parametrize("n,keep", [(300, "all"), (2504, "p1"), (30_000, "p50")])
def test_totals_equal_the_per_variant_counts(n, keep):
    rng = np.random.default_rng(13 * n)
    kept = kept_sets(n, rng)[keep]
    v = 777
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        per_sample = host(eng.sample_counts(d, n_variants=v))
        per_variant = host(eng.genotype_counts(d, n_variants=v))
        eng.wait()
        assert (per_sample.sum(axis=0) == per_variant.sum(axis=0)).all()
        assert (per_sample.sum(axis=1) == v).all()
