"""Windowed pairwise tables and r^2 — GPU leg (pgenhip_pair_stats / _at through GtEngine): byte-exact tables against numpy
(tests/pair_ref.py) at every N, V, W, n_left, layout and keep set where gt_pair.hip takes another path, sentinel framing of both
modes, r^2 within one float32 ulp of the exact rational, streams, a captured graph and the argument errors."""
import numpy as np
import pytest
import torch

import launch_plan as LP
import pair_ref as PR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -0x5A5A5A5B                      # 0xA5A5A5A5 as int32
SENT_U = 0xA5A5A5A5
TILE = LP.CONST["pair.kTile"]            # gt_pair.hip's tile of rows, from csrc/launch_plan.h (16: pinned by tests/test_pair_stats.py)
CHUNK = 32 * LP.CONST["pair.kChunkWords"]   # samples per staged chunk


def keep_set(name, n):
    return {
        "all": None,
        "identity": list(range(n)),
        "k0": [],
        "first": [0],
        "last": [n - 1],
        "every7": list(range(0, n, 7)),
        "cluster": list(range(max(0, min(60, n - 1)), min(n, 70))),      # across the 64-sample edge where N reaches it
        "nminus1": [s for s in range(n) if s != n // 2],
    }[name]


KEEPS = ["all", "identity", "k0", "first", "last", "every7", "cluster", "nminus1"]


def launch(eng, mode, v, n_left, w, **kw):
    """One call into a sentinel-framed buffer; returns the n_left * W entries as uint32 words ((.., 16) tables or (..,) r^2 bits).
    TABLE output sits at a 16-byte boundary that is not a 32-byte one, r^2 output at a 4-byte boundary that is not an 8-byte one:
    the alignments the header promises and no more.  Words before and after the entries must keep the sentinel."""
    per = 16 if mode == "table" else 1
    lead = 4 if mode == "table" else 1
    words = per * n_left * w
    dtype = torch.int32 if mode == "table" else torch.float32
    raw = torch.full((lead + words + 8,), SENT, dtype=torch.int32, device=DEV)
    assert raw.data_ptr() % 32 == 0
    out = raw.view(dtype)[lead:]
    at = "base" in kw
    fn = {("table", False): eng.pair_tables, ("table", True): eng.pair_tables_at,
          ("r2", False): eng.pair_r2, ("r2", True): eng.pair_r2_at}[(mode, at)]
    if at:
        res = fn(kw["base"], kw["record_off"], v, n_left=n_left, window=w, out=out)
    else:
        res = fn(n_variants=v, n_left=n_left, window=w, out=out, **kw)
    eng.wait()
    assert tuple(res.shape) == ((n_left, w, 4, 4) if mode == "table" else (n_left, w)) and res.dtype == dtype
    h = raw.cpu().numpy().view(np.uint32)
    assert (h[:lead] == SENT_U).all() and (h[lead + words:] == SENT_U).all(), f"{mode} wrote outside its entries"
    body = h[lead: lead + words]
    return body.reshape(n_left, w, 16) if mode == "table" else body.reshape(n_left, w)


# one comparison for every GPU file: exact tables, r^2 within one ulp and NaN where the reference has it, the sentinel where no pair exists
check_tables, check_r2 = PR.check_tables, PR.check_r2


def both_modes(eng, codes, v, n_left, w, what, **kw):
    want = PR.pair_tables(codes, n_left, w, fill=-1)
    check_tables(launch(eng, "table", v, n_left, w, **kw), want, v, what)
    check_r2(launch(eng, "r2", v, n_left, w, **kw), want, v, what)
    return want


N_LIST = sorted({1, 2, 3, 4, 5, 6, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 300, 2504, CHUNK - 1, CHUNK, CHUNK + 1})


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", KEEPS)
def test_layouts_and_keep_sets_against_numpy(n, keep):
    rng = np.random.default_rng(n * 41 + len(keep))
    kept = keep_set(keep, n)
    r = PR.rsize(n)
    v, w = 21, 5
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    d_raw = torch.from_numpy(raw).to(DEV)
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3), [4, 4, 4]]).astype(np.int32)   # descending, with repeats
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + int(i) * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    vg = len(gather)
    codes = PR.unpack(recs, n, kept)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        k = eng.kept_count
        t = both_modes(eng, codes, v, v, w, "padded stride", records=d_raw, record_stride=stride, records_offset=3)
        both_modes(eng, codes, v, v, w, "dense from an odd base", records=dense, records_offset=1)
        tg = both_modes(eng, codes[gather], vg, vg, w, "gathered", records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather)
        both_modes(eng, codes[gather], vg, vg, w, "_at with gaps", base=d_raw, record_off=d_offs)
        # one row: nothing is written
        assert (launch(eng, "table", 1, 1, w, records=dense, records_offset=1 + r * (v - 1)) == SENT_U).all()
        assert (launch(eng, "r2", 1, 1, w, records=dense, records_offset=1 + r * (v - 1)) == SENT_U).all()
        # a row paired with itself (the repeated 4s at the gather's end): a diagonal table
        self_pair = tg[vg - 2, 0]
        assert (self_pair == np.diag(np.diag(self_pair))).all() and self_pair.sum() == k
        # invariants against the per-variant counts
        counts = eng.genotype_counts(d_raw, record_stride=stride, n_variants=v, records_offset=3).cpu().numpy().view(np.uint32).astype(np.int64)
        for i, d in PR.pair_list(v, v, w):
            assert (t[i, d - 1].sum(axis=1) == counts[i]).all() and (t[i, d - 1].sum(axis=0) == counts[i + d]).all()
            assert t[i, d - 1].sum() == k
        if k == 0:
            assert (t[0, 0] == 0).all()


V_LIST = [2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 2]
W_LIST = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 1000]


@pytest.fixture(scope="module")
def hwe300():
    """60 HWE rows of 300 samples, their codes and the engine they were made with."""
    n, v = 300, 60
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, first_variant=11, hwe=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        yield eng, d, PR.unpack(recs, n), recs


@pytest.mark.parametrize("v", V_LIST)
@pytest.mark.parametrize("w", W_LIST)
def test_v_w_and_n_left_edges(hwe300, v, w):
    """V and W on both sides of the tile and of the 2 x 2 register tile; W = V - 1 and W > V (every pair, the ragged end);
    n_left = 0, 1, V - W, V."""
    eng, d, codes, _ = hwe300
    full = PR.pair_tables(codes[:v], v, w, fill=-1)
    for n_left in sorted({0, 1, max(v - w, 0), v - 1, v}):
        check_tables(launch(eng, "table", v, n_left, w, records=d), full, v, f"V {v} W {w} n_left {n_left}")
    check_r2(launch(eng, "r2", v, v, w, records=d), full, v, f"V {v} W {w}")
    wv = v - 1
    if wv >= 1:
        check_tables(launch(eng, "table", v, v, wv, records=d), PR.pair_tables(codes[:v], v, wv, fill=-1), v, f"V {v} W = V - 1")


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("keep", ["all", "every7"])
def test_forced_grid_walks_the_grid_stride_loop(blocks, keep):
    n, v, w = 300, 70, 20                      # 5 left tiles x 3 right tiles each: 15 numbered tiles, the last ones past the rows
    kept = keep_set(keep, n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        eng.tune(_capi.KNOB_PAIR_BLOCKS, blocks)
        d = eng.synth_records(v, first_variant=5, hwe=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        codes = PR.unpack(recs, n, kept)
        both_modes(eng, codes, v, v, w, f"{blocks} blocks", records=d)
        both_modes(eng, codes, v, v - w, w, f"{blocks} blocks, n_left = V - W", records=d)
        eng.tune(_capi.KNOB_PAIR_BLOCKS, 0)
        both_modes(eng, codes, v, v, w, "grid by shape", records=d)


@pytest.mark.parametrize("keep", ["all", "every7"])
def test_long_rows_count_past_16_bits(keep):
    n, v, w = 500_000, 40, 8
    kept = keep_set(keep, n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(v, first_variant=2, hwe=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        codes = PR.unpack(recs, n, kept)
        got = launch(eng, "table", v, v, w, records=d)
        want = PR.pair_tables(codes, v, w, fill=-1)
        check_tables(got, want, v, "N = 500 000")
        if keep == "all":
            assert want.max() > 1 << 16
        r2 = launch(eng, "r2", v, 4, w, records=d)
        check_r2(r2, want, v, "N = 500 000")


@pytest.mark.parametrize("n", [5, 301, 2503, CHUNK + 2])
def test_dirty_pad_bits_are_not_counted(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v, w = 35, 17
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        both_modes(eng, PR.unpack(recs, n), v, v, w, "dirty pad", records=d)


def test_r2_special_rows():
    """HWE rows beside an all-missing row, a monomorphic row and two identical rows."""
    n = 300
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 12
        d = eng.synth_records(v, first_variant=100, hwe=True)
        r = eng.record_size
        recs = d.cpu().numpy()[: v * r].reshape(v, r).copy()
        recs[3] = 0xFF                        # all missing
        recs[5] = 0x00                        # monomorphic hom-ref
        recs[6] = np.random.default_rng(6).integers(0, 256, size=r, dtype=np.uint8)
        recs[7] = recs[6]                     # identical to its neighbour
        d = torch.from_numpy(recs.reshape(-1)).to(DEV)
        codes = PR.unpack(recs, n)
        w = v - 1
        want = PR.pair_tables(codes, v, w, fill=-1)
        bits = launch(eng, "r2", v, v, w, records=d)
        check_r2(bits, want, v, "special rows")
        got = bits.view(np.float32)
        assert got[6, 0] == np.float32(1.0)                              # identical rows: exactly 1
        for i, dd in PR.pair_list(v, v, w):
            if 3 in (i, i + dd) or 5 in (i, i + dd):
                assert np.isnan(got[i, dd - 1])


def test_python_wrappers_allocate_defined_ragged_ends(hwe300):
    eng, d, codes, _ = hwe300
    v, w = 9, 4
    t = eng.pair_tables(d, n_variants=v, window=w)
    r2 = eng.pair_r2(d, n_variants=v, window=w)
    eng.wait()
    assert t.shape == (v, w, 4, 4) and t.dtype == torch.int32 and r2.shape == (v, w) and r2.dtype == torch.float32
    want = PR.pair_tables(codes[:v], v, w, fill=0)
    assert (t.cpu().numpy().astype(np.int64) == want).all()              # zeros where no pair exists
    exists = (np.arange(v)[:, None] + np.arange(1, w + 1)[None, :]) < v
    assert np.isnan(r2.cpu().numpy()[~exists]).all()
    with pytest.raises(ValueError):
        eng.pair_tables(d, n_variants=v, window=0)
    with pytest.raises(ValueError):
        eng.pair_r2(d, n_variants=v, n_left=v + 1, window=2)
    with pytest.raises(ValueError):
        eng.pair_r2(d, n_variants=v, window=2, out=torch.zeros(3, dtype=torch.float32, device=DEV))


def test_overlapping_launches_on_three_streams():
    n, v, w = 2504, 200, 32
    kept = list(range(0, n, 3))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        r = eng.record_size
        recs = d.cpu().numpy()[: 3 * v * r].reshape(3 * v, r)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((16 * v * w,), SENT, dtype=torch.int32, device=DEV) for _ in range(3)]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.pair_tables(d, n_variants=v, window=w, records_offset=i * v * r, out=outs[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            want = PR.pair_tables(PR.unpack(recs[i * v:(i + 1) * v], n, kept), v, w, fill=-1)
            check_tables(outs[i].cpu().numpy().view(np.uint32).reshape(v, w, 16), want, v, f"stream {i}")


@pytest.mark.parametrize("mode", ["table", "r2"])
def test_hip_graph_capture_and_replay(mode):
    n, v, w = 300, 50, 9
    rng = np.random.default_rng(77)
    r = PR.rsize(n)
    kept = keep_set("every7", n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        per = 16 if mode == "table" else 1
        out = torch.full((per * v * w,), SENT, dtype=torch.int32, device=DEV).view(torch.int32 if mode == "table" else torch.float32)
        call = eng.pair_tables if mode == "table" else eng.pair_r2
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            call(d_recs, n_variants=v, window=w, out=out)      # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            call(d_recs, n_variants=v, window=w, out=out)
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        d_recs.copy_(torch.from_numpy(recs))
        out.view(torch.int32).fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        eng.use_torch_stream()
        want = PR.pair_tables(PR.unpack(recs.reshape(v, r), n, kept), v, w, fill=-1)
        h = out.view(torch.int32).cpu().numpy().view(np.uint32)
        if mode == "table":
            check_tables(h.reshape(v, w, 16), want, v, "graph replay")
        else:
            check_r2(h.reshape(v, w), want, v, "graph replay")


def test_bad_arguments():
    lib = _capi.lib
    T, R2 = _capi.PAIR_TABLE, _capi.PAIR_R2
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 8, dtype=torch.uint8, device=DEV)
        buf = torch.full((16 * 8 * 4 + 8,), SENT, dtype=torch.int32, device=DEV)
        offs = torch.zeros(8, dtype=torch.int64, device=DEV)
        ctx, rp, op = eng._ctx, recs.data_ptr(), buf.data_ptr()
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 0, op, T) == _capi.ERR_BAD_ARG          # window == 0
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 9, 4, op, T) == _capi.ERR_BAD_ARG          # n_left > n_variants
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, op, 2) == _capi.ERR_BAD_ARG          # unknown flag
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, None, T) == _capi.ERR_BAD_ARG        # NULL out with pairs
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, None, R2) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, op + 4, T) == _capi.ERR_BAD_ARG      # tables need 16 bytes
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, op + 8, T) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 8, 4, op + 2, R2) == _capi.ERR_BAD_ARG     # r^2 needs 4 bytes
        assert lib.pgenhip_pair_stats(ctx, None, 75, None, 8, 8, 4, op, T) == _capi.ERR_BAD_ARG        # NULL records
        assert lib.pgenhip_pair_stats(ctx, rp, 74, None, 8, 8, 4, op, T) == _capi.ERR_BAD_ARG          # stride < R
        assert lib.pgenhip_pair_stats_at(ctx, rp, None, 8, 8, 4, op, T) == _capi.ERR_BAD_ARG           # NULL offsets
        assert lib.pgenhip_pair_stats_at(ctx, rp, offs.data_ptr(), 8, 8, 4, op + 4, T) == _capi.ERR_BAD_ARG
        # n_left * window * 64 reaches 2^52: refused before any launch (the records are never read)
        big = 1 << 23
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, big, big, big, op, R2) == _capi.ERR_TOO_LARGE
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, op, T) == _capi.ERR_TOO_LARGE
        # no pair exists: OK whatever the output pointer
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 8, 0, 4, None, T) == _capi.OK
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 1, 1, 4, None, R2) == _capi.OK
        assert lib.pgenhip_pair_stats(ctx, rp, 75, None, 0, 0, 4, None, T) == _capi.OK
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
