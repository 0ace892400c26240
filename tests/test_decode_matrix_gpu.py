"""Numeric genotype matrix — GPU leg (pgenhip_decode_matrix / _at through GtEngine): AUTO and every forced shape that applies,
byte-equal to numpy on the record bytes (tests/matrix_ref.py) and therefore to each other, into sentinel-filled buffers with padded
pitches (every byte outside the matrix unchanged), at every edge of the launch plan (tests/matrix_plan.py), and against
decode_emit's text, the per-variant and the per-sample counts."""
import numpy as np
import pytest
import torch

import matrix_plan as MP
import matrix_ref as MR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
NP = {torch.int8: np.int8, torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.float16: np.float16,
      torch.float32: np.float32}
# (dtype, random patterns?)
ELEMS = [(torch.int8, False), (torch.uint8, True), (torch.float16, False), (torch.int16, True), (torch.float32, False), (torch.int32, True)]


def kept_sets(n, rng):
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def patterns(dtype, rnd, rng):
    """-> (values argument of the wrapper, the same four elements as a numpy array of raw integers of the element size)"""
    size = torch.empty(0, dtype=dtype).element_size()
    ut = {1: np.uint8, 2: np.uint16, 4: np.uint32}[size]
    if not rnd:
        return None, MR.default_values(NP[dtype]).view(ut)
    bits = rng.integers(0, 1 << (8 * size), size=4, dtype=np.uint64).astype(ut)
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[size]
    t = torch.from_numpy(bits.view({1: np.uint8, 2: np.int16, 4: np.int32}[size]).copy()).view(dtype) if dtype != it else \
        torch.from_numpy(bits.view({1: np.uint8, 2: np.int16, 4: np.int32}[size]).copy())
    return t, bits


def shapes_for(all_kept, sample_major, tile_aligned):
    s = [_capi.MATRIX_AUTO, _capi.MATRIX_GENERAL]
    if all_kept and not sample_major:
        s.append(_capi.MATRIX_STREAM)
    if all_kept and sample_major and tile_aligned:
        s.append(_capi.MATRIX_TILE)
    return s


def run_matrix(eng, kern, dtype, values, sample_major, v, lead, pitch, **kw):
    """The matrix into a 0xA5-filled buffer, `lead` bytes in, rows `pitch` elements apart; nothing outside it may change.
    -> (rows, cols * itemsize) uint8."""
    size = torch.empty(0, dtype=dtype).element_size()
    k = eng.kept_count
    rows, cols = (k, v) if sample_major else (v, k)
    total = lead + (max(rows, 1) * max(pitch, 1) + 16) * size
    buf = torch.full((total,), SENT, dtype=torch.uint8, device=DEV)
    typed = buf[lead: lead + (max(rows, 1) * max(pitch, 1)) * size].view(dtype)
    out = torch.as_strided(typed, (rows, cols), (max(pitch, 1), 1))
    if "base" in kw:
        res = eng.decode_matrix_at(kw["base"], kw["record_off"], v, sample_major=sample_major, values=values, out=out, kernel=kern)
    else:
        res = eng.decode_matrix(n_variants=v, sample_major=sample_major, values=values, out=out, kernel=kern, **kw)
    eng.wait()
    assert res.shape == (rows, cols) and res.dtype == dtype
    h = buf.cpu().numpy()
    if rows == 0 or cols == 0:
        assert (h == SENT).all(), f"shape {kern} wrote with nothing to write"
        return np.zeros((rows, cols * size), dtype=np.uint8)
    body = h[lead: lead + rows * pitch * size].reshape(rows, pitch * size)
    got = body[:, : cols * size].copy()
    outside = (h[:lead] == SENT).all() and (h[lead + rows * pitch * size:] == SENT).all() and (body[:, cols * size:] == SENT).all()
    assert outside, f"shape {kern} wrote outside the matrix"
    return got


def want_bytes(recs, n, kept, bits, sample_major):
    return MR.raw(MR.matrix(recs, n, kept, bits, sample_major))


def out_configs(cols, size, sample_major):
    """(lead bytes, pitch elements, 16-byte aligned?)"""
    al = 16 // size
    if sample_major:
        p16 = (cols + al - 1) // al * al
        return [(16, p16, True), (16, (cols * size + 127) // 128 * 128 // size + al, True), (16 + size, cols + 3, False), (16 + size, cols, False)]
    return [(16, cols, True), (16 + size, cols, False), (16 + size, cols + 3, False)]


N_LIST = sorted({1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 257, 300, 2504, 16383, 16384, 16385, 500_000}
                | {n + d for n in MP.N_EDGES for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_seeded_layouts_against_numpy(n, keep):
    rng = np.random.default_rng(n * 41 + len(keep))
    kept = kept_sets(n, rng)[keep]
    all_kept = keep in ("all", "identity")
    r = MR.rsize(n)
    v = 3 if n >= 100_000 else 37
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    d_raw = torch.from_numpy(raw).to(DEV)
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)
    d_gather = torch.from_numpy(gather).to(DEV)
    d_offs = torch.from_numpy(np.array([3 + i * stride for i in gather], dtype=np.int64)).to(DEV)
    dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
    layouts = [
        ("strided", dict(records=d_raw, record_stride=stride, records_offset=3), recs, v),
        ("gathered", dict(records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather), recs[gather], len(gather)),
        ("_at", dict(base=d_raw, record_off=d_offs), recs[gather], len(gather)),
        ("dense from an odd base", dict(records=dense, records_offset=1), recs, v),
        ("one row", dict(records=dense, records_offset=1 + r * (v - 1)), recs[-1:], 1),
    ]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        cell = 0
        for dtype, rnd in ELEMS:
            values, bits = patterns(dtype, rnd, rng)
            size = bits.itemsize
            for sample_major in (False, True):
                for li, (name, kw, rows_ref, nv) in enumerate(layouts):
                    cols = nv if sample_major else eng.kept_count
                    cfgs = out_configs(cols, size, sample_major)
                    # the first layout takes every output configuration, the others one each in rotation
                    for lead, pitch, aligned in (cfgs if li == 0 else [cfgs[(cell + li) % len(cfgs)]]):
                        want = want_bytes(rows_ref, n, kept, bits, sample_major)
                        for kern in shapes_for(all_kept, sample_major, aligned):
                            got = run_matrix(eng, kern, dtype, values, sample_major, nv, lead, pitch, **kw)
                            assert got.shape == want.shape and (got == want).all(), \
                                f"{name}, {dtype}, sample_major={sample_major}, lead {lead}, pitch {pitch}, shape {kern}"
                cell += 1


# V at 1 and on both sides of every tile, lane-piece and grid edge of the plan; small grids forced through PGENHIP_KNOB_MATRIX_BLOCKS
# so that the grid-stride loops of all three kernels take several rounds
@pytest.mark.parametrize("n", [5, 300, 513, 2504])
@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_variant_count_and_grid_edges(n, blocks):
    rng = np.random.default_rng(n + 11 * blocks)
    vs = sorted({1, 2} | {e + d for e in MP.V_EDGES for d in (-1, 0, 1)} | {3 * MP.TILE_VARIANTS + 5, 1031})
    vmax = vs[-1]
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        if blocks:
            eng.tune(_capi.KNOB_MATRIX_BLOCKS, blocks)
        d = eng.synth_records(vmax, first_variant=3, dirty_pad=True)
        r = eng.record_size
        recs = d[: vmax * r].cpu().numpy().reshape(vmax, r)
        for dtype, rnd in ELEMS[:1] + ELEMS[3:5]:
            values, bits = patterns(dtype, rnd, rng)
            size = bits.itemsize
            for v in vs:
                for sample_major in (False, True):
                    cols = v if sample_major else n
                    want = want_bytes(recs[:v], n, None, bits, sample_major)
                    for lead, pitch, aligned in out_configs(cols, size, sample_major)[:3]:
                        for kern in shapes_for(True, sample_major, aligned):
                            got = run_matrix(eng, kern, dtype, values, sample_major, v, lead, pitch, records=d)
                            assert (got == want).all(), f"V = {v}, {dtype}, sample_major={sample_major}, lead {lead}, pitch {pitch}, shape {kern}"


def test_refusals():
    lib = _capi.lib
    n, r, v = 300, 75, 4
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        recs = torch.zeros(r * v, dtype=torch.uint8, device=DEV)
        buf = torch.full((64 + 4 * n * 8,), SENT, dtype=torch.uint8, device=DEV)
        offs = torch.zeros(v, dtype=torch.int64, device=DEV)
        ctx, rp, op = eng._ctx, recs.data_ptr(), buf.data_ptr()
        assert op % 16 == 0
        SM = _capi.MATRIX_SAMPLE_MAJOR
        bad = [
            (ctx, rp, r, None, v, op, n, 1, None, 0x20),                       # unknown flag bit
            (ctx, rp, r, None, v, op, n, 1, None, 4),                          # unknown shape
            (ctx, rp, r, None, v, op, n, 3, None, 0),                          # elem_bytes
            (ctx, rp, r, None, v, op, n, 0, None, 0),
            (ctx, rp, r, None, v, op, n, 8, None, 0),
            (ctx, None, r, None, v, op, n, 1, None, 0),                        # NULL records
            (ctx, rp, r, None, v, None, n, 1, None, 0),                        # NULL out
            (ctx, rp, r - 1, None, v, op, n, 1, None, 0),                      # record_stride < R
            (ctx, rp, r, None, v, op, n - 1, 1, None, 0),                      # out_stride < K * elem_bytes
            (ctx, rp, r, None, v, op, 4 * n - 4, 4, None, 0),
            (ctx, rp, r, None, v, op, v - 1, 1, None, SM),                     # sample-major: out_stride < V * elem_bytes
            (ctx, rp, r, None, v, op + 1, 2 * n, 2, None, 0),                  # d_out not a multiple of elem_bytes
            (ctx, rp, r, None, v, op + 2, 4 * n, 4, None, 0),
            (ctx, rp, r, None, v, op, 2 * n + 1, 2, None, 0),                  # out_stride not a multiple of elem_bytes
            (ctx, rp, r, None, v, op, 4 * n + 2, 4, None, 0),
            (ctx, rp, r, None, v, op, n, 1, None, _capi.MATRIX_TILE),          # TILE on the variant-major orientation
            (ctx, rp, r, None, v, op, 16, 1, None, _capi.MATRIX_STREAM | SM),  # STREAM on the sample-major orientation
            (ctx, rp, r, None, v, op + 1, 16, 1, None, _capi.MATRIX_TILE | SM),   # TILE needs 16-byte-aligned rows
            (ctx, rp, r, None, v, op, 17, 1, None, _capi.MATRIX_TILE | SM),
            (ctx, rp, r, None, v, op + 4, 16, 4, None, _capi.MATRIX_TILE | SM),
        ]
        for args in bad:
            assert lib.pgenhip_decode_matrix(*args) == _capi.ERR_BAD_ARG, args[4:]
            assert lib.pgenhip_last_error_detail() != b""
        assert lib.pgenhip_decode_matrix_at(ctx, rp, None, v, op, n, 1, None, 0) == _capi.ERR_BAD_ARG           # NULL offsets
        assert lib.pgenhip_decode_matrix_at(ctx, rp, offs.data_ptr(), v, op + 1, 2 * n, 2, None, 0) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_decode_matrix(None, rp, r, None, v, op, n, 1, None, 0) == _capi.ERR_BAD_ARG          # NULL ctx
        assert lib.pgenhip_decode_matrix_at(None, rp, offs.data_ptr(), v, op, n, 1, None, 0) == _capi.ERR_BAD_ARG
        # offsets that do not fit the kernels' index types: refused before any launch
        assert lib.pgenhip_decode_matrix(ctx, rp, r, None, v, op, 1 << 60, 1, None, 0) == _capi.ERR_TOO_LARGE
        assert lib.pgenhip_decode_matrix(ctx, rp, r, None, v, op, 1 << 60, 4, None, SM) == _capi.ERR_TOO_LARGE
        assert lib.pgenhip_decode_matrix(ctx, rp, 1 << 60, None, v, op, n, 1, None, 0) == _capi.ERR_TOO_LARGE
        # nothing to write: OK whatever the pointers
        assert lib.pgenhip_decode_matrix(ctx, None, r, None, 0, None, 0, 1, None, 0) == _capi.OK
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all(), "a refused call wrote"
    for kept in ([], [1, 5, 7]):
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            k = len(kept)
            assert lib.pgenhip_decode_matrix(eng._ctx, rp, r, None, v, op, max(k, 1), 1, None, _capi.MATRIX_STREAM) == _capi.ERR_BAD_ARG
            assert lib.pgenhip_decode_matrix(eng._ctx, rp, r, None, v, op, 16, 1, None, _capi.MATRIX_TILE | SM) == _capi.ERR_BAD_ARG
            if k == 0:   # K == 0 writes nothing, whatever the pointer
                assert lib.pgenhip_decode_matrix(eng._ctx, None, r, None, v, None, 0, 1, None, 0) == _capi.OK
                assert eng.decode_matrix(recs, v).shape == (v, 0) and eng.decode_matrix(recs, v, sample_major=True).shape == (0, v)
            eng.wait()
            assert (buf.cpu().numpy() == SENT).all()


def test_overlapping_launches_on_three_streams():
    n, v = 2504, 3000
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(3 * v, hwe=True)
        recs = d.cpu().numpy().reshape(3 * v, -1)
        r = eng.record_size
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = []
        for i, s in enumerate(streams):
            eng.use_stream(s)
            with torch.cuda.stream(s):
                outs.append(eng.decode_matrix(d, v, records_offset=i * v * r, dtype=torch.int16, sample_major=bool(i & 1)))
        torch.cuda.synchronize()
        eng.use_torch_stream()
        vals = MR.default_values(np.int16)
        for i in range(3):
            want = MR.matrix(recs[i * v:(i + 1) * v], n, None, vals, bool(i & 1))
            assert (outs[i].cpu().numpy() == want).all(), f"stream {i}"


@pytest.mark.parametrize("n,keep,sample_major", [(300, "all", False), (2504, "all", True), (2504, "p50", True), (9000, "p1", False)])
def test_hip_graph_capture_and_replay(n, keep, sample_major):
    """A captured launch keeps the patterns it was captured with; replayed twice onto a re-poisoned buffer."""
    rng = np.random.default_rng(5 + n)
    kept = kept_sets(n, rng)[keep]
    v = 257
    r = MR.rsize(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        k = eng.kept_count
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        rows, cols = (k, v) if sample_major else (v, k)
        pitch = (cols * 4 + 127) // 128 * 32
        store = torch.full((rows, pitch), 7.0, dtype=torch.float32, device=DEV)
        out = store[:, :cols]
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.decode_matrix(d_recs, v, out=out, sample_major=sample_major)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.decode_matrix(d_recs, v, out=out, sample_major=sample_major, values=[0.0, 0.5, 1.0, -9.0])
        vals = np.array([0.0, 0.5, 1.0, -9.0], dtype=np.float32)
        for rep in range(2):
            recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
            d_recs.copy_(torch.from_numpy(recs))
            store.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            h = store.cpu().numpy()
            assert (h[:, :cols] == MR.matrix(recs.reshape(v, r), n, kept, vals, sample_major)).all(), f"replay {rep}"
            assert (h[:, cols:] == 7.0).all()
        eng.use_torch_stream()


@pytest.mark.parametrize("n,keep", [(7, "all"), (300, "p50"), (2504, "last"), (2504, "all"), (513, "identity")])
def test_cross_checks_inside_the_product(n, keep):
    """The int8 matrix equals decode_emit's text field by field; its row histogram equals genotype_counts, its column histogram
    sample_counts; the sample-major result equals the variant-major one transposed."""
    rng = np.random.default_rng(11 * n)
    kept = kept_sets(n, rng)[keep]
    v = 203
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        k = eng.kept_count
        d = eng.synth_records(v, hwe=True)
        m = eng.decode_matrix(d, v, values=[0, 1, 2, 3])
        mt = eng.decode_matrix(d, v, values=[0, 1, 2, 3], sample_major=True)
        gt = eng.decode_emit(d, v)
        per_variant = eng.genotype_counts(d, n_variants=v)
        per_sample = eng.sample_counts(d, n_variants=v)
        eng.wait()
        hm = m.cpu().numpy()
        assert hm.shape == (v, k) and (hm == MR.gt_text_codes(gt.cpu().numpy(), v, k)).all()
        assert (mt.cpu().numpy() == hm.T).all()
        assert (np.stack([(hm == c).sum(axis=1) for c in range(4)], axis=1) == per_variant.cpu().numpy()).all()
        assert (np.stack([(hm == c).sum(axis=0) for c in range(4)], axis=1) == per_sample.cpu().numpy()).all()


@pytest.mark.parametrize("dtype", [torch.int8, torch.uint8, torch.int16, torch.int32, torch.float16, torch.bfloat16, torch.float32])
def test_wrapper_defaults(dtype):
    """Default patterns per dtype; the default sample-major result is a view at a 128-byte-multiple pitch and went through TILE
    (it equals the forced TILE launch into the same kind of buffer and GENERAL's)."""
    n, v = 1000, 333
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        cd = MR.codes(recs, n)
        m = eng.decode_matrix(d, v, dtype=dtype)
        assert m.shape == (v, n) and m.dtype == dtype and m.is_contiguous()
        t = eng.decode_matrix(d, v, dtype=dtype, sample_major=True)
        size = t.element_size()
        assert t.shape == (n, v) and t.stride(1) == 1 and (t.stride(0) * size) % 128 == 0 and t.stride(0) >= v and t.data_ptr() % 128 == 0
        assert MP.auto_shape(True, True, t.data_ptr(), t.stride(0) * size, n) == MP.TILE
        forced = torch.empty_strided((n, v), t.stride(), dtype=dtype, device=DEV)
        eng.decode_matrix(d, v, out=forced, sample_major=True, kernel=_capi.MATRIX_TILE)
        general = eng.decode_matrix(d, v, dtype=dtype, sample_major=True, kernel=_capi.MATRIX_GENERAL)
        eng.wait()
        last = float("nan") if dtype.is_floating_point else (-1 if dtype.is_signed else 255)
        want = torch.tensor([0, 1, 2, last]).to(dtype)[torch.from_numpy(cd.astype(np.int64))]
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[size]
        assert (m.cpu().view(it) == want.view(it)).all()
        wt = want.t().contiguous().view(it)
        for name, x in (("auto", t), ("tile", forced), ("general", general)):
            assert (x.cpu().contiguous().view(it) == wt).all(), name
