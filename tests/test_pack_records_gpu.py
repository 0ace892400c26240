"""Packed records of the kept samples — GPU leg (pgenhip_pack_records / _at through GtEngine): AUTO and every forced shape that
applies, byte-equal to numpy on the record bytes (tests/pack_ref.py), into sentinel-filled buffers at every byte phase with padded
pitches (every byte outside the records unchanged), through every row selection, and back through decode_emit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import pack_ref as PR
import pgen_oracle as oracle
import pgen_rs_amd
from pgen_rs_amd import _capi
from pgen_rs_amd.engine import BED_CODE_MAP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
N_VALUES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16385, 500000]
LAYOUTS = ["dense", "padded", "vidx", "off"]


def rows_for(n):
    return 3 if n == 500000 else 67   # 67 rows: grids of 1, 2 and 3 blocks stride


def kept_sets(n, rng):
    """name -> kept list (None: no list)"""
    out = {"none": None, "identity": list(range(n)), "k0": [], "first": [0], "last": [n - 1], "seventh": list(range(0, n, 7))}
    lo = n // 3
    out["block"] = list(range(lo, min(n, lo + max(1, n // 4))))
    out["half"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    out["but_one"] = [s for s in range(n) if s != n // 2] if n > 1 else [0]
    return out


def shapes_for(kept, n):
    s = [_capi.PACK_AUTO, _capi.PACK_GENERAL]
    if kept is None or len(kept) == n:
        s.append(_capi.PACK_DENSE)
    if kept is not None and len(kept) >= 1:
        s.append(_capi.PACK_GATHER)
    return s


def records(n, v, dirty=False, seed=11):
    r = (n + 3) // 4
    return oracle.synth_records(n, v, first_variant=seed, dirty_pad=dirty).reshape(v, r)


def run_pack(eng, recs, layout, shape, code_map, phase=0, pad=0):
    """Packs the rows of `recs` (V, R) laid out as `layout` into a 0xA5-filled buffer, `phase` bytes in, rows R_K + pad apart.
    -> (the rows the layout selects, the whole buffer, the result view)"""
    v, r = recs.shape
    rk = eng.packed_record_size
    stride = rk + pad
    buf = torch.full((phase + max(v, 1) * max(stride, 1) + 2 * v + 64,), SENT, dtype=torch.uint8, device=DEV)
    kw = dict(out=buf, out_stride=stride, out_offset=phase, code_map=code_map, shape=shape)
    if layout == "dense":
        d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
        res = eng.pack_records(d, n_variants=v, **kw)
        sel = np.arange(v)
    elif layout == "padded":   # an odd pitch from an odd start
        rs = r + 3 if (r + 3) % 2 else r + 4
        host = np.full(1 + v * rs, 0x5A, dtype=np.uint8)
        for j in range(v):
            host[1 + j * rs:1 + j * rs + r] = recs[j]
        res = eng.pack_records(torch.from_numpy(host).to(DEV), rs, n_variants=v, records_offset=1, **kw)
        sel = np.arange(v)
    elif layout == "vidx":   # reversed, with a repeat
        sel = np.arange(v)[::-1].copy()
        if v > 2:
            sel[v // 2] = sel[0]
        d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
        res = eng.pack_records(d, r, torch.from_numpy(sel.astype(np.int32)).to(DEV), n_variants=v, **kw)
    else:   # byte offsets at odd alignments, out of order
        sel = np.arange(v)[::-1].copy()
        gap = r + 5
        host = np.full(3 + v * gap + 16, 0x5A, dtype=np.uint8)
        offs = np.array([3 + int(j) * gap + (int(j) % 3) for j in sel], dtype=np.int64)
        for o, j in zip(offs, sel):
            host[o:o + r] = recs[j]
        res = eng.pack_records_at(torch.from_numpy(host).to(DEV), torch.from_numpy(offs).to(DEV), n_variants=v, **kw)
    torch.cuda.synchronize()
    return sel, buf.cpu().numpy(), res


def check(eng, recs, n, kept, layout, shape, code_map, phase=0, pad=0):
    v = recs.shape[0]
    sel, buf, res = run_pack(eng, recs, layout, shape, code_map, phase, pad)
    want = PR.pack(recs[sel], n, kept, code_map)
    rk = want.shape[1]
    assert tuple(res.shape) == (v, rk)
    expect = np.full(buf.shape, SENT, dtype=np.uint8)
    for j in range(v):
        expect[phase + j * (rk + pad):phase + j * (rk + pad) + rk] = want[j]
    bad = np.nonzero(buf != expect)[0]
    assert bad.size == 0, f"n={n} K={rk} layout={layout} shape={shape} map={code_map} phase={phase}: first differing byte {bad[0]} of {bad.size}"


@pytest.mark.parametrize("n", N_VALUES)
def test_every_keep_set_and_layout(n):
    """Every keep set on this N; layouts, output phases and pitches rotate so that each shape meets each of them."""
    rng = np.random.default_rng(100 + n)
    v = rows_for(n)
    recs = records(n, v)
    for i, (name, kept) in enumerate(kept_sets(n, rng).items()):
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            k = n if kept is None else len(kept)
            assert eng.packed_record_size == (k + 3) // 4
            for t, shape in enumerate(shapes_for(kept, n)):
                layout = LAYOUTS[(i + t) % 4]
                check(eng, recs, n, kept, layout, shape, None, phase=(3 * i + 5 * t + 1) % 16, pad=(i + t) % 3 * 2 + 1)
                check(eng, recs, n, kept, LAYOUTS[(i + t + 1) % 4], shape, BED_CODE_MAP, phase=(7 * i + t) % 16, pad=0 if (i + t) % 2 else 3)


def test_every_residue_of_k():
    """K = 1 .. 33 on one N: K % 16 and K % 4 take every residue."""
    n, v = 300, 67
    rng = np.random.default_rng(9)
    recs = records(n, v)
    for k in range(1, 34):
        kept = sorted(rng.choice(n, size=k, replace=False).tolist())
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            for shape in (_capi.PACK_GATHER, _capi.PACK_GENERAL):
                check(eng, recs, n, kept, LAYOUTS[k % 4], shape, BED_CODE_MAP if k % 2 else None, phase=k % 16, pad=k % 5)


@pytest.mark.parametrize("n,keep", [(1025, "none"), (1025, "half"), (61, "none"), (16385, "seventh")])
def test_output_framing_at_every_byte_phase(n, keep):
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    recs = records(n, 67)
    with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
        pad = 1 if eng.packed_record_size % 2 == 0 else 2   # an odd pitch
        for phase in range(16):
            for shape in shapes_for(kept, n)[1:]:
                check(eng, recs, n, kept, LAYOUTS[phase % 4], shape, None, phase=phase, pad=pad)


@pytest.mark.parametrize("n", [5, 63, 257, 1025, 4097])
def test_dirty_input_pad_bits_give_zero_pad_bits(n):
    rng = np.random.default_rng(n)
    v = 67
    recs = records(n, v, dirty=True)
    assert (recs[:, -1] >> (2 * (n % 4))).any()   # the input's pad bits are set somewhere
    for kept in (None, list(range(n)), kept_sets(n, rng)["but_one"], kept_sets(n, rng)["half"]):
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            k = n if kept is None else len(kept)
            for shape in shapes_for(kept, n):
                for code_map in (None, (3, 3, 3, 3)):
                    check(eng, recs, n, kept, "dense", shape, code_map, phase=1, pad=2)
                    _, _, res = run_pack(eng, recs, "off", shape, code_map)
                    if k % 4:
                        assert not (res.cpu().numpy()[:, -1] >> (2 * (k % 4))).any()


def test_every_map():
    n, v = 1025, 67
    rng = np.random.default_rng(3)
    recs = records(n, v, dirty=True)
    maps = list(itertools.permutations(range(4))) + [(0, 0, 1, 1), (2, 2, 2, 0)]
    assert len(maps) == 26
    for kept in (None, kept_sets(n, rng)["half"], kept_sets(n, rng)["seventh"]):
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            for i, m in enumerate(maps):
                for shape in shapes_for(kept, n)[1:]:
                    check(eng, recs, n, kept, LAYOUTS[i % 4], shape, m, phase=i % 16, pad=i % 3)


@pytest.mark.parametrize("n", [64, 2504, 16385])
def test_forced_shapes_and_small_grids(n):
    rng = np.random.default_rng(n)
    v = 67
    recs = records(n, v)
    sets = kept_sets(n, rng)
    for name in ("none", "identity", "half", "seventh"):
        kept = sets[name]
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            for blocks in (1, 2, 3, 0):
                eng.tune(_capi.KNOB_PACK_BLOCKS, blocks)
                for shape in shapes_for(kept, n):
                    check(eng, recs, n, kept, LAYOUTS[blocks], shape, BED_CODE_MAP, phase=blocks + 1, pad=1)
            d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
            for shape in (_capi.PACK_DENSE, _capi.PACK_GATHER):
                if shape in shapes_for(kept, n):
                    continue
                with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                    eng.pack_records(d, shape=shape)
                assert ei.value.status == _capi.ERR_BAD_ARG and "PGENHIP_PACK_" in str(ei.value)


def test_long_rows_split_over_small_grids():
    """Few rows of very long records: the parts of a row (DENSE) and its dwords (GATHER) walked by grids of 1, 2 and 3 blocks."""
    n, v = 500000, 3
    rng = np.random.default_rng(5)
    recs = records(n, v)
    for kept in (None, kept_sets(n, rng)["half"]):
        with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
            for blocks in (1, 2, 3):
                eng.tune(_capi.KNOB_PACK_BLOCKS, blocks)
                check(eng, recs, n, kept, LAYOUTS[blocks], _capi.PACK_AUTO, None, phase=5 * blocks, pad=blocks)


@pytest.mark.parametrize("n", [64, 300, 2504])
def test_dense_rows_into_dense_output_as_one_stream(n):
    """N a multiple of 4, records and output at their dense pitches: runs of rows go to the kernel as one row.  Row counts around
    the run length (65 536 // R rows), every output phase class, forced grids; N = 301 beside it takes the row-by-row path."""
    r = n // 4
    m = 65536 // r
    for n_, v in ((n, 2 * m - 1), (n, 2 * m), (n, 2 * m + 1), (n, 5 * m + 7), (n + 1, 2 * m + 1)):
        recs = records(n_, v)
        with pgen_rs_amd.GtEngine(n_, device=0) as eng:
            for i, blocks in enumerate((0, 1, 2, 3)):
                eng.tune(_capi.KNOB_PACK_BLOCKS, blocks)
                check(eng, recs, n_, None, "dense", _capi.PACK_DENSE, BED_CODE_MAP if i & 1 else None, phase=(5 * i + v) % 16, pad=0)


def test_empty_calls_write_nothing():
    n = 300
    recs = records(n, 4)
    d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        buf = torch.full((4096,), SENT, dtype=torch.uint8, device=DEV)
        res = eng.pack_records(d, n_variants=0, out=buf)
        assert tuple(res.shape) == (0, 75)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENT).all()
        for shape in (_capi.PACK_AUTO, _capi.PACK_GENERAL, _capi.PACK_DENSE):   # one row: out_stride is not used
            buf.fill_(SENT)
            res = eng.pack_records(d, n_variants=1, out=buf, out_stride=0, out_offset=7, shape=shape)
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert (h[7:82] == PR.pack(recs[:1], n)[0]).all() and (h[:7] == SENT).all() and (h[82:] == SENT).all()
    with pgen_rs_amd.GtEngine(n, [], device=0) as eng:
        assert eng.kept_count == 0 and eng.packed_record_size == 0
        buf = torch.full((4096,), SENT, dtype=torch.uint8, device=DEV)
        for shape in (_capi.PACK_AUTO, _capi.PACK_GENERAL):
            res = eng.pack_records(d, n_variants=4, out=buf, shape=shape)
            assert tuple(res.shape) == (4, 0)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENT).all()


def test_overlapping_launches_on_three_streams():
    n, v = 2504, 3000
    rng = np.random.default_rng(8)
    kept = kept_sets(n, rng)["half"]
    recs = records(n, 3 * v)
    r = recs.shape[1]
    for kp in (None, kept):
        with pgen_rs_amd.GtEngine(n, kp, device=0) as eng:
            d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
            outs = []
            for i, s in enumerate(streams):
                eng.use_stream(s)
                with torch.cuda.stream(s):
                    outs.append(eng.pack_records(d, n_variants=v, records_offset=i * v * r, code_map=BED_CODE_MAP if i & 1 else None))
            torch.cuda.synchronize()
            eng.use_torch_stream()
            for i in range(3):
                want = PR.pack(recs[i * v:(i + 1) * v], n, kp, BED_CODE_MAP if i & 1 else None)
                assert (outs[i].cpu().numpy() == want).all(), f"stream {i}"


@pytest.mark.parametrize("n,keep", [(300, "none"), (2504, "half"), (9000, "seventh")])
def test_hip_graph_keeps_the_map_it_was_captured_with(n, keep):
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    v = 67
    recs = records(n, v)
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
        rk = eng.packed_record_size
        d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
        buf = torch.full((v * (rk + 3) + 32,), SENT, dtype=torch.uint8, device=DEV)
        cmap = (C.c_uint8 * 4)(*BED_CODE_MAP)

        def launch():
            eng.use_torch_stream()
            _capi.check(lib.pgenhip_pack_records(eng._ctx, d.data_ptr(), eng.record_size, None, v, buf.data_ptr() + 5, rk + 3, cmap,
                                                 _capi.PACK_AUTO), "pgenhip_pack_records")

        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launch()
        for c in range(4):
            cmap[c] = 0   # the map's host memory is overwritten; the graph holds its own copy
        want = PR.pack(recs, n, kept, BED_CODE_MAP)
        for rep in range(2):
            buf.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            expect = np.full(h.shape, SENT, dtype=np.uint8)
            for j in range(v):
                expect[5 + j * (rk + 3):5 + j * (rk + 3) + rk] = want[j]
            assert (h == expect).all(), f"replay {rep}"
        eng.use_torch_stream()


def test_refusals():
    n = 300
    recs = records(n, 4)
    d = torch.from_numpy(recs.copy()).to(DEV).view(-1)
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        buf = torch.full((1024,), SENT, dtype=torch.uint8, device=DEV)
        with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
            eng.pack_records(d, out=buf, code_map=(0, 1, 2, 4))
        assert ei.value.status == _capi.ERR_BAD_ARG
        for flags in (4, 8, 0x10, 0x12, 0x80000000):
            with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                eng.pack_records(d, out=buf, shape=flags)
            assert ei.value.status == _capi.ERR_BAD_ARG, flags
        with pytest.raises(pgen_rs_amd.PgenHipError) as ei:   # a pitch below one packed record
            eng.pack_records(d, out=buf, out_stride=74)
        assert ei.value.status == _capi.ERR_BAD_ARG
        call = lambda rs, nv, os_: lib.pgenhip_pack_records(eng._ctx, d.data_ptr(), rs, None, nv, buf.data_ptr(), os_, None, 0)
        assert call(75, 2, 1 << 51) == _capi.ERR_TOO_LARGE      # out_stride * n_variants >= 2^52
        assert call(1 << 51, 2, 75) == _capi.ERR_TOO_LARGE      # record_stride * n_variants >= 2^52
        assert call(1 << 51, 1, 1 << 51) == _capi.OK            # one row: the strides are not used
        vidx = torch.zeros(2, dtype=torch.int32, device=DEV)
        assert lib.pgenhip_pack_records(eng._ctx, d.data_ptr(), 1 << 52, vidx.data_ptr(), 2, buf.data_ptr(), 75, None, 0) == _capi.ERR_TOO_LARGE
        assert lib.pgenhip_pack_records_at(eng._ctx, d.data_ptr(), None, 2, buf.data_ptr(), 75, None, 0) == _capi.ERR_BAD_ARG
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:75] == PR.pack(recs[:1], n)[0]).all() and (h[75:] == SENT).all()   # only the one-row call wrote


@pytest.mark.parametrize("n,keep", [(17, "seventh"), (300, "half"), (2504, "but_one"), (2504, "seventh"), (16385, "half"), (70000, "block")])
def test_closed_loop_through_decode_emit(n, keep):
    """decode_emit of the packed records in a ctx of K samples, all kept == decode_emit with the kept list on the original records."""
    rng = np.random.default_rng(n)
    kept = kept_sets(n, rng)[keep]
    v = 67
    with pgen_rs_amd.GtEngine(n, kept, device=0) as eng:
        d = eng.synth_records(v, hwe=True)
        text = eng.decode_emit(d, v)
        packed = eng.pack_records(d, n_variants=v).contiguous().view(-1)
        with pgen_rs_amd.GtEngine(len(kept), device=0) as eng_k:
            assert eng_k.record_size == eng.packed_record_size
            again = eng_k.decode_emit(packed, v)
        torch.cuda.synchronize()
        assert torch.equal(text, again)
