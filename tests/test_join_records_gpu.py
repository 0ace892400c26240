"""Sample-wise join of records — GPU leg (pgenhip_join_records through GtEngine.join_records): both forced shapes and AUTO,
byte-equal to numpy (tests/join_ref.py).  Source buffers are 0xFF outside the sample bits (dirty pad bits, dirty gaps), source records
sit at odd byte addresses, the output rows lie in a sentinel-filled buffer at a byte phase with a padded pitch, and every byte
outside the records is unchanged.  JOIN_BLOCKS forces grids of 1, 2 and 3 blocks to walk the grid strides."""
import ctypes as C

import numpy as np
import pytest
import torch

import join_ref as JR
import pack_ref as PR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
SIZES = [(1,), (3, 5), (1, 1, 1, 1, 1, 1, 1, 1), (16, 16), (17, 1, 2, 44), (63, 64, 65), (5, 0, 6), (300, 2504), (70001, 3)]
# STREAM's fast path at every bit phase ls & 3, 19, 20 and 21 bytes from the record's end, in the first, a middle and the last of eight
# parts (starts of every residue mod 4): tests/test_join_records.py holds these lists against the kernel's branch conditions
SIZES += [(1, 400), (2, 401, 3), (3, 90, 333), (84, 85, 86, 87, 84, 90, 99, 101)]
PHASE_SIZES = (17, 1, 2, 44, 70, 9)   # test_every_output_address_phase
SHAPES = [_capi.JOIN_GENERAL, _capi.JOIN_STREAM, _capi.JOIN_AUTO]
MODES = ["plain", "flip", "absent", "repeat"]


def rows_for(sizes):
    return [3] if sizes == (70001, 3) else [1, 2, 257]


def make_part(rng, n, v, p):
    """A part of ``n`` samples with ``v`` source rows: (host base, the offsets of its rows).  Records start at odd addresses, in
    reverse order, 0xFF between them and in their pad bits."""
    r = (n + 3) // 4
    gap = r + 3 + (r + 3) % 2   # even pitch from an odd start: every record at an odd address
    base = np.full(1 + v * gap + 16, 0xFF, dtype=np.uint8)
    offs = np.array([1 + (v - 1 - j) * gap for j in range(v)], dtype=np.int64)
    if n:
        recs = PR.pack_codes(rng.integers(0, 4, size=(v, n), dtype=np.uint8))
        if n % 4:
            recs[:, -1] |= (0xFF << (2 * (n % 4))) & 0xFF
        for j in range(v):
            base[offs[j]:offs[j] + r] = recs[j]
    assert (offs % 2 == 1).all()
    return base, offs


def case(sizes, v, mode, seed):
    """-> the parts as join_ref takes them"""
    rng = np.random.default_rng(seed)
    parts = []
    for p, n in enumerate(sizes):
        base, offs = make_part(rng, n, v, p)
        flip = None
        if mode == "flip":
            flip = rng.integers(0, 2, size=v, dtype=np.uint8) * np.uint8(1 + 126 * (p % 2))   # any nonzero byte flips
        elif mode == "absent":
            offs = np.where(rng.random(v) < 0.3, JR.ABSENT, offs)
            flip = rng.integers(0, 2, size=v, dtype=np.uint8) if p % 2 else None
        elif mode == "repeat" and v > 1:
            offs[v - 1] = offs[0]   # two output rows name one source row
            offs[v // 2] = offs[0]
        parts.append([base, offs, n, flip])
    if mode == "absent":
        parts[len(sizes) // 2][1][0] = JR.ABSENT   # a whole part absent in row 0
        for part in parts:
            part[1][v - 1] = JR.ABSENT             # every part absent in the last row
    return [tuple(p) for p in parts]


def to_dev(parts):
    return [(torch.from_numpy(b).to(DEV), torch.from_numpy(np.ascontiguousarray(o)).to(DEV), n, None if f is None else torch.from_numpy(f).to(DEV))
            for b, o, n, f in parts]


def run_and_check(eng, parts, dparts, v, shape, phase, pad, want, what):
    r = want.shape[1]
    stride = r + pad
    buf = torch.full((phase + v * stride + 64,), SENT, dtype=torch.uint8, device=DEV)
    res = eng.join_records(dparts, v, out=buf, out_stride=stride, out_offset=phase, shape=shape)
    torch.cuda.synchronize()
    assert tuple(res.shape) == (v, r)
    expect = np.full(buf.shape, SENT, dtype=np.uint8)
    for j in range(v):
        expect[phase + j * stride:phase + j * stride + r] = want[j]
    got = buf.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, f"{what} shape={shape} phase={phase} pad={pad}: first differing byte {bad[0]} of {bad.size} (row {(bad[0] - phase) // stride}, byte {(bad[0] - phase) % stride})"


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_join_against_numpy(sizes):
    n_out = sum(sizes)
    with pgen_rs_amd.GtEngine(n_out, device=0) as eng:
        assert eng.record_size == (n_out + 3) // 4
        i = 0
        for v in rows_for(sizes):
            for m, mode in enumerate(MODES):
                parts = case(sizes, v, mode, 1000 * len(sizes) + 10 * v + m)
                want = JR.join(parts, v)
                if mode == "absent":
                    assert (want[v - 1, :n_out // 4] == 0xFF).all()
                dparts = to_dev(parts)
                for shape in SHAPES:
                    for blocks in (1, 2, 3):
                        eng.tune(_capi.KNOB_JOIN_BLOCKS, blocks)
                        i += 1
                        run_and_check(eng, parts, dparts, v, shape, phase=(5 * i + 1) % 16, pad=1 + i % 3 * 2, want=want,
                                      what=f"sizes={sizes} V={v} mode={mode} blocks={blocks}")
                eng.tune(_capi.KNOB_JOIN_BLOCKS, 0)
                run_and_check(eng, parts, dparts, v, _capi.JOIN_AUTO, phase=0, pad=0, want=want, what=f"sizes={sizes} V={v} mode={mode} grid by shape")


def test_every_output_address_phase():
    """One seam-rich case at each of the 16 byte phases of the output, dense pitch and padded: the head and tail bytes of every row."""
    sizes, v = PHASE_SIZES, 5
    parts = case(sizes, v, "flip", 77)
    want = JR.join(parts, v)
    dparts = to_dev(parts)
    with pgen_rs_amd.GtEngine(sum(sizes), device=0) as eng:
        for phase in range(16):
            for shape in (_capi.JOIN_GENERAL, _capi.JOIN_STREAM):
                run_and_check(eng, parts, dparts, v, shape, phase, phase % 2, want, f"sizes={sizes}")


def test_graph_capture():
    sizes, v = (63, 64, 65), 9
    parts = case(sizes, v, "flip", 5)
    want = JR.join(parts, v)
    dparts = to_dev(parts)
    with pgen_rs_amd.GtEngine(sum(sizes), device=0) as eng:
        out = torch.zeros(v * want.shape[1], dtype=torch.uint8, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.join_records(dparts, v, out=out)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.join_records(dparts, v, out=out)
        # the graph keeps the part table it was captured with: new record bytes behind the same pointers
        parts2 = case(sizes, v, "flip", 6)
        for (b, _, _, f), (b2, _, _, f2) in zip(dparts, parts2):
            b.copy_(torch.from_numpy(b2))
            f.copy_(torch.from_numpy(f2))
        out.fill_(SENT)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().reshape(v, -1) == JR.join(parts2, v)).all()


def call(eng, table, n_parts, v, d_out, stride, flags):
    return _capi.lib.pgenhip_join_records(eng._ctx, table, n_parts, v, d_out, stride, flags)


def test_refusals_leave_the_output_untouched():
    sizes, v = (3, 5), 4
    parts = case(sizes, v, "plain", 3)
    dparts = to_dev(parts)
    r = 2
    buf = torch.full((64,), SENT, dtype=torch.uint8, device=DEV)

    def table(counts=(3, 5), reserved=(0, 0), null_base=False, null_off=False, off_shift=0):
        t = (_capi.JoinPart * 9)()
        for i, (b, o, _, _) in enumerate(dparts):
            t[i] = _capi.JoinPart(None if null_base and i == 1 else b.data_ptr(), None if null_off and i == 1 else o.data_ptr() + off_shift, None,
                                  counts[i], reserved[i])
        return t

    BAD, BIG = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
    with pgen_rs_amd.GtEngine(8, device=0) as eng, pgen_rs_amd.GtEngine(8, [0, 2, 5], device=0) as sub, \
            pgen_rs_amd.GtEngine(8, list(range(8)), device=0) as ident:
        out = buf.data_ptr() + 8
        cases = [
            ("parts NULL", call(eng, None, 2, v, out, r, 0), BAD),
            ("n_parts 0", call(eng, table(), 0, v, out, r, 0), BAD),
            ("n_parts 9", call(eng, table(), 9, v, out, r, 0), BAD),
            ("reserved", call(eng, table(reserved=(0, 1)), 2, v, out, r, 0), BAD),
            ("sample sum", call(eng, table(counts=(3, 4)), 2, v, out, r, 0), BAD),
            ("sample sum past 2^32", call(eng, table(counts=(2**32 - 1, 9)), 2, v, out, r, 0), BAD),
            ("proper subset", call(sub, table(counts=(1, 2)), 2, v, out, 1, 0), BAD),
            ("NULL d_base", call(eng, table(null_base=True), 2, v, out, r, 0), BAD),
            ("NULL d_record_off", call(eng, table(null_off=True), 2, v, out, r, 0), BAD),
            ("unaligned d_record_off", call(eng, table(off_shift=4), 2, v, out, r, 0), BAD),
            ("d_out NULL", call(eng, table(), 2, v, None, r, 0), BAD),
            ("out_stride < R", call(eng, table(), 2, v, out, r - 1, 0), BAD),
            ("unknown shape", call(eng, table(), 2, v, out, r, 3), BAD),
            ("unknown flag bit", call(eng, table(), 2, v, out, r, 0x10), BAD),
            ("too large", call(eng, table(), 2, v, out, 2**50, 0), BIG),
        ]
        for what, got, want in cases:
            assert got == want, what
        assert _capi.lib.pgenhip_last_error_detail() != b""
        # legal edges: nothing to write is OK whatever the pointers; one row may have any stride; an identity list counts as all samples
        assert call(eng, table(), 2, 0, None, 0, 0) == _capi.OK
        with pgen_rs_amd.GtEngine(0, device=0) as empty:
            assert call(empty, table(counts=(0, 0), null_base=True, null_off=True), 2, v, None, 0, 0) == _capi.OK
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENT).all()
        assert call(ident, table(), 2, 1, out, 0, _capi.JOIN_STREAM) == _capi.OK
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[8:10] == JR.join(parts, 1)[0]).all() and (got[:8] == SENT).all() and (got[10:] == SENT).all()
