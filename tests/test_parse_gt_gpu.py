"""GT text to records on the device: ``pgenhip_parse_gt`` (gt_parse.hip) in its three shapes against the oracle's text of synthesised
records (round trip) and against tests/parse_ref.py (everything that is not fixed-width).  Bit-exact throughout: records with pad
bits zero, flag words, and sentinels in front of, between and behind the rows and the flag words."""
import numpy as np
import pytest
import torch

import parse_plan
import parse_ref
import pgen_oracle as oracle
from pgen_rs_amd import GtEngine, PgenHipError, _capi
from test_parse_gt import case_lines, gt_case_names

pytestmark = pytest.mark.gpu

SHAPES = (_capi.PARSE_FIXED, _capi.PARSE_GENERAL, _capi.PARSE_AUTO)
SENT, FLAG_SENT = 0xA5, 0x5A5A5A5A
V_RT = 70


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: torch wants a writable array)


class Launch:
    """One call with sentinels everywhere: the text ``lead`` bytes into its buffer, rows at ``out_lead`` + j * (R + pad)."""

    def __init__(self, eng, text: bytes, field_off, line_end, lead=0, out_lead=0, pad=3, text_len=None):
        self.eng, self.n, self.r = eng, eng.sample_count, eng.record_size
        self.v = len(field_off)
        self.text = dev(np.frombuffer(bytes(lead) + bytes(text) + bytes(16), dtype=np.uint8).copy())
        self.lead, self.text_len = lead, len(text) if text_len is None else text_len
        self.fo, self.le = dev(np.asarray(field_off, dtype=np.int64)), dev(np.asarray(line_end, dtype=np.int64))
        self.out_lead, self.stride = out_lead, self.r + pad
        self.out_size = 64 + out_lead + self.v * self.stride + 64
        self.out0 = 64 + out_lead

    def want_out(self, records: np.ndarray, rows=None):
        buf = np.full(self.out_size, SENT, dtype=np.uint8)
        for j in (range(self.v) if rows is None else rows):
            buf[self.out0 + j * self.stride:self.out0 + j * self.stride + self.r] = records[j]
        return dev(buf)

    def want_flags(self, flags):
        buf = np.full(self.v + 2, FLAG_SENT, dtype=np.int32)
        buf[1:self.v + 1] = np.asarray(flags, dtype=np.uint32).astype(np.int32)
        return dev(buf)

    def run(self, shape):
        out = torch.full((self.out_size,), SENT, dtype=torch.uint8, device="cuda")
        flags = torch.full((self.v + 2,), FLAG_SENT, dtype=torch.int32, device="cuda")
        self.eng.parse_gt(self.text, self.fo, self.le, out=out, out_stride=self.stride, out_offset=self.out0, shape=shape,
                          text_offset=self.lead, text_len=self.text_len, line_flags=flags[1:self.v + 1])
        return out, flags


def fixed_text(n, v, first_variant=0):
    """(records with pad bits zero, the oracle's text, field_off, line_end) of v synthesised rows."""
    recs = oracle.synth_records(n, v, first_variant=first_variant)
    text = oracle.decode_emit(recs, v, n).tobytes()
    fo = np.arange(v, dtype=np.int64) * (4 * n + 1)
    return parse_ref.mask_pad(recs.reshape(v, -1), n), text, fo, fo + 4 * n


ROUND_TRIP_N = sorted({*range(1, 10), 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                       *[e + d for e in parse_plan.edge_sample_counts() for d in (-1, 0, 1)]})


@pytest.mark.parametrize("n", ROUND_TRIP_N)
def test_round_trip(n):
    recs, text, fo, le = fixed_text(n, V_RT)
    with GtEngine(n, device=0) as eng:
        wants = {}
        for lead in range(16):   # the alignment of line 0's field_off (the lines behind it take every other one: 4 N + 1 is odd)
            out_lead = (0, 1, 7)[lead % 3]
            launch = Launch(eng, text, fo, le, lead=lead, out_lead=out_lead)
            if out_lead not in wants:
                wants[out_lead] = (launch.want_out(recs), launch.want_flags(np.zeros(V_RT)))
            if lead in (3, 4, 5):
                eng.tune(_capi.KNOB_PARSE_BLOCKS, {3: 1, 4: 2, 5: 7}[lead])
            for shape in SHAPES:
                out, flags = launch.run(shape)
                assert torch.equal(out, wants[out_lead][0]) and torch.equal(flags, wants[out_lead][1]), (lead, shape)
            eng.tune(_capi.KNOB_PARSE_BLOCKS, 0)
        launch = Launch(eng, text.replace(b"/", b"|"), fo, le, lead=5, out_lead=1)
        want_flags = launch.want_flags(np.full(V_RT, _capi.PARSE_PHASED))
        for shape in SHAPES:
            out, flags = launch.run(shape)
            assert torch.equal(out, wants[1][0]) and torch.equal(flags, want_flags), shape


@pytest.mark.parametrize("name", gt_case_names())
def test_committed_cases(name):
    n, text, fo, le, want = case_lines(name)
    with GtEngine(n, device=0) as eng:
        launch = Launch(eng, text, fo, le, lead=1, out_lead=2)
        want_out, want_flags = launch.want_out(want), launch.want_flags(np.zeros(len(fo)))
        for shape in SHAPES:
            out, flags = launch.run(shape)
            assert torch.equal(out, want_out) and torch.equal(flags, want_flags), shape


def form_lines(rng, n, v, fixed_share=0.0):
    """v regions whose fields are drawn from the whole form table (or, with probability fixed_share, are fixed-width)."""
    fixed = [f for f, _, _ in parse_ref.FORMS if len(f) == 3 and parse_ref.fixed_takes(b"\t" + f, 1)]
    regions = []
    for _ in range(v):
        pool = fixed if rng.random() < fixed_share else [f for f, _, _ in parse_ref.FORMS]
        regions.append(b"".join(b"\t" + pool[i] for i in rng.integers(0, len(pool), size=n)))
    return regions


def lay_out(regions, sep=b"\n", prefix=b""):
    """Text of the regions, each behind `prefix` and followed by `sep`; field_off, line_end."""
    text, fo, le = bytearray(), [], []
    for reg in regions:
        text += prefix
        fo.append(len(text))
        text += reg
        le.append(len(text))
        text += sep
    return bytes(text), np.array(fo, dtype=np.int64), np.array(le, dtype=np.int64)


def check_against_ref(eng, text, fo, le, shapes=(_capi.PARSE_GENERAL, _capi.PARSE_AUTO), **kw):
    launch = Launch(eng, text, fo, le, **kw)
    recs, flags = parse_ref.parse_lines(text[:launch.text_len], fo, le, eng.sample_count)
    want_out, want_flags = launch.want_out(recs), launch.want_flags(flags)
    for shape in shapes:
        out, got = launch.run(shape)
        assert torch.equal(got, want_flags), (shape, got.cpu().numpy()[1:-1][:8], flags[:8])
        assert torch.equal(out, want_out), shape
    return launch, recs, flags


def test_variable_width_lines_across_every_chunk_boundary():
    """GENERAL cuts a line into chunks from the line's own start.  A first field that grows by one byte per line, from 0 to one chunk,
    slides the fields behind it over the chunk grid: every offset of the chunk boundary inside a run of fields from the whole form
    table is taken by some line."""
    rng = np.random.default_rng(21)
    n = 260
    tails = form_lines(rng, n - 1, 8)
    assert min(len(t) for t in tails) > parse_plan.CHUNK_BYTES
    regions = [b"\t0/1:" + b"9" * k + tails[k % len(tails)] for k in range(parse_plan.CHUNK_BYTES + 1)]
    text, fo, le = lay_out(regions)
    with GtEngine(n, device=0) as eng:
        for lead, blocks in ((0, 0), (1, 0), (2, 3), (7, 0)):   # the four phases of the text against the chunks' dwords
            eng.tune(_capi.KNOB_PARSE_BLOCKS, blocks)
            check_against_ref(eng, text, fo, le, lead=lead, out_lead=lead % 5, pad=lead % 3)


def test_mixed_launch_and_forced_fixed_declines():
    rng = np.random.default_rng(22)
    n = 37
    fixed = form_lines(rng, n, 40, fixed_share=1.0)
    almost = []
    for k, reg in enumerate(form_lines(rng, n, 12, fixed_share=1.0)):   # 4 N bytes, one field outside the pattern
        b = bytearray(reg)
        f = int(rng.integers(0, n))
        b[4 * f:4 * f + 4] = (b"\t0:1", b"\t2/0", b"\t0/2", b"\t1:.")[k % 4]
        almost.append(bytes(b))
    variable = form_lines(rng, n, 12)
    regions = fixed + almost + variable
    order = rng.permutation(len(regions))
    regions = [regions[i] for i in order]
    with GtEngine(n, device=0) as eng:
        for blocks in (0, 1, 3):
            eng.tune(_capi.KNOB_PARSE_BLOCKS, blocks)
            text, fo, le = lay_out(regions)
            launch, recs, flags = check_against_ref(eng, text, fo, le, lead=3, out_lead=1)
            takes = [parse_ref.fixed_takes(r, n) for r in regions]
            assert sum(takes) == len(fixed)
            out, got = launch.run(_capi.PARSE_FIXED)
            want_flags = [fl if t else _capi.PARSE_DECLINED for fl, t in zip(flags, takes)]
            assert torch.equal(got, launch.want_flags(want_flags))
            assert torch.equal(out, launch.want_out(recs, rows=[j for j, t in enumerate(takes) if t]))


def test_late_malformed_field_of_a_line_split_over_many_blocks():
    n = 70_001
    recs, text, fo, le = fixed_text(n, 3)
    bad = bytearray(text)
    at = int(fo[1]) + 4 * (n - 5)
    bad[at:at + 4] = b"\t0/2"
    with GtEngine(n, device=0) as eng:
        assert parse_plan.blocks_per_row(eng.record_size) >= 16
        launch, _, flags = check_against_ref(eng, bytes(bad), fo, le, lead=2)
        assert list(flags) == [0, _capi.PARSE_ALLELE_RANGE, 0]
        out, got = launch.run(_capi.PARSE_FIXED)
        assert torch.equal(got, launch.want_flags([0, _capi.PARSE_DECLINED, 0])) and torch.equal(out, launch.want_out(recs, rows=[0, 2]))


def test_field_count_crlf_and_clamping():
    rng = np.random.default_rng(23)
    n = 21
    with GtEngine(n, device=0) as eng:
        full = form_lines(rng, n, 3, fixed_share=1.0)
        one_less = [r[:4 * (n - 1)] for r in full]
        one_more = [r + b"\t0/1" for r in full]
        none = [b"", b"0/0\t0/1", b"x" + full[0]]
        regions = full + one_less + one_more + none
        text, fo, le = lay_out(regions)
        _, _, flags = check_against_ref(eng, text, fo, le, shapes=SHAPES[1:], lead=1)
        assert not any(f & _capi.PARSE_FIELD_COUNT for f in flags[:3]) and all(f & _capi.PARSE_FIELD_COUNT for f in flags[3:])
        # CRLF: line_end in front of the '\r'
        text, fo, le = lay_out(full, sep=b"\r\n")
        _, _, flags = check_against_ref(eng, text, fo, le, shapes=SHAPES)
        assert not (flags & ~np.uint32(_capi.PARSE_PHASED | _capi.PARSE_HALF_CALL)).any()
        # line_end past text_len, field_off past text_len, field_off > line_end
        text, fo, le = lay_out(full, sep=b"")
        cut = len(text) - 4 * 6   # the last line loses six fields
        fo2, le2 = np.append(fo, [len(text) + 100, 5]), np.append(le, [len(text) + 200, 2])
        le2[2] = len(text) + 1000
        launch, _, flags = check_against_ref(eng, text, fo2, le2, text_len=cut)
        assert [int(f) & _capi.PARSE_FIELD_COUNT for f in flags] == [0, 0] + [_capi.PARSE_FIELD_COUNT] * 3
        out, got = launch.run(_capi.PARSE_FIXED)
        assert got.cpu().tolist()[1:-1] == [int(f) for f in flags[:2]] + [_capi.PARSE_DECLINED] * 3


def test_text_is_a_view_inside_a_larger_buffer():
    """Valid-looking fields in front of and behind the view: a read outside [text, text + text_len) would change a result."""
    n = 9
    recs, text, fo, le = fixed_text(n, 5)
    with GtEngine(n, device=0) as eng:
        launch = Launch(eng, text, fo, le)
        inner = len(text) - 1 - 4 * 3   # the view ends three fields before the last line's end
        le2 = le.copy()
        le2[-1] = len(text) + 64        # and the last line claims more
        launch.le = dev(le2)
        for lead in (32, 33, 36, 47):   # bytes in front of the view, fields up to its first byte
            big = np.frombuffer((b"\t1|1" * 12)[-lead:] + text + b"\t1|1" * 16, dtype=np.uint8)
            launch.text, launch.lead, launch.text_len = dev(big), lead, inner
            want, flags = parse_ref.parse_lines(text[:inner], fo, le2, n)
            assert flags[-1] == _capi.PARSE_FIELD_COUNT
            for shape in (_capi.PARSE_GENERAL, _capi.PARSE_AUTO):
                out, got = launch.run(shape)
                assert torch.equal(out, launch.want_out(want)) and torch.equal(got, launch.want_flags(flags)), shape
        # fields in front of the view: a region that starts at offset 0 with a field that "continues" a digit to its left
        launch.text, launch.lead, launch.text_len = dev(np.frombuffer(b"\t1/1" * 4 + text, dtype=np.uint8)), 16, len(text)
        launch.le = dev(le)
        for shape in SHAPES:
            out, got = launch.run(shape)
            assert torch.equal(out, launch.want_out(recs)) and not got[1:-1].any(), shape


def test_many_short_lines():
    n, v = 5, 100_000
    recs, text, fo, le = fixed_text(n, v, first_variant=3)
    with GtEngine(n, device=0) as eng:
        launch = Launch(eng, text, fo, le, lead=1, out_lead=1, pad=0)
        want_out, want_flags = launch.want_out(recs), launch.want_flags(np.zeros(v))
        for shape in SHAPES:
            out, flags = launch.run(shape)
            assert torch.equal(out, want_out) and torch.equal(flags, want_flags), shape


def test_text_offsets_past_4gib():
    """Lines whose offsets lie past 2^32: the buffer is untouched (never initialised) except at its end."""
    n = 13
    recs, text, fo, le = fixed_text(n, 40)
    base = (1 << 32) + 4099
    big = torch.empty(base + len(text) + 16, dtype=torch.uint8, device="cuda")
    big[base:base + len(text)] = dev(np.frombuffer(text, dtype=np.uint8))
    with GtEngine(n, device=0) as eng:
        launch = Launch(eng, text, fo + base, le + base)
        launch.text, launch.lead, launch.text_len = big, 0, base + len(text)
        want_out, want_flags = launch.want_out(recs), launch.want_flags(np.zeros(40))
        for shape in SHAPES:
            out, flags = launch.run(shape)
            assert torch.equal(out, want_out) and torch.equal(flags, want_flags), shape
    del big


def test_three_streams_and_a_captured_graph():
    n = 300
    recs, text, fo, le = fixed_text(n, 500)
    rng = np.random.default_rng(24)
    var_text, vfo, vle = lay_out(form_lines(rng, n, 20))
    vrecs, vflags = parse_ref.parse_lines(var_text, vfo, vle, n)
    streams = [torch.cuda.Stream() for _ in range(3)]
    engines = [GtEngine(n, device=0) for _ in range(3)]
    try:
        launches, results = [], []
        for eng, s, (t, a, b) in zip(engines, streams, [(text, fo, le), (var_text, vfo, vle), (text, fo, le)]):
            launches.append(Launch(eng, t, a, b, lead=1))
        torch.cuda.synchronize()
        for eng, s, launch in zip(engines, streams, launches):
            with torch.cuda.stream(s):
                eng.use_stream(s)
                results.append([launch.run(_capi.PARSE_AUTO) for _ in range(3)])
        torch.cuda.synchronize()
        for launch, res, (r, f) in zip(launches, results, [(recs, np.zeros(500)), (vrecs, vflags), (recs, np.zeros(500))]):
            for out, flags in res:
                assert torch.equal(out, launch.want_out(r)) and torch.equal(flags, launch.want_flags(f))
        # a captured graph, replayed twice, on mixed lines (both passes of AUTO and the memset in front of them)
        eng, launch = engines[1], launches[1]
        out = torch.full((launch.out_size,), SENT, dtype=torch.uint8, device="cuda")
        flags = torch.full((launch.v + 2,), FLAG_SENT, dtype=torch.int32, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eng.use_torch_stream()
            eng.parse_gt(launch.text, launch.fo, launch.le, out=out, out_stride=launch.stride, out_offset=launch.out0,
                         text_offset=launch.lead, text_len=launch.text_len, line_flags=flags[1:launch.v + 1])
        for _ in range(2):
            out.fill_(SENT)
            flags.fill_(FLAG_SENT)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, launch.want_out(vrecs)) and torch.equal(flags, launch.want_flags(vflags))
    finally:
        for eng in engines:
            eng.close()


def test_refusals_leave_everything_untouched():
    n = 10
    recs, text, fo, le = fixed_text(n, 4)
    lib = _capi.lib
    with GtEngine(n, device=0) as eng, GtEngine(n, kept_idx=[0, 2, 4], device=0) as sub, GtEngine(n, kept_idx=list(range(n)), device=0) as ident:
        launch = Launch(eng, text, fo, le)
        out = torch.full((launch.out_size,), SENT, dtype=torch.uint8, device="cuda")
        flags = torch.full((8,), FLAG_SENT, dtype=torch.int32, device="cuda")
        t, f, l, o, fl = (x.data_ptr() for x in (launch.text, launch.fo, launch.le, out, flags))
        r, tl = eng.record_size, len(text)

        def call(ctx=eng, text=t, text_len=tl, fo=f, le=l, v=4, out=o + 64, stride=r, flags=fl, shape=_capi.PARSE_AUTO):
            return lib.pgenhip_parse_gt(ctx._ctx, text, text_len, fo, le, v, out, stride, flags, shape)

        bad = _capi.ERR_BAD_ARG
        assert call(text=None) == bad and call(fo=None) == bad and call(le=None) == bad and call(out=None) == bad and call(flags=None) == bad
        assert call(flags=fl + 2) == bad and call(fo=f + 4) == bad and call(le=l + 4) == bad
        assert call(stride=r - 1) == bad
        assert call(shape=3) == bad and call(shape=0x10) == bad and call(shape=0x80000000) == bad
        assert call(stride=(1 << 52) // 4) == _capi.ERR_TOO_LARGE
        assert call(ctx=sub) == bad and b"all samples" in lib.pgenhip_last_error_detail()
        eng.wait()
        assert bool((out == SENT).all()) and bool((flags == FLAG_SENT).all())
        # not refused: no lines (whatever the pointers), one line with a stride below R, an identity list
        assert call(v=0, text=None, fo=None, le=None, out=None, flags=None) == _capi.OK
        assert call(v=1, stride=0) == _capi.OK
        eng.wait()
        assert out[64:64 + r].cpu().numpy().tobytes() == recs[0].tobytes() and bool((out[64 + r:] == SENT).all()) and flags[0].item() == 0
        got, got_flags = ident.parse_gt(launch.text, launch.fo, launch.le, text_len=tl)
        assert np.array_equal(got.cpu().numpy(), recs) and not got_flags.any()
        with pytest.raises(PgenHipError):
            sub.parse_gt(launch.text, launch.fo, launch.le, text_len=tl)
