"""The far end of the ABI's index ranges for GT text to records: ``pgenhip_parse_gt`` (gt_parse.hip) with more FIXED items than
32 bits count, output rows and text past 4 GiB, a line across byte 2^32, lines of more than 2^32 bytes, the GENERAL pass's rounds of
picks at the natural grid, and fields and tabless stretches far beyond what tests/test_parse_gt_gpu.py reaches.  The levels and the
records (random bytes, dirty pad bits, row 0 at byte 1, stride R + 1) are test_long_rows_gpu.py's.

The reference is never the parse kernels.  Long rows: ``decode_emit`` writes the text on the device from random records, the text is
held against the records by longrow_ref.check_gt_row (plain torch), and the expected record is the source record with the pad bits of
its last byte cleared.  Edited and variable-width lines: tests/parse_ref.py on the host.  Huge edited lines: only the edited field is
re-derived, by parse_ref.parse_region on those few bytes.  Every comparison is bit-exact; every output and every flag array lies in a
sentinel frame that must come back untouched; every threshold is an assert on parse_plan (the plan header run through its probe) or
on plain arithmetic.  A case is skipped only when the card has less free memory than the case states.

Measured on the MI355X (wall time of one engine call, as each case prints it; the whole test in brackets; the file runs in 5 s):
  a    item pool, 4 190 208 / 4 190 211 / 4 190 213 lines x R 1025: FIXED 0.03 s, AUTO 0.02 s [0.1 - 0.8 s per n_lines]
  b    declined rounds, 4 190 213 lines: AUTO 0.02 s, FIXED 0.03 s [0.1 s]; the cheap twin [0.1 s]
  c    40 rows at stride 2^27 + 3: under 0.01 s per shape [0.03 s]
  d    a line across byte 2^32: GENERAL 0.01 s, FIXED and AUTO under 0.01 s, per phase [0.04 s; 0.9 s with the variable-width
       line, 0.8 s of it parse_ref over 2^20 fields on the host]
  e    N_S32: 0.01 s as emitted, 0.05 s once a line is phased (its waves share one flag word) [0.3 s]; N_MAX: 0.01 s and
       0.10 s [0.6 s]; N_MID with one widened field: GENERAL 0.13 s (two 64-MiB lines, a block each), AUTO 0.13 s [0.3 s]
  f    300 000 fields, a suffix of five tabless chunks: under 0.01 s per call [0.02 s, 0.01 s]
No case was cut to a smaller level.
"""
import time

import numpy as np
import pytest
import torch

import longrow_ref as LR
import parse_plan
import parse_ref
import pgen_oracle as oracle
import pgen_rs_amd
from longrow_ref import GIB, SENT, frame_ok, need_gib, padding_untouched
from pgen_rs_amd import _capi
from test_long_rows_gpu import N_MAX, N_MID, N_S32, Records
from test_parse_gt_gpu import check_against_ref, form_lines, lay_out

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXED, GENERAL, AUTO = _capi.PARSE_FIXED, _capi.PARSE_GENERAL, _capi.PARSE_AUTO
SHAPE_NAMES = {FIXED: "FIXED", GENERAL: "GENERAL", AUTO: "AUTO"}
PHASED, HALF_CALL, DECLINED = _capi.PARSE_PHASED, _capi.PARSE_HALF_CALL, _capi.PARSE_DECLINED
LEVELS = {"N_MID": N_MID, "N_S32": N_S32, "N_MAX": N_MAX}


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def framed(nbytes: int, align: int = 1):
    return LR.framed(nbytes, DEV, align)


def flag_frame(v: int):
    """-> (framed buffer, front, the v flag words inside it as int32, prefilled with sentinel bytes like the frame)."""
    buf, front = framed(4 * v, align=4)
    return buf, front, buf[front: front + 4 * v].view(torch.int32)


def num_cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def parse_call(eng, text, fo, le, out, front, stride, flags, shape, what, text_len=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.parse_gt(text, fo, le, out=out, out_stride=stride, out_offset=front, shape=shape, text_len=text_len, line_flags=flags)
    eng.wait()
    print(f"{what} {SHAPE_NAMES[shape]}: the call took {time.perf_counter() - t0:.2f} s")


def masked(rec: torch.Tensor, n: int) -> torch.Tensor:
    """A copy of one record with the pad bits of its last byte cleared."""
    want = rec.clone()
    if n % 4:
        want[-1] &= (1 << (2 * (n % 4))) - 1
    return want


def emit_text(eng, recs: Records, lead: int = 1):
    """The records' fixed-width text, written by decode_emit with row 0 at byte ``lead`` (an odd address) and held against the
    records by plain torch.  -> (buffer, field_off, line_end) with the offsets as Python lists."""
    n, v = recs.n, recs.v
    row = 4 * n + 1
    text = torch.empty(lead + v * row + 16, dtype=torch.uint8, device=DEV)
    eng.decode_emit(recs.buf, v, record_stride=recs.stride, records_offset=1, out=text, out_stride=row, out_offset=lead)
    eng.wait()
    for j in range(v):
        bad = LR.check_gt_row(text[lead + j * row: lead + (j + 1) * row], recs.rec(j), n)
        assert bad is None, f"the emitted text of row {j} is not the record's: {bad}"
    fo = [lead + j * row for j in range(v)]
    return text, fo, [x + 4 * n for x in fo]


def dev64(a) -> torch.Tensor:
    return torch.tensor([int(x) for x in a], dtype=torch.int64, device=DEV)


# ---- a, b. FIXED items on both sides of 2^32; AUTO's declined rounds at the natural grid ------------------------------------------
N_POOL, R_POOL = 4097, 1025        # P = 1025 is odd: both j and b matter
LINES_BELOW = 4_190_208            # total = 4 294 963 200 = 2^32 - 4096
LINES_EDGE = 4_190_211             # total = 2^32 - 1021: the largest launch of the 32-bit decomposition at this R
LINES_ABOVE = 4_190_213            # total = 4 294 968 325 > 2^32: the 64-bit decomposition
POOL_FIXED, POOL_VAR = 64, 4
POOL_PHASED = (3, 17, 40, 63)


class Pool:
    """64 distinct fixed-width text lines (decode_emit of random records; four of them phased afterwards) and 4 variable-width
    lines drawn from parse_ref.FORMS, in one text buffer of about 1 MiB.  Entry p: its text region, its record and flag word (from
    the source record; from parse_ref for the variable-width lines), and whether FIXED takes it."""

    def __init__(self, eng):
        n = N_POOL
        self.recs = Records(n, POOL_FIXED, 101)
        text, fo, le = emit_text(eng, self.recs)
        for p in POOL_PHASED:
            row = text[fo[p]: le[p]]
            row[row == ord("/")] = ord("|")
        rng = np.random.default_rng(102)
        regions = form_lines(rng, n, POOL_VAR)
        assert not any(parse_ref.fixed_takes(r, n) for r in regions)
        var_text, vfo, vle = lay_out(regions)
        base = text.numel()
        self.text = torch.cat([text, torch.from_numpy(np.frombuffer(var_text + bytes(16), dtype=np.uint8).copy()).to(DEV)])
        self.fo = dev64(fo + [base + int(x) for x in vfo])
        self.le = dev64(le + [base + int(x) for x in vle])
        vrecs, vflags = parse_ref.parse_lines(var_text, vfo, vle, n)
        assert all(int(f) & ~DECLINED for f in vflags)   # every variable-width line says something: DECLINED alone differs
        self.records = torch.cat([torch.stack([masked(self.recs.rec(p), n) for p in range(POOL_FIXED)]), torch.from_numpy(vrecs).to(DEV)])
        self.flags = torch.tensor([PHASED if p in POOL_PHASED else 0 for p in range(POOL_FIXED)] + [int(f) for f in vflags],
                                  dtype=torch.int32, device=DEV)
        # what forced FIXED leaves: DECLINED alone, and the row's bytes as they were
        self.records_fixed = self.records.clone()
        self.records_fixed[POOL_FIXED:] = SENT
        self.flags_fixed = self.flags.clone()
        self.flags_fixed[POOL_FIXED:] = DECLINED


def check_pool_launch(pool: Pool, line_map: torch.Tensor, out, front, stride, fbuf, ffront, flags, fixed: bool, what: str, slab=1 << 18):
    """Rows and flag words of a launch whose line j is pool entry line_map[j]: the expected rows are gathered from the pool's records
    by the same map, a slab of rows at a time."""
    v = line_map.numel()
    total = (v - 1) * stride + R_POOL
    assert frame_ok(out, front, total), f"{what}: bytes outside the output were written"
    assert frame_ok(fbuf, ffront, 4 * v), f"{what}: words outside the flag words were written"
    body = out[front: front + total]
    assert padding_untouched(body, v, R_POOL, stride, SENT), f"{what}: the padding column was written"
    want_flags = (pool.flags_fixed if fixed else pool.flags)[line_map]
    if not torch.equal(flags, want_flags):
        j = int(torch.nonzero(flags != want_flags)[0, 0])
        raise AssertionError(f"{what}: flag word of line {j} ({j:#x}, pool entry {int(line_map[j])}) is {int(flags[j]):#x}, want {int(want_flags[j]):#x}")
    records = pool.records_fixed if fixed else pool.records
    for a in range(0, v, slab):
        b = min(v, a + slab)
        got = body[a * stride:].as_strided((b - a, R_POOL), (stride, 1))
        ne = got != records[line_map[a:b]]
        if bool(ne.any()):
            i = int(torch.nonzero(ne.reshape(-1))[0, 0])
            j, byte = a + i // R_POOL, i % R_POOL
            raise AssertionError(f"{what}: row {j} ({j:#x}, pool entry {int(line_map[j])}) differs first at byte {byte}: item {j * R_POOL + byte:#x}, "
                                 f"output byte {j * stride + byte:#x}")
        del got, ne


def run_pool(n_lines: int, declined: dict, shapes, what: str):
    """One launch of n_lines lines that alias the pool by a seeded random map (``declined``: line -> variable-width pool entry), out
    stride R + 1, through ``shapes``."""
    need_gib(9)
    stride = R_POOL + 1
    with pgen_rs_amd.GtEngine(N_POOL, device=0) as eng:
        assert eng.record_size == R_POOL
        pool = Pool(eng)
        g = torch.Generator(device=DEV)
        g.manual_seed(n_lines % 1000)
        line_map = torch.randint(0, POOL_FIXED, (n_lines,), dtype=torch.int64, device=DEV, generator=g)
        for j, p in declined.items():
            line_map[j] = POOL_FIXED + p
        fo, le = pool.fo[line_map], pool.le[line_map]
        total = (n_lines - 1) * stride + R_POOL
        assert (n_lines - 1) * stride > 1 << 32   # the last rows' offsets j * out_stride pass 2^32
        out, front = framed(total)
        fbuf, ffront, flags = flag_frame(n_lines)
        for k, shape in enumerate(shapes):
            if k:
                out.fill_(SENT)
                fbuf.fill_(SENT)
            parse_call(eng, pool.text, fo, le, out, front, stride, flags, shape, what)
            check_pool_launch(pool, line_map, out, front, stride, fbuf, ffront, flags, shape == FIXED, f"{what} {SHAPE_NAMES[shape]}")
        del out, fbuf, flags, line_map, fo, le, pool


@pytest.mark.parametrize("n_lines", [LINES_BELOW, LINES_EDGE, LINES_ABOVE])
def test_fixed_items_on_both_sides_of_2_32(n_lines):
    """gt_parse_fixed_kernel's two decompositions of an item into (line j, piece b): ``(uint32_t)idx / P`` while
    ``total <= 0xFFFFFFFF``, else ``idx / P`` and ``idx - j * P`` in 64 bits; ``field_off[j]``, ``fo + 16 * b``,
    ``a.out[j * a.out_stride + b]`` past 4 GiB and the flag word ``line_flags[j]``, under FIXED (validate pass, then write pass) and
    AUTO (one pass).  Every line aliases one of 64 distinct text lines by a seeded random map, so a wrong j gives another line's
    bytes and a wrong b another piece's.  4 190 208 lines: total = 2^32 - 4096; 4 190 211: total = 2^32 - 1021, the last launch of
    the 32-bit branch at this R, whose last turn ends at item 2^32 - 1 (kBlockPieces divides 2^32, so a turn's item index cannot pass
    2^32 while total does not: the lanes behind the last item are the ones at 2^32 - 1021 .. 2^32 - 1, which `live` masks);
    4 190 213: total = 2^32 + 1029, the 64-bit branch.  Needs 9 GiB."""
    pieces, total, grid = parse_plan.fixed_plan(R_POOL, n_lines, num_cus())
    assert pieces == R_POOL == parse_plan.pieces_per_line(R_POOL) and total == n_lines * R_POOL
    assert total == {LINES_BELOW: 4_294_963_200, LINES_EDGE: (1 << 32) - 1021, LINES_ABOVE: 4_294_968_325}[n_lines]
    assert (total <= 0xFFFFFFFF) == (n_lines != LINES_ABOVE)
    if n_lines == LINES_EDGE:   # the last turn's lanes run up to item 2^32 - 1, past total
        assert -(-total // parse_plan.BLOCK_PIECES) * parse_plan.BLOCK_PIECES == 1 << 32 and (n_lines + 1) * R_POOL > 0xFFFFFFFF
    assert grid == num_cus() * parse_plan.BLOCKS_PER_CU and total > grid * parse_plan.BLOCK_PIECES   # the cap: many turns per block
    run_pool(n_lines, {}, (FIXED, AUTO), f"pool launch, {n_lines} lines")


def test_declined_rounds_at_the_natural_grid():
    """gt_parse_general_kernel under AUTO (``declined_only``) at the natural grid: the picks ``jt = blockIdx.x + (k0 + tid) * gridDim.x``,
    the ``continue`` past a round in which none of a block's lines was declined, and the rounds behind such a round.  The launch is
    the 4 190 213-line one above; four variable-width pool lines sit on line 0, on the last line, on a run inside round 3 and on a
    few scattered lines of round 5 (one of them in block 0, behind that block's four empty rounds); every other round holds no
    declined line.  Forced FIXED on the same input: those lines carry DECLINED alone and their rows keep the sentinel.  Needs 9 GiB."""
    n_lines = LINES_ABOVE
    grid = parse_plan.general_grid(n_lines, num_cus())
    round_lines = grid * parse_plan.THREADS
    rounds = -(-n_lines // round_lines)
    assert grid == num_cus() * parse_plan.BLOCKS_PER_CU and rounds >= 6
    declined = {0: 0, n_lines - 1: 1}
    for i in range(300):                                   # a run wholly inside round 3: 300 blocks, a line each
        declined[3 * round_lines + 1000 + i] = 2 + i % 2
    for i, at in enumerate((0, 1, grid - 1, grid, 77 * grid + 5, round_lines - 1)):   # round 5; its first line is block 0's
        declined[5 * round_lines + at] = (1 + i) % POOL_VAR
    in_round = sorted({j // round_lines for j in declined})
    assert in_round == [0, 3, 5, rounds - 1] and (5 * round_lines) % grid == 0
    assert [r for r in range(rounds) if r not in in_round] == [1, 2, 4, *range(6, rounds - 1)]   # the empty rounds
    run_pool(n_lines, declined, (AUTO, FIXED), "declined rounds")


def test_declined_rounds_cheap_twin():
    """The same ``continue`` with two blocks: 3 000 lines of N = 37 under KNOB_PARSE_BLOCKS = 2 are six rounds of 512 lines; declined
    lines (variable-width, of both blocks) sit in rounds 0, 3 and 5 only.  Held against parse_ref.parse_lines."""
    n, v = 37, 3000
    round_lines = parse_plan.general_grid(v, num_cus(), 2) * parse_plan.THREADS
    assert round_lines == 512 and -(-v // round_lines) == 6
    rng = np.random.default_rng(31)
    regions = form_lines(rng, n, v, fixed_share=1.0)
    var = form_lines(rng, n, 9)
    assert not any(parse_ref.fixed_takes(r, n) for r in var)
    at = [0, 1, 300, 3 * 512 + 4, 3 * 512 + 5, 3 * 512 + 511, 5 * 512, 5 * 512 + 201, v - 1]
    assert sorted({j // round_lines for j in at}) == [0, 3, 5] and {j % 2 for j in at} == {0, 1}
    for j, r in zip(at, var):
        regions[j] = r
    text, fo, le = lay_out(regions)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_PARSE_BLOCKS, 2)
        _, _, flags = check_against_ref(eng, text, fo, le, lead=1, out_lead=1)
        assert not (flags & DECLINED).any()


# ---- c. rows past 4 GiB by stride ------------------------------------------------------------------------------------------------------
def test_rows_past_4gib_by_stride():
    """``a.out[j * a.out_stride + b]`` (FIXED) and ``a.out + j * a.out_stride`` (GENERAL) with out_stride = 2^27 + 3: row 32 of 40
    begins past 2^32.  N = 13; fixed-width lines and one variable-width line at row 39, which forced FIXED declines.  Rows and flag
    words are parse_ref's; every byte between the rows holds the sentinel.  Needs 8 GiB."""
    need_gib(8)
    n, v, stride = 13, 40, (1 << 27) + 3
    assert 31 * stride < 1 << 32 < 32 * stride
    recs = oracle.synth_records(n, v)
    lines = oracle.decode_emit(recs, v, n).tobytes().split(b"\n")[:v]
    rng = np.random.default_rng(33)
    lines[39] = form_lines(rng, n, 1)[0]
    assert all(parse_ref.fixed_takes(r, n) for r in lines[:39]) and not parse_ref.fixed_takes(lines[39], n)
    text, fo, le = lay_out(lines)
    want, want_flags = parse_ref.parse_lines(text, fo, le, n)
    assert int(want_flags[39]) & ~DECLINED
    d_text = torch.from_numpy(np.frombuffer(text + bytes(16), dtype=np.uint8).copy()).to(DEV)
    d_want = torch.from_numpy(want).to(DEV)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        r = eng.record_size
        total = (v - 1) * stride + r
        out, front = framed(total)
        fbuf, ffront, flags = flag_frame(v)
        for k, shape in enumerate((FIXED, GENERAL, AUTO)):
            what = f"stride 2^27 + 3 {SHAPE_NAMES[shape]}"
            if k:
                out.fill_(SENT)
                fbuf.fill_(SENT)
            parse_call(eng, d_text, dev64(fo), dev64(le), out, front, stride, flags, shape, "stride 2^27 + 3", text_len=len(text))
            assert frame_ok(out, front, total) and frame_ok(fbuf, ffront, 4 * v), f"{what}: bytes outside the output or the flag words were written"
            body = out[front: front + total]
            assert padding_untouched(body, v, r, stride, SENT, slab_rows=8), f"{what}: bytes between the rows were written"
            got = body.as_strided((v, r), (stride, 1))
            fl = [int(f) for f in want_flags]
            if shape == FIXED:
                fl[39] = DECLINED
                assert torch.equal(got[:39], d_want[:39]) and bool((got[39] == SENT).all()), what
            else:
                assert torch.equal(got, d_want), f"{what}: rows {torch.nonzero((got != d_want).any(dim=1)).reshape(-1).tolist()} differ"
            assert flags.tolist() == fl, what
        del out, body, got


# ---- d. a line across byte 2^32 ---------------------------------------------------------------------------------------------------------
N_CROSS = 1 << 20
WIDE_FIELD = b"\t0/1:" + b"0123456789" * 300


@pytest.mark.parametrize("variable", [False, True], ids=["fixed_width", "variable_width"])
def test_a_line_across_byte_2_32(variable):
    """Three lines of N = 2^20 (4 MiB each) in a text buffer that is otherwise never initialised: line 0 wholly below byte 2^32, line 2
    wholly above, line 1 with ``field_off < 2^32 < line_end`` at each of the four phases of field_off mod 4.  Holds GENERAL's signed
    chunk arithmetic (``start``, ``c0``, ``q`` and the loads at ``text + q``) and FIXED's ``le - fo == 4 * N`` and ``fo + 16 * b``
    across 2^32.  fixed_width: decode_emit's text, the records are the source records.  variable_width: one mid-line field of line 1
    is `0/1:` + 3 000 digits and straddles byte 2^32, so the GENERAL pass owns the crossing (under AUTO too) and the chunks at the
    crossing hold no tab; line 1 is then parse_ref's on the host, and forced FIXED declines it.  Needs 6 GiB."""
    need_gib(6)
    n = N_CROSS
    recs = Records(n, 3, 41)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        r = eng.record_size
        small, sfo, sle = emit_text(eng, recs)
        rows = [small[a:b] for a, b in zip(sfo, sle)]
        want = [masked(recs.rec(j), n) for j in range(3)]
        want_flags, fixed_flags = [0, 0, 0], [0, 0, 0]
        field = (1 << 19) - 100                      # line 1's field that begins 400 bytes in front of byte 2^32 (+ phase)
        if variable:
            host = rows[1].cpu().numpy().tobytes()
            host = host[:4 * field] + WIDE_FIELD + host[4 * field + 4:]
            assert len(WIDE_FIELD) > 2 * parse_plan.CHUNK_BYTES + 400   # whole chunks without a tab behind byte 2^32
            rows[1] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(DEV)
            t0 = time.perf_counter()
            rec1, fl1 = parse_ref.parse_lines(host, [0], [len(host)], n)
            print(f"a line across 2^32: parse_ref on {len(host)} bytes took {time.perf_counter() - t0:.2f} s")
            assert int(fl1[0]) == 0 and not parse_ref.fixed_takes(host, n)
            want[1] = torch.from_numpy(rec1[0]).to(DEV)
            fixed_flags[1] = DECLINED
        len1 = rows[1].numel()
        big = torch.empty((1 << 32) + (1 << 23) + 4 * n + 64, dtype=torch.uint8, device=DEV)
        stride = r + 1
        total = 2 * stride + r
        out, front = framed(total)
        fbuf, ffront, flags = flag_frame(3)
        for phase in range(4):
            assert big.data_ptr() % 4 == 0
            fo = [5 + phase, (1 << 32) - (1 << 21) + phase, (1 << 32) + (1 << 23) + 7 - phase]
            le = [fo[0] + 4 * n, fo[1] + len1, fo[2] + 4 * n]
            assert fo[1] % 4 == phase and le[0] < fo[1] < 1 << 32 < le[1] < fo[2] and le[2] <= big.numel()
            if variable:   # the widened field straddles byte 2^32
                assert fo[1] + 4 * field < 1 << 32 < fo[1] + 4 * field + len(WIDE_FIELD) - 2 * parse_plan.CHUNK_BYTES
            for j in range(3):
                big[fo[j]: le[j]] = rows[j]
            for shape in (FIXED, GENERAL, AUTO):
                what = f"a line across 2^32, phase {phase}, {SHAPE_NAMES[shape]}"
                out.fill_(SENT)
                fbuf.fill_(SENT)
                parse_call(eng, big, dev64(fo), dev64(le), out, front, stride, flags, shape, f"a line across 2^32, phase {phase},")
                assert frame_ok(out, front, total) and frame_ok(fbuf, ffront, 12), f"{what}: bytes outside the output or the flag words were written"
                body = out[front: front + total]
                assert padding_untouched(body, 3, r, stride, SENT), f"{what}: the padding column was written"
                assert flags.tolist() == (fixed_flags if shape == FIXED else want_flags), what
                for j in range(3):
                    got = body[j * stride: j * stride + r]
                    if shape == FIXED and fixed_flags[j]:
                        assert bool((got == SENT).all()), f"{what}: the declined row was written"
                        continue
                    ne = got != want[j]
                    assert not bool(ne.any()), f"{what}: line {j} differs first at record byte {int(torch.nonzero(ne)[0, 0]):#x}"
        del big, out, small, rows


# ---- e. long rows ----------------------------------------------------------------------------------------------------------------------
def set_last_field(text: torch.Tensor, le: int, field: bytes):
    text[le - 4: le] = torch.tensor(list(field), dtype=torch.uint8, device=DEV)


def with_last_code(rec: torch.Tensor, n: int, code: int) -> torch.Tensor:
    want = rec.clone()
    sh = 2 * ((n - 1) % 4)
    want[-1] = (int(want[-1]) & ~(3 << sh)) | (code << sh)
    return want


def check_long(eng, text, fo, le, n, shape, want, want_flags, what):
    """One call on two long lines; ``want[j]`` None: the row must keep the sentinel."""
    r = eng.record_size
    stride = r + 1
    total = stride + r
    out, front = framed(total)
    fbuf, ffront, flags = flag_frame(2)
    parse_call(eng, text, dev64(fo), dev64(le), out, front, stride, flags, shape, what)
    what = f"{what} {SHAPE_NAMES[shape]}"
    assert frame_ok(out, front, total) and frame_ok(fbuf, ffront, 8), f"{what}: bytes outside the output or the flag words were written"
    assert int(out[front + r]) == SENT, f"{what}: the padding byte was written"
    assert flags.tolist() == want_flags, f"{what}: flags {flags.tolist()}, want {want_flags}"
    for j in range(2):
        got = out[front + j * stride: front + j * stride + r]
        if want[j] is None:
            assert bool((got == SENT).all()), f"{what}: the declined row {j} was written"
            continue
        ne = got != want[j]
        if bool(ne.any()):
            b = int(torch.nonzero(ne)[0, 0])
            raise AssertionError(f"{what}: row {j} differs first at record byte {b} ({b:#x}; text byte {16 * b:#x} of the line): got {int(got[b]):#x}, "
                                 f"want {int(want[j][b]):#x}")
        del ne
    del out


@pytest.mark.parametrize("level", ["N_S32", "N_MAX"])
def test_long_rows_fixed_and_auto(level):
    """FIXED and AUTO on two lines of N_S32 (4 N > 2^32: ``le - fo == 4ull * N``, ``fo + 16ull * b``) and N_MAX samples (R = 2^29),
    row 0 at an odd text address.  The text is decode_emit's, held against the records by longrow_ref.check_gt_row.  Then line 1's
    `/` become `|` on the device: PHASED on that line alone.  Then line 0's last field becomes `\\t./1`: HALF_CALL there, and the
    last sample's code is 3; N mod 4 = 3 at both levels, so that field lies in the partial piece of ``load_partial_piece``.  Then,
    FIXED only, line 0's last field becomes `\\t0/2`: DECLINED alone on line 0, its row untouched, line 1 exact.  Needs
    8 N bytes + 6 GiB (22 GiB at N_MAX)."""
    n = LEVELS[level]
    need_gib(8 * n / GIB + 6)
    assert n % 4 == 3 and 4 * n > 1 << 32
    recs = Records(n, 2, 51 + n % 7)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        text, fo, le = emit_text(eng, recs)
        assert fo[0] % 2 == 1
        assert parse_plan.fixed_plan(eng.record_size, 2, num_cus())[1] == 2 * eng.record_size
        want = [masked(recs.rec(j), n) for j in range(2)]
        for shape in (FIXED, AUTO):
            check_long(eng, text, fo, le, n, shape, want, [0, 0], f"{level} as emitted")
        for a in range(fo[1] + 2, le[1], 1 << 30):   # every field's separator, a slab at a time
            text[a: min(le[1], a + (1 << 30)): 4] = ord("|")
        for shape in (FIXED, AUTO):
            check_long(eng, text, fo, le, n, shape, want, [0, PHASED], f"{level} line 1 phased")
        set_last_field(text, le[0], b"\t./1")
        assert parse_ref.parse_region(b"\t./1", 1) == ([3], HALF_CALL)
        want3 = [with_last_code(want[0], n, 3), want[1]]
        for shape in (FIXED, AUTO):
            check_long(eng, text, fo, le, n, shape, want3, [HALF_CALL, PHASED], f"{level} last field ./1")
        set_last_field(text, le[0], b"\t0/2")
        assert not parse_ref.fixed_takes(b"\t0/2", 1)
        check_long(eng, text, fo, le, n, FIXED, [None, want[1]], [DECLINED, PHASED], f"{level} last field 0/2")
    del text, recs, want, want3


def test_long_row_general_n_mid():
    """GENERAL, and AUTO with a declined line, on two lines of N_MID samples (64 MiB of text each; one block walks one line at about
    0.2 GB/s, so the 4 - 8 GiB lines above would take tens of seconds): ``n_fields``, ``w0`` and ``out[(w0 >> 2) + tid]`` over 65 537
    chunks.  Line 0 is decode_emit's text with field N - 6 widened to `\\t1|1:7` (the line is 4 N + 2 bytes: FIXED declines it);
    that field's code and flag are parse_ref.parse_region's on its seven bytes, the rest of the record is the source record.  Line 1
    stays fixed-width.  PHASED alone is set, on line 0 alone.  Needs 1 GiB."""
    n = N_MID
    need_gib(1)
    recs = Records(n, 2, 57)
    wide = b"\t1|1:7"
    f = n - 6
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        small, sfo, sle = emit_text(eng, recs)
        assert parse_plan.general_chunks(4 * n + 2, 3) > 65536
        text = torch.empty(small.numel() + 16, dtype=torch.uint8, device=DEV)
        cut = sfo[0] + 4 * f
        text[:cut] = small[:cut]
        text[cut: cut + len(wide)] = torch.tensor(list(wide), dtype=torch.uint8, device=DEV)
        text[cut + len(wide): small.numel() + 2] = small[cut + 4:]
        fo, le = [sfo[0], sfo[1] + 2], [sle[0] + 2, sle[1] + 2]
        (code,), flag = parse_ref.parse_region(wide, 1)
        assert (code, flag) == (2, PHASED)
        want0 = masked(recs.rec(0), n)
        sh = 2 * (f % 4)
        want0[f >> 2] = (int(want0[f >> 2]) & ~(3 << sh)) | (code << sh)
        want = [want0, masked(recs.rec(1), n)]
        for shape in (GENERAL, AUTO):
            check_long(eng, text, fo, le, n, shape, want, [PHASED, 0], "N_MID, one widened field")
        check_long(eng, text, fo, le, n, FIXED, [None, want[1]], [DECLINED, 0], "N_MID, one widened field")
    del text, small, recs


# ---- f. fields far beyond N; a long tabless stretch ---------------------------------------------------------------------------------------
def test_fields_far_beyond_n():
    """GENERAL with N = 3 and 300 000 fields in a line: ``n_fields`` runs on in 64 bits over 1 172 chunks while the window arithmetic
    (``avail``, ``carry``, ``w0``) is 32-bit and stands still at N; FIELD_COUNT, the three codes right, nothing written beyond R.  A
    line of exactly three fields stands beside it.  Held against parse_ref at KNOB_PARSE_BLOCKS 0 and 1."""
    n = 3
    long_line = b"\t0/1\t1/1\t./." + b"\t1/1\t0|1" * 149_998 + b"\t1/1"
    assert long_line.count(b"\t") == 300_000 and parse_plan.general_chunks(len(long_line), 3) > 1000
    text, fo, le = lay_out([b"\t1/1\t0/0\t0/1", long_line, b"\t0/0\t1/1\t1/0"])
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for blocks in (0, 1):
            eng.tune(_capi.KNOB_PARSE_BLOCKS, blocks)
            _, recs, flags = check_against_ref(eng, text, fo, le, lead=1, out_lead=1)
            assert [int(x) for x in flags] == [0, _capi.PARSE_FIELD_COUNT, 0] and recs[1].tolist() == [1 | 2 << 2 | 3 << 4]


def test_a_suffix_of_five_tabless_chunks():
    """GENERAL with N = 260 and one field whose `:`-suffix is 5 * CHUNK_BYTES + 1 bytes: chunks whose block scan counts no tab
    (``chunk_tabs`` = 0, ``avail`` unchanged, the carried codes kept in place), started at every dword phase by a leading field of
    0 .. 3 bytes and by the text's own alignment.  Held against parse_ref at KNOB_PARSE_BLOCKS 0 and 1."""
    n = 260
    rng = np.random.default_rng(61)
    tails = form_lines(rng, n - 2, 4)
    suffix = b"\t0/1:" + b"7" * (5 * parse_plan.CHUNK_BYTES + 1)
    assert len(suffix.split(b":", 1)[1]) == 5 * parse_plan.CHUNK_BYTES + 1
    regions = [b"\t" + lead + suffix + tails[k] for k, lead in enumerate((b"", b"1", b"0/", b"0|1"))]
    text, fo, le = lay_out(regions)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for blocks in (0, 1):
            eng.tune(_capi.KNOB_PARSE_BLOCKS, blocks)
            for lead in range(4):
                check_against_ref(eng, text, fo, le, lead=lead, out_lead=lead)
