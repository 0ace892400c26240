"""The far end of the ABI's index ranges on the device: rows of up to 2^31 - 1 samples (include/pgen_hip.h accepts that many) through
every entry point, byte-exact against the slab-wise torch reference of longrow_ref.py (held against the CPU oracle by
test_longrow_ref.py).  Row positions are 64-bit in every kernel and everything inside a row is 32-bit on purpose; the levels below
are where those 32-bit quantities pass 2^31 and 2^32.

Every output is framed by sentinel bytes (at least 67 in front — rounded up to the alignment the entry point demands — and 64
behind) and, where the kernel allows one, has a padded pitch; the frame and the padding must come back untouched.  Row 0 of the
records sits at byte 1 of its buffer and the stride is R + 1, so the rows have different alignments.  Records are random bytes
(dirty pad bits included), made on the device.  A case is skipped only when the card has less free memory than the case states.

What AUTO runs at these shapes (capi.hip): all samples, GT segments at the dense pitch and full lines: the stream kernel (WIDE);
at a padded pitch: the general kernel (ROWS).  Kept lists: K = 4 099 of 2^31 - 1 is `very_sparse`: ROWS; every 22nd sample is the
two passes' widest record (segment compact pass, then WIDE on one 24.4-MB compact record per chunk); every other sample, and half
of N_MID as full lines: the segment kernel (SCAN), in rounds.  Counts: a wave per row.  Matrix: STREAM / TILE / GENERAL by
orientation and list.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import longrow_ref as LR
import pgen_rs_amd
import subset_plan as SP
from pgen_rs_amd import _capi
from pgen_rs_amd._capi import check, lib

pytestmark = pytest.mark.gpu

from longrow_ref import GIB, SENT, frame_ok, need_gib

DEV = "cuda:0"

# ---- the levels ------------------------------------------------------------------------------------------------------------------
N_MID = (1 << 24) + 1        # above every N the all-samples, count and matrix kernels have seen; 1 025 segments (more than a resident
                             # round of the segment kernel); cheap: R = 4 MiB
N_LINE_MAX = (1 << 29) - 8   # 4K + 1 = 2^31 - 31: with prefixes of at most 30 bytes the longest line pgenhip_emit_lines accepts
N_S31 = (1 << 29) + 3        # 4K + 1 > 2^31: a signed row-relative byte offset wraps
N_S32 = (1 << 30) + 3        # 4K + 1 > 2^32; an f32 matrix row > 2^32 bytes; the per-sample count word index 4k + c > 2^32
N_MAX = (1 << 31) - 1        # the ABI's limit; R = 2^29, and the bit position 2s passes 2^32
N_HALF = (1 << 30) + 6       # every other sample kept: K = 2^29 + 3, so a kept row's text passes 2^31 bytes
LEVELS = {"N_MID": N_MID, "N_LINE_MAX": N_LINE_MAX, "N_S31": N_S31, "N_S32": N_S32, "N_MAX": N_MAX}
BIG = ["N_LINE_MAX", "N_S31", "N_S32", "N_MAX"]

K_AUTO, K_ROWS, K_FLAT, K_WIDE, K_SCAN = _capi.KERNEL_AUTO, _capi.KERNEL_ROWS, _capi.KERNEL_FLAT, _capi.KERNEL_WIDE, _capi.KERNEL_SCAN
KNAMES = {"auto": K_AUTO, "rows": K_ROWS, "flat": K_FLAT, "wide": K_WIDE, "scan": K_SCAN}


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


# ---- records, kept lists, frames ------------------------------------------------------------------------------------------------
class Records:
    """V random records: row j at byte 1 + j * (R + 1) of ``buf`` (row 0 at an odd address, every row at another alignment)."""

    def __init__(self, n: int, v: int, seed: int):
        self.n, self.v, self.r = n, v, LR.rsize(n)
        self.stride = self.r + 1
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        self.buf = torch.randint(0, 256, (1 + v * self.stride + 15,), dtype=torch.uint8, device=DEV, generator=g)

    def off(self, j: int) -> int:
        return 1 + j * self.stride

    def rec(self, j: int) -> torch.Tensor:
        return self.buf[self.off(j): self.off(j) + self.r]


SOURCES = ("stride", "gather", "at")


def select(recs: Records, source: str):
    """-> (the rows in output order, kwargs of the engine's stride / gather methods or None, (base, offsets) of the _at methods or None).
    "gather" names a row twice; "at" takes the rows in reverse order."""
    v = recs.v
    if source == "stride":
        return list(range(v)), dict(records=recs.buf, record_stride=recs.stride, records_offset=1), None
    if source == "gather":
        assert v >= 5
        order = [v - 1, 1, 1, 0, v // 2]
        vidx = torch.tensor(order, dtype=torch.int32, device=DEV)
        return order, dict(records=recs.buf, record_stride=recs.stride, records_offset=1, variant_idx=vidx), None
    order = list(range(v))[::-1]
    offs = torch.tensor([recs.off(j) for j in order], dtype=torch.int64, device=DEV)
    return order, None, (recs.buf, offs)


@functools.lru_cache(maxsize=4)
def kept_sparse(n: int) -> np.ndarray:
    """4 099 samples spread over the whole range, samples 0 and N - 1 among them."""
    kept = np.unique(np.linspace(0, n - 1, 4099).astype(np.int64)).astype(np.uint32)
    assert kept.size == 4099 and kept[0] == 0 and kept[-1] == n - 1
    return kept


@functools.lru_cache(maxsize=2)
def kept_every22(n: int) -> np.ndarray:
    """Every 22nd sample from sample 5: K = floor(N / 22) at N_MAX, the largest K that ``two_pass_shape`` admits."""
    return np.arange(5, n, 22, dtype=np.uint32)


def kept_of(n: int, keep: str):
    return None if keep == "all" else kept_sparse(n) if keep == "sparse" else kept_every22(n)


def framed(nbytes: int, align: int = 1):
    return LR.framed(nbytes, DEV, align)


def all_sentinel(buf: torch.Tensor) -> bool:
    return bool((buf == SENT).all())


def status_of(fn, *args, **kw) -> int:
    try:
        fn(*args, **kw)
    except pgen_rs_amd.PgenHipError as e:
        return e.status
    return _capi.OK


# ---- a. GT segments ---------------------------------------------------------------------------------------------------------------
def emit(eng, recs: Records, source: str, buf: torch.Tensor, front: int, pitch: int, kernel: int):
    order, kw, at = select(recs, source)
    if at is None:
        eng.decode_emit(n_variants=len(order), out=buf, out_offset=front, out_stride=pitch, kernel=kernel, **kw)
    else:
        eng.decode_emit_at(at[0], at[1], len(order), out=buf[front:], out_stride=pitch, kernel=kernel)
    eng.wait()
    return order


def check_segments(buf, front, pitch, order, recs: Records, n, kept, what):
    k = LR.kept_count(n, kept)
    row = 4 * k + 1
    total = (len(order) - 1) * pitch + row
    assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
    out = buf[front: front + total]
    assert LR.padding_untouched(out, len(order), row, pitch, SENT), f"{what}: padding between rows was written"
    d_kept = LR.as_kept(kept, DEV)
    for j, src in enumerate(order):
        bad = LR.check_gt_row(out[j * pitch: j * pitch + row], recs.rec(src), n, d_kept)
        assert bad is None, (f"{what}: row {j} (record {src}) differs first at rank {bad[0]}, byte {bad[1]} = row byte {4 * bad[0] + bad[1]} "
                             f"({4 * bad[0] + bad[1]:#x}): got {bad[2]}, want {bad[3]}")


def run_segments(n, v, source, kernel, padded, keep="all", seed=1, tune=()):
    kept = kept_of(n, keep)
    recs = Records(n, v, seed)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for knob, value in tune:
            eng.tune(knob, value)
        row = eng.gt_row_bytes
        pitch = row + (13 if padded else 0)
        rows = len(select(recs, source)[0])
        buf, front = framed((rows - 1) * pitch + row)
        order = emit(eng, recs, source, buf, front, pitch, kernel)
        check_segments(buf, front, pitch, order, recs, n, kept, f"N={n} {keep} {source} kernel {kernel} pitch +{pitch - row}")
    del buf, recs


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("source", SOURCES)
def test_gt_segments_all_samples_n_mid(source, padded):
    """N_MID, V = 5, every row source, AUTO and every forced kernel that takes the pitch.  Needs 1 GiB."""
    need_gib(1)
    for name in ("auto", "rows") + (() if padded else ("flat", "wide")):
        run_segments(N_MID, 5, source, KNAMES[name], padded)


SEG_BIG = [("auto", "stride", False), ("rows", "stride", False), ("rows", "stride", True), ("flat", "stride", False),
           ("wide", "stride", False), ("auto", "at", False)]


@pytest.mark.parametrize("kernel,source,padded", SEG_BIG, ids=[f"{k}-{s}-{'padded' if p else 'dense'}" for k, s, p in SEG_BIG])
@pytest.mark.parametrize("level", BIG)
def test_gt_segments_all_samples(level, kernel, source, padded):
    """V = 2 at the four long levels: AUTO (the stream kernel), ROWS (dense and padded), FLAT, WIDE, and AUTO through
    pgenhip_decode_emit_at with the rows swapped.  Needs 20 GiB at N_MAX (two rows of 8 GiB of text)."""
    n = LEVELS[level]
    need_gib(8 * n / GIB + 4)
    run_segments(n, 2, source, KNAMES[kernel], padded, seed=LEVELS[level] % 1000)


def test_short_record_kernels_refuse_n_max():
    """PICK (N <= 4 096), RUNS (N <= 3 831) and ROWPICK (needs a kept list) are PGENHIP_ERR_BAD_ARG at N_MAX and write nothing; the
    ctx then still runs AUTO exactly.  Needs 20 GiB."""
    n = N_MAX
    need_gib(8 * n / GIB + 4)
    recs = Records(n, 2, 77)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        row = eng.gt_row_bytes
        buf, front = framed(2 * row)
        for kern in (_capi.KERNEL_PICK, _capi.KERNEL_RUNS, _capi.KERNEL_ROWPICK):
            st = status_of(eng.decode_emit, recs.buf, 2, record_stride=recs.stride, records_offset=1, out=buf, out_offset=front,
                           out_stride=row, kernel=kern)
            assert st == _capi.ERR_BAD_ARG, f"kernel {kern}: status {st}"
            eng.wait()
        assert all_sentinel(buf), "a refused kernel wrote"
        order = emit(eng, recs, "stride", buf, front, row, K_AUTO)
        check_segments(buf, front, row, order, recs, n, None, "AUTO after the refusals")
    del buf, recs


# ---- b. full lines -----------------------------------------------------------------------------------------------------------------
class Lines:
    """Prefixes of the given lengths (random printable bytes), the offset arrays of pgenhip_emit_lines, a framed output."""

    def __init__(self, plens, row_bytes: int, seed: int):
        rng = np.random.default_rng(seed)
        self.plens = [int(p) for p in plens]
        self.poff = np.concatenate([[0], np.cumsum(self.plens)]).astype(np.int64)
        self.loff = np.concatenate([[0], np.cumsum(np.asarray(self.plens, dtype=np.int64) + row_bytes)]).astype(np.int64)
        blob = rng.integers(33, 127, size=max(int(self.poff[-1]), 1), dtype=np.uint8)
        self.blob = torch.from_numpy(blob).to(DEV)
        self.d_poff = torch.from_numpy(self.poff).to(DEV)
        self.d_loff = torch.from_numpy(self.loff).to(DEV)
        self.total = int(self.loff[-1])
        self.buf, self.front = framed(self.total)

    def out(self) -> torch.Tensor:
        return self.buf[self.front: self.front + self.total]


def check_lines(lines: Lines, order, recs: Records, n, kept, what):
    assert frame_ok(lines.buf, lines.front, lines.total), f"{what}: bytes outside the output were written"
    out = lines.out()
    d_kept = LR.as_kept(kept, DEV)
    row = 4 * LR.kept_count(n, kept) + 1
    for j, src in enumerate(order):
        lo, po, pl = int(lines.loff[j]), int(lines.poff[j]), lines.plens[j]
        assert torch.equal(out[lo: lo + pl], lines.blob[po: po + pl]), f"{what}: prefix of line {j} differs"
        bad = LR.check_gt_row(out[lo + pl: lo + pl + row], recs.rec(src), n, d_kept)
        assert bad is None, (f"{what}: line {j} (record {src}, prefix {pl}) differs first at rank {bad[0]}, byte {bad[1]} = GT byte "
                             f"{4 * bad[0] + bad[1]} ({4 * bad[0] + bad[1]:#x}): got {bad[2]}, want {bad[3]}")


def emit_lines(eng, recs: Records, source: str, lines: Lines, bound: int, kernel: int):
    order, kw, at = select(recs, source)
    assert at is None
    eng.emit_lines(kw["records"], len(order), lines.blob, lines.d_poff, lines.d_loff, bound, lines.out(), record_stride=kw["record_stride"],
                   variant_idx=kw.get("variant_idx"), kernel=kernel, records_offset=kw["records_offset"])
    eng.wait()
    return order


@pytest.mark.parametrize("kernel", ["auto", "rows", "wide"])
def test_longest_line(kernel):
    """N_LINE_MAX, all samples, V = 2, prefixes of 30 and 7 bytes under max_prefix_bytes = 30: lines of 2^31 - 1 and 2^31 - 24 bytes, the
    longest the entry point lets through.  Needs 8 GiB."""
    n = N_LINE_MAX
    need_gib(8)
    recs = Records(n, 2, 29)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        assert 30 + eng.gt_row_bytes == (1 << 31) - 1
        lines = Lines([30, 7], eng.gt_row_bytes, 5)
        order = emit_lines(eng, recs, "stride", lines, 30, KNAMES[kernel])
        check_lines(lines, order, recs, n, None, f"longest line, kernel {kernel}")
    del lines, recs


def test_line_bound_refused_then_exact():
    """The same launch under max_prefix_bytes = 31 is PGENHIP_ERR_TOO_LARGE and writes nothing; the next call on the ctx is exact.
    Needs 8 GiB."""
    n = N_LINE_MAX
    need_gib(8)
    recs = Records(n, 2, 31)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        lines = Lines([30, 7], eng.gt_row_bytes, 6)
        for kern in (K_AUTO, K_ROWS, K_WIDE):
            st = status_of(emit_lines, eng, recs, "stride", lines, 31, kern)
            assert st == _capi.ERR_TOO_LARGE, f"kernel {kern}: status {st}"
        eng.wait()
        assert all_sentinel(lines.buf), "a refused call wrote"
        order = emit_lines(eng, recs, "stride", lines, 30, K_AUTO)
        check_lines(lines, order, recs, n, None, "AUTO after the refusal")
    del lines, recs


@pytest.mark.parametrize("case", ["all-stride", "all-gather", "half-stride"])
def test_lines_n_mid(case):
    """N_MID, V = 5, prefixes of 0 .. 200 bytes (bound 200): all samples by stride (AUTO, ROWS, WIDE) and gathered (AUTO, WIDE), and
    AUTO and SCAN with half the samples kept (the segment kernel over 1 025 segments: rounds).  Needs 1 GiB."""
    n = N_MID
    need_gib(1)
    keep, source = case.split("-")
    kept = None
    if keep == "half":
        kept = np.flatnonzero(np.random.default_rng(50).random(n) < 0.5).astype(np.uint32)
        assert SP.arm(n, kept.size, 5, mode="lines").kernel == "scan" and SP.scan_plan(n, kept.size, 5).rounds
    recs = Records(n, 5, 41)
    rows = len(select(recs, source)[0])
    kernels = (K_AUTO, K_SCAN) if kept is not None else (K_AUTO, K_ROWS, K_WIDE) if source == "stride" else (K_AUTO, K_WIDE)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for kern in kernels:
            lines = Lines([0, 200, 1, 37, 128][:rows], eng.gt_row_bytes, 7)
            order = emit_lines(eng, recs, source, lines, 200, kern)
            check_lines(lines, order, recs, n, kept, f"{case}, kernel {kern}")
            del lines
    del recs


# ---- c. kept subsets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "scan", "rows"])
def test_sparse_keep_n_max(kernel):
    """N_MAX, K = 4 099 spread over the whole range with samples 0 and N - 1, V = 2: AUTO takes the general kernel (`very_sparse`);
    SCAN walks 131 072 segments, nearly all of them empty.  Dense and padded pitch, and _at with the rows swapped.  Needs 3 GiB."""
    n = N_MAX
    need_gib(3)
    assert SP.arm(n, 4099, 2).kernel == "rows"
    run_segments(n, 2, "stride", KNAMES[kernel], False, keep="sparse", seed=3)
    run_segments(n, 2, "at", KNAMES[kernel], True, keep="sparse", seed=4)


EVERY22 = ["auto", "scan", "rows", "auto-lines", "auto-single-pass"]


@pytest.mark.parametrize("case", EVERY22)
def test_every_22nd_sample_n_max(case):
    """N_MAX, every 22nd sample (K = floor(N / 22) = 97 612 893), V = 3: under AUTO three one-row chunks of the two passes, each a
    24.4-MB compact record in its 32-MiB slice; SCAN and ROWS forced; AUTO as full lines; AUTO with PGENHIP_KNOB_SCAN_TWO_PASS = -1 (the
    segment kernel in one pass).  Needs 6 GiB."""
    n = N_MAX
    need_gib(6)
    kept = kept_every22(n)
    k = int(kept.size)
    assert k == n // 22 and SP.two_pass_shape(n, k) and not SP.two_pass_shape(n, k + 1)
    msc = SP.max_seg_count(kept, n)
    for mode in ("segments", "lines"):
        plan = SP.arm(n, k, 3, mode=mode, msc=msc)
        assert plan.kernel == "two_pass" and plan.chunk_rows == 1 and [c[:2] for c in plan.chunks] == [(1, "scan")] * 3, plan
    assert SP.arm(n, k, 3, msc=msc, tune=SP.Tune(scan_two_pass=-1)).kernel == "scan"
    if case == "auto-lines":
        recs = Records(n, 3, 9)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            lines = Lines([30, 0, 17], eng.gt_row_bytes, 8)
            order = emit_lines(eng, recs, "stride", lines, 30, K_AUTO)
            check_lines(lines, order, recs, n, kept, "every 22nd, AUTO, full lines")
        del lines, recs
        return
    tune = ((_capi.KNOB_SCAN_TWO_PASS, -1),) if case == "auto-single-pass" else ()
    run_segments(n, 3, "stride", KNAMES[case.split("-")[0]], False, keep="every22", seed=10, tune=tune)


@pytest.mark.parametrize("kernel", ["auto", "scan", "rows"])
def test_every_other_sample(kernel):
    """N = 2^30 + 6, every other sample (K = 2^29 + 3), V = 1: the kept row's text is 2^31 + 13 bytes through the segment kernel (AUTO,
    SCAN) and the general kernel.  The kept list is 2 GiB on the host and on the device.  Needs 10 GiB."""
    n = N_HALF
    need_gib(10)
    kept = np.arange(0, n, 2, dtype=np.uint32)
    assert kept.size == (1 << 29) + 3
    recs = Records(n, 1, 12)
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        del kept
        row = eng.gt_row_bytes
        assert row > (1 << 31)
        buf, front = framed(row)
        order = emit(eng, recs, "stride", buf, front, row, KNAMES[kernel])
        check_segments(buf, front, row, order, recs, n, d_kept, f"every other sample, kernel {kernel}")
    del buf, recs, d_kept


# ---- d. per-variant counts ---------------------------------------------------------------------------------------------------------
COUNT_KERNELS = (_capi.COUNT_AUTO, _capi.COUNT_WAVE_PER_ROW, _capi.COUNT_ROWS_PER_WAVE)


def counts_call(eng, recs: Records, source: str, kernel: int):
    """-> (rows in output order, the 4 * rows counts as Python integers); the counts sit in a sentinel frame that must survive."""
    order, kw, at = select(recs, source)
    rows = len(order)
    buf, front = framed(16 * rows, align=4)
    out = buf[front: front + 16 * rows].view(torch.int32)
    if at is None:
        eng.genotype_counts(out=out, n_variants=rows, kernel=kernel, **kw)
    else:
        eng.genotype_counts_at(at[0], at[1], rows, out=out, kernel=kernel)
    eng.wait()
    assert frame_ok(buf, front, 16 * rows), f"counts kernel {kernel}: words outside the counts were written"
    return order, (out.to(torch.int64) & 0xFFFFFFFF).view(rows, 4).tolist()


@pytest.mark.parametrize("keep", ["all", "sparse", "every22"])
@pytest.mark.parametrize("level", ["N_MID", "N_S32", "N_MAX"])
def test_genotype_counts(level, keep):
    """pgenhip_genotype_counts at N_MID (V = 5, every row source), N_S32 and N_MAX (V = 2, stride and swapped _at): AUTO, a wave per row
    and several rows per wave, all samples and the two kept lists (their masks are record-shaped: 512 MiB at N_MAX).  Needs 4 GiB."""
    n = LEVELS[level]
    need_gib(4)
    kept = kept_of(n, keep)
    v = 5 if level == "N_MID" else 2
    recs = Records(n, v, 20 + len(keep))
    d_kept = LR.as_kept(kept, DEV)
    want = [LR.row_counts(recs.rec(j), n, d_kept) for j in range(v)]
    assert all(sum(w) == LR.kept_count(n, kept) for w in want)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for kern in COUNT_KERNELS:
            # (several rows per wave walks a 512-MiB row with 32 lanes: once is enough)
            for source in SOURCES if level == "N_MID" else ("stride", "at") if kern == _capi.COUNT_AUTO else ("stride",):
                order, got = counts_call(eng, recs, source, kern)
                assert got == [want[j] for j in order], f"{level} {keep} {source} kernel {kern}: got {got}, want {[want[j] for j in order]}"
    del recs, d_kept


def test_genotype_counts_all_missing_row_n_max():
    """A row of 0xFF bytes at N_MAX: missing = 2^31 - 1 (the pad bits of the last byte are set and not counted), beside a random row.
    Needs 2 GiB."""
    n = N_MAX
    need_gib(2)
    recs = Records(n, 2, 23)
    recs.rec(1).fill_(0xFF)
    want = [LR.row_counts(recs.rec(0), n), [0, 0, 0, n]]
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for kern in COUNT_KERNELS:
            order, got = counts_call(eng, recs, "stride", kern)
            assert got == want, f"kernel {kern}: got {got}, want {want}"
    del recs


# ---- e. per-sample counts ----------------------------------------------------------------------------------------------------------
PREFILL = 0xFFFFFFF0


def run_sample_counts(n, v, keep, sources, modes, seed, slab=LR.SLAB):
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    recs = Records(n, v, seed)
    d_kept = LR.as_kept(kept, DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for source in sources:
            order, kw, at = select(recs, source)
            rows = [recs.rec(j) for j in order]
            for kern, accumulate in modes:
                buf, front = framed(16 * k, align=4)
                out = buf[front: front + 16 * k].view(torch.int32)
                if accumulate:
                    out.fill_(PREFILL - (1 << 32))
                if at is None:
                    eng.sample_counts(out=out, n_variants=len(order), kernel=kern, accumulate=accumulate, **kw)
                else:
                    eng.sample_counts_at(at[0], at[1], len(order), out=out, kernel=kern, accumulate=accumulate)
                eng.wait()
                what = f"N={n} {keep} {source} kernel {kern} accumulate={accumulate}"
                assert frame_ok(buf, front, 16 * k), f"{what}: words outside the counts were written"
                bad = LR.check_sample_counts(out, rows, n, d_kept, PREFILL if accumulate else 0, slab=slab)
                assert bad is None, (f"{what}: rank {bad[0]} code {bad[1]} (count word {4 * bad[0] + bad[1]} = {4 * bad[0] + bad[1]:#x}): "
                                     f"got {bad[2]}, want {bad[3]}")
                del buf, out
    del recs, d_kept


SCOUNT_MODES = [(_capi.SCOUNT_AUTO, False), (_capi.SCOUNT_ROWS, False), (_capi.SCOUNT_AUTO, True), (_capi.SCOUNT_ROWS, True)]


@pytest.mark.parametrize("keep", ["all", "sparse", "every22"])
def test_sample_counts_n_mid(keep):
    """N_MID, V = 5, every row source (the gather counts a row twice), AUTO and ROWS, overwrite and ACCUMULATE onto 0xFFFFFFF0 (the
    sums wrap).  Needs 2 GiB."""
    need_gib(2)
    run_sample_counts(N_MID, 5, keep, SOURCES, SCOUNT_MODES, 60)


@pytest.mark.parametrize("source", ["stride", "at"])
@pytest.mark.parametrize("keep", ["all", "sparse", "every22"])
@pytest.mark.parametrize("level", ["N_S32", "N_MAX"])
def test_sample_counts(level, keep, source):
    """N_S32 and N_MAX, V = 2, by stride and through the swapped _at rows: AUTO and ROWS, overwrite and ACCUMULATE onto 0xFFFFFFF0.
    With all samples the counts are 16 B x N (32 GiB at N_MAX, count word indices past 2^32); the kept lists walk the mask and rank
    tables at 2^25 chunks.  Needs 48 GiB at N_MAX with all samples."""
    n = LEVELS[level]
    need_gib(1.5 * 16 * n / GIB if keep == "all" else 6)
    run_sample_counts(n, 2, keep, (source,), SCOUNT_MODES, 61, slab=1 << 25)


# ---- f. genotype matrix ---------------------------------------------------------------------------------------------------------------
SHAPES = {"general": _capi.MATRIX_GENERAL, "stream": _capi.MATRIX_STREAM, "tile": _capi.MATRIX_TILE, "auto": _capi.MATRIX_AUTO}
DTYPES = {"int8": torch.int8, "int16": torch.int16, "f32": torch.float32}


def run_matrix(n, v, keep, source, shape, dtype, sample_major, pad, seed=70):
    """One pgenhip_decode_matrix / _at call through the C ABI (the engine's wrapper wants a 2-D tensor; here the output is a framed byte
    buffer at a chosen pitch).  ``pad``: bytes added to the dense pitch."""
    kept = kept_of(n, keep)
    k = LR.kept_count(n, kept)
    recs = Records(n, v, seed)
    order, kw, at = select(recs, source)
    rows_sel = [recs.rec(j) for j in order]
    nv = len(order)
    pat = pgen_rs_amd.GtEngine.matrix_values(DTYPES[dtype])   # 0, 1, 2 and -1 / NaN: compared as bytes
    eb = pat.size // 4
    out_rows, inner = (k, nv) if sample_major else (nv, k)
    row_bytes = inner * eb
    pitch = row_bytes + pad
    tile_like = shape == "tile" or (shape == "auto" and sample_major)   # 16-byte-aligned rows: what TILE needs and AUTO looks for
    if tile_like:
        pitch = -(-pitch // 16) * 16
    total = (out_rows - 1) * pitch + row_bytes
    buf, front = framed(total, align=16 if tile_like else eb)
    flags = SHAPES[shape] | (_capi.MATRIX_SAMPLE_MAJOR if sample_major else 0)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        if at is None:
            vidx = kw.get("variant_idx")
            check(lib.pgenhip_decode_matrix(eng._ctx, recs.buf.data_ptr() + 1, recs.stride, None if vidx is None else vidx.data_ptr(), nv,
                                            buf.data_ptr() + front, pitch, eb, pat.ctypes.data_as(C.c_void_p), flags), "pgenhip_decode_matrix")
        else:
            check(lib.pgenhip_decode_matrix_at(eng._ctx, at[0].data_ptr(), at[1].data_ptr(), nv, buf.data_ptr() + front, pitch, eb,
                                               pat.ctypes.data_as(C.c_void_p), flags), "pgenhip_decode_matrix_at")
        eng.wait()
    what = f"N={n} V={nv} {keep} {source} {shape} {dtype} {'sample' if sample_major else 'variant'}-major pitch +{pitch - row_bytes}"
    assert frame_ok(buf, front, total), f"{what}: bytes outside the output were written"
    out = buf[front: front + total]
    assert LR.padding_untouched(out, out_rows, row_bytes, pitch, SENT), f"{what}: row padding was written"
    bad = LR.check_matrix(out, rows_sel, n, LR.as_kept(kept, DEV), eb, pat, sample_major, pitch)
    assert bad is None, (f"{what}: row {bad[0]}, rank {bad[1]}, byte {bad[2]} (element byte offset {bad[1] * eb:#x} in its row): "
                         f"got {bad[3]}, want {bad[4]}")
    del buf, out, recs


@pytest.mark.parametrize("sample_major", [False, True], ids=["variant_major", "sample_major"])
@pytest.mark.parametrize("dtype", ["int8", "f32"])
def test_matrix_general_n_mid(dtype, sample_major):
    """GENERAL at N_MID, V = 5, both orientations, every row source, a padded pitch.  Needs 2 GiB."""
    need_gib(2)
    for source in SOURCES:
        run_matrix(N_MID, 5, "all", source, "general", dtype, sample_major, 16 if source != "stride" else 0)


@pytest.mark.parametrize("case", ["all-variant_major", "all-sample_major", "every22-variant_major", "every22-sample_major"])
def test_matrix_general_n_max(case):
    """GENERAL int8 at N_MAX, V = 2 (2^32 - 2 elements: the last launch of its 32-bit index path), both orientations, all samples and the
    every-22nd list.  Needs 10 GiB."""
    need_gib(10)
    keep, orient = case.split("-")
    run_matrix(N_MAX, 2, keep, "stride" if orient == "variant_major" else "at", "general", "int8", orient == "sample_major", 0)


@pytest.mark.parametrize("dtype", ["int8", "int16", "f32"])
def test_matrix_stream_n_mid(dtype):
    """STREAM at N_MID, V = 5: dense pitch (one byte stream) by stride, pitch + 16 B gathered and through _at; AUTO takes it too.
    Needs 2 GiB."""
    need_gib(2)
    run_matrix(N_MID, 5, "all", "stride", "stream", dtype, False, 0)
    run_matrix(N_MID, 5, "all", "gather", "stream", dtype, False, 16)
    run_matrix(N_MID, 5, "all", "at", "auto", dtype, False, 16)


@pytest.mark.parametrize("pad", [0, 16], ids=["dense", "pitch+16"])
@pytest.mark.parametrize("level", ["N_S32", "N_MAX"])
def test_matrix_stream_f32(level, pad):
    """STREAM f32 at N_S32 and N_MAX, V = 2: output rows of more than 2^32 bytes.  Needs 24 GiB at N_MAX."""
    n = LEVELS[level]
    need_gib(2 * 4 * n / GIB + 8)
    run_matrix(n, 2, "all", "stride" if pad else "at", "stream", "f32", False, pad)


@pytest.mark.parametrize("v", [5, 129])
@pytest.mark.parametrize("dtype", ["int8", "f32"])
def test_matrix_tile_n_mid(dtype, v):
    """TILE (sample-major) at N_MID with V = 5 (one ragged variant tile) and V = 129 (a full tile and one row); AUTO takes it too.
    Needs 12 GiB (V = 129, f32: K rows of 528 bytes)."""
    need_gib(12)
    run_matrix(N_MID, v, "all", "stride", "tile", dtype, True, 0)
    if v == 5:
        run_matrix(N_MID, v, "all", "gather", "auto", dtype, True, 16)


def test_matrix_tile_n_max():
    """TILE f32 at N_MAX, V = 4: 2^31 - 1 output rows of 16 bytes (32 GiB), 2^22 bands.  Needs 40 GiB."""
    need_gib(40)
    run_matrix(N_MAX, 4, "all", "stride", "tile", "f32", True, 0)
