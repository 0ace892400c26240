"""Full VCF lines (pgenhip_emit_lines) at the prefix lengths the kernels plan around, byte for byte against the oracle.

The prefix length bound (``max_prefix_bytes``) is the one input of the full-line path that the kernels plan with: rows per item and
seam lanes of the line-run kernel, batch rows and seam-chunk lanes of the pick family's full-line kernel (and its row-by-row
fallback), lanes per line of the prefix copy in the stream / segment / row-owner / pick kernels, tiles per row of the general kernel,
and AUTO's choice between them.  tests/line_plan.py runs that arithmetic from csrc/launch_plan.h; every edge it derives gets a cell on each side, run
through AUTO and through every forced kernel that accepts the shape (a forced kernel that refuses must be one the plan says refuses).
Each output buffer is framed by sentinel bytes that must stay untouched; lines start behind output byte 0 at an unaligned pointer
and the blob does not start at a prefix.  Prefix lengths per cell: all at the bound, uniform in 0 .. bound with 20 % empty, and one
at the bound among 1-byte ones (behind an empty one, as the first and the last line of a batch).

The max_prefix_bytes contract (include/pgen_hip.h):
  * a loose bound (true max + 1, 2x, 4 096, 1 MiB) is exact through every kernel;
  * max_prefix_bytes + 4K + 1 >= 2^31 is PGENHIP_ERR_TOO_LARGE before any launch;
  * an understated bound may give wrong lines but touches no byte outside [line_off[0], line_off[V]).  Audit of the kernels'
    global accesses under an understated bound (what makes that hold):
      - line-run kernel (gt_wide.hip): the loader's blob load is sized by the TRUE prefix offsets (p_start .. p_end of the run,
        at most 64 16-byte pieces of the blob); it parks at most kLrPfxBytes / 16 = 48 pieces in LDS; phase B reads the prefixes
        from LDS only; every store is a chunk of the item's own range [line_off[row0], line_off[row0 + B]) (whole chunks inside
        the launch's lines, the launch's ragged first / last chunk byte by byte);
      - pick-lines kernel (gt_pick.hip): blob loads sized by the true offsets, two 1-KiB pieces at most; prefixes read from the
        LDS stage; interior and seam stores addressed from line_off, seam chunks inside [S0, S1) of the line range;
      - prefix copy (gt_common.hip.h copy_prefix_rows), general kernel (gt_rows.hip), row-owner kernel: lengths and addresses
        from prefix_off / line_off; the bound only sets lanes per line, tiles per row (a short bound leaves line tails
        unwritten, every chunk is checked against the true line length).
    No global address derives from the bound.
  * d_prefix_blob == NULL with bound 0 (every prefix empty) is legal, even with prefix offsets that are not multiples of 16.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import line_plan as LP
import pgen_oracle as oracle
import pgen_rs_amd
from helpers import GOLDEN
from pgen_rs_amd import _capi
from subset_plan import accepts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5
K_AUTO, K_ROWS, K_WIDE, K_SCAN, K_PICK, K_RUNS, K_ROWPICK = (_capi.KERNEL_AUTO, _capi.KERNEL_ROWS, _capi.KERNEL_WIDE, _capi.KERNEL_SCAN,
                                                              _capi.KERNEL_PICK, _capi.KERNEL_RUNS, _capi.KERNEL_ROWPICK)
ALL_KERNELS = (K_AUTO, K_ROWS, K_WIDE, K_SCAN, K_PICK, K_RUNS, K_ROWPICK)
KNAME = {K_AUTO: "AUTO", K_ROWS: "ROWS", K_WIDE: "WIDE", K_SCAN: "SCAN", K_PICK: "PICK", K_RUNS: "RUNS", K_ROWPICK: "ROWPICK"}


def prefix_lengths(rng, v, p, dist, batch=8):
    if dist == "at_bound":
        return np.full(v, p, dtype=np.int64)
    if dist == "uniform":
        lens = rng.integers(0, p + 1, size=v)
        lens[rng.random(v) < 0.2] = 0
        return lens
    assert dist == "spike"
    # one prefix at the bound among 1-byte ones, directly behind an empty one: as the first line, the last line, and the first and
    # the last line of a batch of `batch` rows
    lens = np.ones(v, dtype=np.int64)
    spots = {0, v - 1, batch, 2 * batch - 1, 3 * batch, 5 * batch - 1}
    for i in sorted(s for s in spots if 0 <= s < v):
        if i >= 1:
            lens[i - 1] = 0
        lens[i] = p
    return lens


_BASIC1 = None


def basic1_prefixes():
    """Body-line prefixes of the reference's basic1.pvar: the columns each followed by '\\t', then "GT" (as tests/ref_vcf.py joins them)."""
    global _BASIC1
    if _BASIC1 is None:
        rows = [ln.split(b"\t") for ln in (GOLDEN / "basic1" / "basic1.pvar").read_bytes().split(b"\n") if ln and not ln.startswith(b"#")]
        _BASIC1 = [b"".join(c + b"\t" for c in row) + b"GT" for row in rows]
    return _BASIC1


class Call:
    """One emit_lines call: records, prefixes, offsets, framed output, and the oracle's lines."""

    def __init__(self, rng, n, kept, v, lens=None, prefixes=None, gather=False, out_pad=69, lead_gap=3, blob_lead=3, rec_off=5):
        self.n, self.kept, self.v, self.gather = n, kept, v, gather
        self.k = n if kept is None else int(kept.size)
        r = oracle.variant_record_size(n)
        v_file = v + 7 if gather else v
        self.rec_off = 0 if gather else rec_off
        self.recs = rng.integers(0, 256, size=self.rec_off + v_file * r + 16, dtype=np.uint8)
        self.vidx = np.sort(rng.choice(v_file, size=v, replace=False)).astype(np.uint32) if gather else None
        if prefixes is None:
            prefixes = [bytes(rng.integers(33, 127, size=int(q), dtype=np.uint8)) for q in lens]
        self.plens = np.array([len(q) for q in prefixes], dtype=np.int64)
        self.blob = np.frombuffer(b"?" * blob_lead + b"".join(prefixes) + b"!" * 16, dtype=np.uint8)
        self.poff = (blob_lead + np.concatenate([[0], np.cumsum(self.plens)])).astype(np.int64)
        self.loff = (lead_gap + np.concatenate([[0], np.cumsum(self.plens + 4 * self.k + 1)])).astype(np.int64)
        self.out_pad, self.lead_gap = out_pad, lead_gap
        self.want = oracle.emit_lines(self.recs[self.rec_off:], v, n, self.blob, self.poff.astype(np.uint64),
                                      (self.loff - lead_gap).astype(np.uint64), kept_idx=kept, variant_idx=self.vidx)
        self.d_recs = torch.from_numpy(self.recs).to(DEV)
        self.d_blob = torch.from_numpy(self.blob.copy()).to(DEV)
        self.d_poff = torch.from_numpy(self.poff).to(DEV)
        self.d_loff = torch.from_numpy(self.loff).to(DEV)
        self.d_vidx = None if self.vidx is None else torch.from_numpy(self.vidx.astype(np.int32)).to(DEV)

    @property
    def pmax(self):
        return int(self.plens.max()) if self.plens.size else 0

    def run(self, eng, kernel, bound=None, frame=64, blob=True):
        """-> (status, framed output as numpy, index of the first line byte in it)."""
        bound = self.pmax if bound is None else bound
        pre = frame + self.out_pad                          # the output pointer: unaligned, `frame` sentinel bytes in front of line 0 at least
        total = pre + int(self.loff[-1]) + frame
        out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
        rc = _capi.lib.pgenhip_emit_lines(eng._ctx, self.d_recs.data_ptr() + self.rec_off, oracle.variant_record_size(self.n),
                                          None if self.d_vidx is None else self.d_vidx.data_ptr(), self.v,
                                          self.d_blob.data_ptr() if blob else None, self.d_poff.data_ptr(), self.d_loff.data_ptr(),
                                          bound, out.data_ptr() + pre, kernel)
        eng.wait()
        return rc, out.cpu().numpy(), pre + self.lead_gap

    def check(self, eng, kernel, tag, bound=None, frame=64, expect_ok=True, blob=True):
        """Exact lines + untouched frame when the kernel takes the shape; a refusal exactly where `expect_ok` is False."""
        rc, got, start = self.run(eng, kernel, bound=bound, frame=frame, blob=blob)
        if not expect_ok:
            assert rc == _capi.ERR_BAD_ARG, f"{tag} {KNAME[kernel]}: expected a refusal, got status {rc}"
            assert (got == SENTINEL).all(), f"{tag} {KNAME[kernel]}: a refused call wrote"
            return
        assert rc == _capi.OK, f"{tag} {KNAME[kernel]}: status {rc} ({_capi.lib.pgenhip_last_error_detail().decode()})"
        end = start + self.want.size
        assert (got[:start] == SENTINEL).all() and (got[end:] == SENTINEL).all(), f"{tag} {KNAME[kernel]}: wrote outside the lines"
        body = got[start:end]
        if bytes(body) != self.want.tobytes():
            bad = np.flatnonzero(body != self.want)
            line = int(np.searchsorted(self.loff - self.lead_gap, bad[0], side="right")) - 1
            raise AssertionError(f"{tag} {KNAME[kernel]}: {bad.size} bytes differ, first at {bad[:6]} (line {line}, prefix length "
                                 f"{self.plens[line]}, byte {bad[0] - (self.loff[line] - self.lead_gap)} of the line)")


def run_cell(n, subset, p, shapes, kernels=ALL_KERNELS, seed=0, keep_frac=0.1, kept=None, batch=8):
    """`shapes`: (dist, V, gather) per call; every kernel of `kernels` on each, refusals checked against `accepts`."""
    rng = np.random.default_rng(seed)
    if subset and kept is None:
        kept = np.sort(rng.choice(n, size=max(8, int(n * keep_frac)), replace=False)).astype(np.uint32)
    k = n if kept is None else int(kept.size)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for dist, v, gather in shapes:
            c = Call(rng, n, kept, v, lens=prefix_lengths(rng, v, p, dist, batch=batch), gather=gather)
            for kern in kernels:
                c.check(eng, kern, f"n={n} k={k} P={p} {dist} v={v} gather={gather}", bound=p,
                        expect_ok=accepts(kern, n, k, subset, p, gather))


def _ids(vals):
    return [str(x) for x in vals]


# ---- 1. the line-run kernel's edges: seam lanes (2 -> 3 -> 4 -> 5 -> 6), rows per item 7 -> 6 (AUTO leaves it) and 2 -> 1 (refused)
LR_P = sorted({q for e in LP.LR_SEAM_EDGES + [LP.LR_ROWS_7_6, LP.LR_ROWS_2_1] for q in (e, e + 1)})


@pytest.mark.parametrize("p", LR_P, ids=_ids(LR_P))
@pytest.mark.parametrize("subset", [False, True], ids=["all", "kept"])
@pytest.mark.parametrize("n", [100, 300, 303, 1000])
def test_line_run_kernel_prefix_edges(n, subset, p):
    """Line-run kernel at its prefix-driven limits (N = 1 000: the record and span limits give three rows, so only the 250/251 edge
    moves its rows there; the seam lanes move at every N).  AUTO takes it for all samples below N = 1 000 with >= 7 rows per item and
    for kept subsets below N = 300; forced RUNS refuses from P = 251 (one row per item)."""
    b = max(2, LP.lineruns_rows(n, n if not subset else max(8, n // 10), subset, p))
    shapes = (("at_bound", 5 * b + 3, False), ("uniform", 1, False), ("spike", 6 * b, False), ("uniform", 2 * b - 1, True))
    run_cell(n, subset, p, shapes, seed=1000 * n + p, batch=b)


@pytest.mark.parametrize("p", [LP.LR_LINE_LIMIT - 4 * 1900 - 1, LP.LR_LINE_LIMIT - 4 * 1900], ids=["line7664", "line7665"])
def test_line_run_kernel_line_length_limit(p):
    """N = 1 900, all samples: a line of 4K + 1 + P = 7 664 bytes still gives two lines per span, 7 665 one (forced RUNS refuses)."""
    run_cell(1900, False, p, (("at_bound", 9, False), ("spike", 8, False)), kernels=(K_AUTO, K_RUNS, K_WIDE, K_PICK), seed=p, batch=2)


# ---- 2. the pick family's full-line kernel: seam-chunk lanes, batch rows by the prefix stage, the row-by-row fallback, K 3/4
def _pick_ps(n, k):
    ps = {q for e in LP.PICK_SEAM_EDGES + [LP.PICK_ROWS_FALLBACK, LP.pick_cross_edge(n, k)] for q in (e, e + 1)}
    return sorted(ps)


PICK_CELLS = [(n, p) for n in (61, 300, 2504, 4093, 4096) for p in _pick_ps(n, max(8, n // 10))]


@pytest.mark.parametrize("n,p", PICK_CELLS, ids=[f"{n}-{p}" for n, p in PICK_CELLS])
@pytest.mark.parametrize("subset", [True, False], ids=["kept", "all"])
def test_pick_lines_prefix_edges(n, p, subset):
    """Pick family on dense records: batch rows clamped by kPfxBytes (including where that clamp overtakes the record stage's, e.g.
    290/291 at N = 4 096 with 10 % kept), the fallback to row by row above 677 bytes, and the seam-chunk lanes by (P + 31) / 16
    chunks (48/49, 112/113, 240/241, 496/497).  A gathered call goes row by row at every P."""
    k = n if not subset else max(8, n // 10)
    b = max(2, LP.pick_lines_rows(n, k, p))
    shapes = (("at_bound", 4 * b + 1, False), ("uniform", 1, False), ("spike", 6 * b, False), ("at_bound", b + 2, True))
    run_cell(n, subset, p, shapes, seed=7 * n + p, batch=b)


@pytest.mark.parametrize("p", [0, 49, 166, 677, 678])
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n", [61, 300, 2504])
def test_pick_lines_smallest_keep_lists(n, k, p):
    """K = 3 goes row by row, K = 4 through interiors + seams (rows of 17 bytes: a 16-byte chunk meets at most two rows)."""
    rng = np.random.default_rng(n + 13 * k + p)
    kept = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint32)
    b = max(2, LP.pick_lines_rows(n, k, p))
    run_cell(n, True, p, (("at_bound", 3 * b + 2, False), ("spike", 4 * b, False)), kept=kept, seed=n + p, batch=b)


@pytest.mark.parametrize("frac", [None, 0.26, 0.5], ids=["k1", "k26pct", "k50pct"])
def test_pick_lines_real_prefixes(frac):
    """N = 2 504 with the reference's own basic1.pvar prefixes (130-250 bytes): K = 1 (the reference README's second example), 26 %
    and 50 % kept, and all samples; every kernel that takes the shape, with and without a gather."""
    n = 2504
    rng = np.random.default_rng(2504 if frac is None else int(frac * 1000))
    kept = np.array([17], dtype=np.uint32) if frac is None else np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
    pf = basic1_prefixes()
    for kk in (kept, None):
        with pgen_rs_amd.GtEngine(n, kept_idx=kk, device=0) as eng:
            k = n if kk is None else int(kk.size)
            for v, gather in ((1, False), (301, False), (97, True)):
                i0 = int(rng.integers(0, len(pf) - v))
                c = Call(rng, n, kk, v, prefixes=pf[i0 : i0 + v], gather=gather)
                for kern in ALL_KERNELS:
                    c.check(eng, kern, f"basic1 prefixes n={n} k={k} v={v} gather={gather}", expect_ok=accepts(kern, n, k, kk is not None, c.pmax, gather))


# ---- 3. the prefix copy (8 -> 16 lanes per line at 48/49) and prefixes longer than a 4-KiB group and a span
COPY_CELLS = [(n, p) for n in (1400, 2504, 70_001) for p in (LP.COPY_SHIFT_EDGE, LP.COPY_SHIFT_EDGE + 1, 4096, 16384)]


@pytest.mark.parametrize("n,p", COPY_CELLS, ids=[f"{n}-{p}" for n, p in COPY_CELLS])
@pytest.mark.parametrize("subset", [False, True], ids=["all", "kept"])
def test_prefix_copy_long_prefixes(n, p, subset):
    """Stream kernel (WIDE), segment kernel (SCAN), row-owner kernel, pick row by row (a gather, and P > 677), the general kernel."""
    v = 37 if n < 70_000 else 9
    run_cell(n, subset, p, (("at_bound", v, False), ("uniform", v, True), ("spike", 2 * v, False)), seed=n + p, batch=8)


# ---- 4. the row-owner kernel (AUTO needs 8 x CUs x 4 waves = 8 192 rows on the MI355X) and the two passes
ROWPICK_CELLS = [(n, p) for n in (16_385, 20_000, 40_000) for p in (0, 49, 166, 250, 700, 4096)]


@pytest.mark.parametrize("n,p", ROWPICK_CELLS, ids=[f"{n}-{p}" for n, p in ROWPICK_CELLS])
def test_row_owner_kernel_prefixes(n, p):
    """Kept subsets of 10 % on long records with 8 192 rows: AUTO (the row-owner kernel for this density), forced ROWPICK, SCAN."""
    dist = ("at_bound", "uniform", "spike")[p % 3]
    run_cell(n, True, p, ((dist, 8192, False), ("at_bound", 40, True)), kernels=(K_AUTO, K_ROWPICK, K_SCAN), seed=n + p, batch=64)


@pytest.mark.parametrize("p", [166, 700, 4096])
def test_two_pass_lines_prefixes(p):
    """N = 70 001, K = 1 915 (the two-pass band), V below the row owner's 8 192 rows: compact pass + the stream kernel's lines."""
    rng = np.random.default_rng(p)
    kept = np.sort(rng.choice(70_001, size=1915, replace=False)).astype(np.uint32)
    run_cell(70_001, True, p, (("at_bound", 300, False), ("uniform", 301, True), ("spike", 64, False)), kernels=(K_AUTO, K_ROWS),
             kept=kept, seed=p, batch=16)


# ---- 5. the max_prefix_bytes contract
LOOSE_CELLS = [(100, False), (300, True), (300, False), (2504, True), (2504, False), (20_000, True)]


@pytest.mark.parametrize("n,subset", LOOSE_CELLS, ids=[f"{n}-{'kept' if s else 'all'}" for n, s in LOOSE_CELLS])
@pytest.mark.parametrize("how", ["plus1", "twice", "4096", "1MiB"])
def test_loose_bound_is_exact(n, subset, how):
    """A bound above the longest prefix is legal and moves every plan (line-run declines, pick-lines goes row by row, the general kernel
    grows its grid): lines stay byte-exact through AUTO and every forced kernel that takes the shape at that bound."""
    rng = np.random.default_rng(n + len(how))
    kept = np.sort(rng.choice(n, size=max(8, n // 10), replace=False)).astype(np.uint32) if subset else None
    k = n if kept is None else int(kept.size)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for dist, v, gather in (("uniform", 61, False), ("at_bound", 9, True)):
            c = Call(rng, n, kept, v, lens=prefix_lengths(rng, v, 40, dist), gather=gather)
            bound = {"plus1": c.pmax + 1, "twice": 2 * c.pmax, "4096": 4096, "1MiB": 1 << 20}[how]
            for kern in ALL_KERNELS:
                c.check(eng, kern, f"n={n} k={k} bound={bound} (max {c.pmax})", bound=bound, expect_ok=accepts(kern, n, k, subset, bound, gather))


@pytest.mark.parametrize("kernel", ALL_KERNELS, ids=[KNAME[q] for q in ALL_KERNELS])
def test_absurd_bound_is_too_large(kernel):
    """max_prefix_bytes + 4K + 1 >= 2^31 is PGENHIP_ERR_TOO_LARGE before any launch (the general kernel would otherwise grid-stride
    over ~2^26 tiles per row, or truncate its tiles per row): nothing is written, and the ctx stays usable."""
    rng = np.random.default_rng(5)
    n = 300
    kept = np.sort(rng.choice(n, size=30, replace=False)).astype(np.uint32)
    for kk in (None, kept):
        k = n if kk is None else int(kk.size)
        with pgen_rs_amd.GtEngine(n, kept_idx=kk, device=0) as eng:
            c = Call(rng, n, kk, 17, lens=prefix_lengths(rng, 17, 30, "uniform"))
            for bound in (1 << 40, (1 << 31) - 4 * k - 1, (1 << 64) - 1):
                rc, got, _ = c.run(eng, kernel, bound=bound)
                assert rc == _capi.ERR_TOO_LARGE, f"bound {bound}: status {rc}"
                assert (got == SENTINEL).all()
            # the largest bound that is planned: legal, exact where the kernel takes it (ROWS: a grid of V x 2^17 tiles, a few ms)
            if kernel == K_ROWS:
                c.check(eng, kernel, f"bound 2^31 - 4K - 2 k={k}", bound=(1 << 31) - 4 * k - 2)
            c.check(eng, kernel, "after TOO_LARGE", expect_ok=accepts(kernel, n, k, kk is not None, c.pmax, False))


UNDER_CELLS = [(100, False, 95), (300, False, 128), (300, True, 166), (1000, False, 251), (2504, True, 291), (2504, False, 166),
               (4096, True, 678), (20_000, True, 700), (1400, False, 4096)]


@pytest.mark.parametrize("n,subset,p", UNDER_CELLS, ids=[f"{n}-{'kept' if s else 'all'}-{p}" for n, s, p in UNDER_CELLS])
def test_understated_bound_stays_in_bounds(n, subset, p):
    """Stated bound = true - 1, true / 2 and 0 (non-NULL blob): the call returns PGENHIP_OK and no byte outside [line_off[0],
    line_off[V]) changes — 64-KiB sentinel frames on both sides inside the same allocation.  The lines themselves may be wrong (see the
    module docstring for the audit)."""
    rng = np.random.default_rng(n + p)
    kept = np.sort(rng.choice(n, size=max(8, n // 10), replace=False)).astype(np.uint32) if subset else None
    k = n if kept is None else int(kept.size)
    frame = 64 << 10
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for dist, v in (("at_bound", 64), ("spike", 97)):
            c = Call(rng, n, kept, v, lens=prefix_lengths(rng, v, p, dist, batch=6))
            for bound in (p - 1, p // 2, 0):
                for kern in ALL_KERNELS:
                    if not accepts(kern, n, k, subset, bound, False):
                        continue
                    rc, got, start = c.run(eng, kern, bound=bound, frame=frame)
                    tag = f"n={n} k={k} P={p} bound={bound} {dist} {KNAME[kern]}"
                    assert rc == _capi.OK, f"{tag}: status {rc}"
                    end = start + c.want.size
                    assert (got[:start] == SENTINEL).all(), f"{tag}: wrote in front of line 0 ({np.flatnonzero(got[:start] != SENTINEL)[:4] - start})"
                    assert (got[end:] == SENTINEL).all(), f"{tag}: wrote behind the last line ({np.flatnonzero(got[end:] != SENTINEL)[:4]})"


@pytest.mark.parametrize("n,subset", [(100, False), (300, True), (300, False), (1400, False), (2504, True), (20_000, True)],
                         ids=["100-all", "300-kept", "300-all", "1400-all", "2504-kept", "20000-kept"])
def test_null_blob_with_empty_prefixes(n, subset):
    """d_prefix_blob = NULL, bound 0, every prefix_off entry 3 (not a multiple of 16): each line is the K-sample GT text + '\\n', through
    AUTO and every kernel that takes the shape (the line-run loader loads no prefix piece when a run has no prefix bytes)."""
    rng = np.random.default_rng(n)
    kept = np.sort(rng.choice(n, size=max(8, n // 10), replace=False)).astype(np.uint32) if subset else None
    k = n if kept is None else int(kept.size)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for v in (1, 40, 8192 if n >= 16_385 else 301):
            c = Call(rng, n, kept, v, lens=np.zeros(v, dtype=np.int64))
            assert (c.poff == 3).all()
            assert c.want.tobytes() == oracle.decode_emit(c.recs[c.rec_off:], v, n, kept_idx=kept).tobytes()
            for kern in ALL_KERNELS:
                c.check(eng, kern, f"NULL blob n={n} k={k} v={v}", bound=0, blob=False, expect_ok=accepts(kern, n, k, subset, 0, False))


# ---- 6. the row-owner kernel at its advertised K limit
@pytest.mark.parametrize("n", [20_000, 65_536])
@pytest.mark.parametrize("lines", [False, True], ids=["segments", "lines"])
def test_row_owner_kernel_at_its_kept_limit(n, lines):
    """K = 16 384 (dynamic LDS 65 632 / 65 648 bytes per block at N = 20 000 / 65 536: above 64 KiB, within gfx950's 160 KiB per CU)
    with 8 192 rows, forced ROWPICK and AUTO (the row-owner kernel at N = 20 000; at N = 65 536 25 % kept is outside its band); and
    K = 16 385: forced ROWPICK refuses, AUTO stays exact."""
    assert LP.rowpick_lds_bytes(n, LP.ROWPICK_MAX_KEPT) > 65536
    rng = np.random.default_rng(n)
    v = 8192
    for k in (LP.ROWPICK_MAX_KEPT, LP.ROWPICK_MAX_KEPT + 1):
        kept = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            if lines:
                c = Call(rng, n, kept, v, lens=np.full(v, 166, dtype=np.int64))
                for kern in (K_AUTO, K_ROWPICK):
                    c.check(eng, kern, f"n={n} K={k} lines", expect_ok=kern == K_AUTO or k <= LP.ROWPICK_MAX_KEPT)
                continue
            r = oracle.variant_record_size(n)
            recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
            want = oracle.decode_emit(recs, v, n, kept_idx=kept)
            d_recs = torch.from_numpy(recs).to(DEV)
            for kern in (K_AUTO, K_ROWPICK):
                out = torch.full((want.size + 128,), SENTINEL, dtype=torch.uint8, device=DEV)
                if kern == K_ROWPICK and k > LP.ROWPICK_MAX_KEPT:
                    with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                        eng.decode_emit(d_recs, v, out=out, kernel=kern, out_offset=64)
                    assert ei.value.status == _capi.ERR_BAD_ARG
                    continue
                eng.decode_emit(d_recs, v, out=out, kernel=kern, out_offset=64)
                eng.wait()
                got = out.cpu().numpy()
                assert (got[:64] == SENTINEL).all() and (got[64 + want.size :] == SENTINEL).all()
                assert bytes(got[64 : 64 + want.size]) == want.tobytes(), f"n={n} K={k} {KNAME[kern]}: GT segments differ"


# ---- 7. randomized AUTO differential with real prefix lengths
_EDGES_N = [8, 9, 60, 61, 64, 100, 299, 300, 301, 303, 399, 400, 767, 768, 999, 1000, 1001, 1023, 1024, 1399, 1400, 1401, 1900, 1915, 1916,
            2504, 4093, 4095, 4096, 4097, 16_385, 20_011, 65_535, 65_536, 70_001]


def _mixed_lengths(rng, v):
    real = [len(q) for q in basic1_prefixes()]
    pick = rng.random(v)
    lens = np.where(pick < 0.4, rng.choice(real, size=v),
                    np.where(pick < 0.6, rng.integers(0, 61, size=v), np.where(pick < 0.85, rng.integers(60, 701, size=v), rng.integers(700, 5001, size=v))))
    return lens.astype(np.int64)


@pytest.mark.parametrize("seed", range(16))
def test_randomized_auto_real_prefix_lengths(seed):
    """AUTO against the oracle: N on the dispatch edges, prefix lengths a mixture (40 % basic1.pvar lengths, 20 % 0-60, 25 % 60-700,
    15 % 700-5 000), a loose bound (true max + 0 .. 300) in a third of the cases, keep lists none / dense / sparse, gathers.
    16 seeds x 25 cases."""
    rng = np.random.default_rng(31_000 + seed)
    for case_i in range(25):
        n = int(rng.choice(_EDGES_N))
        v = int(min(max(1, 3_000_000 // (n + 500)), rng.choice([1, 2, 17, 64, 257, 1031])))
        mode = rng.choice(["all", "dense", "sparse"])
        kept = None
        if mode == "dense" and n >= 2:
            kept = np.sort(rng.choice(n, size=max(1, int(n * rng.uniform(0.2, 0.9))), replace=False)).astype(np.uint32)
        elif mode == "sparse" and n >= 2:
            kept = np.sort(rng.choice(n, size=max(1, int(n * rng.uniform(0.005, 0.06))), replace=False)).astype(np.uint32)
        gather = bool(rng.random() < 0.3)
        c = Call(rng, n, kept, v, lens=_mixed_lengths(rng, v), gather=gather, out_pad=int(rng.integers(0, 130)),
                 lead_gap=int(rng.integers(0, 20)), blob_lead=int(rng.integers(0, 20)), rec_off=int(rng.integers(0, 18)))
        bound = c.pmax + (int(rng.integers(0, 301)) if rng.random() < 1 / 3 else 0)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            c.check(eng, K_AUTO, f"seed={seed} case={case_i} n={n} k={c.k} v={v} gather={gather} bound={bound}", bound=bound)
