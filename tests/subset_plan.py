"""The kept-subset GT path's dispatch and launch plans, RUN from csrc/launch_plan.h (namespace plan::emit, through
tests/emit_plan_probe.cpp and tests/launch_plan.py) so that the subset tests can place their cells on both sides of every edge AUTO
and the kernels' launch plans derive from N, K, V and the CU count.  numpy only (no torch): the CPU coverage test imports the cell
table from here.

What the header decides and this module only asks for: AUTO's kept-subset chain (``two_pass_shape``, ``very_sparse``,
``rowpick_shape``, ``two_pass``, ``choose_subset``), the forced kernel ids (``accepts``), the chunks of the two passes, the launch
plans of the segment and row-owner kernels, and every constant.  What lives here: the cell table, ``kept_list``, the arm and edge
bookkeeping, and the occupancy figures.

Occupancy-API results cannot be computed on a CPU; they are stated below as constants with their derivation, are UNMEASURED
(gfx950: 160 KiB of LDS per CU, at most 32 waves = 8 four-wave blocks per CU) and go into the header's plans as arguments, where the
launchers pass what the occupancy API says.  Every GPU cell whose arm depends on one of them also runs with the blocks-per-CU knob
set explicitly.

Unreachable edges (listed, not tested): ``two_pass_shape``'s K >= 8 (K * 170 >= N > 4 096 already means K >= 25); ``two_pass``'s
record_size >= 16 (N > 4 096 means R >= 1 024); the compact pass's own max_seg_count > 4 096 refusal (``two_pass`` checks it
first); the row owner's n_seg >= 1 (R >= 16 means N >= 61).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np

import launch_plan

_call = functools.partial(launch_plan.call_into, launch_plan.load("emit_plan_probe"))

# plan::emit's constants (test_subset_plan.py and test_line_plan.py pin their values)
(WAVES, SEG_SAMPLES, COMPACT_MAX_SEG_CODES, COMPACT_SLICE_BYTES, ROWPICK_MAX_KEPT, ROWPICK_MAX_SEGS, ROWPICK_ROWS_PER_WAVE, RUN_LOAD_BYTES,
 RUN_SPAN_BYTES, LR_MAX_ROWS, LR_PFX_BYTES, LR_TAB_MAX_SAMPLES, PICK_MAX_SAMPLES, PICK_STAGE_BYTES, PICK_MAX_BATCH_ROWS, PICK_MAX_PACKED_ROWS,
 PICK_PFX_BYTES, PICK_MAX_LINES_ROWS, PICK_MAX_LINES_PREFIX) = _call("emit_constants", 19)

# plan::emit::Emit, by value
CHOICES = ("rows", "flat", "wide", "runs", "lineruns", "pick", "scan", "rowpick", "two_pass")
assert _call("emit_choices", len(CHOICES)) == tuple(range(len(CHOICES)))

# ---- occupancy (UNMEASURED: what the occupancy API is expected to say, from the LDS each block holds) ---------------------------
LDS_PER_CU = 160 * 1024
MAX_BLOCKS_PER_CU = 8        # 32 waves per CU / 4 waves per block
# gt_scan_pick_kernel: s_idx[16 384 + 16] u16 + s_stage[4][4 096] = 49 184 bytes -> 3 blocks per CU
SCAN_OCCUPANCY = LDS_PER_CU // (2 * (SEG_SAMPLES + 16) + WAVES * (SEG_SAMPLES // 4))
# gt_compact_kernel: s_idx[4 096 + 8] u16 + s_stage[4][4 096] + s_out[4][1 024 + 64] = 28 944 bytes -> 5 blocks per CU
COMPACT_OCCUPANCY = LDS_PER_CU // (2 * (COMPACT_MAX_SEG_CODES + 8) + WAVES * (SEG_SAMPLES // 4) + WAVES * (COMPACT_MAX_SEG_CODES // 4 + 64))

LDS_64K = 65536
NUM_CUS = 256                # MI355X; the GPU tests use the device's own count


def record_size(n: int) -> int:
    """pgenhip_variant_record_size: bytes of a record of n samples."""
    return (2 * n + 7) // 8


def shape(n: int, k: int, v: int = 2, *, kept_list: bool, lines: bool = False, gathered: bool = False, records_dense: bool = True,
          out_dense: bool = True, bound: int = 0, prefix_blob: bool = True) -> tuple:
    """The scalars of a plan::emit::Shape, in the order of its fields (what kernels.h's emit_shape fills from a call): V rows of N
    samples, K kept; `bound`: max_prefix_bytes of a full-line call; one row is dense whatever its strides."""
    return (n, k, record_size(n), v, kept_list, lines, gathered, records_dense or v <= 1, out_dense or v <= 1, bound + 4 * k + 1 if lines else 0,
            prefix_blob)


def n_segments(n: int) -> int:
    return _call("emit_n_segments", 1, n)[0]


def rowpick_lds_bytes(n: int, k: int) -> int:
    """Dynamic LDS of one row-owner block: table | kept-before-segment | four waves x (stage + compact record)."""
    return _call("emit_rowpick_lds_bytes", 1, n, k)[0]


def rowpick_occupancy(n: int, k: int) -> int:
    """UNMEASURED: blocks per CU the LDS allows (the row owner is LDS-limited)."""
    return max(1, min(MAX_BLOCKS_PER_CU, LDS_PER_CU // rowpick_lds_bytes(n, k)))


# ---- the cells' kept lists -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def kept_list(n: int, k: int, layout: str = "random", cluster: int = 0, seed: int = 0) -> np.ndarray:
    """Sorted kept sample indices.  "random": K distinct samples; "all": 0 .. N-1; "cluster": `cluster` of them in segment 1 (its
    first samples), the other K - cluster spread over the other segments (never more than `cluster` in one)."""
    rng = np.random.default_rng(seed * 1_000_003 + n * 7 + k)
    if layout == "all":
        assert k == n
        return np.arange(n, dtype=np.uint32)
    if layout == "cluster":
        seg1 = np.arange(SEG_SAMPLES, SEG_SAMPLES + cluster)
        rest = np.concatenate([np.arange(0, SEG_SAMPLES), np.arange(2 * SEG_SAMPLES, n)])
        others = rng.choice(rest, size=k - cluster, replace=False)
        kept = np.sort(np.concatenate([seg1, others])).astype(np.uint32)
    else:
        kept = np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint32)
    assert kept.size == k
    kept.flags.writeable = False
    return kept


def max_seg_count(kept: np.ndarray, n: int) -> int:
    return int(np.bincount(kept // SEG_SAMPLES, minlength=n_segments(n)).max()) if kept.size else 0


# ---- plans -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScanPlan:
    n_seg: int
    per_cu: int
    groups: int
    xcd_groups: int
    bands: int
    grid: int
    rounds: bool          # more blocks than one resident round holds


@dataclass(frozen=True)
class RowPickPlan:
    lds: int
    per_cu: int
    max_blocks: int
    grid: int
    over_64k: bool


@dataclass(frozen=True)
class Plan:
    kernel: str                        # "rowpick" | "two_pass" | "scan" | "rows" | "pick" | "lineruns" | "all_samples"
    status: str = "ok"                 # "ok" | "bad_arg" (capi.hip refuses) | "hip" (the launcher refuses: PGENHIP_ERR_HIP)
    scan: Optional[ScanPlan] = None
    rowpick: Optional[RowPickPlan] = None
    chunk_rows: int = 0                # two passes: rows per chunk after rounding
    chunks: tuple = ()                 # two passes: (rows, pass-1 kernel, pass-1 plan) per chunk


@dataclass(frozen=True)
class Tune:
    """Knob values as pgenhip_tune takes them (0: not set, the default)."""
    scan_blocks_per_cu: int = 0
    rowpick_blocks_per_cu: int = 0
    scan_chunk_rows: int = 0
    scan_xcd_map: int = 0        # < 0: plain block map
    scan_two_pass: int = 0       # < 0: single pass
    scan_rowpick: int = 0        # < 0: never the row owner

    def rowpick_mode(self) -> int:
        return 0 if self.scan_rowpick < 0 else 1

    def knobs(self) -> dict:
        return {name: value for name, value in self.__dict__.items() if value}


def scan_plan(n: int, k: int, v: int, tune: Tune = Tune(), num_cus: int = NUM_CUS, compact: bool = False, occupancy: Optional[int] = None) -> ScanPlan:
    """plan::emit::scan_plan, what launch_gt_scan (gt_scan.hip) launches, with the unmeasured occupancy figure (or `occupancy`)."""
    occ = occupancy if occupancy is not None else COMPACT_OCCUPANCY if compact else SCAN_OCCUPANCY
    n_seg, per_cu, groups, xcd_groups, bands, grid = _call("emit_scan_plan", 6, n, k, v, compact, occ, tune.scan_blocks_per_cu, tune.scan_xcd_map >= 0, num_cus)
    return ScanPlan(n_seg, per_cu, groups, xcd_groups, bands, grid, grid > per_cu * num_cus)


def rowpick_plan(n: int, k: int, v: int, tune: Tune = Tune(), num_cus: int = NUM_CUS, compact: bool = False, occupancy: Optional[int] = None) -> Optional[RowPickPlan]:
    """plan::emit::rowpick_plan, what launch_gt_rowpick (gt_rowpick.hip) launches, with the unmeasured occupancy figure (or
    `occupancy`); None where it refuses (rowpick_takes)."""
    if not _call("emit_applicable", 11, *shape(n, k, v, kept_list=True), num_cus)[7]:
        return None
    lds = rowpick_lds_bytes(n, k)
    occ = occupancy if occupancy is not None else rowpick_occupancy(n, k)
    per_cu, max_blocks, grid = _call("emit_rowpick_plan", 3, n, v, compact, occ, tune.rowpick_blocks_per_cu, num_cus)
    return RowPickPlan(lds, per_cu, max_blocks, grid, lds > LDS_64K)


def rowpick_applicable(n: int, k: int, v: int, num_cus: int = NUM_CUS) -> bool:
    return bool(_call("emit_applicable", 11, *shape(n, k, v, kept_list=True), num_cus)[8])


def two_pass_shape(n: int, k: int) -> bool:
    return bool(_call("emit_two_pass_shape", 1, n, k)[0])


def very_sparse(n: int, k: int) -> bool:
    return bool(_call("emit_very_sparse", 1, n, k)[0])


def rowpick_shape(n: int, k: int, v: int, tune: Tune, num_cus: int) -> bool:
    return bool(_call("emit_rowpick_shape", 1, *shape(n, k, v, kept_list=True), tune.rowpick_mode() != 0, num_cus)[0])


def two_pass(n: int, k: int, msc: int, lines: bool, tune: Tune) -> bool:
    """plan::emit::two_pass for a kept list that is not the identity, dense output pitch (the cells' only pitch)."""
    return bool(_call("emit_two_pass", 1, *shape(n, k, kept_list=True, lines=lines), tune.scan_two_pass >= 0, msc)[0])


def two_pass_chunks(n: int, k: int, v: int, tune: Tune, num_cus: int):
    """The chunks dispatch_two_pass (capi.hip) walks: (chunk rows, ((rows, pass-1 kernel, pass-1 plan), ...)), by plan::emit::chunks
    and chunk_by_row_owner."""
    rp = rowpick_plan(n, k, v, tune, num_cus, compact=True) if tune.rowpick_mode() != 0 else None
    round_rows = rp.max_blocks * WAVES if rp else 0   # gt_rowpick_resident_waves
    chunk, row_owner = _call("emit_chunks", 2, *shape(n, k, v, kept_list=True), COMPACT_SLICE_BYTES, tune.scan_chunk_rows, tune.rowpick_mode() != 0,
                             round_rows, num_cus)
    out = []
    for row0 in range(0, v, chunk):
        rows = min(chunk, v - row0)
        if _call("emit_chunk_by_row_owner", 1, chunk, row_owner, rows)[0]:
            out.append((rows, "rowpick", rowpick_plan(n, k, rows, tune, num_cus, compact=True)))
        else:
            out.append((rows, "scan", scan_plan(n, k, rows, tune, num_cus, compact=True)))
    return chunk, tuple(out)


# include/pgen_hip.h: PGENHIP_KERNEL_* (test_subset_plan.py checks them against the header)
KERNEL_IDS = {"auto": 0, "rows": 1, "flat": 2, "scan": 3, "wide": 4, "pick": 6, "runs": 7, "rowpick": 8}


def runs_rows(n: int) -> int:
    """Rows per work item of the RUNS mode, all samples kept (plan::emit::run_rows): one wide load of the run's records and one
    span of its text; 0 from N = 3 832 (no whole row of 4N + 1 bytes in a span)."""
    return _call("emit_applicable", 11, *shape(n, n, kept_list=False), NUM_CUS)[9]


def accepts(kernel: int, n: int, k: int, subset: bool, bound: int = 0, gather: bool = False, mode: str = "lines",
            dense_pitch: bool = True) -> bool:
    """Does a call of more than one row take this kernel id: pgenhip_emit_lines (mode "lines", `bound` = max_prefix_bytes) or
    pgenhip_decode_emit / _at (mode "segments", `dense_pitch`: out_stride == 4K + 1)?  plan::emit::accepts, for dense records.
    `subset`: the ctx has a kept list (an identity list is one: forced kernels see it); `gather`: a variant list or record byte
    offsets.  False for AUTO's neighbours that are no kernel id (5, 9 .. 15, bits above the mask)."""
    s = shape(n, k, kept_list=subset, lines=mode == "lines", gathered=gather, out_dense=dense_pitch, bound=bound)
    taken, is_id, _ = _call("emit_accepts", 3, *s, kernel)
    return bool(taken and is_id)


def choose_all_samples(n: int, v: int = 2, **kw) -> str:
    """AUTO for all samples kept (plan::emit::choose_all_samples); kw: the fields of `shape`."""
    return CHOICES[_call("emit_choose_all_samples", 1, *shape(n, n, v, kept_list=False, **kw))[0]]


def choose_subset(n: int, k: int, v: int, *, msc: Optional[int] = None, tune: Tune = Tune(), num_cus: int = NUM_CUS, **kw) -> str:
    """AUTO for a kept list that is not the identity (plan::emit::choose_subset); kw: the fields of `shape`."""
    msc = min(k, SEG_SAMPLES) if msc is None else msc
    return CHOICES[_call("emit_choose_subset", 1, *shape(n, k, v, kept_list=True, **kw), tune.rowpick_mode() != 0, tune.scan_two_pass >= 0, msc, num_cus)[0]]


KERNELS = ("auto", "rows", "scan", "rowpick")


def arm(n: int, k: int, v: int, *, mode: str = "segments", kernel: str = "auto", msc: Optional[int] = None, tune: Tune = Tune(),
        num_cus: int = NUM_CUS) -> Plan:
    """What pgenhip_decode_emit / _at / pgenhip_emit_lines run for a kept list of K of N samples (`msc`: its most kept samples in one
    segment), V rows at the dense pitch, under `kernel` (AUTO: plan::emit::choose_subset; or a forced ROWS / SCAN / ROWPICK).  A
    gathered or offset-addressed launch plans the same (only the kernels' HAS_VIDX instantiation differs).  Full lines are planned
    for empty prefixes (tests/line_plan.py has the prefix-driven limits)."""
    lines = mode == "lines"
    if msc is None:
        msc = min(k, SEG_SAMPLES)
    if kernel != "auto" and not accepts(KERNEL_IDS[kernel], n, k, True, mode=mode):
        return Plan(kernel, status="bad_arg")
    if kernel == "auto":
        if k == n:
            return Plan("all_samples")   # an identity list: AUTO drops it (capi.hip) and takes the all-samples kernels
        kernel = choose_subset(n, k, v, msc=msc, tune=tune, num_cus=num_cus, lines=lines)
    if kernel == "scan":
        return Plan("scan", scan=scan_plan(n, k, v, tune, num_cus))
    if kernel == "rowpick":
        rp = rowpick_plan(n, k, v, tune, num_cus)
        return Plan("rowpick", status="ok" if rp else "hip", rowpick=rp)
    if kernel == "two_pass":
        chunk, chunks = two_pass_chunks(n, k, v, tune, num_cus)
        return Plan("two_pass", chunk_rows=chunk, chunks=chunks)
    return Plan(kernel)   # "rows" | "pick" | "lineruns"


# ---- the GPU cell table --------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Cell:
    group: str
    n: int
    k: int
    v: int
    mode: str = "segments"     # "segments" | "lines"
    gathered: bool = False     # a variant list (pgenhip_decode_emit / _emit_lines with variant_idx)
    at: bool = False           # record byte offsets (pgenhip_decode_emit_at)
    layout: str = "random"
    cluster: int = 0
    tune: Tune = field(default_factory=Tune)
    kernels: tuple = KERNELS   # AUTO + the forced kernels the cell also runs (those that refuse must be refused)

    def kept(self) -> np.ndarray:
        return kept_list(self.n, self.k, self.layout, self.cluster)

    def msc(self) -> int:
        if self.layout == "all":
            return min(self.n, SEG_SAMPLES)
        if self.layout == "cluster":
            return self.cluster
        return max_seg_count(self.kept(), self.n)

    def plan(self, kernel: str = "auto", num_cus: int = NUM_CUS) -> Plan:
        return arm(self.n, self.k, self.v, mode=self.mode, kernel=kernel, msc=self.msc(), tune=self.tune, num_cus=num_cus)


def rowpick_lds_edge(n: int) -> int:
    """The first K whose row-owner block needs more than 64 KiB of LDS (16 337 at N = 20 000, 16 329 at N = 65 536)."""
    return min(k for k in range(1, ROWPICK_MAX_KEPT + 1) if rowpick_lds_bytes(n, k) > LDS_64K)


def cells(num_cus: int = NUM_CUS) -> list:
    """The GPU cells for a device of `num_cus` CUs (every edge that depends on the CU count moves with it)."""
    rp_rows = ROWPICK_ROWS_PER_WAVE * num_cus * WAVES           # 8 192 at 256 CUs
    c = []
    # 1. banded / one band of the segment kernel (N = 10 000: one segment, 2 blocks per CU -> 2 * num_cus groups; bands need
    #    ceil(V / 4) >= 64 groups)
    g1 = 2 * num_cus
    vb = 4 * 64 * g1                                           # 131 072
    c += [Cell("banded", 10_000, 1_000, vb), Cell("banded", 10_000, 999, vb),
          Cell("banded", 10_000, 1_000, vb - 3), Cell("banded", 10_000, 1_000, vb - 4),
          Cell("banded", 10_000, 1_000, vb, tune=Tune(scan_xcd_map=-1), kernels=("auto", "scan")),
          Cell("banded", 10_000, 1_000, vb, tune=Tune(scan_blocks_per_cu=2), kernels=("scan",)),
          Cell("banded", 10_000, 1_000, vb, gathered=True, kernels=("auto", "scan")),
          Cell("banded", 10_000, 1_000, vb, at=True, kernels=("auto", "scan")),
          Cell("banded", 10_000, 1_000, vb, mode="lines", kernels=("auto", "scan"))]
    # groups % 8: n_seg = 9 -> floor(2 * num_cus / 9) groups (56 at 256 CUs), n_seg = 10 -> 51 (other CU counts: the segment count
    #    nearest 9 where the same holds)
    s9 = min((s for s in range(2, 64) if (g1 // s) % 8 == 0 and (g1 // (s + 1)) % 8 != 0), key=lambda s: abs(s - 9))
    n9 = s9 * SEG_SAMPLES
    v9 = 4 * 64 * (g1 // s9)                                   # 14 336
    c += [Cell("banded", n9, 20_000, v9, kernels=("auto", "rows", "scan")), Cell("banded", n9 + 1, 20_000, v9, kernels=("auto", "rows", "scan"))]
    # 2. row owner with more than 64 KiB of LDS, at its kept limit and around the 64-KiB edge; V = rows of every resident wave (AUTO
    #    takes it at N = 20 000) and one row fewer (AUTO goes elsewhere)
    for n in (20_000, 65_536):
        e = rowpick_lds_edge(n)
        for k in sorted({ROWPICK_MAX_KEPT, ROWPICK_MAX_KEPT - 1, e, e - 1}):
            for mode in ("segments", "lines"):
                c.append(Cell("rowpick_lds", n, k, rp_rows, mode=mode))
                c.append(Cell("rowpick_lds", n, k, rp_rows - 1, mode=mode, kernels=("auto",)))
    c += [Cell("rowpick_lds", 20_000, ROWPICK_MAX_KEPT + 1, rp_rows), Cell("rowpick_lds", 20_000, ROWPICK_MAX_KEPT, rp_rows, tune=Tune(rowpick_blocks_per_cu=2), kernels=("auto", "rowpick"))]
    n_max = ROWPICK_MAX_SEGS * SEG_SAMPLES                      # 67 108 864
    c.append(Cell("rowpick_lds", n_max, ROWPICK_MAX_KEPT, 8, tune=Tune(rowpick_blocks_per_cu=1)))
    c.append(Cell("rowpick_lds", n_max, ROWPICK_MAX_KEPT, 8, kernels=("rowpick",)))
    # 3. the row owner's n_seg limit
    c += [Cell("rowpick_nseg", n_max, 1_000, 8), Cell("rowpick_nseg", n_max + 1, 1_000, 8)]
    # 4. more segments than one resident round of blocks (2 per CU)
    nr = 2 * num_cus * SEG_SAMPLES
    c += [Cell("rounds", nr + 1, (nr + 1) // 100, 16), Cell("rounds", nr + 1, (nr + 1) // 100, 16, tune=Tune(scan_blocks_per_cu=2), kernels=("auto",)),
          Cell("rounds", nr + 1, (nr + 1) // 20, 16), Cell("rounds", nr, nr // 20, 16),
          Cell("rounds", nr + 1, (nr + 1) // 20, 16, tune=Tune(scan_blocks_per_cu=2), kernels=("scan",)),
          Cell("rounds", nr + 1, nr + 1, 16, layout="all", kernels=("auto", "rows", "scan"))]
    # 5. two passes whose chunks change kernel: three row-owner chunks of 8 192 rows (at 256 CUs), then a short one through the
    #    segment kernel
    vt = 3 * rp_rows + 1000
    two = Tune(scan_chunk_rows=rp_rows)
    c += [Cell("two_pass", 100_000, 1_999, vt, tune=two), Cell("two_pass", 100_000, 1_999, vt, tune=two, gathered=True, kernels=("auto",)),
          Cell("two_pass", 100_000, 1_999, vt, tune=two, at=True, kernels=("auto",)),
          Cell("two_pass", 100_000, 1_999, vt, tune=two, mode="lines", kernels=("auto",))]
    # default chunks: 32 MiB / 500 B = 67 108 rows, rounded to whole row-owner rounds (65 536 at 256 CUs), then 4 096 rows
    vd = 65_536 + 4_096
    c += [Cell("two_pass", 100_000, 1_999, vd, kernels=("auto",)),
          Cell("two_pass", 100_000, 1_999, vd, tune=Tune(rowpick_blocks_per_cu=2, scan_blocks_per_cu=2), kernels=("auto",))]
    # 6. record byte offsets through the row owner
    c += [Cell("at", 50_000, 5_000, rp_rows, at=True, kernels=("auto", "rowpick"))]
    # 7. AUTO's own edges, both sides, at the smallest V that reaches the arm
    c += [Cell("auto_edges", 20_000, 2_000, rp_rows - 1), Cell("auto_edges", 20_000, 2_000, rp_rows),
          Cell("auto_edges", 24_575, 10_000, rp_rows), Cell("auto_edges", 24_576, 10_000, rp_rows),
          Cell("auto_edges", 16_384, 1_638, rp_rows), Cell("auto_edges", 16_385, 1_638, rp_rows),
          Cell("auto_edges", 100_000, 2_000, rp_rows), Cell("auto_edges", 100_000, 1_999, rp_rows, kernels=("auto",)),
          Cell("auto_edges", 50_000, 10_000, rp_rows), Cell("auto_edges", 50_000, 10_001, rp_rows),
          Cell("auto_edges", 170_000, 1_000, 33), Cell("auto_edges", 170_000, 999, 33),
          Cell("auto_edges", 44_000, 2_000, 33), Cell("auto_edges", 44_000, 2_001, 33),
          Cell("auto_edges", 280_000, 1_000, 33), Cell("auto_edges", 280_000, 1_001, 33),
          Cell("auto_edges", 65_536, 234, 33), Cell("auto_edges", 65_535, 234, 33),
          Cell("auto_edges", 100_000, 4_500, 33, layout="cluster", cluster=COMPACT_MAX_SEG_CODES),
          Cell("auto_edges", 100_000, 4_500, 33, layout="cluster", cluster=COMPACT_MAX_SEG_CODES + 1),
          Cell("auto_edges", 100_000, 1_023, 33, mode="lines"), Cell("auto_edges", 100_000, 1_024, 33, mode="lines")]
    return c


# ---- what the cells must reach (test_subset_plan.py) ------------------------------------------------------------------------------
def arm_tags(cell: Cell, num_cus: int = NUM_CUS) -> set:
    """The arms one cell reaches, over AUTO and its forced kernels."""
    tags = set()
    io = "at" if cell.at else "gathered" if cell.gathered else "plain"
    for kern in cell.kernels:
        p = cell.plan(kern, num_cus)
        tags.add(f"{kern}:{p.kernel}:{p.status}")
        if p.scan:
            s = p.scan
            tags.add(f"scan:{'banded' if s.bands > 1 else 'one_band'}")
            tags.add(f"scan:{'xcd_map' if s.xcd_groups else 'plain_map'}")
            if s.rounds:
                tags.add("scan:rounds")
            if s.bands > 1:
                tags.add(f"scan:banded:{io}:{cell.mode}")
                if not s.xcd_groups:
                    tags.add("scan:banded:plain_map")
        if p.rowpick:
            tags.add(f"rowpick:lds_{'over' if p.rowpick.over_64k else 'within'}_64k:{cell.mode}")
            tags.add(f"rowpick:{io}")
        for rows, k1, sub in p.chunks:
            tags.add(f"two_pass:pass1_{k1}:{io}:{cell.mode}")
            if k1 == "scan" and sub.rounds:
                tags.add("two_pass:pass1_scan:rounds")
        if len({k1 for _, k1, _ in p.chunks}) > 1:
            tags.add(f"two_pass:switch:{io}:{cell.mode}")
    return tags


REACHABLE_ARMS = {
    "auto:rowpick:ok", "auto:two_pass:ok", "auto:scan:ok", "auto:rows:ok", "auto:all_samples:ok",
    "rowpick:rowpick:ok", "rowpick:rowpick:hip", "rowpick:rowpick:bad_arg", "scan:scan:ok", "rows:rows:ok",
    "scan:banded", "scan:one_band", "scan:xcd_map", "scan:plain_map", "scan:rounds", "scan:banded:plain_map",
    "scan:banded:plain:segments", "scan:banded:gathered:segments", "scan:banded:at:segments", "scan:banded:plain:lines",
    "rowpick:lds_over_64k:segments", "rowpick:lds_over_64k:lines", "rowpick:lds_within_64k:segments", "rowpick:lds_within_64k:lines",
    "rowpick:plain", "rowpick:at",
    "two_pass:pass1_rowpick:plain:segments", "two_pass:pass1_rowpick:gathered:segments", "two_pass:pass1_rowpick:at:segments",
    "two_pass:pass1_rowpick:plain:lines", "two_pass:pass1_scan:plain:segments", "two_pass:pass1_scan:gathered:segments",
    "two_pass:pass1_scan:at:segments", "two_pass:pass1_scan:plain:lines", "two_pass:pass1_scan:rounds",
    "two_pass:switch:plain:segments", "two_pass:switch:gathered:segments", "two_pass:switch:at:segments", "two_pass:switch:plain:lines",
}


# An edge: (name, the variable that crosses it, the condition as the source spells it, the forced kernel whose plan it moves).
# Covered when two cells differ only in that variable by one, sit on both sides of the condition and get different plans.
EDGES = [
    ("rowpick_applicable: V >= 8 * num_cus * 4", "v", lambda c, cus: c.v >= ROWPICK_ROWS_PER_WAVE * cus * WAVES, "auto"),
    ("rowpick_shape: N > 16 384", "n", lambda c, cus: c.n > SEG_SAMPLES, "auto"),
    ("rowpick_shape: N < 24 576", "n", lambda c, cus: c.n < 24576, "auto"),
    ("rowpick_shape: K * 50 >= N", "k", lambda c, cus: c.k * 50 >= c.n, "auto"),
    ("rowpick_shape: K * 5 <= N", "k", lambda c, cus: c.k * 5 <= c.n, "auto"),
    ("rowpick_applicable: K <= kRowPickMaxKept", "k", lambda c, cus: c.k <= ROWPICK_MAX_KEPT, "auto"),
    ("two_pass_shape: K * 170 >= N", "k", lambda c, cus: c.k * 170 >= c.n, "auto"),
    ("two_pass_shape: K * 22 <= N", "k", lambda c, cus: c.k * 22 <= c.n, "auto"),
    ("very_sparse: K * 280 <= N", "k", lambda c, cus: c.k * 280 <= c.n, "auto"),
    ("very_sparse: N >= 65 536", "n", lambda c, cus: c.n >= 65536, "auto"),
    ("two_pass: max_seg_count <= kCompactMaxSegCodes", "cluster", lambda c, cus: c.msc() <= COMPACT_MAX_SEG_CODES, "auto"),
    ("two_pass (lines): K >= 1 024", "k", lambda c, cus: c.k >= 1024, "auto"),
    ("banded: K * 10 >= N", "k", lambda c, cus: c.k * 10 >= c.n, "scan"),
    ("banded: ceil(V / 4) >= 64 * groups", "v", lambda c, cus: scan_plan(c.n, c.k, c.v, c.tune, cus).bands > 1, "scan"),
    ("banded: groups % 8 == 0", "n", lambda c, cus: scan_plan(c.n, c.k, c.v, c.tune, cus).groups % 8 == 0, "scan"),
    ("rounds: n_seg > resident blocks", "n", lambda c, cus: scan_plan(c.n, c.k, c.v, c.tune, cus).rounds, "scan"),
    ("row owner: LDS > 64 KiB", "k", lambda c, cus: rowpick_lds_bytes(c.n, c.k) > LDS_64K, "rowpick"),
    ("row owner: n_seg <= 4 096", "n", lambda c, cus: n_segments(c.n) <= ROWPICK_MAX_SEGS, "rowpick"),
]


def edge_pairs(table, num_cus: int = NUM_CUS):
    """{edge name: [(cell on the True side, cell on the False side), ...]} over the cell table."""
    out = {}
    for name, var, cond, kern in EDGES:
        pairs = []
        for a in table:
            if kern not in a.kernels:
                continue
            for b in table:
                if kern not in b.kernels or getattr(b, var) != getattr(a, var) + 1:
                    continue
                if replace(a, **{var: getattr(b, var)}, kernels=b.kernels, group=b.group) != b:
                    continue
                ca, cb = cond(a, num_cus), cond(b, num_cus)
                if ca == cb or a.plan(kern, num_cus) == b.plan(kern, num_cus):
                    continue
                pairs.append((a, b) if ca else (b, a))
        out[name] = pairs
    return out
