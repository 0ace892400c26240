"""The launch plan of gt_gapply.hip, RUN from csrc/launch_plan.h (namespace plan::gapply) rather than restated, for the tests that
are placed around its constants and its slices.  tests/gapply_plan_probe.cpp is built and loaded by tests/launch_plan.py (``load``),
as every probe is."""
from __future__ import annotations

import functools
from collections import namedtuple

import launch_plan

_call = functools.partial(launch_plan.call_into, launch_plan.load("gapply_plan_probe"))


(THREADS, WAVES, GROUP, ROW_TILE, STEP_SAMPLES, SAMPLE_TILE, STEP_ROWS, MIN_SLICE_SAMPLES, MIN_SLICE_ROWS, MAX_GRID_TILES,
 MAX_GRID_BLOCKS) = _call("gapply_constants", 11)

Plan = namedtuple("Plan", "p_tiles y_tiles p_grid y_grid sample_slices row_slices")


def plan(n_variants: int, kept_count: int, n_columns: int, mfma: bool, sample_slices: int = 0, row_slices: int = 0, num_cus: int = 256) -> Plan:
    """Tiles, grid and slices of the two passes of one launch."""
    return Plan(*_call("gapply_plan", 6, n_variants, kept_count, n_columns, int(mfma), sample_slices, row_slices, num_cus))


def slice_samples(k: int, slice_: int, slices: int) -> tuple[int, int]:
    """Samples [begin, end) of one slice of the P pass, as the kernels cut them."""
    return _call("gapply_slice_samples", 2, k, slice_, slices)
