"""The launch plan of gt_logit.hip, RUN from csrc/launch_plan.h (namespace plan::logit) rather than restated, for the tests that are
placed around its buckets and groups.  tests/logit_plan_probe.cpp is built and loaded by tests/launch_plan.py (``load``), as every
probe is."""
from __future__ import annotations

import functools
from collections import namedtuple

import launch_plan

_call = functools.partial(launch_plan.call_into, launch_plan.load("logit_plan_probe"))

THREADS, WAVES, MAX_P, SUMS, BLOCKS_PER_CU = _call("logit_constants", 5)

Shape = namedtuple("Shape", "bucket waves_per_row group_rows sum_fmas")
Grids = namedtuple("Grids", "groups fast general")


def shape(p: int) -> Shape:
    """What FAST is compiled for at p = n_cov + 1 design columns, and the FMAs per sample that the sums of one evaluation take."""
    return Shape(*_call("logit_shape", 4, p))


def row_part(a: int, waves: int) -> int:
    """Which of a row's waves owns row a of H."""
    return _call("logit_row_part", 1, a, waves)[0]


def grids(n_variants: int, p: int, num_cus: int = 256, blocks: int = 0) -> Grids:
    return Grids(*_call("logit_grids", 3, n_variants, p, num_cus, blocks))
