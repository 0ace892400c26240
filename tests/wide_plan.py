"""The launch rule of the stream kernel (gt_wide.hip), RUN from csrc/launch_plan.h (namespace plan::wide) rather than restated.
tests/wide_plan_probe.cpp is built and loaded by tests/launch_plan.py (``load``), as every probe is."""
from __future__ import annotations

import functools
from collections import namedtuple

import launch_plan

_call = functools.partial(launch_plan.call_into, launch_plan.load("wide_plan_probe"))


THREADS, STORERS, SPAN_CHUNKS, SHORT_LAUNCH_BYTES, WT_ONE_SPAN_MAX_BYTES, FRONT_STEPS, NT, WT, BURST_ONE_MIN_BYTES, RUNS_LONG_BYTES = _call("wide_constants", 10)

Rule = namedtuple("Rule", "policy burst blocks_per_cu fronts grid")


def spans_per_row(row_bytes: int) -> int:
    return _call("wide_spans_per_row", 1, row_bytes)[0]


def steps(n_items: int) -> int:
    return _call("wide_steps", 1, n_items)[0]


def kernel_choice(text_bytes: int, spans: int, runs: bool = False, policy: int = 0, burst: int = 0) -> tuple[int, int]:
    """(store policy, burst): the kernel a launch runs."""
    return _call("wide_kernel_choice", 5, text_bytes, spans, int(runs), policy, burst)[:2]


def rule(text_bytes: int, spans: int, steps_needed: int, runs: bool = False, occupancy: int = 4, num_cus: int = 256, policy: int = 0,
         blocks_per_cu: int = 0, fronts: int = 0, burst: int = 0) -> Rule:
    """What a launch of `text_bytes` of text in rows of `spans` spans is given; policy, blocks_per_cu, fronts, burst: the forced knobs."""
    return Rule(*_call("wide_rule", 5, text_bytes, spans, int(runs), steps_needed, occupancy, num_cus, policy, blocks_per_cu, fronts, burst))


def launch(n_samples: int, n_variants: int, runs_rows: int = 0, **kw) -> Rule:
    """The rule for a launch of n_variants rows of n_samples kept samples (runs_rows: RUNS mode with that many rows per item)."""
    row = 4 * n_samples + 1
    if runs_rows:
        return rule(n_variants * row, 1, steps(-(-n_variants // runs_rows)), runs=True, occupancy=3, **kw)
    spans = spans_per_row(row)
    return rule(n_variants * row, spans, steps(n_variants * spans), **kw)
