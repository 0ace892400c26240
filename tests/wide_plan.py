"""The launch rule of the stream kernel (gt_wide.hip), RUN from csrc/launch_plan.h (namespace plan::wide) rather than restated.  Like
tests/launch_plan.py: tests/wide_plan_probe.cpp is compiled with g++ into a directory under the system temp dir, named by a hash of
the two sources, and loaded with ctypes; nothing is written into the repository, and a failed compile is an error."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile
from collections import namedtuple
from pathlib import Path

TESTS = Path(__file__).resolve().parent
PROBE = TESTS / "wide_plan_probe.cpp"
HEADER = TESTS.parent / "pgen_rs_amd" / "csrc" / "launch_plan.h"


def _build() -> Path:
    digest = hashlib.sha256(PROBE.read_bytes() + HEADER.read_bytes()).hexdigest()[:16]
    out_dir = Path(tempfile.gettempdir()) / f"pgen_wide_plan_probe_{os.getuid()}_{digest}"
    lib = out_dir / "wide_plan_probe.so"
    if not lib.exists():
        out_dir.mkdir(parents=True, exist_ok=True)
        tmp = out_dir / f"wide_plan_probe.{os.getpid()}.so"
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", str(tmp), str(PROBE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"wide plan probe did not compile ({' '.join(cmd)}):\n{proc.stdout}{proc.stderr}")
        os.replace(tmp, lib)   # atomic: parallel test processes never load a half-written file
    return lib


_lib = ctypes.CDLL(str(_build()))


def _call(name: str, n_out: int, *args: int) -> tuple[int, ...]:
    fn = getattr(_lib, name)
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)]
    a = (ctypes.c_int64 * max(len(args), 1))(*[int(x) for x in args])
    out = (ctypes.c_uint64 * n_out)()
    fn(a, out)
    return tuple(out)


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
