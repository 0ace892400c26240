"""The launch plan of gt_gapply.hip, RUN from csrc/launch_plan.h (namespace plan::gapply) rather than restated, for the tests that
are placed around its constants and its slices.  Like tests/launch_plan.py: tests/gapply_plan_probe.cpp is compiled with g++ into a
directory under the system temp dir, named by a hash of the two sources, and loaded with ctypes; nothing is written into the
repository, and a failed compile is an error."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile
from collections import namedtuple
from pathlib import Path

TESTS = Path(__file__).resolve().parent
PROBE = TESTS / "gapply_plan_probe.cpp"
HEADER = TESTS.parent / "pgen_rs_amd" / "csrc" / "launch_plan.h"


def _build() -> Path:
    digest = hashlib.sha256(PROBE.read_bytes() + HEADER.read_bytes()).hexdigest()[:16]
    out_dir = Path(tempfile.gettempdir()) / f"pgen_gapply_plan_probe_{os.getuid()}_{digest}"
    lib = out_dir / "gapply_plan_probe.so"
    if not lib.exists():
        out_dir.mkdir(parents=True, exist_ok=True)
        tmp = out_dir / f"gapply_plan_probe.{os.getpid()}.so"
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", str(tmp), str(PROBE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"gapply plan probe did not compile ({' '.join(cmd)}):\n{proc.stdout}{proc.stderr}")
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


(THREADS, WAVES, GROUP, ROW_TILE, STEP_SAMPLES, SAMPLE_TILE, STEP_ROWS, MIN_SLICE_SAMPLES, MIN_SLICE_ROWS, MAX_GRID_TILES,
 MAX_GRID_BLOCKS) = _call("gapply_constants", 11)

Plan = namedtuple("Plan", "p_tiles y_tiles p_grid y_grid sample_slices row_slices")


def plan(n_variants: int, kept_count: int, n_columns: int, mfma: bool, sample_slices: int = 0, row_slices: int = 0, num_cus: int = 256) -> Plan:
    """Tiles, grid and slices of the two passes of one launch."""
    return Plan(*_call("gapply_plan", 6, n_variants, kept_count, n_columns, int(mfma), sample_slices, row_slices, num_cus))


def slice_samples(k: int, slice_: int, slices: int) -> tuple[int, int]:
    """Samples [begin, end) of one slice of the P pass, as the kernels cut them."""
    return _call("gapply_slice_samples", 2, k, slice_, slices)
