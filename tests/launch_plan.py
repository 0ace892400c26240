"""The launch plans of the analysis kernels, RUN rather than restated: compiles tests/plan_probe.cpp (csrc/launch_plan.h behind
extern "C" functions) with g++ into a directory under the system temp dir, named by a hash of the two sources, and loads it with
ctypes.  The ``*_plan.py`` modules call into it; nothing is written into the repository.  A failed compile is an error.

    call("scount_plan", 6, record_size, n_variants, num_cus, slices_per_tile) -> (G, tiles, cols, slices, lds_bytes, slots)
    CONST["vsum.kTileBytes"] -> 32
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile
from pathlib import Path

TESTS = Path(__file__).resolve().parent
PROBE = TESTS / "plan_probe.cpp"
HEADER = TESTS.parent / "pgen_rs_amd" / "csrc" / "launch_plan.h"


def _build() -> Path:
    digest = hashlib.sha256(PROBE.read_bytes() + HEADER.read_bytes()).hexdigest()[:16]
    out_dir = Path(tempfile.gettempdir()) / f"pgen_plan_probe_{os.getuid()}_{digest}"
    lib = out_dir / "plan_probe.so"
    if not lib.exists():
        out_dir.mkdir(parents=True, exist_ok=True)
        tmp = out_dir / f"plan_probe.{os.getpid()}.so"
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", str(tmp), str(PROBE)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"plan probe did not compile ({' '.join(cmd)}):\n{proc.stdout}{proc.stderr}")
        os.replace(tmp, lib)   # atomic: parallel test processes never load a half-written file
    return lib


_lib = ctypes.CDLL(str(_build()))
_lib.plan_constant.restype = ctypes.c_char_p
_lib.plan_constant.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]


def _constants() -> dict[str, int]:
    out, i, v = {}, 0, ctypes.c_uint64()
    while (name := _lib.plan_constant(i, ctypes.byref(v))) is not None:
        out[name.decode()] = v.value
        i += 1
    return out


CONST = _constants()


def call(name: str, n_out: int, *args: int) -> tuple[int, ...]:
    """Probe function ``name`` on the scalars ``args``: its ``n_out`` results."""
    fn = getattr(_lib, name)
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)]
    a = (ctypes.c_int64 * max(len(args), 1))(*[int(x) for x in args])
    out = (ctypes.c_uint64 * n_out)()
    fn(a, out)
    return tuple(out)


def cu_count(num_cus: int) -> int:
    return call("cu_count", 1, num_cus)[0]


def grid_blocks(work: int, per_cu: int, num_cus: int = 256, forced: int = 0) -> int:
    return call("grid_blocks", 1, work, per_cu, num_cus, forced)[0]


def slice_rows(v: int, slice_: int, slices: int) -> tuple[int, int]:
    """Rows [begin, end) of one slice, as the kernels cut them."""
    return call("slice_rows", 2, v, slice_, slices)
