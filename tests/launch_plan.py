"""The launch plans of csrc/launch_plan.h, RUN rather than restated: ``load`` compiles a probe (tests/*_plan_probe.cpp, plan_probe.cpp:
the header behind extern "C" functions) with g++ into a directory under the system temp dir, named by a hash of the sources, and
loads it with ctypes.  The ``*_plan.py`` modules call into the probes; nothing is written into the repository.  A failed compile is
an error.  This module's own probe is plan_probe.cpp, the analysis kernels:

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
HEADER = TESTS.parent / "pgen_rs_amd" / "csrc" / "launch_plan.h"
ABI_HEADER = TESTS.parent / "include" / "pgen_hip.h"   # launch_plan.h takes the kernel ids from it


def load(probe: str) -> ctypes.CDLL:
    """tests/<probe>.cpp compiled against the plan header and loaded: the one builder of every probe (plan_probe, wide_plan_probe,
    gapply_plan_probe, emit_plan_probe)."""
    src = TESTS / f"{probe}.cpp"
    digest = hashlib.sha256(src.read_bytes() + HEADER.read_bytes() + ABI_HEADER.read_bytes()).hexdigest()[:16]
    out_dir = Path(tempfile.gettempdir()) / f"pgen_{probe}_{os.getuid()}_{digest}"
    lib = out_dir / f"{probe}.so"
    if not lib.exists():
        out_dir.mkdir(parents=True, exist_ok=True)
        tmp = out_dir / f"{probe}.{os.getpid()}.so"
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", str(tmp), str(src)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"{probe} did not compile ({' '.join(cmd)}):\n{proc.stdout}{proc.stderr}")
        os.replace(tmp, lib)   # atomic: parallel test processes never load a half-written file
    return ctypes.CDLL(str(lib))


def call_into(lib: ctypes.CDLL, name: str, n_out: int, *args: int) -> tuple[int, ...]:
    """Function ``name`` of a probe on the scalars ``args``: its ``n_out`` results."""
    fn = getattr(lib, name)
    fn.restype = None
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)]
    a = (ctypes.c_int64 * max(len(args), 1))(*[int(x) for x in args])
    out = (ctypes.c_uint64 * n_out)()
    fn(a, out)
    return tuple(out)


_lib = load("plan_probe")
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
    """Function ``name`` of plan_probe.cpp."""
    return call_into(_lib, name, n_out, *args)


def cu_count(num_cus: int) -> int:
    return call("cu_count", 1, num_cus)[0]


def grid_blocks(work: int, per_cu: int, num_cus: int = 256, forced: int = 0) -> int:
    return call("grid_blocks", 1, work, per_cu, num_cus, forced)[0]


def slice_rows(v: int, slice_: int, slices: int) -> tuple[int, int]:
    """Rows [begin, end) of one slice, as the kernels cut them."""
    return call("slice_rows", 2, v, slice_, slices)
