"""Test-side helpers of the large genotype-count tests: the oracle's counts of device-resident records (copied back in chunks,
counted on a bounded thread pool: the C loop releases the GIL), sentinel-guarded launches, and a comparison that names the
first mismatching row."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np
import torch

import pgen_oracle as oracle

THREADS = 12                 # the oracle's pool; never sized by os.cpu_count() (a GPU host shows far more CPUs than a job may use)
CHUNK_BYTES = 256 << 20      # records copied back per step
SENT = -0x5A5A5A5B           # 0xA5A5A5A5 as int32


def pool() -> ThreadPoolExecutor:
    return ThreadPoolExecutor(max_workers=THREADS)


def oracle_counts_dense(host: np.ndarray, n: int, kept_sets, ex: ThreadPoolExecutor) -> dict:
    """host: (V, R) uint8 records on the host -> {key: (V, 4) int64 oracle counts} for every kept set of ``kept_sets``."""
    v = host.shape[0]
    piece = max(1, -(-v // (4 * THREADS)))
    out = {key: np.empty((v, 4), dtype=np.int64) for key in kept_sets}
    futs = []
    for a in range(0, v, piece):
        b = min(v, a + piece)
        for key, kept in kept_sets.items():
            futs.append((key, a, b, ex.submit(oracle.genotype_counts, host[a:b].reshape(-1), b - a, n, kept)))
    for key, a, b, f in futs:
        out[key][a:b] = f.result()
    return out


def oracle_counts_device(d_recs: torch.Tensor, v: int, n: int, kept_sets, ex: ThreadPoolExecutor) -> dict:
    """Oracle counts of V dense device records (stride R from the tensor's first byte): copied back CHUNK_BYTES at a time while
    the pool counts the chunk before."""
    r = oracle.variant_record_size(n)
    rows = max(1, CHUNK_BYTES // r)
    piece = max(1, -(-rows // THREADS))
    out = {key: np.empty((v, 4), dtype=np.int64) for key in kept_sets}
    inflight = []   # (futures of one chunk); at most two chunks on the host at a time

    def drain(futs):
        for key, a, b, f in futs:
            out[key][a:b] = f.result()

    for c0 in range(0, v, rows):
        c1 = min(v, c0 + rows)
        host = d_recs[c0 * r: c1 * r].cpu().numpy()
        futs = []
        for a in range(c0, c1, piece):
            b = min(c1, a + piece)
            seg = host[(a - c0) * r: (b - c0) * r]
            for key, kept in kept_sets.items():
                futs.append((key, a, b, ex.submit(oracle.genotype_counts, seg, b - a, n, kept)))
        inflight.append(futs)
        if len(inflight) > 1:
            drain(inflight.pop(0))
    for futs in inflight:
        drain(futs)
    return out


def host_counts(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 4)


def guarded_counts(eng, kern: int, n_rows: int, lead: int = 1, **kw) -> np.ndarray:
    """Counts into a sentinel-framed int32 buffer at an odd 4-byte offset (``lead`` words of sentinel in front, 8 behind); a write
    outside the n_rows x 4 words fails.  ``base`` + ``record_off`` in kw: the _at entry point."""
    dev = eng.torch_device
    buf = torch.full((lead + 4 * n_rows + 8,), SENT, dtype=torch.int32, device=dev)
    out = buf[lead:]
    if "base" in kw:
        res = eng.genotype_counts_at(kw["base"], kw["record_off"], n_rows, out=out, kernel=kern)
    else:
        res = eng.genotype_counts(out=out, n_variants=n_rows, kernel=kern, **kw)
    eng.wait()
    h = buf.cpu().numpy()
    assert (h[:lead] == SENT).all() and (h[lead + 4 * n_rows:] == SENT).all(), f"kernel {kern} wrote outside its {n_rows} rows of counts"
    assert res.shape == (n_rows, 4) and res.dtype == torch.int32
    return h[lead: lead + 4 * n_rows].view(np.uint32).astype(np.int64).reshape(n_rows, 4)


def assert_counts_equal(got: np.ndarray, want: np.ndarray, what: str, rows_per_grid: Optional[int] = None):
    """Exact int64 comparison; on a mismatch: how many rows differ, the first of them with both count vectors (and, given the rows
    one grid covers, which pass of the grid-stride loop and which row of that pass it is)."""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return
    j = int(bad[0])
    where = f" (grid pass {j // rows_per_grid}, row {j % rows_per_grid} of it)" if rows_per_grid else ""
    raise AssertionError(f"{what}: {bad.size} of {len(want)} rows differ; first row {j}{where}: got {got[j].tolist()} "
                         f"(hom-ref, het, hom-alt, missing), oracle {want[j].tolist()}; last differing row {int(bad[-1])}")
