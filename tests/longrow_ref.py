"""A slab-wise reference for rows too long to decode on the host: plain torch integer ops on the record bytes (src/pfile.rs:172-175:
sample s in byte s >> 2, bits 2 * (s & 3)), on whatever device the tensors live on, a slab of samples (or of kept ranks) at a time.
Nothing here calls a product kernel; test_longrow_ref.py holds every function against the CPU oracle and the numpy references with
a slab of 97 samples, so that slab seams fall inside bytes.

Conventions: ``rec`` is a 1-D uint8 tensor whose first byte is the record's first byte (>= ceil(n / 4) bytes); ``kept`` is None (all
samples) or the ascending kept list as a numpy uint32 array or an int32 / int64 tensor (``as_kept`` moves it to a device once);
``recs_rows`` is the list of the selected rows' records in output order (a gathered row that repeats appears twice).  Every check
returns None when all bytes agree, else a tuple that names the first difference (tests put it in the assertion message: the
offset is what tells which 32-bit quantity wrapped)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

SLAB = 1 << 26
SENT = 0xA5               # the sentinel byte of every output frame
FRONT, BACK = 67, 64      # sentinel bytes in front of an output (at least) and behind it
GIB = 1 << 30
GT_TEXT = np.frombuffer(b"\t0/0\t0/1\t1/1\t./.", dtype=np.uint8).reshape(4, 4)


def rsize(n: int) -> int:
    return (2 * n + 7) // 8


def as_kept(kept, device) -> Optional[torch.Tensor]:
    """The kept list as a tensor on ``device`` (uint32 numpy arrays travel as int32: every sample index is below 2^31)."""
    if kept is None:
        return None
    if isinstance(kept, torch.Tensor):
        return kept.to(device)
    a = np.ascontiguousarray(np.asarray(kept, dtype=np.uint32))
    return torch.from_numpy(a.view(np.int32)).to(device)


def kept_count(n: int, kept) -> int:
    return n if kept is None else int(kept.numel() if isinstance(kept, torch.Tensor) else np.asarray(kept).size)


def codes(rec: torch.Tensor, s0: int, s1: int, kept=None) -> torch.Tensor:
    """The 2-bit codes (uint8, 0..3) of samples [s0, s1) of one record; with a kept list, of the samples of ranks [s0, s1)."""
    if s1 <= s0:
        return torch.empty(0, dtype=torch.uint8, device=rec.device)
    if kept is None:
        b0, b1 = s0 >> 2, (s1 + 3) >> 2
        by = rec[b0:b1]
        c = torch.stack([(by >> sh) & 3 for sh in (0, 2, 4, 6)], dim=1).reshape(-1)
        return c[s0 - 4 * b0: s1 - 4 * b0]
    s = as_kept(kept, rec.device)[s0:s1].to(torch.int64)
    return (rec[s >> 2] >> (2 * (s & 3)).to(torch.uint8)) & 3


def _slabs(count: int, slab: int):
    for a in range(0, count, slab):
        yield a, min(count, a + slab)


def _first_diff(got: torch.Tensor, want: torch.Tensor) -> Optional[int]:
    """Flat index of the first differing element of two equal-shaped tensors, or None."""
    ne = (got != want).reshape(-1)
    if not bool(ne.any()):
        return None
    return int(torch.nonzero(ne)[0, 0])


def check_gt_row(out_row: torch.Tensor, rec: torch.Tensor, n: int, kept=None, slab: int = SLAB):
    """``out_row``: the 4K + 1 bytes of one GT segment.  -> None, or (rank, byte in the rank's four, got, want) of the first wrong
    byte; a wrong line feed is reported as (K, 0, got, 10)."""
    kept = as_kept(kept, rec.device)
    k = kept_count(n, kept)
    text = torch.from_numpy(GT_TEXT.copy()).to(rec.device)
    for a, b in _slabs(k, slab):
        want = text[codes(rec, a, b, kept).to(torch.int64)]
        got = out_row[4 * a: 4 * b].view(b - a, 4)
        i = _first_diff(got, want)
        if i is not None:
            return a + i // 4, i % 4, int(got.reshape(-1)[i]), int(want.reshape(-1)[i])
    if int(out_row[4 * k]) != 10:
        return k, 0, int(out_row[4 * k]), 10
    return None


def row_counts(rec: torch.Tensor, n: int, kept=None, slab: int = SLAB) -> list:
    """[hom-ref, het, hom-alt, missing] of one record over the kept samples, as Python integers."""
    kept = as_kept(kept, rec.device)
    tot = [0, 0, 0, 0]
    for a, b in _slabs(kept_count(n, kept), slab):
        c = codes(rec, a, b, kept)
        for code in range(4):
            tot[code] += int((c == code).sum())
    return tot


def check_sample_counts(counts: torch.Tensor, recs_rows: Sequence[torch.Tensor], n: int, kept=None, prefill: int = 0,
                        slab: int = SLAB):
    """``counts``: the 4K int32 words pgenhip_sample_counts wrote (u32 bit patterns).  The expected word is the number of rows of
    ``recs_rows`` in which the rank has the code, plus ``prefill``, modulo 2^32.  -> None or (rank, code, got, want)."""
    dev = counts.device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    flat = counts.reshape(-1)
    for a, b in _slabs(k, slab):
        want = torch.full((b - a, 4), prefill, dtype=torch.int64, device=dev)
        for rec in recs_rows:
            c = codes(rec, a, b, kept)
            for code in range(4):
                want[:, code] += c == code
        want &= 0xFFFFFFFF
        got = flat[4 * a: 4 * b].view(b - a, 4).to(torch.int64) & 0xFFFFFFFF
        i = _first_diff(got, want)
        if i is not None:
            return a + i // 4, i % 4, int(got.reshape(-1)[i]), int(want.reshape(-1)[i])
    return None


def check_matrix(out: torch.Tensor, recs_rows: Sequence[torch.Tensor], n: int, kept, elem_bytes: int, patterns, sample_major: bool,
                 pitch: int, slab: int = SLAB):
    """``out``: uint8 tensor whose first byte is element (0, 0); ``patterns``: the 4 * elem_bytes bytes written for codes 0..3;
    ``pitch``: bytes between rows (variants, or samples with ``sample_major``).  -> None or (row j, rank k, byte, got, want)."""
    dev = out.device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    v = len(recs_rows)
    eb = elem_bytes
    pat = torch.from_numpy(np.ascontiguousarray(np.asarray(patterns, dtype=np.uint8)).reshape(4, eb).copy()).to(dev)
    if not sample_major:
        for j, rec in enumerate(recs_rows):
            for a, b in _slabs(k, slab):
                want = pat[codes(rec, a, b, kept).to(torch.int64)]
                got = out[j * pitch + a * eb: j * pitch + b * eb].view(b - a, eb)
                i = _first_diff(got, want)
                if i is not None:
                    return j, a + i // eb, i % eb, int(got.reshape(-1)[i]), int(want.reshape(-1)[i])
        return None
    if v == 0:
        return None
    slab = max(1, min(slab, (1 << 30) // (v * eb)))   # a slab of ranks holds all V columns: bound its bytes, not its ranks
    for a, b in _slabs(k, slab):
        want = torch.stack([pat[codes(rec, a, b, kept).to(torch.int64)] for rec in recs_rows], dim=1)   # (ranks, V, eb)
        got = out[a * pitch:].as_strided((b - a, v, eb), (pitch, eb, 1))
        i = _first_diff(got, want)
        if i is not None:
            return (i // eb) % v, a + i // (eb * v), i % eb, int(got.reshape(-1)[i]), int(want.reshape(-1)[i])
    return None


def padding_untouched(out: torch.Tensor, rows: int, row_bytes: int, pitch: int, fill: int, slab_rows: int = 1 << 24) -> bool:
    """Do the ``pitch - row_bytes`` bytes behind each of the first ``rows - 1`` rows of ``out`` still hold ``fill``?"""
    if pitch == row_bytes or rows <= 1:
        return True
    for a, b in _slabs(rows - 1, slab_rows):
        pad = out[a * pitch + row_bytes:].as_strided((b - a, pitch - row_bytes), (pitch, 1))
        if not bool((pad == fill).all()):
            return False
    return True


# ---- shared by the GPU files: free-memory gate and sentinel frames -----------------------------------------------------------------
def need_gib(gib: float):
    """Skip the calling test when the card has less free memory than the case states."""
    import pytest

    free, _total = torch.cuda.mem_get_info(0)
    if free < gib * GIB:
        pytest.skip(f"needs {gib:.0f} GiB of free HBM, have {free / GIB:.0f}")


def framed(nbytes: int, device, align: int = 1):
    """-> (buffer of sentinel bytes, byte offset of the payload: >= FRONT and a multiple of ``align`` from the allocation's start)."""
    front = -(-FRONT // align) * align
    buf = torch.full((front + nbytes + BACK,), SENT, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    return buf, front


def frame_ok(buf: torch.Tensor, front: int, nbytes: int) -> bool:
    return bool((buf[:front] == SENT).all()) and bool((buf[front + nbytes:] == SENT).all())
