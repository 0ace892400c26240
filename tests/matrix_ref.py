"""The reference of every genotype-matrix comparison: numpy on the record bytes (src/pfile.rs:172-175: sample s in byte s/4, bits
2*(s%4)).  Comparisons are on raw bytes (``view(uint8)``), so NaN patterns compare exactly."""
from __future__ import annotations

import numpy as np


def rsize(n: int) -> int:
    return (2 * n + 7) // 8


def codes(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (V, K) uint8 codes 0..3 of the kept samples (pad bits never read as samples)."""
    v = recs.shape[0]
    c = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, 4 * recs.shape[1])[:, :n]   # (-1 cannot be inferred for V == 0)
    if kept is not None:
        c = c[:, np.asarray(kept, dtype=np.int64)]
    return c


def matrix(recs: np.ndarray, n: int, kept, values: np.ndarray, sample_major: bool = False) -> np.ndarray:
    """``values[codes]`` ((V, K), or its transpose (K, V) with ``sample_major``); ``values``: four elements of the dtype."""
    m = np.asarray(values)[codes(recs, n, kept)]
    return np.ascontiguousarray(m.T) if sample_major else m


def raw(m: np.ndarray) -> np.ndarray:
    """The bytes of a 2-D array, row by row: (rows, cols * itemsize) uint8."""
    m = np.ascontiguousarray(m)
    return m.view(np.uint8).reshape(m.shape[0], m.shape[1] * m.itemsize)


def default_values(np_dtype) -> np.ndarray:
    """0, 1, 2 and: -1 for signed integers, all ones for unsigned, NaN for floating dtypes."""
    dt = np.dtype(np_dtype)
    if dt.kind == "f":
        return np.array([0, 1, 2, np.nan], dtype=dt)
    if dt.kind == "u":
        return np.array([0, 1, 2, np.iinfo(dt).max], dtype=dt)
    return np.array([0, 1, 2, -1], dtype=dt)


def gt_text_codes(gt: np.ndarray, v: int, k: int) -> np.ndarray:
    """decode_emit's GT text (v rows of 4k + 1 bytes) -> (v, k) codes: 0/0 -> 0, 0/1 -> 1, 1/1 -> 2, ./. -> 3."""
    if k == 0:
        return np.zeros((v, 0), dtype=np.uint8)
    rows = np.asarray(gt, dtype=np.uint8)[: v * (4 * k + 1)].reshape(v, 4 * k + 1)[:, : 4 * k].reshape(v, k, 4)
    a, b = rows[:, :, 1], rows[:, :, 3]
    out = np.full((v, k), 255, dtype=np.uint8)
    out[(a == ord("0")) & (b == ord("0"))] = 0
    out[(a == ord("0")) & (b == ord("1"))] = 1
    out[(a == ord("1")) & (b == ord("1"))] = 2
    out[(a == ord(".")) & (b == ord("."))] = 3
    assert (out != 255).all() and (rows[:, :, 0] == 9).all() and (rows[:, :, 2] == ord("/")).all()
    return out
