"""numpy reference of pgenhip_pack_records: unpack the 2-bit codes, select the kept samples, map, pack with a zero pad."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

BED_MAP = (3, 2, 0, 1)


def unpack(recs: np.ndarray, n: int) -> np.ndarray:
    """(V, >= ceil(n/4)) uint8 records -> (V, n) codes (sample s in byte s/4, bits 2*(s%4))."""
    recs = np.asarray(recs, dtype=np.uint8)
    s = np.arange(n)
    return (recs[:, s >> 2] >> (2 * (s & 3)).astype(np.uint8)) & 3


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """(V, K) codes -> (V, ceil(K/4)) uint8 records, pad bits zero."""
    v, k = codes.shape
    rk = (k + 3) // 4
    padded = np.zeros((v, 4 * rk), dtype=np.uint8)
    padded[:, :k] = codes
    q = padded.reshape(v, rk, 4)
    return (q[:, :, 0] | q[:, :, 1] << 2 | q[:, :, 2] << 4 | q[:, :, 3] << 6).astype(np.uint8)


def pack(recs: np.ndarray, n: int, kept: Optional[Sequence[int]] = None, code_map: Optional[Sequence[int]] = None) -> np.ndarray:
    """The packed records of the kept samples (all of them when ``kept`` is None) of every row of ``recs``."""
    codes = unpack(recs, n)
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    if code_map is not None:
        codes = np.asarray(code_map, dtype=np.uint8)[codes]
    return pack_codes(codes)


def pgen_file(packed: np.ndarray, k: int) -> bytes:
    """The fixed-width .pgen that holds ``packed`` as its records of ``k`` samples."""
    v = packed.shape[0]
    return bytes([0x6C, 0x1B, 0x02]) + v.to_bytes(4, "little") + k.to_bytes(4, "little") + b"\x40" + packed.tobytes()


def bed_file(packed: np.ndarray) -> bytes:
    return bytes([0x6C, 0x1B, 0x01]) + packed.tobytes()
