"""numpy reference of pgenhip_join_records: unpack each part's 2-bit codes, apply flip and absent, concatenate, pack with a zero pad."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

import pack_ref

ABSENT = -1
FLIP = np.array([2, 1, 0, 3], dtype=np.uint8)


def join(parts: Sequence[tuple[np.ndarray, np.ndarray, int, Optional[np.ndarray]]], n_variants: int) -> np.ndarray:
    """``parts``: ``(base, record_off, sample_count, flip_or_None)`` — ``base`` a flat uint8 array, ``record_off`` ``n_variants`` byte
    offsets into it (``ABSENT`` = the part has no such row), ``flip`` ``n_variants`` bytes.  -> (n_variants, ceil(N_out/4)) records."""
    cols = []
    for base, record_off, n, flip in parts:
        base = np.asarray(base, dtype=np.uint8).reshape(-1)
        r = (n + 3) // 4
        codes = np.full((n_variants, n), 3, dtype=np.uint8)
        for j in range(n_variants):
            off = int(record_off[j])
            if off == ABSENT or n == 0:
                continue
            row = pack_ref.unpack(base[None, off:off + r], n)[0]
            codes[j] = FLIP[row] if flip is not None and flip[j] else row
        cols.append(codes)
    return pack_ref.pack_codes(np.concatenate(cols, axis=1) if cols else np.zeros((n_variants, 0), dtype=np.uint8))
