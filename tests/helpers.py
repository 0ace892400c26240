"""Shared helpers for the parity tests (test-side only)."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"


def load_case(name: str):
    """-> (n_variants, n_samples, records (V,R) uint8, kept or None, expected GT bytes)."""
    raw = (GOLDEN / "cases" / f"{name}.pgen").read_bytes()
    assert raw[:3] == b"\x6c\x1b\x02" and raw[11] == 0x40
    v = int.from_bytes(raw[3:7], "little")
    n = int.from_bytes(raw[7:11], "little")
    r = (2 * n + 7) // 8
    recs = np.frombuffer(raw[12:], dtype=np.uint8).reshape(v, r)
    keep_path = GOLDEN / "cases" / f"{name}.keep"
    kept: Optional[np.ndarray] = None
    if keep_path.exists():
        txt = keep_path.read_text().split()
        kept = np.array([int(t) for t in txt], dtype=np.uint32)
    gt = np.frombuffer((GOLDEN / "cases" / f"{name}.gt").read_bytes(), dtype=np.uint8)
    return v, n, recs, kept, gt


def case_names():
    return sorted(p.stem for p in (GOLDEN / "cases").glob("*.pgen"))


def sha_table():
    return json.loads((GOLDEN / "sha256.json").read_text())


def basic1_known():
    return json.loads((GOLDEN / "basic1_known.json").read_text())


def plain_record_filesets(d: Path, n_samples: int = 40, n_plain: int = 60, seed: int = 2031):
    """-> (variable-width prefix, fixed-width prefix): the same `n_plain` plain 2-bit records and the same rows for them in .pvar
    (two chromosomes, RTYPE 0) and .psam.  In the mode-0x10 file a compressed record (RTYPE 1) follows every fourth plain one,
    by turns shorter than a record (the host stages over such a gap) and four records long (it starts a new span), so
    `--include-var 'RTYPE == "0"'` keeps the same rows of both filesets and only the staging differs."""
    import sys

    sys.path.insert(0, str(GOLDEN))
    import make_golden_vw as writer

    rng = np.random.default_rng(seed)
    r = (2 * n_samples + 7) // 8
    plain = [rng.integers(0, 256, size=r, dtype=np.uint8).tobytes() for _ in range(n_plain)]
    row = lambda i, t: b"%d\t%d\tv%d\tC\tT\t%d\n" % (7 if i < n_plain // 2 else 8, 500 + 3 * i, i, t)
    recs, vw_rows, fixed_rows = [], [], []
    for i, rec in enumerate(plain):
        recs.append((0, rec))
        vw_rows.append(row(i, 0))
        fixed_rows.append(row(i, 0))
        if i % 4 == 3:
            recs.append((1, bytes(3 if i % 8 == 3 else 4 * r)))
            vw_rows.append(b"9\t%d\tc%d\tC\tT\t1\n" % (500 + 3 * i + 1, i))
    data, _ = writer.write_vw(n_samples, recs, 8, 2)
    fixed = bytes([0x6C, 0x1B, 0x02]) + n_plain.to_bytes(4, "little") + n_samples.to_bytes(4, "little") + b"\x40" + b"".join(plain)
    for name, pgen, rows in (("vw", data, vw_rows), ("fixed", fixed, fixed_rows)):
        (d / f"{name}.pgen").write_bytes(pgen)
        (d / f"{name}.pvar").write_bytes(b"#CHROM\tPOS\tID\tREF\tALT\tRTYPE\n" + b"".join(rows))
        (d / f"{name}.psam").write_bytes(b"#IID\tSEX\n" + b"".join(b"S%04d\tNA\n" % k for k in range(n_samples)))
    return d / "vw", d / "fixed"
