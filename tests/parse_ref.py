"""The grammar of ``pgenhip_parse_gt`` (include/pgen_hip.h) restated in Python: what the GENERAL kernel, the FIXED kernel on the
lines it takes, and AUTO all have to return.  Built on a regular expression, so that the per-byte state machine of
tests/test_parse_gt.py is a second, independent statement.

The sample region of a line is a sequence of fields, each introduced by a tab.  A field's GT is its bytes up to the first ':'.
An allele is ``[0-9]+`` or ``.``; a GT is ``A`` or ``A [/|] B``.  A GT of another form sets BAD_CALL; otherwise a digit token
other than exactly ``0`` and ``1`` sets ALLELE_RANGE; in both cases the code is 3 and the field sets no other flag.  PHASED,
HALF_CALL and HAPLOID come from well-formed, in-range GTs only.
"""
from __future__ import annotations

import re

import numpy as np

FIELD_COUNT, BAD_CALL, ALLELE_RANGE, HALF_CALL, HAPLOID, PHASED, DECLINED = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40

_GT = re.compile(rb"([0-9]+|\.)(?:([/|])([0-9]+|\.))?")

# every field form of the grammar: (field bytes, code, flags)
FORMS = [
    (b"0/0", 0, 0), (b"0/1", 1, 0), (b"1/0", 1, 0), (b"1/1", 2, 0), (b"./.", 3, 0),
    (b"0|0", 0, PHASED), (b"0|1", 1, PHASED), (b"1|0", 1, PHASED), (b"1|1", 2, PHASED), (b".|.", 3, PHASED),
    (b"./0", 3, HALF_CALL), (b"1/.", 3, HALF_CALL), (b".|1", 3, HALF_CALL | PHASED), (b"0|.", 3, HALF_CALL | PHASED),
    (b"0", 0, HAPLOID), (b"1", 2, HAPLOID), (b".", 3, HAPLOID),
    (b"0/1:12:0.5,0.5", 1, 0), (b"1|1:.", 2, PHASED), (b"1:7", 2, HAPLOID), (b".:.:.", 3, HAPLOID), (b"./.:0/1", 3, 0),
    (b"2/0", 3, ALLELE_RANGE), (b"0/2", 3, ALLELE_RANGE), (b"10/1", 3, ALLELE_RANGE), (b"0|01", 3, ALLELE_RANGE), (b"2", 3, ALLELE_RANGE),
    (b"00", 3, ALLELE_RANGE), (b"./3", 3, ALLELE_RANGE), (b"12345678901234567890/0:9", 3, ALLELE_RANGE),
    (b"", 3, BAD_CALL), (b":0/1", 3, BAD_CALL), (b"0/1/1", 3, BAD_CALL), (b"0/", 3, BAD_CALL), (b"/1", 3, BAD_CALL), (b"0//1", 3, BAD_CALL),
    (b"a/0", 3, BAD_CALL), (b"0\\1", 3, BAD_CALL), (b"0 /1", 3, BAD_CALL), (b"..", 3, BAD_CALL), (b".1", 3, BAD_CALL), (b"1.", 3, BAD_CALL),
    (b"0/1|1", 3, BAD_CALL), (b"2/x", 3, BAD_CALL), (b"-1/0", 3, BAD_CALL), (b"0/1\r", 3, BAD_CALL), (b"\x00", 3, BAD_CALL),
    (b"0/\xff", 3, BAD_CALL),
]


def parse_field(field: bytes) -> tuple[int, int]:
    """(code, flags) of one field (the bytes between two tabs)."""
    gt = field.split(b":", 1)[0]
    m = _GT.fullmatch(gt)
    if m is None:
        return 3, BAD_CALL
    alleles = [m.group(1)] + ([m.group(3)] if m.group(2) else [])
    if any(a not in (b"0", b"1", b".") for a in alleles):
        return 3, ALLELE_RANGE
    if len(alleles) == 1:
        return {b"0": 0, b"1": 2, b".": 3}[alleles[0]], HAPLOID
    flags = PHASED if m.group(2) == b"|" else 0
    missing = alleles.count(b".")
    if missing:
        return 3, flags | (HALF_CALL if missing == 1 else 0)
    return int(alleles[0]) + int(alleles[1]), flags


def parse_region(region: bytes, n: int) -> tuple[list[int], int]:
    """The n codes and the flag word of one line's sample region."""
    fields = region.split(b"\t")[1:] if region[:1] == b"\t" else []
    codes, flags = [], 0
    for f in fields[:n]:
        c, fl = parse_field(f)
        codes.append(c)
        flags |= fl
    if len(fields) != n:
        flags |= FIELD_COUNT
    codes += [3] * (n - len(codes))
    return codes, flags


def pack_codes(codes) -> np.ndarray:
    """Codes of one row as a mode-0x02 record: sample s in byte s/4, bits 2*(s%4); pad bits zero."""
    c = np.asarray(codes, dtype=np.uint8)
    r = (c.size + 3) // 4
    p = np.zeros(4 * r, dtype=np.uint8)
    p[:c.size] = c
    p = p.reshape(r, 4)
    return (p[:, 0] | (p[:, 1] << 2) | (p[:, 2] << 4) | (p[:, 3] << 6)).astype(np.uint8)


def parse_lines(text: bytes, field_off, line_end, n: int) -> tuple[np.ndarray, np.ndarray]:
    """``pgenhip_parse_gt`` on host bytes: (records uint8 (V, R), flags uint32 (V)).  Offsets past the text are clamped."""
    text = bytes(text)
    r = (n + 3) // 4
    recs = np.zeros((len(field_off), r), dtype=np.uint8)
    flags = np.zeros(len(field_off), dtype=np.uint32)
    for j, (fo, le) in enumerate(zip(field_off, line_end)):
        fo, le = min(int(fo), len(text)), min(int(le), len(text))
        codes, flags[j] = parse_region(text[fo:le] if fo < le else b"", n)
        recs[j] = pack_codes(codes)
    return recs, flags


def mask_pad(records: np.ndarray, n: int) -> np.ndarray:
    """Records with the pad bits of the last byte zeroed."""
    out = np.array(records, dtype=np.uint8, copy=True)
    if n % 4 and out.size:
        out[..., -1] &= (1 << (2 * (n % 4))) - 1
    return out


def fixed_takes(region: bytes, n: int) -> bool:
    """Whether the FIXED shape takes a line: exactly 4n bytes of ``\\t[01.][/|][01.]``."""
    return len(region) == 4 * n and re.fullmatch(rb"(?:\t[01.][/|][01.])*", region) is not None
