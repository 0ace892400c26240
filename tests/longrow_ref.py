"""A slab-wise reference for rows too long to decode on the host: plain torch integer ops on the record bytes (src/pfile.rs:172-175:
sample s in byte s >> 2, bits 2 * (s & 3)), on whatever device the tensors live on, a slab of samples (or of kept ranks) at a time.
Nothing here calls a product kernel; test_longrow_ref.py holds every function against the CPU oracle and the numpy references with
a slab of 97 samples (the Gram product's two functions with slabs of 1, 7 and 64 ranks), so that slab seams fall inside bytes.

Conventions: ``rec`` is a 1-D uint8 tensor whose first byte is the record's first byte (>= ceil(n / 4) bytes); ``kept`` is None (all
samples) or the ascending kept list as a numpy uint32 array or an int32 / int64 tensor (``as_kept`` moves it to a device once);
``recs_rows`` is the list of the selected rows' records in output order (a gathered row that repeats appears twice).  Every check
returns None when all bytes agree, else a tuple that names the first difference (tests put it in the assertion message: the
offset is what tells which 32-bit quantity wrapped)."""
from __future__ import annotations

from fractions import Fraction
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


def check_packed(out_row: torch.Tensor, rec: torch.Tensor, n: int, kept=None, map4=None, slab: int = SLAB):
    """``out_row``: the ceil(K / 4) bytes of one packed row (pgenhip_pack_records); ``map4``: the four codes written for input codes
    0..3 (None: the identity).  Compared rank by rank, so slab seams fall inside bytes of both rows.  -> None, or (rank, got code,
    want code) of the first wrong code = output byte rank >> 2; set pad bits in the last byte are reported as (K, pad bits, 0)."""
    kept = as_kept(kept, rec.device)
    k = kept_count(n, kept)
    m = torch.tensor([0, 1, 2, 3] if map4 is None else [int(x) for x in map4], dtype=torch.uint8, device=rec.device)
    for a, b in _slabs(k, slab):
        want = m[codes(rec, a, b, kept).to(torch.int64)]
        got = codes(out_row, a, b)
        i = _first_diff(got, want)
        if i is not None:
            return a + i, int(got[i]), int(want[i])
    if k % 4:
        pad = int(out_row[(k - 1) >> 2]) >> (2 * (k % 4))
        if pad:
            return k, pad, 0
    return None


def check_joined(out_row: torch.Tensor, parts_rows: Sequence[Optional[torch.Tensor]], starts: Sequence[int], counts: Sequence[int],
                 flips: Sequence[bool], absent: Sequence[bool], n: int, slab: int = SLAB):
    """``out_row``: the ceil(n / 4) bytes of one joined row (pgenhip_join_records).  Part p's record ``parts_rows[p]`` (not read where
    ``absent[p]``) holds ``counts[p]`` samples that must appear as output samples ``starts[p]`` onwards: as they are, with codes 0 and
    2 exchanged where ``flips[p]``, all 3 where ``absent[p]``.  Compared sample by sample, so slab seams and part seams fall inside
    bytes of both sides.  -> None, or (output sample, got code, want code) of the first wrong code in sample order; set pad bits in the
    last byte are reported as (n, pad bits, 0)."""
    flip = torch.tensor([2, 1, 0, 3], dtype=torch.uint8, device=out_row.device)
    assert sum(counts) == n and all(s == sum(counts[:p]) for p, s in enumerate(starts))
    for p, (start, count) in enumerate(zip(starts, counts)):
        for a, b in _slabs(count, slab):
            got = codes(out_row, start + a, start + b)
            if absent[p]:
                want = torch.full_like(got, 3)
            else:
                want = codes(parts_rows[p], a, b)
                if flips[p]:
                    want = flip[want.to(torch.int64)]
            i = _first_diff(got, want)
            if i is not None:
                return start + a + i, int(got[i]), int(want[i])
    if n % 4:
        pad = int(out_row[(n - 1) >> 2]) >> (2 * (n % 4))
        if pad:
            return n, pad, 0
    return None


def check_scores(scores: torch.Tensor, recs_rows: Sequence[torch.Tensor], n: int, kept, weights, miss=None, prefill: int = 0,
                 slab: int = SLAB):
    """``scores``: the K * C float64 values pgenhip_sample_scores wrote.  ``weights``: (V, C) small integers, ``miss``: V small integers
    or None, both indexed by the row's position in ``recs_rows``; ``prefill``: the integer every score held before an accumulating call
    (0 otherwise).  The sums are formed in int64, so the scores must equal them exactly as float64.  -> None or (rank, column, got, want)."""
    dev = scores.device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    w = torch.from_numpy(np.asarray(weights, dtype=np.int64).reshape(len(recs_rows), -1).copy()).to(dev)
    c = int(w.shape[1])
    ms = [0] * len(recs_rows) if miss is None else [int(x) for x in np.asarray(miss).reshape(-1)]
    flat = scores.reshape(-1)
    slab = max(1, min(slab, (1 << 26) // c))   # a slab of ranks holds C columns of int64 and of float64: bound its bytes
    for a, b in _slabs(k, slab):
        want = torch.full((b - a, c), int(prefill), dtype=torch.int64, device=dev)
        for j, rec in enumerate(recs_rows):
            code = codes(rec, a, b, kept).to(torch.int64)
            d = torch.where(code == 3, torch.full_like(code, ms[j]), code)
            want += d[:, None] * w[j][None, :]
        want = want.to(torch.float64)
        got = flat[c * a: c * b].view(b - a, c)
        i = _first_diff(got, want)   # (NaN differs from everything, itself included)
        if i is not None:
            return a + i // c, i % c, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])
    return None


def pair_table(rec_i: torch.Tensor, rec_j: torch.Tensor, n: int, kept=None, slab: int = SLAB) -> list:
    """The 4 x 4 table of two records over the kept samples, as Python integers: t[a][b] = samples with code a in ``rec_i`` and code b
    in ``rec_j`` (sixteen masked sums per slab)."""
    kept = as_kept(kept, rec_i.device)
    tot = [0] * 16
    for a, b in _slabs(kept_count(n, kept), slab):
        code = 4 * codes(rec_i, a, b, kept) + codes(rec_j, a, b, kept)
        sums = torch.stack([(code == q).sum() for q in range(16)]).tolist()
        tot = [x + int(y) for x, y in zip(tot, sums)]
    return [tot[4 * a: 4 * a + 4] for a in range(4)]


def r2_of_table(t) -> np.float32:
    """r^2 of a 4 x 4 table's cells with a, b in {0, 1, 2} (include/pgen_hip.h), from Python integers: the exact rational
    (n Sxy - Sx Sy)^2 / ((n Sxx - Sx^2)(n Syy - Sy^2)) rounded ONCE to float32 (to nearest, ties to even, by integer division);
    NaN when a variance is 0."""
    n = sx = sy = sxx = syy = sxy = 0
    for a in range(3):
        for b in range(3):
            c = int(t[a][b])
            n, sx, sy, sxx, syy, sxy = n + c, sx + a * c, sy + b * c, sxx + a * a * c, syy + b * b * c, sxy + a * b * c
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if vx == 0 or vy == 0:
        return np.float32(np.nan)
    cov = n * sxy - sx * sy
    x = Fraction(cov * cov, vx * vy)
    if x == 0:
        return np.float32(0.0)
    num, den = x.numerator, x.denominator
    e = 23 - (num.bit_length() - den.bit_length())      # 2^22 < x 2^e < 2^24
    if (num << max(e, 0)) < (den << (23 + max(-e, 0))):
        e += 1                                          # 2^23 <= x 2^e < 2^24: 24 significant bits in front of the point
    e = min(e, 149)                                     # subnormals: fewer bits
    top, bottom = num << max(e, 0), den << max(-e, 0)
    q, rem = divmod(top, bottom)
    if 2 * rem > bottom or (2 * rem == bottom and q & 1):
        q += 1
    return np.float32(np.ldexp(np.float64(q), -e))      # q <= 2^24: exact in both formats


def sample_pair_tables(recs_rows: Sequence[torch.Tensor], n: int, kept, a_ranks, b_ranks) -> torch.Tensor:
    """(a_count, b_count, 4, 4) int64: entry [i, l, x, y] = rows of ``recs_rows`` in which rank a_begin + i has code x and rank
    b_begin + l has code y.  ``a_ranks``, ``b_ranks``: (begin, count), small ranges of rows of any length."""
    dev = recs_rows[0].device
    kept = as_kept(kept, dev)
    (a0, ac), (b0, bc) = a_ranks, b_ranks
    out = torch.zeros((ac, bc, 16), dtype=torch.int64, device=dev)
    cells = torch.arange(16, device=dev)
    for rec in recs_rows:
        ca = codes(rec, a0, a0 + ac, kept).to(torch.int64)
        cb = codes(rec, b0, b0 + bc, kept).to(torch.int64)
        out += (4 * ca[:, None] + cb[None, :])[:, :, None] == cells
    return out.view(ac, bc, 4, 4)


def _int_array(x, what: str) -> np.ndarray:
    """``x`` as int64, after checking that it holds integers only (the exact comparisons rest on that)."""
    a = np.asarray(x)
    assert np.array_equal(a, np.rint(a)), f"{what} must be integers: the comparison is exact"
    return a.astype(np.int64)


def gram_ranges(recs_rows: Sequence[torch.Tensor], n: int, kept, tables, a_ranks, b_ranks) -> torch.Tensor:
    """(a_count, b_count) int64: entry [i, l] = the sum over the rows of ``recs_rows`` of t_j[x] * t_j[y], x and y the codes of rank
    a_begin + i and of rank b_begin + l in row j, t_j = ``tables[j]`` (the (V, 4) small integers of pgenhip_sample_gram, indexed by the
    row's position in ``recs_rows``).  ``a_ranks``, ``b_ranks``: (begin, count), small ranges of rows of any length."""
    dev = recs_rows[0].device
    kept = as_kept(kept, dev)
    t = torch.from_numpy(_int_array(tables, "tables").reshape(len(recs_rows), 4).copy()).to(dev)
    (a0, ac), (b0, bc) = a_ranks, b_ranks
    out = torch.zeros((ac, bc), dtype=torch.int64, device=dev)
    for j, rec in enumerate(recs_rows):
        za = t[j][codes(rec, a0, a0 + ac, kept).to(torch.int64)]
        zb = t[j][codes(rec, b0, b0 + bc, kept).to(torch.int64)]
        out += za[:, None] * zb[None, :]
    return out


def check_gram(got: torch.Tensor, want: torch.Tensor):
    """``got``: the (a_count, b_count) float64 entries pgenhip_sample_gram wrote (any row stride); ``want``: the int64 sums they must
    equal exactly.  -> None or (i, l, got, want) of the first wrong entry (NaN differs from everything)."""
    i = _first_diff(got, want.to(torch.float64))
    if i is None:
        return None
    bc = int(want.shape[1])
    return i // bc, i % bc, float(got[i // bc, i % bc]), int(want[i // bc, i % bc])


def check_variant_sums(sums: torch.Tensor, recs_rows: Sequence[torch.Tensor], n: int, kept, values, slab: int = SLAB):
    """``sums``: the V * C * 4 float64 values pgenhip_variant_sums wrote.  ``values``: (K, C) or (K,) small integers, one row per kept
    sample: a numpy array, or a tensor on the device of ``sums`` (an int64 tensor is used as it is, rows of any stride).  For every
    row, column and code the expected sum is formed in int64, slab by slab, as a masked sum of the values, so ``sums`` must equal it
    exactly as float64.  -> None or (row, column, code, got, want)."""
    dev = sums.device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    if isinstance(values, torch.Tensor):
        vals = values if values.dtype == torch.int64 else values.to(torch.int64)
        assert values.dtype == torch.int64 or bool((vals == values).all()), "values must be integers: the comparison is exact"
        vals = vals.to(dev)
    else:
        vals = torch.from_numpy(_int_array(values, "values").copy()).to(dev)
    if vals.dim() == 1:
        vals = vals[:, None]
    assert vals.shape[0] >= k
    c = int(vals.shape[1])
    v = len(recs_rows)
    want = torch.zeros((v, c, 4), dtype=torch.int64, device=dev)
    slab = max(1, min(slab, (1 << 26) // c))   # a slab of ranks holds C columns of int64, masked: bound its bytes
    for a, b in _slabs(k, slab):
        va = vals[a:b]
        for j, rec in enumerate(recs_rows):
            code = codes(rec, a, b, kept)
            for x in range(4):
                want[j, :, x] += torch.where((code == x)[:, None], va, 0).sum(dim=0)
    got = sums.reshape(-1)[: v * c * 4].view(v, c, 4)
    i = _first_diff(got, want.to(torch.float64))   # (NaN differs from everything, itself included)
    if i is None:
        return None
    return i // (4 * c), (i // 4) % c, i % 4, float(got.reshape(-1)[i]), int(want.reshape(-1)[i])


def _int_tensor(x, what: str, device) -> torch.Tensor:
    """``x`` (a numpy array, or a tensor with rows of any stride) as an int64 tensor on ``device``, after checking that it holds
    integers only."""
    if not isinstance(x, torch.Tensor):
        return torch.from_numpy(_int_array(x, what).copy()).to(device)
    xi = x if x.dtype == torch.int64 else x.to(torch.int64)
    assert x.dtype == torch.int64 or bool((xi == x).all()), f"{what} must be integers: the comparison is exact"
    return xi.to(device)


def apply_proj(recs_rows: Sequence[torch.Tensor], n: int, kept, tables, q, slab: int = SLAB) -> torch.Tensor:
    """(V, C) int64: P[j, c] = the sum over the kept ranks k of t_j[code of rank k in row j] * q[k, c], the P pass of
    pgenhip_gram_apply.  ``tables``: (V, 4) small integers by the row's position in ``recs_rows``; ``q``: (K, C) small integers, a
    numpy array or a tensor on the records' device with rows of any stride (the padded Q the call reads).  Summed over slabs of
    ranks; every partial sum is an integer below 2^52 (asserted from K and the largest |t| and |q|)."""
    dev = recs_rows[0].device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    v = len(recs_rows)
    t = _int_tensor(tables, "tables", dev).reshape(v, 4)
    if not isinstance(q, torch.Tensor):
        q = torch.from_numpy(np.asarray(q).copy()).to(dev)
    assert q.dim() == 2 and q.shape[0] == k
    c = int(q.shape[1])
    out = torch.zeros((v, c), dtype=torch.int64, device=dev)
    slab = max(1, min(slab, (1 << 26) // c))   # a slab of ranks holds C columns of int64: bound its bytes
    t_max, q_max = int(t.abs().max()) if v else 0, 0
    for a, b in _slabs(k, slab):
        qi = _int_tensor(q[a:b], "q", dev)
        q_max = max(q_max, int(qi.abs().max()))
        for j, rec in enumerate(recs_rows):
            z = t[j][codes(rec, a, b, kept).to(torch.int64)]
            out[j] += (z[:, None] * qi).sum(dim=0)
    assert k * t_max * q_max < 2 ** 52, "a partial sum of P may not be exact in float64"
    return out


def check_apply_out(out: torch.Tensor, recs_rows: Sequence[torch.Tensor], n: int, kept, tables, proj, slab: int = SLAB):
    """``out``: the (K, C) float64 view (rows of any stride) of what the Y pass of pgenhip_gram_apply wrote; ``proj``: the (V, C)
    integers it summed (apply_proj; twice them after an ACCUMULATE call on top: the sums are linear in proj).  want[k, c] = the sum
    over the rows j of t_j[code of rank k in row j] * proj[j, c] is formed in int64 slab by slab, so ``out`` must equal it exactly
    as float64.  -> None or (rank, column, got, want) of the first wrong entry (NaN differs from everything)."""
    dev = out.device
    kept = as_kept(kept, dev)
    k = kept_count(n, kept)
    v = len(recs_rows)
    t = _int_tensor(tables, "tables", dev).reshape(v, 4)
    p = _int_tensor(proj, "proj", dev)
    assert p.shape[0] == v and tuple(out.shape) == (k, p.shape[1])
    c = int(p.shape[1])
    if v:
        assert v * int(t.abs().max()) * int(p.abs().max()) < 2 ** 52, "a partial sum of Y may not be exact in float64"
    slab = max(1, min(slab, (1 << 26) // c))   # a slab of ranks holds C columns of int64 and of float64: bound its bytes
    for a, b in _slabs(k, slab):
        want = torch.zeros((b - a, c), dtype=torch.int64, device=dev)
        for j, rec in enumerate(recs_rows):
            z = t[j][codes(rec, a, b, kept).to(torch.int64)]
            want += z[:, None] * p[j][None, :]
        got = out[a:b]
        i = _first_diff(got, want.to(torch.float64))
        if i is not None:
            return a + i // c, i % c, float(got[i // c, i % c]), int(want[i // c, i % c])
    return None


# ---- periodic rows: a closed form for windows too wide to enumerate ------------------------------------------------------------------
PERIOD = 45   # shares no factor with the pair kernel's 16-row tile: every tile phase meets every row of the period


def periodic_tables(codes_p: np.ndarray) -> np.ndarray:
    """(P, P, 16) int64 from the (P, K) codes of the P distinct rows (pair_ref.table): the table of rows x and y."""
    import pair_ref as PR

    p = codes_p.shape[0]
    return np.stack([np.stack([PR.table(codes_p[x], codes_p[y]).reshape(16) for y in range(p)]) for x in range(p)])


def periodic_expected(tab: torch.Tensor, i0: int, i1: int, window: int, v: int, fill) -> torch.Tensor:
    """Entries [i0, i1) x [0, W) of pgenhip_pair_stats when selected row j is row j mod P: entry (i, d - 1) is ``tab[i % P, (i + d) % P]``
    (``tab``: (P, P, ...) on the device), and ``fill`` where i + d >= v (the library leaves those untouched)."""
    p = tab.shape[0]
    i = torch.arange(i0, i1, device=tab.device)[:, None]
    j = i + torch.arange(1, window + 1, device=tab.device)[None, :]
    want = tab[i % p, j % p]
    want[j >= v] = fill
    return want


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


def fill_periodic(dst: torch.Tensor, pattern: torch.Tensor):
    """dst[i] = pattern[i % len(pattern)] for a 1-D ``dst`` of any length, without a temporary of its size"""
    p = pattern.numel()
    whole = dst.numel() // p
    dst[: whole * p].view(whole, p).copy_(pattern[None, :].expand(whole, p))
    dst[whole * p:].copy_(pattern[: dst.numel() - whole * p])


def frame_ok(buf: torch.Tensor, front: int, nbytes: int) -> bool:
    return bool((buf[:front] == SENT).all()) and bool((buf[front + nbytes:] == SENT).all())
