"""The slab-wise torch reference of the long-row GPU tests (longrow_ref.py) against the CPU oracle's GT text (pgen_oracle.decode_emit),
the oracle's counts (count_ref.py) and the numpy matrix reference (matrix_ref.py) — on the CPU, with a slab of 97 samples so that
slab seams fall inside record bytes, on records with dirty pad bits."""
import numpy as np
import pytest
import torch

import count_ref as CR
import longrow_ref as LR
import matrix_ref as MR
import pgen_oracle as oracle

SLAB = 97
N_LIST = [1, 5, 97, 1003, 70_001]
KEEPS = ["all", "first", "last", "p1", "p50"]
V = 3


def kept_of(n: int, keep: str):
    rng = np.random.default_rng(n * 13 + len(keep))
    if keep == "all":
        return None
    if keep == "first":
        return np.array([0], dtype=np.uint32)
    if keep == "last":
        return np.array([n - 1], dtype=np.uint32)
    k = max(1, n // 100) if keep == "p1" else max(1, n // 2)
    return np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint32)


def records(n: int):
    """(V, R) random bytes: the pad bits of every record's last byte are dirty whenever N is no multiple of 4."""
    rng = np.random.default_rng(n)
    recs = rng.integers(0, 256, size=(V, LR.rsize(n)), dtype=np.uint8)
    if n % 4:
        recs[:, -1] |= (0xFF << (2 * (n % 4))) & 0xFF
    return recs


CASES = [(n, keep) for n in N_LIST for keep in KEEPS]


@pytest.mark.parametrize("n,keep", CASES)
def test_codes_and_gt_text_equal_the_oracle(n, keep):
    kept = kept_of(n, keep)
    recs = records(n)
    k = LR.kept_count(n, kept)
    text = oracle.decode_emit(recs.reshape(-1), V, n, kept).reshape(V, 4 * k + 1)
    want_codes = MR.codes(recs, n, kept)
    for j in range(V):
        rec = torch.from_numpy(recs[j].copy())
        # codes over windows that start and end inside bytes
        for a, b in ((0, k), (k // 3, k - k // 5), (min(1, k), min(k, 98))):
            assert (LR.codes(rec, a, b, kept).numpy() == want_codes[j, a:b]).all()
        row = torch.from_numpy(text[j].copy())
        assert LR.check_gt_row(row, rec, n, kept, slab=SLAB) is None
        # every kind of damage is found, and at the right place
        for pos in sorted({0, 4 * (k // 2) + 1, 4 * k - 1, 4 * k}):
            bad = row.clone()
            bad[pos] ^= 1
            found = LR.check_gt_row(bad, rec, n, kept, slab=SLAB)
            assert found is not None and (found[0], found[1]) == (pos // 4, pos % 4), (pos, found)


@pytest.mark.parametrize("n,keep", CASES)
def test_row_counts_equal_the_oracle(n, keep):
    kept = kept_of(n, keep)
    recs = records(n)
    with CR.pool() as ex:
        want = CR.oracle_counts_dense(recs, n, {"k": kept}, ex)["k"]
    for j in range(V):
        assert LR.row_counts(torch.from_numpy(recs[j].copy()), n, kept, slab=SLAB) == want[j].tolist()


@pytest.mark.parametrize("n,keep", CASES)
def test_sample_counts_check(n, keep):
    kept = kept_of(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2]   # a gather that repeats a row
    c = MR.codes(recs[rows], n, kept)
    k = c.shape[1]
    for prefill in (0, 0xFFFFFFF0):
        want = (np.stack([(c == code).sum(axis=0) for code in range(4)], axis=1).astype(np.int64) + prefill) & 0xFFFFFFFF
        got = torch.from_numpy(want.astype(np.uint32).view(np.int32).reshape(-1).copy())
        recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
        assert LR.check_sample_counts(got, recs_rows, n, kept, prefill, slab=SLAB) is None
        for rank, code in {(0, 0), (k - 1, 3), (k // 2, 1)}:
            bad = got.clone()
            bad[4 * rank + code] += 1
            found = LR.check_sample_counts(bad, recs_rows, n, kept, prefill, slab=SLAB)
            assert found is not None and found[:2] == (rank, code), found


@pytest.mark.parametrize("n,keep", CASES)
@pytest.mark.parametrize("np_dtype", [np.int8, np.int16, np.float32])
@pytest.mark.parametrize("sample_major", [False, True])
def test_matrix_check(n, keep, np_dtype, sample_major):
    kept = kept_of(n, keep)
    recs = records(n)
    rows = [1, 0, 1]
    vals = MR.default_values(np_dtype)
    eb = vals.itemsize
    m = MR.raw(MR.matrix(recs[rows], n, kept, vals, sample_major))      # (rows, cols * eb) bytes
    nrow, row_bytes = m.shape
    pitch = row_bytes + 16
    buf = np.full(nrow * pitch, 0xA5, dtype=np.uint8)
    buf.reshape(nrow, pitch)[:, :row_bytes] = m
    out = torch.from_numpy(buf)
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    pat = vals.view(np.uint8)
    assert LR.check_matrix(out, recs_rows, n, kept, eb, pat, sample_major, pitch, slab=SLAB) is None
    assert LR.padding_untouched(out, nrow, row_bytes, pitch, 0xA5)
    k = LR.kept_count(n, kept)
    for j, rank in {(0, 0), (len(rows) - 1, k - 1), (1, k // 2)}:
        bad = out.clone()
        pos = (rank * pitch + j * eb) if sample_major else (j * pitch + rank * eb)
        bad[pos + eb - 1] ^= 0x40
        found = LR.check_matrix(bad, recs_rows, n, kept, eb, pat, sample_major, pitch, slab=SLAB)
        assert found is not None and found[:3] == (j, rank, eb - 1), found
    if nrow > 1:
        bad = out.clone()
        bad[row_bytes] = 0
        assert not LR.padding_untouched(bad, nrow, row_bytes, pitch, 0xA5)
