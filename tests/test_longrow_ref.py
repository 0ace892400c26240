"""The slab-wise torch reference of the long-row GPU tests (longrow_ref.py) against the CPU oracle's GT text (pgen_oracle.decode_emit),
the oracle's counts (count_ref.py) and the numpy references (matrix_ref.py, pack_ref.py, score_ref.py, pair_ref.py, spair_ref.py,
gram_ref.py, vsum_ref.py, gapply_ref.py) — on the CPU, with a slab of 97 samples so that slab seams fall inside record bytes, on records with dirty
pad bits."""
import numpy as np
import pytest
import torch

import count_ref as CR
import gapply_ref as AR
import gram_ref as GR
import longrow_ref as LR
import matrix_ref as MR
import pack_ref as PK
import pair_ref as PR
import pgen_oracle as oracle
import score_ref as SCR
import spair_ref as SPR
import vsum_ref as VR

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


# ---- packed rows, scores, pair tables, r^2, sample-pair tables: against pack_ref, score_ref, pair_ref and spair_ref -------------------
@pytest.mark.parametrize("n,keep", CASES)
@pytest.mark.parametrize("map4", [None, (3, 2, 1, 0), PK.BED_MAP], ids=["identity", "reversed", "bed"])
def test_packed_check(n, keep, map4):
    kept = kept_of(n, keep)
    recs = records(n)
    k = LR.kept_count(n, kept)
    want = PK.pack(recs, n, kept, map4)
    for j in range(V):
        rec, row = torch.from_numpy(recs[j].copy()), torch.from_numpy(want[j].copy())
        assert LR.check_packed(row, rec, n, kept, map4, slab=SLAB) is None
        for rank in sorted({0, k // 2, k - 1}):
            bad = row.clone()
            bad[rank >> 2] ^= 1 << (2 * (rank & 3))
            found = LR.check_packed(bad, rec, n, kept, map4, slab=SLAB)
            assert found is not None and found[0] == rank, (rank, found)
        if k % 4:
            bad = row.clone()
            bad[-1] |= 0x80
            assert LR.check_packed(bad, rec, n, kept, map4, slab=SLAB) == (k, 0x80 >> (2 * (k % 4)), 0)


def test_fill_periodic():
    pattern = torch.arange(7, dtype=torch.int32) + 100
    for n in (0, 3, 7, 8, 20, 21, 1000):
        dst = torch.full((n,), -1, dtype=torch.int32)
        LR.fill_periodic(dst, pattern)
        assert dst.tolist() == [100 + i % 7 for i in range(n)]


JOINS = [(3, 5), (97, 1, 96), (1, 400), (63, 64, 65, 2), (84, 85, 0, 87, 84, 90, 99, 101)]


@pytest.mark.parametrize("sizes", JOINS, ids=lambda s: "x".join(map(str, s)))
def test_joined_check(sizes):
    """check_joined against join_ref.join (sources with dirty pad bits at odd addresses): plain, flipped and absent parts agree;
    a wrong sample on either side of every seam, a set pad bit and a wrong last byte are each reported where they were planted."""
    import join_ref as JR

    n = sum(sizes)
    starts = [sum(sizes[:p]) for p in range(len(sizes))]
    rng = np.random.default_rng(n)
    v = 3
    parts = []
    for cnt in sizes:
        r = (cnt + 3) // 4
        base = rng.integers(0, 256, size=1 + v * (r + 2), dtype=np.uint8)   # random bytes: the pad bits are dirty
        parts.append([base, np.array([1 + j * (r + 2) for j in range(v)], dtype=np.int64), cnt,
                      np.array([0, 1, 0], dtype=np.uint8) if len(parts) % 2 else np.array([0, 0, 1], dtype=np.uint8)])
    parts[len(sizes) // 2][1][2] = JR.ABSENT
    want = JR.join([tuple(p) for p in parts], v)
    for j in range(v):
        row = torch.from_numpy(want[j].copy())
        rows = [torch.from_numpy(b[int(o[j]):].copy()) if o[j] != JR.ABSENT else None for b, o, _, _ in parts]
        flips = [bool(f[j]) for _, _, _, f in parts]
        absent = [r is None for r in rows]
        assert any(flips) or j == 0
        assert absent == [j == 2 and p == len(sizes) // 2 for p in range(len(sizes))]
        args = (rows, starts, list(sizes), flips, absent, n)
        assert LR.check_joined(row, *args, slab=SLAB) is None
        if any(f and c >= 60 and not a for f, c, a in zip(flips, sizes, absent)):   # 60 random codes hold a 0 or a 2
            assert LR.check_joined(row, rows, starts, list(sizes), [False] * len(sizes), absent, n, slab=SLAB) is not None
        seams = {s for p, s in enumerate(starts) if sizes[p]} | {s - 1 for s in starts if s} | {0, n - 1, SLAB - 1, SLAB}
        for sample in sorted(s for s in seams if 0 <= s < n):
            bad = row.clone()
            bad[sample >> 2] ^= 1 << (2 * (sample & 3))
            found = LR.check_joined(bad, *args, slab=SLAB)
            assert found is not None and found[0] == sample and found[1] == found[2] ^ 1, (sample, found)
        bad = row.clone()
        bad[-1] ^= 0x02                                                  # the last byte's first sample: always a real one
        found = LR.check_joined(bad, *args, slab=SLAB)
        assert found is not None and found[0] >> 2 == (n - 1) >> 2
        if n % 4:
            bad = row.clone()
            bad[-1] |= 0x80
            assert LR.check_joined(bad, *args, slab=SLAB) == (n, 0x80 >> (2 * (n % 4)), 0)


@pytest.mark.parametrize("n,keep", CASES)
@pytest.mark.parametrize("c", [1, 3, 8])
def test_scores_check(n, keep, c):
    kept = kept_of(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2]   # a gather that repeats a row
    k = LR.kept_count(n, kept)
    rng = np.random.default_rng(n + c)
    weights = rng.integers(-8, 9, size=(len(rows), c))
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    for miss, prefill in ((None, 0), (rng.integers(0, 4, size=len(rows)), 0), (rng.integers(0, 4, size=len(rows)), -37)):
        want = SCR.score_ref(recs[rows], n, weights.astype(np.float32), None if miss is None else miss.astype(np.float32), kept)[0] + prefill
        got = torch.from_numpy(want.reshape(-1).copy())
        assert LR.check_scores(got, recs_rows, n, kept, weights, miss, prefill, slab=SLAB) is None
        for rank, col in {(0, 0), (k - 1, c - 1), (k // 2, c // 2)}:
            bad = got.clone()
            bad[rank * c + col] += 1.0
            found = LR.check_scores(bad, recs_rows, n, kept, weights, miss, prefill, slab=SLAB)
            assert found is not None and found[:2] == (rank, col), found
        bad = got.clone()
        bad[0] = float("nan")
        assert LR.check_scores(bad, recs_rows, n, kept, weights, miss, prefill, slab=SLAB)[:2] == (0, 0)


def same_f32(a, b) -> bool:
    return (np.isnan(a) and np.isnan(b)) or np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


@pytest.mark.parametrize("n,keep", CASES)
def test_pair_table_and_r2(n, keep):
    kept = kept_of(n, keep)
    recs = records(n)
    codes = PR.unpack(recs, n, kept)
    for i, j in ((0, 1), (1, 2), (2, 2), (2, 0)):
        t = LR.pair_table(torch.from_numpy(recs[i].copy()), torch.from_numpy(recs[j].copy()), n, kept, slab=SLAB)
        want = PR.table(codes[i], codes[j])
        assert t == want.tolist()
        assert all(isinstance(x, int) for row in t for x in row)
        assert same_f32(LR.r2_of_table(t), PR.r2_f32(want)), (t, LR.r2_of_table(t), PR.r2_f32(want))


def test_r2_of_table_extremes():
    """Tables whose terms sit just below 2^64 (K = 2^31 - 1, nearly every sample hom-alt in both rows), monomorphic rows, an empty
    table, perfect correlation, and seeded tables of every size: the same float32 bits as pair_ref's once-rounded fraction."""
    big = (1 << 31) - 1
    tables = [[[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, big, 0], [0, 0, 0, 0]],                       # monomorphic: NaN
              [[0] * 4] * 4,                                                                  # empty: NaN
              [[0, 0, 0, 0], [0, 1, 0, 0], [1, 1, big - 3, 0], [0, 0, 0, 0]],                 # n Sxx and Sx^2 within 2^35 of 2^64
              [[3, 0, 0, 0], [0, 0, 2, 0], [0, 5, big - 10, 0], [0, 0, 0, 0]],
              [[5, 0, 0, 0], [0, 7, 0, 0], [0, 0, 9, 0], [0, 0, 0, 4]],                         # r^2 = 1
              [[1, 1, 1, 9], [1, 1, 1, 9], [1, 1, 1, 9], [9, 9, 9, 9]]]                         # cov = 0: r^2 = 0
    rng = np.random.default_rng(16)
    for bits in (3, 8, 16, 24, 29):
        tables += [rng.integers(0, 1 << bits, size=(4, 4)).tolist() for _ in range(40)]
    for t in tables:
        got, want = LR.r2_of_table(t), PR.r2_f32(np.asarray(t, dtype=object))
        assert same_f32(got, want), (t, got, want)
    assert np.isnan(LR.r2_of_table(tables[0])) and LR.r2_of_table(tables[4]) == np.float32(1.0) and LR.r2_of_table(tables[5]) == 0.0
    t = tables[2]
    n, sx, sxx = big, 2 * (big - 1) + 1, 4 * (big - 1) + 1   # row x: one het, hom-alt elsewhere
    assert 0 < (1 << 64) - n * sxx < 1 << 35 and 0 < (1 << 64) - sx * sx < 1 << 35 and n * sxx > sx * sx


@pytest.mark.parametrize("n,keep", CASES)
def test_sample_pair_tables(n, keep):
    kept = kept_of(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2, 0]
    k = LR.kept_count(n, kept)
    codes = SPR.unpack(recs[rows], n, kept)
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    for a, b in (((0, min(k, 70)), (max(0, k - 33), min(k, 33))), ((k - 1, 1), (0, min(k, 5))), ((k // 3, min(7, k - k // 3)), (k // 3, min(7, k - k // 3)))):
        got = LR.sample_pair_tables(recs_rows, n, kept, a, b)
        assert got.dtype == torch.int64 and (got.numpy() == SPR.ranges(codes, a, b)).all()


@pytest.mark.parametrize("v,w", [(2, 1), (46, 45), (100, 1), (100, 7), (137, 50), (137, 136), (137, 200)])
def test_periodic_closed_form(v, w):
    """Selected row j = row j mod 45 of 45 distinct records: the closed form equals pair_ref on the V gathered rows, and entries with
    i + d >= V hold the fill."""
    n, p = 11, LR.PERIOD
    kept = np.array([0, 1, 3, 4, 6, 9, 10], dtype=np.uint32)
    recs = np.random.default_rng(45).integers(0, 256, size=(p, LR.rsize(n)), dtype=np.uint8)
    codes_p = PR.unpack(recs, n, kept)
    assert len({c.tobytes() for c in codes_p}) == p
    tab = torch.from_numpy(LR.periodic_tables(codes_p))
    codes = codes_p[np.arange(v) % p]
    for n_left in (v, v - 1, max(1, v // 2)):
        want = PR.pair_tables(codes, n_left, w, fill=-1).reshape(n_left, w, 16)
        for i0, i1 in ((0, n_left), (n_left // 3, n_left - n_left // 4)):
            got = LR.periodic_expected(tab, i0, i1, w, v, -1)
            assert (got.numpy() == want[i0:i1]).all()
    r2 = torch.from_numpy(np.array([[PR.r2_f32(t.reshape(4, 4)) for t in row] for row in tab.numpy()], dtype=np.float32).view(np.int32).copy())
    want = PR.pair_r2(PR.pair_tables(codes, v, w, fill=-1), v, fill=np.float32(0)).view(np.int32)
    got = LR.periodic_expected(r2, 0, v, w, v, 0).numpy()
    assert (got == want).all()


# ---- Gram ranges and per-variant sums: against gram_ref and vsum_ref ------------------------------------------------------------------
SUMS_N = [5, 63, 300, 2504]
SUMS_KEEPS = ["all", "sparse", "every7"]


def sums_kept(n: int, keep: str):
    if keep == "all":
        return None
    if keep == "sparse":
        return np.unique(np.linspace(0, n - 1, min(n, 9)).astype(np.int64)).astype(np.uint32)   # samples 0 and N - 1 among them
    return np.arange(0, n, 7, dtype=np.uint32)


@pytest.mark.parametrize("keep", SUMS_KEEPS)
@pytest.mark.parametrize("n", SUMS_N)
def test_gram_ranges(n, keep):
    """gram_ranges equals gram_ref.gram_ref on ranges that begin and end inside record bytes, on a gather that repeats a row (the
    tables go with the position), and check_gram names a single planted wrong entry."""
    kept = sums_kept(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2, 0]
    k = LR.kept_count(n, kept)
    tables = np.random.default_rng(n + len(keep)).integers(-8, 9, size=(len(rows), 4)).astype(np.float64)
    codes = GR.unpack(recs[rows], n, kept)
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    for a, b in (((0, min(k, 70)), (max(0, k - 33), min(k, 33))), ((k - 1, 1), (0, min(k, 5))), ((k // 3, min(7, k - k // 3)), (k // 3, min(7, k - k // 3))),
                 ((min(1, k - 1), min(k - min(1, k - 1), 67)), (0, k))):
        want = GR.gram_ref(codes[:, a[0]:a[0] + a[1]], tables, codes[:, b[0]:b[0] + b[1]])
        got = LR.gram_ranges(recs_rows, n, kept, tables, a, b)
        assert got.dtype == torch.int64 and got.shape == (a[1], b[1]) and np.array_equal(got.numpy().astype(np.float64), want)
        out = torch.full((a[1], b[1] + 3), -1.5, dtype=torch.float64)[:, :b[1]]   # a padded pitch, as the GPU tests have
        out.copy_(torch.from_numpy(want))
        assert LR.check_gram(out, got) is None
        for i, l in {(0, 0), (a[1] - 1, b[1] - 1), (a[1] // 2, b[1] // 3)}:
            bad = out.clone()
            bad[i, l] += 1.0
            found = LR.check_gram(bad, got)
            assert found is not None and found[:2] == (i, l) and found[2] == found[3] + 1, found
        bad = out.clone()
        bad[0, 0] = float("nan")
        assert LR.check_gram(bad, got)[:2] == (0, 0)


@pytest.mark.parametrize("slab", [7, SLAB])
@pytest.mark.parametrize("c", [1, 3, 16])
@pytest.mark.parametrize("keep", SUMS_KEEPS)
@pytest.mark.parametrize("n", SUMS_N)
def test_variant_sums_check(n, keep, c, slab):
    """check_variant_sums accepts vsum_ref.vsum_ref's sums with slabs of 7 and 97 ranks (seams inside record bytes), values given as a
    numpy array, as an int64 tensor and (C = 3) as a view of 16-wide rows, and names a single planted wrong entry."""
    kept = sums_kept(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2]   # a gather that repeats a row
    k = LR.kept_count(n, kept)
    v16 = np.random.default_rng(n + c).integers(-8, 9, size=(k, 16))
    vals = v16[:, :c]
    want, _ = VR.vsum_ref(recs[rows], n, vals.astype(np.float64), kept)
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    got = torch.from_numpy(want.reshape(-1).copy())
    assert LR.check_variant_sums(got, recs_rows, n, kept, vals.astype(np.float64), slab=slab) is None
    t_vals = torch.from_numpy(v16.astype(np.int64))[:, :c]
    assert t_vals.stride(0) == 16
    assert LR.check_variant_sums(got.view(len(rows), c, 4), recs_rows, n, kept, t_vals[:, 0] if c == 1 else t_vals, slab=slab) is None
    for row, col, code in {(0, 0, 0), (len(rows) - 1, c - 1, 3), (1, c // 2, 2)}:
        bad = got.clone()
        bad[(row * c + col) * 4 + code] += 1.0
        found = LR.check_variant_sums(bad, recs_rows, n, kept, t_vals, slab=slab)
        assert found is not None and found[:3] == (row, col, code) and found[3] == found[4] + 1, found
    bad = got.clone()
    bad[0] = float("nan")
    assert LR.check_variant_sums(bad, recs_rows, n, kept, t_vals, slab=slab)[:3] == (0, 0, 0)


# ---- the Gram product's two passes: against gapply_ref ----------------------------------------------------------------------------------
APPLY_N = [5, 63, 128, 301]   # 128: slabs of 64 ranks end on the data's last rank; the others are no multiple of 4


@pytest.mark.parametrize("slab", [1, 7, 64])
@pytest.mark.parametrize("c", [1, 3, 16])
@pytest.mark.parametrize("keep", SUMS_KEEPS)
@pytest.mark.parametrize("n", APPLY_N)
def test_apply_proj_and_check_apply_out(n, keep, c, slab):
    """apply_proj equals gapply_ref.apply_int's P, and check_apply_out accepts its Y, with slabs of 1, 7 and 64 ranks (seams inside
    record bytes, between them and on the last rank), on a gather that repeats a row (the tables go with the position), with Q and
    the output as views of wider rows; twice proj goes with twice Y; a single planted wrong entry is named."""
    kept = sums_kept(n, keep)
    recs = records(n)
    rows = [0, 2, 1, 2, 0]
    k = LR.kept_count(n, kept)
    rng = np.random.default_rng(n + c + len(keep))
    tables = rng.integers(-8, 9, size=(len(rows), 4)).astype(np.float64)
    q = rng.integers(-4, 5, size=(k, c)).astype(np.float64)
    wp, wy = AR.apply_int(AR.unpack(recs[rows], n, kept), tables, q)
    recs_rows = [torch.from_numpy(recs[j].copy()) for j in rows]
    q_wide = torch.full((k, c + 3), -1.5, dtype=torch.float64)
    q_wide[:, :c] = torch.from_numpy(q)
    for q_arg in (q, q_wide[:, :c]):
        proj = LR.apply_proj(recs_rows, n, kept, tables, q_arg, slab=slab)
        assert proj.dtype == torch.int64 and proj.shape == (len(rows), c) and np.array_equal(proj.numpy(), wp)
    out = torch.full((k, c + 3), -1.5, dtype=torch.float64)[:, :c]   # a padded pitch, as the GPU tests have
    out.copy_(torch.from_numpy(wy.astype(np.float64)))
    assert LR.check_apply_out(out, recs_rows, n, kept, tables, proj, slab=slab) is None
    assert LR.check_apply_out(out, recs_rows, n, kept, tables, wp.astype(np.float64), slab=slab) is None
    assert LR.check_apply_out(2.0 * out, recs_rows, n, kept, tables, 2 * proj, slab=slab) is None
    for rank, col in {(0, 0), (k - 1, c - 1), (k // 2, c // 2)}:
        bad = out.clone()
        bad[rank, col] += 1.0
        found = LR.check_apply_out(bad, recs_rows, n, kept, tables, proj, slab=slab)
        assert found is not None and found[:2] == (rank, col) and found[2] == found[3] + 1 == wy[rank, col] + 1, found
    bad = out.clone()
    bad[0, 0] = float("nan")
    assert LR.check_apply_out(bad, recs_rows, n, kept, tables, proj, slab=slab)[:2] == (0, 0)
