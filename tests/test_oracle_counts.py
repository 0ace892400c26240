"""CPU leg of the counting oracle (``pgo_genotype_counts[_at]``), the reference of every genotype-count test: on the golden
cases and on random strided, gathered and byte-offset layouts with kept lists it must equal two independent counts, numpy's
unpack + bincount and ``pgo_decode_emit``'s GT text counted.  No GPU, no product code."""
import numpy as np
import pytest
import torch

import count_ref as CR
import pgen_oracle as oracle
from helpers import case_names, load_case


def np_counts(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (V, 4) int64: unpack every 2-bit code, keep samples [0, n) (or the kept columns), bincount."""
    v = recs.shape[0]
    codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    out = np.zeros((v, 4), dtype=np.int64)
    for j in range(v):
        out[j] = np.bincount(codes[j], minlength=4)[:4]
    return out


def text_counts(gt: bytes, v: int) -> np.ndarray:
    rows = gt.split(b"\n")[:v]
    assert len(rows) == v
    return np.array([[r.count(b"\t0/0"), r.count(b"\t0/1"), r.count(b"\t1/1"), r.count(b"\t./.")] for r in rows], dtype=np.int64).reshape(v, 4)


def test_truth_table_e4():
    assert oracle.genotype_counts(np.array([0xE4], dtype=np.uint8), 1, 4).tolist() == [[1, 1, 1, 1]]
    assert oracle.genotype_counts(np.array([0xE4], dtype=np.uint8), 1, 3).tolist() == [[1, 1, 1, 0]]   # pad code not counted
    assert oracle.genotype_counts(np.array([0xE4], dtype=np.uint8), 1, 4, kept_idx=[3, 3, 1]).tolist() == [[0, 1, 0, 2]]


@pytest.mark.parametrize("name", case_names())
def test_golden_case_counts(name):
    v, n, recs, kept, gt = load_case(name)
    got = oracle.genotype_counts(recs.reshape(-1), v, n, kept_idx=kept)
    assert got.dtype == np.int64 and got.shape == (v, 4)
    assert (got == text_counts(gt.tobytes(), v)).all()
    assert (got == np_counts(recs, n, kept)).all()
    k = n if kept is None else len(kept)
    assert (got.sum(axis=1) == k).all()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 255, 709, 2504])
@pytest.mark.parametrize("keep", ["all", "half", "last", "repeat"])
def test_random_layouts_against_numpy_and_decode_emit(n, keep):
    rng = np.random.default_rng(1000 * n + len(keep))
    r = oracle.variant_record_size(n)
    v = 23
    kept = {"all": None, "half": np.sort(rng.choice(n, size=max(1, n // 2), replace=False)), "last": [n - 1],
            "repeat": rng.integers(0, n, size=2 * n + 1)}[keep]
    stride, lead = r + 5, 3
    raw = rng.integers(0, 256, size=lead + v * stride + 7, dtype=np.uint8)   # every byte random: pad bits dirty
    recs = np.stack([raw[lead + i * stride: lead + i * stride + r] for i in range(v)])
    want = np_counts(recs, n, kept)
    text = oracle.decode_emit(raw, v, n, kept_idx=kept, record_stride=stride, records_offset=lead).tobytes()
    assert (text_counts(text, v) == want).all()
    # strided from an odd base
    assert (oracle.genotype_counts(raw, v, n, kept_idx=kept, record_stride=stride, records_offset=lead) == want).all()
    # gathered: repeats, descending, through a variant index
    vidx = np.array([v - 1, 0, 5, 5, 11, 2], dtype=np.uint32)
    got = oracle.genotype_counts(raw, len(vidx), n, kept_idx=kept, record_stride=stride, variant_idx=vidx, records_offset=lead)
    assert (got == want[vidx]).all()
    # byte offsets (_at), shuffled
    order = rng.permutation(v)
    offs = np.array([lead + i * stride for i in order], dtype=np.uint64)
    assert (oracle.genotype_counts_at(raw, offs, n, kept_idx=kept) == want[order]).all()
    at_text = oracle.decode_emit_at(raw, offs, n, kept_idx=kept).tobytes()
    assert (text_counts(at_text, v) == want[order]).all()
    # dense
    assert (oracle.genotype_counts(recs.reshape(-1), v, n, kept_idx=kept) == want).all()


def test_hwe_rows_at_configs2_length():
    n, v = 500_000, 3
    recs = oracle.synth_records(n, v, first_variant=77, hwe=True)
    kept = np.arange(0, n, 100, dtype=np.uint32)
    for k in (None, kept):
        got = oracle.genotype_counts(recs, v, n, kept_idx=k)
        assert (got == np_counts(recs.reshape(v, -1), n, k)).all()
        assert (got[:, 1] > 0).all() and (got[:, 3] > 0).all()


def test_errors():
    with pytest.raises(IndexError):
        oracle.genotype_counts(np.zeros(2, dtype=np.uint8), 1, 5, kept_idx=[5])
    with pytest.raises(IndexError):
        oracle.genotype_counts_at(np.zeros(2, dtype=np.uint8), [0], 5, kept_idx=[1, 5])
    with pytest.raises(ValueError):
        oracle.genotype_counts(np.zeros(2, dtype=np.uint8), 2, 5)   # second row past the end
    with pytest.raises(ValueError):
        oracle.genotype_counts_at(np.zeros(4, dtype=np.uint8), [3], 5)
    assert oracle.genotype_counts(np.zeros(1, dtype=np.uint8), 0, 5).shape == (0, 4)


def test_chunked_pooled_reference_equals_one_call(monkeypatch):
    """count_ref's chunked copy-back + thread-pool split (the reference of the full-size GPU tests) covers every row once, in
    order, for every kept set: run here on a CPU tensor with chunks and pieces that do not divide the rows."""
    n, v = 2504, 1001
    r = oracle.variant_record_size(n)
    recs = oracle.synth_records(n, v, hwe=True)
    monkeypatch.setattr(CR, "CHUNK_BYTES", 37 * r + 5)
    kept = {"all": None, "p": oracle.synth_keep(n, modulus=7)}
    with CR.pool() as ex:
        got = CR.oracle_counts_device(torch.from_numpy(recs), v, n, kept, ex)
        got2 = CR.oracle_counts_dense(recs.reshape(v, r), n, kept, ex)
    for key, k in kept.items():
        want = oracle.genotype_counts(recs, v, n, kept_idx=k)
        assert (got[key] == want).all() and (got2[key] == want).all()
    bad = want.copy()
    bad[600, 1] += 1
    with pytest.raises(AssertionError, match="first row 600 .*grid pass 2, row 88 of it"):
        CR.assert_counts_equal(bad, want, "x", rows_per_grid=256)
