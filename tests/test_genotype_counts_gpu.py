"""Per-variant genotype counts — GPU leg (pgenhip_genotype_counts / _at through GtEngine): every forced shape and AUTO against
numpy (unpack the 2-bit codes, bincount the kept columns) and against the committed golden GT text, counted."""
import numpy as np
import pytest
import torch

import count_plan as CP
import pgen_rs_amd
from helpers import case_names, load_case
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = [_capi.COUNT_AUTO, _capi.COUNT_WAVE_PER_ROW, _capi.COUNT_ROWS_PER_WAVE]
SENT = -0x5A5A5A5B   # 0xA5A5A5A5 as int32


def rsize(n):
    return (2 * n + 7) // 8


def np_counts(recs: np.ndarray, n: int, kept=None) -> np.ndarray:
    """(V, R) uint8 records -> (V, 4) counts of codes 0..3 over the kept samples (pad bits ignored)."""
    v = recs.shape[0]
    codes = np.stack([(recs >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(v, -1)[:, :n]
    if kept is not None:
        codes = codes[:, np.asarray(kept, dtype=np.int64)]
    return np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.int64)


def gt_text_counts(gt: bytes, v: int) -> np.ndarray:
    rows = gt.split(b"\n")[:v]
    return np.array([[r.count(b"0/0"), r.count(b"0/1"), r.count(b"1/1"), r.count(b"./.")] for r in rows], dtype=np.int64).reshape(v, 4)


def kept_sets(n, rng):
    out = {"all": None, "k0": [], "first": [0], "last": [n - 1], "identity": list(range(n))}
    out["p1"] = sorted(rng.choice(n, size=max(1, n // 100), replace=False).tolist())
    out["p50"] = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    return out


def host_counts(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def run_counts(eng, kern, n_rows, **kw):
    """counts into a sentinel-guarded buffer at an odd 4-byte offset (and an aligned one); nothing else may change."""
    got = None
    for lead in (4, 1):
        buf = torch.full((lead + 4 * n_rows + 8,), SENT, dtype=torch.int32, device=DEV)
        out = buf[lead:]
        res = eng.genotype_counts(out=out, n_variants=n_rows, kernel=kern, **kw) if "base" not in kw else \
            eng.genotype_counts_at(kw["base"], kw["record_off"], n_rows, out=out, kernel=kern)
        eng.wait()
        h = buf.cpu().numpy()
        assert (h[:lead] == SENT).all() and (h[lead + 4 * n_rows:] == SENT).all(), f"kernel {kern} wrote outside its counts"
        assert res.shape == (n_rows, 4) and res.dtype == torch.int32
        g = host_counts(res)
        assert got is None or (g == got).all()
        got = g
    return got


@pytest.mark.parametrize("name", case_names())
def test_golden_cases_equal_counted_gt_text(name):
    v, n, recs, kept, gt = load_case(name)
    want = gt_text_counts(gt.tobytes(), v)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d = torch.from_numpy(recs.copy().reshape(-1)).to(DEV)
        for kern in KERNELS:
            got = host_counts(eng.genotype_counts(d, kernel=kern, n_variants=v))
            eng.wait()
            assert (got == want).all(), f"kernel {kern}"


# each shape threshold of the AUTO rule (lanes per row 4 / 8 / 16 / 32 / a wave) +- 1, from the launch plan's mirror: the last N
# of a class and the first of the next (708, 1476, 3012, 6084 today; test_count_plan.py pins them to gt_count.hip)
N_LIST = sorted({1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 257, 300, 2504, 500_000} | {n + d for n in CP.CLASS_EDGES for d in (0, 1)})


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("keep", ["all", "k0", "first", "last", "p1", "p50", "identity"])
def test_seeded_layouts_against_numpy(n, keep):
    rng = np.random.default_rng(n * 31 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = rsize(n)
    v = 5 if n >= 100_000 else 37
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    d_raw = torch.from_numpy(raw).to(DEV)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        want = np_counts(recs, n, kept)
        gather = np.array(sorted(rng.choice(v, size=v // 2 + 1, replace=False).tolist())[::-1], dtype=np.int32)   # descending: gathered
        d_gather = torch.from_numpy(gather).to(DEV)
        offs = np.array([3 + i * stride for i in gather], dtype=np.int64)
        d_offs = torch.from_numpy(offs).to(DEV)
        for kern in KERNELS:
            got = run_counts(eng, kern, v, records=d_raw, record_stride=stride, records_offset=3)
            assert (got == want).all(), f"strided, kernel {kern}"
            got = run_counts(eng, kern, len(gather), records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather)
            assert (got == want[gather]).all(), f"gathered, kernel {kern}"
            got = run_counts(eng, kern, len(gather), base=d_raw, record_off=d_offs)
            assert (got == want[gather]).all(), f"_at, kernel {kern}"
            # dense rows (stride R) from an odd base; a single row
            dense = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)])).to(DEV)
            got = run_counts(eng, kern, v, records=dense, records_offset=1)
            assert (got == want).all(), f"dense, kernel {kern}"
            got = run_counts(eng, kern, 1, records=dense, records_offset=1 + r * (v - 1))
            assert (got == want[-1:]).all(), f"one row, kernel {kern}"


# rows in which every sample has the same code: one category is K, the others 0, and with 0xFF the set pad bits are not counted
# (6 084 / 6 085: the last N of the 32-lanes class and the first that AUTO gives a wave per row)
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 300, 2504, 6084, 6085, 70_001])
@pytest.mark.parametrize("keep", ["all", "p50"])
def test_constant_rows(n, keep):
    rng = np.random.default_rng(n * 17 + len(keep))
    kept = kept_sets(n, rng)[keep]
    k = n if kept is None else len(kept)
    r, v = rsize(n), 9
    stride = r + 5
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for fill, code in ((0x55, 1), (0xAA, 2), (0xFF, 3), (0x00, 0)):
            # strided rows from byte 3, the bytes around them the opposite pattern
            raw = np.full(3 + v * stride, fill ^ 0xFF, dtype=np.uint8)
            raw[3:].reshape(v, stride)[:, :r] = fill
            want = np.zeros((v, 4), dtype=np.int64)
            want[:, code] = k
            assert (np_counts(np.full((v, r), fill, dtype=np.uint8), n, kept) == want).all()
            d_raw = torch.from_numpy(raw).to(DEV)
            for kern in KERNELS:
                got = run_counts(eng, kern, v, records=d_raw, record_stride=stride, records_offset=3)
                assert (got == want).all(), f"fill {fill:#04x}, kernel {kern}"


def test_n_variants_zero_is_a_no_op_and_bad_flags():
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        buf = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
        recs = torch.zeros(75, dtype=torch.uint8, device=DEV)
        for kern in KERNELS:
            assert eng.genotype_counts(recs, n_variants=0, out=buf, kernel=kern).shape == (0, 4)
            assert eng.genotype_counts_at(recs, torch.zeros(1, dtype=torch.int64, device=DEV), 0, out=buf, kernel=kern).shape == (0, 4)
        eng.wait()
        assert (buf.cpu().numpy() == SENT).all()
        with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
            eng.genotype_counts(recs, n_variants=1, kernel=7)
        assert ei.value.status == _capi.ERR_BAD_ARG
        lib, ctx = _capi.lib, eng._ctx
        assert lib.pgenhip_genotype_counts(ctx, None, 75, None, 1, buf.data_ptr(), 0) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_genotype_counts(ctx, recs.data_ptr(), 75, None, 1, None, 0) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_genotype_counts(ctx, recs.data_ptr(), 74, None, 2, buf.data_ptr(), 0) == _capi.ERR_BAD_ARG
        assert lib.pgenhip_genotype_counts_at(ctx, recs.data_ptr(), None, 1, buf.data_ptr(), 0) == _capi.ERR_BAD_ARG


@pytest.mark.parametrize("keep", [None, "p1"])
def test_hwe_records_at_configs2_row_length(keep):
    n, v = 500_000, 48
    kept = None if keep is None else np.arange(0, n, 100, dtype=np.uint32)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=1000, hwe=True)
        host = recs.cpu().numpy().reshape(v, -1)
        want = np_counts(host, n, kept)
        assert want[:, 1].sum() > 0 and want[:, 3].sum() > 0
        for kern in KERNELS:
            got = host_counts(eng.genotype_counts(recs, n_variants=v, kernel=kern))
            eng.wait()
            assert (got == want).all(), f"kernel {kern}"


def test_row_past_4_gib():
    """A record whose byte offset is past 4 GiB, through _at and through a variant index x stride: u64 addressing."""
    n = 2504
    r = rsize(n)
    far = (1 << 32) + 4099
    free, _total = torch.cuda.mem_get_info(0)
    need = far + 2 * r + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / 2**30:.0f} GiB of free HBM, have {free / 2**30:.0f}")
    rng = np.random.default_rng(4)
    rec = rng.integers(0, 256, size=r, dtype=np.uint8)
    big = torch.empty(far + 2 * r, dtype=torch.uint8, device=DEV)
    big[far: far + r] = torch.from_numpy(rec).to(DEV)
    kept = np.arange(1, n, 3, dtype=np.uint32)
    for kidx in (None, kept):
        want = np_counts(rec[None, :], n, kidx)
        with pgen_rs_amd.GtEngine(n, kept_idx=kidx, device=0) as eng:
            for kern in KERNELS:
                got = host_counts(eng.genotype_counts_at(big, torch.tensor([far], dtype=torch.int64, device=DEV), 1, kernel=kern))
                eng.wait()
                assert (got == want).all(), f"_at, kernel {kern}"
                # row index 1 at a stride of `far` bytes: offset = 1 * far > 4 GiB
                got = host_counts(eng.genotype_counts(big, record_stride=far, n_variants=1,
                                                      variant_idx=torch.tensor([1], dtype=torch.int32, device=DEV), kernel=kern))
                eng.wait()
                assert (got == want).all(), f"variant_idx x stride, kernel {kern}"
    del big
    torch.cuda.empty_cache()


def test_counts_follow_the_gt_text_of_decode_emit():
    """The counts of a row equal its GT fields as pgenhip_decode_emit writes them, counted."""
    n, v = 2504, 64
    kept = np.arange(3, n, 7, dtype=np.uint32)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=77, dirty_pad=True)
        text = eng.decode_emit(recs, v)
        got = host_counts(eng.genotype_counts(recs, n_variants=v))
        eng.wait()
        assert (got == gt_text_counts(text.cpu().numpy().tobytes(), v)).all()
