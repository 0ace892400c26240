"""Genotype counts across the grid-stride loop of ``gt_count_kernel``.  ``launch_shape`` caps the grid at num_cus x kBlocksPerCu
blocks, so past S rows (the rows one grid covers, from count_plan.py and the device's CU count) every wave goes round
``r0 += n_waves * kRowsPerStep`` again.  Each executed shape runs V = S - 1, S, S + 1 and 2S + one block's rows + 3 (a third,
partial pass), for all samples, a random half (the kept-mask path) and the last sample alone, on four layouts of the same rows:
dense, strided from an odd base at an odd stride (all 16 alignments), a random row permutation through ``variant_idx`` and
shuffled byte offsets (``_at``).  Counts go to sentinel-framed output; the reference is the C oracle's literal loop."""
import numpy as np
import pytest
import torch

import count_plan as CP
import count_ref as CR
import pgen_rs_amd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEAD = 3                       # odd base of the strided layout
# (label, N, kernel): every class edge under AUTO, the first wave-per-row N, and both forced kernels off their AUTO class
# (neighbours share N: the records of one N are built once)
SHAPES = [("auto", 708, CP.AUTO), ("wave", 708, CP.WAVE_PER_ROW), ("auto", 1476, CP.AUTO), ("auto", 3012, CP.AUTO), ("auto", 6084, CP.AUTO),
          ("auto", 6085, CP.AUTO), ("rows", 6085, CP.ROWS_PER_WAVE)]
V_CASES = ["S-1", "S", "S+1", "2S+block+3"]
KEEPS = ["all", "half", "last"]


def num_cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def n_rows(case: str, g: int, ru: int, cus: int) -> int:
    s = CP.rows_per_grid(g, ru, cus)
    return {"S-1": s - 1, "S": s, "S+1": s + 1, "2S+block+3": 2 * s + CP.rows_per_block(g, ru) + 3}[case]


def odd_stride(r: int) -> int:
    """The smallest odd stride >= R + 5: coprime to 16, so consecutive rows start at every alignment."""
    return r + 5 if (r + 5) % 2 else r + 6


_CACHE = {}


def data_for(n: int):
    """Records, layouts and oracle counts of the largest V any cell of this N runs (smaller V are prefixes); one N held at a time."""
    if _CACHE.get("n") != n:
        _CACHE.clear()
        torch.cuda.empty_cache()
        cus = num_cus()
        v = max(n_rows("2S+block+3", *CP.shape(n, k)[:2], cus) for _, nn, k in SHAPES if nn == n)
        r = CP.record_size(n)
        stride = odd_stride(r)
        rng = np.random.default_rng(n)
        host = rng.integers(0, 256, size=(v, r), dtype=np.uint8)          # every byte random: pad bits dirty
        strided = np.zeros(LEAD + v * stride + 16, dtype=np.uint8)
        strided[LEAD: LEAD + v * stride].reshape(v, stride)[:, :r] = host
        kept = {"all": None, "half": np.sort(rng.choice(n, size=n // 2, replace=False)).astype(np.uint32),
                "last": np.array([n - 1], dtype=np.uint32)}
        with CR.pool() as ex:
            want = CR.oracle_counts_dense(host, n, kept, ex)
        perm = rng.permutation(v)
        order = rng.permutation(v)
        _CACHE.update(n=n, v=v, r=r, stride=stride, kept=kept, want=want, perm=perm, order=order,
                      d_dense=torch.from_numpy(host.reshape(-1)).to(DEV), d_strided=torch.from_numpy(strided).to(DEV),
                      d_perm=torch.from_numpy(perm.astype(np.int32)).to(DEV),
                      d_off=torch.from_numpy((LEAD + order.astype(np.int64) * stride)).to(DEV))
    return _CACHE


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", V_CASES)
@pytest.mark.parametrize("label,n,kern", SHAPES, ids=[f"{lab}-{n}" for lab, n, _ in SHAPES])
def test_grid_stride_edges(label, n, kern, case, keep):
    g, ru, _u = CP.shape(n, kern)
    cus = num_cus()
    s = CP.rows_per_grid(g, ru, cus)
    v = n_rows(case, g, ru, cus)
    d = data_for(n)
    assert v <= d["v"] and d["d_strided"].numel() < (110 << 20)     # a cell stays near 100 MB of records per layout
    want = d["want"][keep]
    stride = d["stride"]
    # the strided rows start at all 16 alignments (LEAD odd, stride odd)
    assert len({(LEAD + i * stride) % 16 for i in range(min(v, 16))}) == 16
    with pgen_rs_amd.GtEngine(n, kept_idx=d["kept"][keep], device=0) as eng:
        assert eng.kept_count == want[0].sum() and (keep == "all") == (eng.kept_count == n)   # half / last: the kept-mask path
        tag = f"N={n} {label} (G={g}, RU={ru}) V={v} ({case}, S={s}) keep={keep}"
        got = CR.guarded_counts(eng, kern, v, records=d["d_dense"])
        CR.assert_counts_equal(got, want[:v], f"dense, {tag}", s)
        got = CR.guarded_counts(eng, kern, v, records=d["d_strided"], record_stride=stride, records_offset=LEAD)
        CR.assert_counts_equal(got, want[:v], f"stride {stride} from byte {LEAD}, {tag}", s)
        got = CR.guarded_counts(eng, kern, v, records=d["d_dense"], variant_idx=d["d_perm"][:v])
        CR.assert_counts_equal(got, want[d["perm"][:v]], f"variant_idx permutation, {tag}", s)
        got = CR.guarded_counts(eng, kern, v, base=d["d_strided"], record_off=d["d_off"][:v])
        CR.assert_counts_equal(got, want[d["order"][:v]], f"shuffled _at offsets, {tag}", s)
