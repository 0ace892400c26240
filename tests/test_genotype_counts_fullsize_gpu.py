"""Genotype counts at the measured shapes, full size: the four shapes of tools/count_bench.py (configs[2] 100 000 x 500 000, the
c5shard 1 % subset of it with count_bench's RNG, the chr22 shape 1 103 547 x 2 504 and basic2's 9 200 000 x 300) plus
configs[2] with K = N - 1 (the kept-mask path at full row length), on the HWE records count_bench times, through AUTO and
both forced kernels.  configs[2] also runs a random permutation of all rows through ``variant_idx`` and the rows in reverse
through ``_at`` offsets.  These are the shapes that reach the grid-stride loop many times over and, at configs[2], dense row
addresses past 4 GiB (from row 34 360 on).

The reference: the device records copied back in chunks and counted by the C oracle's literal per-sample loop on a pool of
count_ref.THREADS threads; the comparison is exact over every row."""
import numpy as np
import pytest
import torch

import count_plan as CP
import count_ref as CR
import pgen_rs_amd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = {"auto": CP.AUTO, "wave": CP.WAVE_PER_ROW, "rows": CP.ROWS_PER_WAVE}
# name -> (variants, samples, kept set); records of one (variants, samples) are shared
CASES = {
    "configs2": (100_000, 500_000, "all"),
    "configs2_k_n_minus_1": (100_000, 500_000, "n_minus_1"),
    "c5shard": (125_000, 500_000, "p1"),
    "chr22": (1_103_547, 2_504, "all"),
    "basic2": (9_200_000, 300, "all"),
}


def kept_set(n: int, key: str):
    if key == "all":
        return None
    if key == "p1":   # tools/count_bench.py's c5shard subset: 1 % of the samples, default_rng(5)
        rng = np.random.default_rng(5)
        return np.sort(rng.choice(n, size=int(n * 0.01), replace=False)).astype(np.uint32)
    drop = int(np.random.default_rng(7).integers(n))   # every sample but one, seeded
    return np.delete(np.arange(n, dtype=np.uint32), drop)


_CACHE = {}


def records_for(v: int, n: int):
    """HWE records of count_bench's shape on the device and the oracle's counts for every kept set used with them."""
    if _CACHE.get("shape") != (v, n):
        _CACHE.clear()
        torch.cuda.empty_cache()
        r = CP.record_size(n)
        free, _total = torch.cuda.mem_get_info(0)
        need = v * r + 64 * v + (1 << 30)
        if free < need:
            pytest.skip(f"needs {need / 2**30:.1f} GiB of free HBM, have {free / 2**30:.1f}")
        keys = sorted({k for vv, nn, k in CASES.values() if (vv, nn) == (v, n)})
        kept = {k: kept_set(n, k) for k in keys}
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            recs = eng.synth_records(v, hwe=True)
            eng.wait()
        with CR.pool() as ex:
            want = CR.oracle_counts_device(recs, v, n, kept, ex)
        _CACHE.update(shape=(v, n), recs=recs, kept=kept, want=want)
    return _CACHE


@pytest.mark.parametrize("kname", list(KERNELS))
@pytest.mark.parametrize("key", ["all", "n_minus_1"])
def test_configs2_permuted_rows_and_reversed_offsets(key, kname):
    """(first in the module: the configs2 records and references are then reused by the dense configs2 cells)"""
    v, n = 100_000, 500_000
    d = records_for(v, n)
    want = d["want"][key]
    r = CP.record_size(n)
    perm = np.random.default_rng(11).permutation(v)
    rev = np.arange(v - 1, -1, -1, dtype=np.int64)
    with pgen_rs_amd.GtEngine(n, kept_idx=d["kept"][key], device=0) as eng:
        got = CR.guarded_counts(eng, KERNELS[kname], v, records=d["recs"], variant_idx=torch.from_numpy(perm.astype(np.int32)).to(DEV))
        CR.assert_counts_equal(got, want[perm], f"configs2 keep={key}, variant_idx permutation, kernel {kname}")
        got = CR.guarded_counts(eng, KERNELS[kname], v, base=d["recs"], record_off=torch.from_numpy(rev * r).to(DEV))
        CR.assert_counts_equal(got, want[rev], f"configs2 keep={key}, reversed _at offsets, kernel {kname}")


@pytest.mark.parametrize("kname", list(KERNELS))
@pytest.mark.parametrize("case", list(CASES))
def test_measured_shape_full_size(case, kname):
    v, n, key = CASES[case]
    d = records_for(v, n)
    want = d["want"][key]
    g, ru, _u = CP.shape(n, KERNELS[kname])
    s = CP.rows_per_grid(g, ru, torch.cuda.get_device_properties(0).multi_processor_count)
    with pgen_rs_amd.GtEngine(n, kept_idx=d["kept"][key], device=0) as eng:
        assert eng.kept_count == want[0].sum()
        got = CR.guarded_counts(eng, KERNELS[kname], v, records=d["recs"])
    CR.assert_counts_equal(got, want, f"{case} ({v} x {n}, K = {want[0].sum()}), kernel {kname} (G={g}, RU={ru}, S={s})", s)
