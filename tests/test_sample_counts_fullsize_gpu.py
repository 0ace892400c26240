"""Per-sample genotype counts at the measured shapes, full size: the four shapes of tools/scount_bench.py (configs[2] 100 000 x
500 000, the c5shard 1 % subset with count_bench's RNG, the chr22 shape 1 103 547 x 2 504 and basic2's 9 200 000 x 300) plus
configs[2] with K = N - 1, on the HWE records the tools time, through AUTO and every forced shape.  These are the launches with
many flush windows per slot, every column tile of a 500 000-sample row and dense row addresses past 4 GiB.

Two references, neither through the HIP kernels: the records unpacked and summed over rows chunk by chunk by torch on the device
(int64), and numpy on 256 seeded columns gathered back to the host."""
import numpy as np
import pytest
import torch

import pgen_rs_amd
import scount_plan as SP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = {"auto": SP.AUTO, "rows": SP.ROWS}
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


def torch_counts(recs: torch.Tensor, v: int, n: int) -> torch.Tensor:
    """(N, 4) int64 counts of every sample over the V dense rows: unpacked and summed by torch, a chunk of rows at a time."""
    r = SP.record_size(n)
    out = torch.zeros((n, 4), dtype=torch.int64, device=recs.device)
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=recs.device)
    rows = max(1, (128 << 20) // (4 * r))
    for a in range(0, v, rows):
        b = min(v, a + rows)
        codes = ((recs[a * r: b * r].view(b - a, r, 1) >> shifts) & 3).view(b - a, 4 * r)[:, :n]
        for c in range(4):
            out[:, c] += (codes == c).sum(dim=0, dtype=torch.int64)
    return out


def numpy_columns(recs: torch.Tensor, v: int, n: int, samples: np.ndarray) -> np.ndarray:
    r = SP.record_size(n)
    cols = torch.from_numpy(samples // 4).to(recs.device)
    shift = (2 * (samples % 4)).astype(np.uint8)
    out = np.zeros((len(samples), 4), dtype=np.int64)
    rows = max(1, (64 << 20) // len(samples))
    for a in range(0, v, rows):
        b = min(v, a + rows)
        codes = (recs[a * r: b * r].view(b - a, r).index_select(1, cols).cpu().numpy() >> shift) & 3
        out += np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1)
    return out


_CACHE = {}


def records_for(v: int, n: int):
    if _CACHE.get("shape") != (v, n):
        _CACHE.clear()
        torch.cuda.empty_cache()
        r = SP.record_size(n)
        free, _total = torch.cuda.mem_get_info(0)
        need = v * r + (4 << 30)
        if free < need:
            pytest.skip(f"needs {need / 2**30:.1f} GiB of free HBM, have {free / 2**30:.1f}")
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            recs = eng.synth_records(v, hwe=True)
            eng.wait()
        want = torch_counts(recs, v, n).cpu().numpy()
        _CACHE.update(shape=(v, n), recs=recs, want=want)
    return _CACHE


@pytest.mark.parametrize("case", list(CASES))
def test_full_size_against_torch_and_numpy(case):
    v, n, key = CASES[case]
    d = records_for(v, n)
    kept = kept_set(n, key)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        k = eng.kept_count
        want = d["want"] if kept is None else d["want"][kept.astype(np.int64)]
        ranks = np.unique(np.concatenate([[0, k - 1], np.random.default_rng(99).choice(k, size=min(k, 256), replace=False)]))
        want_np = numpy_columns(d["recs"], v, n, ranks if kept is None else kept[ranks].astype(np.int64))
        for kname, kern in KERNELS.items():
            buf = torch.full((4 * k + 5,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)
            got = eng.sample_counts(d["recs"], n_variants=v, out=buf[1:], kernel=kern)
            eng.wait()
            h = buf.cpu().numpy()
            assert h[0] == -0x5A5A5A5B and (h[1 + 4 * k:] == -0x5A5A5A5B).all(), f"{case} shape {kname}: wrote outside its counts"
            got = got.cpu().numpy().view(np.uint32).astype(np.int64)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (f"{case} shape {kname}: {bad.size} of {k} kept samples differ; first {bad[0]}: "
                                   f"got {got[bad[0]].tolist()}, torch {want[bad[0]].tolist()}")
            assert (got[ranks] == want_np).all(), f"{case} shape {kname}: numpy columns differ"
