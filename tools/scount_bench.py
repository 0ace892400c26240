#!/usr/bin/env python3
"""Times pgenhip_sample_counts (GtEngine.sample_counts) on the measurement shapes of tools/count_bench.py: HWE records synthesised
on the device, a warm-up, then device events around --steps launches.  One JSON line per shape: ms per launch, algorithmic bytes
(V*R records read + 16*K counts written), that traffic's fraction of the 8 TB/s HBM peak and of the ~6.3 TB/s measured read
ceiling, and the per-variant count kernel's ms on the same records in the same run.
After the timed loop the counts of --check-samples seeded samples (and the first and last kept sample) are compared with numpy
over those samples' record bytes, gathered by torch; a wrong sample ends the run with an error.

    python tools/scount_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 20] [--warmup 3] [--kernel auto|rows]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import numpy as np
import torch

import pgen_rs_amd
from pgen_rs_amd import _capi

PEAK = 8.0e12
READ_CEILING = 6.3e12
# name -> (variants, samples, kept fraction: None = all samples)
SHAPES = {
    "configs2": (100_000, 500_000, None),
    "c5shard": (125_000, 500_000, 0.01),
    "chr22": (1_103_547, 2_504, None),
    "basic2": (9_200_000, 300, None),
}
KERNELS = {"auto": _capi.SCOUNT_AUTO, "rows": _capi.SCOUNT_ROWS}


def timed(eng, steps, warmup, fn):
    for _ in range(warmup):
        fn()
    eng.wait()
    eng.timer_start()
    for _ in range(steps):
        fn()
    return eng.timer_stop() / steps


def check(name, recs, v, r, n, kept, counts, n_check):
    """numpy over the record bytes of seeded kept samples (the byte columns holding them, gathered on the device)."""
    k = counts.shape[0]
    ranks = np.unique(np.concatenate([[0, k - 1], np.random.default_rng(12345).choice(k, size=min(k, n_check), replace=False)]))
    samples = ranks if kept is None else kept[ranks].astype(np.int64)
    cols = torch.from_numpy(samples // 4).to(recs.device)
    rows = max(1, (1 << 30) // max(1, len(samples)))
    got_bytes = []
    for a in range(0, v, rows):
        b = min(v, a + rows)
        got_bytes.append(recs[a * r: b * r].view(b - a, r).index_select(1, cols).cpu().numpy())
    codes = (np.concatenate(got_bytes) >> (2 * (samples % 4)).astype(np.uint8)) & 3
    want = np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1)
    bad = np.flatnonzero((counts[ranks] != want).any(axis=1))
    if bad.size:
        j = int(ranks[bad[0]])
        raise SystemExit(f"{name}: {bad.size} of {len(ranks)} sampled samples differ from numpy; first kept sample {j}: "
                         f"got {counts[j].tolist()}, numpy {want[bad[0]].tolist()}")
    return len(ranks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", default="auto", choices=list(KERNELS))
    ap.add_argument("--check-samples", type=int, default=64, help="seeded kept samples whose counts are compared with numpy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scount_bench needs a GPU (the count kernels have no CPU path)")
    for name in args.shapes:
        v, n, frac = SHAPES[name]
        kept = None
        if frac is not None:   # count_bench's c5shard subset
            rng = np.random.default_rng(5)
            kept = np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r = eng.record_size
            recs = eng.synth_records(v, hwe=True)
            out = torch.empty(4 * eng.kept_count, dtype=torch.int32, device=eng.torch_device)
            ms = timed(eng, args.steps, args.warmup, lambda: eng.sample_counts(recs, n_variants=v, out=out, kernel=KERNELS[args.kernel]))
            counts = out.view(-1, 4).cpu().numpy().view(np.uint32).astype(np.int64)
            vout = torch.empty(4 * v, dtype=torch.int32, device=eng.torch_device)
            ms_variant = timed(eng, args.steps, args.warmup, lambda: eng.genotype_counts(recs, n_variants=v, out=vout))
            del vout
            checked = check(name, recs, v, r, n, kept, counts, args.check_samples)
            assert (counts.sum(axis=1) == v).all(), "a sample's counts do not add up to V"
            alg = v * r + 16 * eng.kept_count
            print(json.dumps({"shape": name, "variants": v, "samples": n, "kept": eng.kept_count, "kernel": args.kernel, "ms": round(ms, 4),
                              "alg_bytes": alg, "tb_per_s": round(alg / (ms * 1e-3) / 1e12, 3),
                              "frac_of_8tbs": round(alg / (ms * 1e-3) / PEAK, 3), "frac_of_read_ceiling": round(alg / (ms * 1e-3) / READ_CEILING, 3),
                              "per_variant_ms": round(ms_variant, 4), "vs_per_variant": round(ms / ms_variant, 3), "samples_checked": checked}),
                  flush=True)
            del recs, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
