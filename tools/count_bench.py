#!/usr/bin/env python3
"""Times pgenhip_genotype_counts (GtEngine.genotype_counts) on the measurement shapes: records synthesised on the device, a
warm-up, then device events around --steps launches.  One JSON line per shape: ms per launch, algorithmic bytes (V*R records
read + 16*V counts written) and that traffic's fraction of the 8 TB/s HBM peak and of the ~6.3 TB/s measured read ceiling.
After the timed loop the counts of --check-rows seeded rows (and the first and last row) are compared with the CPU oracle's;
a wrong row ends the run with an error, so a launch that skipped rows or chunks cannot pass as a fast one.

    python tools/count_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 20] [--warmup 3] [--kernel auto|wave|rows]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]
import numpy as np
import torch

import pgen_oracle as oracle   # the checker only: nothing timed goes through it
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
KERNELS = {"auto": _capi.COUNT_AUTO, "wave": _capi.COUNT_WAVE_PER_ROW, "rows": _capi.COUNT_ROWS_PER_WAVE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", default="auto", choices=list(KERNELS))
    ap.add_argument("--check-rows", type=int, default=512, help="seeded rows whose counts are compared with the CPU oracle")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("count_bench needs a GPU (the count kernels have no CPU path)")
    for name in args.shapes:
        v, n, frac = SHAPES[name]
        kept = None
        if frac is not None:
            rng = np.random.default_rng(5)
            kept = np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r = eng.record_size
            recs = eng.synth_records(v, hwe=True)
            out = torch.empty(4 * v, dtype=torch.int32, device=eng.torch_device)
            for _ in range(args.warmup):
                eng.genotype_counts(recs, n_variants=v, out=out, kernel=KERNELS[args.kernel])
            eng.wait()
            eng.timer_start()
            for _ in range(args.steps):
                eng.genotype_counts(recs, n_variants=v, out=out, kernel=KERNELS[args.kernel])
            ms = eng.timer_stop() / args.steps
            counts = out.view(v, 4).cpu().numpy().view(np.uint32).astype(np.int64)
            rows = np.unique(np.concatenate([[0, v - 1], np.random.default_rng(12345).choice(v, size=min(v, args.check_rows), replace=False)]))
            sample = recs.view(v, r)[torch.from_numpy(rows).to(recs.device)].cpu().numpy()
            want = oracle.genotype_counts(sample.reshape(-1), len(rows), n, kept_idx=kept)
            bad = np.flatnonzero((counts[rows] != want).any(axis=1))
            if bad.size:
                j = int(rows[bad[0]])
                raise SystemExit(f"{name}: {bad.size} of {len(rows)} sampled rows differ from the CPU oracle; first row {j}: "
                                 f"got {counts[j].tolist()}, oracle {want[bad[0]].tolist()}")
            # over-count guard only, over every row: the kernel writes hom-ref = K - the other three, so this holds by construction
            # unless a row counted more than K samples; skipped rows or chunks are what the sampled oracle check above catches
            assert (counts.sum(axis=1) == eng.kept_count).all(), "counts do not add up to K"
            alg = v * r + 16 * v
            print(json.dumps({"shape": name, "variants": v, "samples": n, "kept": eng.kept_count, "kernel": args.kernel, "ms": round(ms, 4),
                              "alg_bytes": alg, "tb_per_s": round(alg / (ms * 1e-3) / 1e12, 3),
                              "frac_of_8tbs": round(alg / (ms * 1e-3) / PEAK, 3), "frac_of_read_ceiling": round(alg / (ms * 1e-3) / READ_CEILING, 3),
                              "rows_checked": len(rows)}),
                  flush=True)
            del recs, out, sample
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
