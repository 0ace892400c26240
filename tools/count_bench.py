#!/usr/bin/env python3
"""Times pgenhip_genotype_counts (GtEngine.genotype_counts) on the measurement shapes: records synthesised on the device, a
warm-up, then device events around --steps launches.  One JSON line per shape: ms per launch, algorithmic bytes (V*R records
read + 16*V counts written) and that traffic's fraction of the 8 TB/s HBM peak and of the ~6.3 TB/s measured read ceiling.

    python tools/count_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 20] [--warmup 3] [--kernel auto|wave|rows]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
KERNELS = {"auto": _capi.COUNT_AUTO, "wave": _capi.COUNT_WAVE_PER_ROW, "rows": _capi.COUNT_ROWS_PER_WAVE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", default="auto", choices=list(KERNELS))
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
            counts = out.view(v, 4).cpu().numpy().view(np.uint32)
            assert (counts.astype(np.int64).sum(axis=1) == eng.kept_count).all(), "counts do not add up to K"
            alg = v * r + 16 * v
            print(json.dumps({"shape": name, "variants": v, "samples": n, "kept": eng.kept_count, "kernel": args.kernel, "ms": round(ms, 4),
                              "alg_bytes": alg, "tb_per_s": round(alg / (ms * 1e-3) / 1e12, 3),
                              "frac_of_8tbs": round(alg / (ms * 1e-3) / PEAK, 3), "frac_of_read_ceiling": round(alg / (ms * 1e-3) / READ_CEILING, 3)}),
                  flush=True)
            del recs, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
