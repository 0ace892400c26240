#!/usr/bin/env python3
"""Times pgenhip_sample_scores (GtEngine.sample_scores) on the measurement shapes of tools/scount_bench.py, with C = 1 and C = 8
weight columns, beside pgenhip_sample_counts on the same records in the same run: HWE records synthesised on the device, random
f32 weights and miss values, a warm-up, then device events around --steps launches.  One JSON line per shape: ms per launch of the
three kernels, the two ratios to the count kernel (the yardstick: it reads the same bytes and is the nearest column reduction), and
genotype-columns per second.
After the timed loops the scores of --check-samples seeded samples (and the first and last kept sample) are compared with a
float64 numpy sum over those samples' record bytes, gathered by torch, within twice the any-order summation bound
(V + 1) 2^-53 sum|term| (both sums are any-order sums of the same exact terms); a sample outside it ends the run with an error.

    python tools/score_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 10] [--warmup 2]
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

# name -> (variants, samples, kept fraction: None = all samples)
SHAPES = {
    "configs2": (100_000, 500_000, None),
    "c5shard": (125_000, 500_000, 0.01),
    "chr22": (1_103_547, 2_504, None),
    "basic2": (9_200_000, 300, None),
}
COLUMNS = (1, 8)


def timed(eng, steps, warmup, fn):
    for _ in range(warmup):
        fn()
    eng.wait()
    eng.timer_start()
    for _ in range(steps):
        fn()
    return eng.timer_stop() / steps


def check(name, recs, v, r, kept, w, miss, scores, n_check):
    """float64 numpy over the record bytes of seeded kept samples (the byte columns holding them, gathered on the device)."""
    k, c = scores.shape
    ranks = np.unique(np.concatenate([[0, k - 1], np.random.default_rng(12345).choice(k, size=min(k, n_check), replace=False)]))
    samples = ranks if kept is None else kept[ranks].astype(np.int64)
    cols = torch.from_numpy(samples // 4).to(recs.device)
    w64, m64 = w.astype(np.float64), miss.astype(np.float64)
    want, scale = np.zeros((len(ranks), c)), np.zeros((len(ranks), c))
    rows = max(1, (1 << 26) // max(1, len(samples)))
    for a in range(0, v, rows):
        b = min(v, a + rows)
        by = recs[a * r: b * r].view(b - a, r).index_select(1, cols).cpu().numpy()
        codes = (by >> (2 * (samples % 4)).astype(np.uint8)) & 3
        d = np.where(codes == 3, m64[a:b, None], codes.astype(np.float64))
        want += d.T @ w64[a:b]
        scale += np.abs(d).T @ np.abs(w64[a:b])
    lim = 2.02 * (v + 1) * 2.0 ** -53 * scale
    bad = np.flatnonzero((np.abs(scores[ranks] - want) > lim).any(axis=1))
    if bad.size:
        j = int(ranks[bad[0]])
        raise SystemExit(f"{name}: {bad.size} of {len(ranks)} sampled samples differ from numpy at C = {c}; first kept sample {j}: "
                         f"got {scores[j].tolist()}, numpy {want[bad[0]].tolist()}")
    return len(ranks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-samples", type=int, default=16, help="seeded kept samples whose scores are compared with numpy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs a GPU (the score kernel has no CPU path)")
    for name in args.shapes:
        v, n, frac = SHAPES[name]
        kept = None
        if frac is not None:   # scount_bench's c5shard subset
            rng = np.random.default_rng(5)
            kept = np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r, k = eng.record_size, eng.kept_count
            recs = eng.synth_records(v, hwe=True)
            rng = np.random.default_rng(7)
            w = rng.normal(size=(v, 8)).astype(np.float32)
            miss = rng.uniform(0.0, 2.0, size=v).astype(np.float32)
            d_w8, d_miss = torch.from_numpy(w).to(eng.torch_device), torch.from_numpy(miss).to(eng.torch_device)
            counts = torch.empty(4 * k, dtype=torch.int32, device=eng.torch_device)
            ms_counts = timed(eng, args.steps, args.warmup, lambda: eng.sample_counts(recs, n_variants=v, out=counts))
            res = {"shape": name, "variants": v, "samples": n, "kept": k, "sample_counts_ms": round(ms_counts, 4)}
            for c in COLUMNS:
                d_w = d_w8[:, :c].contiguous()
                out = torch.empty(k * c, dtype=torch.float64, device=eng.torch_device)
                ms = timed(eng, args.steps, args.warmup, lambda: eng.sample_scores(recs, d_w, miss=d_miss, out=out))
                checked = check(name, recs, v, r, kept, w[:, :c], miss, out.view(k, c).cpu().numpy(), args.check_samples)
                res.update({f"score_c{c}_ms": round(ms, 4), f"score_c{c}_vs_sample_counts": round(ms / ms_counts, 2),
                            f"score_c{c}_genotype_columns_per_s": round(v * n * c / (ms * 1e-3), -6)})
                del out, d_w
            res["samples_checked"] = checked
            print(json.dumps(res), flush=True)
            del recs, counts, d_w8, d_miss
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
