#!/usr/bin/env python3
"""Times pgenhip_variant_sums (GtEngine.variant_sums), GENERAL and the matrix-core shape, with C = 1, 8 and 16 value columns on the
measurement shapes of tools/score_bench.py, in the same process beside its two yardsticks on the same records:
pgenhip_genotype_counts (the same bytes, the same per-row reduction) and pgenhip_sample_scores at C = 8 (the same
genotype-columns).  HWE records synthesised on the device, random FP64 values, a warm-up, then device events around --steps
launches, --rounds times over: the JSON line of a shape holds the median ms per launch, the spread (max / min over the rounds), the
ratios to the yardsticks and, for the matrix-core shape, the fraction of the MFMA issue bound (one v_mfma_f64_16x16x4_f64 per 4 rows
and record byte of a tile, --mfma-cycles cycles each per SIMD).
After the timed loops the sums of --check-rows seeded rows (and the first and last) are compared with a float64 numpy sum within
twice the any-order bound (K + 1) 2^-53 A_c; a row outside it ends the run with an error.

    python tools/vsum_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 5] [--warmup 1] [--rounds 3]
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

# name -> (variants, samples, kept fraction: None = all samples)
SHAPES = {
    "configs2": (100_000, 500_000, None),
    "c5shard": (125_000, 500_000, 0.01),
    "chr22": (1_103_547, 2_504, None),
    "basic2": (9_200_000, 300, None),
}
COLUMNS = (1, 8, 16)
TILE_BYTES = 32   # kTileBytes of csrc/gt_vsum.hip


def timed(eng, steps, warmup, rounds, fn):
    for _ in range(warmup):
        fn()
    eng.wait()
    ms = []
    for _ in range(rounds):
        eng.timer_start()
        for _ in range(steps):
            fn()
        ms.append(eng.timer_stop() / steps)
    return float(np.median(ms)), max(ms) / min(ms)


def check(name, recs, v, r, n, kept, vals, sums, n_check):
    c = sums.shape[1]
    rows = np.unique(np.concatenate([[0, v - 1], np.random.default_rng(12345).choice(v, size=min(v, n_check), replace=False)]))
    by = torch.stack([recs[j * r:(j + 1) * r] for j in rows.tolist()]).cpu().numpy()
    codes = np.stack([(by >> (2 * i)) & 3 for i in range(4)], axis=2).reshape(len(rows), -1)[:, :n]
    if kept is not None:
        codes = codes[:, kept.astype(np.int64)]
    want = np.stack([(codes == x).astype(np.float64) @ vals for x in range(4)], axis=2)
    lim = 2.02 * (vals.shape[0] + 1) * 2.0 ** -53 * np.abs(vals).sum(axis=0)[None, :, None]
    got = sums[torch.from_numpy(rows).to(sums.device)].cpu().numpy()
    bad = np.flatnonzero((np.abs(got - want) > lim).any(axis=(1, 2)))
    if bad.size:
        raise SystemExit(f"{name}: {bad.size} of {len(rows)} sampled rows differ from numpy at C = {c}; first row {int(rows[bad[0]])}")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-rows", type=int, default=8)
    ap.add_argument("--mfma-cycles", type=float, default=64.0, help="issue interval of v_mfma_f64_16x16x4_f64 per SIMD the bound assumes")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vsum_bench needs a GPU (the kernels have no CPU path)")
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    for name in args.shapes:
        v, n, frac = SHAPES[name]
        kept = None
        if frac is not None:   # score_bench's c5shard subset
            kept = np.sort(np.random.default_rng(5).choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r, k, dev = eng.record_size, eng.kept_count, eng.torch_device
            recs = eng.synth_records(v, hwe=True)
            rng = np.random.default_rng(7)
            vals = rng.normal(size=(k, 16))
            d_v16 = torch.from_numpy(vals).to(dev)
            counts = torch.empty(4 * v, dtype=torch.int32, device=dev)
            t = lambda fn: timed(eng, args.steps, args.warmup, args.rounds, fn)
            ms_counts, sp_counts = t(lambda: eng.genotype_counts(recs, n_variants=v, out=counts))
            d_w = torch.from_numpy(rng.normal(size=(v, 8)).astype(np.float32)).to(dev)
            scores = torch.empty(k * 8, dtype=torch.float64, device=dev)
            ms_score, sp_score = t(lambda: eng.sample_scores(recs, d_w, out=scores))
            del d_w, scores
            tiles = (r + TILE_BYTES - 1) // TILE_BYTES
            bound_ms = ((v + 3) // 4) * tiles * TILE_BYTES * args.mfma_cycles / (simds * args.clock_ghz * 1e9) * 1e3
            res = {"shape": name, "variants": v, "samples": n, "kept": k, "genotype_counts_ms": round(ms_counts, 4), "genotype_counts_spread": round(sp_counts, 3),
                   "score_c8_ms": round(ms_score, 4), "score_c8_spread": round(sp_score, 3), "mfma_issue_bound_ms": round(bound_ms, 4)}
            for c in COLUMNS:
                d_v = d_v16[:, :c].contiguous()
                out = torch.empty(v * c * 4, dtype=torch.float64, device=dev)
                for label, flag in (("general", _capi.VSUM_GENERAL), ("mfma", _capi.VSUM_MFMA)):
                    ms, sp = t(lambda: eng.variant_sums(recs, d_v, n_variants=v, out=out, flags=flag))
                    eng.wait()
                    sums = out.view(v, c, 4)
                    checked = check(name, recs, v, r, n, kept, vals[:, :c], sums, args.check_rows)
                    res.update({f"vsum_{label}_c{c}_ms": round(ms, 4), f"vsum_{label}_c{c}_spread": round(sp, 3),
                                f"vsum_{label}_c{c}_vs_genotype_counts": round(ms / ms_counts, 2)})
                    if c == 8:
                        res[f"vsum_{label}_c8_vs_score_c8"] = round(ms / ms_score, 2)
                    if label == "mfma":
                        res[f"vsum_mfma_c{c}_fraction_of_issue_bound"] = round(bound_ms / ms, 3)
                del out, d_v
            res["rows_checked"] = checked
            print(json.dumps(res), flush=True)
            del recs, counts, d_v16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
