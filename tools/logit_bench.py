#!/usr/bin/env python3
"""Times pgenhip_variant_logistic (GtEngine.variant_logistic), GENERAL beside FAST, with n_cov = 1, 4, 11 and 15 design columns on three
shapes: a block of chr22 rows (2 504 samples), of basic2 rows (300 samples) and of configs[2] rows (500 000 samples).  HWE records
synthesised on the device, a design of an intercept and standard normal covariates, a Bernoulli phenotype that depends on the first
covariate, the null model fitted here in numpy; mean imputation.  A warm-up, then device events around --steps launches, --rounds
times over.  The JSON line of a shape holds, per n_cov and kernel shape, the median ms per launch, the spread (max / min over the
rounds), rows per second, the evaluations the rows took, and the FP64 FMA issue bound of the sums alone: per evaluation and 64 samples
p (p + 1) / 2 + p FMAs of 4 cycles each on one SIMD, every SIMD of the chip busy (p = n_cov + 1) — what is left out of it (the linear
predictor, the exponential, the division, the reductions, the solve) is what the fraction below 1 shows.
GENERAL and FAST must agree: status words equal, evaluations within one, coefficients within 1e-8 — else the run ends with an error.

    python tools/logit_bench.py [--shapes chr22 basic2 configs2] [--steps 3] [--warmup 1] [--rounds 3]
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

# name -> (rows of one block, samples)
SHAPES = {
    "chr22": (8192, 2_504),
    "basic2": (65536, 300),
    "configs2": (256, 500_000),
}
N_COV = (1, 4, 11, 15)   # p = 2, 5, 12, 16: one per bucket the FAST kernel is compiled for


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


def null_fit(design, y):
    beta = np.zeros(design.shape[1])
    for _ in range(50):
        mu = 1.0 / (1.0 + np.exp(-(design @ beta)))
        delta = np.linalg.solve((design * (mu * (1.0 - mu))[:, None]).T @ design, design.T @ (y - mu))
        if np.abs(delta).max() <= 1e-13:
            break
        beta += delta
    return beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=25)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logit_bench needs a GPU (the kernels have no CPU path)")
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    for name in args.shapes:
        v, n = SHAPES[name]
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            dev = eng.torch_device
            recs = eng.synth_records(v, hwe=True)
            counts = eng.genotype_counts(recs, n_variants=v).view(v, 4).to(torch.float64)
            called = counts[:, :3].sum(dim=1).clamp(min=1.0)
            table = torch.stack([torch.zeros_like(called), torch.ones_like(called), 2.0 * torch.ones_like(called),
                                 (counts[:, 1] + 2.0 * counts[:, 2]) / called], dim=1).contiguous()
            rng = np.random.default_rng(7)
            x15 = np.column_stack([np.ones(n), rng.standard_normal((n, 14))])
            y = (rng.random(n) < 1.0 / (1.0 + np.exp(0.4 - 0.5 * x15[:, 1]))).astype(np.float64)
            d_y = torch.from_numpy(y).to(dev)
            res = {"shape": name, "rows": v, "samples": n, "max_iter": args.max_iter, "tol": args.tol}
            for nc in N_COV:
                p = nc + 1
                design = np.ascontiguousarray(x15[:, :nc])
                d_x, d_s = torch.from_numpy(design).to(dev), torch.from_numpy(null_fit(design, y)).to(dev)
                outs = {}
                for label, flag in (("general", _capi.LOGIT_GENERAL), ("fast", _capi.LOGIT_FAST)):
                    coef = torch.empty(v * p, dtype=torch.float64, device=dev)
                    se = torch.empty(v, dtype=torch.float64, device=dev)
                    status = torch.empty(v, dtype=torch.int32, device=dev)
                    fn = lambda: eng.variant_logistic(recs, table, d_x, d_y, d_s, max_iter=args.max_iter, tol=args.tol, n_variants=v,
                                                      coef=coef, se=se, status=status, flags=flag)
                    ms, sp = timed(eng, args.steps, args.warmup, args.rounds, fn)
                    eng.wait()
                    evals = int((status & 0xFF).sum().item())
                    bound_ms = evals * ((n + 63) // 64) * (p * (p + 1) // 2 + p) * 4.0 / (simds * args.clock_ghz * 1e9) * 1e3
                    res.update({f"{label}_c{nc}_ms": round(ms, 4), f"{label}_c{nc}_spread": round(sp, 3), f"{label}_c{nc}_rows_per_s": round(v / ms * 1e3),
                                f"{label}_c{nc}_evaluations": evals, f"{label}_c{nc}_fma_issue_bound_ms": round(bound_ms, 4),
                                f"{label}_c{nc}_fraction_of_issue_bound": round(bound_ms / ms, 3)})
                    outs[label] = (coef.view(v, p), status)
                (cg, sg), (cf, sf) = outs["general"], outs["fast"]
                same = ((sg & ~0xFF) == (sf & ~0xFF)).all().item() and ((sg & 0xFF) - (sf & 0xFF)).abs().max().item() <= 1
                conv = (sg & _capi.LOGIT_CONVERGED) != 0
                if not same or (conv.any() and (cg[conv] - cf[conv]).abs().max().item() > 1e-8):
                    raise SystemExit(f"{name}, n_cov = {nc}: GENERAL and FAST disagree")
                res[f"c{nc}_converged"] = int(conv.sum().item())
                res[f"c{nc}_fast_speedup"] = round(res[f"general_c{nc}_ms"] / res[f"fast_c{nc}_ms"], 2)
            print(json.dumps(res), flush=True)
            del recs, counts, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
