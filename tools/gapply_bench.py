#!/usr/bin/env python3
"""Times pgenhip_gram_apply (GtEngine.gram_apply) on the measurement shapes of tools/gram_bench.py: HWE records synthesised on the
device, integer tables drawn per row and an integer Q, a warm-up, then device events around --steps calls per forced shape and per
column count C = 1, 4, 16.  One call is what `pgen-hip pca` would issue for one staged block of variants (128 MiB of records) and one
group of columns:
  chr22     2 504 samples   (many short rows: row tiles alone fill the chip)
  basic2    300 samples
  configs2  500 000 samples (few long rows: the P pass must split the samples)
One JSON line per shape and C, printed and appended to --out: ms of MFMA and of GENERAL (GENERAL on --general-rows rows at most,
scaled by the row count, and said so), and beside them two bounds of the MFMA shape, both arithmetic from the code:
  mfma_bound_ms   one v_mfma_f64_16x16x4_f64 per 16 rows x 4 samples (P pass) and per 16 samples x 4 rows (Y pass), whatever C, at the
                  64-cycle issue interval DESIGN.md §16 infers, on 256 CUs x 4 SIMDs at 2.4 GHz;
  bytes_bound_ms  the records twice, Q once per 64-row tile of the P pass, proj written once and read once per 256-sample tile of
                  the Y pass, Y once, at 8 TB/s;
--keep-every M runs the kept-list instantiations on every M-th sample (the byte bound then still counts whole records);
and, for the shapes whose K x K square fits (chr22, basic2), gram_mfma_ms: pgenhip_sample_gram's MFMA shape on the same rows.
Where GENERAL ran on all the rows the two shapes' P and Y must be equal bit for bit (the inputs are integers).

Run one shape per process, each under its own time limit, and stop at the first failure:
    timeout 300 python tools/gapply_bench.py --shapes chr22 --out profiles/r13_gapply/gapply_bench.jsonl &&
    timeout 300 python tools/gapply_bench.py --shapes basic2 --out profiles/r13_gapply/gapply_bench.jsonl &&
    timeout 300 python tools/gapply_bench.py --shapes configs2 --out profiles/r13_gapply/gapply_bench.jsonl
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

SIMDS = 256 * 4
CLOCK = 2.4e9
MFMA_CYCLES = 64
HBM_BYTES_PER_S = 8e12
BLOCK_BYTES = 128 << 20
ROW_TILE, SAMPLE_TILE = 64, 256   # plan::gapply::kRowTile, kSampleTile
# name -> (samples, time sample_gram's full square beside it)
SHAPES = {"chr22": (2_504, True), "basic2": (300, True), "configs2": (500_000, False)}


def timed(eng, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    eng.wait()
    eng.timer_start()
    for _ in range(steps):
        fn()
    return eng.timer_stop() / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--columns", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--general-rows", type=int, default=16384, help="rows of the GENERAL timing (its ms is scaled to the block's rows)")
    ap.add_argument("--keep-every", type=int, default=0, help="keep every M-th sample through a kept list (0: all samples, no list)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gapply_bench needs a GPU (the Gram product kernels have no CPU path)")
    for name in args.shapes:
        n, with_gram = SHAPES[name]
        kept = list(range(0, n, args.keep_every)) if args.keep_every else None
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r, k = eng.record_size, eng.kept_count
            v = BLOCK_BYTES // r
            recs = eng.synth_records(v, hwe=True)
            rng = np.random.default_rng(7)
            d_t = torch.from_numpy(rng.integers(-8, 9, size=(v, 4)).astype(np.float64)).to(eng.torch_device)
            ms_gram = None
            if with_gram:
                sq = torch.empty(k * k, dtype=torch.float64, device=eng.torch_device)
                ms_gram = timed(eng, lambda: eng.sample_gram(recs, n_variants=v, code_values=d_t, out=sq, kernel=_capi.GRAM_MFMA), args.steps, args.warmup)
                del sq
            for c in args.columns:
                d_q = torch.from_numpy(rng.integers(-4, 5, size=(k, c)).astype(np.float64)).to(eng.torch_device)
                proj = torch.empty(v * c, dtype=torch.float64, device=eng.torch_device)
                out = torch.empty(k * c, dtype=torch.float64, device=eng.torch_device)
                run = lambda rows, kernel: eng.gram_apply(recs, d_t, d_q, n_variants=rows, proj=proj, out=out, kernel=kernel)
                ms_mfma = timed(eng, lambda: run(v, _capi.GAPPLY_MFMA), args.steps, args.warmup)
                p_mfma, y_mfma = proj.clone(), out.clone()
                vg = min(v, args.general_rows)
                ms_general = timed(eng, lambda: run(vg, _capi.GAPPLY_GENERAL), 1, 1) * (v / vg)
                if vg == v and not (torch.equal(proj, p_mfma) and torch.equal(out, y_mfma)):
                    raise SystemExit(f"{name} C = {c}: GENERAL and MFMA differ")
                mfmas = 2 * (-(-v // 16)) * (-(-k // 4))
                mfma_bound = MFMA_CYCLES * mfmas / (SIMDS * CLOCK) * 1e3
                nbytes = 2 * v * r + (-(-v // ROW_TILE)) * k * c * 8 + v * c * 8 * (1 + -(-k // SAMPLE_TILE)) + k * c * 8
                bytes_bound = nbytes / HBM_BYTES_PER_S * 1e3
                line = {"shape": name, "samples": n, "kept": k, "rows": v, "columns": c, "mfma_ms": round(ms_mfma, 3), "general_ms": round(ms_general, 3),
                        "general_rows_timed": vg, "general_over_mfma": round(ms_general / ms_mfma, 2), "mfma_bound_ms": round(mfma_bound, 3),
                        "bytes_bound_ms": round(bytes_bound, 3), "fraction_of_mfma_bound": round(mfma_bound / ms_mfma, 3),
                        "fraction_of_bytes_bound": round(bytes_bound / ms_mfma, 3)}
                if ms_gram is not None:
                    line["gram_mfma_ms"] = round(ms_gram, 3)
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(text + "\n")
                del d_q, proj, out, p_mfma, y_mfma
            del recs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
