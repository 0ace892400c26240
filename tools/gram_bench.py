#!/usr/bin/env python3
"""Times pgenhip_sample_gram (GtEngine.sample_gram) on the measurement shapes of tools/spair_bench.py: HWE records synthesised on the
device, integer tables drawn per row, a warm-up, then device events around --steps calls per forced shape.  One call per shape is
what `pgen-hip grm` issues for one staged block of variants (128 MiB of records), one pair of rank tiles and one of its two tables:
  chr22     2 504 samples, the full square (one call)
  basic2    300 samples, the full square
  configs2  500 000 samples, one 4 096 x 4 096 rank tile
One JSON line per shape, printed and appended to --out: ms of MFMA and of GENERAL (GENERAL on --general-rows rows at most, scaled by
the row count, and said so), sample-pair-rows per second, and the MFMA time beside two yardsticks of the same run:
  spair_mfma_ms  pgenhip_sample_pair_stats, MFMA shape, on the same rows and ranks (the int8 kernel of DESIGN.md §15);
  mfma_bound_ms  one v_mfma_f64_16x16x4_f64 per 16 x 16 ranks x 4 rows at the 64-cycle issue interval DESIGN.md §16 infers,
                 on 256 CUs x 4 SIMDs at 2.4 GHz (3.9e13 sample-pair-rows per second).
After the timed loop --check-pairs seeded entries are compared with numpy (the tables are integers, so the sums are exact).

Run one shape per process, each under its own time limit, and stop at the first failure:
    timeout 300 python tools/gram_bench.py --shapes chr22 --out profiles/r12_gram/gram_bench.jsonl &&
    timeout 300 python tools/gram_bench.py --shapes basic2 --out profiles/r12_gram/gram_bench.jsonl &&
    timeout 300 python tools/gram_bench.py --shapes configs2 --out profiles/r12_gram/gram_bench.jsonl
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
BLOCK_BYTES = 128 << 20
# name -> (samples, ranks of the tile: None = all)
SHAPES = {"chr22": (2_504, None), "basic2": (300, None), "configs2": (500_000, 4_096)}


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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--general-rows", type=int, default=8192, help="rows of the GENERAL timing (its ms is scaled to the block's rows)")
    ap.add_argument("--slices", type=int, default=0, help="force PGENHIP_KNOB_GRAM_SLICES")
    ap.add_argument("--check-pairs", type=int, default=24)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gram_bench needs a GPU (the Gram kernels have no CPU path)")
    for name in args.shapes:
        n, tile = SHAPES[name]
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            if args.slices:
                eng.tune(_capi.KNOB_GRAM_SLICES, args.slices)
            r = eng.record_size
            v = BLOCK_BYTES // r
            k = n if tile is None else tile
            a = b = (0, k)
            recs = eng.synth_records(v, hwe=True)
            tables = np.random.default_rng(7).integers(-8, 9, size=(v, 4)).astype(np.float64)
            d_t = torch.from_numpy(tables).to(eng.torch_device)
            out = torch.empty(k * k, dtype=torch.float64, device=eng.torch_device)
            ms_mfma = timed(eng, lambda: eng.sample_gram(recs, n_variants=v, code_values=d_t, a=a, b=b, out=out, kernel=_capi.GRAM_MFMA), args.steps, args.warmup)
            got_mfma = out.view(k, k).clone()
            vg = min(v, args.general_rows)
            ms_general = timed(eng, lambda: eng.sample_gram(recs, n_variants=vg, code_values=d_t, a=a, b=b, out=out, kernel=_capi.GRAM_GENERAL), 1, 1) * (v / vg)
            if vg == v and not torch.equal(out.view(k, k), got_mfma):
                raise SystemExit(f"{name}: GENERAL and MFMA differ")
            del out
            # seeded entries against numpy
            rng = np.random.default_rng(99)
            picks = sorted({int(x) for x in rng.integers(0, k, size=8)} | {0, k - 1})
            cols = {}
            for s in picks:
                col = recs.view(v, r)[:, s // 4].cpu().numpy()
                cols[s] = np.take_along_axis(tables, ((col >> (2 * (s % 4))) & 3).astype(np.int64)[:, None], axis=1)[:, 0]
            checked = 0
            for _ in range(args.check_pairs):
                i, l = (picks[int(x)] for x in rng.integers(0, len(picks), size=2))
                if float(got_mfma[i, l]) != float(np.dot(cols[i], cols[l])):
                    raise SystemExit(f"{name}: MFMA entry of ranks ({i}, {l}) differs from numpy")
                checked += 1
            del got_mfma
            pairs = torch.empty(16 * k * k, dtype=torch.int32, device=eng.torch_device)
            ms_spair = timed(eng, lambda: eng.sample_pair_tables(recs, n_variants=v, a=a, b=b, out=pairs, kernel=_capi.SPAIR_MFMA), args.steps, args.warmup)
            del pairs
            pair_rows = k * k * v
            bound_ms = MFMA_CYCLES * (-(-k // 16)) ** 2 * (-(-v // 4)) / (SIMDS * CLOCK) * 1e3
            line = json.dumps({"shape": name, "samples": n, "ranks": k, "rows": v, "mfma_ms": round(ms_mfma, 3),
                               "general_ms": round(ms_general, 3), "general_rows_timed": vg,
                               "mfma_pair_rows_per_s": round(pair_rows / (ms_mfma * 1e-3), 0),
                               "general_pair_rows_per_s": round(pair_rows / (ms_general * 1e-3), 0),
                               "spair_mfma_ms": round(ms_spair, 3), "mfma_over_spair_mfma": round(ms_mfma / ms_spair, 2),
                               "mfma_bound_ms": round(bound_ms, 3), "fraction_of_bound": round(bound_ms / ms_mfma, 3),
                               "entries_checked": checked})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del recs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
