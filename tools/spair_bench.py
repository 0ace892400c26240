#!/usr/bin/env python3
"""Times pgenhip_sample_pair_stats (GtEngine.sample_pair_tables) on the measurement shapes of the other tools: HWE records
synthesised on the device, a warm-up, then device events around --steps calls per forced shape.  One call per shape is what
`pgen-hip kinship` issues for one staged block of variants (128 MiB of records) and one pair of rank tiles:
  chr22     2 504 samples, the full square (one call)
  basic2    300 samples, the full square
  configs2  500 000 samples, one 4 096 x 4 096 rank tile
One JSON line per shape: ms of MFMA and of GENERAL (GENERAL on --general-rows rows at most, scaled by the row count, and said
so), sample-pair-rows per second, and the MFMA time as a multiple of two yardsticks measured or computed in the same run:
  matrix_ms     pgenhip_decode_matrix, sample-major int8, on the same rows: the transpose-and-expand work alone (of ALL samples of
                the rows, once; the pair kernel expands a rank tile once per tile it meets);
  mfma_bound_ms nine v_mfma_i32_16x16x64_i8 per 16 x 16 samples x 64 rows at 16 cycles each (the guide's cycles for this M x N),
                on 256 CUs x 4 SIMDs at 2.4 GHz.
After the timed loop --check-pairs seeded entries are compared with numpy for both shapes.

    python tools/spair_bench.py [--shapes chr22 basic2 configs2] [--steps 3] [--warmup 1]
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
MFMA_CYCLES = 16
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
    ap.add_argument("--slices", type=int, default=0, help="force PGENHIP_KNOB_SPAIR_SLICES")
    ap.add_argument("--check-pairs", type=int, default=24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spair_bench needs a GPU (the pair kernels have no CPU path)")
    for name in args.shapes:
        n, tile = SHAPES[name]
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            if args.slices:
                eng.tune(_capi.KNOB_SPAIR_SLICES, args.slices)
            r = eng.record_size
            v = BLOCK_BYTES // r
            k = n if tile is None else tile
            a = b = (0, k)
            recs = eng.synth_records(v, hwe=True)
            out = torch.empty(16 * k * k, dtype=torch.int32, device=eng.torch_device)
            ms_mfma = timed(eng, lambda: eng.sample_pair_tables(recs, n_variants=v, a=a, b=b, out=out, kernel=_capi.SPAIR_MFMA), args.steps, args.warmup)
            got_mfma = out.view(k, k, 4, 4).clone()
            vg = min(v, args.general_rows)
            ms_general = timed(eng, lambda: eng.sample_pair_tables(recs, n_variants=vg, a=a, b=b, out=out, kernel=_capi.SPAIR_GENERAL), 1, 1) * (v / vg)
            if vg == v and not torch.equal(out.view(k, k, 4, 4), got_mfma):
                raise SystemExit(f"{name}: GENERAL and MFMA differ")
            del out
            # seeded entries against numpy
            rng = np.random.default_rng(99)
            picks = sorted({int(x) for x in rng.integers(0, k, size=8)} | {0, k - 1})
            cols = {}
            for s in picks:
                col = recs.view(v, r)[:, s // 4].cpu().numpy()
                cols[s] = ((col >> (2 * (s % 4))) & 3).astype(np.int64)
            checked = 0
            for _ in range(args.check_pairs):
                i, l = (picks[int(x)] for x in rng.integers(0, len(picks), size=2))
                t = np.bincount(4 * cols[i] + cols[l], minlength=16).reshape(4, 4)
                if not np.array_equal(got_mfma[i, l].cpu().numpy().view(np.uint32), t):
                    raise SystemExit(f"{name}: MFMA table of ranks ({i}, {l}) differs from numpy")
                checked += 1
            del got_mfma
            mat = eng.decode_matrix(recs, v, dtype=torch.int8, sample_major=True)
            ms_matrix = timed(eng, lambda: eng.decode_matrix(recs, v, dtype=torch.int8, sample_major=True, out=mat), args.steps, args.warmup)
            del mat
            pair_rows = k * k * v
            bound_ms = 9 * MFMA_CYCLES * (-(-k // 16)) ** 2 * (-(-v // 64)) / (SIMDS * CLOCK) * 1e3
            print(json.dumps({"shape": name, "samples": n, "ranks": k, "rows": v, "mfma_ms": round(ms_mfma, 3),
                              "general_ms": round(ms_general, 3), "general_rows_timed": vg,
                              "mfma_pair_rows_per_s": round(pair_rows / (ms_mfma * 1e-3), 0),
                              "general_pair_rows_per_s": round(pair_rows / (ms_general * 1e-3), 0),
                              "matrix_ms": round(ms_matrix, 3), "mfma_over_matrix": round(ms_mfma / ms_matrix, 2),
                              "mfma_bound_ms": round(bound_ms, 3), "mfma_over_bound": round(ms_mfma / bound_ms, 2),
                              "entries_checked": checked}), flush=True)
            del recs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
