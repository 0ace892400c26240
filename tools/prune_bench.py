#!/usr/bin/env python3
"""Times LD pruning's two device steps (GtEngine.pair_mask, GtEngine.prune_resolve) on the shapes of tools/pair_bench.py.

  mask_vs_r2   pair_mask against pair_r2 on the same HWE rows in the same process, interleaved: R2, MASK, R2, MASK, ...  Every arm
               run is the median of --steps passes, each between device events; the margin a difference is read against is the
               spread (max - min) of the R2 arm's own medians in that run.  A pass is cut into the launches pair_bench.py cuts it
               into (the r^2 output under --out-gib); the masks stay resident for all rows.
  mask_vs_r2_ld  the same two arms on the rows WITH LD of the resolve arm (about 7 edges per row), where tiles near the diagonal take
               the mask epilogue's shuffle-and-atomic path.
  resolve      prune_resolve GENERAL against BLOCK on masks made from rows WITH LD (HWE rows have none): every row is the row
               before it with a fraction --redraw of its samples drawn anew, a fresh row every --ld-block rows.  Priorities are the
               minor-allele frequencies from genotype_counts.  Per shape: calls of the host loop and its wall time (launches, the
               counter's D2H and the synchronisation included), median of --repeats loops, and the two final states compared.

One JSON line per measurement.

    python tools/prune_bench.py [--shapes chr22 basic2 configs2] [--windows 32 128] [--steps 10] [--arm-runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch

import pgen_rs_amd
from pgen_rs_amd import _capi

# name -> (variants, samples) of the mask_vs_r2 arm; configs2 is ONE block of configs[2]'s rows
SHAPES = {"chr22": (1_103_547, 2_504), "basic2": (9_200_000, 300), "configs2": (4_096, 500_000)}
# rows of the LD set per shape (the rows are made on the device, V x N codes at a time in column chunks)
LD_ROWS = {"chr22": 262_144, "basic2": 1_048_576, "configs2": 4_096}


def ld_records(eng, v, n, redraw, ld_block, seed):
    """(v, R) uint8 records with LD, made with torch on the device: sample s of row r holds the draw of the last row <= r at which
    s was redrawn (every sample is redrawn at the first row of an LD block); draws are HWE at the row's own allele frequency."""
    dev = eng.torch_device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = eng.record_size
    out = torch.zeros((v, r), dtype=torch.uint8, device=dev)
    p = 0.05 + 0.45 * torch.rand((v, 1), generator=g, device=dev)
    fresh = (torch.arange(v, device=dev) % ld_block == 0).unsqueeze(1)
    rows = torch.arange(v, device=dev, dtype=torch.int32).unsqueeze(1)
    cols = max(4, (32_000_000 // v) // 4 * 4)
    for c0 in range(0, n, cols):
        c = min(cols, n - c0)
        draw = ((torch.rand((v, c), generator=g, device=dev) < p).to(torch.uint8) + (torch.rand((v, c), generator=g, device=dev) < p).to(torch.uint8))
        flag = (torch.rand((v, c), generator=g, device=dev) < redraw) | fresh
        src = torch.cummax(torch.where(flag, rows, torch.zeros_like(rows)), dim=0).values.long()
        codes = torch.gather(draw, 0, src)
        pad = (-c) % 4
        if pad:
            codes = torch.cat([codes, torch.zeros((v, pad), dtype=torch.uint8, device=dev)], dim=1)
        q = codes.view(v, -1, 4)
        out[:, c0 // 4: c0 // 4 + q.shape[1]] = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
        del draw, flag, src, codes, q
    return out.view(-1)


def maf_priority(counts):
    c = counts.to(torch.float64)
    called = c[:, 0] + c[:, 1] + c[:, 2]
    alt = c[:, 1] + 2 * c[:, 2]
    maf = torch.where(called > 0, torch.minimum(alt, 2 * called - alt) / (2 * called).clamp(min=1), torch.zeros_like(called))
    return (maf * 4294967294.0).to(torch.int64).to(torch.int32)   # maf <= 0.5: the u32 fits an int32 tensor


def popcount(words):
    return sum(int(((words >> b) & 1).sum().item()) for b in range(32))


def timed_median(eng, one_pass, steps):
    ms = []
    for _ in range(steps):
        eng.timer_start()
        one_pass()
        ms.append(eng.timer_stop())
    return statistics.median(ms)


def mask_vs_r2(eng, name, v, n, w, args, ld=False):
    r = eng.record_size
    recs = ld_records(eng, v, n, args.redraw, args.ld_block, seed=v + w) if ld else eng.synth_records(v, hwe=True)
    bv = max(1, min(v, int(args.out_gib * (1 << 30)) // (w * 4)))
    out = torch.empty(bv * w, dtype=torch.float32, device=eng.torch_device)
    blocks = [(b0, min(bv, v - b0), min(v - b0, bv + w)) for b0 in range(0, v, bv)]
    fwd, bwd = (torch.zeros((v, (w + 31) // 32), dtype=torch.int32, device=eng.torch_device) for _ in range(2))

    def r2_pass():
        for b0, nl, nv in blocks:
            eng.pair_r2(recs, n_variants=nv, n_left=nl, window=w, out=out, records_offset=b0 * r)

    def mask_pass():
        for b0, nl, nv in blocks:
            eng.pair_mask(recs, n_variants=nv, n_left=nl, window=w, min_r2=args.r2, fwd=fwd[b0:], bwd=bwd[b0:], records_offset=b0 * r)

    for _ in range(args.warmup):
        r2_pass()
        mask_pass()
    eng.wait()
    med = {"r2": [], "mask": []}
    for _ in range(args.arm_runs):
        med["r2"].append(timed_median(eng, r2_pass, args.steps))
        med["mask"].append(timed_median(eng, mask_pass, args.steps))
    edges = popcount(fwd)
    spread = max(med["r2"]) - min(med["r2"])
    r2_ms, mask_ms = statistics.median(med["r2"]), statistics.median(med["mask"])
    print(json.dumps({"bench": "mask_vs_r2_ld" if ld else "mask_vs_r2", "shape": name, "variants": v, "samples": n, "window": w, "min_r2": args.r2, "launches": len(blocks),
                      "steps": args.steps, "r2_medians_ms": [round(x, 3) for x in med["r2"]], "mask_medians_ms": [round(x, 3) for x in med["mask"]],
                      "r2_ms": round(r2_ms, 3), "mask_ms": round(mask_ms, 3), "r2_spread_ms": round(spread, 3),
                      "mask_slower_beyond_spread": bool(mask_ms > r2_ms + spread), "edges": edges}), flush=True)


def resolve(eng, name, v, n, w, args):
    r = eng.record_size
    recs = ld_records(eng, v, n, args.redraw, args.ld_block, seed=v + w)
    counts = eng.genotype_counts(recs, n_variants=v)
    prio = maf_priority(counts.view(v, 4))
    t0 = time.perf_counter()
    fwd, bwd = eng.pair_mask(recs, n_variants=v, window=w, min_r2=args.r2)
    eng.wait()
    mask_ms = (time.perf_counter() - t0) * 1e3
    edges = popcount(fwd)
    finals = {}
    for shape, label in ((_capi.PRUNE_GENERAL, "general"), (_capi.PRUNE_BLOCK, "block")):
        ms, calls = [], 0
        for _ in range(args.repeats + 1):                 # the first loop is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            state, calls = eng.prune_resolve(fwd, bwd, w, priority=prio, shape=shape)
            ms.append((time.perf_counter() - t0) * 1e3)
        finals[label] = state
        print(json.dumps({"bench": "resolve", "shape": name, "rows": v, "samples": n, "window": w, "min_r2": args.r2, "redraw": args.redraw,
                          "ld_block": args.ld_block, "edges": edges, "edges_per_row": round(edges / v, 2), "kernel": label, "calls": calls,
                          "loop_ms": round(statistics.median(ms[1:]), 3), "loop_ms_all": [round(x, 3) for x in ms[1:]],
                          "kept": int((state == 1).sum().item()), "removed": int((state == 2).sum().item()),
                          "pair_mask_first_call_ms": round(mask_ms, 3)}), flush=True)
    if not torch.equal(finals["general"], finals["block"]):
        raise SystemExit(f"{name} W {w}: GENERAL and BLOCK ended at different states")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--windows", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--benches", nargs="+", default=["mask_vs_r2", "mask_vs_r2_ld", "resolve"], choices=["mask_vs_r2", "mask_vs_r2_ld", "resolve"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--arm-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--redraw", type=float, default=0.1)
    ap.add_argument("--ld-block", type=int, default=200)
    ap.add_argument("--out-gib", type=float, default=2.0, help="r^2 output bytes per launch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prune_bench needs a GPU (the kernels have no CPU path)")
    for name in args.shapes:
        v, n = SHAPES[name]
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            for w in args.windows:
                if "mask_vs_r2" in args.benches:
                    mask_vs_r2(eng, name, v, n, w, args)
                    torch.cuda.empty_cache()
                if "mask_vs_r2_ld" in args.benches:
                    mask_vs_r2(eng, name, LD_ROWS[name], n, w, args, ld=True)
                    torch.cuda.empty_cache()
                if "resolve" in args.benches:
                    resolve(eng, name, LD_ROWS[name], n, w, args)
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
