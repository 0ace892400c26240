#!/usr/bin/env python3
"""Times pgenhip_pair_stats (GtEngine.pair_tables / pair_r2) on the measurement shapes of tools/count_bench.py: HWE records
synthesised on the device, a warm-up, then device events around --steps passes over all rows.  A pass is cut into launches of as
many left rows as keep the output under --out-gib (the blocks a host would stream: each launch gets its rows and the W that
follow).  One JSON line per shape, window, mode and keep set: ms per pass and the two bounds it is read against,
  byte bound   records read once per tile (32 rows of R bytes, 16 on a diagonal tile) + the entries written, at the 6.3 TB/s
               measured read ceiling;
  issue bound  VALU per pair-word of the accumulation loop (19 in the disassembly: 9 v_and_b32 + 9 v_bcnt_u32_b32 + 1 of loop
               overhead, per lane and 2 x 2 pairs: 76 per step) x the pair-words the tiles compute / 64 lanes, at one wave64 VALU
               instruction per 2 cycles and SIMD: 256 CUs x 4 SIMDs x 2.4 GHz / 2,
and pgenhip_genotype_counts' ms on the same records.  After the timed loop --check-pairs seeded pairs are compared with numpy.

    python tools/pair_bench.py [--shapes chr22 basic2 configs2] [--windows 32 128] [--steps 3] [--warmup 1]
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

READ_CEILING = 6.3e12
VALU_PER_S = 256 * 4 * 2.4e9 / 2          # wave64 VALU instructions per second, whole chip
VALU_PER_PAIR_WORD = 19
TILE = 16
# name -> (variants, samples)
SHAPES = {"chr22": (1_103_547, 2_504), "basic2": (9_200_000, 300), "configs2": (100_000, 500_000)}


def tiles(v, n_left, w):
    """(tiles that meet the band, diagonal ones among them) of one launch: gt_pair.hip's numbering."""
    total = diag = 0
    right_tiles = -(-v // TILE)
    for lt in range(-(-n_left // TILE)):
        i_last = min(lt * TILE + TILE - 1, n_left - 1)
        last = min((i_last + w) // TILE, right_tiles - 1)
        total += last - lt + 1
        diag += 1
    return total, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--windows", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out-gib", type=float, default=2.0, help="output bytes per launch")
    ap.add_argument("--check-pairs", type=int, default=24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_bench needs a GPU (the pair kernel has no CPU path)")
    for name in args.shapes:
        v, n = SHAPES[name]
        for keep in ("all", "1pct"):
            kept = None
            if keep == "1pct":
                kept = np.sort(np.random.default_rng(5).choice(n, size=max(1, n // 100), replace=False)).astype(np.uint32)
            with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
                r = eng.record_size
                recs = eng.synth_records(v, hwe=True)
                vout = torch.empty(4 * v, dtype=torch.int32, device=eng.torch_device)
                for _ in range(args.warmup):
                    eng.genotype_counts(recs, n_variants=v, out=vout)
                eng.wait()
                eng.timer_start()
                for _ in range(args.steps):
                    eng.genotype_counts(recs, n_variants=v, out=vout)
                ms_counts = eng.timer_stop() / args.steps
                del vout
                for w in args.windows:
                    for mode in ("table", "r2"):
                        entry = 64 if mode == "table" else 4
                        bv = max(1, min(v, int(args.out_gib * (1 << 30)) // (w * entry)))
                        out = torch.empty(bv * w * entry // 4, dtype=torch.int32 if mode == "table" else torch.float32, device=eng.torch_device)
                        call = eng.pair_tables if mode == "table" else eng.pair_r2
                        blocks = [(b0, min(bv, v - b0), min(v - b0, bv + w)) for b0 in range(0, v, bv)]

                        def one_pass():
                            for b0, nl, nv in blocks:
                                call(recs, n_variants=nv, n_left=nl, window=w, out=out, records_offset=b0 * r)

                        for _ in range(args.warmup):
                            one_pass()
                        eng.wait()
                        eng.timer_start()
                        for _ in range(args.steps):
                            one_pass()
                        ms = eng.timer_stop() / args.steps
                        # the last block's entries against numpy, on seeded pairs
                        b0, nl, nv = blocks[-1]
                        host = out.cpu().numpy().view(np.uint32)
                        rng = np.random.default_rng(99)
                        checked = 0
                        for _ in range(args.check_pairs):
                            i = int(rng.integers(0, nl))
                            d = int(rng.integers(1, w + 1))
                            if i + d >= nv:
                                continue
                            rows = recs[(b0 + i) * r: (b0 + i + 1) * r].cpu().numpy(), recs[(b0 + i + d) * r: (b0 + i + d + 1) * r].cpu().numpy()
                            codes = [np.stack([(x >> (2 * k)) & 3 for k in range(4)], axis=1).reshape(-1)[:n].astype(np.int64) for x in rows]
                            if kept is not None:
                                codes = [c[kept.astype(np.int64)] for c in codes]
                            t = np.bincount(4 * codes[0] + codes[1], minlength=16)
                            p = i * w + d - 1
                            if mode == "table":
                                if not (host[16 * p: 16 * p + 16] == t).all():
                                    raise SystemExit(f"{name}: table of pair ({b0 + i}, {b0 + i + d}) differs from numpy")
                            else:
                                tt = t.reshape(4, 4)[:3, :3].astype(object)
                                a = np.arange(3, dtype=object)
                                nn, sx, sy = tt.sum(), (tt.sum(1) * a).sum(), (tt.sum(0) * a).sum()
                                sxx, syy, sxy = (tt.sum(1) * a * a).sum(), (tt.sum(0) * a * a).sum(), (tt * np.outer(a, a)).sum()
                                den = (nn * sxx - sx * sx) * (nn * syy - sy * sy)
                                got = host[p: p + 1].view(np.float32)[0]
                                if den == 0:
                                    ok = np.isnan(got)
                                else:
                                    want = np.float32(float((nn * sxy - sx * sy) ** 2) / float(den))
                                    ok = abs(float(got) - float(want)) <= 2 * float(np.spacing(want))
                                if not ok:
                                    raise SystemExit(f"{name}: r^2 of pair ({b0 + i}, {b0 + i + d}) differs from numpy")
                            checked += 1
                        n_tiles = n_diag = 0
                        for b0, nl, nv in blocks:
                            t_, d_ = tiles(nv, nl, min(w, nv - 1))
                            n_tiles += t_
                            n_diag += d_
                        we = min(w, v - 1)
                        pairs = (v - we) * we + we * (we - 1) // 2
                        words = -(-n // 32)
                        rec_bytes = (32 * n_tiles - 16 * n_diag) * r
                        out_bytes = pairs * entry
                        byte_ms = (rec_bytes + out_bytes) / READ_CEILING * 1e3
                        issue_ms = VALU_PER_PAIR_WORD * n_tiles * TILE * TILE * words / 64 / VALU_PER_S * 1e3
                        bound = max(byte_ms, issue_ms)
                        print(json.dumps({"shape": name, "variants": v, "samples": n, "kept": eng.kept_count, "window": w, "mode": mode,
                                          "launches": len(blocks), "ms": round(ms, 3), "tiles": n_tiles, "pairs": pairs,
                                          "byte_bound_ms": round(byte_ms, 3), "issue_bound_ms": round(issue_ms, 3),
                                          "binding": "issue" if issue_ms >= byte_ms else "bytes", "x_over_bound": round(ms / bound, 2),
                                          "genotype_counts_ms": round(ms_counts, 3), "pairs_checked": checked}), flush=True)
                        del out
                del recs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
