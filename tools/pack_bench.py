#!/usr/bin/env python3
"""Times pgenhip_pack_records (GtEngine.pack_records) on the measurement shapes chr22 / basic2 / configs[2] with all samples kept,
a seeded random half and a seeded 1 %: HWE records synthesised on the device, a warm-up, then every timed step between its own
pair of device events.  One JSON line per shape, keep and kernel shape: median / min / max ms, the byte bound (DENSE: V*R read +
V*R_K written; GATHER: the 64-byte sectors of each row that hold a kept sample + V*R_K written) at the 6.3 TB/s read ceiling, the
ratio to it, and for DENSE with the identity map a device-to-device copy of the same record bytes timed in the same run.
After the timed loop --check-rows seeded rows (and the first and the last) are compared with numpy on their record bytes.

    python tools/pack_bench.py [--shapes chr22 basic2 configs2] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import numpy as np
import torch

import pgen_rs_amd
from pgen_rs_amd import _capi
from pgen_rs_amd.engine import BED_CODE_MAP

CEILING = 6.3e12
SHAPES = {"chr22": (1_103_547, 2_504), "basic2": (9_200_000, 300), "configs2": (100_000, 500_000)}
KEEPS = {"all": None, "half": 0.5, "p1": 0.01}
NAMES = {_capi.PACK_GENERAL: "general", _capi.PACK_DENSE: "dense", _capi.PACK_GATHER: "gather"}


def timed(eng, steps, warmup, fn):
    """ms of every timed step (each between its own events; timer_stop synchronises)."""
    for _ in range(warmup):
        fn()
    eng.wait()
    ms = []
    for _ in range(steps):
        eng.timer_start()
        fn()
        ms.append(eng.timer_stop())
    return ms


def check(name, recs, v, r, n, kept, out, code_map, n_check):
    rows = np.unique(np.concatenate([[0, v - 1], np.random.default_rng(12345).choice(v, size=min(v, n_check), replace=False)]))
    d_rows = torch.from_numpy(rows).to(recs.device)
    h = recs[: v * r].view(v, r).index_select(0, d_rows).cpu().numpy()
    codes = np.stack([(h >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(rows), -1)[:, :n]
    if kept is not None:
        codes = codes[:, kept.astype(np.int64)]
    if code_map is not None:
        codes = np.asarray(code_map, dtype=np.uint8)[codes]
    k = codes.shape[1]
    padded = np.zeros((len(rows), (k + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :k] = codes
    q = padded.reshape(len(rows), -1, 4)
    want = q[:, :, 0] | q[:, :, 1] << 2 | q[:, :, 2] << 4 | q[:, :, 3] << 6
    got = out.index_select(0, d_rows).cpu().numpy()
    if not (got == want).all():
        i, b = np.argwhere(got != want)[0]
        raise SystemExit(f"{name}: variant {rows[i]}, byte {b}: got {got[i, b]}, numpy {want[i, b]}")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--keeps", nargs="+", default=list(KEEPS), choices=list(KEEPS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=32, help="seeded variants compared with numpy, every byte")
    ap.add_argument("--no-general", action="store_true", help="skip the GENERAL baseline")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pack_bench needs a GPU (the pack kernels have no CPU path)")
    dev_name = torch.cuda.get_device_name(0)
    for name in args.shapes:
        v, n = SHAPES[name]
        for keep in args.keeps:
            kept = None
            if KEEPS[keep] is not None:
                kept = np.sort(np.random.default_rng(5).choice(n, size=max(1, int(n * KEEPS[keep])), replace=False)).astype(np.uint32)
            with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
                r, k, rk = eng.record_size, eng.kept_count, eng.packed_record_size
                recs = eng.synth_records(v, hwe=True)
                big = torch.empty(v * rk, dtype=torch.uint8, device=eng.torch_device)
                if kept is None:
                    bound = v * (r + rk)
                    fast = _capi.PACK_DENSE
                else:
                    bound = v * (64 * len(np.unique(kept // 256)) + rk)
                    fast = _capi.PACK_GATHER
                copy_ms = None
                if kept is None:   # the yardstick: the same bytes through a device-to-device copy, in the same run
                    copy_ms = statistics.median(timed(eng, args.steps, args.warmup, lambda: big.copy_(recs[: v * r])))
                forms = [(fast, None, False), (fast, BED_CODE_MAP, False)] + ([] if args.no_general else [(_capi.PACK_GENERAL, None, True)])
                for shape, cmap, slow in forms:
                    steps, warmup = (2, 1) if slow else (args.steps, args.warmup)
                    big.fill_(0xA5)
                    ms = timed(eng, steps, warmup, lambda: eng.pack_records(recs, n_variants=v, out=big, code_map=cmap, shape=shape))
                    med = statistics.median(ms)
                    out = eng.pack_records(recs, n_variants=v, out=big, code_map=cmap, shape=shape)
                    checked = check(name, recs, v, r, n, kept, out, cmap, args.check_rows)
                    bound_ms = bound / CEILING * 1e3
                    line = {"device": dev_name, "shape": name, "variants": v, "samples": n, "keep": keep, "kept": k, "kernel": NAMES[shape],
                            "map": "bed" if cmap else "identity", "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                            "steps": steps, "bound_bytes": bound, "bound_ms": round(bound_ms, 4), "x_bound": round(med / bound_ms, 2),
                            "tb_per_s": round(bound / (med * 1e-3) / 1e12, 3), "rows_checked": checked}
                    if copy_ms is not None:
                        line["d2d_copy_ms"] = round(copy_ms, 4)
                        line["vs_d2d_copy"] = round(med / copy_ms, 3)
                    print(json.dumps(line), flush=True)
                del recs, big, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
