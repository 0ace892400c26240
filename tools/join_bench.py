#!/usr/bin/env python3
"""Times pgenhip_join_records (GtEngine.join_records) on the measurement shapes chr22 / basic2 / one block of configs[2], joined from
two and from eight equal parts, with no row flipped and with every row flipped: HWE records synthesised on the device per part, a
warm-up, then every timed step between its own pair of device events.  One JSON line per shape, part count, flip case and kernel
shape: median / min / max ms, the byte bound ((sum of the parts' record bytes + R) per row at the 8 TB/s roofline), the ratio to it,
and, timed in the same run, a device-to-device copy of the same bytes and pack_records DENSE on the joined records.
After the timed loop --check-rows seeded rows (and the first and the last) are compared with numpy on their record bytes.

    python tools/join_bench.py [--shapes chr22 basic2 configs2] [--parts 2 8] [--steps 10] [--warmup 2]
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

ROOFLINE = 8.0e12
SHAPES = {"chr22": (1_103_547, 2_504), "basic2": (9_200_000, 300), "configs2": (2_048, 500_000)}
NAMES = {_capi.JOIN_GENERAL: "general", _capi.JOIN_STREAM: "stream", _capi.JOIN_AUTO: "auto"}
FLIP = np.array([2, 1, 0, 3], dtype=np.uint8)


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


def unpack(h, n):
    return np.stack([(h >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(h.shape[0], -1)[:, :n]


def check(name, parts, sizes, v, flipped, out, n_check):
    rows = np.unique(np.concatenate([[0, v - 1], np.random.default_rng(12345).choice(v, size=min(v, n_check), replace=False)]))
    d_rows = torch.from_numpy(rows).to(out.device)
    cols = []
    for recs, _, n, _ in parts:
        r = (n + 3) // 4
        codes = unpack(recs[: v * r].view(v, r).index_select(0, d_rows).cpu().numpy(), n)
        cols.append(FLIP[codes] if flipped else codes)
    codes = np.concatenate(cols, axis=1)
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
    ap.add_argument("--parts", nargs="+", type=int, default=[2, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=32, help="seeded variants compared with numpy, every byte")
    ap.add_argument("--no-general", action="store_true", help="skip the GENERAL baseline")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("join_bench needs a GPU (the join kernels have no CPU path)")
    dev_name = torch.cuda.get_device_name(0)
    for name in args.shapes:
        v, n = SHAPES[name]
        for n_parts in args.parts:
            sizes = [n // n_parts + (1 if p < n % n_parts else 0) for p in range(n_parts)]
            src = []
            for p, n_p in enumerate(sizes):
                with pgen_rs_amd.GtEngine(n_p, device=0) as part_eng:
                    recs = part_eng.synth_records(v, hwe=True)
                    torch.cuda.synchronize()
                off = torch.arange(v, dtype=torch.int64, device=recs.device) * ((n_p + 3) // 4)
                src.append((recs, off, n_p))
            with pgen_rs_amd.GtEngine(n, device=0) as eng:
                r = eng.record_size
                read_bytes = sum((n_p + 3) // 4 for n_p in sizes) * v
                bound = read_bytes + v * r
                bound_ms = bound / ROOFLINE * 1e3
                big = torch.empty(v * r, dtype=torch.uint8, device=eng.torch_device)
                # the yardsticks, in the same run: the same bytes through device-to-device copies (each part's records into the
                # output buffer), and pack_records DENSE on the joined records
                scratch = torch.empty(read_bytes, dtype=torch.uint8, device=eng.torch_device)

                def copy_all():
                    at = 0
                    for recs, _, n_p in src:
                        nb = v * ((n_p + 3) // 4)
                        scratch[at:at + nb].copy_(recs[:nb])
                        at += nb

                copy_ms = statistics.median(timed(eng, args.steps, args.warmup, copy_all))
                del scratch
                for flipped in (False, True):
                    flip = torch.full((v,), 1 if flipped else 0, dtype=torch.uint8, device=eng.torch_device)
                    parts = [(recs, off, n_p, flip if flipped else None) for recs, off, n_p in src]
                    shapes = [_capi.JOIN_STREAM] + ([] if args.no_general else [_capi.JOIN_GENERAL])
                    for shape in shapes:
                        steps, warmup = (3, 1) if shape == _capi.JOIN_GENERAL else (args.steps, args.warmup)
                        big.fill_(0xA5)
                        ms = timed(eng, steps, warmup, lambda: eng.join_records(parts, v, out=big, shape=shape))
                        med = statistics.median(ms)
                        out = eng.join_records(parts, v, out=big, shape=shape)
                        checked = check(name, parts, sizes, v, flipped, out, args.check_rows)
                        line = {"device": dev_name, "shape": name, "variants": v, "samples": n, "parts": n_parts, "flipped": flipped,
                                "kernel": NAMES[shape], "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": steps,
                                "bound_bytes": bound, "bound_ms": round(bound_ms, 4), "x_bound": round(med / bound_ms, 2),
                                "tb_per_s": round(bound / (med * 1e-3) / 1e12, 3), "d2d_copy_ms": round(copy_ms, 4),
                                "vs_d2d_copy": round(med / copy_ms, 3), "rows_checked": checked}
                        if shape == _capi.JOIN_STREAM and not flipped:
                            packed = torch.empty(v * r, dtype=torch.uint8, device=eng.torch_device)
                            pack_ms = statistics.median(timed(eng, args.steps, args.warmup,
                                                              lambda: eng.pack_records(big, n_variants=v, out=packed, shape=_capi.PACK_DENSE)))
                            line["pack_dense_ms"] = round(pack_ms, 4)
                            del packed
                        print(json.dumps(line), flush=True)
                del big, out, parts
            del src
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
