#!/usr/bin/env python3
"""Times pgenhip_decode_matrix (GtEngine.decode_matrix) on the measurement shapes of tools/scount_bench.py: HWE records synthesised
on the device, a warm-up, then every timed step between its own pair of device events.  One JSON line per shape and form (element
type, orientation, pitch, kernel shape): median / min / max ms, algorithmic bytes V*(R + K*elem_bytes), that traffic's fraction of
the 8 TB/s HBM peak, and decode_emit's (AUTO) median and step-to-step spread on the same records in the same run.
After the timed loop --check-rows seeded variants (and the first and the last) are compared, every sample, with numpy on their record
bytes; a wrong element ends the run with an error.

    python tools/matrix_bench.py [--shapes configs2 c5shard chr22 basic2] [--steps 10] [--warmup 2]
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

PEAK = 8.0e12
# name -> (variants, samples, kept fraction: None = all samples)
SHAPES = {
    "configs2": (100_000, 500_000, None),
    "c5shard": (125_000, 500_000, 0.01),
    "chr22": (1_103_547, 2_504, None),
    "basic2": (9_200_000, 300, None),
}
# (dtype, sample_major, pitch: "dense" | "padded", forced kernel shape, slow: few steps)
STREAM = [(torch.int8, False, "dense", _capi.MATRIX_STREAM, False), (torch.float16, False, "dense", _capi.MATRIX_STREAM, False),
          (torch.float32, False, "dense", _capi.MATRIX_STREAM, False)]
FORMS = {
    "configs2": STREAM + [(torch.int8, True, "padded", _capi.MATRIX_TILE, False), (torch.int8, True, "dense", _capi.MATRIX_TILE, False),
                          (torch.float32, True, "padded", _capi.MATRIX_TILE, False)],
    "chr22": STREAM + [(torch.int8, True, "padded", _capi.MATRIX_TILE, False), (torch.float32, True, "padded", _capi.MATRIX_TILE, False),
                       (torch.int8, True, "dense", _capi.MATRIX_GENERAL, True)],
    "basic2": STREAM,
    "c5shard": [(torch.int8, False, "dense", _capi.MATRIX_GENERAL, True)],
}
NAMES = {_capi.MATRIX_GENERAL: "general", _capi.MATRIX_STREAM: "stream", _capi.MATRIX_TILE: "tile"}


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


def check(name, recs, v, r, n, kept, out, sample_major, n_check):
    rows = np.unique(np.concatenate([[0, v - 1], np.random.default_rng(12345).choice(v, size=min(v, n_check), replace=False)]))
    d_rows = torch.from_numpy(rows).to(recs.device)
    h = recs[: v * r].view(v, r).index_select(0, d_rows).cpu().numpy()
    codes = np.stack([(h >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(rows), -1)[:, :n]
    if kept is not None:
        codes = codes[:, kept.astype(np.int64)]
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32}[out.element_size()]
    want = torch.from_numpy(pgen_rs_amd.GtEngine.matrix_values(out.dtype).copy()).view(it).numpy()[codes]
    got = (out.view(it).index_select(1, d_rows).t() if sample_major else out.view(it).index_select(0, d_rows)).cpu().numpy()
    if not (got == want).all():
        i, k = np.argwhere(got != want)[0]
        raise SystemExit(f"{name}: variant {rows[i]}, kept sample {k}: got {got[i, k]}, numpy {want[i, k]}")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=32, help="seeded variants compared with numpy, every sample")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matrix_bench needs a GPU (the matrix kernels have no CPU path)")
    dev_name = torch.cuda.get_device_name(0)
    for name in args.shapes:
        v, n, frac = SHAPES[name]
        kept = None
        if frac is not None:   # count_bench's c5shard subset
            rng = np.random.default_rng(5)
            kept = np.sort(rng.choice(n, size=int(n * frac), replace=False)).astype(np.uint32)
        with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
            r, k = eng.record_size, eng.kept_count
            recs = eng.synth_records(v, hwe=True)
            # one buffer for every form and for decode_emit's text (configs[2]: 200 GB, only one of them fits beside the records)
            sizes = [v * eng.gt_row_bytes]
            for dtype, sm, pitch, _shape, _slow in FORMS[name]:
                e = torch.empty(0, dtype=dtype).element_size()
                rows, cols = (k, v) if sm else (v, k)
                sizes.append(rows * ((cols * e + 127) // 128 * 128 if pitch == "padded" else cols * e))
            big = torch.empty(max(sizes), dtype=torch.uint8, device=eng.torch_device)
            emit_ms = timed(eng, args.steps, args.warmup, lambda: eng.decode_emit(recs, v, out=big))
            emit_med = statistics.median(emit_ms)
            emit_spread = (max(emit_ms) - min(emit_ms)) / emit_med
            for dtype, sm, pitch, shape, slow in FORMS[name]:
                e = torch.empty(0, dtype=dtype).element_size()
                rows, cols = (k, v) if sm else (v, k)
                pitch_e = (cols * e + 127) // 128 * 128 // e if pitch == "padded" else cols
                out = torch.as_strided(big[: rows * pitch_e * e].view(dtype), (rows, cols), (pitch_e, 1))
                steps, warmup = (2, 1) if slow else (args.steps, args.warmup)
                ms = timed(eng, steps, warmup, lambda: eng.decode_matrix(recs, v, out=out, sample_major=sm, kernel=shape))
                med = statistics.median(ms)
                checked = check(name, recs, v, r, n, kept, out, sm, args.check_rows)
                alg = v * (r + k * e)
                print(json.dumps({"device": dev_name, "shape": name, "variants": v, "samples": n, "kept": k, "kernel": NAMES[shape],
                                  "dtype": str(dtype).replace("torch.", ""), "sample_major": sm, "pitch_bytes": pitch_e * e,
                                  "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": steps,
                                  "alg_bytes": alg, "tb_per_s": round(alg / (med * 1e-3) / 1e12, 3),
                                  "frac_of_8tbs": round(alg / (med * 1e-3) / PEAK, 3),
                                  "decode_emit_ms": round(emit_med, 4), "decode_emit_spread": round(emit_spread, 4),
                                  "vs_decode_emit": round(med / emit_med, 3), "rows_checked": checked}), flush=True)
            del recs, big, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
