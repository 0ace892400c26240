#!/usr/bin/env python3
"""Times pgenhip_parse_gt (GtEngine.parse_gt) on the measurement shapes chr22 / basic2 and one block of configs[2]: HWE records
synthesised on the device, their text made by decode_emit (the fixed-width text the FIXED shape takes), a warm-up, then every
timed step between its own pair of device events.  One JSON line per shape and parse shape (fixed = forced FIXED, its validate and
write passes; general; auto = one FIXED pass and the GENERAL pass over the declined lines, none here): median / min / max ms, the
byte bound (4N + R bytes per line: the text read once, the record written once) at 8 TB/s, the ratio to it, and decode_emit's time
on the same rows, measured in the same run, with the ratio to that.  After the timed loop the records of every shape are compared
with the records the text was made from (pad bits are zero in both).

    python tools/parse_bench.py [--shapes chr22 basic2 configs2] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import torch

import pgen_rs_amd
from pgen_rs_amd import _capi

PEAK = 8.0e12
SHAPES = {"chr22": (1_103_547, 2_504), "basic2": (9_200_000, 300), "configs2": (2_048, 500_000)}   # configs2: one block of its rows
NAMES = {_capi.PARSE_FIXED: "fixed", _capi.PARSE_GENERAL: "general", _capi.PARSE_AUTO: "auto"}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--general-steps", type=int, default=3, help="timed steps of the GENERAL baseline")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("parse_bench needs a GPU (the parse kernels have no CPU path)")
    dev_name = torch.cuda.get_device_name(0)
    for name in args.shapes:
        v, n = SHAPES[name]
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            r = eng.record_size
            recs = eng.synth_records(v, hwe=True)
            text = torch.empty(v * (4 * n + 1), dtype=torch.uint8, device=eng.torch_device)
            emit_ms = statistics.median(timed(eng, args.steps, args.warmup, lambda: eng.decode_emit(recs, v, out=text)))
            field_off = torch.arange(v, dtype=torch.int64, device=eng.torch_device) * (4 * n + 1)
            line_end = field_off + 4 * n
            out = torch.empty(v * r, dtype=torch.uint8, device=eng.torch_device)
            flags = torch.empty(v, dtype=torch.int32, device=eng.torch_device)
            bound = v * (4 * n + r)
            bound_ms = bound / PEAK * 1e3
            for shape in (_capi.PARSE_FIXED, _capi.PARSE_AUTO, _capi.PARSE_GENERAL):
                steps = args.general_steps if shape == _capi.PARSE_GENERAL else args.steps
                out.fill_(0xA5)
                run = lambda: eng.parse_gt(text, field_off, line_end, out=out, line_flags=flags, shape=shape)
                ms = timed(eng, steps, min(args.warmup, steps), run)
                med = statistics.median(ms)
                eng.wait()
                if not torch.equal(out, recs.view(-1)[: v * r]) or bool(flags.any()):
                    raise SystemExit(f"{name} {NAMES[shape]}: records or flags differ from the records the text was made from")
                print(json.dumps({"device": dev_name, "shape": name, "lines": v, "samples": n, "kernel": NAMES[shape], "shape_id": shape,
                                  "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": steps,
                                  "bound_bytes": bound, "bound_ms": round(bound_ms, 4), "of_bound": round(bound_ms / med, 3),
                                  "tb_per_s": round(bound / (med * 1e-3) / 1e12, 3), "decode_emit_ms": round(emit_ms, 4),
                                  "vs_decode_emit": round(med / emit_ms, 3)}), flush=True)
            del recs, text, out, flags, field_off, line_end
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
