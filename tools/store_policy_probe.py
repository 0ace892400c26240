#!/usr/bin/env python3
"""Store policy of the emit kernels, interleaved in one process: non-temporal stores (knob 1) against non-temporal
write-through stores (knob 2, `sc1 nt`) through pgenhip_decode_emit, AUTO dispatch.

    python tools/store_policy_probe.py                       # the sizes of profiles/r04_short_launches.md
    python tools/store_policy_probe.py --shapes 300:200000   # N:V[:keep modulus]

Both arms write the SAME record and output allocation, round-robin (the method of tools/ab_probe.py: process-to-process
placement cancels).  Two timings per arm and size, each the median over the rounds:
  single  one call between a synchronize and an event pair: the launch on an idle chip, its ramp, tail and whatever the
          stop event waits for at the kernel's end;
  b2b     several calls in a row on one stream, one event pair around all of them, per call: what bench.py sees; a flush
          that lands in the gap behind a kernel shows here and not in `single`.
Prints one markdown table row per size.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pgen_rs_amd
from pgen_rs_amd import _capi
from pgen_rs_amd.synth import keep_indices

# (label, N, V, keep modulus)
DEFAULT = [
    ("N=300 134 MB", 300, 105_000, 0),
    ("N=300 255 MB (basic2)", 300, 200_000, 0),
    ("N=300 1 GB", 300, 785_000, 0),
    ("N=4940 0.5 GB (config 5, second pass)", 4_940, 25_000, 0),
    ("N=2504 134 MB", 2_504, 12_600, 0),
    ("N=2504 2 GB", 2_504, 188_000, 0),
    ("N=2504 11.7 GB (chr22)", 2_504, 1_103_547, 0),
    ("N=500000 12 GB", 500_000, 5_650, 0),
    ("c5shard (125000 x 500000, 1 % kept)", 500_000, 125_000, 100),
]


def probe(label, n, v, modulus, rounds, budget_ms):
    kept = keep_indices(n, modulus=modulus) if modulus else None
    arms = []
    for name, policy in (("nt", 1), ("nt sc1", 2)):
        eng = pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0)
        eng.tune(_capi.KNOB_STORE_POLICY, policy)
        arms.append((name, eng))
    e0 = arms[0][1]
    recs = e0.synth_records(v)
    out = torch.empty(v * e0.gt_row_bytes, dtype=torch.uint8, device="cuda:0")
    alg = v * (e0.record_size + e0.gt_row_bytes)
    digests = []
    for _, eng in arms:                      # warm-up, and the arms agree on every output byte's sum
        out.zero_()
        eng.decode_emit(recs, v, out=out)
        torch.cuda.synchronize()
        digests.append(int(out[: out.numel() // 8 * 8].view(torch.int64).sum().item()))
    if digests[0] != digests[1]:
        print(f"!! {label}: the arms' outputs differ")

    def timed(eng, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            eng.decode_emit(recs, v, out=out)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    once = timed(e0, 1)
    reps = max(2, min(20, int(budget_ms / max(once, 1e-3))))
    single = {name: [] for name, _ in arms}
    b2b = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, eng in arms:
            single[name].append(timed(eng, 1))
        for name, eng in arms:
            b2b[name].append(timed(eng, reps))
    med = statistics.median
    s1, s2, t1, t2 = med(single["nt"]), med(single["nt sc1"]), med(b2b["nt"]), med(b2b["nt sc1"])
    spread = max(b2b["nt"]) - min(b2b["nt"])
    print(f"| {label} | {alg / 1e9:.3f} | {s1 * 1e3:.1f} | {s2 * 1e3:.1f} | {(s2 / s1 - 1) * 100:+.1f} % | {t1 * 1e3:.1f} | {t2 * 1e3:.1f} | "
          f"{(t2 / t1 - 1) * 100:+.1f} % | {spread * 1e3:.1f} | {reps} |", flush=True)
    del recs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None, metavar="N:V[:M]")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--budget-ms", type=float, default=40.0, help="time of one back-to-back timing (sets the calls per timing, 2 .. 20)")
    args = ap.parse_args()
    shapes = DEFAULT
    if args.shapes:
        shapes = []
        for spec in args.shapes:
            f = [int(x) for x in spec.split(":")]
            shapes.append((spec, f[0], f[1], f[2] if len(f) > 2 else 0))
    print(f"device: {torch.cuda.get_device_name(0)}; times in us, medians of {args.rounds} rounds; spread = max - min of the nt arm's back-to-back timings")
    print("| size | GB algorithmic | single nt | single nt sc1 | delta | b2b nt | b2b nt sc1 | delta | b2b spread nt | calls per b2b timing |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for label, n, v, m in shapes:
        probe(label, n, v, m, args.rounds, args.budget_ms)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
