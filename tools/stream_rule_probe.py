#!/usr/bin/env python3
"""The stream kernel's launch rule (plan::wide::rule), measured as ONE grid: store policy x write fronts x blocks per CU x burst, all
arms interleaved in one process per shape, through pgenhip_decode_emit with AUTO dispatch.

    python tools/stream_rule_probe.py                          # every shape of profiles/r05_stream_rule.md, one child process each
    python tools/stream_rule_probe.py --only chr22 "N=2504 2 GB"
    python tools/stream_rule_probe.py --shape 2504:1103547 --allocations 4     # one shape in this process

The parent never touches the GPU: it runs each shape as a child under `timeout` and stops at the first non-zero status.  In a child
all arms write the SAME record allocation and the same output allocation, round-robin (the method of tools/store_policy_probe.py:
placement cancels), and every timing is the median over the rounds:
  single  one call between a synchronize and an event pair;
  b2b     several calls in a row on one stream, one event pair around all of them, per call: what bench.py sees.
Arm 0 is the library's own rule (every knob at 0); the deltas are against it and `spread` is max - min of its b2b timings, so an arm
is ahead only where its delta is below minus that spread.  With --allocations A the whole grid runs on A separate output allocations
(held together, as tools/placement_probe.py does), which shows whether an arm also closes the placement spread.  Compare arms within
one run, never across runs.  Prints markdown tables; --json keeps every number.
"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (label, N, V, keep modulus, allocations, seconds allowed)
SHAPES = [
    ("c3 (212 GB)", 500_000, 100_000, 0, 1, 600),
    ("N=500000 12 GB", 500_000, 5_650, 0, 1, 240),
    ("N=20000 12 GB", 20_000, 141_000, 0, 1, 240),
    ("chr22 (11.7 GB)", 2_504, 1_103_547, 0, 4, 400),
    ("N=2504 2 GB", 2_504, 188_000, 0, 1, 200),
    ("N=2504 4 GB", 2_504, 376_000, 0, 1, 200),
    ("N=1916 12 GB", 1_916, 1_473_000, 0, 1, 240),
    ("K=4940 0.5 GB (second pass of c5shard)", 4_940, 25_000, 0, 1, 200),
    ("N=300 RUNS 255 MB", 300, 200_000, 0, 1, 200),
    ("N=300 RUNS 11 GB", 300, 8_620_000, 0, 1, 240),
]


def child(args):
    import torch

    import pgen_rs_amd
    from pgen_rs_amd import _capi
    from pgen_rs_amd.synth import keep_indices

    n, v, modulus = args.shape
    runs = n < 1916                     # AUTO: the RUNS mode, which has no burst
    bursts = args.bursts if not runs else [0]
    # arm = (policy, fronts, blocks per CU, burst); 0 = the rule's choice
    arms = [(0, 0, 0, 0)] + [(p, f, b, u) for p, f, b, u in itertools.product(args.policies, args.fronts, args.blocks, bursts)]
    kept = keep_indices(n, modulus=modulus) if modulus else None
    eng = pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0)

    def set_arm(arm):
        eng.tune(_capi.KNOB_STORE_POLICY, arm[0])
        eng.tune(_capi.KNOB_WIDE_RANGES, arm[1])
        eng.tune(_capi.KNOB_WIDE_BLOCKS_PER_CU, arm[2])
        eng.tune(_capi.KNOB_WIDE_BURST, arm[3])

    recs = eng.synth_records(v)
    outs = [torch.empty(v * eng.gt_row_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(args.allocations)]   # held together
    alg = v * (eng.record_size + eng.gt_row_bytes)
    result = {"shape": args.label, "samples": n, "variants": v, "algorithmic_bytes": alg, "device": torch.cuda.get_device_name(0),
              "rounds": args.rounds, "arms": [list(a) for a in arms], "allocations": []}

    def timed(out, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            eng.decode_emit(recs, v, out=out)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for ai, out in enumerate(outs):
        digests = []
        for arm in arms:                     # warm-up, and the arms agree on every output byte's sum
            set_arm(arm)
            out.zero_()
            eng.decode_emit(recs, v, out=out)
            torch.cuda.synchronize()
            digests.append(int(out[: out.numel() // 8 * 8].view(torch.int64).sum().item()))
        if len(set(digests)) != 1:
            print(f"!! {args.label}: the arms' outputs differ: {[a for a, d in zip(arms, digests) if d != digests[0]]}", flush=True)
            return 3
        set_arm(arms[0])
        once = timed(out, 1)
        reps = max(2, min(10, int(args.budget_ms / max(once, 1e-3))))
        single = [[] for _ in arms]
        b2b = [[] for _ in arms]
        for _ in range(args.rounds):
            for i, arm in enumerate(arms):
                set_arm(arm)
                single[i].append(timed(out, 1))
            for i, arm in enumerate(arms):
                set_arm(arm)
                b2b[i].append(timed(out, reps))
        med = statistics.median
        s = [med(x) for x in single]
        t = [med(x) for x in b2b]
        spread = max(b2b[0]) - min(b2b[0])
        result["allocations"].append({"address": hex(out.data_ptr()), "reps": reps, "single_ms": s, "b2b_ms": t, "b2b_all_ms": b2b,
                                      "rule_b2b_spread_ms": spread})
        print(f"\n#### {args.label}, allocation {ai} at {hex(out.data_ptr())}: {alg / 1e9:.3f} GB algorithmic; rule arm single {s[0] * 1e3:.1f} us, "
              f"b2b {t[0] * 1e3:.1f} us = {alg / t[0] / 1e6:.0f} GB/s, b2b spread {spread * 1e3:.1f} us ({spread / t[0] * 100:.2f} %), {reps} calls per b2b timing\n")
        print("| policy | fronts | blocks/CU | " + " | ".join(f"burst {u}: single us | b2b us | b2b delta" for u in bursts) + " |")
        print("|---|---|---|" + "---|---|---|" * len(bursts))
        for p, f, b in itertools.product(args.policies, args.fronts, args.blocks):
            cells = []
            for u in bursts:
                i = arms.index((p, f, b, u))
                cells.append(f"{s[i] * 1e3:.1f} | {t[i] * 1e3:.1f} | {(t[i] / t[0] - 1) * 100:+.2f} %")
            print(f"| {p} | {f} | {b} | " + " | ".join(cells) + " |")
        best = min(range(len(arms)), key=lambda i: t[i])
        print(f"\nbest b2b: arm {arms[best]} {t[best] * 1e3:.1f} us ({(t[best] / t[0] - 1) * 100:+.2f} %)", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh)
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, help="labels (or their first words) of the shapes to run")
    ap.add_argument("--shape", default=None, metavar="N:V[:M]", help="run this one shape in this process")
    ap.add_argument("--label", default=None)
    ap.add_argument("--allocations", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--budget-ms", type=float, default=20.0, help="time of one back-to-back timing (sets the calls per timing, 2 .. 10)")
    ap.add_argument("--policies", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--fronts", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--blocks", type=int, nargs="*", default=[2, 3, 4])
    ap.add_argument("--bursts", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--json", default=None, help="child: file for every number; parent: directory for one file per shape")
    args = ap.parse_args()
    if args.shape:
        f = [int(x) for x in args.shape.split(":")]
        args.shape = (f[0], f[1], f[2] if len(f) > 2 else 0)
        args.label = args.label or f"N={f[0]} V={f[1]}"
        return child(args)
    picked = [s for s in SHAPES if args.only is None or any(s[0].startswith(o) for o in args.only)]
    if args.json:
        os.makedirs(args.json, exist_ok=True)
    for i, (label, n, v, m, allocations, seconds) in enumerate(picked):
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--shape", f"{n}:{v}:{m}", "--label", label,
               "--allocations", str(allocations), "--rounds", str(args.rounds), "--budget-ms", str(args.budget_ms),
               "--policies", *map(str, args.policies), "--fronts", *map(str, args.fronts), "--blocks", *map(str, args.blocks),
               "--bursts", *map(str, args.bursts)]
        if args.json:
            cmd += ["--json", os.path.join(args.json, f"shape_{SHAPES.index(picked[i])}.json")]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"!! {label}: status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
