"""bench.py --dump-outputs: what the last timed step wrote, dumped as float32 text bytes at float64 byte offsets, must be
byte-equal to the oracle's GT text of the same seeded workload at those offsets — sampled or whole, in one launch per step
or in several (the samples of the earlier launches are gathered inside the step, before `out` is re-used)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pgen_oracle as oracle

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("config,n,v,keep_mod,max_launch", [
    ("chr22", 2504, 3001, 0, 0),      # 30 MB of text: a seeded sample of it, one launch per step
    ("chr22", 2504, 3001, 7, 700),    # 1/7 of the samples kept, five launches per step
    ("basic2", 300, 1000, 0, 0),      # 1.2 MB of text: every byte
])
def test_dump_outputs_equal_the_oracle(tmp_path, config, n, v, keep_mod, max_launch):
    p = subprocess.run([sys.executable, str(REPO / "bench.py"), "--config", config, "--variants", str(v), "--keep-modulus", str(keep_mod),
                        "--max-launch-variants", str(max_launch), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--no-host-delivered", "--no-live-traffic", "--no-secondary", "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=600, cwd=str(REPO))
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["self_check"]["ok"]
    if max_launch:
        assert line["config"]["launches_per_step"] > 1
    dump = line["dump_outputs"]
    assert dump["files"] == ["gt_text.npy", "gt_text_offset.npy"]
    assert sum(f.stat().st_size for f in (tmp_path / "dump").iterdir()) <= 64e6
    vals = np.load(tmp_path / "dump" / "gt_text.npy")
    offs = np.load(tmp_path / "dump" / "gt_text_offset.npy")
    assert vals.dtype == np.float32 and offs.dtype == np.float64 and vals.shape == offs.shape == (dump["bytes_sampled"],)

    kept = oracle.synth_keep(n, modulus=keep_mod) if keep_mod else None
    want = oracle.decode_emit(oracle.synth_records(n, v), v, n, kept_idx=kept)
    assert dump["text_bytes"] == want.size
    o = offs.astype(np.int64)
    assert np.all(np.diff(o) > 0) and 0 <= o[0] and o[-1] < want.size
    if want.size <= 1 << 22:
        assert o.size == want.size
    else:
        assert o.size > 1 << 21 and np.unique(o // dump["row_bytes"]).size == v  # every variant's row is sampled
    assert np.array_equal(vals, want[o].astype(np.float32))
