"""The stream kernel's launch rule (plan::wide::rule of csrc/launch_plan.h, run through tests/wide_plan.py): both sides of every
threshold it contains, every forced knob, the launches of the seven bench.py presets, and equality with a literal copy of the
choices the launchers made before the rule moved into the plan header (`legacy` below) everywhere but in the two branches that
profiles/r05_stream_rule.md measured in afterwards (`expect` states them on top of the copy).  No GPU."""
import itertools

import pytest

import wide_plan as W
from pgen_rs_amd.synth import keep_indices

GB = 10 ** 9


def legacy(text, spans, need, runs=False, occupancy=4, num_cus=256, policy=0, blocks_per_cu=0, fronts=0):
    """launch_gt_wide / launch_gt_runs as they chose before plan::wide::rule existed, line by line (they had no burst knob: always 2)."""
    if runs:
        pol = 2 if policy == 2 else 1
        per_cu = blocks_per_cu if blocks_per_cu > 0 else 2
        return W.Rule(pol, 2, per_cu, fronts if fronts > 0 else 2, min(need, num_cus * per_cu))
    wt_rule = text > 1_000_000_000 and (spans > 1 or text <= 4_500_000_000)
    wt = wt_rule if policy == 0 else policy == 2
    per_cu = occupancy
    if text <= 1_000_000_000 and per_cu > 2:
        per_cu = 2
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    g = min(need, num_cus * per_cu)
    return W.Rule(2 if wt else 1, 2, per_cu, fronts if fronts > 0 else (8 if spans > 1 and need >= 64 * g else 2), g)


def expect(text, spans, need, burst=0, **kw):
    """LEGACY, and on it the two branches that profiles/r05_stream_rule.md measured in: everything else must equal the old choice."""
    want = legacy(text, spans, need, **kw)
    runs = kw.get("runs", False)
    # rows of several spans from 9 GB of text: single store steps
    if not runs and spans > 1 and text >= 9_000_000_000:
        want = want._replace(burst=1)
    # RUNS above 3 GB of text: every resident block and eight fronts
    if runs and text > 3_000_000_000:
        per_cu = kw.get("blocks_per_cu", 0) or kw.get("occupancy", 4)
        want = want._replace(blocks_per_cu=per_cu, grid=min(need, kw.get("num_cus", 256) * per_cu), fronts=kw.get("fronts", 0) or 8)
    if burst:
        want = want._replace(burst=burst)
    return want


def test_constants():
    assert (W.THREADS, W.STORERS, W.SPAN_CHUNKS, W.NT, W.WT) == (512, 7, 1024, 1, 2)
    assert W.SHORT_LAUNCH_BYTES == 1_000_000_000 and W.WT_ONE_SPAN_MAX_BYTES == 4_500_000_000 and W.FRONT_STEPS == 64
    assert W.BURST_ONE_MIN_BYTES == 9_000_000_000 and W.RUNS_LONG_BYTES == 3_000_000_000


def test_spans_and_steps():
    # a row owns ceil(S / 16) + 1 chunks at most and its first span starts up to 63 chunks before them: 1 024 chunks per span
    for n, spans in ((1024, 1), (2504, 1), (3839, 1), (3840, 2), (4940, 2), (20_000, 5), (500_000, 123)):
        assert W.spans_per_row(4 * n + 1) == spans, n
    assert [W.steps(i) for i in (1, 7, 8, 14, 15)] == [1, 1, 2, 2, 3]


@pytest.mark.parametrize("spans", [1, 2])
def test_size_thresholds(spans):
    """Text bytes -1, 0, +1 around each size constant, rows of one span and of two."""
    need = 10 ** 6
    for text in (c + d for c in (W.SHORT_LAUNCH_BYTES, W.WT_ONE_SPAN_MAX_BYTES, W.BURST_ONE_MIN_BYTES, W.RUNS_LONG_BYTES) for d in (-1, 0, 1)):
        got = W.rule(text, spans, need)
        assert got == expect(text, spans, need), (text, spans)
        assert W.kernel_choice(text, spans) == (got.policy, got.burst)
    # short: two blocks per CU and nt stores up to the constant, the occupancy figure and write-through right above it
    assert W.rule(W.SHORT_LAUNCH_BYTES, spans, need)[:3] == (W.NT, 2, 2) and W.rule(W.SHORT_LAUNCH_BYTES + 1, spans, need)[:3] == (W.WT, 2, 4)
    assert W.rule(W.WT_ONE_SPAN_MAX_BYTES, spans, need).policy == W.WT and W.rule(W.WT_ONE_SPAN_MAX_BYTES + 1, spans, need).policy == (W.NT if spans == 1 else W.WT)
    # single store steps from the constant on, for rows of several spans only
    assert W.rule(W.BURST_ONE_MIN_BYTES - 1, spans, need).burst == 2 and W.rule(W.BURST_ONE_MIN_BYTES, spans, need).burst == (2 if spans == 1 else 1)
    for occupancy in (1, 2, 3, 4):
        assert W.rule(W.SHORT_LAUNCH_BYTES, spans, need, occupancy=occupancy).blocks_per_cu == min(occupancy, 2)
        assert W.rule(W.SHORT_LAUNCH_BYTES + 1, spans, need, occupancy=occupancy).blocks_per_cu == occupancy


def test_front_rule_bound():
    """Eight fronts for rows of several spans from FRONT_STEPS steps per block, on either side of the bound and of the grid cap."""
    for text, per_cu in ((12 * GB, 4), (GB // 2, 2)):
        cap = 256 * per_cu
        for need in (cap * W.FRONT_STEPS - 1, cap * W.FRONT_STEPS, cap * W.FRONT_STEPS + 1):
            for spans in (1, 2):
                got = W.rule(text, spans, need)
                assert got == expect(text, spans, need), (text, spans, need)
                assert got.grid == cap
        # a grid below the cap: the bound follows the grid
        for need in (1, 63, 64, cap - 1, cap):
            got = W.rule(text, 2, need)
            assert got.grid == need and got == expect(text, 2, need)
    assert W.rule(12 * GB, 2, 1024 * 64).fronts == 8 and W.rule(12 * GB, 2, 1024 * 64 - 1).fronts == 2


def test_forced_knobs_override_the_rule():
    for text, spans in itertools.product((GB // 2, 2 * GB, 12 * GB), (1, 2)):
        need = 10 ** 6
        base = W.rule(text, spans, need)
        for policy in (1, 2):
            got = W.rule(text, spans, need, policy=policy)
            assert got == base._replace(policy=policy) and W.kernel_choice(text, spans, policy=policy)[0] == policy
        for per_cu in (1, 2, 3, 4, 7):
            got = W.rule(text, spans, need, blocks_per_cu=per_cu)
            assert got.blocks_per_cu == per_cu and got.grid == 256 * per_cu and got == expect(text, spans, need, blocks_per_cu=per_cu)
        for fronts in (1, 2, 4, 8, 16, 64):
            assert W.rule(text, spans, need, fronts=fronts) == base._replace(fronts=fronts)
        for cus in (1, 256, 304):
            assert W.rule(text, spans, need, num_cus=cus).grid == cus * base.blocks_per_cu
        for burst in (1, 2):
            assert W.rule(text, spans, need, burst=burst) == base._replace(burst=burst) and W.kernel_choice(text, spans, burst=burst)[1] == burst
    # RUNS: nt; two blocks per CU and two fronts up to RUNS_LONG_BYTES, the occupancy figure and eight fronts above; unless forced
    for text in (GB // 4, 2 * GB, W.RUNS_LONG_BYTES):
        assert W.rule(text, 1, 10 ** 6, runs=True, occupancy=3) == W.Rule(W.NT, 2, 2, 2, 512) == expect(text, 1, 10 ** 6, runs=True, occupancy=3)
        assert W.rule(text, 1, 10 ** 6, runs=True, occupancy=1) == W.Rule(W.NT, 2, 2, 2, 512) == expect(text, 1, 10 ** 6, runs=True, occupancy=1)   # two, whatever the figure
    for text in (W.RUNS_LONG_BYTES + 1, 11 * GB):
        assert W.rule(text, 1, 10 ** 6, runs=True, occupancy=3) == W.Rule(W.NT, 2, 3, 8, 768) == expect(text, 1, 10 ** 6, runs=True, occupancy=3)
        assert W.rule(text, 1, 10 ** 6, runs=True, occupancy=2).blocks_per_cu == 2
    for text in (GB // 4, 11 * GB):
        got = W.rule(text, 1, 10 ** 6, runs=True, occupancy=3, policy=2, blocks_per_cu=1, fronts=16)
        assert got == W.Rule(W.WT, 2, 1, 16, 256) == expect(text, 1, 10 ** 6, runs=True, occupancy=3, policy=2, blocks_per_cu=1, fronts=16)
    assert W.rule(1201 * 5, 1, 1, runs=True).grid == 1


K5 = len(keep_indices(500_000, modulus=100))   # the kept samples of configs[4]: the second pass of the two passes runs on rows of K5 samples

# preset -> (samples of the stream kernel's rows, rows per launch, RUNS rows per item): the launches bench.py makes on one MI355X
# (c4 and c5 are cut into eight ranks' shards, which are the c4shard and c5shard launches; the second pass of c5 runs in chunks of as
# many compact records as 32 MiB hold, rounded down to whole rounds of the compact pass)
PRESET_LAUNCHES = {
    "c3": (500_000, 100_000, 0),
    "chr22": (2_504, 1_103_547, 0),
    "c4": (500_000, 125_000, 0),
    "c4shard": (500_000, 125_000, 0),
    "c5": (K5, (32 << 20) // ((K5 + 3) // 4), 0),
    "c5shard": (K5, (32 << 20) // ((K5 + 3) // 4), 0),
    "basic2": (300, 200_000, 12),
}
PRESET_RULES = {
    "c3": W.Rule(W.WT, 1, 4, 8, 1024),
    "chr22": W.Rule(W.NT, 2, 4, 2, 1024),
    "c4": W.Rule(W.WT, 1, 4, 8, 1024),
    "c4shard": W.Rule(W.WT, 1, 4, 8, 1024),
    "c5": W.Rule(W.NT, 2, 2, 2, 512),
    "c5shard": W.Rule(W.NT, 2, 2, 2, 512),
    "basic2": W.Rule(W.NT, 2, 2, 2, 512),
}


@pytest.mark.parametrize("preset", sorted(PRESET_LAUNCHES))
def test_bench_presets(preset):
    n, v, runs_rows = PRESET_LAUNCHES[preset]
    got = W.launch(n, v, runs_rows)
    assert got == PRESET_RULES[preset]
    row = 4 * n + 1
    spans = 1 if runs_rows else W.spans_per_row(row)
    need = W.steps(-(-v // runs_rows) if runs_rows else v * spans)
    assert got == expect(v * row, spans, need, runs=bool(runs_rows), occupancy=3 if runs_rows else 4)
    if preset.startswith("c5"):
        assert 4_500 < n < 5_500 and spans == 2
        # any chunk the two passes cut (down to a few thousand rows) is a short launch of the same class
        assert W.launch(n, 20_000)[:4] == got[:4]


def test_rule_equals_legacy_on_a_grid():
    """Every class of input at once: sizes around the constants x spans x steps x occupancy x knobs."""
    sizes = [1, GB // 2, GB, GB + 1, 2 * GB, 3 * GB, 3 * GB + 1, 4_500_000_000, 4_500_000_001, 9 * GB - 1, 9 * GB, 12 * GB, 212 * GB]
    for text, spans, need, occupancy in itertools.product(sizes, (1, 2, 123), (1, 500, 1024 * 64 - 1, 1024 * 64, 10 ** 7), (2, 4)):
        for kw in ({}, {"policy": 1}, {"policy": 2}, {"blocks_per_cu": 3}, {"fronts": 4}, {"num_cus": 304}, {"burst": 1}, {"burst": 2}):
            assert W.rule(text, spans, need, occupancy=occupancy, **kw) == expect(text, spans, need, occupancy=occupancy, **kw)
            if spans == 1:
                kw = {k: v for k, v in kw.items() if k != "burst"}   # (RUNS has no burst)
                assert W.rule(text, 1, need, runs=True, occupancy=min(occupancy, 3), **kw) == expect(text, 1, need, runs=True, occupancy=min(occupancy, 3), **kw)
