"""AUTO for all samples kept (plan::emit::choose_all_samples of csrc/launch_plan.h, run through tests/subset_plan.py): equality with
a literal copy of the chain and of the predicates it asks, as capi.hip and the launchers stated them before they moved into the plan
header (`legacy` below), at N - 1, N, N + 1 around every sample threshold, for full lines and GT segments, dense / gathered / padded
records, dense / padded output and prefixes on both sides of the line-run kernel's limits.  Every bench.py preset goes through this
chain.  No GPU."""
import itertools

import pytest

import subset_plan as SP

# the literals of the chain and its predicates: 8 (FLAT, RUNS, line runs), 61 (R = 16: the pick family), 1 000 (line runs), 1 024 (the
# stream kernel), 1 400 (full lines through it), 1 915 / 1 916 (two rows per run -> one), 2 000 (pick -> stream kernel on gathered
# rows), 3 831 / 3 832 (one row per run -> none), 4 096 (the pick family's table); 539 .. 592: a run of full lines goes from seven
# lines to six (by its span at P = 0, by its record load for short prefixes)
LITERALS = (8, 61, 1000, 1024, 1400, 1915, 1916, 2000, 3831, 3832, 4096)
NS = sorted({n + d for n in LITERALS for d in (-1, 0, 1)} | set(range(530, 600)) | {1, 100, 300, 2504, 5000, 500_000})
PREFIXES = (0, 30, 94, 95, 166, 250, 251)


def legacy(n, v, lines, gathered, records_dense, out_dense, p, prefix_off=True, counters=True):
    """choose_all_samples with gt_*_applicable / _preferred / gt_lineruns_rows behind it, line by line as in the commit before
    plan::emit (kept_idx == nullptr, K = N; a.work_counters and a.prefix_off set, as emit_core always had them by then)."""
    k, r = n, (2 * n + 7) // 8
    records_dense = v <= 1 or records_dense          # a.n_variants <= 1 || a.record_stride == a.record_size
    out_dense = v <= 1 or out_dense                  # a.n_variants <= 1 || a.out_stride == 4K + 1
    max_line_bytes = p + 4 * k + 1 if lines else 0

    def run_rows_for():
        if r == 0:
            return 0
        s = 4 * k + 1
        by_load, by_span = 1040 // r, 15328 // s
        return by_load if by_load < by_span else by_span

    def lineruns_rows_for():
        if r == 0 or max_line_bytes == 0 or max_line_bytes > 15328:
            return 0
        max_prefix = max_line_bytes - (4 * k + 1)
        b = 1040 // r
        b = min(b, 15328 // max_line_bytes)
        b = min(b, 30)
        if max_prefix:
            b = min(b, (768 - 16) // max_prefix - (1 if (768 - 16) // max_prefix else 0))
        return b

    def gt_wide_lines_applicable():
        return lines and prefix_off and n >= 1024 and counters

    def gt_lineruns_applicable():
        return n >= 8 and lines and prefix_off and not gathered and records_dense and counters and lineruns_rows_for() >= 2

    def gt_pick_applicable():
        return n <= 4096 and r >= 16 and k >= 1 and (lines or out_dense)

    def gt_runs_applicable():
        return not lines and not gathered and n >= 8 and (v <= 1 or (out_dense and records_dense)) and counters and run_rows_for() >= 1

    def gt_wide_applicable():
        return not lines and n >= 1024 and out_dense

    def gt_flat_applicable():
        return not lines and n >= 8 and out_dense

    if lines:
        if gt_wide_lines_applicable() and n >= 1400:
            return "wide"
        if gt_lineruns_applicable() and lineruns_rows_for() >= 7 and n < 1000:
            return "lineruns"
        if gt_pick_applicable():
            return "pick"
        return "rows"
    if gt_runs_applicable() and run_rows_for() >= 2:
        return "runs"
    if gt_pick_applicable() and n < 2000:
        return "pick"
    if gt_wide_applicable():
        return "wide"
    if gt_flat_applicable():
        return "flat"
    return "rows"


RECORDS = {"dense": dict(gathered=False, records_dense=True), "gathered": dict(gathered=True, records_dense=True),
           "padded": dict(gathered=False, records_dense=False)}


@pytest.mark.parametrize("records", sorted(RECORDS))
def test_full_lines_equal_the_legacy_chain(records):
    for n, p, v in itertools.product(NS, PREFIXES, (1, 2, 1000)):
        got = SP.choose_all_samples(n, v, lines=True, bound=p, out_dense=False, **RECORDS[records])   # (full lines have no pitch)
        assert got == legacy(n, v, True, p=p, out_dense=False, **RECORDS[records]), (n, p, v)


@pytest.mark.parametrize("records", sorted(RECORDS))
@pytest.mark.parametrize("out_dense", [True, False])
def test_gt_segments_equal_the_legacy_chain(records, out_dense):
    for n, v in itertools.product(NS, (1, 2, 1000)):
        got = SP.choose_all_samples(n, v, out_dense=out_dense, **RECORDS[records])
        assert got == legacy(n, v, False, p=0, out_dense=out_dense, **RECORDS[records]), (n, v)


def test_the_chain_at_its_thresholds():
    """The arms themselves, so that the copy above cannot drift with the header unnoticed."""
    seg = lambda n, **kw: SP.choose_all_samples(n, 1000, **kw)                          # noqa: E731
    lin = lambda n, p=30, **kw: SP.choose_all_samples(n, 1000, lines=True, bound=p, **kw)   # noqa: E731
    # GT segments, dense: rows below 8 samples, runs of rows to 1 915, the pick family to 1 999, the stream kernel from 2 000
    assert [seg(n) for n in (7, 8, 1915, 1916, 1999, 2000, 3831, 3832, 500_000)] == ["rows", "runs", "runs", "pick", "pick", "wide", "wide", "wide", "wide"]
    # gathered rows: flat below R = 16, the pick family to 1 999
    assert [seg(n, gathered=True) for n in (7, 8, 60, 61, 1999, 2000)] == ["rows", "flat", "flat", "pick", "pick", "wide"]
    assert [seg(n, records_dense=False) for n in (60, 61, 1999, 2000)] == ["flat", "pick", "pick", "wide"]
    # a padded pitch: only the row-tiled kernel
    assert {seg(n, out_dense=False) for n in (8, 61, 1024, 2000, 5000)} == {"rows"}
    # full lines: runs of lines (seven per run) below 1 000, the pick family to 1 399 and 4 096 (gathered), the stream kernel from 1 400
    assert [lin(n) for n in (7, 8, 538, 999, 1000, 1399, 1400, 5000)] == ["rows", "lineruns", "lineruns", "pick", "pick", "pick", "wide", "wide"]
    assert [lin(300, p) for p in (94, 95)] == ["lineruns", "pick"] and [lin(n, 0) for n in (547, 548)] == ["lineruns", "pick"]
    assert [lin(n, gathered=True) for n in (60, 61, 1399, 1400)] == ["rows", "pick", "pick", "wide"]
    # the second pass of the two passes: compact records of K kept samples, dense, all of them kept
    assert seg(4940) == "wide" and lin(4940, 166) == "wide" and seg(1999) == "pick"
