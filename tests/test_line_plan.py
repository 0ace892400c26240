"""CPU tests of the full-line kernels' planning arithmetic (plan::emit of csrc/launch_plan.h, run through tests/line_plan.py): the
constants, the values on both sides of every limit, and the edges that test_emit_lines_prefixes_gpu.py places its cells around.  A
changed constant fails here and points at that edge table, instead of silently moving an edge away from the cells that test it."""
import line_plan as LP
import subset_plan as SP


def test_constants_are_pinned():
    assert (LP.LR_PFX_BYTES, LP.LR_MAX_ROWS, LP.LR_LOAD_BYTES, LP.SPAN_BYTES, SP.LR_TAB_MAX_SAMPLES) == (768, 30, 1040, 15328, 4096)
    assert (LP.PICK_PFX_BYTES, LP.PICK_STAGE_BYTES, LP.PICK_MAX_PACKED_ROWS, LP.PICK_MAX_SAMPLES, SP.PICK_MAX_BATCH_ROWS) == (2048, 8192, 64, 4096, 12)
    assert (SP.PICK_MAX_LINES_ROWS, SP.PICK_MAX_LINES_PREFIX) == (62, 993)
    assert LP.ROWPICK_MAX_KEPT == 16384


def test_line_run_plan_on_both_sides_of_every_limit():
    rows = LP.lineruns_rows
    # a line longer than a span: none (N = 3 831: 15 325 bytes of GT text)
    assert [rows(3831, 3831, False, p) for p in (2, 3, 4)] == [1, 1, 0]
    # the records of one wide load: 1 040 // R, one fewer with a kept list (the record behind the run comes along)
    assert [rows(n, 8, True, 0) for n in (1384, 1385, 1388)] == [2, 1, 1] and SP.record_size(1384) == 346 and 3 * 346 <= 1040 < 3 * 347
    assert [rows(n, 8, True, 0) for n in (4160, 4161)] == [0, 0] and rows(2080, 8, True, 0) == 1
    # whole lines of a span
    assert [rows(1900, 1900, False, p) for p in (62, 63, 64)] == [2, 2, 1] and [rows(n, n, False, 0) for n in (1915, 1916)] == [2, 1]
    # at most 30 lines; prefixes of B + 1 lines in 768 - 16 bytes
    assert [rows(8, 8, False, p) for p in (0, 1, 23, 24, 25)] == [30, 30, 30, 30, 29]
    assert [rows(8, 8, False, p) for p in (94, 95, 250, 251, 376, 377, 752, 753)] == [7, 6, 2, 1, 1, 0, 0, 0]
    # what the kernel takes: two lines per item, N >= 8 (all samples) or K >= 8 of N <= 4 096 (kept list)
    acc = LP.lineruns_accepts
    assert [acc(8, 8, False, p) for p in (250, 251)] == [True, False]
    assert [acc(n, n, False, 30) for n in (7, 8, 9)] == [False, True, True]
    # (a kept list's N <= 4 096 cannot be reached: two lines and the record behind them already need R <= 346)
    assert [acc(300, k, True, 30) for k in (7, 8, 9)] == [False, True, True] and [acc(n, 50, True, 30) for n in (1384, 1385, 4096, 4097)] == [True, False, False, False]
    # lanes per seam by P + 1 bytes
    assert [LP.lineruns_seam_shift(p) for p in (0, 15, 16, 31, 32, 63, 64, 127, 128, 3000)] == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6]


def test_pick_lines_plan_on_both_sides_of_every_limit():
    # rows per batch: 32 KiB of text, at most 64 rows, what the 8 192-byte stage holds beside 16 bytes of misalignment
    assert [LP.pick_batch_rows(n, n) for n in (61, 129, 130, 510, 4096)] == [64, 64, 63, 17, 2]
    assert [LP.pick_batch_rows(n, 1) for n in (61, 2044, 2045, 4096)] == [64, 16, 15, 7] and LP.pick_batch_rows(4096, 409) == 7
    # full lines: at most 62 rows, the row behind the batch and its prefix come along
    plr = LP.pick_lines_rows
    assert [plr(n, n, 0) for n in (61, 510, 4096)] == [62, 17, 2] and [plr(4096, 409, p) for p in (0, 290, 291)] == [6, 6, 5]
    assert [plr(61, 61, p) for p in (32, 33, 677, 678, 1016, 1017, 2032, 2033)] == [62, 60, 2, 1, 1, 0, 0, -1]
    # gt_pick_lines_kernel runs from two rows per batch (prefixes longer than 993 bytes never get there: two of them overflow the stage),
    # K >= 4, dense records, prefix bytes present
    def taken(n, k, p, **kw):
        return bool(SP._call("emit_pick_plan", 6, *SP.shape(n, k, kept_list=k != n, lines=True, bound=p, **kw), 0)[3])
    assert [taken(61, 61, p) for p in (677, 678, 993, 994)] == [True, False, False, False]
    assert [taken(300, k, 30) for k in (3, 4, 5)] == [False, True, True]
    assert not taken(300, 300, 30, gathered=True) and not taken(300, 300, 30, records_dense=False) and not taken(300, 300, 30, prefix_blob=False)
    assert not SP._call("emit_pick_plan", 6, *SP.shape(300, 300, kept_list=False), 0)[3]   # GT segments
    # batches of gathered / padded records: rows at a power-of-two pitch, 12 loads of 64 / lanes-per-row rows
    assert SP._call("emit_pick_plan", 6, *SP.shape(300, 300, kept_list=False, gathered=True), 0)[:3] == (0, 128, 28)
    assert SP._call("emit_pick_plan", 6, *SP.shape(4096, 4096, kept_list=False, records_dense=False), 0)[:3] == (0, 1024, 2)
    assert SP._call("emit_pick_plan", 6, *SP.shape(4096, 409, kept_list=True, gathered=True), 0)[:3] == (0, 1024, 8)
    assert SP._call("emit_pick_plan", 6, *SP.shape(300, 30, kept_list=True), 1000)[2] == 9 and SP._call("emit_pick_plan", 6, *SP.shape(300, 30, kept_list=True), 1)[2] == 1
    # lanes per seam by ceil-ish (P + 31) / 16 chunks; lanes per line of the prefix copy
    assert [LP.pick_cps_shift(p) for p in (0, 48, 49, 112, 113, 240, 241, 496, 497, 3000)] == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert [LP.prefix_copy_shift(p) for p in (0, 47, 48, 49, 3000)] == [3, 3, 3, 4, 4]


def test_derived_edges():
    """The edges the GPU matrix places its cells around, as derived today (a change here means re-reading the planning code)."""
    assert LP.LR_SEAM_EDGES == [15, 31, 63, 127]
    assert (LP.LR_ROWS_7_6, LP.LR_ROWS_2_1, LP.LR_LINE_LIMIT) == (94, 250, 7664)
    assert LP.PICK_SEAM_EDGES == [48, 112, 240, 496]
    assert LP.PICK_ROWS_FALLBACK == 677 and LP.COPY_SHIFT_EDGE == 48
    assert LP.pick_lines_rows(4096, 409, 0) == 6 and LP.pick_cross_edge(4096, 409) == 290
    assert LP.rowpick_lds_bytes(20_000, 16_384) == 65_632 and LP.rowpick_lds_bytes(65_536, 16_384) == 65_648
    assert [LP.lineruns_rows(1900, 1900, False, p) for p in (63, 64)] == [2, 1]
