"""CPU tests of the kept-subset dispatch and launch plans (plan::emit of csrc/launch_plan.h, run through tests/subset_plan.py): the
values on both sides of every condition AUTO, the forced kernel ids, the two-pass chunks and the launch plans contain, the
constants, the shape of capi.hip's emit path, and that the GPU cell table of test_subset_plan_gpu.py reaches every arm and both
sides of every edge.  A changed threshold fails here instead of silently moving an edge away from the cells that test it."""
import re
from pathlib import Path

import subset_plan as SP

CSRC = Path(__file__).resolve().parent.parent / "pgen_rs_amd" / "csrc"
T = SP.Tune


def _src(file):
    return (CSRC / file).read_text()


def _body(file, signature):
    s = _src(file)
    b = s[s.index(signature):]
    return b[: b.index("\n}\n")]


def test_constants_are_pinned():
    assert (SP.SEG_SAMPLES, SP.COMPACT_MAX_SEG_CODES, SP.ROWPICK_MAX_KEPT, SP.COMPACT_SLICE_BYTES) == (16384, 4096, 16384, 32 << 20)
    assert (SP.WAVES, SP.ROWPICK_MAX_SEGS, SP.ROWPICK_ROWS_PER_WAVE) == (4, 4096, 8)
    assert SP.CHOICES == ("rows", "flat", "wide", "runs", "lineruns", "pick", "scan", "rowpick", "two_pass")
    # the static LDS the unmeasured occupancy constants are derived from
    scan = _src("gt_scan.hip")
    assert "__shared__ __attribute__((aligned(16))) uint16_t s_idx[kPickMaxSegCodes + 16];" in scan
    assert "constexpr uint32_t kPickMaxSegCodes = kSegSamples;" in scan
    assert "__shared__ uint16_t s_idx[kCompactMaxSegCodes + 8];" in scan
    assert scan.count("__shared__ __attribute__((aligned(16))) uint8_t s_stage[kWaves][kStageBytes];") == 2
    assert "__shared__ uint8_t s_out[kWaves][kCompactMaxSegCodes / 4u + 64u];" in scan
    assert (SP.SCAN_OCCUPANCY, SP.COMPACT_OCCUPANCY) == (3, 5)


def _around(f, edge):
    return [bool(f(edge + d)) for d in (-1, 0, 1)]


def test_auto_predicates_on_both_sides_of_every_condition():
    """two_pass_shape, very_sparse, rowpick_shape and two_pass at -1, 0, +1 of each of their conditions."""
    # two_pass_shape: N > 4 096, K * 170 >= N, K * 22 <= N (K >= 8 cannot be reached: K * 170 >= N > 4 096 means K >= 25)
    assert _around(lambda n: SP.two_pass_shape(n, 100), 4096) == [False, False, True]
    assert _around(lambda k: SP.two_pass_shape(170_000, k), 1000) == [False, True, True]
    assert _around(lambda k: SP.two_pass_shape(44_000, k), 2000) == [True, True, False]
    assert not any(SP.two_pass_shape(n, 7) for n in (1, 1190, 4097, 100_000))
    # very_sparse: N >= 65 536, K * 280 <= N
    assert _around(lambda n: SP.very_sparse(n, 234), 65536) == [False, True, True]
    assert _around(lambda k: SP.very_sparse(280_000, k), 1000) == [True, True, False]
    # rowpick_shape: the knob, N > 16 384, N < 24 576, else K * 50 >= N and K * 5 <= N; applicability: K in 1 .. 16 384, rows for every wave
    rs = lambda n, k, v=8192, tune=T(), cus=256: SP.rowpick_shape(n, k, v, tune, cus)   # noqa: E731
    assert rs(20_000, 2_000) and not rs(20_000, 2_000, tune=T(scan_rowpick=-1))
    assert _around(lambda n: rs(n, 1_638), 16384) == [False, False, True]
    assert _around(lambda n: rs(n, 10_000), 24576) == [True, False, False]
    assert _around(lambda k: rs(100_000, k), 2000) == [False, True, True]
    assert _around(lambda k: rs(50_000, k), 10_000) == [True, True, False]
    assert _around(lambda k: rs(20_000, k), 16384) == [True, True, False] and _around(lambda k: SP.rowpick_applicable(20_000, k, 8192), 1) == [False, True, True]
    for cus in (80, 256, 304):
        assert _around(lambda v: rs(20_000, 2_000, v, cus=cus), 32 * cus) == [False, True, True]
    assert _around(lambda n: SP.rowpick_applicable(n, 1_000, 8192), 4096 * 16384 + 1) == [True, False, False]   # 4 096 segments
    assert _around(lambda n: SP.rowpick_applicable(n, 5, 8192), 61) == [False, True, True]                        # records of 16 bytes
    # two_pass: the knob, the shape, max_seg_count <= 4 096, full lines from K = 1 024
    assert SP.two_pass(100_000, 1_999, 1_999, False, T()) and not SP.two_pass(100_000, 1_999, 1_999, False, T(scan_two_pass=-1))
    assert not SP.two_pass(100_000, 20_000, 4_000, False, T())
    assert _around(lambda m: SP.two_pass(100_000, 4_500, m, False, T()), 4096) == [True, True, False]
    assert _around(lambda k: SP.two_pass(100_000, k, k, True, T()), 1024) == [False, True, True]
    s = SP.shape(100_000, 1_999, kept_list=True)
    assert SP._call("emit_two_pass", 1, *s, 1, 1_999)[0] == 1
    assert SP._call("emit_two_pass", 1, *SP.shape(100_000, 1_999, kept_list=True, out_dense=False), 1, 1_999)[0] == 0   # padded output
    assert SP._call("emit_two_pass", 1, *SP.shape(100_000, 1_999, kept_list=False), 1, 1_999)[0] == 0                  # no kept list


def test_choose_subset_takes_its_arms_in_order():
    """One chain for GT segments and full lines: row owner, two passes, line runs (full lines, N < 300), pick, rows, segment kernel."""
    cs = SP.choose_subset
    # both the row owner's and the two passes' shape: the row owner first; one row fewer than every wave needs: the two passes
    assert SP.two_pass(100_000, 3_000, 3_000, False, T()) and cs(100_000, 3_000, 8192) == "rowpick" and cs(100_000, 3_000, 8191) == "two_pass"
    assert cs(100_000, 3_000, 8192, tune=T(scan_rowpick=-1)) == "two_pass" and cs(100_000, 3_000, 8191, tune=T(scan_two_pass=-1)) == "scan"
    assert cs(100_000, 4_500, 33, msc=4096) == "two_pass" and cs(100_000, 4_500, 33, msc=4097) == "scan"
    for mode in (False, True):
        assert [cs(n, 409, 33, lines=mode) for n in (4095, 4096, 4097)] == ["pick", "pick", "scan"]
        assert [cs(280_000, k, 33, lines=mode) for k in (999, 1000, 1001)] == ["rows", "rows", "scan"]
        assert [cs(65_536 + d, 234, 33, lines=mode) for d in (-1, 0, 1)] == ["scan", "rows", "rows"]
    assert [cs(n, 5, 33) for n in (59, 60, 61, 62)] == ["rows", "rows", "pick", "pick"]
    # full lines: runs of lines below N = 300 while a run holds seven (30-byte prefixes); the pick family from there, and for GT segments
    assert [cs(n, 50, 33, lines=True, bound=30) for n in (100, 298, 299, 300, 301)] == ["lineruns", "lineruns", "lineruns", "pick", "pick"]
    assert [cs(100, 50, 33, lines=True, bound=p) for p in (93, 94, 95)] == ["lineruns", "lineruns", "pick"]
    assert cs(100, 50, 33, bound=30) == "pick" and cs(100, 50, 33, lines=True, bound=30, gathered=True) == "pick"
    assert cs(100, 50, 33, lines=True, bound=30, records_dense=False) == "pick" and [cs(100, k, 33, lines=True, bound=30) for k in (7, 8, 9)] == ["pick", "lineruns", "lineruns"]
    # full lines through the two passes from K = 1 024
    assert [cs(100_000, k, 33, lines=True) for k in (1023, 1024, 1025)] == ["scan", "two_pass", "two_pass"]


def test_two_pass_chunks_on_both_sides_of_every_condition():
    rc = (1_999 + 3) // 4
    full = (32 << 20) // rc                                    # 67 108 rows of 500 bytes
    chunks = lambda v, tune=T(), cus=256, n=100_000, k=1_999: SP.two_pass_chunks(n, k, v, tune, cus)   # noqa: E731
    # the rows a slice holds, rounded down to whole row-owner rounds (2 blocks per CU x 4 waves) where the row owner takes the chunk
    assert chunks(200_000)[0] == full - full % 2048 == 65_536 and chunks(200_000, cus=304)[0] == full - full % 2432
    assert chunks(200_000, T(scan_rowpick=-1))[0] == full and chunks(200_000, T(scan_rowpick=-1))[1][0][1] == "scan"
    assert chunks(8191)[0] == full and chunks(8191)[1] == ((8191, "scan", SP.scan_plan(100_000, 1_999, 8191, compact=True)),)   # too few rows for the row owner
    assert chunks(8192)[0] == 65_536 and chunks(8192)[1][0][:2] == (8192, "scan")                              # (a short only chunk)
    # the knob caps the chunk and is not rounded
    assert chunks(200_000, T(scan_chunk_rows=10_000))[0] == 10_000 and chunks(200_000, T(scan_chunk_rows=100_000))[0] == full
    assert chunks(200_000, T(rowpick_blocks_per_cu=1))[0] == full - full % 1024
    # at least one row however long the compact record
    assert SP._call("emit_chunks", 2, *SP.shape(4096 * 16384, 3_000_000, 10, kept_list=True), 1000, 0, 1, 0, 256) == (1, 0)
    # the short last chunk: the row owner while it has at least half a chunk of rows
    assert [SP._call("emit_chunk_by_row_owner", 1, 100, 1, n)[0] for n in (49, 50, 51)] == [0, 1, 1]
    assert SP._call("emit_chunk_by_row_owner", 1, 100, 0, 100)[0] == 0
    assert [k for _, k, _ in chunks(65_536 + 32_767)[1]] == ["rowpick", "scan"] and [k for _, k, _ in chunks(65_536 + 32_768)[1]] == ["rowpick", "rowpick"]


def test_segment_plan_on_both_sides_of_every_condition():
    sp = SP.scan_plan
    # blocks per CU: the occupancy figure, two from K * 170 >= N and in the compact pass, the knob over both
    assert [sp(170_000, k, 1000).per_cu for k in (999, 1000, 1001)] == [3, 2, 2]
    assert [sp(170_000, 1000, 1000, occupancy=o).per_cu for o in (0, 1, 2, 3)] == [1, 1, 2, 2] and sp(170_000, 999, 1000, occupancy=5).per_cu == 5
    assert sp(170_000, 999, 1000, compact=True).per_cu == 2 and sp(170_000, 999, 1000, compact=True, occupancy=1).per_cu == 1
    assert sp(170_000, 1000, 1000, T(scan_blocks_per_cu=4)).per_cu == 4 and sp(170_000, 999, 1000, T(scan_blocks_per_cu=1), compact=True).per_cu == 1
    # row groups: resident blocks / segments, floored; at least one; no more than the rows need
    p = sp(147_456, 20_000, 14_336)
    assert (p.n_seg, p.groups, p.grid) == (9, 56, 504) and sp(147_457, 20_000, 14_336).groups == 51
    assert [sp(n, n // 20, 16).groups for n in (2 * 256 * 16384, 2 * 256 * 16384 + 1)] == [1, 1]
    assert [sp(10_000, 1_000, v).groups for v in (4, 5, 2044, 2045, 2048, 2049)] == [1, 2, 511, 512, 512, 512]
    assert sp(1, 1, 1).n_seg == 1
    # the XCD-aware map takes whole eights of row groups; the plain map none
    assert [sp(10_000, 1_000, v).xcd_groups for v in (28, 29, 32, 33, 60, 61)] == [0, 8, 8, 8, 8, 16]
    assert sp(10_000, 1_000, 131_072, T(scan_xcd_map=-1)).xcd_groups == 0
    # eight bands: K * 10 >= N, a multiple of eight groups, 64 steps of every group; never in the compact pass
    assert [sp(10_000, k, 131_072).bands for k in (999, 1000, 1001)] == [1, 8, 8]
    assert [sp(10_000, 1_000, v).bands for v in (131_068, 131_069, 131_072)] == [1, 8, 8]
    assert [sp(n, 20_000, 14_336).bands for n in (147_456, 147_457)] == [8, 1] and sp(10_000, 1_000, 131_072, compact=True).bands == 1


def test_row_owner_plan_on_both_sides_of_every_condition():
    rp = SP.rowpick_plan
    # what the launcher refuses: more than 16 384 kept samples, more than 4 096 segments, records below 16 bytes
    assert [rp(20_000, k, 100) is None for k in (16_383, 16_384, 16_385)] == [False, False, True]
    assert [rp(n, 1_000, 100) is None for n in (4096 * 16384 - 1, 4096 * 16384, 4096 * 16384 + 1)] == [False, False, True]
    assert [rp(n, 5, 100) is None for n in (60, 61, 62)] == [True, False, False]
    # the LDS of a block
    # (table of K + 8 u16 | ranks of 3 u32 | four waves x (4 096 + ceil(K / 4) + 16), each part rounded up to 16)
    assert [SP.rowpick_lds_bytes(20_000, k) for k in (1, 8, 9, 16_336, 16_337)] == [32 + 16 + 4 * (4096 + 32)] * 2 + [48 + 16 + 4 * (4096 + 32), 65_536, 65_552]
    assert SP.rowpick_lds_bytes(16_384 * 3, 1) - SP.rowpick_lds_bytes(16_384 * 3 + 1, 1) == -16   # the rank table grows every four segments
    # blocks per CU: four (text, N < 24 576) or two, never more than fit; the knob caps
    assert [rp(n, 2_000, 8192).per_cu for n in (24_575, 24_576, 24_577)] == [4, 2, 2]
    assert rp(24_575, 2_000, 8192, compact=True).per_cu == 2
    assert [rp(20_000, 2_000, 8192, occupancy=o).per_cu for o in (0, 1, 3, 4, 5)] == [1, 1, 3, 4, 4]
    assert rp(20_000, 16_384, 8192).per_cu == 2 == SP.rowpick_occupancy(20_000, 16_384)
    assert [rp(20_000, 2_000, 8192, T(rowpick_blocks_per_cu=b)).per_cu for b in (1, 3, 6)] == [1, 3, 6] and rp(20_000, 2_000, 8192, T(rowpick_blocks_per_cu=8), occupancy=5).per_cu == 5
    # one resident round; a block per four rows up to it
    for cus in (80, 256, 304):
        p = rp(100_000, 2_000, 10 ** 6, num_cus=cus)
        assert (p.max_blocks, p.grid) == (2 * cus, 2 * cus)
        assert [rp(100_000, 2_000, v, num_cus=cus).grid for v in (1, 4, 5, 8 * cus - 4, 8 * cus - 3, 8 * cus, 8 * cus + 1)] == [1, 1, 2, 2 * cus - 1, 2 * cus, 2 * cus, 2 * cus]


def test_emit_path_of_capi_has_one_choice_and_one_switch():
    """capi.hip: three entry points -> one emit_core -> one choice (plan::emit) -> one `run` switch; no predicate of its own."""
    src = _src("capi.hip")
    for sig in ("int pgenhip_decode_emit(", "int pgenhip_decode_emit_at(", "int pgenhip_emit_lines("):
        b = _body("capi.hip", sig)
        assert b.count("return emit_core(ctx, ") == 1 and "launch_gt_" not in b and "choose" not in b and "PGENHIP_KERNEL_" not in b, sig
    core = _body("capi.hip", "static int emit_core(")
    steps = ["bind(ctx)", "fill_args(ctx, a, ", "claim_counters(ctx, a)", "choose(ctx, a, flags, choice)", "return run(ctx, a, sc, choice);"]
    assert [core.index(s) for s in steps] == sorted(core.index(s) for s in steps) and all(core.count(s) == 1 for s in steps)
    assert src.count("const ScanArgs sc{") == 1 and "launch_gt_" not in core
    # the one place a kernel id becomes what runs: AUTO by the header's chains (an identity list dropped first), a forced id by the header's table
    b = _body("capi.hip", "static int choose(const pgenhip_ctx *ctx, EmitArgs &a, uint32_t kernel, Emit &out)")
    assert b.count("a.kept_idx = nullptr") == 1 and b.index("if (ctx->identity) a.kept_idx = nullptr;") < b.index("emit_shape(a)")
    assert b.count("E::choose_all_samples(") == 1 and b.count("E::choose_subset(") == 1 and b.count("E::accepts(kernel, s)") == 1 and b.count("E::forced(kernel, s.lines)") == 1
    assert src.count("E::choose_subset(") == 1 and src.count("E::choose_all_samples(") == 2 and src.count("E::accepts(") == 1
    assert not re.search(r"gt_\w+_(applicable|preferred|rows)\b", src)
    run = _body("capi.hip", "static int run(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc, Emit choice)\n{")
    emit_launches = re.findall(r"LAUNCH_TRY\(launch_gt_(\w+)\(", src)
    assert sorted(re.findall(r"LAUNCH_TRY\(launch_gt_(\w+)\(", run)) == sorted(["rows", "flat", "wide", "runs", "lineruns", "pick", "scan", "rowpick"])
    assert len(emit_launches) == 10   # + the two compact passes of dispatch_two_pass
    two = _body("capi.hip", "static int dispatch_two_pass(")
    assert "const int rc = run(ctx, d, sc, E::choose_all_samples(emit_shape(d)));" in two
    assert sorted(re.findall(r"LAUNCH_TRY\(launch_gt_(\w+)\(", two)) == ["rowpick", "scan"] and two.count("E::chunks(") == 1 and two.count("E::chunk_by_row_owner(") == 1


def test_forced_kernel_acceptance_table():
    """accepts(): the kernel ids as include/pgen_hip.h numbers them, and where each forced kernel is taken on the shapes of
    test_emit_kernel_ids_gpu.py (GT segments at the dense pitch; at pitch 4K + 4 only ROWS, SCAN and ROWPICK; no id that is not a kernel)."""
    header = (CSRC.parent.parent / "include" / "pgen_hip.h").read_text()
    ids = {m[0].lower(): int(m[1]) for m in re.findall(r"#define PGENHIP_KERNEL_([A-Z]+) (\d+)u", header)}
    assert ids == SP.KERNEL_IDS and "#define PGENHIP_KERNEL_MASK 0xFu" in header
    shapes = {"40": (40, 40, False), "40/5": (40, 5, True), "300": (300, 300, False), "300/30": (300, 30, True), "300/id": (300, 300, True),
              "1024": (1024, 1024, False), "5000/50": (5000, 50, True), "20000/16385": (20_000, 16_385, True)}
    lists = {"300/30", "300/id", "5000/50", "20000/16385"}
    table = {"rows": set(shapes), "flat": {"40", "300", "1024"}, "wide": {"1024"}, "runs": {"40", "300", "1024"},
             "pick": {"300", "300/30", "300/id", "1024"}, "scan": lists, "rowpick": lists - {"20000/16385"}}
    for name, taken in table.items():
        for tag, (n, k, subset) in shapes.items():
            seg = dict(mode="segments")
            assert SP.accepts(SP.KERNEL_IDS[name], n, k, subset, **seg) == (tag in taken), (name, tag)
            assert SP.accepts(SP.KERNEL_IDS[name], n, k, subset, dense_pitch=False, **seg) == (tag in taken and name in ("rows", "scan", "rowpick"))
            assert SP.accepts(SP.KERNEL_IDS[name], n, k, subset, gather=True, **seg) == (tag in taken and name != "runs")
            assert not SP.accepts(SP.KERNEL_IDS["flat"], n, k, subset, 10, False)   # full lines: never FLAT
    assert not any(SP.accepts(i, 300, 300, False, mode=m) for i in (5, 9, 10, 11, 12, 13, 14, 15, 0x10, 0x13) for m in ("segments", "lines"))
    assert (SP.runs_rows(3831), SP.runs_rows(3832)) == (1, 0) and SP.accepts(7, 3831, 3831, False, mode="segments") and not SP.accepts(7, 3832, 3832, False, mode="segments")


def test_forced_kernel_ids_on_both_sides_of_every_condition():
    ids = SP.KERNEL_IDS
    acc = lambda name, n, k=None, subset=False, **kw: SP.accepts(ids[name], n, n if k is None else k, subset, **kw)   # noqa: E731
    for mode in ("segments", "lines"):
        assert [acc("scan", n, 5, True, mode=mode) for n in (60, 61, 62)] == [False, True, True] and not acc("scan", 300, mode=mode)
        assert [acc("rowpick", n, 5, True, mode=mode) for n in (60, 61, 62)] == [False, True, True] and not acc("rowpick", 20_000, mode=mode)
        assert [acc("rowpick", 20_000, k, True, mode=mode) for k in (0, 1, 2, 16_383, 16_384, 16_385)] == [False, True, True, True, True, False]
        assert [acc("wide", n, mode=mode) for n in (1023, 1024, 1025)] == [False, True, True] and not acc("wide", 1024, 1024, True, mode=mode)
        assert [acc("pick", n, mode=mode) for n in (60, 61, 62, 4095, 4096, 4097)] == [False, True, True, True, True, False]
        assert [acc("pick", 300, k, True, mode=mode) for k in (0, 1, 2)] == [False, True, True]
    assert [acc("flat", n, mode="segments") for n in (7, 8, 9)] == [False, True, True] and not acc("flat", 300, 30, True, mode="segments")
    assert [acc("runs", n, mode="segments") for n in (7, 8, 9, 3830, 3831, 3832)] == [False, True, True, True, True, False]
    assert acc("wide", 1024, mode="lines", dense_pitch=False) and acc("pick", 300, mode="lines", dense_pitch=False)
    # RUNS for full lines: the line-run kernel (tests/test_line_plan.py has its prefix-driven limits)
    assert [acc("runs", n, mode="lines", bound=30) for n in (7, 8, 9)] == [False, True, True]
    assert [acc("runs", n, 50, True, mode="lines", bound=30) for n in (1384, 1385, 4096, 4097)] == [True, False, False, False]
    assert [acc("runs", 300, k, True, mode="lines", bound=30) for k in (7, 8, 9)] == [False, True, True]
    assert not acc("runs", 300, mode="lines", bound=30, gather=True)
    # what a forced id runs
    forced = lambda name, lines: SP.CHOICES[SP._call("emit_accepts", 3, *SP.shape(300, 300, kept_list=False, lines=lines), ids[name])[2]]   # noqa: E731
    assert [forced(k, False) for k in ("rows", "flat", "scan", "wide", "pick", "runs", "rowpick")] == ["rows", "flat", "scan", "wide", "pick", "runs", "rowpick"]
    assert forced("runs", True) == "lineruns" and forced("pick", True) == "pick"


def test_derived_edges():
    """The edges the GPU cells sit on at 256 CUs, as derived today (a change here means re-reading the planning code)."""
    assert SP.rowpick_lds_bytes(20_000, 16_384) == 65_632 and SP.rowpick_lds_bytes(65_536, 16_384) == 65_648
    assert (SP.rowpick_lds_edge(20_000), SP.rowpick_lds_edge(65_536), SP.rowpick_lds_edge(4096 * 16384)) == (16_337, 16_329, 10_881)
    assert SP.rowpick_lds_bytes(20_000, 16_336) == 65_536 and SP.rowpick_lds_bytes(4096 * 16384, 16384) == 82_016
    assert SP.scan_plan(10_000, 1_000, 131_069).bands == 8 and SP.scan_plan(10_000, 1_000, 131_068).bands == 1
    assert SP.scan_plan(147_456, 20_000, 14_336).groups == 56 and SP.scan_plan(147_457, 20_000, 14_336).groups == 51
    assert SP.scan_plan(2 * 256 * 16384 + 1, 419_430, 16).rounds and not SP.scan_plan(2 * 256 * 16384, 419_430, 16).rounds
    chunk, chunks = SP.two_pass_chunks(100_000, 1_999, 65_536 + 4_096, SP.Tune(), 256)
    assert chunk == 65_536 and [(r, k) for r, k, _ in chunks] == [(65_536, "rowpick"), (4_096, "scan")]
    chunk, chunks = SP.two_pass_chunks(100_000, 1_999, 3 * 8192 + 1000, SP.Tune(scan_chunk_rows=8192), 256)
    assert [(r, k) for r, k, _ in chunks] == [(8192, "rowpick")] * 3 + [(1000, "scan")]
    # unreachable: two_pass_shape's K >= 8
    assert all(k >= 25 for n in range(4097, 200_000, 997) for k in range(1, 2000) if k * 170 >= n)


def test_cells_reach_every_arm_and_both_sides_of_every_edge():
    for cus in (256, 304, 80):
        table = SP.cells(cus)
        reached = set()
        for c in table:
            reached |= SP.arm_tags(c, cus)
        missing = SP.REACHABLE_ARMS - reached
        assert not missing, f"{cus} CUs: no cell reaches {sorted(missing)}"
        pairs = SP.edge_pairs(table, cus)
        assert [e[0] for e in SP.EDGES] == list(pairs)
        uncovered = [name for name, p in pairs.items() if not p]
        assert not uncovered, f"{cus} CUs: no cell pair across {uncovered}"
