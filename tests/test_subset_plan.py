"""CPU guard of tests/subset_plan.py: what it restates must still read the same in csrc/, and its GPU cell table must reach every
arm and both sides of every edge of the kept-subset dispatch and launch plans.  A changed constant, literal or condition fails here
instead of silently moving an edge away from the cells of test_subset_plan_gpu.py that test it."""
import re
from pathlib import Path

import subset_plan as SP

CSRC = Path(__file__).resolve().parent.parent / "pgen_rs_amd" / "csrc"


def _src(file):
    return (CSRC / file).read_text()


def _const(file, name):
    m = re.findall(rf"constexpr\s+(?:uint32_t|int|size_t)\s+{name}\s*=\s*([^;]+);", _src(file))
    assert len(m) == 1, f"{name} in {file}: {m}"
    return m[0].strip()


def _body(file, signature):
    s = _src(file)
    b = s[s.index(signature):]
    return b[: b.index("\n}\n")]


def _conditions(body):
    """The branch points of a body: `if`s, `&&`, `||` and `?`."""
    return len(re.findall(r"\bif \(|&&|\|\||\?", body))


def test_mirrored_constants_match_the_sources():
    assert _const("kernels.h", "kScanSegmentSamples") == f"{SP.SEG_SAMPLES}u"
    assert _const("kernels.h", "kCompactMaxSegCodes") == f"{SP.COMPACT_MAX_SEG_CODES}u"
    assert _const("kernels.h", "kRowPickMaxKept") == f"{SP.ROWPICK_MAX_KEPT}u"
    assert _const("capi.hip", "kCompactSliceBytes") == "32u << 20" and SP.COMPACT_SLICE_BYTES == 32 << 20
    for f in ("gt_scan.hip", "gt_rowpick.hip"):
        assert _const(f, "kThreads") == "256" and _const(f, "kWaves") == "kThreads / 64" and SP.WAVES == 4
    # the static LDS the unmeasured occupancy constants are derived from
    scan = _src("gt_scan.hip")
    assert "__shared__ __attribute__((aligned(16))) uint16_t s_idx[kPickMaxSegCodes + 16];" in scan
    assert "constexpr uint32_t kPickMaxSegCodes = kSegSamples;" in scan
    assert "__shared__ uint16_t s_idx[kCompactMaxSegCodes + 8];" in scan
    assert scan.count("__shared__ __attribute__((aligned(16))) uint8_t s_stage[kWaves][kStageBytes];") == 2
    assert "__shared__ uint8_t s_out[kWaves][kCompactMaxSegCodes / 4u + 64u];" in scan
    assert (SP.SCAN_OCCUPANCY, SP.COMPACT_OCCUPANCY) == (3, 5)


def test_mirrored_dispatch_matches_capi():
    """capi.hip: the literals of two_pass_shape, very_sparse, rowpick_shape and two_pass, the chunk rounding of dispatch_two_pass,
    the AUTO arms (choose_subset: one chain for GT segments and full lines; choose_all_samples: one per mode) and the one place
    that maps a kernel id (choose) for the three entry points; a new condition in any of them changes its branch count and fails
    here until subset_plan.py, line_plan.py and the cells follow."""
    b = _body("capi.hip", "bool two_pass_shape(uint32_t sample_count, uint32_t kept_count)")
    assert ("sample_count > 4096u && kept_count >= 8u && (uint64_t)kept_count * 170ull >= (uint64_t)sample_count &&\n"
            "           (uint64_t)kept_count * 22ull <= (uint64_t)sample_count;") in b
    assert _conditions(b) == 3
    b = _body("capi.hip", "static bool very_sparse(const pgenhip_ctx *ctx)")
    assert "ctx->sample_count >= 65536u && (uint64_t)ctx->kept_count * 280ull <= ctx->sample_count;" in b and _conditions(b) == 1
    b = _body("capi.hip", "static bool rowpick_shape(const pgenhip_ctx *ctx, const EmitArgs &a)")
    assert ("if (ctx->tune.scan_rowpick == 0 || ctx->sample_count <= kScanSegmentSamples || very_sparse(ctx) || "
            "!gt_rowpick_applicable(a, ctx->num_cus)) return false;") in b
    assert "if (N < 24576ull) return true;" in b and "return K * 50ull >= N && K * 5ull <= N;" in b
    assert _conditions(b) == 6
    b = _body("capi.hip", "static bool two_pass(const pgenhip_ctx *ctx, const EmitArgs &a)")
    assert ("ctx->tune.scan_two_pass != 0 && ctx->d_compact != nullptr && a.kept_idx != nullptr && a.record_size >= 16u &&\n"
            "           ctx->max_seg_count <= kCompactMaxSegCodes &&\n"
            "           (a.line_off != nullptr ? a.kept_count >= 1024u : (a.n_variants <= 1u || a.out_stride == 4ull * a.kept_count + 1ull));") in b
    assert _conditions(b) == 7
    assert "if (two_pass_shape(sample_count, kept_count)) {\n                ctx->compact_bytes = kCompactSliceBytes;" in _src("capi.hip")
    b = _body("capi.hip", "static int dispatch_two_pass(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc)")
    assert "const uint32_t rc_bytes = (a.kept_count + 3u) / 4u;" in b
    assert "uint64_t chunk_rows = std::max<uint64_t>(1ull, ctx->compact_bytes / rc_bytes);" in b
    assert "if (ctx->tune.scan_chunk_rows > 0) chunk_rows = std::min<uint64_t>(chunk_rows, (uint64_t)ctx->tune.scan_chunk_rows);" in b
    assert "probe.n_variants = (uint32_t)std::min<uint64_t>(chunk_rows, a.n_variants);" in b
    assert "const uint64_t round = gt_rowpick_resident_waves(probe, ctx->tune, ctx->num_cus, true);" in b
    assert "if (row_owner && round && chunk_rows > round && ctx->tune.scan_chunk_rows <= 0) chunk_rows -= chunk_rows % round;" in b
    assert "if (row_owner && (uint64_t)n * 2ull >= chunk_rows)" in b
    assert "if (a.record_off) c.record_off = a.record_off + row0;" in b and "else if (a.variant_idx) c.variant_idx = a.variant_idx + row0;" in b
    assert _conditions(b) == 12
    # the AUTO arms for kept subsets: one chain for GT segments and full lines, in this order
    b = _body("capi.hip", "static Emit choose_subset(const pgenhip_ctx *ctx, const EmitArgs &a)")
    order = ["if (rowpick_shape(ctx, a)) return Emit::RowPick;", "if (two_pass(ctx, a) && !very_sparse(ctx)) return Emit::TwoPass;",
             "if (gt_lineruns_applicable(a) && gt_lineruns_rows(a) >= 7u && a.sample_count < 300u) return Emit::LineRuns;",
             "if (gt_pick_applicable(a)) return Emit::Pick;", "if (very_sparse(ctx) || ctx->record_size < 16u) return Emit::Rows;",
             "return Emit::Scan;"]
    assert [b.index(s) for s in order] == sorted(b.index(s) for s in order) and _conditions(b) == 9
    # the AUTO arms for all samples kept (tests/line_plan.py): the full-line chain, then the GT-segment chain
    b = _body("capi.hip", "static Emit choose_all_samples(const EmitArgs &a)")
    order = ["if (a.line_off != nullptr) {", "if (gt_wide_lines_applicable(a) && a.sample_count >= 1400u) return Emit::Wide;",
             "if (gt_lineruns_applicable(a) && gt_lineruns_rows(a) >= 7u && a.sample_count < 1000u) return Emit::LineRuns;",
             "if (gt_pick_applicable(a)) return Emit::Pick;", "return Emit::Rows;\n    }", "if (gt_runs_preferred(a)) return Emit::Runs;",
             "if (gt_pick_applicable(a) && a.sample_count < 2000u) return Emit::Pick;", "if (gt_wide_applicable(a)) return Emit::Wide;",
             "if (gt_flat_applicable(a)) return Emit::Flat;", "return Emit::Rows;"]
    at = []
    for s in order:
        at.append(b.index(s, at[-1] + 1 if at else 0))   # each behind the one before it
    assert _conditions(b) == 12
    # AUTO: an identity list goes with all samples, a kept list through the chain above; forced kernels see the list
    b = _body("capi.hip", "static int choose(const pgenhip_ctx *ctx, EmitArgs &a, uint32_t kernel, Emit &out)")
    auto = b[b.index("case PGENHIP_KERNEL_AUTO:"): b.index("case PGENHIP_KERNEL_ROWS:")]
    assert "if (ctx->identity) a.kept_idx = nullptr;\n            out = a.kept_idx == nullptr ? choose_all_samples(a) : choose_subset(ctx, a);" in auto
    assert b.count("a.kept_idx = nullptr") == 1 and _conditions(b) == 17
    # forced ROWPICK: capi.hip's own checks (the launcher refuses more than 4 096 segments: PGENHIP_ERR_HIP), once for every entry point
    src = _src("capi.hip")
    assert src.count("if (!ctx->subset || ctx->record_size < 16u || ctx->kept_count < 1u || ctx->kept_count > kRowPickMaxKept)") == 1
    assert all(src.count(f"case PGENHIP_KERNEL_{k.upper()}:") == 1 for k in SP.KERNEL_IDS)
    # the three entry points reach the one core, which chooses once and launches through the one switch
    for sig in ("int pgenhip_decode_emit(", "int pgenhip_decode_emit_at(", "int pgenhip_emit_lines("):
        b = _body("capi.hip", sig)
        assert b.count("return emit_core(ctx, ") == 1 and "launch_gt_" not in b and "choose" not in b and "PGENHIP_KERNEL_" not in b, sig
    core = _body("capi.hip", "static int emit_core(")
    steps = ["bind(ctx)", "fill_args(ctx, a, ", "claim_counters(ctx, a)", "choose(ctx, a, flags, choice)", "return run(ctx, a, sc, choice);"]
    assert [core.index(s) for s in steps] == sorted(core.index(s) for s in steps) and all(core.count(s) == 1 for s in steps)
    assert src.count("const ScanArgs sc{") == 1 and "launch_gt_" not in core
    run = _body("capi.hip", "static int run(pgenhip_ctx *ctx, const EmitArgs &a, const ScanArgs &sc, Emit choice)\n{")
    emit_launches = re.findall(r"LAUNCH_TRY\(launch_gt_(\w+)\(", src)
    assert sorted(re.findall(r"LAUNCH_TRY\(launch_gt_(\w+)\(", run)) == sorted(["rows", "flat", "wide", "runs", "lineruns", "pick", "scan", "rowpick"])
    assert len(emit_launches) == 10   # + the two compact passes of dispatch_two_pass
    assert "const int rc = run(ctx, d, sc, choose_all_samples(d));" in _body("capi.hip", "static int dispatch_two_pass(")


def test_mirrored_segment_plan_and_knobs_match_the_source():
    b = _body("gt_scan.hip", "hipError_t launch_gt_scan(")
    assert "const uint32_t n_seg = (a.sample_count + kSegSamples - 1u) / kSegSamples;" in b
    assert "const uint64_t groups_needed = ((uint64_t)a.n_variants + kWaves - 1ull) / kWaves;" in b
    assert "uint64_t groups = (uint64_t)resident_blocks(ckern, kThreads, num_cus, t, 2) / n_seg_eff;" in b
    assert "const int preferred = (uint64_t)a.kept_count * 170ull >= (uint64_t)a.sample_count ? 2 : 0;" in b
    assert "uint64_t groups = (uint64_t)resident_blocks(kern, kThreads, num_cus, t, preferred) / n_seg_eff;" in b
    assert b.count("if (groups < 1ull) groups = 1ull;") == 2 and b.count("if (groups > groups_needed) groups = groups_needed;") == 2
    assert b.count("const uint32_t xcd_groups = t.scan_xcd_map != 0 ? (uint32_t)(groups & ~7ull) : 0u;") == 2
    assert ("const bool banded = (uint64_t)a.kept_count * 10ull >= (uint64_t)a.sample_count && groups % 8ull == 0ull && "
            "groups_needed >= 64ull * groups;") in b
    assert "const uint32_t bands = banded ? 8u : 1u;" in b and "const uint32_t grid = (uint32_t)(groups * n_seg_eff);" in b
    r = _body("gt_scan.hip", "static uint32_t resident_blocks(")
    assert "if (preferred > 0 && preferred < per_cu) per_cu = preferred;" in r and "if (t.scan_blocks_per_cu > 0) per_cu = t.scan_blocks_per_cu;" in r
    k = _src("gt_scan.hip")
    assert "const uint32_t band = row_group % bands, group_in_band = row_group / bands;" in k
    assert "const uint64_t row_step = (uint64_t)(row_groups / bands) * kWaves;" in k
    tune = _src("capi.hip")
    assert "case PGENHIP_KNOB_SCAN_XCD_MAP: t.scan_xcd_map = value < 0 ? 0 : 1; break;" in tune
    assert "case PGENHIP_KNOB_SCAN_TWO_PASS: t.scan_two_pass = value < 0 ? 0 : 1; break;" in tune
    assert "case PGENHIP_KNOB_SCAN_ROWPICK: t.scan_rowpick = value < 0 ? 0 : 1; break;" in tune


def test_mirrored_row_owner_plan_matches_the_source():
    s = _src("gt_rowpick.hip")
    assert "inline uint32_t table_bytes(uint32_t K) { return (2u * (K + 8u) + 15u) & ~15u; }" in s
    assert "inline uint32_t rank_bytes(uint32_t n_seg) { return (4u * (n_seg + 1u) + 15u) & ~15u; }" in s
    assert "inline uint32_t codes_bytes(uint32_t K) { return ((K + 3u) / 4u + 16u + 15u) & ~15u; }" in s
    assert "constexpr uint32_t kStageBytes = kSegSamples / 4u;" in s
    p = _body("gt_rowpick.hip", "bool plan(const EmitArgs &a, const Tuning &t, int num_cus, bool compact, RowPickLaunch &L)")
    assert "L.lds = table_bytes(a.kept_count) + rank_bytes(L.n_seg) + (uint32_t)kWaves * (kStageBytes + codes_bytes(a.kept_count));" in p
    assert "if (L.n_seg < 1u || L.n_seg > 4096u || a.record_size < 16u) return false;" in p
    assert "const int want = t.rowpick_blocks_per_cu > 0 ? t.rowpick_blocks_per_cu : (!compact && a.sample_count < 24576u ? 4 : 2);" in p
    assert "if (want < per_cu) per_cu = want;" in p and "L.max_blocks = (uint32_t)per_cu * (uint32_t)num_cus;" in p
    a = _body("gt_rowpick.hip", "bool gt_rowpick_applicable(const EmitArgs &a, int num_cus)")
    assert ("a.kept_idx != nullptr && a.kept_count >= 1u && a.kept_count <= kRowPickMaxKept && a.record_size >= 16u && n_seg >= 1u && "
            "n_seg <= 4096u &&\n           (uint64_t)a.n_variants >= 8ull * (uint64_t)num_cus * kWaves;") in a
    assert (SP.ROWPICK_MAX_SEGS, SP.ROWPICK_ROWS_PER_WAVE) == (4096, 8)
    l = _body("gt_rowpick.hip", "hipError_t launch_gt_rowpick(")
    assert "dim3((uint32_t)(need < L.max_blocks ? need : L.max_blocks))" in l


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
