"""Seeded random cases shared by every analytics entry (numpy only: no torch, no GPU).

``draw_case(rng)`` draws one case: a sample count N clustered on both sides of every edge the plan twins export, a keep list, V rows
in one of four layouts over one byte buffer with dirty gaps and dirty pad bits, LD-shaped codes, and the arguments of every family.
``expected(case)`` computes every entry's output from ONE (V, K) code matrix (``case["codes"]``: the selected rows, the kept samples)
with the references the family tests already trust; it adds no arithmetic of its own.  ``cases(seed)`` is the seed's list of cases,
``describe(case)`` the scalar fields a failure message carries (with the seed and the case index they replay the case).

FP inputs alternate by case index between small integers (every partial sum far below 2^53: the comparison is ``array_equal``) and
reals across 2^+-20 of mixed sign, drawn as the families' rounding legs draw them.  ``gapply_ref.apply_exact`` runs in Python
integers, V * K * C of them, so an odd case is real-valued only where that product is at most ``REAL_BUDGET``; above it the case is
an integer one, whose comparison is the stricter of the two.  ``parse_ref.parse_lines`` runs a regular expression per field, so a
case's text holds at most about ``PARSE_FIELDS`` fields: the first rows of the selection, one row at least."""
from __future__ import annotations

import functools

import numpy as np

import count_plan
import gapply_ref as AR
import gram_plan
import gram_ref as GR
import join_plan
import join_ref as JR
import matrix_plan
import matrix_ref as MX
import pack_ref as PK
import pair_ref as PR
import parse_plan
import parse_ref as PA
import prune_ref as R
import scount_plan
import score_ref as SC
import spair_ref as SP
import vsum_ref as VS

SEED_BASE = 91_000
SEEDS = range(30)
CASES_PER_SEED = 40
MIN_R2 = 0.21337          # test_pair_mask_gpu.py's threshold: no small rational sits next to its float32
REAL_BUDGET = 150_000     # V * K * C of a real-valued case (see the module docstring)
PARSE_FIELDS = 12_000
MAX_RANKS = 96            # ranks of a sample range of sample_pair_stats and sample_gram
N_UNIFORM = 9_000
MAX_PARTS = 8             # PGENHIP_JOIN_MAX_PARTS

V_LIST = [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 96]
W_LIST = [1, 5, 31, 32, 33, 40]
C_LIST = [1, 3, 8, 16]
KEEP_KINDS = ["none", "dense", "sparse", "tiny", "strided"]
LAYOUTS = ["dense", "strided", "gathered", "at"]
PRIORITY_KINDS = ["none", "u32", "ties", "constant"]       # the kinds of test_prune_resolve_gpu.py
DTYPES = ["int8", "uint8", "int16", "int32", "float16", "bfloat16", "float32"]
BF16_VALUES = np.array([0x0000, 0x3F80, 0x4000, 0x7FC0], dtype=np.uint16)   # 0, 1, 2, NaN as bfloat16 bit patterns
ACC_FAMILIES = ["sample_counts", "sample_scores", "sample_pair_stats", "sample_gram", "gram_apply"]
ENTRIES = ["genotype_counts", "sample_counts", "decode_matrix", "pair_tables", "pair_r2", "pair_mask", "prune_resolve", "pack_records",
           "sample_scores", "sample_pair_stats", "variant_sums", "sample_gram", "gram_apply", "parse_gt", "join_records"]

# every N edge of the plan twins; a case at an edge sits on it or one sample to either side
N_EDGES = sorted(set(count_plan.CLASS_EDGES) | set(scount_plan.CLASS_EDGES) | set(matrix_plan.N_EDGES)
                 | set(parse_plan.edge_sample_counts()) | {m * gram_plan.TILE for m in (1, 2, 3, 4)})
EDGE_NS = sorted({e + d for e in N_EDGES for d in (-1, 0, 1) if e + d >= 1})
EDGE_RECORD_SIZES = join_plan.edge_record_sizes()


def rsize(n: int) -> int:
    return (n + 3) // 4


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def draw_n(rng) -> int:
    p = rng.random()
    if p < 0.62:
        i = int(rng.integers(0, len(EDGE_NS) + len(EDGE_RECORD_SIZES)))
        if i < len(EDGE_NS):
            return EDGE_NS[i]
        return max(1, 4 * EDGE_RECORD_SIZES[i - len(EDGE_NS)] - int(rng.integers(0, 4)))   # any N of that record size
    if p < 0.72:
        return int(rng.integers(1, 6))
    return int(rng.integers(1, N_UNIFORM + 1))


def draw_keep(rng, n: int):
    """(kind, sorted kept list or None)"""
    kind = KEEP_KINDS[int(rng.choice(len(KEEP_KINDS), p=[0.28, 0.18, 0.18, 0.18, 0.18]))]
    if kind == "none":
        return kind, None
    if kind == "strided":
        step = int(rng.integers(2, 9))
        phase = [0, (n - 1) % step, int(rng.integers(0, step))][int(rng.integers(0, 3))]   # from sample 0, to sample N - 1, anywhere
        kept = np.arange(min(phase, n - 1), n, step)
    else:
        if kind == "dense":
            size = max(1, int(n * rng.uniform(0.40, 0.95)))
        elif kind == "sparse":
            size = max(1, int(n * rng.uniform(0.005, 0.10)))
        else:
            size = int(rng.integers(1, min(n, 5) + 1))
        kept = rng.choice(n, size=size, replace=False)
        ends = int(rng.integers(0, 4))            # bit 0: sample 0 is kept, bit 1: sample N - 1 is
        if ends & 1:
            kept[0] = 0
        if ends & 2:
            kept[-1] = n - 1
        kept = np.unique(kept)
    return kind, kept.astype(np.int64)


def dirty_pad(rng, recs: np.ndarray, n: int) -> np.ndarray:
    """The records with random pad bits in the last byte, at least one of them set in every row, where N % 4 != 0."""
    recs = recs.copy()
    if n % 4 and recs.size:
        shift = 2 * (n % 4)
        bits = rng.integers(0, 256, size=recs.shape[0]) >> shift
        bits[bits == 0] = 0xFF >> shift
        recs[:, -1] |= (bits << shift).astype(np.uint8)
    return recs


def draw_layout(rng, layout: str, v: int, r: int):
    """Where the file's rows lie in one random byte buffer and which of them the call selects, in call order:
    (file rows, (file rows,) byte offsets, buffer size, the selection's arguments, (V,) file row of every selected row)."""
    if layout == "dense":
        v_file = v
        base = 2 * int(rng.integers(0, 8)) + 1
        offs = base + r * np.arange(v_file, dtype=np.int64)
        args = dict(records_offset=base, record_stride=r)
        sel = np.arange(v)
    elif layout == "strided":
        v_file = v
        base = int(rng.choice([1, 2, 3, 5, 6, 7, 9, 13]))
        stride = r + int(rng.integers(1, 20))
        offs = base + stride * np.arange(v_file, dtype=np.int64)
        args = dict(records_offset=base, record_stride=stride)
        sel = np.arange(v)
    elif layout == "gathered":
        v_file = v + int(rng.integers(1, v + 2))
        base = int(rng.integers(0, 8))
        stride = r + int(rng.choice([0, 0, 1, 5]))
        offs = base + stride * np.arange(v_file, dtype=np.int64)
        runs = []
        while sum(len(q) for q in runs) < v:       # descending runs, a row now and then twice in a row
            start, length = int(rng.integers(0, v_file)), int(rng.integers(1, 6))
            run = np.maximum(start - np.arange(length), 0)
            runs.append(np.repeat(run, rng.integers(1, 3, size=length)) if rng.random() < 0.3 else run)
        sel = np.concatenate(runs)[:v]
        if v >= 2:
            sel[-1] = sel[0]
        args = dict(records_offset=base, record_stride=stride, variant_idx=sel.astype(np.uint32))
    else:
        v_file = v + int(rng.integers(0, v + 1))
        gaps = rng.integers(0, 6, size=v_file)     # offsets of mixed parity
        offs = int(rng.integers(0, 8)) + np.cumsum(gaps + r) - r
        sel = rng.permutation(v_file)[:v]
        args = dict(record_off=offs[sel].astype(np.int64))
    size = int(offs[-1]) + r + int(rng.integers(0, 17))
    return v_file, offs.astype(np.int64), size, args, sel.astype(np.int64)


def draw_range(rng, k: int):
    """(begin, count): at most MAX_RANKS ranks, one time in three ending at K."""
    count = int(rng.integers(1, min(k, MAX_RANKS) + 1))
    begin = k - count if rng.random() < 1 / 3 else int(rng.integers(0, k - count + 1))
    return begin, count


def reals(rng, shape):
    """Reals across 2^+-20 of mixed sign (the rounding legs of test_sample_gram_gpu.py and test_gram_apply_gpu.py)."""
    return rng.standard_normal(shape) * np.exp2(rng.uniform(-20, 20, size=shape))


def signed_reals(rng, shape):
    """The same as the rounding legs of test_variant_sums_gpu.py and test_sample_scores_gpu.py draw them."""
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(1.0, 2.0, size=shape) * 2.0 ** rng.uniform(-20.0, 20.0, size=shape)


def draw_parse(rng, rows: np.ndarray, n: int):
    """Text of the first rows of the selection, about PARSE_FIELDS fields: fixed-width lines of the rows' own codes and lines of the
    grammar's forms (tests/parse_ref.py FORMS), some a field short or long, behind prefixes of random length."""
    lines = min(rows.shape[0], max(1, PARSE_FIELDS // n))
    fixed = {"/": np.frombuffer(b"\t0/0\t0/1\t1/1\t./.", dtype=np.uint8).reshape(4, 4),
             "|": np.frombuffer(b"\t0|0\t1|0\t1|1\t.|.", dtype=np.uint8).reshape(4, 4)}
    text, field_off, line_end = bytearray(rng.integers(33, 127, size=int(rng.integers(0, 9)), dtype=np.uint8).tobytes()), [], []
    for j in range(lines):
        text += rng.integers(33, 127, size=int(rng.integers(0, 30)), dtype=np.uint8).tobytes()
        if rng.random() < 0.6:
            region = fixed["/" if rng.random() < 0.7 else "|"][rows[j]].tobytes()
        else:
            count = max(0, n + int(rng.choice([0, 0, 0, 0, -1, 1])))
            region = b"".join(b"\t" + PA.FORMS[i][0] for i in rng.integers(0, len(PA.FORMS), size=count))
        field_off.append(len(text))
        text += region
        line_end.append(len(text))
        text += b"\n"
    return dict(text=bytes(text), field_off=np.array(field_off, dtype=np.int64), line_end=np.array(line_end, dtype=np.int64),
                text_offset=2 * int(rng.integers(0, 4)) + 1)


def draw_join(rng, rows: np.ndarray, n: int):
    """The selection's N samples cut into 2-8 contiguous parts (a part may be empty), each a buffer of its own with its rows in
    permuted order at offsets of any parity, dirty pad bits, a row absent now and then, flip bytes or none."""
    v = rows.shape[0]
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(1, MAX_PARTS))))
    bounds = np.concatenate([[0], cuts, [n]])
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        n_p = int(hi - lo)
        r_p = rsize(n_p)
        recs = dirty_pad(rng, PK.pack_codes(rows[:, lo:hi]), n_p) if n_p else np.zeros((v, 0), dtype=np.uint8)
        order = rng.permutation(v)
        place = int(rng.integers(0, 8)) + np.cumsum(rng.integers(0, 4, size=v) + r_p) - r_p
        base = rng.integers(0, 256, size=int(place[-1]) + r_p + int(rng.integers(1, 9)), dtype=np.uint8)
        off = np.empty(v, dtype=np.int64)
        for slot, j in enumerate(order):
            off[j] = place[slot]
            base[place[slot]: place[slot] + r_p] = recs[j]
        off[rng.random(v) < 0.1] = JR.ABSENT
        flip = None if rng.random() < 0.4 else (rng.integers(1, 256, size=v) * (rng.random(v) < 0.3)).astype(np.uint8)
        parts.append((base, off, n_p, flip))
    return parts


def draw_case(rng, index: int = 0) -> dict:
    """One case; ``index`` (its place in the seed's list) decides the kind of the FP inputs."""
    c = {"index": index}
    n = c["n"] = draw_n(rng)
    c["keep_kind"], kept = draw_keep(rng, n)
    if n < 2 and c["keep_kind"] not in ("none", "tiny"):
        c["keep_kind"], kept = "none", None
    c["kept"] = kept
    k = c["k"] = n if kept is None else int(kept.size)
    c["all_kept"] = k == n                 # no list, or the identity: parse_gt and join_records take the context
    v = c["v"] = int(rng.choice(V_LIST))
    r = c["r"] = rsize(n)
    layout = c["layout"] = LAYOUTS[int(rng.integers(0, len(LAYOUTS)))]
    c["v_file"], offs, size, c["rows"], sel = draw_layout(rng, layout, v, r)
    c["redraw"], c["fresh_every"], c["missing"] = float(rng.choice([0.05, 0.2, 1.0])), int(rng.choice([0, 7])), float(rng.choice([0.0, 0.02, 0.3]))
    codes_file = R.ld_codes(rng, c["v_file"], n, redraw=c["redraw"], fresh_every=c["fresh_every"], missing=c["missing"])
    recs_file = dirty_pad(rng, PK.pack_codes(codes_file), n)
    raw = rng.integers(0, 256, size=size, dtype=np.uint8)      # every gap byte random
    for i in range(c["v_file"]):
        raw[offs[i]: offs[i] + r] = recs_file[i]
    c["raw"] = raw
    c["recs_sel"] = np.stack([raw[offs[i]: offs[i] + r] for i in sel])      # (V, R), read back from the buffer the calls read
    c["rows_all"] = codes_file[sel]                                          # (V, N)
    c["codes"] = c["rows_all"] if kept is None else c["rows_all"][:, kept]   # (V, K): what every expectation is computed from

    # per-family arguments
    c["w"] = int(rng.choice(W_LIST))
    c["n_left"] = [v, v // 2, 0][int(rng.integers(0, 3))]
    c["c"] = int(rng.choice(C_LIST))
    c["c_score"], c["c_vsum"], c["c_gapply"] = min(c["c"], 8), min(c["c"], 16), min(c["c"], 16)
    c["spair_a"], c["spair_b"] = draw_range(rng, k), draw_range(rng, k)
    c["gram_a"], c["gram_b"] = draw_range(rng, k), draw_range(rng, k)
    if rng.random() < 0.25:
        c["spair_b"] = c["spair_a"]
    if rng.random() < 0.25:
        c["gram_b"] = c["gram_a"]
    c["sample_major"] = bool(rng.integers(0, 2))
    c["dtype"] = DTYPES[int(rng.integers(0, len(DTYPES)))]
    c["code_map"] = [None, PK.BED_MAP, tuple(int(x) for x in rng.permutation(4)), tuple(int(x) for x in rng.integers(0, 4, size=4))][int(rng.integers(0, 4))]
    c["accumulate"] = {f: bool(rng.integers(0, 2)) for f in ACC_FAMILIES}
    c["priority_kind"] = PRIORITY_KINDS[int(rng.integers(0, len(PRIORITY_KINDS)))]
    c["priority"] = {"none": None, "u32": rng.integers(0, 1 << 32, size=v, dtype=np.uint64).astype(np.uint32),
                     "ties": rng.integers(0, 3, size=v).astype(np.uint32), "constant": np.full(v, 7, dtype=np.uint32)}[c["priority_kind"]]
    c["fp"] = "real" if index % 2 and v * k * c["c_gapply"] <= REAL_BUDGET else "int"
    if c["fp"] == "int":
        c["weights"] = rng.integers(-8, 9, size=(v, c["c_score"])).astype(np.float32)
        c["miss"] = None if rng.random() < 0.3 else rng.integers(0, 3, size=v).astype(np.float32)
        c["values"] = rng.integers(-4, 5, size=(k, c["c_vsum"])).astype(np.float64)
        c["tables"] = rng.integers(-8, 9, size=(v, 4)).astype(np.float64)
        c["q"] = rng.integers(-4, 5, size=(k, c["c_gapply"])).astype(np.float64)
        fill = lambda shape: rng.integers(-1000, 1001, size=shape).astype(np.float64)
    else:
        c["weights"] = signed_reals(rng, (v, c["c_score"])).astype(np.float32)
        c["miss"] = rng.uniform(0.0, 2.0, size=v).astype(np.float32)
        c["values"] = signed_reals(rng, (k, c["c_vsum"]))
        c["tables"] = reals(rng, (v, 4))
        c["q"] = reals(rng, (k, c["c_gapply"]))
        fill = lambda shape: reals(rng, shape)
    # what an output holds before an ACCUMULATE call
    c["prefill"] = {"sample_counts": rng.integers(0, 1000, size=(k, 4)).astype(np.int64),
                    "sample_pair_stats": rng.integers(0, 1000, size=(c["spair_a"][1], c["spair_b"][1], 4, 4)).astype(np.int64),
                    "sample_scores": fill((k, c["c_score"])), "sample_gram": fill((c["gram_a"][1], c["gram_b"][1])),
                    "gram_apply": fill((k, c["c_gapply"]))}
    c["order"] = [ENTRIES[i] for i in rng.permutation(len(ENTRIES))]
    c["parse"] = draw_parse(rng, c["rows_all"], n)
    c["join"] = draw_join(rng, c["rows_all"], n)
    c["chain_parts"] = int(rng.integers(2, 9))
    c["chain_seed"] = int(rng.integers(0, 1 << 31))
    return c


@functools.lru_cache(maxsize=2)
def cases(seed: int) -> list:
    rng = np.random.default_rng(SEED_BASE + seed)
    return [draw_case(rng, i) for i in range(CASES_PER_SEED)]


def describe(case: dict) -> dict:
    """The scalar fields of a case."""
    out = {key: val for key, val in case.items() if isinstance(val, (bool, int, float, str, tuple)) or val is None}
    out["accumulate"] = [f for f, on in case["accumulate"].items() if on]
    out["rows"] = {key: (val if np.isscalar(val) else f"[{len(val)}]") for key, val in case["rows"].items()}
    return out


# ---- every output, from the one code matrix ----------------------------------------------------------------------------------------
def matrix_values(dtype: str) -> np.ndarray:
    return BF16_VALUES if dtype == "bfloat16" else MX.default_values(np.dtype(dtype))


def counts(codes: np.ndarray, axis: int) -> np.ndarray:
    """bincount of the codes along rows (axis 1: per variant) or columns (axis 0: per sample): (., 4) int64."""
    lines = codes if axis == 1 else codes.T
    return np.stack([np.bincount(line, minlength=4) for line in lines]).astype(np.int64).reshape(-1, 4)


def cols(codes: np.ndarray, rng_: tuple) -> np.ndarray:
    return codes[:, rng_[0]: rng_[0] + rng_[1]]


def expected(case: dict) -> dict:
    c, codes = case, case["codes"]
    v, k, n, kept = c["v"], c["k"], c["n"], c["kept"]
    e = {}
    e["genotype_counts"] = counts(codes, 1)
    e["sample_counts"] = counts(codes, 0)
    e["decode_matrix"] = MX.matrix(c["recs_sel"], n, kept, matrix_values(c["dtype"]), c["sample_major"])
    e["pair_tables"] = PR.pair_tables(codes, c["n_left"], c["w"], fill=-1)
    e["edges"] = R.edges(codes, c["n_left"], c["w"], MIN_R2)          # raises ThresholdTooClose: the module's own guard
    e["fwd"], e["bwd"] = R.masks(e["edges"])
    e["prune_resolve"] = R.resolve(e["fwd"], e["bwd"], c["w"], c["priority"])
    e["pack_records"] = PK.pack(c["recs_sel"], n, kept, c["code_map"])
    e["sample_scores"], a = SC.score_from_codes(codes, c["weights"], c["miss"])
    e["sample_scores_bound"] = SC.bound(v, a)
    e["sample_pair_stats"] = SP.ranges(codes, c["spair_a"], c["spair_b"])
    e["variant_sums"], a = VS.vsum_from_codes(codes, c["values"])
    e["variant_sums_bound"] = VS.bound(k, a)
    ca, cb = cols(codes, c["gram_a"]), cols(codes, c["gram_b"])
    e["sample_gram"] = GR.gram_ref(ca, c["tables"], cb) if c["fp"] == "int" else GR.gram_fsum(ca, c["tables"], cb)
    e["sample_gram_abs"] = GR.gram_abs(ca, c["tables"], cb)
    if c["fp"] == "int":
        p, y = AR.apply_int(codes, c["tables"], c["q"])
        e["gram_apply_p"], e["gram_apply_y"] = p.astype(np.float64), y.astype(np.float64)
    else:
        e["gram_apply_p"], e["gram_apply_y"] = AR.apply_exact(codes, c["tables"], c["q"])
    e["gram_apply_p_bound"], e["gram_apply_y_bound"] = AR.apply_bounds(codes, c["tables"], c["q"])
    if c["all_kept"]:
        t = c["parse"]
        e["parse_gt"], e["parse_flags"] = PA.parse_lines(t["text"], t["field_off"], t["line_end"], n)
        e["join_records"] = JR.join(c["join"], v)
    return e


def nonempty(case: dict, e: dict) -> dict:
    """Per FP64 family, the entries whose exact sum has a nonzero term (the others are exact zeros with a zero scale or no sample)."""
    return {"sample_scores": e["sample_scores_bound"] > 0,
            "variant_sums": np.broadcast_to((e["genotype_counts"] > 0)[:, None, :], e["variant_sums"].shape),
            "sample_gram": e["sample_gram_abs"] > 0,
            "gram_apply_p": e["gram_apply_p_bound"] > 0, "gram_apply_y": e["gram_apply_y_bound"] > 0}
