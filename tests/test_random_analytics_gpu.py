"""Randomised differential test of every analytics entry on shared cases (tests/random_cases.py; its CPU leg is
tests/test_random_cases.py).  Per case ONE context takes every entry (genotype_counts, sample_counts, decode_matrix, pair tables,
pair r^2, pair_mask, prune_resolve, pack_records, sample_scores, sample_pair_stats, variant_sums, sample_gram, gram_apply, parse_gt,
join_records) back to back in an order drawn from the seed, through the default dispatch and the default plans (no shape flag, no
knob), waiting only as often as PGENHIP_LAUNCHES_IN_FLIGHT demands, and every output is read after the last call: what one family
leaves on the context (counter ring, stream-ordered memsets, scratch) meets the next.  Outputs lie between sentinels at the least
alignment the header allows, with padded strides where an entry takes one.  Integer and byte outputs are exact; r^2 by
pair_ref.check_r2; FP64 outputs ``array_equal`` on integer inputs and inside the bound the family's own test asserts on real ones
(an ACCUMULATE call's prefill is one more term of the sum: the same bound with |prefill| added to its scale).  parse_gt and
join_records take contexts that keep every sample; on the others the test asserts that they refuse and write nothing.

A second test per seed runs the round trip across contexts of different N: pack_records -> decode_emit on a context of K samples ->
parse_gt, and pack_records of 2-8 contiguous parts of the keep list -> join_records.

30 seeds x 40 cases.  Measured on one MI355X: the whole file (60 tests) 54 s; ``test_every_entry_on_one_context`` 0.85 - 2.14 s per
seed (median 1.3 s, most of it the numpy references of ``random_cases.expected``), ``test_round_trip_chain_across_contexts``
0.27 - 0.60 s per seed.  A failure message carries the seed, the case index, the case's scalar fields and the call order; replay it
with ``run_case(RC.cases(seed)[index], ...)``."""
import numpy as np
import pytest
import torch

import join_ref as JR
import matrix_ref as MX
import pack_ref as PK
import pair_ref as PR
import parse_ref as PA
import pgen_rs_amd
import random_cases as RC
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_F = -12345.678
SENT_U = PR.SENT_U
SENT_B = 0xA5
TORCH_DTYPES = {"int8": torch.int8, "uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32, "float16": torch.float16,
                "bfloat16": torch.bfloat16, "float32": torch.float32}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Frame:
    """``rows`` x ``cols`` entries at a pitch of ``pitch`` elements, ``lead`` elements into a buffer filled with a sentinel."""

    def __init__(self, dtype, fill, rows, cols, pitch=None, lead=1, prefill=None):
        self.rows, self.cols, self.pitch, self.lead, self.fill = rows, cols, max(pitch or cols, 1), lead, fill
        self.buf = torch.full((lead + max(rows, 1) * self.pitch + 8,), fill, dtype=dtype, device=DEV)
        if prefill is not None and rows and cols:
            self.entries().copy_(dev(prefill).to(dtype))

    def entries(self):
        return self.buf[self.lead: self.lead + self.rows * self.pitch].view(self.rows, self.pitch)[:, :self.cols]

    @property
    def out(self):
        """The flat tensor a call gets: the buffer from the first entry on."""
        return self.buf[self.lead:]

    def untouched(self) -> bool:
        return bool((self.buf == self.fill).all())

    def take(self, np_view=None):
        """(the entries, whether everything around them still holds the sentinel), read back from the device."""
        t = self.buf.cpu()
        h = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().copy()
        if np_view is not None:
            h = h.view(np_view)
        fill = h.dtype.type(self.fill) if np_view is None and t.dtype != torch.bfloat16 else h[-1]   # the tail is never written
        body = h[self.lead: self.lead + self.rows * self.pitch].reshape(self.rows, self.pitch)
        got = body[:, :self.cols].copy()
        body[:, :self.cols] = fill
        return got, bool((h == fill).all())


class Queue:
    """Counts every call on the context and waits before the one that would exceed the header's allowance."""

    def __init__(self, eng):
        self.eng, self.in_flight, self.calls, self.waits = eng, 0, 0, 0

    def call(self, fn, *args, **kw):
        if self.in_flight == _capi.LAUNCHES_IN_FLIGHT:
            self.wait()
        self.in_flight += 1
        self.calls += 1
        return fn(*args, **kw)

    def wait(self):
        self.eng.wait()
        self.in_flight = 0
        self.waits += 1


def run_case(c, e, tag):
    n, v, k, w, n_left = c["n"], c["v"], c["k"], c["w"], c["n_left"]
    real = c["fp"] == "real"
    acc, pre = c["accumulate"], c["prefill"]
    problems = []

    def check(ok, what):
        if not ok:
            problems.append(what)

    with pgen_rs_amd.GtEngine(n, kept_idx=c["kept"], device=0) as eng:
        assert eng.kept_count == k and eng.record_size == c["r"], tag
        qu = Queue(eng)
        d_raw = dev(c["raw"])
        rows = c["rows"]
        at = "record_off" in rows
        if at:
            d_off = dev(rows["record_off"])
            sel = {}
        else:
            sel = dict(record_stride=rows["record_stride"], records_offset=rows["records_offset"], n_variants=v)
            if "variant_idx" in rows:
                sel["variant_idx"] = dev(rows["variant_idx"].view(np.int32))

        def rows_call(plain, at_fn, **kw):
            """The entry on the case's selection: the plain method with stride / offset / variant_idx, or its ``_at`` twin."""
            if at:
                return qu.call(at_fn, d_raw, d_off, **kw)
            return qu.call(plain, d_raw, **sel, **kw)

        words = (w + 31) // 32
        f = {}
        f["genotype_counts"] = Frame(torch.int32, SENT_U - (1 << 32), v, 4, lead=1)
        f["sample_counts"] = Frame(torch.int32, SENT_U - (1 << 32), k, 4, lead=1, prefill=pre["sample_counts"] if acc["sample_counts"] else None)
        mdt = TORCH_DTYPES[c["dtype"]]
        mrows, mcols = (k, v) if c["sample_major"] else (v, k)
        f["decode_matrix"] = Frame(mdt, 77, mrows, mcols, pitch=mcols + 3, lead=1)
        f["pair_tables"] = Frame(torch.int32, SENT_U - (1 << 32), n_left * w, 16, lead=4)          # 16-byte aligned
        f["pair_r2"] = Frame(torch.int32, SENT_U - (1 << 32), n_left, w, lead=1)
        f["fwd"] = Frame(torch.int32, SENT_U - (1 << 32), v, words, pitch=words + 1, lead=1)
        f["bwd"] = Frame(torch.int32, SENT_U - (1 << 32), v, words, pitch=words + 1, lead=1)
        f["fwd"].entries().zero_()
        f["bwd"].entries().zero_()
        f["prune_resolve"] = Frame(torch.uint8, SENT_B, 1, v, lead=3)
        f["prune_resolve"].entries().zero_()
        rk = (k + 3) // 4
        f["pack_records"] = Frame(torch.uint8, SENT_B, v, rk, pitch=rk + 5, lead=3)
        f["sample_scores"] = Frame(torch.float64, SENT_F, k, c["c_score"], lead=1, prefill=pre["sample_scores"] if acc["sample_scores"] else None)
        sa, sb, ga, gb = c["spair_a"], c["spair_b"], c["gram_a"], c["gram_b"]
        f["sample_pair_stats"] = Frame(torch.int32, SENT_U - (1 << 32), sa[1] * sb[1], 16, lead=4,
                                       prefill=pre["sample_pair_stats"].reshape(-1, 16) if acc["sample_pair_stats"] else None)
        f["variant_sums"] = Frame(torch.float64, SENT_F, v, 4 * c["c_vsum"], lead=1)
        f["sample_gram"] = Frame(torch.float64, SENT_F, ga[1], gb[1], pitch=gb[1] + 3, lead=1, prefill=pre["sample_gram"] if acc["sample_gram"] else None)
        cg = c["c_gapply"]
        f["gram_apply_p"] = Frame(torch.float64, SENT_F, v, cg, lead=1)
        f["gram_apply_y"] = Frame(torch.float64, SENT_F, k, cg, pitch=cg + 3, lead=1, prefill=pre["gram_apply"] if acc["gram_apply"] else None)
        # inputs
        d_w = torch.full((v, c["c_score"] + 2), 9.0, dtype=torch.float32, device=DEV)            # padded row stride
        d_w[:, :c["c_score"]] = dev(c["weights"])
        d_miss = None if c["miss"] is None else dev(c["miss"])
        d_vals = torch.full((k, c["c_vsum"] + 1), 9.0, dtype=torch.float64, device=DEV)
        d_vals[:, :c["c_vsum"]] = dev(c["values"])
        d_tab = dev(c["tables"])
        d_q = torch.full((k, cg + 2), 9.0, dtype=torch.float64, device=DEV)
        d_q[:, :cg] = dev(c["q"])
        d_fwd, d_bwd = dev(e["fwd"].view(np.int32)), dev(e["bwd"].view(np.int32))                 # prune_resolve is fed the masks directly
        d_prio = None if c["priority"] is None else dev(c["priority"].view(np.int32))
        refused = []
        t = c["parse"]
        lines = len(t["field_off"])
        f["parse_gt"] = Frame(torch.uint8, SENT_B, lines, c["r"], pitch=c["r"] + 3, lead=1)
        f["parse_flags"] = Frame(torch.int32, SENT_U - (1 << 32), 1, lines, lead=1)
        f["join_records"] = Frame(torch.uint8, SENT_B, v, c["r"], pitch=c["r"] + 2, lead=5)
        d_text = dev(np.concatenate([np.full(t["text_offset"], 9, dtype=np.uint8), np.frombuffer(t["text"], dtype=np.uint8)]))
        d_fo, d_le = dev(t["field_off"]), dev(t["line_end"])
        parts = [(dev(base), dev(off), n_p, None if flip is None else dev(flip)) for base, off, n_p, flip in c["join"]]

        def guarded(fn, *args, **kw):
            """parse_gt / join_records: on a proper subset the call must be refused."""
            if c["all_kept"]:
                return qu.call(fn, *args, **kw)
            try:
                qu.call(fn, *args, **kw)
            except _capi.PgenHipError as err:
                refused.append(err)
            else:
                problems.append(f"{fn.__name__} took a context that keeps a proper subset")

        def entry(name):
            if name == "genotype_counts":
                rows_call(eng.genotype_counts, eng.genotype_counts_at, out=f[name].out)
            elif name == "sample_counts":
                rows_call(eng.sample_counts, eng.sample_counts_at, out=f[name].out, accumulate=acc[name])
            elif name == "decode_matrix":
                fr = f[name]
                out = torch.as_strided(fr.buf, (mrows, mcols), (fr.pitch, 1), fr.lead)
                # numpy has no bfloat16: its four values are given as bit patterns; the other dtypes take the defaults
                values = torch.from_numpy(RC.BF16_VALUES.view(np.int16)).view(torch.bfloat16) if c["dtype"] == "bfloat16" else None
                rows_call(eng.decode_matrix, eng.decode_matrix_at, sample_major=c["sample_major"], out=out, values=values)
            elif name == "pair_tables":
                rows_call(eng.pair_tables, eng.pair_tables_at, n_left=n_left, window=w, out=f[name].out)
            elif name == "pair_r2":
                rows_call(eng.pair_r2, eng.pair_r2_at, n_left=n_left, window=w, out=f[name].out.view(torch.float32))
            elif name == "pair_mask":
                rows_call(eng.pair_mask, eng.pair_mask_at, n_left=n_left, window=w, min_r2=RC.MIN_R2, fwd=f["fwd"].out, bwd=f["bwd"].out,
                          mask_stride=words + 1)
            elif name == "prune_resolve":
                fr = f[name]
                state = fr.buf[fr.lead: fr.lead + v]
                _, calls = eng.prune_resolve(d_fwd, d_bwd, w, priority=d_prio, state=state)
                qu.calls += calls
                qu.in_flight = 0                     # the host loop waits after every call
            elif name == "pack_records":
                fr = f[name]
                rows_call(eng.pack_records, eng.pack_records_at, out=fr.buf, out_stride=fr.pitch, out_offset=fr.lead, code_map=c["code_map"])
            elif name == "sample_scores":
                if at:
                    qu.call(eng.sample_scores_at, d_raw, d_off, d_w[:, :c["c_score"]], miss=d_miss, out=f[name].out, accumulate=acc[name])
                else:
                    qu.call(eng.sample_scores, d_raw, d_w[:, :c["c_score"]], miss=d_miss, out=f[name].out, accumulate=acc[name], **sel)
            elif name == "sample_pair_stats":
                rows_call(eng.sample_pair_tables, eng.sample_pair_tables_at, a=sa, b=sb, out=f[name].out, accumulate=acc[name])
            elif name == "variant_sums":
                if at:
                    qu.call(eng.variant_sums_at, d_raw, d_off, d_vals[:, :c["c_vsum"]], out=f[name].out)
                else:
                    qu.call(eng.variant_sums, d_raw, d_vals[:, :c["c_vsum"]], out=f[name].out, **sel)
            elif name == "sample_gram":
                fr = f[name]
                if at:
                    qu.call(eng.sample_gram_at, d_raw, d_off, d_tab, a=ga, b=gb, out=fr.out, out_stride=fr.pitch, accumulate=acc[name])
                else:
                    qu.call(eng.sample_gram, d_raw, code_values=d_tab, a=ga, b=gb, out=fr.out, out_stride=fr.pitch, accumulate=acc[name], **sel)
            elif name == "gram_apply":
                kw = dict(proj=f["gram_apply_p"].out, out=f["gram_apply_y"].out, out_stride=f["gram_apply_y"].pitch, accumulate=acc[name])
                if at:
                    qu.call(eng.gram_apply_at, d_raw, d_off, d_tab, d_q[:, :cg], **kw)
                else:
                    qu.call(eng.gram_apply, d_raw, d_tab, d_q[:, :cg], **kw, **sel)
            elif name == "parse_gt":
                fr = f[name]
                guarded(eng.parse_gt, d_text, d_fo, d_le, out=fr.buf, out_stride=fr.pitch, out_offset=fr.lead, text_offset=t["text_offset"],
                        line_flags=f["parse_flags"].out)
            elif name == "join_records":
                fr = f[name]
                guarded(eng.join_records, parts, v, out=fr.buf, out_stride=fr.pitch, out_offset=fr.lead)
            else:
                raise KeyError(name)

        for name in c["order"]:
            entry(name)
        qu.wait()
        assert qu.calls >= len(RC.ENTRIES), tag

        # ---- everything is read only now -----------------------------------------------------------------------------------------
        def exact(name, want, np_view=None, what=None):
            got, intact = f[name].take(np_view)
            check(intact, f"{what or name}: wrote outside its entries")
            want = np.asarray(want).reshape(got.shape)
            if not np.array_equal(got.astype(np.int64) if got.dtype.kind in "iu" else got, want):
                bad = np.argwhere(got != want)
                check(False, f"{what or name}: {len(bad)} of {got.size} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")

        def close(name, want, bound, prefill, scale_of_one):
            """An FP64 output: equal on integer inputs; on real ones inside ``bound``, to which an ACCUMULATE call's prefill adds
            ``scale_of_one * |prefill|`` (the prefill is one more term of the any-order sum the bound is about)."""
            got, intact = f[name].take()
            check(intact, f"{name}: wrote outside its entries")
            want = np.asarray(want, dtype=np.float64).reshape(got.shape)
            if prefill is not None:
                prefill = prefill.reshape(got.shape)
                if real:
                    bound = np.broadcast_to(bound, got.shape) + scale_of_one * np.abs(prefill)
                want = want + prefill
            if not real:
                if not np.array_equal(got, want):
                    bad = np.argwhere(got != want)
                    check(False, f"{name}: {len(bad)} of {got.size} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
            else:
                err = np.abs(got - want)
                bound = np.broadcast_to(bound, got.shape)
                if not (err <= bound).all():
                    bad = np.argwhere(~(err <= bound))
                    i = tuple(bad[0])
                    check(False, f"{name}: {len(bad)} of {got.size} entries outside the bound, first at {list(i)}: got {got[i]!r}, want {want[i]!r}, bound {bound[i]!r}")

        u = 2.0 ** -53
        exact("genotype_counts", e["genotype_counts"])
        exact("sample_counts", e["sample_counts"] + (pre["sample_counts"] if acc["sample_counts"] else 0))
        want_m = e["decode_matrix"]
        exact("decode_matrix", want_m.view(np.int16) if c["dtype"] in ("bfloat16", "float16") else want_m.view(np.int32) if c["dtype"] == "float32" else want_m,
              np_view={"float16": np.int16, "float32": np.int32}.get(c["dtype"]))
        got, intact = f["pair_tables"].take(np.uint32)
        check(intact, "pair_tables: wrote outside its entries")
        got_r2, intact = f["pair_r2"].take(np.uint32)
        check(intact, "pair_r2: wrote outside its entries")
        try:
            PR.check_tables(got.reshape(n_left, w, 16), e["pair_tables"], v, "pair_tables")
            PR.check_r2(got_r2, e["pair_tables"], v, "pair_r2")
        except AssertionError as err:
            problems.append(str(err))
        exact("fwd", e["fwd"], np.uint32)
        exact("bwd", e["bwd"], np.uint32)
        exact("prune_resolve", e["prune_resolve"])
        exact("pack_records", e["pack_records"])
        exact("sample_pair_stats", e["sample_pair_stats"].reshape(-1, 16) + (pre["sample_pair_stats"].reshape(-1, 16) if acc["sample_pair_stats"] else 0))
        close("sample_scores", e["sample_scores"], e["sample_scores_bound"], pre["sample_scores"] if acc["sample_scores"] else None, 1.01 * (v + 1) * u)
        close("variant_sums", e["variant_sums"], np.broadcast_to(e["variant_sums_bound"][None, :, None], e["variant_sums"].shape).reshape(v, -1), None, 0.0)
        close("sample_gram", e["sample_gram"], 1.01 * (v + 2) * u * e["sample_gram_abs"], pre["sample_gram"] if acc["sample_gram"] else None, 1.01 * (v + 2) * u)
        close("gram_apply_p", e["gram_apply_p"], e["gram_apply_p_bound"], None, 0.0)
        close("gram_apply_y", e["gram_apply_y"], e["gram_apply_y_bound"], pre["gram_apply"] if acc["gram_apply"] else None, (v + k + 4) * u)
        if c["all_kept"]:
            exact("parse_gt", e["parse_gt"])
            exact("parse_flags", e["parse_flags"], np.uint32)
            exact("join_records", e["join_records"])
        else:
            check(len(refused) == 2 and all(err.status == _capi.ERR_BAD_ARG for err in refused), f"parse_gt / join_records on a subset: {refused}")
            for name in ("parse_gt", "parse_flags", "join_records"):
                check(f[name].untouched(), f"{name}: a refused call wrote")
    assert not problems, f"{tag} order={c['order']}: " + "; ".join(problems)


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_every_entry_on_one_context(seed):
    for c in RC.cases(seed):
        tag = f"seed={seed} case={c['index']} {RC.describe(c)}"
        run_case(c, RC.expected(c), tag)


def run_chain(c, tag):
    n, v, k, r = c["n"], c["v"], c["k"], c["r"]
    rng = np.random.default_rng(c["chain_seed"])
    kept = np.arange(n) if c["kept"] is None else c["kept"]
    rows = c["rows"]
    d_raw = dev(c["raw"])
    if "record_off" in rows:
        d_off = dev(rows["record_off"])
        pack = lambda eng, **kw: eng.pack_records_at(d_raw, d_off, **kw)
        emit = lambda eng: eng.decode_emit_at(d_raw, d_off, v)
    else:
        sel = dict(record_stride=rows["record_stride"], records_offset=rows["records_offset"], n_variants=v)
        if "variant_idx" in rows:
            sel["variant_idx"] = dev(rows["variant_idx"].view(np.int32))
        pack = lambda eng, **kw: eng.pack_records(d_raw, **sel, **kw)
        emit = lambda eng: eng.decode_emit(d_raw, **sel)
    rk = (k + 3) // 4
    with pgen_rs_amd.GtEngine(n, kept_idx=c["kept"], device=0) as eng:
        packed = pack(eng).contiguous()                       # (V, R_K), pad bits zero
        text = emit(eng)
        eng.wait()
    want_packed = PK.pack_codes(c["codes"])
    assert np.array_equal(packed.cpu().numpy(), want_packed), f"{tag}: pack_records"
    with pgen_rs_amd.GtEngine(k, device=0) as eng2:
        assert eng2.record_size == rk and eng2.gt_row_bytes == 4 * k + 1
        text2 = eng2.decode_emit(packed.view(-1), v)
        eng2.wait()
        assert torch.equal(text2[: v * (4 * k + 1)], text[: v * (4 * k + 1)]), f"{tag}: decode_emit of the packed records != decode_emit with the keep list"
        assert np.array_equal(MX.gt_text_codes(text2.cpu().numpy(), v, k), c["codes"]), f"{tag}: the text is not the case's codes"
        field_off = torch.arange(v, dtype=torch.int64, device=DEV) * (4 * k + 1)
        recs, flags = eng2.parse_gt(text2, field_off, field_off + 4 * k)
        eng2.wait()
        assert np.array_equal(recs.cpu().numpy(), PA.mask_pad(want_packed, k)) and not flags.any(), f"{tag}: parse_gt of the text"
        # the keep list in 2-8 contiguous parts, each packed on a context of its own, joined on the context of K samples
        cuts = np.sort(rng.integers(0, k + 1, size=min(c["chain_parts"], RC.MAX_PARTS) - 1))
        bounds = np.concatenate([[0], cuts, [k]])
        parts, host_parts = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            n_p = int(hi - lo)
            if n_p:
                with pgen_rs_amd.GtEngine(n, kept_idx=kept[lo:hi], device=0) as part_eng:
                    base = pack(part_eng).contiguous().view(-1)
                    part_eng.wait()
            else:
                base = torch.zeros(1, dtype=torch.uint8, device=DEV)
            off = np.arange(v, dtype=np.int64) * ((n_p + 3) // 4)
            flip = None if rng.random() < 0.5 else (rng.integers(1, 256, size=v) * (rng.random(v) < 0.3)).astype(np.uint8)
            parts.append((base, off, n_p, flip))
        for with_flip in (False, True):
            call = [(base, dev(off), n_p, dev(flip) if with_flip and flip is not None else None) for base, off, n_p, flip in parts]
            host = [(base.cpu().numpy(), off, n_p, flip if with_flip else None) for base, off, n_p, flip in parts]
            got = eng2.join_records(call, v)
            eng2.wait()
            want = JR.join(host, v)
            assert np.array_equal(got.cpu().numpy(), want), f"{tag}: join_records of {len(parts)} parts, flips {with_flip}"
            if not with_flip:
                assert np.array_equal(want, want_packed), f"{tag}: the joined parts are not the one-piece pack"


@pytest.mark.parametrize("seed", RC.SEEDS)
def test_round_trip_chain_across_contexts(seed):
    for c in RC.cases(seed):
        run_chain(c, f"seed={seed} case={c['index']} {RC.describe(c)}")

