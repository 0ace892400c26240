"""Gram product — GPU leg (pgenhip_gram_apply / _at through GtEngine), GENERAL, MFMA and AUTO.
Exact leg: integer tables in [-8, 8] and integer Q in [-4, 4] make every partial sum an integer far below 2^53, so every shape must
equal the int64 reference (tests/gapply_ref.py) bit for bit: sample counts around the 16-sample MFMA tile, the 64-sample step and the
256-sample block tile, row counts around the 64-row step and tile, every column count that changes the staged tile, both slice knobs
(26, 27) at 1, 2 and 7 and the default plan, a 2 504-sample row, few rows of 70 001 samples.  Layouts: keep sets x row layouts, with
q_stride > C, out_stride > C and sentinel doubles around and between the rows of d_out and around d_proj.  Map leg: real tables and a Q
of all-distinct entries on a rectangular shape, every entry inside the documented bound, so a transposed fragment map cannot pass.
Cross-checks against sample_gram and variant_sums.  Rounding leg: random FP64 tables and Q across 2^+-20 against the correctly
rounded results.  ACCUMULATE, streams, a captured graph, every refusal."""
import math

import numpy as np
import pytest
import torch

import gapply_plan as AP
import gapply_ref as AR
import gram_ref as GR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -12345.678
KERNELS = {"general": _capi.GAPPLY_GENERAL, "mfma": _capi.GAPPLY_MFMA, "auto": _capi.GAPPLY_AUTO}
C_LIST = [1, 2, 7, 8, 15, 16]


def int_tables(v, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(v, 4)).astype(np.float64)


def int_q(k, c, seed):
    return np.random.default_rng(1000 + seed).integers(-4, 5, size=(k, c)).astype(np.float64)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_apply(eng, tables, q, at=None, pad=3, accumulate_onto=None, **kw):
    """(P, Y) computed into dirty buffers: Q has `pad` more doubles per row than columns, d_out has `pad` sentinel doubles behind every
    row and four on either side, d_proj four on either side; nothing but the entries may change.  accumulate_onto: what the K x C entries
    hold before an ACCUMULATE call."""
    k, (v, c) = eng.kept_count, (tables.reshape(-1, 4).shape[0], q.shape[1])
    assert q.shape[0] == k
    d_q = torch.full((max(k, 1), c + pad), SENT, dtype=torch.float64, device=DEV)[:k]
    d_q[:, :c] = dev(q)
    stride = c + pad
    obuf = torch.full((4 + max(k, 1) * stride + 4,), SENT, dtype=torch.float64, device=DEV)
    if accumulate_onto is not None:
        obuf[4:4 + k * stride].view(k, stride)[:, :c] = dev(accumulate_onto)
        kw["accumulate"] = True
    pbuf = torch.full((4 + max(v * c, 1) + 4,), SENT, dtype=torch.float64, device=DEV)
    d_t = dev(tables.reshape(-1, 4))
    args = dict(proj=pbuf[4:], out=obuf[4:], out_stride=stride, **kw)
    if at is not None:
        proj, out = eng.gram_apply_at(at[0], at[1], d_t, d_q[:, :c], **args)
    else:
        proj, out = eng.gram_apply(code_values=d_t, q=d_q[:, :c], **args)
    eng.wait()
    assert proj.shape == (v, c) and out.shape == (k, c) and proj.dtype == out.dtype == torch.float64
    pframe, oframe = pbuf.cpu().numpy().copy(), obuf.cpu().numpy().copy()
    p = pframe[4:4 + v * c].reshape(v, c).copy()
    pframe[4:4 + v * c] = SENT
    assert (pframe == SENT).all(), "wrote outside d_proj's entries"
    body = oframe[4:4 + max(k, 1) * stride].reshape(-1, stride)
    y = body[:k, :c].copy()
    body[:k, :c] = SENT
    assert (oframe == SENT).all(), "wrote outside d_out's entries"
    assert (d_q[:, c:] == SENT).all()
    return p, y


def check_all(eng, codes, tables, q, at=None, what="", **kw):
    """Every shape against the int64 reference, bit for bit."""
    wp, wy = AR.apply_int(codes, tables, q)
    for name, kernel in KERNELS.items():
        p, y = run_apply(eng, tables, q, at=at, kernel=kernel, **kw)
        assert np.array_equal(p, wp.astype(np.float64)), f"{name} P {what}"
        assert np.array_equal(y, wy.astype(np.float64)), f"{name} Y {what}"


def synth_codes(eng, v, n, first_variant=0, kept=None):
    d = eng.synth_records(max(v, 1), first_variant=first_variant, hwe=True)
    return d, GR.unpack(d.cpu().numpy()[: v * eng.record_size].reshape(v, -1), n, kept)


N_LIST = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257, 300]


@pytest.mark.parametrize("n", N_LIST)
def test_sample_count_edges(n):
    v, c = 67, C_LIST[N_LIST.index(n) % len(C_LIST)]
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 2)
        check_all(eng, codes, int_tables(v, n), int_q(n, c, n), records=d, n_variants=v)


V_LIST = [0, 1, 3, 4, 5, 31, 32, 33, 63, 65, 1000]


@pytest.mark.parametrize("knob", ["sample", "row", "both"])
@pytest.mark.parametrize("slices", [1, 2, 7])
def test_row_count_edges_at_forced_slices(knob, slices):
    n = 300
    assert AP.plan(1000, n, 7, True, 7, 7)[4:] == (5, 7)   # both passes really are cut
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        if knob != "row":
            eng.tune(_capi.KNOB_GAPPLY_SAMPLE_SLICES, slices)
        if knob != "sample":
            eng.tune(_capi.KNOB_GAPPLY_ROW_SLICES, slices)
        d, codes = synth_codes(eng, V_LIST[-1], n, 5)
        t = int_tables(V_LIST[-1], slices)
        for i, v in enumerate(V_LIST):
            c = C_LIST[(i + slices) % len(C_LIST)]
            check_all(eng, codes[:v], t[:v], int_q(n, c, v), records=d, n_variants=v, what=f"V = {v}, C = {c}")


@pytest.mark.parametrize("c", C_LIST)
def test_column_counts_on_the_default_plan(c):
    n, v = 130, 70
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 1)
        check_all(eng, codes, int_tables(v, c), int_q(n, c, c), records=d)


def test_default_plan_cuts_many_row_slices():
    n, v = 130, 5000
    assert AP.plan(v, n, 4, True).row_slices > 7 and AP.plan(v, n, 4, False).row_slices > 7
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n)
        check_all(eng, codes, int_tables(v, 3), int_q(n, 4, 3), records=d)


def test_the_two_ends_of_a_2504_sample_row():
    """The whole row, and through a kept list its first 70 and last 67 samples only."""
    n, v = 2504, 131
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 3)
        check_all(eng, codes, int_tables(v, 9), int_q(n, 5, 9), records=d)
    ends = list(range(70)) + list(range(n - 67, n))
    with pgen_rs_amd.GtEngine(n, kept_idx=ends, device=0) as eng:
        check_all(eng, codes[:, ends], int_tables(v, 10), int_q(len(ends), 16, 10), records=d, what="the two ends")


def test_few_rows_of_70001_samples():
    """Few long rows: the default plan must split the samples of the P pass; the Y pass has one slice."""
    n, v = 70_001, 5
    assert AP.plan(v, n, 3, True).sample_slices > 7 and AP.plan(v, n, 3, True).row_slices == 1
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 7)
        check_all(eng, codes, int_tables(v, 4), int_q(n, 3, 4), records=d)
        eng.tune(_capi.KNOB_GAPPLY_SAMPLE_SLICES, 1)
        check_all(eng, codes, int_tables(v, 4), int_q(n, 3, 5), records=d, what="one sample slice")


def kept_sets(n, rng):
    return {"all": None, "identity": list(range(n)), "none": [], "last": [n - 1], "every7": list(range(0, n, 7)),
            "cluster": list(range(n // 2 - 40, n // 2 + 41)),
            "holes": sorted(set(range(n)) - set(rng.choice(n, size=n // 5, replace=False).tolist()))}


@pytest.mark.parametrize("keep", ["all", "identity", "none", "last", "every7", "cluster", "holes"])
def test_keep_sets_and_layouts(keep):
    n = 299
    rng = np.random.default_rng(43 + len(keep))
    kept = kept_sets(n, rng)[keep]
    r = GR.rsize(n)
    v = 75
    stride = r + 5
    # strided rows at an unaligned base, every byte random (pad bits of the last record byte dirty)
    raw = rng.integers(0, 256, size=3 + v * stride, dtype=np.uint8)
    recs = np.stack([raw[3 + i * stride: 3 + i * stride + r] for i in range(v)])
    assert (recs[:, -1] >> (2 * (n % 4))).any(), "the pad bits are clean"
    codes = GR.unpack(recs, n, kept)
    k = codes.shape[1]
    d_raw = dev(raw)
    gather = np.concatenate([np.arange(v - 1, -1, -2), np.arange(v - 1, v // 2, -3)]).astype(np.int32)   # descending, with repeats
    d_gather = dev(gather)
    d_offs = dev(np.array([3 + i * stride for i in gather], dtype=np.int64))   # odd and even byte offsets
    dense = dev(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)]))
    t = int_tables(v, 7)
    tg = int_tables(len(gather), 8)   # tables go with the position in the selection, not with the row number
    q = int_q(k, 13, 7)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        assert eng.kept_count == k
        check_all(eng, codes, t, q, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, what="padded stride")
        check_all(eng, codes[gather], tg, q, records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather, what="gathered with repeats")
        check_all(eng, codes[gather], tg, q, at=(d_raw, d_offs), what="_at, odd offsets")
        check_all(eng, codes, t, q, records=dense, records_offset=1, what="dense from an odd base")
        check_all(eng, codes[-1:], t[:1], q[:, :1], records=dense, records_offset=1 + r * (v - 1), n_variants=1, what="one row, one column")


@pytest.mark.parametrize("n", [5, 299])
def test_dirty_pad_bits_are_not_samples(n):
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        v = 67
        d = eng.synth_records(v, first_variant=1, dirty_pad=True)
        recs = d.cpu().numpy()[: v * eng.record_size].reshape(v, -1)
        assert (recs[:, -1] >> (2 * (n % 4))).any(), "the generator left the pad bits clean"
        check_all(eng, GR.unpack(recs, n), int_tables(v, n), int_q(n, 6, n), records=d, n_variants=v)


def hwe_records(n, v, seed):
    """(V, R) records of Hardy-Weinberg genotypes with 1 % missing calls, drawn on the host, and their (V, n) codes."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, size=(v, 1))
    codes = (rng.random((v, n)) < p).astype(np.uint8) + (rng.random((v, n)) < p).astype(np.uint8)
    codes[rng.random((v, n)) < 0.01] = 3
    padded = np.zeros((v, 4 * GR.rsize(n)), dtype=np.uint8)
    padded[:, :n] = codes
    quads = padded.reshape(v, -1, 4)
    return (quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6).astype(np.uint8), codes


def within(got, want, bound, what):
    """Every entry within the documented bound of the correctly rounded value (whose own half ulp the bound's room covers)."""
    err = np.abs(got - want)
    frac = float((err / np.where(bound > 0, bound, 1.0)).max(initial=0.0))
    print(f"{what}: worst error / bound = {frac:.4f}")
    assert (err <= bound).all(), f"{what}: worst error / bound = {frac}"
    return frac


def test_map_leg_real_tables_and_distinct_q():
    """V = 70, K = 37, C = 13: no two of the three extents are equal and no entry of Q repeats, so a transposed A, B or D fragment map
    puts a wrong value into every entry; all of them must be inside the documented bounds."""
    n, v, c = 37, 70, 13
    recs, codes = hwe_records(n, v, 2)
    assert np.array_equal(GR.unpack(recs, n), codes)
    t, _, _ = GR.grm_tables(GR.variant_counts(codes))
    q = (np.random.default_rng(3).permutation(n * c).reshape(n, c) + 1.0) / 7.0
    assert len(np.unique(q)) == q.size
    wp, wy = AR.apply_exact(codes, t, q)
    bp, by = AR.apply_bounds(codes, t, q)
    assert (np.abs(wy) > 100 * by).mean() > 0.9, "the bound does not tell a right entry from a wrong one"
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d = dev(recs.reshape(-1))
        for name, kernel in KERNELS.items():
            p, y = run_apply(eng, t, q, records=d, kernel=kernel)
            within(p, wp, bp, f"map {name} P")
            within(y, wy, by, f"map {name} Y")


def exact_matmul(a, b):
    """a @ b with every entry correctly rounded (error-free products, math.fsum)."""
    out = np.zeros((a.shape[0], b.shape[1]))
    for i in range(a.shape[0]):
        for l in range(b.shape[1]):
            pr = a[i] * b[:, l]
            out[i, l] = math.fsum(np.concatenate([pr, GR._two_product_err(a[i], b[:, l], pr)]).tolist())
    return out


def test_cross_checks_against_sample_gram_and_variant_sums():
    """Y against sample_gram's full square times Q, P against sum over x of t_j[x] * variant_sums[j, c, x]: each within the sum of
    the two entry points' documented bounds (the host-side products are correctly rounded)."""
    n, v, c = 131, 400, 6
    rng = np.random.default_rng(11)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 4)
        t, _, _ = GR.grm_tables(GR.variant_counts(codes))
        q = rng.standard_normal((n, c))
        d_t, d_q = dev(t), dev(q)
        gram = eng.sample_gram(d, code_values=d_t).cpu().numpy()
        sums = eng.variant_sums(d, d_q).cpu().numpy()           # (V, C, 4)
        bp, by = AR.apply_bounds(codes, t, q)
        y_other = exact_matmul(gram, q)
        by_other = ((v + 2) * 2.0 ** -53 * GR.gram_abs(codes, t)) @ np.abs(q)
        p_other = np.array([[math.fsum((t[j] * sums[j, l]).tolist()) for l in range(c)] for j in range(v)])
        bp_other = np.abs(t).sum(axis=1, keepdims=True) * ((n + 1) * 2.0 ** -53 * np.abs(q).sum(axis=0, keepdims=True))
        for name, kernel in KERNELS.items():
            p, y = run_apply(eng, t, q, records=d, kernel=kernel)
            within(y, y_other, by + by_other, f"cross {name} Y vs sample_gram @ Q")
            within(p, p_other, bp + bp_other, f"cross {name} P vs variant_sums")


@pytest.mark.parametrize("v", [64, 1000])
def test_rounding_leg_inside_the_documented_bound(v):
    """Random FP64 tables and Q across 2^-20 .. 2^20: every entry of P and of Y within the header's bound of the correctly rounded
    result, on the default plan and with both passes cut into slices."""
    n, c = 100, 5
    rng = np.random.default_rng(v)
    t = rng.standard_normal((v, 4)) * np.exp2(rng.uniform(-20, 20, size=(v, 4)))
    q = rng.standard_normal((n, c)) * np.exp2(rng.uniform(-20, 20, size=(n, c)))
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, codes = synth_codes(eng, v, n, 8)
        wp, wy = AR.apply_exact(codes, t, q)
        bp, by = AR.apply_bounds(codes, t, q)
        for slices in (0, 2):
            eng.tune(_capi.KNOB_GAPPLY_SAMPLE_SLICES, slices)
            eng.tune(_capi.KNOB_GAPPLY_ROW_SLICES, slices)
            for name, kernel in KERNELS.items():
                p, y = run_apply(eng, t, q, records=d, kernel=kernel)
                within(p, wp, bp, f"rounding V={v} {name} slices={slices} P")
                within(y, wy, by, f"rounding V={v} {name} slices={slices} Y")


@pytest.mark.parametrize("n,keep", [(70, "all"), (300, "holes")])
def test_accumulate_and_overwrite(n, keep):
    kept = kept_sets(n, np.random.default_rng(n))[keep]
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        v, half, c = 301, 123, 9
        d, codes = synth_codes(eng, v, n, 0, kept)
        r, k = eng.record_size, eng.kept_count
        t, q = int_tables(v, 5), int_q(k, c, 5)
        wp, wy = AR.apply_int(codes, t, q)
        d_t, d_q = dev(t), dev(q)
        # real tables: the two halves summed in place equal one call within the bound
        tr, _, _ = GR.grm_tables(GR.variant_counts(codes))
        qr = np.random.default_rng(6).standard_normal((k, c))
        _, ey = AR.apply_exact(codes, tr, qr)
        _, by = AR.apply_bounds(codes, tr, qr)
        for name, kernel in KERNELS.items():
            out = torch.full((k * c,), 7.0, dtype=torch.float64, device=DEV)
            p1, _ = eng.gram_apply(d, d_t, d_q, n_variants=half, out=out, kernel=kernel)                                  # overwrites the 7s
            p2, _ = eng.gram_apply(d, d_t[half:].contiguous(), d_q, n_variants=v - half, out=out, accumulate=True, records_offset=half * r, kernel=kernel)
            eng.wait()
            assert np.array_equal(out.view(k, c).cpu().numpy(), wy.astype(np.float64)), f"{name}: two row blocks summed in place != one call over both"
            assert np.array_equal(torch.cat([p1, p2]).cpu().numpy(), wp.astype(np.float64)), name   # proj is overwritten per block, never accumulated
            eng.gram_apply(d, d_t, d_q, n_variants=0, out=out, accumulate=True, kernel=kernel)                            # a no-op
            eng.wait()
            assert np.array_equal(out.view(k, c).cpu().numpy(), wy.astype(np.float64)), name
            eng.gram_apply(d, d_t, d_q, n_variants=0, out=out, kernel=kernel)                                             # overwrite with nothing
            eng.wait()
            assert not out.any(), name
            _, y1 = run_apply(eng, tr[:half], qr, records=d, n_variants=half, kernel=kernel)
            _, y = run_apply(eng, tr[half:], qr, records=d, n_variants=v - half, records_offset=half * r, kernel=kernel, accumulate_onto=y1)
            within(y, ey, by, f"accumulate {name} Y in two halves")


def test_overlapping_launches_on_three_streams():
    n, v, c = 300, 2000, 8
    kept = list(range(0, n, 3))
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        d, codes = synth_codes(eng, 3 * v, n, 0, kept)
        r, k = eng.record_size, eng.kept_count
        t, q = int_tables(3 * v, 6), int_q(k, c, 6)
        d_ts = [dev(t[i * v:(i + 1) * v]) for i in range(3)]
        d_q = dev(q)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = [torch.full((k * c,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        projs = [torch.full((v * c,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        kernels = [_capi.GAPPLY_MFMA, _capi.GAPPLY_GENERAL, _capi.GAPPLY_AUTO]
        for i, s in enumerate(streams):
            eng.use_stream(s)
            eng.gram_apply(d, d_ts[i], d_q, n_variants=v, records_offset=i * v * r, proj=projs[i], out=outs[i], kernel=kernels[i])
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            wp, wy = AR.apply_int(codes[i * v:(i + 1) * v], t[i * v:(i + 1) * v], q)
            assert np.array_equal(outs[i].view(k, c).cpu().numpy(), wy.astype(np.float64)), f"stream {i}"
            assert np.array_equal(projs[i].view(v, c).cpu().numpy(), wp.astype(np.float64)), f"stream {i}"


@pytest.mark.parametrize("kernel", ["general", "mfma"])
def test_hip_graph_replayed_twice(kernel):
    """A capture on one stream of an overwriting call (zeroing + two kernels) and of an ACCUMULATE call, replayed twice onto new
    records, tables and Q: the overwrite gives Y once, the accumulate adds it twice."""
    n, v, c = 130, 257, 4
    rng = np.random.default_rng(5)
    r = GR.rsize(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_GAPPLY_ROW_SLICES, 3)      # memsets are part of the capture
        eng.tune(_capi.KNOB_GAPPLY_SAMPLE_SLICES, 2)
        d_recs = torch.zeros(v * r, dtype=torch.uint8, device=DEV)
        d_t = torch.zeros((v, 4), dtype=torch.float64, device=DEV)
        d_q = torch.zeros((n, c), dtype=torch.float64, device=DEV)
        proj = torch.zeros(v * c, dtype=torch.float64, device=DEV)
        proj2 = torch.zeros(v * c, dtype=torch.float64, device=DEV)
        out = torch.zeros(n * c, dtype=torch.float64, device=DEV)
        acc = torch.zeros(n * c, dtype=torch.float64, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.gram_apply(d_recs, d_t, d_q, proj=proj, out=out, kernel=KERNELS[kernel])   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.gram_apply(d_recs, d_t, d_q, proj=proj, out=out, kernel=KERNELS[kernel])
            eng.gram_apply(d_recs, d_t, d_q, proj=proj2, out=acc, accumulate=True, kernel=KERNELS[kernel])
        recs = rng.integers(0, 256, size=v * r, dtype=np.uint8)
        t, q = int_tables(v, 12), int_q(n, c, 12)
        d_recs.copy_(torch.from_numpy(recs))
        d_t.copy_(torch.from_numpy(t))
        d_q.copy_(torch.from_numpy(q))
        out.fill_(9.0)
        proj.fill_(9.0)
        acc.zero_()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        wp, wy = AR.apply_int(GR.unpack(recs.reshape(v, r), n), t, q)
        assert np.array_equal(out.view(n, c).cpu().numpy(), wy.astype(np.float64))
        assert np.array_equal(acc.view(n, c).cpu().numpy(), 2.0 * wy)
        assert np.array_equal(proj.view(v, c).cpu().numpy(), wp.astype(np.float64)) and torch.equal(proj, proj2)
        eng.use_torch_stream()


def test_bad_arguments():
    lib = _capi.lib
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        tabs = torch.ones(4 * 4 + 1, dtype=torch.float64, device=DEV)
        qb = torch.ones(300 * 4 + 1, dtype=torch.float64, device=DEV)
        pbuf = torch.full((4 * 4 + 8,), SENT, dtype=torch.float64, device=DEV)
        obuf = torch.full((300 * 4 + 8,), SENT, dtype=torch.float64, device=DEV)
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctx, rp, tp, qp, pp, op, fp = eng._ctx, recs.data_ptr(), tabs.data_ptr(), qb.data_ptr(), pbuf.data_ptr(), obuf.data_ptr(), offs.data_ptr()
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE
        call, call_at = lib.pgenhip_gram_apply, lib.pgenhip_gram_apply_at
        assert call(None, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 4, 0) == bad                    # NULL ctx
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 0, pp, op, 4, 0) == bad                     # no column
        assert call(ctx, rp, 75, None, 4, tp, qp, 17, 17, pp, op, 17, 0) == bad                  # 17 columns
        assert call(ctx, rp, 75, None, 4, tp, qp, 3, 4, pp, op, 4, 0) == bad                     # q_stride < n_columns
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 3, 0) == bad                     # out_stride < n_columns
        assert call(ctx, rp, 75, None, 4, None, qp, 4, 4, pp, op, 4, 0) == bad                   # NULL tables
        assert call(ctx, rp, 75, None, 4, tp + 4, qp, 4, 4, pp, op, 4, 0) == bad                 # tables not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, None, 4, 4, pp, op, 4, 0) == bad                   # NULL q
        assert call(ctx, rp, 75, None, 4, tp, qp + 4, 4, 4, pp, op, 4, 0) == bad                 # q not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, None, op, 4, 0) == bad                   # NULL proj
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp + 4, op, 4, 0) == bad                 # proj not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, None, 4, 0) == bad                   # NULL out
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op + 4, 4, 0) == bad                 # out not 8-byte aligned
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 4, 0x20) == bad                  # unknown flag bit
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 4, 3) == bad                     # unknown shape id
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 4, 0xF | _capi.GAPPLY_ACCUMULATE) == bad
        assert call(ctx, None, 75, None, 4, tp, qp, 4, 4, pp, op, 4, 0) == bad                   # NULL records
        assert call(ctx, rp, 74, None, 4, tp, qp, 4, 4, pp, op, 4, 0) == bad                     # stride < R
        assert call_at(None, rp, fp, 4, tp, qp, 4, 4, pp, op, 4, 0) == bad
        assert call_at(ctx, rp, None, 4, tp, qp, 4, 4, pp, op, 4, 0) == bad                      # NULL offsets
        assert call_at(ctx, rp, fp, 4, tp, qp, 4, 4, pp, op + 4, 4, 0) == bad
        assert call_at(ctx, rp, fp, 4, tp, qp, 4, 17, pp, op, 4, 0) == bad
        assert call(ctx, rp, 1 << 51, None, 2, tp, qp, 4, 4, pp, op, 4, 0) == big                # record_stride * n_variants >= 2^52
        assert call(ctx, rp, 1 << 52, fp, 2, tp, qp, 4, 4, pp, op, 4, 0) == big                  # with a variant list the stride alone
        assert call(ctx, rp, 75, None, 4, tp, qp, 1 << 41, 4, pp, op, 4, 0) == big               # K * q_stride * 8 >= 2^52
        assert call(ctx, rp, 75, None, 4, tp, qp, 4, 4, pp, op, 1 << 41, 0) == big               # K * out_stride * 8 >= 2^52
        eng.wait()
        assert (pbuf == SENT).all() and (obuf == SENT).all(), "a refused call wrote"
        # no rows: nothing is read, d_proj is not needed; without ACCUMULATE the K x C entries are zeroed, with it nothing happens
        assert call(ctx, None, 75, None, 0, None, None, 4, 4, None, None, 4, _capi.GAPPLY_ACCUMULATE) == _capi.OK
        eng.wait()
        assert (obuf == SENT).all()
        assert call(ctx, None, 75, None, 0, None, None, 4, 3, None, op + 8 * 4, 4, _capi.GAPPLY_MFMA) == _capi.OK
        eng.wait()
        got = obuf.cpu().numpy()[:4 + 300 * 4 + 4].copy()
        body = got[4:4 + 300 * 4].reshape(300, 4)
        assert not body[:, :3].any() and (body[:, 3] == SENT).all() and (got[:4] == SENT).all() and (got[-4:] == SENT).all()
        assert (pbuf == SENT).all()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0: zeros to d_proj, nothing to d_out, whatever its pointer
        pbuf.fill_(SENT)
        assert lib.pgenhip_gram_apply(eng._ctx, rp, 75, None, 4, None, None, 0, 2, pp + 8 * 4, None, 0, 0) == _capi.OK
        eng.wait()
        got = pbuf.cpu().numpy()
        assert (got[:4] == SENT).all() and not got[4:12].any() and (got[12:] == SENT).all()
        assert lib.pgenhip_gram_apply(eng._ctx, rp, 75, None, 4, None, None, 0, 2, None, None, 0, 0) == _capi.ERR_BAD_ARG
    with pgen_rs_amd.GtEngine(300, kept_idx=[299], device=0) as eng:   # K == 1: the strides are not used
        d, codes = synth_codes(eng, 9, 300, 0, [299])
        t, q = int_tables(9, 2), int_q(1, 3, 2)
        wp, wy = AR.apply_int(codes, t, q)
        d_t, d_q = dev(t), dev(q)
        for kernel in KERNELS.values():
            out = torch.zeros(3, dtype=torch.float64, device=DEV)
            proj = torch.zeros(27, dtype=torch.float64, device=DEV)
            assert lib.pgenhip_gram_apply(eng._ctx, d.data_ptr(), 75, None, 9, d_t.data_ptr(), d_q.data_ptr(), 0, 3, proj.data_ptr(), out.data_ptr(), 0, kernel) == _capi.OK
            eng.wait()
            assert np.array_equal(out.cpu().numpy(), wy[0].astype(np.float64)) and np.array_equal(proj.view(9, 3).cpu().numpy(), wp.astype(np.float64))
