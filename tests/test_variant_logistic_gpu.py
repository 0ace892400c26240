"""Per-variant logistic regression — GPU leg (pgenhip_variant_logistic / _at through GtEngine), against tests/logit_ref.py.

Compare leg: the cases, V, frequencies, missing rate, tol = 1e-10 and max_iter = 25 of logit_ref.COMPARE_CASES, both missing-call
policies, every shape.  A row is compared where the reference converges (at least 90 % of a case's rows must be): status bits equal,
evaluations within +-1 (the stop decision may flip at |delta| ~ tol), beta and SE against the reference run to tol = 1e-13.
Tolerance (logit_ref.tolerances, derived, printed by the fixture): twice the reference's own gap between its 1e-10-stopped and its
converged answers plus 100 x the disagreement of the two formulations (newton, irls_qr), because the kernel's summation order is its
own.  Measured on these cases (1 728 rows, all converged, at most 6 evaluations): beta gap 1.0e-10 (Newton's last step is below
tol), relative SE gap 3.0e-11, formulations 1.3e-15 absolute in beta and 7.0e-15 relative in SE, so 2.0e-10 and 6.0e-11 are allowed.

One-step leg, plumbing (shapes x forced grids x row sources x keep sets, dirty pad bits, group edges, sentinels, streams, a graph),
the status cases and every refusal follow."""
import numpy as np
import pytest
import torch

import logit_ref as LR
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1.2345e300
ISENT = 0x5A5A5A5A
SHAPES = [_capi.LOGIT_GENERAL, _capi.LOGIT_FAST, _capi.LOGIT_AUTO]
BITS = _capi.LOGIT_CONVERGED | _capi.LOGIT_NOT_CONVERGED | _capi.LOGIT_SINGULAR


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_logit(eng, v, nc, at=None, **kw):
    """The three outputs inside sentinels: the call writes its v x (nc + 1) coefficients, v errors and v words and nothing else"""
    lead = 3
    cbuf = torch.full((lead + v * (nc + 1) + 8,), SENT, dtype=torch.float64, device=DEV)
    sbuf = torch.full((lead + v + 8,), SENT, dtype=torch.float64, device=DEV)
    wbuf = torch.full((lead + v + 8,), ISENT, dtype=torch.int32, device=DEV)
    outs = dict(coef=cbuf[lead:], se=sbuf[lead:], status=wbuf[lead:])
    if at is not None:
        coef, se, status = eng.variant_logistic_at(at[0], at[1], **outs, **kw)
    else:
        coef, se, status = eng.variant_logistic(**outs, **kw)
    eng.wait()
    hc, hs, hw = cbuf.cpu().numpy(), sbuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (hc[:lead] == SENT).all() and (hc[lead + v * (nc + 1):] == SENT).all(), "wrote outside its coefficients"
    assert (hs[:lead] == SENT).all() and (hs[lead + v:] == SENT).all(), "wrote outside its errors"
    assert (hw[:lead] == ISENT).all() and (hw[lead + v:] == ISENT).all(), "wrote outside its status words"
    assert coef.shape == (v, nc + 1) and se.shape == (v,) and status.shape == (v,)
    return coef.cpu().numpy(), se.cpu().numpy(), status.cpu().numpy().astype(np.int64)


def well_formed(status, max_iter):
    it, bits = status & 0xFF, status & ~0xFF
    assert ((it >= 1) & (it <= max_iter)).all(), status
    assert np.isin(bits, [_capi.LOGIT_CONVERGED, _capi.LOGIT_NOT_CONVERGED, _capi.LOGIT_SINGULAR]).all(), status


def compare(got, ref_loose, ref_tight, tol_b, tol_se, what, need=0.0):
    """got against the reference on the rows where the reference converges; returns the worst errors"""
    coef, se, status = got
    ok = ((ref_loose[2] & LR.CONVERGED) != 0) & ((ref_tight[2] & LR.CONVERGED) != 0)
    assert ok.mean() >= need, f"{what}: the reference converges on {ok.mean():.0%} of the rows only"
    assert ((status[ok] & BITS) == (ref_loose[2][ok] & BITS)).all(), f"{what}: status {status[ok]} against {ref_loose[2][ok]}"
    assert (np.abs((status[ok] & 0xFF) - (ref_loose[2][ok] & 0xFF)) <= 1).all(), f"{what}: evaluations"
    eb = np.abs(coef[ok] - ref_tight[0][ok]).max() if ok.any() else 0.0
    es = (np.abs(se[ok] - ref_tight[1][ok]) / ref_tight[1][ok]).max() if ok.any() else 0.0
    assert eb <= tol_b and es <= tol_se, f"{what}: beta off by {eb:.3g} of {tol_b:.3g}, SE by {es:.3g} of {tol_se:.3g}"
    nconv = (status & _capi.LOGIT_CONVERGED) == 0
    assert np.isnan(se[nconv]).all(), f"{what}: a row that did not converge has an SE"
    return eb, es


@pytest.fixture(scope="module")
def refs():
    """Every compare-leg case with both policies, computed once, and the tolerances they give"""
    out = {}
    for i, (k, nc) in enumerate(LR.COMPARE_CASES):
        for impute in (True, False):
            out[(k, nc, impute)] = LR.reference(1000 + i, k, nc, impute)
    m = LR.measure(out.values())
    tol_b, tol_se = LR.tolerances(m)
    print(f"reference: beta gap {m['beta_gap']:.3g}, SE gap {m['se_gap']:.3g}, formulations {m['beta_form']:.3g} / {m['se_form']:.3g}, "
          f"at most {m['max_it']} evaluations on {m['rows']} rows; allowed: beta {tol_b:.3g}, SE {tol_se:.3g}")
    assert m["beta_gap"] <= 1e-10 and tol_b < 1e-9 and tol_se < 1e-9   # Newton's last step is below tol; the tolerance stays of that order
    return out, tol_b, tol_se


@pytest.mark.parametrize("impute", [True, False])
@pytest.mark.parametrize("k,nc", LR.COMPARE_CASES)
def test_compare_against_reference(refs, k, nc, impute):
    cases, tol_b, tol_se = refs
    r = cases[(k, nc, impute)]
    v = LR.COMPARE_V
    with pgen_rs_amd.GtEngine(k, device=0) as eng:
        recs = dev(LR.pack_codes(r["codes"]).reshape(-1))
        args = dict(records=recs, code_values=dev(r["table"]), design=dev(r["design"]), y=dev(r["y"]), start=dev(r["start"]),
                    max_iter=25, tol=1e-10, n_variants=v)
        for shape in SHAPES:
            got = run_logit(eng, v, nc, flags=shape, **args)
            well_formed(got[2], 25)
            eb, es = compare(got, r["loose"], r["tight"], tol_b, tol_se, f"K = {k}, n_cov = {nc}, impute {impute}, shape {shape}", need=0.9)
            print(f"K = {k}, n_cov = {nc}, impute {impute}, shape {shape}: beta off by {eb:.3g} of {tol_b:.3g}, SE by {es:.3g} of {tol_se:.3g}")


@pytest.mark.parametrize("k,nc", [(65, 4), (257, 15), (1000, 15), (2504, 8)])
def test_one_step(refs, k, nc):
    """max_iter = 1: no step, the start bit for bit, NOT_CONVERGED.  max_iter = 2, tol = 0: one Newton step, inside 100 x what the two
    formulations disagree by after one step."""
    cases, _, _ = refs
    r = cases[(k, nc, True)]
    v = LR.COMPARE_V
    one_n = LR.fit_rows(LR.newton, r["codes"], r["table"], r["design"], r["y"], r["start"], 2, 0.0)
    one_q = LR.fit_rows(LR.irls_qr, r["codes"], r["table"], r["design"], r["y"], r["start"], 2, 0.0)
    assert (one_n[2] == (LR.NOT_CONVERGED | 2)).all() and (one_q[2] == (LR.NOT_CONVERGED | 2)).all()
    allowed = 100.0 * np.abs(one_n[0] - one_q[0]).max()
    assert 0 < allowed < 1e-9
    with pgen_rs_amd.GtEngine(k, device=0) as eng:
        args = dict(records=dev(LR.pack_codes(r["codes"]).reshape(-1)), code_values=dev(r["table"]), design=dev(r["design"]), y=dev(r["y"]),
                    start=dev(r["start"]), n_variants=v)
        for shape in SHAPES:
            coef, se, status = run_logit(eng, v, nc, flags=shape, max_iter=1, tol=1e-10, **args)
            want = np.tile(np.concatenate([r["start"], [0.0]]), (v, 1))
            assert coef.tobytes() == want.tobytes() and np.isnan(se).all() and (status == (_capi.LOGIT_NOT_CONVERGED | 1)).all()
            coef, se, status = run_logit(eng, v, nc, flags=shape, max_iter=2, tol=0.0, **args)
            err = np.abs(coef - one_n[0]).max()
            print(f"K = {k}, n_cov = {nc}, shape {shape}: one step off by {err:.3g} of {allowed:.3g}")
            assert (status == (_capi.LOGIT_NOT_CONVERGED | 2)).all() and np.isnan(se).all() and err <= allowed


def keep_sets(n):
    return {"all": None, "identity": list(range(n)), "no first": list(range(1, n)), "no last": list(range(n - 1)), "every 7th": list(range(0, n, 7))}


def plumbing_case(seed, n, nc, v, kept):
    """Records of n samples with dirty pad bits, and the reference over the kept samples (mean imputation)"""
    codes, _, _ = LR.make_case(seed, n, nc, v=v)
    sel = np.arange(n) if kept is None else np.asarray(kept, dtype=np.int64)
    _, design, y = LR.make_case(seed + 1, len(sel), nc, v=1)
    recs = LR.pack_codes(codes)
    if n % 4:
        recs[:, -1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)   # pad bits set: they are no samples
    kc = codes[:, sel]
    table = LR.tables(kc, True)
    start = LR.null_fit(design, y)
    loose = LR.fit_rows(LR.newton, kc, table, design, y, start, 25, 1e-10)
    tight = LR.fit_rows(LR.newton, kc, table, design, y, start, 25, 1e-13)
    return recs, table, design, y, start, loose, tight


@pytest.mark.parametrize("keep", ["all", "identity", "no first", "no last", "every 7th"])
@pytest.mark.parametrize("nc", [4, 15])
def test_row_sources_keep_sets_shapes_and_grids(refs, keep, nc):
    _, tol_b, tol_se = refs
    n, v = (259, 21) if nc == 4 else (1403, 11)
    kept = keep_sets(n)[keep]
    recs, table, design, y, start, loose, tight = plumbing_case(50 + nc, n, nc, v, kept)
    r = LR.rsize(n)
    stride = r + 5
    raw = np.full(3 + v * stride, 0xA5, dtype=np.uint8)
    for i in range(v):
        raw[3 + i * stride: 3 + i * stride + r] = recs[i]
    gather = np.array(list(range(v - 1, -1, -2)) + [2, 2, 0], dtype=np.int32)   # descending, with a repeat
    d_raw, d_gather = dev(raw), dev(gather)
    d_offs = dev(np.array([3 + int(i) * stride for i in gather], dtype=np.int64))
    dense = dev(np.concatenate([np.zeros(1, np.uint8), recs.reshape(-1)]))
    wide = torch.zeros((design.shape[0], nc + 3), dtype=torch.float64, device=DEV)
    wide[:, 2:2 + nc] = dev(design)
    sub = lambda ref, idx: tuple(a[idx] for a in ref)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        base = dict(y=dev(y), start=dev(start), max_iter=25, tol=1e-10)
        for blocks in (1, 2, 3, 0):
            eng.tune(_capi.KNOB_LOGIT_BLOCKS, blocks)
            for shape in SHAPES:
                what = f"keep {keep}, n_cov {nc}, blocks {blocks}, shape {shape}"
                x = wide[:, 2:2 + nc] if blocks == 2 else dev(design)   # a design with a row stride above n_cov
                got = run_logit(eng, v, nc, records=d_raw, record_stride=stride, records_offset=3, n_variants=v, code_values=dev(table), design=x, flags=shape, **base)
                compare(got, loose, tight, tol_b, tol_se, "padded stride, " + what)
                got = run_logit(eng, len(gather), nc, records=d_raw, record_stride=stride, records_offset=3, variant_idx=d_gather,
                                code_values=dev(table[gather]), design=x, flags=shape, **base)
                compare(got, sub(loose, gather), sub(tight, gather), tol_b, tol_se, "gathered, " + what)
                got = run_logit(eng, len(gather), nc, at=(d_raw, d_offs), code_values=dev(table[gather]), design=x, flags=shape, **base)
                compare(got, sub(loose, gather), sub(tight, gather), tol_b, tol_se, "_at, " + what)
                got = run_logit(eng, v, nc, records=dense, records_offset=1, n_variants=v, code_values=dev(table), design=x, flags=shape, **base)
                compare(got, loose, tight, tol_b, tol_se, "dense from an odd base, " + what)


@pytest.mark.parametrize("nc", [1, 3, 4, 7, 8, 11, 12, 15])
@pytest.mark.parametrize("blocks", [1, 2])
def test_row_counts_on_both_sides_of_every_group_and_bucket_edge(refs, nc, blocks):
    """n_cov on both sides of every bucket of the FAST kernel (p = 4, 8, 12, 16), row counts around its groups of 4 and 2 rows"""
    _, tol_b, tol_se = refs
    n, vmax = 300, 9
    recs, table, design, y, start, loose, tight = plumbing_case(70 + nc, n, nc, vmax, None)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        eng.tune(_capi.KNOB_LOGIT_BLOCKS, blocks)
        args = dict(records=dev(recs.reshape(-1)), code_values=dev(table), design=dev(design), y=dev(y), start=dev(start), max_iter=25, tol=1e-10)
        for v in (1, 2, 3, 4, 5, 7, 8, 9):
            for shape in SHAPES:
                got = run_logit(eng, v, nc, n_variants=v, flags=shape, **args)
                compare(got, tuple(a[:v] for a in loose), tuple(a[:v] for a in tight), tol_b, tol_se, f"n_cov {nc}, V {v}, blocks {blocks}, shape {shape}")


@pytest.mark.parametrize("k", [1, 3, 4])
def test_tiny_sample_counts_end_without_convergence(k):
    """K below p = 5: H has rank K at most, so no row converges; which of the other two it ends as depends on rounding"""
    nc, v = 4, 13
    codes, design, y = LR.make_case(5 + k, k, nc, v=v)
    with pgen_rs_amd.GtEngine(k, device=0) as eng:
        for shape in SHAPES:
            coef, se, status = run_logit(eng, v, nc, records=dev(LR.pack_codes(codes).reshape(-1)), n_variants=v, code_values=dev(LR.tables(codes, True)),
                                         design=dev(design), y=dev(y), start=dev(np.zeros(nc)), max_iter=25, tol=1e-10, flags=shape)
            well_formed(status, 25)
            assert ((status & _capi.LOGIT_CONVERGED) == 0).all() and np.isnan(se).all()


def test_status_cases(refs):
    _, tol_b, tol_se = refs
    n, nc = 200, 3
    codes, design, y = LR.make_case(17, n, nc, v=6)
    codes[0] = 0                                       # all 0/0: the genotype column is zero
    codes[2] = np.where(y > 0.5, 2, 0)                 # perfectly separated: cases 1/1, controls 0/0
    codes[3] = 3                                       # all missing, dropped: no included sample
    table = LR.tables(codes, True)
    table[1] = np.nan                                  # an all-NaN table
    table[3, 3] = np.nan
    start = LR.null_fit(design, y)
    ref = LR.fit_rows(LR.newton, codes, table, design, y, start, 25, 1e-10)
    tight = LR.fit_rows(LR.newton, codes, table, design, y, start, 25, 1e-13)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for shape in SHAPES:
            coef, se, status = run_logit(eng, 6, nc, records=dev(LR.pack_codes(codes).reshape(-1)), n_variants=6, code_values=dev(table),
                                         design=dev(design), y=dev(y), start=dev(start), max_iter=25, tol=1e-10, flags=shape)
            well_formed(status, 25)
            assert status[0] & _capi.LOGIT_SINGULAR and status[1] == (_capi.LOGIT_SINGULAR | 1) and status[3] == (_capi.LOGIT_SINGULAR | 1)
            assert not status[2] & _capi.LOGIT_CONVERGED
            assert np.isnan(se[:4]).all()
            want0 = np.concatenate([start, [0.0]])
            assert coef[1].tobytes() == want0.tobytes() and coef[3].tobytes() == want0.tobytes()   # SINGULAR keeps the last beta
            for j in (4, 5):
                assert status[j] & _capi.LOGIT_CONVERGED and (status[j] & BITS) == (ref[2][j] & BITS)
                assert np.abs(coef[j] - tight[0][j]).max() <= tol_b and abs(se[j] - tight[1][j]) <= tol_se * tight[1][j]


def test_overflowing_exponent_gives_no_nan():
    """A start that sends e^-eta to inf: mu = 0, weights 0, H singular at once, and no NaN in the coefficients"""
    n, nc = 130, 2
    codes, design, y = LR.make_case(23, n, nc, v=3)
    start = np.array([-800.0, 0.0])
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        for shape in SHAPES:
            coef, se, status = run_logit(eng, 3, nc, records=dev(LR.pack_codes(codes).reshape(-1)), n_variants=3, code_values=dev(LR.tables(codes, True)),
                                         design=dev(design), y=dev(y), start=dev(start), max_iter=25, tol=1e-10, flags=shape)
            assert (status == (_capi.LOGIT_SINGULAR | 1)).all() and not np.isnan(coef).any()


def test_overlapping_launches_on_three_streams(refs):
    _, tol_b, tol_se = refs
    n, nc, v = 500, 5, 3 * 40
    recs, table, design, y, start, loose, tight = plumbing_case(90, n, nc, v, None)
    r = LR.rsize(n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d, d_x, d_y, d_s = dev(recs.reshape(-1)), dev(design), dev(y), dev(start)
        tabs = [dev(table[i * 40:(i + 1) * 40]) for i in range(3)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
        outs = []
        for i, s in enumerate(streams):
            eng.use_stream(s)
            outs.append(eng.variant_logistic(d, tabs[i], d_x, d_y, d_s, max_iter=25, tol=1e-10, records_offset=i * 40 * r, n_variants=40))
        torch.cuda.synchronize()
        eng.use_torch_stream()
        for i in range(3):
            got = (outs[i][0].cpu().numpy(), outs[i][1].cpu().numpy(), outs[i][2].cpu().numpy().astype(np.int64))
            sl = slice(i * 40, (i + 1) * 40)
            compare(got, tuple(a[sl] for a in loose), tuple(a[sl] for a in tight), tol_b, tol_se, f"stream {i}")


def test_hip_graph_replayed_twice(refs):
    """One kernel captured on one stream and replayed twice over dirty outputs: the fit of the records the buffer holds at replay"""
    _, tol_b, tol_se = refs
    n, nc, v = 300, 4, 37
    recs, table, design, y, start, loose, tight = plumbing_case(95, n, nc, v, None)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        d_recs = torch.zeros(v * LR.rsize(n), dtype=torch.uint8, device=DEV)
        d_t, d_x, d_y, d_s = dev(table), dev(design), dev(y), dev(start)
        coef = torch.zeros(v * (nc + 1), dtype=torch.float64, device=DEV)
        se = torch.zeros(v, dtype=torch.float64, device=DEV)
        status = torch.zeros(v, dtype=torch.int32, device=DEV)
        kw = dict(max_iter=25, tol=1e-10, coef=coef, se=se, status=status)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            eng.variant_logistic(d_recs, d_t, d_x, d_y, d_s, **kw)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.use_torch_stream()
            eng.variant_logistic(d_recs, d_t, d_x, d_y, d_s, **kw)
        d_recs.copy_(dev(recs.reshape(-1)))
        coef.fill_(SENT)
        se.fill_(SENT)
        status.fill_(ISENT)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        got = (coef.view(v, nc + 1).cpu().numpy(), se.cpu().numpy(), status.cpu().numpy().astype(np.int64))
        compare(got, loose, tight, tol_b, tol_se, "graph")
        eng.use_torch_stream()


def test_bad_arguments():
    lib = _capi.lib
    nan = float("nan")
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        recs = torch.zeros(75 * 4, dtype=torch.uint8, device=DEV)
        dbl = torch.ones(300 * 16 + 64, dtype=torch.float64, device=DEV)
        cbuf = torch.full((4 * 16 + 8,), SENT, dtype=torch.float64, device=DEV)
        sbuf = torch.full((4 + 8,), SENT, dtype=torch.float64, device=DEV)
        wbuf = torch.full((4 + 8,), ISENT, dtype=torch.int32, device=DEV)
        offs = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctx, rp, dp, cp, sp, wp, op = eng._ctx, recs.data_ptr(), dbl.data_ptr(), cbuf.data_ptr(), sbuf.data_ptr(), wbuf.data_ptr(), offs.data_ptr()
        bad, big = _capi.ERR_BAD_ARG, _capi.ERR_TOO_LARGE

        def call(ctx=ctx, rp=rp, stride=75, idx=None, v=4, tab=dp, x=dp, xs=15, nc=15, y=dp, start=dp, it=25, tol=1e-9, c=cp, cs=16, se=sp, w=wp, flags=0):
            return lib.pgenhip_variant_logistic(ctx, rp, stride, idx, v, tab, x, xs, nc, y, start, it, tol, c, cs, se, w, flags)

        def call_at(ctx=ctx, off=op, v=4, tab=dp, x=dp, xs=15, nc=15, c=cp, cs=16, flags=0):
            return lib.pgenhip_variant_logistic_at(ctx, rp, off, v, tab, dp, xs, nc, dp, dp, 25, 1e-9, c, cs, sp, wp, flags)

        assert call(ctx=None) == bad and call_at(ctx=None) == bad
        assert call(nc=0) == bad and call(nc=16, xs=16, cs=17) == bad
        assert call(it=0) == bad and call(it=65) == bad
        assert call(tol=nan) == bad and call(tol=-1e-9) == bad
        assert call(xs=14) == bad and call(cs=15) == bad
        for name in ("tab", "x", "y", "start", "c", "se", "w", "rp"):
            assert call(**{name: None}) == bad, name
        for name, p in (("tab", dp), ("x", dp), ("y", dp), ("start", dp), ("c", cp), ("se", sp)):
            assert call(**{name: p + 4}) == bad, name
        assert call(w=wp + 2) == bad
        assert call(flags=0x10) == bad and call(flags=3) == bad
        assert call(stride=74) == bad
        assert call_at(off=None) == bad and call_at(c=cp + 4) == bad
        assert call(xs=1 << 50) == big and call(cs=1 << 50) == big
        assert call(stride=1 << 51) == big and call(stride=1 << 52, idx=op) == big
        assert call_at(xs=1 << 50) == big
        assert call(v=0) == _capi.OK
        eng.wait()
        assert (cbuf.cpu().numpy() == SENT).all() and (sbuf.cpu().numpy() == SENT).all() and (wbuf.cpu().numpy() == ISENT).all(), "a refused call wrote"
        assert call(stride=0, v=1, cs=0) == _capi.OK   # a single row needs no strides
        eng.wait()
    with pgen_rs_amd.GtEngine(300, kept_idx=[], device=0) as eng:   # K == 0: SINGULAR for every row, design and y not read
        for shape in SHAPES:
            cbuf.fill_(SENT)
            sbuf.fill_(SENT)
            wbuf.fill_(ISENT)
            assert lib.pgenhip_variant_logistic(eng._ctx, rp, 75, None, 4, dp, None, 0, 3, None, dp, 25, 1e-9, cp, 4, sp, wp, shape) == _capi.OK
            eng.wait()
            assert (wbuf.cpu().numpy()[:4] == (_capi.LOGIT_SINGULAR | 1)).all() and (wbuf.cpu().numpy()[4:] == ISENT).all()
            assert np.isnan(sbuf.cpu().numpy()[:4]).all() and (sbuf.cpu().numpy()[4:] == SENT).all()
            h = cbuf.cpu().numpy()
            assert (h[:16].reshape(4, 4) == np.array([1.0, 1.0, 1.0, 0.0])).all() and (h[16:] == SENT).all()
