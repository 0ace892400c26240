"""Every GtEngine method that exists twice, by stride / ``variant_idx`` and as an ``_at`` twin by byte offset: the two fronts of a pair
do the same thing.

Shapes: N = 70 (R = 18, the last byte half-filled), V = 9 rows from ``synth_records`` with dirty pad bits, two keep sets (all samples,
every third).  The rows are read in shuffled order: the ``_at`` call gets the offsets ``ORDER[j] * R``, the plain call the same order
through ``variant_idx``.

Agreement: both twins write into sentinel-framed buffers of the caller and their results are equal bit for bit.  The FP64 entries get
integer-valued weights, values and tables, so their sums are exact whatever the order of the additions.  ``variant_logistic``: equal
status words, and both twins' coefficients and errors against tests/logit_ref.py under ``logit_ref.tolerances(logit_ref.measure(.))``
of this file's own two cases (the formula of tests/test_variant_logistic_gpu.py, imported).  ``pack_records`` gets the framed buffer
from its first byte and ``out_offset = LEAD``: its result view counts ``out_offset`` from the start of ``out``'s storage, so an ``out``
that is itself an offset view comes back misplaced (the records are written where they belong); that is as it was, and not this
file's subject.

Refusals: one wrong argument at a time raises ``ValueError`` on both twins where the argument exists, and afterwards no buffer has
changed: nothing was launched.  Two cells of that table do not exist in the library and are left out, not asserted: ``decode_emit``
checks its ``out`` for size only, never for dtype, and a ``records`` tensor is checked for size only where rows are read by stride
(``variant_idx`` and ``record_off`` may point anywhere), so "one byte short" is a plain call without ``variant_idx``.

Defaults: with ``out=None`` both twins return the same shape, dtype, strides and storage offset, also for ``n_variants = 0`` and for a
context that keeps no sample.  One pair differs there and the difference is pinned as it is: ``decode_emit`` with ``n_variants = 0``
allocates nothing, ``decode_emit_at`` one row."""
import numpy as np
import pytest
import torch

import logit_ref as LR
import pgen_rs_amd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, V = 70, 9
R = (N + 3) // 4
KEEPS = {"all": None, "every third": list(range(0, N, 3)), "none": []}
ORDER = [4, 0, 7, 2, 8, 5, 1, 6, 3]
W, C, NC = 3, 3, 3            # window, columns of the FP64 families, covariates
LEAD, TAIL = 4, 8             # frame entries: 4 keep an int32 output 16-byte aligned
FROM_OUT_OFFSET = "the output begins at the buffer's first byte and the call gets out_offset = LEAD"
SENT = {torch.uint8: 0xA5, torch.int8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A, torch.float32: -1.25e30,
        torch.float64: -1.2345e300}
PAIRS = ["decode_emit", "genotype_counts", "sample_counts", "sample_scores", "variant_sums", "variant_logistic", "decode_matrix",
         "pack_records", "pair_tables", "pair_r2", "pair_mask", "sample_pair_tables", "sample_gram", "gram_apply"]
u8, i8, i32, f32, f64 = torch.uint8, torch.int8, torch.int32, torch.float32, torch.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """One context with its records and every family's inputs, for one keep set"""

    def __init__(self, keep):
        self.keep = keep
        self.eng = eng = pgen_rs_amd.GtEngine(N, kept_idx=KEEPS[keep], device=0)
        self.k = k = eng.kept_count
        self.recs = eng.synth_records(V, first_variant=3, dirty_pad=True)
        assert self.recs.numel() == V * R
        self.vidx = dev(np.array(ORDER, dtype=np.int32))
        self.offs = dev(np.array(ORDER, dtype=np.int64) * R)
        rng = np.random.default_rng(2024)
        self.weights = dev(rng.integers(-8, 9, size=(V, C)).astype(np.float32))
        self.miss = dev(rng.integers(0, 3, size=V).astype(np.float32))
        self.values = dev(rng.integers(-4, 5, size=(k, C)).astype(np.float64))
        self.tables = dev(rng.integers(-8, 9, size=(V, 4)).astype(np.float64))
        self.q = dev(rng.integers(-4, 5, size=(k, C)).astype(np.float64))
        self.key = dev(2 * np.arange(V, dtype=np.int64))
        self.ref = None
        if k:
            sel = np.arange(N) if KEEPS[keep] is None else np.array(KEEPS[keep])
            eng.wait()
            codes = LR.unpack_codes(self.recs.cpu().numpy().reshape(V, R), N)[ORDER][:, sel]   # the selection's rows, the kept samples
            _, design, y = LR.make_case(77, k, NC, v=1)
            table, start = LR.tables(codes, True), LR.null_fit(design, y)
            self.ref = {name: LR.fit_rows(fit, codes, table, design, y, start, 25, tol)
                        for name, fit, tol in (("loose", LR.newton, 1e-10), ("tight", LR.newton, 1e-13), ("qr", LR.irls_qr, 1e-13))}
        else:
            design, y, table, start = np.zeros((0, NC)), np.zeros(0), np.zeros((V, 4)), np.zeros(NC)
        self.logit = dict(code_values=dev(table), design=dev(design), y=dev(y), start=dev(start), max_iter=25, tol=1e-10)

    def rows(self, at, n=V):
        if at:
            return dict(base=self.recs, record_off=self.offs, n_variants=n)
        return dict(records=self.recs, variant_idx=self.vidx, n_variants=n)

    def spec(self, name, n=V):
        """(the family's own arguments, {output argument: (dtype, entries, shape or None)}, the inputs whose rows and dtype are checked)"""
        k, eng = self.k, self.eng
        a, b = ((1, 6), (0, 5)) if k else ((0, 0), (0, 0))
        return {
            "decode_emit": ({}, {"out": (u8, n * eng.gt_row_bytes, None)}, []),
            "genotype_counts": ({}, {"out": (i32, 4 * n, None)}, []),
            "sample_counts": ({}, {"out": (i32, 4 * k, None)}, []),
            "sample_scores": (dict(weights=self.weights, miss=self.miss), {"out": (f64, k * C, None)}, ["weights"]),
            "variant_sums": (dict(values=self.values), {"out": (f64, n * C * 4, None)}, ["values"]),
            "variant_logistic": (self.logit, {"coef": (f64, n * (NC + 1), None), "se": (f64, n, None), "status": (i32, n, None)},
                                 ["code_values", "design"]),
            "decode_matrix": ({}, {"out": (i8, n * k, (n, k))}, []),
            "pack_records": (dict(out_offset=LEAD), {"out": (u8, n * eng.packed_record_size, FROM_OUT_OFFSET)}, []),
            "pair_tables": (dict(window=W), {"out": (i32, 16 * n * W, None)}, []),
            "pair_r2": (dict(window=W), {"out": (f32, n * W, None)}, []),
            "pair_mask": (dict(window=W, min_r2=0.01, key=self.key, max_span=4), {"fwd": (i32, n, None), "bwd": (i32, n, None)}, ["key"]),
            "sample_pair_tables": (dict(a=a, b=b), {"out": (i32, 16 * a[1] * b[1], None)}, []),
            "sample_gram": (dict(code_values=self.tables, a=a, b=b), {"out": (f64, a[1] * b[1], None)}, ["code_values"]),
            "gram_apply": (dict(code_values=self.tables, q=self.q), {"proj": (f64, n * C, None), "out": (f64, k * C, None)},
                           ["code_values", "q"]),
        }[name]

    def call(self, name, at, rows=None, **kw):
        res = getattr(self.eng, name + ("_at" if at else ""))(**(self.rows(at) if rows is None else rows), **kw)
        return res if isinstance(res, tuple) else (res,)


@pytest.fixture(scope="module")
def cases():
    """One Case per keep set, shared by every test of the module"""
    out = {keep: Case(keep) for keep in KEEPS}
    yield out
    for c in out.values():
        c.eng.close()


@pytest.fixture(params=["all", "every third"])
def case(cases, request):
    return cases[request.param]


@pytest.fixture(params=list(KEEPS))
def any_case(cases, request):
    return cases[request.param]


@pytest.fixture(scope="module")
def logit_tol(cases):
    """The bound of tests/test_variant_logistic_gpu.py over this file's own two cases"""
    m = LR.measure([c.ref for c in cases.values() if c.k])
    tol_b, tol_se = LR.tolerances(m)
    print(f"reference: beta gap {m['beta_gap']:.3g}, SE gap {m['se_gap']:.3g}, formulations {m['beta_form']:.3g} / {m['se_form']:.3g} "
          f"on {m['rows']} rows; allowed: beta {tol_b:.3g}, SE {tol_se:.3g}")
    assert m["rows"] >= V and 0 < tol_b < 1e-9 and 0 < tol_se < 1e-9
    return tol_b, tol_se


class Framed:
    """A caller's output between sentinels; mask outputs start as zeros because the call only ORs bits in"""

    def __init__(self, name, dtype, need, shape):
        self.need = need
        self.buf = torch.full((LEAD + need + TAIL,), SENT[dtype], dtype=dtype, device=DEV)
        if name in ("fwd", "bwd"):
            self.buf[LEAD:LEAD + need] = 0
        self.before = self.buf.clone()
        self.first = self.buf.data_ptr() + LEAD * self.buf.element_size()     # where the result begins
        if shape == FROM_OUT_OFFSET:
            self.out = self.buf[:LEAD + need]
        else:
            self.out = self.buf[LEAD:LEAD + need]
            if shape is not None:
                self.out = self.out.view(shape)

    def frame_intact(self):
        return torch.equal(self.buf[:LEAD], self.before[:LEAD]) and torch.equal(self.buf[LEAD + self.need:], self.before[LEAD + self.need:])

    def untouched(self):
        return torch.equal(self.buf, self.before)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(-1).view(u8), y.contiguous().view(-1).view(u8))


@pytest.mark.parametrize("name", PAIRS)
def test_twins_agree(case, logit_tol, name):
    kw, outs, _ = case.spec(name)
    got = []
    for at in (False, True):
        framed = {arg: Framed(arg, *o) for arg, o in outs.items()}
        res = case.call(name, at, **kw, **{arg: f.out for arg, f in framed.items()})
        case.eng.wait()
        for arg, f in framed.items():
            assert f.frame_intact(), f"{name}{'_at' if at else ''} wrote outside its {arg}"
            assert not f.untouched(), f"{name}{'_at' if at else ''} left its {arg} as it was"
        assert len(res) == len(framed)
        for t, f in zip(res, framed.values()):
            assert t.data_ptr() == f.first and t.numel() == f.need, "the result is not the caller's output"
        got.append(res)
    if name != "variant_logistic":
        for p, q in zip(*got):
            assert same_bits(p, q), f"{name}: the twins differ"
        return
    tol_b, tol_se = logit_tol
    assert torch.equal(got[0][2], got[1][2]), "variant_logistic: the twins' status words differ"
    loose, tight = case.ref["loose"], case.ref["tight"]
    ok = ((loose[2] & LR.CONVERGED) != 0) & ((tight[2] & LR.CONVERGED) != 0)
    assert ok.sum() >= V - 1, f"the reference converges on {ok.sum()} of {V} rows only"
    for twin, (coef, se, status) in zip(("variant_logistic", "variant_logistic_at"), got):
        coef, se, status = coef.cpu().numpy(), se.cpu().numpy(), status.cpu().numpy().astype(np.int64)
        assert coef.shape == (V, NC + 1) and ((status[ok] & ~0xFF) == (loose[2][ok] & ~0xFF)).all()
        eb = np.abs(coef[ok] - tight[0][ok]).max()
        es = (np.abs(se[ok] - tight[1][ok]) / tight[1][ok]).max()
        print(f"{twin}, keep {case.keep}: beta off by {eb:.3g} of {tol_b:.3g}, SE by {es:.3g} of {tol_se:.3g}")
        assert eb <= tol_b and es <= tol_se, f"{twin}: beta off by {eb:.3g} of {tol_b:.3g}, SE by {es:.3g} of {tol_se:.3g}"


def other_dtype(t):
    return {f64: f32, f32: f64, torch.int64: i32, i32: torch.int64}.get(t, f64)


def row_faults(case, at):
    src, idx = ("base", "record_off") if at else ("records", "variant_idx")
    good = case.rows(at)
    yield "a CPU " + src, {**good, src: good[src].cpu()}
    yield "a non-contiguous " + src, {**good, src: torch.zeros(2 * V * R, dtype=u8, device=DEV)[::2]}
    yield idx + " of the other width", {**good, idx: good[idx].to(other_dtype(good[idx].dtype))}
    yield idx + " one entry short", {**good, idx: good[idx][:V - 1]}
    if not at:
        yield "records one byte short", dict(records=case.recs[:V * R - 1], n_variants=V)


@pytest.mark.parametrize("name", PAIRS)
def test_single_fault_refusals(case, name):
    kw, outs, inputs = case.spec(name)
    framed = {arg: Framed(arg, *o) for arg, o in outs.items()}
    good = {arg: f.out for arg, f in framed.items()}
    watched = list(framed.values())
    for at in (False, True):
        twin = name + ("_at" if at else "")
        for what, rows in row_faults(case, at):
            with pytest.raises(ValueError):
                case.call(name, at, rows=rows, **kw, **good)
                pytest.fail(f"{twin} took {what}")
        for arg, (dtype, need, shape) in outs.items():
            wrong = Framed(arg, other_dtype(dtype), need, shape)
            watched.append(wrong)
            bad = {"a CPU " + arg: good[arg].cpu(), arg + " one entry short": good[arg][:-1]}
            if name != "decode_emit":            # its out is checked for size only (see the module docstring)
                bad[arg + " of the wrong dtype"] = wrong.out
            for what, t in bad.items():
                with pytest.raises(ValueError):
                    case.call(name, at, **kw, **{**good, arg: t})
                    pytest.fail(f"{twin} took {what}")
        for arg in inputs:
            t = kw[arg]
            for what, t_bad in ((arg + " one row short", t[:-1]), (arg + " of the wrong dtype", t.to(other_dtype(t.dtype)))):
                with pytest.raises(ValueError):
                    case.call(name, at, **{**kw, arg: t_bad}, **good)
                    pytest.fail(f"{twin} took {what}")
    case.eng.wait()
    for f in watched:
        assert f.untouched(), f"a refused {name} call wrote"


@pytest.mark.parametrize("n", [V, 0])
@pytest.mark.parametrize("name", PAIRS)
def test_defaults_agree(any_case, name, n):
    case = any_case
    kw, outs, _ = case.spec(name, n)
    plain, at = case.call(name, False, rows=case.rows(False, n), **kw), case.call(name, True, rows=case.rows(True, n), **kw)
    case.eng.wait()
    assert len(plain) == len(at) == len(outs)
    if name == "decode_emit" and n == 0:         # the one difference between twins (see the module docstring)
        assert plain[0].dtype == at[0].dtype == u8 and plain[0].shape == (0,) and at[0].shape == (case.eng.gt_row_bytes,)
        return
    for p, q, (dtype, need, shape) in zip(plain, at, outs.values()):
        assert p.dtype == q.dtype == dtype and p.shape == q.shape and p.stride() == q.stride() and p.storage_offset() == q.storage_offset()
        assert p.device == q.device == case.recs.device
        if name != "decode_emit":                # (decode_emit returns the whole flat buffer)
            assert p.numel() == need
