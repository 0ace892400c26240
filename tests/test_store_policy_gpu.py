"""GPU leg: the text-store policy knob (PGENHIP_KNOB_STORE_POLICY: 1 = non-temporal stores, 2 = non-temporal write-through stores,
`global_store_dwordx4 ... sc1 nt` through inline asm) forced to both values at the smallest shape that reaches each store site.
Every case is byte equality with the CPU oracle, the output framed by 256 sentinel bytes on both sides.

The stream kernel (row items, LINES, RUNS) takes the policy; the other kernels of the table below store as before whatever the
knob says, and run here under both values all the same (a forced value must never change a byte anywhere).  A write-through store
that the compiler does not count (the asm form) could lose bytes only by being dropped or mis-addressed: both show as sentinels
inside the text or text outside it.
"""
import numpy as np
import pytest
import torch

import pgen_oracle as oracle
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5
FRAME = 256
POLICIES = [1, 2]


def emit_and_check(eng, recs, host, v, n, kept, kernel=_capi.KERNEL_AUTO, base=0, what=""):
    """GT segments at out + FRAME + base (any byte offset), compared with the oracle; sentinels around them untouched."""
    want = oracle.decode_emit(host, v, n, kept_idx=kept).tobytes()
    out = torch.full((FRAME + base + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
    eng.decode_emit(recs, v, out=out, kernel=kernel, out_offset=FRAME + base)
    eng.wait()
    got = out.cpu().numpy()
    lo = FRAME + base
    assert (got[:lo] == SENTINEL).all() and (got[lo + len(want):] == SENTINEL).all(), f"{what}: wrote outside the text"
    assert got[lo:lo + len(want)].tobytes() == want, what


def lines_and_check(eng, recs, host, v, n, kept, seed, kernel=_capi.KERNEL_AUTO, what=""):
    k = n if kept is None else len(kept)
    rng = np.random.default_rng(seed)
    plen = rng.integers(22, 39, size=v).astype(np.int64)                     # prefixes of 22-38 bytes
    poff = np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)
    loff = np.concatenate([[0], np.cumsum(plen + 4 * k + 1)]).astype(np.int64)
    blob = rng.integers(65, 91, size=int(poff[-1]) + 1, dtype=np.uint8)
    want = oracle.emit_lines(host, v, n, blob, poff.astype(np.uint64), loff.astype(np.uint64), kept_idx=kept).tobytes()
    d_blob, d_poff, d_loff = (torch.from_numpy(x).to(DEV) for x in (blob, poff, loff))
    out = torch.full((FRAME + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
    eng.emit_lines(recs, v, d_blob, d_poff, d_loff, int(plen.max()), out[FRAME:], kernel=kernel)
    eng.wait()
    got = out.cpu().numpy()
    assert (got[:FRAME] == SENTINEL).all() and (got[FRAME + len(want):] == SENTINEL).all(), f"{what}: wrote outside the lines"
    assert got[FRAME:FRAME + len(want)].tobytes() == want, what


def engine(n, policy, kept=None):
    eng = pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0)
    eng.tune(_capi.KNOB_STORE_POLICY, policy)
    return eng


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("base", [0, 1, 15])
def test_row_items_one_span(policy, base):
    """N = 2 504, V = 9: one span per row; the output base at byte offsets 0, 1 and 15 of a 16-byte chunk (head chunk, byte-wise first
    and last chunk of the stream, the '\\n' merge of every row's last chunk)."""
    n, v = 2504, 9
    r = oracle.variant_record_size(n)
    with engine(n, policy) as eng:
        recs = eng.synth_records(v, first_variant=base)
        emit_and_check(eng, recs, recs[: v * r].cpu().numpy(), v, n, None, base=base, what=f"policy {policy} base {base}")


@pytest.mark.parametrize("policy", POLICIES)
def test_row_items_several_spans(policy):
    """N = 20 000, V = 3: five spans per row, the last one short."""
    n, v = 20_000, 3
    r = oracle.variant_record_size(n)
    with engine(n, policy) as eng:
        recs = eng.synth_records(v, first_variant=2)
        emit_and_check(eng, recs, recs[: v * r].cpu().numpy(), v, n, None, base=3, what=f"policy {policy}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,v", [(300, 100), (8, 50)])
def test_runs(policy, n, v):
    """RUNS mode: several runs and a partial last run (N = 300: 12 rows per item), and the shortest rows it takes (N = 8)."""
    r = oracle.variant_record_size(n)
    with engine(n, policy) as eng:
        recs = eng.synth_records(v, first_variant=7, hwe=True)
        for base in (0, 5):
            emit_and_check(eng, recs, recs[: v * r].cpu().numpy(), v, n, None, base=base, what=f"policy {policy} N={n} base {base}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,v", [(2504, 9), (300, 40)])
def test_full_lines(policy, n, v):
    """pgenhip_emit_lines with prefixes of 22-38 bytes: the stream kernel's LINES mode (N = 2 504) and line runs (N = 300)."""
    r = oracle.variant_record_size(n)
    with engine(n, policy) as eng:
        recs = eng.synth_records(v, first_variant=9)
        lines_and_check(eng, recs, recs[: v * r].cpu().numpy(), v, n, None, 70 + n, what=f"policy {policy} N={n}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,k,v,kernel", [(2504, 250, 64, _capi.KERNEL_PICK), (20_000, 2_000, 64, _capi.KERNEL_SCAN), (20_000, 200, 300, _capi.KERNEL_AUTO)])
def test_subset_kernels(policy, n, k, v, kernel):
    """The pick kernel, the segment kernel, and the two passes with the segment compact kernel (K = 200 of 20 000 lies inside
    two_pass_shape; 300 rows are too few for the row-owner compact pass): the second pass is the stream kernel on the compact records."""
    kept = np.sort(np.random.default_rng(n + k).choice(n, size=k, replace=False)).astype(np.uint32)
    r = oracle.variant_record_size(n)
    with engine(n, policy, kept) as eng:
        recs = eng.synth_records(v, first_variant=13)
        emit_and_check(eng, recs, recs[: v * r].cpu().numpy(), v, n, kept, kernel=kernel, base=1, what=f"policy {policy} N={n} K={k}")


@pytest.fixture(scope="module")
def row_owner_case():
    """N = 24 600, K = 246 and as many rows as the row-owner kernel asks for under AUTO (8 x CUs x 4): ~50 MB of records; the records
    and the oracle's text are made once for both policies.  (Below N = 24 576 AUTO lets the row-owner kernel write the text in one
    pass; from there 1 % kept takes the two passes, and with this many rows the compact pass is the row-owner kernel's.)"""
    n, k = 24_600, 246
    v = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    kept = np.sort(np.random.default_rng(246).choice(n, size=k, replace=False)).astype(np.uint32)
    host = oracle.synth_records(n, v, first_variant=21)
    return n, v, kept, host, oracle.decode_emit(host, v, n, kept_idx=kept).tobytes()


@pytest.mark.parametrize("policy", POLICIES)
def test_row_owner_compact_pass_and_text(policy, row_owner_case):
    """The two passes with the row-owner compact pass (AUTO: K = 1 % of N, enough rows), and the row-owner kernel writing text (forced)."""
    n, v, kept, host, want = row_owner_case
    with engine(n, policy, kept) as eng:
        recs = torch.from_numpy(host).to(DEV)
        for kernel in (_capi.KERNEL_AUTO, _capi.KERNEL_ROWPICK):
            out = torch.full((FRAME + 7 + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
            eng.decode_emit(recs, v, out=out, kernel=kernel, out_offset=FRAME + 7)
            eng.wait()
            got = out.cpu().numpy()
            lo = FRAME + 7
            assert (got[:lo] == SENTINEL).all() and (got[lo + len(want):] == SENTINEL).all(), f"policy {policy} kernel {kernel}: wrote outside"
            assert got[lo:lo + len(want)].tobytes() == want, f"policy {policy} kernel {kernel}"


def test_knob_values():
    with pgen_rs_amd.GtEngine(2504, device=0) as eng:
        for bad in (-1, 3):
            with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                eng.tune(_capi.KNOB_STORE_POLICY, bad)
            assert ei.value.status == _capi.ERR_BAD_ARG
        for ok in (2, 1, 0):
            eng.tune(_capi.KNOB_STORE_POLICY, ok)
