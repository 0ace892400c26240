"""GPU leg of the stream kernel's launch rule (plan::wide::rule): forced write fronts, store policies, blocks per CU and every burst
length; and coverage of the row-tail path, where the chunk that holds row j's '\n' takes the first byte of row j+1 from the loader's
one-lane load, at the record alignments and row lengths at which that byte lies in another 16-byte piece than the record's last.

Every case is byte equality with the CPU oracle, the output framed by 256 sentinel bytes on both sides as in
tests/test_store_policy_gpu.py.  All launches are forced onto the row-item kernel (KERNEL_WIDE), so the short rows of the burst cases
reach it too.  The shapes are the smallest that reach each path: one-span rows whose added byte stays in the last 16-byte piece or
opens a new one (record address mod 16 = 13 with R = 626), R a multiple of 16, the tail span of a multi-span row, a 123-span row, the
shortest AUTO row-item rows (N = 1 916); each dense, through a variant list and with padded records (the pad bytes are 0xFF, so a
launch that read the byte behind a padded record for the next row's first byte would write '.' where a digit belongs).
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
BURSTS = (1, 2)   # every burst length the tree has an instantiation for (PGENHIP_KNOB_WIDE_BURST)


class Case:
    """Records of one shape on the host, and the oracle's text of them, made once per shape."""

    def __init__(self, n, v, first_variant):
        self.n, self.v, self.r = n, v, oracle.variant_record_size(n)
        self.host = oracle.synth_records(n, v, first_variant=first_variant)
        self.rows = oracle.decode_emit(self.host, v, n).reshape(v, 4 * n + 1)
        self.perm = np.random.default_rng(n + v).permutation(v).astype(np.uint32)

    def device_records(self, mode, offset):
        """(device tensor, record_stride, variant_idx, expected text): the records start `offset` bytes into the tensor."""
        recs2d = self.host.reshape(self.v, self.r)
        stride = self.r + 3 if mode == "padded" else self.r
        buf = np.full(offset + self.v * stride + 16, 0xFF, dtype=np.uint8)
        view = buf[offset:offset + self.v * stride].reshape(self.v, stride)
        view[:, :self.r] = recs2d
        vidx = torch.from_numpy(self.perm.astype(np.int32)).to(DEV) if mode == "list" else None
        want = (self.rows[self.perm] if mode == "list" else self.rows).tobytes()
        return torch.from_numpy(buf).to(DEV), stride, vidx, want


CASES = {}


def case(n, v, first_variant=3):
    key = (n, v, first_variant)
    if key not in CASES:
        CASES[key] = Case(n, v, first_variant)
    return CASES[key]


def emit_and_check(eng, c, mode, rec_offset, base, what):
    recs, stride, vidx, want = c.device_records(mode, rec_offset)
    assert recs.data_ptr() % 16 == 0
    out = torch.full((FRAME + base + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 16 == 0
    eng.decode_emit(recs, c.v, record_stride=stride, variant_idx=vidx, out=out, kernel=_capi.KERNEL_WIDE, records_offset=rec_offset, out_offset=FRAME + base)
    eng.wait()
    got = out.cpu().numpy()
    lo = FRAME + base
    assert (got[:lo] == SENTINEL).all() and (got[lo + len(want):] == SENTINEL).all(), f"{what}: wrote outside the text"
    assert got[lo:lo + len(want)].tobytes() == want, what


MODES = ["dense", "list", "padded"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rec_mod16", [0, 1, 13, 14, 15])
def test_row_tail_one_span_rows(mode, rec_mod16):
    """N = 2 504 (R = 626), V = 9: the first record's address mod 16 over 0, 1, 13, 14, 15 (with R = 626 the byte behind a record
    lies in a new 16-byte piece at 13: 13 + 626 = 639 = 16 * 40 - 1); the output base at 0, 1 and 15."""
    c = case(2504, 9)
    with pgen_rs_amd.GtEngine(c.n, device=0) as eng:
        for base in (0, 1, 15):
            emit_and_check(eng, c, mode, rec_mod16, base, f"{mode} records at +{rec_mod16} out at +{base}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,v", [(2560, 5), (20_000, 3), (500_000, 2), (1916, 40)])
def test_row_tail_other_rows(mode, n, v):
    """R a multiple of 16 (N = 2 560), the tail span of a five-span row (N = 20 000), a 123-span row (N = 500 000) and the shortest
    rows AUTO gives the row-item kernel (N = 1 916, R = 479); records at address mod 16 = 0 and 13, output base 0, 1 and 15."""
    c = case(n, v)
    with pgen_rs_amd.GtEngine(c.n, device=0) as eng:
        for rec_offset, base in ((0, 0), (0, 1), (13, 15), (13, 0)):
            emit_and_check(eng, c, mode, rec_offset, base, f"N={n} {mode} records at +{rec_offset} out at +{base}")


@pytest.mark.parametrize("n,v", [(2504, 9), (20_000, 3)])
@pytest.mark.parametrize("fronts", [1, 2, 8, 64])
def test_forced_fronts(n, v, fronts):
    """Write fronts forced to 1, 2, 8 and 64 on launches of 9 and 15 items: most ranges are empty, so a block steals through drained
    ranges; alone and crossed with both store policies and 1 and 4 blocks per CU."""
    c = case(n, v)
    with pgen_rs_amd.GtEngine(c.n, device=0) as eng:
        eng.tune(_capi.KNOB_WIDE_RANGES, fronts)
        emit_and_check(eng, c, "dense", 0, 1, f"N={n} fronts {fronts}")
        for policy in (1, 2):
            for per_cu in (1, 4):
                eng.tune(_capi.KNOB_STORE_POLICY, policy)
                eng.tune(_capi.KNOB_WIDE_BLOCKS_PER_CU, per_cu)
                emit_and_check(eng, c, "dense", 0, 1, f"N={n} fronts {fronts} policy {policy} blocks per CU {per_cu}")


@pytest.mark.parametrize("burst", BURSTS)
@pytest.mark.parametrize("n", [1024, 1280, 1536, 2504])
def test_burst_lengths(burst, n):
    """Rows of 4, 5, 6 and 9 whole store steps, V = 7: the number of plain steps of a row below, at and above every burst length; dense
    and gathered rows, and N = 20 000 (V = 3), whose five-span rows are the kind the rule gives single store steps on long launches."""
    c = case(n, 7)
    with pgen_rs_amd.GtEngine(c.n, device=0) as eng:
        eng.tune(_capi.KNOB_WIDE_BURST, burst)
        for policy in (1, 2):
            eng.tune(_capi.KNOB_STORE_POLICY, policy)
            for base in (0, 9):
                emit_and_check(eng, c, "dense", 0, base, f"N={n} burst {burst} policy {policy} out at +{base}")
            emit_and_check(eng, c, "list", 0, 1, f"N={n} burst {burst} policy {policy} variant list")
    if n == 2504:
        c = case(20_000, 3)
        with pgen_rs_amd.GtEngine(c.n, device=0) as eng:
            eng.tune(_capi.KNOB_WIDE_BURST, burst)
            for policy in (1, 2):
                eng.tune(_capi.KNOB_STORE_POLICY, policy)
                emit_and_check(eng, c, "dense", 0, 3, f"N=20000 burst {burst} policy {policy}")


def test_burst_knob_values():
    with pgen_rs_amd.GtEngine(2504, device=0) as eng:
        for bad in (-1, 3, 4):
            with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                eng.tune(_capi.KNOB_WIDE_BURST, bad)
            assert ei.value.status == _capi.ERR_BAD_ARG
        for ok in (2, 1, 0):
            eng.tune(_capi.KNOB_WIDE_BURST, ok)
