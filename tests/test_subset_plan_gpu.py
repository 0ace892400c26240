"""The kept-subset GT path at every edge of its dispatch and launch plans, byte for byte against the oracle.

tests/subset_plan.py runs, from csrc/launch_plan.h, AUTO's subset dispatch (row owner, two passes, segment kernel, general kernel), the segment kernel's
launch plan (groups, XCD map, bands, rounds), the chunking of the two passes and the row owner's plan (LDS bytes, blocks per CU,
its segment limit); its cell table places cells on both sides of every edge those derive from N, K, V and the CU count (the
device's own: the table is computed from it).  Each cell runs AUTO and every forced kernel that accepts the shape (forced kernels
that refuse must refuse with the status the plan names and write nothing), as GT segments, through a variant gather, through
record byte offsets (pgenhip_decode_emit_at: records at odd offsets, in permuted order, inside one buffer) or as full lines.
Every output is framed by sentinel bytes that must stay untouched, and the whole buffer is compared with the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pgen_oracle as oracle
import pgen_rs_amd
import subset_plan as SP
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5
LEAD, TAIL = 67, 64
KID = {"auto": _capi.KERNEL_AUTO, "rows": _capi.KERNEL_ROWS, "scan": _capi.KERNEL_SCAN, "rowpick": _capi.KERNEL_ROWPICK}
STATUS = {"bad_arg": _capi.ERR_BAD_ARG, "hip": _capi.ERR_HIP}
KNOB = {"scan_blocks_per_cu": _capi.KNOB_SCAN_BLOCKS_PER_CU, "rowpick_blocks_per_cu": _capi.KNOB_ROWPICK_BLOCKS_PER_CU,
        "scan_chunk_rows": _capi.KNOB_SCAN_CHUNK_ROWS, "scan_xcd_map": _capi.KNOB_SCAN_XCD_MAP,
        "scan_two_pass": _capi.KNOB_SCAN_TWO_PASS, "scan_rowpick": _capi.KNOB_SCAN_ROWPICK}

_TABLE = SP.cells()   # (the ids; the cells themselves come from the device's CU count: same table layout)


def _cell(i):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table = SP.cells(cus)
    assert len(table) == len(_TABLE)
    return table[i], cus


def _id(c):
    io = ",at" if c.at else ",gathered" if c.gathered else ""
    knobs = "".join(f",{k}={v}" for k, v in c.tune.knobs().items())
    return f"{c.group}:n={c.n},k={c.k},v={c.v},{c.mode}{io}{',cluster=%d' % c.cluster if c.cluster else ''}{knobs}:{'+'.join(c.kernels)}"


class Inputs:
    """Records (dense, gathered from a larger file, or at byte offsets), the kept list's oracle output, and a launcher per kernel."""

    def __init__(self, eng, cell, kept, rng):
        n, v = cell.n, cell.v
        r = oracle.variant_record_size(n)
        self.cell, self.eng = cell, eng
        v_file = v + v // 8 + 3 if cell.gathered else v
        d_recs = eng.synth_records(v_file, first_variant=cell.k, seed=0x5EED + n)
        recs = d_recs.cpu().numpy()
        self.vidx = self.d_vidx = None
        self.d_base = self.d_off = None
        if cell.gathered:
            self.vidx = np.sort(rng.choice(v_file, size=v, replace=False)).astype(np.uint32)
            self.d_vidx = torch.from_numpy(self.vidx.astype(np.int32)).to(DEV)
        if cell.at:
            # record j at odd byte offset 1 + perm[j] * S of one buffer (S even), the other bytes filler
            s = r + (2 if r % 2 == 0 else 1)
            perm = rng.permutation(v)
            base = np.full(1 + v * s + 16, 0x5A, dtype=np.uint8)
            base[1 : 1 + v * s].reshape(v, s)[perm, :r] = recs.reshape(v, r)
            off = (1 + perm.astype(np.int64) * s).astype(np.int64)
            self.want = oracle.decode_emit_at(base, off.astype(np.uint64), n, kept_idx=kept)
            assert np.array_equal(self.want, oracle.decode_emit(recs, v, n, kept_idx=kept))
            self.d_base, self.d_off = torch.from_numpy(base).to(DEV), torch.from_numpy(off).to(DEV)
            del d_recs
            self.d_recs = None
        else:
            self.d_recs = d_recs
        if cell.mode == "lines":
            lens = rng.integers(0, 41, size=v)
            lens[rng.random(v) < 0.2] = 0
            self.pmax = int(lens.max())
            blob = np.concatenate([rng.integers(33, 127, size=int(lens.sum()), dtype=np.uint8), np.frombuffer(b"!" * 16, dtype=np.uint8)])
            poff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            loff = np.concatenate([[0], np.cumsum(lens + 4 * cell.k + 1)]).astype(np.int64)
            self.want = oracle.emit_lines(recs, v, n, blob, poff.astype(np.uint64), loff.astype(np.uint64), kept_idx=kept, variant_idx=self.vidx)
            self.d_blob, self.d_poff, self.d_loff = (torch.from_numpy(x).to(DEV) for x in (blob, poff, loff))
        elif not cell.at:
            self.want = oracle.decode_emit(recs, v, n, kept_idx=kept, variant_idx=self.vidx)
        assert self.want.size == (int(loff[-1]) if cell.mode == "lines" else v * (4 * cell.k + 1))

    def launch(self, kern, out):
        c, eng = self.cell, self.eng
        if c.mode == "lines":
            eng.emit_lines(self.d_recs, c.v, self.d_blob, self.d_poff, self.d_loff, self.pmax, out[LEAD:], variant_idx=self.d_vidx, kernel=KID[kern])
        elif c.at:
            eng.decode_emit_at(self.d_base, self.d_off, c.v, out=out[LEAD:], kernel=KID[kern])
        else:
            eng.decode_emit(self.d_recs, c.v, variant_idx=self.d_vidx, out=out, out_offset=LEAD, kernel=KID[kern])


@pytest.mark.parametrize("i", range(len(_TABLE)), ids=[_id(c) for c in _TABLE])
def test_subset_cell(i):
    cell, cus = _cell(i)
    r = oracle.variant_record_size(cell.n)
    out_bytes = cell.v * (4 * cell.k + 1 + (40 if cell.mode == "lines" else 0))
    rec_bytes = (cell.v + cell.v // 8 + 3) * r * (2 if cell.at else 1)
    free, _ = torch.cuda.mem_get_info(0)
    if free < rec_bytes + out_bytes + (2 << 30):
        pytest.skip(f"needs {(rec_bytes + out_bytes) / 2**30:.1f} GiB of free HBM and 2 GiB to spare")
    kept = cell.kept()
    rng = np.random.default_rng(i)
    with pgen_rs_amd.GtEngine(cell.n, kept_idx=kept, device=0) as eng:
        for name, value in cell.tune.knobs().items():
            eng.tune(KNOB[name], value)
        inp = Inputs(eng, cell, kept, rng)
        size = inp.want.size
        for kern in cell.kernels:
            plan = cell.plan(kern, cus)
            what = f"{_id(cell)} kernel={kern} plan={plan}"
            out = torch.full((LEAD + size + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
            if plan.status != "ok":
                with pytest.raises(pgen_rs_amd.PgenHipError) as ei:
                    inp.launch(kern, out)
                eng.wait()
                assert ei.value.status == STATUS[plan.status], what
                assert bool((out == SENTINEL).all()), f"{what}: a refused launch wrote bytes"
                continue
            inp.launch(kern, out)
            eng.wait()
            got = out.cpu().numpy()
            assert (got[:LEAD] == SENTINEL).all() and (got[LEAD + size :] == SENTINEL).all(), f"{what}: bytes written outside the output"
            body = got[LEAD : LEAD + size]
            if not np.array_equal(body, inp.want):
                bad = np.flatnonzero(body != inp.want)
                row = 4 * cell.k + 1
                raise AssertionError(f"{what}: {bad.size} bytes differ, first at byte {bad[0]} (row {bad[0] // row} of GT segments), "
                                     f"last at {bad[-1]} (row {bad[-1] // row})")
            del out, got, body
    del inp
    torch.cuda.empty_cache()
