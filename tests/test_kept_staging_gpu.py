"""GPU leg: the kept-list staging of the subset kernels (stage_kept_list, gt_common.hip.h) at its edges, every case byte for byte
against the CPU oracle with sentinels around the output.

The helper copies the kept list into a block's LDS table in batches of 16-byte loads (four entries), the up to three entries in
front of the slice's first 16-byte boundary and behind its last one as single loads, 16 * 256 entries per batch and block.  So the
edges are: lists shorter than one quad, list lengths around a multiple of four and around the 256 threads of a block, slices that
start at every rank residue mod 4 (the segment kernels: a segment's slice starts at seg_rank[segment]), and lists just below and
above one batch (4 096 entries, the row-owner kernel).  A wrong or missing table entry picks the wrong sample: the text differs.
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


def seeded_keep(n, k, seed):
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False)).astype(np.uint32)


def check_segments(eng, recs, host, v, n, kept, kernel, tune=()):
    k = len(kept)
    want = oracle.decode_emit(host, v, n, kept_idx=kept).tobytes()
    for knob, value in tune:
        eng.tune(knob, value)
    out = torch.full((FRAME + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
    eng.decode_emit(recs, v, out=out, kernel=kernel, out_offset=FRAME)
    eng.wait()
    got = out.cpu().numpy()
    assert (got[:FRAME] == SENTINEL).all() and (got[FRAME + len(want):] == SENTINEL).all(), f"kernel {kernel} K={k} wrote outside"
    assert got[FRAME:FRAME + len(want)].tobytes() == want, f"kernel {kernel} K={k}"


def check_lines(eng, recs, host, v, n, kept, kernel, seed):
    k = len(kept)
    rng = np.random.default_rng(seed)
    plen = rng.integers(22, 39, size=v).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)
    loff = np.concatenate([[0], np.cumsum(plen + 4 * k + 1)]).astype(np.int64)
    blob = rng.integers(65, 91, size=int(poff[-1]) + 1, dtype=np.uint8)
    want = oracle.emit_lines(host, v, n, blob, poff.astype(np.uint64), loff.astype(np.uint64), kept_idx=kept).tobytes()
    d_blob, d_poff, d_loff = (torch.from_numpy(x).to(DEV) for x in (blob, poff, loff))
    out = torch.full((FRAME + len(want) + FRAME,), SENTINEL, dtype=torch.uint8, device=DEV)
    eng.emit_lines(recs, v, d_blob, d_poff, d_loff, int(plen.max()), out[FRAME:], kernel=kernel)
    eng.wait()
    got = out.cpu().numpy()
    assert (got[:FRAME] == SENTINEL).all() and (got[FRAME + len(want):] == SENTINEL).all(), f"lines, kernel {kernel} K={k} wrote outside"
    assert got[FRAME:FRAME + len(want)].tobytes() == want, f"lines, kernel {kernel} K={k}"


@pytest.mark.parametrize("k", [1, 3, 4, 5, 255, 256, 257, 2503])
def test_pick_kernels_list_lengths(k):
    """N = 2 504 through the short-record pick kernel (GT segments) and its full-line kernel: lists of less than one quad, around a
    multiple of four, around the block's 256 threads, and all but one sample."""
    n, v = 2504, 9
    kept = seeded_keep(n, k, 1000 + k)
    r = oracle.variant_record_size(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=k)
        host = recs[: v * r].cpu().numpy()
        check_segments(eng, recs, host, v, n, kept, _capi.KERNEL_PICK)
        check_lines(eng, recs, host, v, n, kept, _capi.KERNEL_PICK, 2000 + k)


@pytest.mark.parametrize("k", [8, 9, 11, 255, 256, 257, 299])
def test_line_run_kernel_list_lengths(k):
    """The line-run kernel's kept table (it takes a keep list of >= 8 out of <= 4 096 samples and at least two lines per item, so
    N = 300, not 2 504): the same length edges."""
    n, v = 300, 40
    kept = seeded_keep(n, k, 3000 + k)
    r = oracle.variant_record_size(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=k)
        host = recs[: v * r].cpu().numpy()
        check_lines(eng, recs, host, v, n, kept, _capi.KERNEL_RUNS, 4000 + k)


@pytest.mark.parametrize("res1,res2", [(0, 1), (1, 2), (2, 3), (3, 0)])
def test_segment_kernels_slices_at_every_rank_residue(res1, res2):
    """N = 40 000 = three segments of 16 384 samples.  The kept list is built so that seg_rank[1] = res1 and seg_rank[2] = res2 mod 4:
    the slices of segments 1 and 2 start 4 * res bytes past a 16-byte boundary of the kept list (the unaligned 16-byte path: 3, 2, 1
    or 0 single entries in front of the first quad).  The single-pass segment kernel (forced) and the segment compact kernel (AUTO
    takes the two passes at ~1 % kept; few rows, so the compact pass is the segment kernel's) both stage per segment."""
    n, v = 40_000, 24
    rng = np.random.default_rng(5000 + 4 * res1 + res2)
    c0 = 200 + res1                                      # kept samples in segment 0
    c1 = 148 + (res2 - (c0 + 148)) % 4                   # ... in segment 1: c0 + c1 = res2 mod 4
    c2 = 77
    kept = np.sort(np.concatenate([rng.choice(16_384, size=c0, replace=False), 16_384 + rng.choice(16_384, size=c1, replace=False),
                                   32_768 + rng.choice(n - 32_768, size=c2, replace=False)])).astype(np.uint32)
    assert int((kept < 16_384).sum()) % 4 == res1 and int((kept < 32_768).sum()) % 4 == res2
    r = oracle.variant_record_size(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=31)
        host = recs[: v * r].cpu().numpy()
        check_segments(eng, recs, host, v, n, kept, _capi.KERNEL_SCAN)
        check_segments(eng, recs, host, v, n, kept, _capi.KERNEL_AUTO, tune=((_capi.KNOB_SCAN_ROWPICK, -1),))


@pytest.mark.parametrize("k", [4093, 4094, 4095, 4096, 4097, 4098, 4099])
def test_row_owner_kernel_lists_around_one_batch(k):
    """N = 16 400 (two segments, the second 16 samples long) through the row-owner kernel, whose table is the WHOLE kept list: K just
    below, at and just above the 4 096 entries one batch of a 256-thread block holds (the second batch then has one to three
    entries, or one quad)."""
    n, v = 16_400, 10
    kept = seeded_keep(n, k, 6000 + k)
    r = oracle.variant_record_size(n)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        recs = eng.synth_records(v, first_variant=k)
        host = recs[: v * r].cpu().numpy()
        check_segments(eng, recs, host, v, n, kept, _capi.KERNEL_ROWPICK)
