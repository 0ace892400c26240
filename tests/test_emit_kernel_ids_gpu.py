"""Every kernel id through every emit entry point: accepted exactly where tests/subset_plan.py ``accepts`` says, refused elsewhere.

capi.hip chooses the emit kernel in one place (``choose``) for pgenhip_decode_emit, pgenhip_decode_emit_at and pgenhip_emit_lines.
This walks flags 0 .. 15, 0x10 and 0x13 over small shapes on both sides of every forced-kernel check (N below and above 61 and
1 024, all samples / a kept list / an identity list / one sample past the row owner's kept limit / an empty list) and five calls
per shape: GT segments at the dense pitch, at pitch 4K + 4, through a variant gather, through record byte offsets, and full lines
with 10-byte prefixes.  An accepted call returns PGENHIP_OK and writes the oracle's bytes inside an untouched sentinel frame; a
refused one returns PGENHIP_ERR_BAD_ARG and writes nothing.  Every launch is one the library documents as legal or refuses before
launching."""
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
V = 5
PREFIX = 10
KERNEL_IDS = tuple(range(16)) + (0x10, 0x13)
AUTO_AND_ROWS = (_capi.KERNEL_AUTO, _capi.KERNEL_ROWS)
CALLS = ("dense", "padded", "gathered", "at", "lines")

# (N, kept list: None = all samples, "identity", or a sample count), the kernel ids the shape runs
SHAPES = [(40, None, KERNEL_IDS), (40, 5, KERNEL_IDS), (300, None, KERNEL_IDS), (300, 30, KERNEL_IDS), (300, "identity", KERNEL_IDS),
          (1024, None, KERNEL_IDS), (5000, 50, KERNEL_IDS), (20_000, SP.ROWPICK_MAX_KEPT + 1, KERNEL_IDS), (300, 0, AUTO_AND_ROWS)]


def _kept(rng, n, spec):
    if spec is None:
        return None
    if spec == "identity":
        return np.arange(n, dtype=np.uint32)
    return np.sort(rng.choice(n, size=spec, replace=False)).astype(np.uint32)


class Call:
    """One call of one entry point on V rows: its device inputs, where its bytes land in the framed output, and the oracle's bytes."""

    def __init__(self, rng, kind, n, kept):
        self.kind = kind
        k = n if kept is None else int(kept.size)
        r = oracle.variant_record_size(n)
        row = 4 * k + 1
        self.stride = row + 3 if kind == "padded" else row
        v_file = V + 3 if kind == "gathered" else V
        recs = rng.integers(0, 256, size=v_file * r + 16, dtype=np.uint8)
        self.d_recs = torch.from_numpy(recs).to(DEV)
        self.d_vidx = self.d_off = None
        vidx = None
        if kind == "gathered":
            vidx = np.sort(rng.choice(v_file, size=V, replace=False)).astype(np.uint32)
            self.d_vidx = torch.from_numpy(vidx.astype(np.int32)).to(DEV)
        if kind == "at":
            # record j at odd byte offset 1 + perm[j] * s of one buffer
            s = r + (2 if r % 2 == 0 else 1)
            perm = rng.permutation(V)
            base = np.full(1 + V * s + 16, 0x5A, dtype=np.uint8)
            base[1 : 1 + V * s].reshape(V, s)[perm, :r] = recs[: V * r].reshape(V, r)
            off = 1 + perm.astype(np.int64) * s
            self.d_recs, self.d_off = torch.from_numpy(base).to(DEV), torch.from_numpy(off).to(DEV)
            want = oracle.decode_emit_at(base, off.astype(np.uint64), n, kept_idx=kept)
        elif kind == "lines":
            blob = np.concatenate([rng.integers(33, 127, size=V * PREFIX, dtype=np.uint8), np.frombuffer(b"!" * 16, dtype=np.uint8)])
            poff = (np.arange(V + 1) * PREFIX).astype(np.int64)
            loff = (np.arange(V + 1) * (PREFIX + row)).astype(np.int64)
            self.d_blob, self.d_poff, self.d_loff = (torch.from_numpy(x).to(DEV) for x in (blob, poff, loff))
            want = oracle.emit_lines(recs, V, n, blob, poff.astype(np.uint64), loff.astype(np.uint64), kept_idx=kept)
        else:
            want = oracle.decode_emit(recs, V, n, kept_idx=kept, variant_idx=vidx)
        # the whole framed buffer as an accepted call leaves it: the rows at their pitch, sentinel bytes everywhere else
        if kind == "lines":
            body = want
        else:
            body = np.full((V - 1) * self.stride + row, SENTINEL, dtype=np.uint8)
            for j in range(V):
                body[j * self.stride : j * self.stride + row] = want[j * row : (j + 1) * row]
        self.size = LEAD + body.size + TAIL
        self.accepted = np.full(self.size, SENTINEL, dtype=np.uint8)
        self.accepted[LEAD : LEAD + body.size] = body

    def run(self, eng, flags, n_variants=V):
        """-> (status, the framed output)."""
        out = torch.full((self.size,), SENTINEL, dtype=torch.uint8, device=DEV)
        lib, o = _capi.lib, out.data_ptr() + LEAD
        if self.kind == "lines":
            rc = lib.pgenhip_emit_lines(eng._ctx, self.d_recs.data_ptr(), eng.record_size, None, n_variants, self.d_blob.data_ptr(),
                                        self.d_poff.data_ptr(), self.d_loff.data_ptr(), PREFIX, o, flags)
        elif self.kind == "at":
            rc = lib.pgenhip_decode_emit_at(eng._ctx, self.d_recs.data_ptr(), self.d_off.data_ptr(), n_variants, o, self.stride, flags)
        else:
            rc = lib.pgenhip_decode_emit(eng._ctx, self.d_recs.data_ptr(), eng.record_size,
                                         None if self.d_vidx is None else self.d_vidx.data_ptr(), n_variants, o, self.stride, flags)
        eng.wait()
        return rc, out.cpu().numpy()


def _accepts(kernel, kind, n, k, subset):
    if kind == "lines":
        return SP.accepts(kernel, n, k, subset, PREFIX, False)
    return SP.accepts(kernel, n, k, subset, gather=kind in ("gathered", "at"), mode="segments", dense_pitch=kind != "padded")


@pytest.mark.parametrize("n,spec,kernels", SHAPES, ids=[f"n={n},kept={'all' if s is None else s}" for n, s, _ in SHAPES])
def test_kernel_ids(n, spec, kernels):
    rng = np.random.default_rng(n + (0 if spec is None else 7 if spec == "identity" else 13 + spec))
    kept = _kept(rng, n, spec)
    k = n if kept is None else int(kept.size)
    with pgen_rs_amd.GtEngine(n, kept_idx=kept, device=0) as eng:
        for kind in CALLS:
            call = Call(rng, kind, n, kept)
            for kernel in kernels:
                ok = _accepts(kernel, kind, n, k, kept is not None)
                rc, got = call.run(eng, kernel)
                what = f"n={n} k={k} kept={'all' if spec is None else spec} {kind} flags={kernel:#x}"
                if not ok:
                    assert rc == _capi.ERR_BAD_ARG, f"{what}: expected a refusal, got status {rc}"
                    assert (got == SENTINEL).all(), f"{what}: a refused call wrote"
                    assert _capi.lib.pgenhip_last_error_detail(), f"{what}: a refusal without a detail"
                    continue
                assert rc == _capi.OK, f"{what}: status {rc} ({_capi.lib.pgenhip_last_error_detail().decode()})"
                if not np.array_equal(got, call.accepted):
                    bad = np.flatnonzero(got != call.accepted)
                    raise AssertionError(f"{what}: {bad.size} bytes differ from the oracle's framed output, first at {bad[:6] - LEAD}")


def test_empty_calls():
    """n_variants == 0.  GT segments: flag bits outside PGENHIP_KERNEL_MASK are refused first, an unknown id inside the mask is
    not looked at; full lines: PGENHIP_OK whatever flags holds.  Nothing is written either way."""
    rng = np.random.default_rng(0)
    with pgen_rs_amd.GtEngine(300, device=0) as eng:
        for kind, status in (("dense", {5: _capi.OK, 0x10: _capi.ERR_BAD_ARG}), ("at", {5: _capi.OK, 0x10: _capi.ERR_BAD_ARG}),
                             ("lines", {5: _capi.OK, 0x10: _capi.OK})):
            call = Call(rng, kind, 300, None)
            for flags, want in status.items():
                rc, got = call.run(eng, flags, n_variants=0)
                assert rc == want, f"{kind} flags={flags:#x} n_variants=0: status {rc}"
                assert (got == SENTINEL).all()
