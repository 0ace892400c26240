"""Numeric genotype matrix at the measured shapes, full size: configs[2] (100 000 x 500 000: int8 in both orientations, the
sample-major one at the padded pitch and at the dense pitch of 100 000 bytes, a multiple of 16 but not of 128; f32 variant-major,
the 212-GB launch; int8 through a permutation of all rows), the chr22 shape (1 103 547 x 2 504, both orientations) and the basic2
shape (9 200 000 x 300), on the HWE records the tools time.  Offsets pass 4 GiB in both orientations.

The reference is a torch unpack on the device (shift, mask, table lookup), done in row bands that fit beside the output; every
element is compared, none sampled.  One exception, as the issue allows: the chr22 dense sample-major matrix has an odd pitch, so AUTO
takes GENERAL there; it is run and checked on a band of the first 100 001 variants (an odd pitch again), every element of the band."""
import numpy as np
import pytest
import torch

import matrix_plan as MP
import pgen_rs_amd
from pgen_rs_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND_ELEMS = 64 << 20
_CACHE = {}


def records_for(v: int, n: int, extra_bytes: int):
    """The shape's HWE records (cached across the tests of one shape); skips when records + output + checker do not fit."""
    r = MP.record_size(n)
    if _CACHE.get("shape") != (v, n):
        _CACHE.clear()
        torch.cuda.empty_cache()
        free, _total = torch.cuda.mem_get_info(0)
        if free < v * r + (4 << 30):
            pytest.skip(f"needs {(v * r + (4 << 30)) / 2**30:.1f} GiB of free HBM, have {free / 2**30:.1f}")
        with pgen_rs_amd.GtEngine(n, device=0) as eng:
            recs = eng.synth_records(v, hwe=True)
            eng.wait()
        _CACHE.update(shape=(v, n), recs=recs)
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(0)
    if free < extra_bytes + (6 << 30):
        pytest.skip(f"needs {(extra_bytes + (6 << 30)) / 2**30:.1f} GiB of free HBM beside the records, have {free / 2**30:.1f}")
    return _CACHE["recs"]


def lut_for(dtype) -> torch.Tensor:
    """The default patterns as integers of the element size, on the device."""
    bits = pgen_rs_amd.GtEngine.matrix_values(dtype)
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32}[bits.size // 4]
    return torch.from_numpy(bits.copy()).view(it).to(DEV)


def check_all(out: torch.Tensor, recs: torch.Tensor, v: int, n: int, sample_major: bool, rows_of=None, what=""):
    """Every element of `out` ((v, n), or (n, v) with sample_major) against the torch unpack, a band of rows at a time."""
    r = MP.record_size(n)
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32}[out.element_size()]
    lut = lut_for(out.dtype)
    bits = out.view(it)
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=DEV)
    rec2 = recs[: v * r].view(v, r) if rows_of is None else recs.view(-1, r)
    band = max(1, BAND_ELEMS // n)
    for a in range(0, v, band):
        b = min(v, a + band)
        rows = rec2[a:b] if rows_of is None else rec2.index_select(0, rows_of[a:b])
        codes = ((rows.reshape(b - a, r, 1) >> shifts) & 3).view(b - a, 4 * r)[:, :n]
        want = lut[codes.to(torch.int32)]
        got = bits[:, a:b].t() if sample_major else bits[a:b]
        same = got == want
        if not bool(same.all()):
            bad = torch.nonzero(~same)[0].tolist()
            raise AssertionError(f"{what}: row {a + bad[0]}, sample {bad[1]}: got {int(got[bad[0], bad[1]])}, want {int(want[bad[0], bad[1]])}")
        del codes, want, same


CONFIGS2 = (100_000, 500_000)
CHR22 = (1_103_547, 2_504)
BASIC2 = (9_200_000, 300)


@pytest.mark.parametrize("shape", [CONFIGS2, CHR22, BASIC2], ids=["configs2", "chr22", "basic2"])
def test_int8_variant_major(shape):
    v, n = shape
    recs = records_for(v, n, v * n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = eng.decode_matrix(recs, v)
        eng.wait()
        assert out.shape == (v, n) and out.is_contiguous()
        if shape == CONFIGS2:
            assert (v - 1) * n > 1 << 32 and (v - 1) * MP.record_size(n) > 1 << 32   # output and record offsets pass 4 GiB
        check_all(out, recs, v, n, False, what="variant-major int8")
    del out


@pytest.mark.parametrize("shape", [CONFIGS2, CHR22, BASIC2], ids=["configs2", "chr22", "basic2"])
def test_int8_sample_major_padded_pitch(shape):
    v, n = shape
    pitch = (v + 127) // 128 * 128
    recs = records_for(v, n, n * pitch)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = eng.decode_matrix(recs, v, sample_major=True)
        eng.wait()
        assert out.shape == (n, v) and out.stride(0) == pitch
        assert MP.auto_shape(True, True, out.data_ptr(), pitch, n) == MP.TILE
        if shape == CONFIGS2:
            assert (n - 1) * pitch > 1 << 32
        check_all(out, recs, v, n, True, what="sample-major int8, padded pitch")
    del out


def test_int8_sample_major_dense_pitch_configs2():
    v, n = CONFIGS2
    recs = records_for(v, n, n * v)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = torch.empty((n, v), dtype=torch.int8, device=DEV)
        assert v % 16 == 0 and v % 128 != 0 and MP.auto_shape(True, True, out.data_ptr(), v, n) == MP.TILE
        eng.decode_matrix(recs, v, sample_major=True, out=out)
        eng.wait()
        check_all(out, recs, v, n, True, what="sample-major int8, dense pitch")
    del out


def test_int8_sample_major_dense_odd_pitch_chr22_band():
    """The dense chr22 sample-major matrix has an odd pitch: GENERAL under AUTO.  Run and checked on the first 100 001 variants."""
    v_all, n = CHR22
    v = 100_001
    recs = records_for(v_all, n, n * v)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = torch.empty((n, v), dtype=torch.int8, device=DEV)
        assert MP.auto_shape(True, True, out.data_ptr(), v, n) == MP.GENERAL and v_all % 2 == 1
        eng.decode_matrix(recs, v, sample_major=True, out=out)
        eng.wait()
        check_all(out, recs, v, n, True, what="sample-major int8, odd pitch (GENERAL)")
    del out


def test_f32_variant_major_configs2():
    v, n = CONFIGS2
    recs = records_for(v, n, 4 * v * n)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = eng.decode_matrix(recs, v, dtype=torch.float32)
        eng.wait()
        assert out.shape == (v, n) and out.numel() * 4 + v * MP.record_size(n) > 212 * 10**9
        check_all(out, recs, v, n, False, what="variant-major f32")
    del out


def test_int8_through_a_permutation_of_all_rows_configs2():
    v, n = CONFIGS2
    recs = records_for(v, n, v * n)
    perm = torch.from_numpy(np.random.default_rng(17).permutation(v).astype(np.int32)).to(DEV)
    with pgen_rs_amd.GtEngine(n, device=0) as eng:
        out = eng.decode_matrix(recs, variant_idx=perm)
        eng.wait()
        check_all(out, recs, v, n, False, rows_of=perm.to(torch.int64), what="variant-major int8, permuted rows")
    del out
    _CACHE.clear()
    torch.cuda.empty_cache()
