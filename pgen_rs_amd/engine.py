"""Python face of the GT decode/emit engine: a thin wrapper over the C ABI (``include/pgen_hip.h``).

PyTorch is plumbing only (device buffers, streams, process groups); every byte of output is
produced by the gfx950 kernels inside ``libpgen_hip.so``.  Nothing here computes genotypes on
the CPU and nothing here touches ``oracle/``.

Reference seam: ``/root/reference/src/pfile.rs:156-192`` (``Pfile::output_vcf`` hot loop).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._capi import KERNEL_AUTO, check, lib


def variant_record_size(sample_count: int) -> int:
    """``Pfile::variant_record_size`` (src/pfile.rs:196-200) through the C ABI."""
    return int(lib.pgenhip_variant_record_size(sample_count))


def record_offset(var_idx: int, record_size: int) -> int:
    """Byte offset of record ``var_idx`` (src/pfile.rs:165, u64 — see SURVEY.md F5)."""
    return int(lib.pgenhip_record_offset(var_idx, record_size))


def parse_header(header: bytes) -> tuple[int, int]:
    """12-byte .pgen header -> (variant_count, sample_count); raises on the reference's asserts (src/pfile.rs:47,53,69)."""
    if len(header) < 12:
        raise _capi.PgenHipError(_capi.ERR_IO, "parse_header: short header")
    nv, ns = C.c_uint32(), C.c_uint32()
    check(lib.pgenhip_parse_header(bytes(header[:12]), C.byref(nv), C.byref(ns)), "pgenhip_parse_header")
    return nv.value, ns.value


def device_count() -> int:
    n = C.c_int()
    rc = lib.pgenhip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ---- variable-width storage modes: header and offset-table walk (src/pgen.rs) ---------
def vw_parse_header(header: bytes) -> "_capi.VwHeader":
    """12 header bytes of a variable-width .pgen -> ``pgenhip_vw_header`` (src/pgen.rs:21-137); raises on its asserts."""
    if len(header) < 12:
        raise _capi.PgenHipError(_capi.ERR_IO, "vw_parse_header: short header")
    h = _capi.VwHeader()
    check(lib.pgenhip_vw_parse_header(bytes(header[:12]), C.byref(h)), "pgenhip_vw_parse_header")
    return h


def vw_walk_index(h: "_capi.VwHeader", index: bytes):
    """File bytes [12, variant_records_offset) -> (record_type u8[V], record_len u32[V], record_off u64[V]) (src/pgen.rs:140-258)."""
    v = int(h.variant_count)
    types = np.zeros(max(v, 1), dtype=np.uint8)
    lens = np.zeros(max(v, 1), dtype=np.uint32)
    offs = np.zeros(max(v, 1), dtype=np.uint64)
    buf = np.frombuffer(bytes(index), dtype=np.uint8)
    check(lib.pgenhip_vw_walk_index(C.byref(h), buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size,
                                    types.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p)),
          "pgenhip_vw_walk_index")
    return types[:v], lens[:v], offs[:v]


def vw_select_uncompressed(types: np.ndarray, lens: np.ndarray, offs: np.ndarray, record_size: int,
                           variant_idx: Optional[Sequence[int]] = None) -> np.ndarray:
    """Byte offsets of the selected variants' records, all of which must be plain 2-bit records (type 0, length R);
    raises ``PgenHipError`` with status ``ERR_COMPRESSED_RECORD`` otherwise."""
    types = np.ascontiguousarray(types, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    vidx = None if variant_idx is None else np.ascontiguousarray(np.asarray(variant_idx, dtype=np.uint32))
    n = int(types.size if vidx is None else vidx.size)
    sel = np.zeros(max(n, 1), dtype=np.uint64)
    check(lib.pgenhip_vw_select_uncompressed(types.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                             int(types.size), vidx.ctypes.data_as(C.c_void_p) if vidx is not None and vidx.size else None, n,
                                             record_size, sel.ctypes.data_as(C.c_void_p)), "pgenhip_vw_select_uncompressed")
    return sel[:n]


def vcf_index_lines(data: bytes, format_col: int, last_block: bool = True, max_lines: Optional[int] = None):
    """The lines of a block of VCF body text (``pgenhip_vcf_index_lines``): ``(line_start, format_off, field_off, line_end,
    consumed)``, four uint64 arrays with one entry per line and the offset just past the last line reported.  ``field_off`` is
    the tab behind column ``format_col`` (``line_end`` for a line whose last column that is, 2**64 - 1 for a line with fewer
    columns); ``last_block``: a final line without a newline counts."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = buf.size + 1 if max_lines is None else int(max_lines)   # a line takes at least one byte
    arrs = [np.zeros(max(cap, 1), dtype=np.uint64) for _ in range(4)]
    n, consumed = C.c_uint64(), C.c_uint64()
    check(lib.pgenhip_vcf_index_lines(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, format_col, cap,
                                      _capi.VCF_LAST_BLOCK if last_block else 0, *[a.ctypes.data_as(C.c_void_p) for a in arrs],
                                      C.byref(n), C.byref(consumed)), "pgenhip_vcf_index_lines")
    return (*[a[:n.value] for a in arrs], int(consumed.value))


# pack_records' code_map for PLINK 1 .bed with ALT as A1: 00 hom A1, 01 missing, 10 het, 11 hom A2
BED_CODE_MAP = (3, 2, 0, 1)


def _ptr(t: Optional[torch.Tensor], byte_offset: int = 0) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr() + byte_offset


class _Rows(NamedTuple):
    """A checked row selection (``GtEngine._rows`` / ``_rows_at``), as ``GtEngine._entry`` passes it to the C ABI."""
    n: int          # n_variants, its default filled in
    args: tuple     # the ABI's leading row arguments: (ptr, record_stride, variant_idx ptr, n) or (base ptr, record_off ptr, n)
    suffix: str     # which twin of an entry takes them: "" or "_at"


# pair_tables / pair_r2: (mode, dtype, what an allocated result holds where no pair is written, the shape of one pair's entry)
_PAIR_TABLES = (_capi.PAIR_TABLE, torch.int32, 0, (4, 4))
_PAIR_R2 = (_capi.PAIR_R2, torch.float32, float("nan"), ())


class GtEngine:
    """One context = one device + one kept-sample list (src/pfile.rs:128 ``sam_idx_rcs``).

    ``kept_idx=None`` keeps all samples (K = N).  Launches are asynchronous on torch's current
    stream of the device (``use_torch_stream``), so torch ops and kernels are stream-ordered.
    """

    def __init__(self, sample_count: int, kept_idx: Optional[Sequence[int]] = None, device: int = 0):
        self._ctx = C.c_void_p()
        self.device = int(device)
        self.sample_count = int(sample_count)
        arr = None
        if kept_idx is not None:
            arr = np.ascontiguousarray(np.asarray(kept_idx, dtype=np.uint32))
        check(
            lib.pgenhip_create(
                C.byref(self._ctx),
                self.device,
                self.sample_count,
                arr.ctypes.data_as(C.c_void_p) if arr is not None and arr.size else None,
                int(arr.size) if arr is not None else 0,
                _capi.CREATE_KEEP_LIST if arr is not None else 0,  # an empty list is a list, not "all samples"
            ),
            "pgenhip_create",
        )
        self.kept_count = int(lib.pgenhip_kept_count(self._ctx))
        self.record_size = variant_record_size(self.sample_count)
        self.gt_row_bytes = int(lib.pgenhip_gt_row_bytes(self._ctx))
        self.torch_device = torch.device("cuda", self.device)
        self.use_torch_stream()

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            lib.pgenhip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- streams / timing -------------------------------------------------------------------
    def use_torch_stream(self) -> None:
        stream = torch.cuda.current_stream(self.torch_device)
        check(lib.pgenhip_set_stream(self._ctx, C.c_void_p(stream.cuda_stream)), "pgenhip_set_stream")

    def use_own_stream(self) -> None:
        check(lib.pgenhip_reset_stream(self._ctx), "pgenhip_reset_stream")

    def use_stream(self, stream: "torch.cuda.Stream") -> None:
        check(lib.pgenhip_set_stream(self._ctx, C.c_void_p(stream.cuda_stream)), "pgenhip_set_stream")

    def tune(self, knob: int, value: int) -> None:
        """Launch-shape knob of this context (``_capi.KNOB_*``): tests force small grids, probes A/B."""
        check(lib.pgenhip_tune(self._ctx, knob, value), "pgenhip_tune")

    def wait(self) -> None:
        check(lib.pgenhip_wait(self._ctx), "pgenhip_wait")

    def timer_start(self) -> None:
        check(lib.pgenhip_timer_start(self._ctx), "pgenhip_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(lib.pgenhip_timer_stop(self._ctx, C.byref(ms)), "pgenhip_timer_stop")
        return float(ms.value)

    # -- which rows a call reads: one contract for every method below (csrc/kernels.h, RowSource) ------------
    def _rows(self, records: torch.Tensor, record_stride: Optional[int], variant_idx: Optional[torch.Tensor],
              n_variants: Optional[int], records_offset: int, vidx_msg: Optional[str] = None) -> _Rows:
        """Checks a selection by stride or ``variant_idx`` and returns it with the defaults filled in: the record size as the stride,
        and ``variant_idx``'s length or else the rows ``records`` holds as ``n_variants``.  ``vidx_msg``: the caller's one message
        for both ``variant_idx`` refusals."""
        if record_stride is None:
            record_stride = self.record_size
        self._check_dev(records, "records")
        if variant_idx is not None:
            self._check_dev(variant_idx, "variant_idx")
            if variant_idx.dtype not in (torch.int32, torch.uint32):
                raise ValueError(vidx_msg or "variant_idx must be a 32-bit integer tensor")
        if n_variants is None:
            if variant_idx is not None:
                n_variants = variant_idx.numel()
            else:
                avail = records.numel() - records_offset
                if self.record_size == 0 or avail < self.record_size:
                    n_variants = 0
                else:
                    n_variants = (avail - self.record_size) // max(record_stride, 1) + 1
        if variant_idx is not None and variant_idx.numel() < n_variants:
            raise ValueError(vidx_msg or "variant_idx has fewer than n_variants entries")
        if n_variants and variant_idx is None:
            need_in = records_offset + (n_variants - 1) * record_stride + self.record_size
            if records.numel() < need_in:
                raise ValueError(f"records too small: {records.numel()} < {need_in}")
        return _Rows(n_variants, (_ptr(records, records_offset), record_stride, _ptr(variant_idx), n_variants), "")

    def _rows_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int], msg: Optional[str] = None) -> _Rows:
        """Checks a selection by byte offsets into ``base`` and returns it (``n_variants`` defaults to ``record_off``'s length)."""
        self._check_dev(base, "base")
        self._check_dev(record_off, "record_off")
        if record_off.dtype != torch.int64:
            raise ValueError(msg or "record_off must be an int64 tensor (u64 byte offsets)")
        if n_variants is None:
            n_variants = record_off.numel()
        if record_off.numel() < n_variants:
            raise ValueError(msg or "record_off has fewer than n_variants entries")
        return _Rows(n_variants, (_ptr(base), _ptr(record_off), n_variants), "_at")

    def _entry(self, name: str, rows: _Rows, *tail) -> None:
        """Calls the twin of ABI entry ``name`` that takes ``rows``, with the arguments behind the row arguments."""
        name += rows.suffix
        check(getattr(lib, name)(self._ctx, *rows.args, *tail), name)

    # -- what the methods below share: outputs given or allocated, checked inputs ------------------------------
    def _flat_out(self, out: Optional[torch.Tensor], dtype: torch.dtype, need: int, msg: str, *, name: str = "out", floor: int = 1,
                  fill=None) -> torch.Tensor:
        """The flat output of ``dtype`` with at least ``need`` entries: the caller's, checked (``msg``: the refusal of a wrong
        dtype or size, formatted with ``name``, ``dtype`` and ``need`` only when it is raised), or one of ``max(need, floor)``
        entries allocated here, uninitialised or holding ``fill``."""
        if out is None:
            size = max(need, floor)
            if fill is None:
                return torch.empty(size, dtype=dtype, device=self.torch_device)
            return torch.full((size,), fill, dtype=dtype, device=self.torch_device)
        self._check_dev(out, name)
        if out.dtype != dtype or out.numel() < need:
            raise ValueError(msg.format(name=name, dtype=dtype, need=need))
        return out if out.dim() == 1 else out.view(-1)   # (a view of a flat tensor is the one step here that costs a microsecond)

    def _pitched_out(self, out: Optional[torch.Tensor], n_rows: int, row_bytes: int, out_stride: Optional[int], out_offset: int):
        """A flat uint8 output that takes ``n_rows`` rows of ``row_bytes`` at pitch ``out_stride`` (default ``row_bytes``) from byte
        ``out_offset``, given or allocated: (the flat tensor, the pitch, the ``(n_rows, row_bytes)`` view of the rows)."""
        if out_stride is None:
            out_stride = row_bytes
        if out is None:
            out = torch.empty(out_offset + max(n_rows * out_stride, row_bytes, 1), dtype=torch.uint8, device=self.torch_device)
        self._check_dev(out, "out")
        if out.dtype != torch.uint8:
            raise ValueError("out must be a uint8 tensor")
        if n_rows and out.numel() < out_offset + (n_rows - 1) * out_stride + row_bytes:
            raise ValueError("out too small")
        out = out.view(-1)
        return out, out_stride, torch.as_strided(out, (n_rows, row_bytes), (out_stride, 1), out_offset)

    def _column_matrix(self, t: torch.Tensor, name: str, dtype: torch.dtype, shape_msg: str, empty_too: bool = False) -> tuple[int, int]:
        """Checks an input of shape ``(rows, C)`` or ``(rows,)``, contiguous along its columns (``empty_too``: also where it has no
        row), and returns ``(row stride, C)``; a tensor of one row has no stride of its own and gets C."""
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}")
        if t.dtype != dtype or t.dim() not in (1, 2):
            raise ValueError(shape_msg)
        n_columns = t.shape[1] if t.dim() == 2 else 1
        if t.dim() == 2 and n_columns > 1 and (empty_too or t.shape[0] > 0) and t.stride(1) != 1:
            raise ValueError(f"{name} must be contiguous along its columns")
        return int(t.stride(0) if t.shape[0] > 1 else n_columns), int(n_columns)

    def _code_values(self, code_values: torch.Tensor, n_variants: int, kind: str = "") -> None:
        self._check_dev(code_values, "code_values")
        if code_values.dtype != torch.float64 or code_values.numel() < 4 * n_variants:
            raise ValueError(f"code_values must be a {kind}float64 tensor of shape (n_variants, 4)")

    def _rank_ranges(self, a, b) -> tuple[tuple[int, int], tuple[int, int]]:
        """Two ``(begin, count)`` ranges of ranks in the kept list, default all K."""
        a = (0, self.kept_count) if a is None else (int(a[0]), int(a[1]))
        b = (0, self.kept_count) if b is None else (int(b[0]), int(b[1]))
        if min(a + b) < 0:
            raise ValueError("sample ranges are (begin, count) with begin, count >= 0")
        return a, b

    @staticmethod
    def _pair_window(n_variants: int, n_left: Optional[int], window: int) -> int:
        """``n_left`` with its default, all rows."""
        if n_left is None:
            n_left = n_variants
        if window < 1 or not 0 <= n_left <= n_variants:
            raise ValueError("need window >= 1 and 0 <= n_left <= n_variants")
        return n_left

    # -- the hot path -----------------------------------------------------------------------
    def decode_emit(
        self,
        records: torch.Tensor,
        n_variants: int,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None,
        out_stride: Optional[int] = None,
        kernel: int = KERNEL_AUTO,
        records_offset: int = 0,
        out_offset: int = 0,
    ) -> torch.Tensor:
        """GT segments of ``n_variants`` rows (src/pfile.rs:165-190); returns the uint8 output tensor.

        ``records``: uint8 CUDA tensor; row r at byte ``records_offset + r*record_stride``.
        ``variant_idx``: optional int32/uint32 CUDA tensor of row numbers (gapped kept-variant lists).
        Row j is written at byte ``out_offset + j*out_stride`` of ``out`` (dense 4K+1 by default).
        """
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset,
                          "variant_idx must be a 32-bit integer tensor with >= n_variants entries")
        return self._decode_emit(rows, out, out_stride, kernel, out_offset)

    def decode_emit_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: int, out: Optional[torch.Tensor] = None,
                       out_stride: Optional[int] = None, kernel: int = KERNEL_AUTO) -> torch.Tensor:
        """GT segments of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor): the
        uncompressed records of a variable-width .pgen staged to HBM as it lies on disk."""
        rows = self._rows_at(base, record_off, n_variants, "record_off must be an int64 tensor (u64 byte offsets) with >= n_variants entries")
        return self._decode_emit(rows, out, out_stride, kernel)

    def _decode_emit(self, rows: _Rows, out: Optional[torch.Tensor], out_stride: Optional[int], kernel: int, out_offset: int = 0) -> torch.Tensor:
        n = rows.n
        if out_stride is None:
            out_stride = self.gt_row_bytes
        if out is None:   # for no rows the twins have always differed: nothing by stride, one row's pitch by offset
            out = torch.empty(out_offset + (max(n, 1) if rows.suffix else n) * out_stride, dtype=torch.uint8, device=self.torch_device)
        self._check_dev(out, "out")
        if n:
            need_out = out_offset + (n - 1) * out_stride + self.gt_row_bytes
            if out.numel() < need_out:
                raise ValueError(f"out too small: {out.numel()} < {need_out}")
        self._entry("pgenhip_decode_emit", rows, _ptr(out, out_offset), out_stride, kernel)
        return out

    def emit_lines(
        self,
        records: torch.Tensor,
        n_variants: int,
        prefix_blob: torch.Tensor,
        prefix_off: torch.Tensor,
        line_off: torch.Tensor,
        max_prefix_bytes: int,
        out: torch.Tensor,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        kernel: int = KERNEL_AUTO,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """Complete VCF body lines (src/pfile.rs:156-192): prefix + GT segment + newline per variant."""
        if record_stride is None:
            record_stride = self.record_size
        for t, name in ((records, "records"), (prefix_blob, "prefix_blob"), (prefix_off, "prefix_off"), (line_off, "line_off"), (out, "out")):
            self._check_dev(t, name)
        if prefix_off.dtype != torch.int64 or line_off.dtype != torch.int64:
            raise ValueError("prefix_off/line_off must be int64 tensors (u64 offsets)")
        if prefix_off.numel() < n_variants + 1 or line_off.numel() < n_variants + 1:
            raise ValueError("offset arrays need n_variants+1 entries")
        check(
            lib.pgenhip_emit_lines(
                self._ctx,
                _ptr(records, records_offset),
                record_stride,
                _ptr(variant_idx),
                n_variants,
                _ptr(prefix_blob),
                _ptr(prefix_off),
                _ptr(line_off),
                max_prefix_bytes,
                _ptr(out),
                kernel,
            ),
            "pgenhip_emit_lines",
        )
        return out

    def genotype_counts(
        self,
        records: torch.Tensor,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        n_variants: Optional[int] = None,
        out: Optional[torch.Tensor] = None,
        kernel: int = _capi.COUNT_AUTO,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """Per-variant genotype counts of the kept samples: an ``(n, 4)`` int32 CUDA tensor holding the u32 counts of codes 0-3
        (hom-ref, het, hom-alt, missing) of row j — the GT fields ``decode_emit`` would write for that row, counted.

        Rows are selected as in ``decode_emit``: row j's record is at byte ``records_offset + r*record_stride`` of ``records``,
        ``r = variant_idx[j]`` or ``j``.  ``n_variants`` defaults to ``variant_idx``'s length, else to the rows ``records`` holds.
        ``out``: optional int32 CUDA tensor of >= 4n entries (written from its first element; nothing else is touched)."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._counts("pgenhip_genotype_counts", rows, rows.n, out, kernel)

    def genotype_counts_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None,
                           out: Optional[torch.Tensor] = None, kernel: int = _capi.COUNT_AUTO) -> torch.Tensor:
        """``genotype_counts`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        rows = self._rows_at(base, record_off, n_variants)
        return self._counts("pgenhip_genotype_counts", rows, rows.n, out, kernel)

    def _counts(self, name: str, rows: _Rows, n: int, out: Optional[torch.Tensor], kernel: int, accumulate: bool = False) -> torch.Tensor:
        """Both count entries: an ``(n, 4)`` int32 result, n the selected rows or the kept samples."""
        out = self._flat_out(out, torch.int32, 4 * n, "out must be an int32 tensor with >= 4 * n_variants entries", floor=4,
                             fill=0 if accumulate else None)
        self._entry(name, rows, _ptr(out), kernel | (_capi.SCOUNT_ACCUMULATE if accumulate else 0))
        return out[: 4 * n].view(n, 4)

    def sample_counts(
        self,
        records: torch.Tensor,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        n_variants: Optional[int] = None,
        out: Optional[torch.Tensor] = None,
        kernel: int = _capi.SCOUNT_AUTO,
        accumulate: bool = False,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """Per-sample genotype counts over the selected rows: a ``(K, 4)`` int32 CUDA tensor holding, for kept sample k, the u32
        numbers of rows in which it has code 0-3 (hom-ref, het, hom-alt, missing).

        Rows are selected as in ``genotype_counts`` (a row named twice in ``variant_idx`` counts twice).  ``out``: optional int32
        CUDA tensor of >= 4K entries (written from its first element; nothing else is touched).  ``accumulate``: add to what
        ``out`` holds instead of overwriting it."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._counts("pgenhip_sample_counts", rows, self.kept_count, out, kernel, accumulate)

    def sample_counts_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None,
                         out: Optional[torch.Tensor] = None, kernel: int = _capi.SCOUNT_AUTO, accumulate: bool = False) -> torch.Tensor:
        """``sample_counts`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        rows = self._rows_at(base, record_off, n_variants)
        return self._counts("pgenhip_sample_counts", rows, self.kept_count, out, kernel, accumulate)

    # -- per-sample weighted dosage sums (polygenic scores) --------------------------------------
    def sample_scores(
        self,
        records: torch.Tensor,
        weights: torch.Tensor,
        *,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        miss: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None,
        accumulate: bool = False,
        flags: int = 0,
        n_variants: Optional[int] = None,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """Per-sample weighted dosage sums over the selected rows: a ``(K, C)`` float64 CUDA tensor,
        ``S[k, c] = sum_j float64(weights[j, c]) * D(j, k)`` with D = 0, 1, 2 for codes 0-2 and ``miss[j]`` (0 without ``miss``)
        for a missing call.  Terms are exact in FP64 and accumulated in FP64 in no fixed order (include/pgen_hip.h).

        ``weights``: float32 CUDA tensor of shape (V, C) or (V,), C <= 8, contiguous along the columns; its row stride is taken
        from the tensor.  ``miss``: float32 CUDA tensor of V entries, or None.  Both are indexed by the row's position in the
        selection.  Rows are selected as in ``sample_counts``; ``n_variants`` defaults to ``weights``' rows.  ``out``: optional
        float64 CUDA tensor of >= K * C entries (written from its first element; nothing else is touched).  ``accumulate``:
        add to what ``out`` holds instead of overwriting it.  ``flags``: a forced shape (``_capi.SCORE_*``)."""
        return self._sample_scores(lambda n: self._rows(records, record_stride, variant_idx, n, records_offset), weights, miss, out,
                                   accumulate, flags, n_variants)

    def sample_scores_at(self, base: torch.Tensor, record_off: torch.Tensor, weights: torch.Tensor, *, miss: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, accumulate: bool = False, flags: int = 0,
                         n_variants: Optional[int] = None) -> torch.Tensor:
        """``sample_scores`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._sample_scores(lambda n: self._rows_at(base, record_off, n), weights, miss, out, accumulate, flags, n_variants)

    def _sample_scores(self, select, weights: torch.Tensor, miss: Optional[torch.Tensor], out: Optional[torch.Tensor], accumulate: bool,
                       flags: int, n_variants: Optional[int]) -> torch.Tensor:
        """``select(n_variants)`` checks the rows: they come after ``weights``, whose row count is the default of ``n_variants``."""
        w_stride, n_columns = self._column_matrix(weights, "weights", torch.float32, "weights must be a float32 tensor of shape (V, C) or (V,)",
                                                  empty_too=True)
        if n_variants is None:
            n_variants = weights.shape[0]
        if weights.shape[0] < n_variants:
            raise ValueError("weights has fewer than n_variants rows")
        if miss is not None:
            self._check_dev(miss, "miss")
            if miss.dtype != torch.float32 or miss.numel() < n_variants:
                raise ValueError("miss must be a float32 tensor with >= n_variants entries")
        rows = select(int(n_variants))
        need = self.kept_count * n_columns
        out = self._flat_out(out, torch.float64, need, "out must be a float64 tensor with >= K * C entries", fill=0 if accumulate else None)
        self._entry("pgenhip_sample_scores", rows, _ptr(weights), w_stride, n_columns, _ptr(miss), _ptr(out),
                    flags | (_capi.SCORE_ACCUMULATE if accumulate else 0))
        return out[:need].view(self.kept_count, n_columns)

    # -- per-variant sums of per-sample values by genotype code -----------------------------------
    def variant_sums(
        self,
        records: torch.Tensor,
        values: torch.Tensor,
        *,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None,
        flags: int = 0,
        n_variants: Optional[int] = None,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """Per-variant sums of per-sample values, split by genotype code: a ``(n_variants, C, 4)`` float64 CUDA tensor,
        ``S[j, c, x] = sum of values[k, c] over the kept samples k whose code in row j is x`` (0 hom-ref, 1 het, 2 hom-alt,
        3 missing).  Every addition is FP64, in no fixed order (include/pgen_hip.h).

        ``values``: float64 CUDA tensor of shape (K, C) or (K,), C <= 16, contiguous along the columns; its row stride is taken
        from the tensor and row k belongs to the k-th kept sample.  Rows are selected as in ``genotype_counts``.  ``out``: optional
        float64 CUDA tensor of >= n_variants * C * 4 entries (written from its first element; nothing else is touched).
        ``flags``: a forced shape (``_capi.VSUM_*``)."""
        return self._variant_sums(lambda: self._rows(records, record_stride, variant_idx, n_variants, records_offset), values, out, flags)

    def variant_sums_at(self, base: torch.Tensor, record_off: torch.Tensor, values: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                        flags: int = 0, n_variants: Optional[int] = None) -> torch.Tensor:
        """``variant_sums`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._variant_sums(lambda: self._rows_at(base, record_off, n_variants), values, out, flags)

    def _variant_sums(self, select, values: torch.Tensor, out: Optional[torch.Tensor], flags: int) -> torch.Tensor:
        """``select()`` checks the rows, after ``values`` as ever."""
        v_stride, n_columns = self._column_matrix(values, "values", torch.float64, "values must be a float64 tensor of shape (K, C) or (K,)")
        if values.shape[0] < self.kept_count:
            raise ValueError("values has fewer than K rows")
        rows = select()
        need = rows.n * n_columns * 4
        out = self._flat_out(out, torch.float64, need, "out must be a float64 tensor with >= n_variants * C * 4 entries")
        self._entry("pgenhip_variant_sums", rows, _ptr(values), v_stride, n_columns, _ptr(out), flags)
        return out[:need].view(rows.n, n_columns, 4)

    # -- per-variant logistic regression ----------------------------------------------------------
    def variant_logistic(
        self,
        records: torch.Tensor,
        code_values: torch.Tensor,
        design: torch.Tensor,
        y: torch.Tensor,
        start: torch.Tensor,
        *,
        max_iter: int = 25,
        tol: float = 1e-9,
        record_stride: Optional[int] = None,
        variant_idx: Optional[torch.Tensor] = None,
        coef: Optional[torch.Tensor] = None,
        se: Optional[torch.Tensor] = None,
        status: Optional[torch.Tensor] = None,
        flags: int = 0,
        n_variants: Optional[int] = None,
        records_offset: int = 0,
    ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Per-variant logistic regression of ``y`` on ``[design, g]``, ``g = code_values[j, code]``: the Newton iteration that
        include/pgen_hip.h fixes (``pgenhip_variant_logistic``).  Returns ``(coef, se, status)``: a ``(n_variants, n_cov + 1)``
        float64 tensor (the covariates' coefficients, then the genotype's), the genotype's standard errors ``(n_variants,)``
        float64 (NaN unless converged) and the status words ``(n_variants,)`` int32 (evaluations in the low 8 bits and one of
        ``_capi.LOGIT_CONVERGED`` / ``NOT_CONVERGED`` / ``SINGULAR``).

        ``code_values``: float64 CUDA tensor ``(n_variants, 4)``, contiguous; a NaN entry leaves the samples with that code out of
        the row's fit.  ``design``: float64 CUDA tensor ``(K, n_cov)`` or ``(K,)``, n_cov <= 15, contiguous along the columns (its
        row stride is taken from the tensor; the intercept is a column of it).  ``y``: float64, K values in [0, 1].  ``start``:
        float64, n_cov coefficients of the null model.  Rows are selected as in ``variant_sums``.  ``coef`` / ``se`` / ``status``:
        optional outputs (written from their first element, ``coef`` with rows of n_cov + 1).  ``flags``: a forced shape
        (``_capi.LOGIT_*``)."""
        return self._variant_logistic(lambda: self._rows(records, record_stride, variant_idx, n_variants, records_offset), code_values, design, y,
                                      start, max_iter, tol, coef, se, status, flags)

    def variant_logistic_at(self, base: torch.Tensor, record_off: torch.Tensor, code_values: torch.Tensor, design: torch.Tensor,
                            y: torch.Tensor, start: torch.Tensor, *, max_iter: int = 25, tol: float = 1e-9,
                            coef: Optional[torch.Tensor] = None, se: Optional[torch.Tensor] = None,
                            status: Optional[torch.Tensor] = None, flags: int = 0,
                            n_variants: Optional[int] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``variant_logistic`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._variant_logistic(lambda: self._rows_at(base, record_off, n_variants), code_values, design, y, start, max_iter, tol,
                                      coef, se, status, flags)

    def _variant_logistic(self, select, code_values: torch.Tensor, design: torch.Tensor, y: torch.Tensor, start: torch.Tensor,
                          max_iter: int, tol: float, coef: Optional[torch.Tensor], se: Optional[torch.Tensor],
                          status: Optional[torch.Tensor], flags: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``select()`` checks the rows, after the design, ``y`` and ``start`` as ever."""
        for t, name in ((design, "design"), (y, "y"), (start, "start")):
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name} must live on cuda:{self.device}")
            if t.dtype != torch.float64:
                raise ValueError(f"{name} must be a float64 tensor")
        x_stride, n_cov = self._column_matrix(design, "design", torch.float64, "design must be a float64 tensor of shape (K, n_cov) or (K,)")
        if design.shape[0] < self.kept_count or y.numel() < self.kept_count:
            raise ValueError("design or y has fewer than K rows")
        if not y.is_contiguous() or not start.is_contiguous() or start.numel() < n_cov:
            raise ValueError("y and start must be contiguous, start with >= n_cov entries")
        rows = select()
        n = rows.n
        self._code_values(code_values, n, "contiguous ")
        coef, se, status = (
            self._flat_out(t, dtype, need, "{name} must be a contiguous {dtype} tensor with >= {need} entries", name=name)
            for t, name, dtype, need in ((coef, "coef", torch.float64, n * (n_cov + 1)), (se, "se", torch.float64, n),
                                         (status, "status", torch.int32, n)))
        self._entry("pgenhip_variant_logistic", rows, _ptr(code_values), _ptr(design), x_stride, n_cov, _ptr(y), _ptr(start), max_iter,
                    tol, _ptr(coef), n_cov + 1, _ptr(se), _ptr(status), flags)
        return coef[: n * (n_cov + 1)].view(n, n_cov + 1), se[:n], status[:n]

    # -- numeric genotype matrix ---------------------------------------------------------------
    def decode_matrix(
        self,
        records: torch.Tensor,
        n_variants: Optional[int] = None,
        *,
        dtype: torch.dtype = torch.int8,
        sample_major: bool = False,
        values=None,
        out: Optional[torch.Tensor] = None,
        variant_idx: Optional[torch.Tensor] = None,
        record_stride: Optional[int] = None,
        kernel: int = _capi.MATRIX_AUTO,
        records_offset: int = 0,
    ) -> torch.Tensor:
        """The genotypes as numbers: a ``(V, K)`` tensor (``(K, V)`` with ``sample_major``) of ``dtype`` (int8, uint8, int16, int32,
        float16, bfloat16, float32) whose element for row j and kept sample k is ``values[code]``: the GT field ``decode_emit``
        prints there, mapped through a four-entry table.

        Rows are selected as in ``decode_emit`` (``variant_idx`` / ``record_stride``; ``n_variants`` defaults as in
        ``genotype_counts``).  ``values``: four numbers (or a 4-element tensor / array of ``dtype``) for codes 0-3, default 0, 1, 2
        and -1 for signed integers, all bits set for unsigned ones, NaN for floating dtypes.  ``out``: any 2-D CUDA tensor of the
        result's shape and dtype with unit stride in its last dimension (its row stride may be padded; the padding is not touched).
        Without ``out`` the variant-major result is contiguous; the sample-major result is a ``[:, :V]`` view of rows allocated at
        a pitch rounded up to 128 bytes, so that the transpose kernel stores whole lines: ``.contiguous()`` is the caller's choice
        and cost."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._decode_matrix(rows, dtype, sample_major, values, out, kernel)

    def decode_matrix_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None, *,
                         dtype: torch.dtype = torch.int8, sample_major: bool = False, values=None,
                         out: Optional[torch.Tensor] = None, kernel: int = _capi.MATRIX_AUTO) -> torch.Tensor:
        """``decode_matrix`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._decode_matrix(self._rows_at(base, record_off, n_variants), dtype, sample_major, values, out, kernel)

    def _decode_matrix(self, rows: _Rows, dtype: torch.dtype, sample_major: bool, values, out: Optional[torch.Tensor], kernel: int) -> torch.Tensor:
        out, res, stride, tab = self._matrix_out(out, rows.n, dtype, sample_major, values)
        self._entry("pgenhip_decode_matrix", rows, out.data_ptr(), stride, out.element_size(), tab.ctypes.data_as(C.c_void_p),
                    kernel | (_capi.MATRIX_SAMPLE_MAJOR if sample_major else 0))
        return res

    # -- packed records of the kept samples -----------------------------------------------------
    @property
    def packed_record_size(self) -> int:
        """``ceil(K / 4)``: bytes of one packed record of the kept samples."""
        return int(lib.pgenhip_packed_record_size(self._ctx))

    def pack_records(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, *, out_stride: Optional[int] = None, code_map=None,
                     shape: int = _capi.PACK_AUTO, n_variants: Optional[int] = None, records_offset: int = 0,
                     out_offset: int = 0) -> torch.Tensor:
        """The selection written back as records: a ``(n_variants, R_K)`` uint8 view whose row j is the mode-0x02 record of the K
        kept samples of selected row j (kept sample k in byte k/4, bits 2*(k%4)), pad bits zero; behind a 12-byte header the rows are
        a .pgen of the subset.

        Rows are selected as in ``decode_emit`` (``n_variants`` defaults as in ``genotype_counts``).  ``code_map``: four codes
        0-3 written for input codes 0-3 (``BED_CODE_MAP`` for PLINK 1 .bed), default the identity.  ``out``: a flat uint8 CUDA
        tensor; row j goes to byte ``out_offset + j*out_stride`` (default stride ``R_K``) and nothing else is touched.  The result
        is a view of ``out`` with row pitch ``out_stride``."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._pack_records(rows, out, out_stride, out_offset, code_map, shape)

    def pack_records_at(self, base: torch.Tensor, record_off: torch.Tensor, out: Optional[torch.Tensor] = None, *,
                        out_stride: Optional[int] = None, code_map=None, shape: int = _capi.PACK_AUTO,
                        n_variants: Optional[int] = None, out_offset: int = 0) -> torch.Tensor:
        """``pack_records`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._pack_records(self._rows_at(base, record_off, n_variants), out, out_stride, out_offset, code_map, shape)

    def _pack_records(self, rows: _Rows, out: Optional[torch.Tensor], out_stride: Optional[int], out_offset: int, code_map,
                      shape: int) -> torch.Tensor:
        out, out_stride, view = self._pitched_out(out, rows.n, self.packed_record_size, out_stride, out_offset)
        cmap = None
        if code_map is not None:
            vals = [int(v) for v in code_map]
            if len(vals) != 4 or any(not 0 <= v <= 255 for v in vals):
                raise ValueError("code_map must hold four codes (for input codes 0, 1, 2, 3)")
            cmap = (C.c_uint8 * 4)(*vals)
        self._entry("pgenhip_pack_records", rows, _ptr(out, out_offset), out_stride, cmap, shape)
        return view

    # -- sample-wise join of records --------------------------------------------------------------
    def join_records(self, parts, n_variants: Optional[int] = None, *, out: Optional[torch.Tensor] = None,
                     out_stride: Optional[int] = None, out_offset: int = 0, shape: int = _capi.JOIN_AUTO) -> torch.Tensor:
        """Several filesets' samples side by side: a ``(n_variants, R)`` uint8 view whose row j is the mode-0x02 record of the
        context's N samples, the samples of part 0 first, then part 1, and so on; pad bits zero.

        ``parts``: a sequence of ``(base, record_off, sample_count, flip_or_None)``, at most ``_capi.JOIN_MAX_PARTS`` of them, whose
        sample counts add up to N.  ``base``: a uint8 CUDA tensor; ``record_off``: an int64 CUDA tensor of ``n_variants`` byte offsets
        into it, ``-1`` where the part has no record for the row (its samples get code 3); ``flip``: a uint8 CUDA tensor of
        ``n_variants`` bytes, nonzero where the part's codes 0 and 2 are exchanged.  A part of 0 samples adds nothing.
        ``n_variants`` defaults to the shortest ``record_off``.  ``out``: a flat uint8 CUDA tensor; row j goes to byte
        ``out_offset + j*out_stride`` (default stride R) and nothing else is touched.  The context must keep all samples."""
        parts = list(parts)
        if n_variants is None:
            n_variants = min((p[1].numel() for p in parts), default=0)
        table = (_capi.JoinPart * max(len(parts), 1))()
        for i, (base, record_off, count, flip) in enumerate(parts):
            self._rows_at(base, record_off, n_variants)
            if base.dtype != torch.uint8:
                raise ValueError("base must be a uint8 tensor")
            if flip is not None:
                self._check_dev(flip, "flip")
                if flip.dtype != torch.uint8 or flip.numel() < n_variants:
                    raise ValueError("flip must be a uint8 tensor of n_variants entries")
            table[i] = _capi.JoinPart(_ptr(base), _ptr(record_off), _ptr(flip), int(count), 0)
        out, out_stride, view = self._pitched_out(out, n_variants, self.record_size, out_stride, out_offset)
        check(lib.pgenhip_join_records(self._ctx, table, len(parts), n_variants, _ptr(out, out_offset), out_stride, shape),
              "pgenhip_join_records")
        return view

    # -- GT text to records ---------------------------------------------------------------------
    def parse_gt(self, text: torch.Tensor, field_off: torch.Tensor, line_end: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                 out_stride: Optional[int] = None, out_offset: int = 0, shape: int = _capi.PARSE_AUTO, text_offset: int = 0,
                 text_len: Optional[int] = None, line_flags: Optional[torch.Tensor] = None,
                 n_lines: Optional[int] = None) -> tuple[torch.Tensor, torch.Tensor]:
        """The inverse of ``decode_emit``: ``(records, line_flags)``, a ``(n_lines, R)`` uint8 view whose row j is the mode-0x02
        record of the N samples of line j's fields (pad bits zero), and an int32 tensor of the lines' ``_capi.PARSE_*`` flag bits.

        ``text``: a flat uint8 CUDA tensor; the library reads bytes ``[text_offset, text_offset + text_len)`` of it and nothing
        else (default: to its end), and ``field_off`` / ``line_end`` (int64 CUDA tensors: the tab in front of sample 0's field, and
        one past the last field) count from ``text_offset``.  ``out``: a flat uint8 CUDA tensor; row j goes to byte
        ``out_offset + j*out_stride`` (default stride R) and nothing else is touched.  ``line_flags``: an int32 CUDA tensor of
        ``n_lines`` words to write into.  The context must keep all samples."""
        for t, name in ((text, "text"), (field_off, "field_off"), (line_end, "line_end")):
            self._check_dev(t, name)
        if text.dtype != torch.uint8:
            raise ValueError("text must be a uint8 tensor")
        if field_off.dtype not in (torch.int64, torch.uint64) or line_end.dtype not in (torch.int64, torch.uint64):
            raise ValueError("field_off and line_end must be 64-bit integer tensors")
        if n_lines is None:
            n_lines = field_off.numel()
        if field_off.numel() < n_lines or line_end.numel() < n_lines:
            raise ValueError("field_off or line_end has fewer than n_lines entries")
        if text_len is None:
            text_len = text.numel() - text_offset
        if text_offset < 0 or text_len < 0 or text_offset + text_len > text.numel():
            raise ValueError("text_offset / text_len lie outside text")
        out, out_stride, view = self._pitched_out(out, n_lines, self.record_size, out_stride, out_offset)
        if line_flags is None:
            line_flags = torch.empty(max(n_lines, 1), dtype=torch.int32, device=self.torch_device)
        self._check_dev(line_flags, "line_flags")
        if line_flags.dtype not in (torch.int32, torch.uint32) or line_flags.numel() < n_lines:
            raise ValueError("line_flags must be a 32-bit integer tensor of n_lines entries")
        check(lib.pgenhip_parse_gt(self._ctx, _ptr(text, text_offset), text_len, _ptr(field_off), _ptr(line_end), n_lines,
                                   _ptr(out, out_offset), out_stride, _ptr(line_flags), shape), "pgenhip_parse_gt")
        return view, line_flags[:n_lines]

    # -- windowed pairwise tables / r^2 ---------------------------------------------------------
    def pair_tables(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                    n_variants: Optional[int] = None, *, n_left: Optional[int] = None, window: int,
                    out: Optional[torch.Tensor] = None, records_offset: int = 0) -> torch.Tensor:
        """Joint genotype tables of the row pairs inside a sliding window: an int32 ``(n_left, W, 4, 4)`` CUDA tensor whose entry
        ``[i, d - 1, a, b]`` is the u32 number of kept samples with code ``a`` in row i and code ``b`` in row i + d (codes 0-3:
        hom-ref, het, hom-alt, missing), for ``1 <= d <= W`` and ``i + d < n_variants``.

        Rows are selected as in ``genotype_counts``.  ``n_left`` (default: all rows) is how many leading rows own pairs, so blocks
        that overlap by ``window`` rows compute no pair twice.  Entries with ``i + d >= n_variants`` are NOT written by the
        library: they keep what the buffer held.  Without ``out`` the result is allocated with zeros, so that ragged end reads as
        empty tables; a caller-supplied ``out`` (int32, >= 16 * n_left * W entries, 16-byte aligned) is used as given."""
        return self._pair_stats(self._rows(records, record_stride, variant_idx, n_variants, records_offset), n_left, window, out, *_PAIR_TABLES)

    def pair_tables_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None, *,
                       n_left: Optional[int] = None, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pair_tables`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._pair_stats(self._rows_at(base, record_off, n_variants), n_left, window, out, *_PAIR_TABLES)

    def pair_r2(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                n_variants: Optional[int] = None, *, n_left: Optional[int] = None, window: int,
                out: Optional[torch.Tensor] = None, records_offset: int = 0) -> torch.Tensor:
        """Unphased genotype r^2 of the same pairs: a float32 ``(n_left, W)`` CUDA tensor, entry ``[i, d - 1]`` for rows i and
        i + d, computed from the pair's table over the samples called in both rows; NaN where a row is monomorphic among them (or
        none is).  Entries with ``i + d >= n_variants`` are not written: NaN in a result allocated here, untouched in ``out``
        (float32, >= n_left * W entries)."""
        return self._pair_stats(self._rows(records, record_stride, variant_idx, n_variants, records_offset), n_left, window, out, *_PAIR_R2)

    def pair_r2_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None, *,
                   n_left: Optional[int] = None, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pair_r2`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._pair_stats(self._rows_at(base, record_off, n_variants), n_left, window, out, *_PAIR_R2)

    def _pair_stats(self, rows: _Rows, n_left: Optional[int], window: int, out: Optional[torch.Tensor], mode: int, dtype: torch.dtype,
                    fill, per_pair: tuple) -> torch.Tensor:
        """``mode``'s result: ``per_pair`` entries of ``dtype`` for every pair, ``fill`` where the library writes none."""
        n_left = self._pair_window(rows.n, n_left, window)
        need = n_left * window * math.prod(per_pair)
        out = self._flat_out(out, dtype, need, "out must be a {dtype} tensor with >= {need} entries", floor=4, fill=fill)
        self._entry("pgenhip_pair_stats", rows, n_left, window, _ptr(out), mode)
        return out[:need].view(n_left, window, *per_pair)

    # -- LD pruning: one bit per pair, the greedy independent set -------------------------------------
    def pair_mask(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                  n_variants: Optional[int] = None, *, n_left: Optional[int] = None, window: int, min_r2: float,
                  key: Optional[torch.Tensor] = None, max_span: int = 0, fwd: Optional[torch.Tensor] = None,
                  bwd: Optional[torch.Tensor] = None, want_bwd: bool = True, mask_stride: Optional[int] = None,
                  records_offset: int = 0) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
        """One bit per pair of ``pair_r2``'s pairs: ``(fwd, bwd)``, int32 ``(n_variants, mask_stride)`` CUDA tensors.  Pair
        (i, j = i + d) is an edge iff its r^2 (``pair_r2``'s float32) is ``> min_r2`` and, with ``key`` (int64 CUDA tensor, one u64
        per row), ``(key[j] - key[i]) mod 2^64 <= max_span``; bit ``(d - 1) % 32`` of word ``(d - 1) // 32`` of ``fwd``'s row i and
        of ``bwd``'s row j is then set.  The call only ORs bits in: masks that are given (int32, ``mask_stride`` words per row,
        default ``ceil(window / 32)``) keep what they hold, masks allocated here start as zeros.  ``want_bwd=False`` without
        ``bwd`` leaves the backward mask out (``None``)."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._pair_mask(rows, n_left, window, min_r2, key, max_span, fwd, bwd, want_bwd, mask_stride)

    def pair_mask_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None, *,
                     n_left: Optional[int] = None, window: int, min_r2: float, key: Optional[torch.Tensor] = None, max_span: int = 0,
                     fwd: Optional[torch.Tensor] = None, bwd: Optional[torch.Tensor] = None, want_bwd: bool = True,
                     mask_stride: Optional[int] = None) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``pair_mask`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        rows = self._rows_at(base, record_off, n_variants)
        return self._pair_mask(rows, n_left, window, min_r2, key, max_span, fwd, bwd, want_bwd, mask_stride)

    def _pair_mask(self, rows: _Rows, n_left: Optional[int], window: int, min_r2: float, key: Optional[torch.Tensor], max_span: int,
                   fwd: Optional[torch.Tensor], bwd: Optional[torch.Tensor], want_bwd: bool,
                   mask_stride: Optional[int]) -> tuple[torch.Tensor, Optional[torch.Tensor]]:
        n = rows.n
        n_left = self._pair_window(n, n_left, window)
        words = (window + 31) // 32
        if mask_stride is None:
            mask_stride = words
        if mask_stride < words:
            raise ValueError(f"mask_stride must be >= ceil(window / 32) = {words}")
        if key is not None:
            self._check_dev(key, "key")
            if key.dtype != torch.int64 or key.numel() < n:
                raise ValueError("key must be an int64 tensor (u64 keys) with >= n_variants entries")
        masks, need = [], n * mask_stride
        for name, m, want in (("fwd", fwd, True), ("bwd", bwd, want_bwd)):
            if m is not None:     # a given mask is checked like a flat output and returned as it came, in its own shape
                self._flat_out(m, torch.int32, need, "{name} must be an int32 tensor with >= n_variants * mask_stride = {need} entries", name=name)
            elif want:
                m = torch.zeros((n, mask_stride), dtype=torch.int32, device=self.torch_device)
            masks.append(m)
        fwd, bwd = masks
        self._entry("pgenhip_pair_mask", rows, n_left, window, min_r2, _ptr(key), max_span, _ptr(fwd), _ptr(bwd), mask_stride, 0)
        return fwd, bwd

    def prune_resolve(self, fwd: torch.Tensor, bwd: torch.Tensor, window: int, priority: Optional[torch.Tensor] = None,
                      state: Optional[torch.Tensor] = None, shape: int = _capi.PRUNE_AUTO, max_calls: Optional[int] = None,
                      *, n_rows: Optional[int] = None, mask_stride: Optional[int] = None, on_call=None) -> tuple[torch.Tensor, int]:
        """The priority-greedy independent set of the graph two ``pair_mask`` masks hold: ``(state, calls)``, ``state`` a uint8
        CUDA tensor of ``n_rows`` bytes (1 kept, 2 removed).  Row u beats v iff ``priority[u] > priority[v]`` (int32 tensor holding
        u32 values; ``None``: all equal) or they are equal and u < v; a row is kept iff none of its neighbours that beat it is kept.
        Rows whose byte in a given ``state`` is already 1 or 2 keep it.  Runs ``pgenhip_prune_resolve`` and reads its counter back
        until no row is undecided; ``max_calls`` (default ``n_rows``) bounds the loop, and a loop that reaches it raises.
        ``on_call(calls, undecided)`` is called after every call (tests watch the intermediate states through it)."""
        for name, m in (("fwd", fwd), ("bwd", bwd)):
            self._check_dev(m, name)
            if m.dtype != torch.int32:
                raise ValueError(f"{name} must be an int32 tensor")
        if n_rows is None:
            n_rows = fwd.shape[0] if fwd.dim() == 2 else (state.numel() if state is not None else 0)
        if mask_stride is None:
            mask_stride = fwd.shape[1] if fwd.dim() == 2 else (window + 31) // 32
        if priority is not None:
            self._check_dev(priority, "priority")
            if priority.dtype not in (torch.int32, torch.uint32) or priority.numel() < n_rows:
                raise ValueError("priority must be a 32-bit integer tensor with >= n_rows entries")
        if state is None:
            state = torch.zeros(max(n_rows, 1), dtype=torch.uint8, device=self.torch_device)[:n_rows]
        else:
            self._check_dev(state, "state")
            if state.dtype != torch.uint8 or state.numel() < n_rows:
                raise ValueError("state must be a uint8 tensor with >= n_rows entries")
        counter = torch.zeros(1, dtype=torch.int64, device=self.torch_device)
        limit = max(n_rows, 1) if max_calls is None else max_calls
        calls = 0
        while True:
            check(lib.pgenhip_prune_resolve(self._ctx, _ptr(fwd), _ptr(bwd), mask_stride, window, n_rows, _ptr(priority), _ptr(state),
                                            _ptr(counter), shape), "pgenhip_prune_resolve")
            calls += 1
            self.wait()                  # the ctx stream, whichever it is
            left = int(counter.item())
            if on_call is not None:
                on_call(calls, left)
            if left == 0:
                return state, calls
            if calls >= limit:
                raise RuntimeError(f"prune_resolve: {left} rows undecided after {calls} calls")

    # -- pairwise sample tables ------------------------------------------------------------------
    def sample_pair_tables(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                           n_variants: Optional[int] = None, *, a: Optional[tuple[int, int]] = None, b: Optional[tuple[int, int]] = None,
                           out: Optional[torch.Tensor] = None, accumulate: bool = False, kernel: int = _capi.SPAIR_AUTO,
                           records_offset: int = 0) -> torch.Tensor:
        """Joint genotype tables of pairs of kept samples over the selected rows: an int32 ``(a_count, b_count, 4, 4)`` CUDA view
        whose entry ``[i, l, x, y]`` is the u32 number of rows in which the sample of rank ``a_begin + i`` has code ``x`` and the
        sample of rank ``b_begin + l`` has code ``y`` (codes 0-3: hom-ref, het, hom-alt, missing).

        ``a``, ``b``: ``(begin, count)`` ranges of ranks in the kept list (default: all K).  Rows are selected as in
        ``sample_counts``.  ``out``: optional int32 CUDA tensor of >= 16 * a_count * b_count entries, 16-byte aligned (written from
        its first element; nothing else is touched).  ``accumulate``: add to what ``out`` holds instead of overwriting it.
        ``kernel``: a forced shape (``_capi.SPAIR_*``)."""
        return self._sample_pair_tables(self._rows(records, record_stride, variant_idx, n_variants, records_offset), a, b, out, accumulate, kernel)

    def sample_pair_tables_at(self, base: torch.Tensor, record_off: torch.Tensor, n_variants: Optional[int] = None, *,
                              a: Optional[tuple[int, int]] = None, b: Optional[tuple[int, int]] = None,
                              out: Optional[torch.Tensor] = None, accumulate: bool = False,
                              kernel: int = _capi.SPAIR_AUTO) -> torch.Tensor:
        """``sample_pair_tables`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        return self._sample_pair_tables(self._rows_at(base, record_off, n_variants), a, b, out, accumulate, kernel)

    def _sample_pair_tables(self, rows: _Rows, a, b, out: Optional[torch.Tensor], accumulate: bool, kernel: int) -> torch.Tensor:
        a, b = self._rank_ranges(a, b)
        need = 16 * a[1] * b[1]
        out = self._flat_out(out, torch.int32, need, "out must be an int32 tensor with >= {need} entries", floor=4,
                             fill=0 if accumulate else None)
        self._entry("pgenhip_sample_pair_stats", rows, *a, *b, _ptr(out), kernel | (_capi.SPAIR_ACCUMULATE if accumulate else 0))
        return out[:need].view(a[1], b[1], 4, 4)

    # -- sample Gram matrix -------------------------------------------------------------------------
    def sample_gram(self, records: torch.Tensor, record_stride: Optional[int] = None, variant_idx: Optional[torch.Tensor] = None,
                    n_variants: Optional[int] = None, *, code_values: torch.Tensor, a: Optional[tuple[int, int]] = None,
                    b: Optional[tuple[int, int]] = None, out: Optional[torch.Tensor] = None, out_stride: Optional[int] = None,
                    accumulate: bool = False, kernel: int = _capi.GRAM_AUTO, records_offset: int = 0) -> torch.Tensor:
        """Weighted cross-products of pairs of kept samples over the selected rows: a float64 ``(a_count, b_count)`` CUDA view whose
        entry ``[i, l]`` is the FP64 sum over the rows j of ``code_values[j, x] * code_values[j, y]``, x and y the codes of the
        samples of rank ``a_begin + i`` and ``b_begin + l`` in row j.

        ``code_values``: float64 CUDA tensor ``(n_variants, 4)``, contiguous, indexed by the row's position in the selection.
        ``a``, ``b``: ``(begin, count)`` ranges of ranks in the kept list (default: all K).  Rows are selected as in
        ``sample_counts``.  ``out``: optional float64 CUDA tensor of >= (a_count - 1) * out_stride + b_count entries (written from
        its first element; row padding and everything else are untouched); ``out_stride``: doubles between its rows (default
        b_count).  ``accumulate``: add to what ``out`` holds instead of overwriting it.  ``kernel``: a forced shape
        (``_capi.GRAM_*``)."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._sample_gram(rows, code_values, a, b, out, out_stride, accumulate, kernel)

    def sample_gram_at(self, base: torch.Tensor, record_off: torch.Tensor, code_values: torch.Tensor, n_variants: Optional[int] = None, *,
                       a: Optional[tuple[int, int]] = None, b: Optional[tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
                       out_stride: Optional[int] = None, accumulate: bool = False, kernel: int = _capi.GRAM_AUTO) -> torch.Tensor:
        """``sample_gram`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        rows = self._rows_at(base, record_off, n_variants)
        return self._sample_gram(rows, code_values, a, b, out, out_stride, accumulate, kernel)

    def _sample_gram(self, rows: _Rows, code_values: torch.Tensor, a, b, out: Optional[torch.Tensor], out_stride: Optional[int],
                     accumulate: bool, kernel: int) -> torch.Tensor:
        self._code_values(code_values, rows.n)
        a, b = self._rank_ranges(a, b)
        if out_stride is None:
            out_stride = b[1]
        need = (a[1] - 1) * out_stride + b[1] if a[1] and b[1] else 0
        out = self._flat_out(out, torch.float64, need, "out must be a float64 tensor with >= {need} entries", fill=0 if accumulate else None)
        self._entry("pgenhip_sample_gram", rows, _ptr(code_values), *a, *b, _ptr(out), out_stride,
                    kernel | (_capi.GRAM_ACCUMULATE if accumulate else 0))
        return torch.as_strided(out, (a[1], b[1]), (out_stride, 1))

    # -- Gram product -------------------------------------------------------------------------------
    def gram_apply(self, records: torch.Tensor, code_values: torch.Tensor, q: torch.Tensor, *, record_stride: Optional[int] = None,
                   variant_idx: Optional[torch.Tensor] = None, n_variants: Optional[int] = None, proj: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, out_stride: Optional[int] = None, accumulate: bool = False,
                   kernel: int = _capi.GAPPLY_AUTO, records_offset: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
        """``(Z^T Z) q`` without ``Z^T Z``: with ``Z[j, k] = code_values[j, code of the sample of rank k in row j]`` over the selected
        rows and all K kept samples, returns ``(proj, out)``: ``proj = Z q`` as a float64 ``(n_variants, C)`` CUDA view (always
        overwritten) and ``out = Z^T proj`` as a float64 ``(K, C)`` CUDA view.

        ``code_values``: float64 CUDA tensor ``(n_variants, 4)``, contiguous, indexed by the row's position in the selection.
        ``q``: float64 CUDA tensor ``(K, C)`` with unit column stride, C <= 16 (its row stride is passed on).  Rows are selected as in
        ``sample_counts``.  ``proj``: optional float64 CUDA tensor of >= n_variants * C entries.  ``out``: optional float64 CUDA
        tensor of >= (K - 1) * out_stride + C entries (written from its first element; row padding and everything else are
        untouched); ``out_stride``: doubles between its rows (default C).  ``accumulate``: add to what ``out`` holds instead of
        overwriting it.  ``kernel``: a forced shape (``_capi.GAPPLY_*``)."""
        rows = self._rows(records, record_stride, variant_idx, n_variants, records_offset)
        return self._gram_apply(rows, code_values, q, proj, out, out_stride, accumulate, kernel)

    def gram_apply_at(self, base: torch.Tensor, record_off: torch.Tensor, code_values: torch.Tensor, q: torch.Tensor, *,
                      n_variants: Optional[int] = None, proj: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      out_stride: Optional[int] = None, accumulate: bool = False,
                      kernel: int = _capi.GAPPLY_AUTO) -> tuple[torch.Tensor, torch.Tensor]:
        """``gram_apply`` of records addressed by BYTE OFFSET into ``base`` (``record_off``: int64 CUDA tensor)."""
        rows = self._rows_at(base, record_off, n_variants)
        return self._gram_apply(rows, code_values, q, proj, out, out_stride, accumulate, kernel)

    def _gram_apply(self, rows: _Rows, code_values: torch.Tensor, q: torch.Tensor, proj: Optional[torch.Tensor], out: Optional[torch.Tensor],
                    out_stride: Optional[int], accumulate: bool, kernel: int) -> tuple[torch.Tensor, torch.Tensor]:
        n, k = rows.n, self.kept_count
        self._code_values(code_values, n)
        # q is not a _column_matrix: exactly two dimensions, exactly K rows, and a stride rule of its own that C = 1 does not escape
        if not q.is_cuda or q.device.index != self.device:
            raise ValueError(f"q must live on cuda:{self.device}")
        if q.dtype != torch.float64 or q.dim() != 2 or q.shape[0] != k or not 1 <= q.shape[1] <= _capi.GAPPLY_MAX_COLUMNS:
            raise ValueError(f"q must be a float64 tensor of shape (K = {k}, 1 .. {_capi.GAPPLY_MAX_COLUMNS})")
        c = q.shape[1]
        if k and q.stride(1) != 1 or k > 1 and q.stride(0) < c:
            raise ValueError("q must have unit column stride and a row stride >= its column count")
        q_stride = q.stride(0) if k > 1 else c
        if out_stride is None:
            out_stride = c
        proj = self._flat_out(proj, torch.float64, n * c, "proj must be a float64 tensor with >= {need} entries", name="proj")
        need = (k - 1) * out_stride + c if k else 0
        out = self._flat_out(out, torch.float64, need, "out must be a float64 tensor with >= {need} entries", fill=0 if accumulate else None)
        self._entry("pgenhip_gram_apply", rows, _ptr(code_values), _ptr(q), q_stride, c, _ptr(proj), _ptr(out), out_stride,
                    kernel | (_capi.GAPPLY_ACCUMULATE if accumulate else 0))
        return proj[: n * c].view(n, c), torch.as_strided(out, (k, c), (out_stride, 1))

    _MATRIX_DTYPES = {torch.int8: np.int8, torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32,
                      torch.float16: np.float16, torch.bfloat16: None, torch.float32: np.float32}

    @classmethod
    def matrix_values(cls, dtype: torch.dtype, values=None) -> np.ndarray:
        """The four bit patterns of codes 0-3 as ``4 * itemsize`` bytes (what ``code_values`` of the C ABI points at)."""
        if dtype not in cls._MATRIX_DTYPES:
            raise ValueError(f"decode_matrix does not support {dtype}")
        if values is None:
            values = [0, 1, 2, float("nan") if dtype.is_floating_point else (-1 if dtype.is_signed else torch.iinfo(dtype).max)]
        t = values.detach().cpu().to(dtype) if isinstance(values, torch.Tensor) else torch.tensor(list(values)).to(dtype)
        if t.numel() != 4:
            raise ValueError("values must hold four elements (codes 0, 1, 2, 3)")
        return np.ascontiguousarray(t.contiguous().view(torch.uint8).numpy())

    def _matrix_out(self, out: Optional[torch.Tensor], n_variants: int, dtype: torch.dtype, sample_major: bool, values):
        """(the tensor that owns the memory, the result view, row stride in bytes, the four patterns)"""
        if out is not None:
            dtype = out.dtype
        tab = self.matrix_values(dtype, values)
        rows, cols = (self.kept_count, n_variants) if sample_major else (n_variants, self.kept_count)
        if out is None:
            item = tab.size // 4
            pitch = cols
            if sample_major:
                pitch = (cols * item + 127) // 128 * 128 // item
            out = torch.empty((rows, max(pitch, 1)), dtype=dtype, device=self.torch_device)
            return out, out[:, :cols], max(pitch, 1) * item, tab
        if not out.is_cuda or out.device.index != self.device:
            raise ValueError(f"out must live on cuda:{self.device}")
        if out.dim() != 2 or tuple(out.shape) != (rows, cols):
            raise ValueError(f"out must have shape {(rows, cols)}")
        if cols > 1 and out.stride(1) != 1:
            raise ValueError("out must have unit stride in its last dimension")
        stride = out.stride(0) * out.element_size() if rows > 1 else cols * out.element_size()
        return out, out, stride, tab

    def synth_records(
        self,
        n_variants: int,
        first_variant: int = 0,
        seed: int = 0x5047454E,
        record_stride: Optional[int] = None,
        dirty_pad: bool = False,
        out: Optional[torch.Tensor] = None,
        out_offset: int = 0,
        hwe: bool = False,
    ) -> torch.Tensor:
        """Synthetic records generated on the device (bit-exact twin of the oracle's generator); ``hwe``: the
        Hardy-Weinberg value distribution of SURVEY.md §8d instead of uniform codes."""
        if record_stride is None:
            record_stride = self.record_size
        if out is None:
            out = torch.zeros(out_offset + max(n_variants, 1) * max(record_stride, 1), dtype=torch.uint8, device=self.torch_device)
        self._check_dev(out, "out")
        check(
            lib.pgenhip_synth_records(
                self._ctx, _ptr(out, out_offset), record_stride, first_variant, n_variants, seed,
                (_capi.SYNTH_DIRTY_PAD if dirty_pad else 0) | (_capi.SYNTH_HWE if hwe else 0),
            ),
            "pgenhip_synth_records",
        )
        return out

    def _check_dev(self, t: torch.Tensor, name: str) -> None:
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
