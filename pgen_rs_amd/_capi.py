"""ctypes binding of ``libpgen_hip.so`` (the C ABI in ``include/pgen_hip.h``).

There is no fallback: if the shared library is missing this module raises at import, and if
no HIP device is usable ``pgenhip_create`` returns ``PGENHIP_ERR_NO_DEVICE``.

torch is imported first on purpose: the PyTorch-ROCm wheel bundles its own
``libamdhip64.so.7``; loading it before our library makes the dynamic linker bind our
``DT_NEEDED libamdhip64.so.7`` to that same runtime, so device pointers from torch tensors and
our kernel launches live in one HIP runtime instance.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch  # noqa: F401  (must precede CDLL — see module docstring)

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libpgen_hip.so"

OK = 0
ERR_BAD_ARG = -1
ERR_HIP = -2
ERR_OOM = -3
ERR_INDEX_RANGE = -4
ERR_BAD_MAGIC = -5
ERR_BAD_MODE = -6
ERR_BAD_FLAGS = -7
ERR_NO_DEVICE = -8
ERR_TOO_LARGE = -9
ERR_IO = -10
ERR_BAD_INDEX = -11
ERR_COMPRESSED_RECORD = -12

KERNEL_AUTO = 0
KERNEL_ROWS = 1
KERNEL_FLAT = 2
KERNEL_SCAN = 3
KERNEL_WIDE = 4
KERNEL_PICK = 6
KERNEL_RUNS = 7
KERNEL_ROWPICK = 8
COUNT_AUTO = 0
COUNT_WAVE_PER_ROW = 1
COUNT_ROWS_PER_WAVE = 2

SCOUNT_AUTO = 0
SCOUNT_ROWS = 2
SCOUNT_SHAPE_MASK = 0xF
SCOUNT_ACCUMULATE = 0x10
SCORE_MAX_COLUMNS = 8
SCORE_AUTO = 0
SCORE_ROWS = 1
SCORE_SHAPE_MASK = 0xF
SCORE_ACCUMULATE = 0x10
VSUM_MAX_COLUMNS = 16
VSUM_AUTO = 0
VSUM_GENERAL = 1
VSUM_MFMA = 2
VSUM_SHAPE_MASK = 0xF
LOGIT_MAX_COVARIATES = 15
LOGIT_MAX_ITER = 64
LOGIT_AUTO = 0
LOGIT_GENERAL = 1
LOGIT_FAST = 2
LOGIT_SHAPE_MASK = 0xF
LOGIT_CONVERGED = 0x100
LOGIT_NOT_CONVERGED = 0x200
LOGIT_SINGULAR = 0x400
SPAIR_AUTO = 0
SPAIR_GENERAL = 1
SPAIR_MFMA = 2
SPAIR_SHAPE_MASK = 0xF
SPAIR_ACCUMULATE = 0x10
GRAM_AUTO = 0
GRAM_GENERAL = 1
GRAM_MFMA = 2
GRAM_SHAPE_MASK = 0xF
GRAM_ACCUMULATE = 0x10
GAPPLY_MAX_COLUMNS = 16
GAPPLY_AUTO = 0
GAPPLY_GENERAL = 1
GAPPLY_MFMA = 2
GAPPLY_SHAPE_MASK = 0xF
GAPPLY_ACCUMULATE = 0x10
MATRIX_AUTO = 0
MATRIX_GENERAL = 1
MATRIX_STREAM = 2
MATRIX_TILE = 3
MATRIX_SHAPE_MASK = 0xF
MATRIX_SAMPLE_MAJOR = 0x10
PACK_AUTO = 0
PACK_GENERAL = 1
PACK_DENSE = 2
PACK_GATHER = 3
PARSE_AUTO = 0
PARSE_GENERAL = 1
PARSE_FIXED = 2
PARSE_SHAPE_MASK = 0xF
PARSE_FIELD_COUNT = 0x01
PARSE_BAD_CALL = 0x02
PARSE_ALLELE_RANGE = 0x04
PARSE_HALF_CALL = 0x08
PARSE_HAPLOID = 0x10
PARSE_PHASED = 0x20
PARSE_DECLINED = 0x40
JOIN_AUTO = 0
JOIN_GENERAL = 1
JOIN_STREAM = 2
JOIN_MAX_PARTS = 8
JOIN_ABSENT = 0xFFFFFFFFFFFFFFFF
VCF_LAST_BLOCK = 1
PAIR_TABLE = 0
PAIR_R2 = 1
PRUNE_UNDECIDED = 0
PRUNE_KEPT = 1
PRUNE_REMOVED = 2
PRUNE_AUTO = 0
PRUNE_GENERAL = 1
PRUNE_BLOCK = 2
SYNTH_DIRTY_PAD = 1
SYNTH_HWE = 2
CREATE_KEEP_LIST = 1
LAUNCHES_IN_FLIGHT = 16

KNOB_WIDE_BLOCKS_PER_CU = 1
KNOB_WIDE_RANGES = 2
KNOB_FLAT_BLOCKS_PER_CU = 3
KNOB_SCAN_BLOCKS_PER_CU = 4
KNOB_PICK_BATCH_BYTES = 6
KNOB_RUNS_ROWS = 7
KNOB_SCAN_XCD_MAP = 8
KNOB_SCAN_TWO_PASS = 9
KNOB_SCAN_CHUNK_ROWS = 10
KNOB_ROWPICK_BLOCKS_PER_CU = 11
KNOB_SCAN_ROWPICK = 12
KNOB_ALIGN_STORES = 16
KNOB_SCOUNT_SLICES = 17
KNOB_MATRIX_BLOCKS = 18
KNOB_PAIR_BLOCKS = 19
KNOB_PACK_BLOCKS = 20
KNOB_SCORE_SLICES = 21
KNOB_SPAIR_SLICES = 22
KNOB_VSUM_BLOCKS = 23
KNOB_STORE_POLICY = 24
KNOB_GRAM_SLICES = 25
KNOB_GAPPLY_SAMPLE_SLICES = 26
KNOB_GAPPLY_ROW_SLICES = 27
KNOB_WIDE_BURST = 28
KNOB_PARSE_BLOCKS = 29
KNOB_JOIN_BLOCKS = 30
KNOB_PRUNE_BLOCKS = 31
KNOB_LOGIT_BLOCKS = 32



class VwHeader(C.Structure):
    """``pgenhip_vw_header`` (include/pgen_hip.h): header of a variable-width .pgen (src/pgen.rs:21-137)."""
    _fields_ = [("variant_count", C.c_uint32), ("sample_count", C.c_uint32), ("storage_mode", C.c_uint8),
                ("record_type_bits", C.c_uint8), ("record_length_bytes", C.c_uint8), ("allele_count_bytes", C.c_uint8),
                ("provisional_ref_storage", C.c_uint8), ("reserved", C.c_uint8 * 3), ("block_count", C.c_uint64),
                ("main_header_body_offset", C.c_uint64), ("variant_records_offset", C.c_uint64)]


class JoinPart(C.Structure):
    """``pgenhip_join_part`` (include/pgen_hip.h): one input of ``pgenhip_join_records``."""
    _fields_ = [("d_base", C.c_void_p), ("d_record_off", C.c_void_p), ("d_flip", C.c_void_p), ("sample_count", C.c_uint32),
                ("reserved", C.c_uint32)]


u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
ctx_p = C.c_void_p


def _twins(name: str, *tail) -> dict:
    """An entry that reads rows, and its ``_at`` twin: rows by (records, stride, variant_idx, n) or by (base, record_off, n), then one tail."""
    return {name: (C.c_int, [ctx_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, *tail]),
            name + "_at": (C.c_int, [ctx_p, C.c_void_p, C.c_void_p, C.c_uint32, *tail])}


# name -> (restype, argtypes); every symbol include/pgen_hip.h declares
PROTOTYPES = {
    "pgenhip_abi_version": (C.c_uint32, []),
    "pgenhip_strerror": (C.c_char_p, [C.c_int]),
    "pgenhip_last_error_detail": (C.c_char_p, []),
    "pgenhip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pgenhip_variant_record_size": (C.c_uint32, [C.c_uint32]),
    "pgenhip_parse_header": (C.c_int, [C.c_char_p, u32p, u32p]),
    "pgenhip_record_offset": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "pgenhip_shard_range": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]),
    "pgenhip_vw_parse_header": (C.c_int, [C.c_char_p, C.POINTER(VwHeader)]),
    "pgenhip_vw_walk_index": (C.c_int, [C.POINTER(VwHeader), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgenhip_vw_select_uncompressed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "pgenhip_create": (C.c_int, [C.POINTER(ctx_p), C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]),
    "pgenhip_destroy": (C.c_int, [ctx_p]),
    "pgenhip_set_stream": (C.c_int, [ctx_p, C.c_void_p]),
    "pgenhip_reset_stream": (C.c_int, [ctx_p]),
    "pgenhip_sample_count": (C.c_uint32, [ctx_p]),
    "pgenhip_kept_count": (C.c_uint32, [ctx_p]),
    "pgenhip_gt_row_bytes": (C.c_uint64, [ctx_p]),
    **_twins("pgenhip_decode_emit", C.c_void_p, C.c_uint64, C.c_uint32),
    "pgenhip_emit_lines": (C.c_int, [ctx_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    **_twins("pgenhip_genotype_counts", C.c_void_p, C.c_uint32),
    **_twins("pgenhip_sample_counts", C.c_void_p, C.c_uint32),
    **_twins("pgenhip_sample_scores", C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_variant_sums", C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_variant_logistic", C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double,
             C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_decode_matrix", C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_sample_pair_stats", C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_sample_gram", C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32),
    **_twins("pgenhip_gram_apply", C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32),
    **_twins("pgenhip_pair_stats", C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32),
    **_twins("pgenhip_pair_mask", C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32),
    "pgenhip_prune_resolve": (C.c_int, [ctx_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "pgenhip_packed_record_size": (C.c_uint32, [ctx_p]),
    **_twins("pgenhip_pack_records", C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32),
    "pgenhip_parse_gt": (C.c_int, [ctx_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "pgenhip_join_records": (C.c_int, [ctx_p, C.POINTER(JoinPart), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32]),
    "pgenhip_vcf_index_lines": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p]),
    "pgenhip_tune": (C.c_int, [ctx_p, C.c_uint32, C.c_int32]),
    "pgenhip_wait": (C.c_int, [ctx_p]),
    "pgenhip_timer_start": (C.c_int, [ctx_p]),
    "pgenhip_timer_stop": (C.c_int, [ctx_p, C.POINTER(C.c_float)]),
    "pgenhip_timer_mark": (C.c_int, [ctx_p]),
    "pgenhip_timer_read": (C.c_int, [ctx_p, C.POINTER(C.c_float)]),
    "pgenhip_device_malloc": (C.c_int, [ctx_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "pgenhip_device_free": (C.c_int, [ctx_p, C.c_void_p]),
    "pgenhip_host_malloc_pinned": (C.c_int, [ctx_p, C.POINTER(C.c_void_p), C.c_size_t]),
    "pgenhip_host_free_pinned": (C.c_int, [ctx_p, C.c_void_p]),
    "pgenhip_memcpy_h2d": (C.c_int, [ctx_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgenhip_memcpy_d2h": (C.c_int, [ctx_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgenhip_device_memory": (C.c_int, [ctx_p, u64p, u64p]),
    "pgenhip_synth_records": (C.c_int, [ctx_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32]),
}


class PgenHipError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        detail = lib.pgenhip_last_error_detail().decode(errors="replace")
        msg = lib.pgenhip_strerror(status).decode()
        super().__init__(f"{where}: {msg} (status {status}){': ' + detail if detail else ''}")


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing — the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback."
        )
    handle = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(handle, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    return handle


lib = _load()


def check(status: int, where: str) -> None:
    if status != OK:
        raise PgenHipError(status, where)
