/*
 * pgen_hip.h — C ABI of libpgen_hip.so, the MI355X (gfx950) engine for the
 * one hot path of teoremma/pgen-rs: fixed-width .pgen (storage mode 0x02)
 * variant records -> 2-bit hard-call unpack -> kept-sample select -> VCF GT
 * text.  This is the drop-in boundary: plain pointers and sizes, no C++ or
 * torch types.  The reference has no FFI of its own (it is one private Rust
 * function), so each entry point cites the reference lines it replaces;
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Reference seam: /root/reference/src/pfile.rs:156-192 (Pfile::output_vcf hot
 * loop), :196-200 (variant_record_size), :38-76 (header), :165 (record offset).
 *
 * Error convention: every call returns int, 0 = PGENHIP_OK, negative =
 * pgenhip_status.  Nothing throws or aborts across the boundary (the
 * reference panics at src/pfile.rs:47,53,69,169,170,173; a host maps a
 * negative status to a non-zero exit + stderr).  There is NO CPU fallback:
 * without a usable HIP device pgenhip_create fails with
 * PGENHIP_ERR_NO_DEVICE / PGENHIP_ERR_HIP.
 *
 * Threading: a ctx is bound to one device and is not thread-safe; use one
 * ctx per device per host thread.  Distinct ctxs are independent.
 *
 * Streams: launches are asynchronous on the ctx stream (its own, or the one
 * given to pgenhip_set_stream).  A ctx may be moved between streams at any
 * time and launches queued on different streams may overlap: every launch
 * takes its own block of work-queue counters from a ring of
 * PGENHIP_LAUNCHES_IN_FLIGHT, so at most that many launches of ONE ctx may be
 * in flight at once (a host that keeps more queued must pgenhip_wait in
 * between).  The scratch of the two-pass path (sparse keeps on long
 * records) is sliced the same way: each launch in flight has its own slice.
 * A launch captured into a HIP graph keeps the ring slot it was captured
 * with, so a REPLAY of that graph must not overlap other launches of the same
 * ctx (they come round to its slot every PGENHIP_LAUNCHES_IN_FLIGHT
 * launches): replay on the stream the ctx launches on, or give the graph a
 * ctx of its own.  The kernels leave their counter block zeroed; after a launch
 * that FAILED (any negative status from a launch call) the ctx re-zeroes the
 * whole ring in stream order before its next launch.  A kernel that faults
 * on the device takes the process down like any HIP fault; nothing is
 * recoverable in that case.
 *
 * Nothing in this library reads the process environment: launch-shape knobs
 * are per ctx (pgenhip_tune) and default to the measured best.
 */
#ifndef PGEN_HIP_H
#define PGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGENHIP_ABI_VERSION 2u
#define PGENHIP_LAUNCHES_IN_FLIGHT 16u

typedef enum pgenhip_status {
    PGENHIP_OK = 0,
    PGENHIP_ERR_BAD_ARG = -1,     /* NULL/zero/misordered argument */
    PGENHIP_ERR_HIP = -2,         /* a HIP runtime call failed; see pgenhip_last_error_detail */
    PGENHIP_ERR_OOM = -3,         /* host or device allocation failed */
    PGENHIP_ERR_INDEX_RANGE = -4, /* kept sample index >= sample_count (ref: slice panic, src/pfile.rs:173) */
    PGENHIP_ERR_BAD_MAGIC = -5,   /* src/pfile.rs:47 */
    PGENHIP_ERR_BAD_MODE = -6,    /* src/pfile.rs:53 (only storage mode 0x02) */
    PGENHIP_ERR_BAD_FLAGS = -7,   /* src/pfile.rs:69 (byte 11 must be 0x40) */
    PGENHIP_ERR_NO_DEVICE = -8,   /* no HIP device / ordinal out of range */
    PGENHIP_ERR_TOO_LARGE = -9,   /* a size does not fit the kernel's index types */
    PGENHIP_ERR_IO = -10,         /* file read/write failed (ref: unwrap at src/pfile.rs:169-170) */
    PGENHIP_ERR_BAD_INDEX = -11,  /* variable-width file: block offsets not ascending (src/pgen.rs:160-165), tables truncated, records overlap */
    PGENHIP_ERR_COMPRESSED_RECORD = -12 /* variable-width file: a selected variant's record is not a plain 2-bit record (type != 0 or length != R) */
} pgenhip_status;

typedef struct pgenhip_ctx pgenhip_ctx;

/* ---- library-level ---------------------------------------------------- */
uint32_t pgenhip_abi_version(void);
const char *pgenhip_strerror(int status);
/* thread-local detail string of the last failing call (HIP error text etc.) */
const char *pgenhip_last_error_detail(void);
int pgenhip_device_count(int *count);

/* ---- format geometry (host-side, pure) -------------------------------- */
/* src/pfile.rs:196-200  Pfile::variant_record_size: ceil(2*N/8), u32 like the reference */
uint32_t pgenhip_variant_record_size(uint32_t sample_count);
/* src/pfile.rs:44-69  the 12-byte header: magic 6C 1B, mode 02, u32 LE variants, u32 LE samples, 0x40 */
int pgenhip_parse_header(const uint8_t header[12], uint32_t *variant_count, uint32_t *sample_count);
/* src/pfile.rs:165  byte offset of record var_idx in the file; computed in u64
 * (the reference multiplies in u32 and wraps at var_idx*R >= 2^32 — SURVEY.md F5). */
uint64_t pgenhip_record_offset(uint64_t var_idx, uint32_t record_size);
/* src/pfile.rs:156  the outer loop walks the kept-variant list in file order; a shard is a
 * contiguous slice of that iteration space.  [*begin, *end) of the n_variants
 * kept variants owned by `rank` of `world`; sizes differ by at most one, low ranks take the
 * extra.  The ONE partitioner: the C++ host's device threads, bench.py's ranks and the tests
 * all call this.  PGENHIP_ERR_BAD_ARG for world == 0 or rank >= world. */
int pgenhip_shard_range(uint64_t n_variants, uint32_t world, uint32_t rank, uint64_t *begin, uint64_t *end);

/* ---- variable-width storage modes: header and offset-table walk ----------------------
 * The reference only VALIDATES these tables (src/pgen.rs, the dead `Pgen` type: header bits :52-67, block offsets
 * :140-169, per-block type / length arrays :172-258) and its tool refuses every mode but 0x02 (src/pfile.rs:53).
 * This slice turns the same tables into per-variant byte offsets so that the records such a file stores
 * UNCOMPRESSED (record type 0: the mode-0x02 2-bit layout, length R) can be decoded in place by the kernels
 * (pgenhip_decode_emit_at); any other record type is reported, never guessed at.  Allele-count arrays
 * (allele_count_bytes != 0) are outside the slice: PGENHIP_ERR_BAD_FLAGS. */
typedef struct pgenhip_vw_header {
    uint32_t variant_count;           /* src/pgen.rs:42 */
    uint32_t sample_count;            /* :47 */
    uint8_t storage_mode;             /* :34 (0x10 = standard variable-width; the reference prints it, asserts nothing) */
    uint8_t record_type_bits;         /* :61-65  4 or 8 */
    uint8_t record_length_bytes;      /* :67     1..4 */
    uint8_t allele_count_bytes;       /* :56 */
    uint8_t provisional_ref_storage;  /* :57 */
    uint8_t reserved[3];
    uint64_t block_count;             /* :100-102  ceil(variant_count / 65 536) */
    uint64_t main_header_body_offset; /* :112-114  12 + 8 * block_count */
    uint64_t variant_records_offset;  /* :135-137  end of the type/length tables (type arrays rounded up per block, as the file stores them) */
} pgenhip_vw_header;
/* src/pgen.rs:21-98: BAD_MAGIC (:30), BAD_FLAGS (provisional_ref_storage != 1 :58, record storage mode >= 8 :64, allele counts present) */
int pgenhip_vw_parse_header(const uint8_t header[12], pgenhip_vw_header *out);
/* src/pgen.rs:140-258 turned into per-variant tables.  `index` = the file's bytes [12, variant_records_offset)
 * (index_len of them); outputs are HOST arrays of variant_count entries: the record's type (4- or 8-bit value),
 * its length and its byte offset in the file (block offset + lengths of the block's earlier records).
 * PGENHIP_ERR_BAD_INDEX: table truncated, block offsets not strictly ascending (:160-165), a block's records
 * run into the next block, the first record starts inside the tables, or offsets overflow 64 bits.
 * PGENHIP_ERR_BAD_ARG: *h is not what pgenhip_vw_parse_header produces — record_type_bits not 4 / 8, record_length_bytes
 * not 1..4, or block_count / variant_records_offset that do not follow from variant_count and those widths (the walk
 * recomputes them; nothing derived is trusted). */
int pgenhip_vw_walk_index(const pgenhip_vw_header *h, const uint8_t *index, uint64_t index_len,
                          uint8_t *record_type, uint32_t *record_len, uint64_t *record_off);
/* The selected variants (variant_idx[0..n), or the first n when NULL) must all be plain 2-bit records:
 * type 0 and length == R; writes their offsets to sel_off (n entries).  Else PGENHIP_ERR_COMPRESSED_RECORD
 * (pgenhip_last_error_detail names the first offending variant and its type). */
int pgenhip_vw_select_uncompressed(const uint8_t *record_type, const uint32_t *record_len, const uint64_t *record_off,
                                   uint32_t variant_count, const uint32_t *variant_idx, uint32_t n,
                                   uint32_t record_size, uint64_t *sel_off);

/* ---- context ---------------------------------------------------------- */
/* Binds a device and the kept-sample list (src/pfile.rs:128 sam_idx_rcs; the
 * list filter_metadata :319-333 builds is strictly ascending, and that is
 * required here).  Without PGENHIP_CREATE_KEEP_LIST, kept_idx == NULL means
 * "all samples" (K = N fast path) and a non-NULL kept_idx is a HOST array of
 * kept_count indices, copied.  With PGENHIP_CREATE_KEEP_LIST in `flags` the
 * pair (kept_idx, kept_count) IS the list whatever the pointer: kept_count
 * may be 0 (every row is then just "\n") and kept_idx may then be NULL — a
 * host whose filter kept nobody must say so with the flag, not with the
 * pointer (an empty std::vector's data() is NULL). */
#define PGENHIP_CREATE_KEEP_LIST 1u
int pgenhip_create(pgenhip_ctx **ctx, int device_ordinal, uint32_t sample_count,
                   const uint32_t *kept_idx, uint32_t kept_count, uint32_t flags);
int pgenhip_destroy(pgenhip_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the ctx's own.
 * NULL means HIP's default (null) stream — that IS torch's current stream unless a stream
 * context is active.  pgenhip_reset_stream goes back to the ctx's own non-blocking stream. */
int pgenhip_set_stream(pgenhip_ctx *ctx, void *hip_stream);
int pgenhip_reset_stream(pgenhip_ctx *ctx);
uint32_t pgenhip_sample_count(const pgenhip_ctx *ctx);
uint32_t pgenhip_kept_count(const pgenhip_ctx *ctx);
/* 4*K + 1: bytes one variant's GT segment occupies (src/pfile.rs:186-190) */
uint64_t pgenhip_gt_row_bytes(const pgenhip_ctx *ctx);

/* ---- the hot path (device-resident, asynchronous on the ctx stream) ---- */
/* kernel selection for pgenhip_decode_emit flags (0 = automatic) */
#define PGENHIP_KERNEL_AUTO 0u
#define PGENHIP_KERNEL_ROWS 1u   /* general row-tiled kernel (any stride/alignment, list gather) */
#define PGENHIP_KERNEL_FLAT 2u   /* dense all-samples stream kernel (out_stride == 4N+1) */
#define PGENHIP_KERNEL_SCAN 3u   /* kept subset on long records: per-segment rank->sample table pick (N >= 61) */
#define PGENHIP_KERNEL_WIDE 4u   /* dense all-samples, wide LDS-staged record loads, one row piece per item (N >= 1024) */
/* 5u was round 1's stream-span kernel (measured level with WIDE, removed) */
#define PGENHIP_KERNEL_PICK 6u   /* kept subset on short records (61 <= N <= 4096, K >= 1, dense pitch): output-driven pick through the kept list */
#define PGENHIP_KERNEL_RUNS 7u   /* dense all-samples on SHORT rows (8 <= N <= ~2000, dense records, no gather): runs of rows as one work item */
#define PGENHIP_KERNEL_ROWPICK 8u /* sparse kept subset (1 <= K <= 16384) on long records: one wave per row, the row's compact record assembled in LDS, text written in one go; any strides */
#define PGENHIP_KERNEL_MASK 0xFu

/* src/pfile.rs:165-190 for a block of n_variants kept variants.
 *   row j reads the record at d_records + r*record_stride, r = d_variant_idx ? d_variant_idx[j] : j
 *   (record layout: sample s in byte s/4, bits 2*(s%4), LSB first — :172-175)
 *   and writes K x {'\t',a,'/',b} + '\n' = 4K+1 bytes at d_out + j*out_stride (:177-190).
 * All pointers are DEVICE pointers; any alignment and any strides with
 * record_stride >= R, out_stride >= 4K+1 (or n_variants <= 1).  Bytes of d_out
 * outside the n_variants segments are not touched.  No allocation, no
 * synchronisation: the launch is queued on the ctx stream (graph-capturable). */
int pgenhip_decode_emit(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride,
                        const uint32_t *d_variant_idx, uint32_t n_variants,
                        void *d_out, uint64_t out_stride, uint32_t flags);

/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of n_variants byte offsets): the
 * uncompressed records of a variable-width file staged to HBM as it lies on disk, or any other gapped layout.
 * Every kernel family takes this gather (it replaces variant_idx * record_stride); RUNS needs dense records. */
int pgenhip_decode_emit_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                           void *d_out, uint64_t out_stride, uint32_t flags);

/* Full VCF body lines (src/pfile.rs:156-192): line j = prefix bytes
 * d_prefix_blob[d_prefix_off[j] .. d_prefix_off[j+1]) (pvar columns + '\t' each,
 * then "GT", :157-161) + GT segment + '\n', written at d_out + d_line_off[j].
 * d_prefix_off/d_line_off are device arrays of n_variants+1 u64 with
 * d_line_off[j+1]-d_line_off[j] == prefix_len(j) + 4K + 1 (lines packed back to back);
 * max_prefix_bytes is a host-known upper bound of any prefix length.  It must be a TRUE bound: the kernels size their LDS staging
 * and their seam passes by it; with a smaller value lines come out wrong (nothing is read or written out of bounds: blob loads
 * are sized by d_prefix_off, stores addressed from d_line_off and kept inside [d_line_off[0], d_line_off[n_variants])).  A loose
 * bound is legal and exact.  A bound with max_prefix_bytes + 4K + 1 >= 2^31 is PGENHIP_ERR_TOO_LARGE before any launch.
 * d_prefix_blob may be NULL only with max_prefix_bytes == 0 (every prefix empty; d_prefix_off entries then need not be 0).
 * flags: PGENHIP_KERNEL_AUTO picks by shape — all samples kept: the work-queue stream kernel from 1 400 samples (GT segments
 * in place behind their prefixes), below it runs of whole lines assembled in LDS (short prefixes, N < 1 000) or the pick
 * family's interiors + seams kernel; a kept subset: the pick family on records of up to 4 096 samples, the segment kernels or
 * the two passes on longer ones, the general kernel for tiny shapes.  Every kernel writes the prefixes itself (no separate
 * copy).  PGENHIP_KERNEL_ROWS, _WIDE, _SCAN, _PICK, _RUNS or _ROWPICK force one (tests, A/B). */
int pgenhip_emit_lines(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride,
                       const uint32_t *d_variant_idx, uint32_t n_variants,
                       const void *d_prefix_blob, const uint64_t *d_prefix_off,
                       const uint64_t *d_line_off, uint64_t max_prefix_bytes,
                       void *d_out, uint32_t flags);

/* ---- per-variant genotype counts (device-resident, asynchronous on the ctx stream) ----
 * For row j (records selected exactly as in pgenhip_decode_emit / pgenhip_decode_emit_at) writes four u32 at
 * d_counts[4*j + c]: the number of the ctx's kept samples with code c — 0 hom-ref ("0/0"), 1 het ("0/1"),
 * 2 hom-alt ("1/1"), 3 missing ("./.") — i.e. the GT fields pgenhip_decode_emit writes for that row, counted
 * (src/pfile.rs:172-183).  The pad bits of a record's last byte are never counted.  Records may start at any byte
 * alignment; with record_stride >= R (or n_variants <= 1).  Nothing outside d_counts[0 .. 4*n_variants) is written.
 * n_variants == 0 is a no-op.  Same launch contract as pgenhip_decode_emit: device pointers only, no allocation, no
 * synchronisation, queued on the ctx stream, graph-capturable.
 * flags: PGENHIP_COUNT_AUTO picks the shape by N (a wave per row above 6 084 samples); the other two force one. */
#define PGENHIP_COUNT_AUTO 0u
#define PGENHIP_COUNT_WAVE_PER_ROW 1u    /* long rows: one wave per row, wave reduction, one 16-byte store */
#define PGENHIP_COUNT_ROWS_PER_WAVE 2u   /* short rows: 4 .. 32 lanes per row, several rows per wave */
int pgenhip_genotype_counts(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                            uint32_t n_variants, uint32_t *d_counts, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets): the plain records of a
 * variable-width file staged as they lie on disk. */
int pgenhip_genotype_counts_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                               uint32_t *d_counts, uint32_t flags);

/* ---- per-sample genotype counts (device-resident, asynchronous on the ctx stream) ----
 * The other half of pgenhip_genotype_counts: for every kept sample, the number of selected rows in which it has each code.
 * Rows are selected exactly as in pgenhip_genotype_counts / pgenhip_genotype_counts_at (and pgenhip_decode_emit); each selected
 * row counts once per appearance, so a gather that repeats a row counts it twice.  Writes four u32 per kept sample at
 * d_counts[4*k + c]: k is the sample's rank in the ctx's kept list (its index when all samples are kept), c is 0 hom-ref ("0/0"),
 * 1 het ("0/1"), 2 hom-alt ("1/1"), 3 missing ("./."), the order of the per-variant counts.  The pad bits of a record's last
 * byte are never counted.  Records may start at any byte alignment, with record_stride >= R (or n_variants <= 1).
 *   - Without PGENHIP_SCOUNT_ACCUMULATE the call overwrites d_counts[0 .. 4K) (zeros when n_variants == 0).  With it the counts
 *     are added to what d_counts holds, so a host can sum blocks of rows in place; n_variants == 0 is then a no-op.
 *   - Nothing outside d_counts[0 .. 4K) is written; K == 0 writes nothing.  d_counts must be 4-byte aligned, else
 *     PGENHIP_ERR_BAD_ARG.
 *   - Counts wrap modulo 2^32 only if one sample is counted more than 2^32 - 1 times, which takes repeated rows (a file's
 *     variant count is a u32).
 * Same launch contract as pgenhip_genotype_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable.
 * flags: a shape (PGENHIP_SCOUNT_AUTO or a forced one) | PGENHIP_SCOUNT_ACCUMULATE. */
#define PGENHIP_SCOUNT_AUTO 0u
/* 1u is reserved for a dense byte-stream shape (columns fixed modulo lcm(R, 16)); not built */
#define PGENHIP_SCOUNT_ROWS 2u        /* row by row, any layout (variant_idx, record_off, padded strides): what AUTO takes */
#define PGENHIP_SCOUNT_SHAPE_MASK 0xFu
#define PGENHIP_SCOUNT_ACCUMULATE 0x10u
int pgenhip_sample_counts(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, uint32_t *d_counts, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_sample_counts_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             uint32_t *d_counts, uint32_t flags);

/* ---- per-sample weighted dosage sums: polygenic scores (device-resident, asynchronous on the ctx stream) ----
 * pgenhip_sample_counts with a weight per row: for every kept sample k and column c < n_columns
 *     S[k, c] = sum over the selected rows j of (double)d_weights[j * w_stride + c] * D(j, k)
 * where D is 0, 1, 2 for codes 0, 1, 2 (the number of alternate alleles) and (double)d_miss[j] for code 3 (missing); 0.0 for a
 * missing call when d_miss is NULL.  Rows are selected exactly as in pgenhip_sample_counts / pgenhip_sample_counts_at; a gather
 * that repeats a row adds it twice.  d_weights and d_miss are DEVICE arrays of f32 indexed by j, the row's position in the
 * selection (not the file's row number); w_stride is in floats, >= n_columns (or n_variants <= 1).  The pad bits of a record's
 * last byte are never read as samples.  Records may start at any byte alignment.
 *   - Arithmetic: every term is formed in FP64, where it is exact (f32 times 1, 2 or an f32 fits 53 bits), and the terms are
 *     accumulated in FP64 only; there are no f32 partial sums.  The ORDER of the additions is not fixed (blocks combine through
 *     FP64 atomics), so the result of any (k, c) is within (n_variants + 1) * 2^-53 * sum|term| of the exact sum, and two runs
 *     on the same input may differ in the last bits: bitwise run-to-run reproducibility is NOT promised.  Sums whose every
 *     partial sum is an integer below 2^53 are exact whatever the order.  Non-finite weights or miss values give unspecified
 *     results.
 *   - Writes n_columns doubles per kept sample at d_scores[k * n_columns + c]; k is the sample's rank in the ctx's kept list
 *     (its index when all samples are kept).  Without PGENHIP_SCORE_ACCUMULATE the call overwrites d_scores[0 .. K * n_columns)
 *     (zeros when n_variants == 0).  With it the sums are added to what d_scores holds; n_variants == 0 is then a no-op.
 *     Nothing outside d_scores[0 .. K * n_columns) is written; K == 0 writes nothing.
 *   - d_scores must be ORDINARY device memory (hipMalloc, pgenhip_device_malloc), not fine-grained or host-mapped memory: the
 *     kernel adds with hardware FP64 atomics, which such memory does not serve.
 *   - PGENHIP_ERR_BAD_ARG: n_columns == 0 or > PGENHIP_SCORE_MAX_COLUMNS; w_stride < n_columns with n_variants > 1; d_weights
 *     NULL with n_variants > 0; d_scores NULL or not 8-byte aligned with K > 0; d_weights or d_miss not 4-byte aligned; unknown
 *     flag bits or shapes.  PGENHIP_ERR_TOO_LARGE, before any launch: byte offsets of 2^52 or more (w_stride * n_variants * 4,
 *     record_stride * n_variants as in pgenhip_decode_matrix).  A host with more than PGENHIP_SCORE_MAX_COLUMNS scores calls
 *     once per group of columns (d_weights + first column of the group, the same w_stride).
 * Same launch contract as pgenhip_sample_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable (the overwrite is a hipMemsetAsync ahead of the kernel).
 * flags: a shape (PGENHIP_SCORE_AUTO or a forced one) | PGENHIP_SCORE_ACCUMULATE. */
#define PGENHIP_SCORE_MAX_COLUMNS 8u
#define PGENHIP_SCORE_AUTO 0u
#define PGENHIP_SCORE_ROWS 1u         /* row by row, any layout (variant_idx, record_off, padded strides): what AUTO takes */
/* 2u is reserved for a matrix-core form for many columns (v_mfma_f64_16x16x4_f64); not built */
#define PGENHIP_SCORE_SHAPE_MASK 0xFu
#define PGENHIP_SCORE_ACCUMULATE 0x10u
int pgenhip_sample_scores(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, const float *d_weights, uint64_t w_stride, uint32_t n_columns,
                          const float *d_miss, double *d_scores, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_sample_scores_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             const float *d_weights, uint64_t w_stride, uint32_t n_columns,
                             const float *d_miss, double *d_scores, uint32_t flags);

/* ---- per-variant sums of per-sample values by genotype code (device-resident, asynchronous on the ctx stream) ----
 * The transpose of pgenhip_sample_scores: for every selected row j, value column c < n_columns and code x in {0, 1, 2, 3}
 *     d_sums[(j * n_columns + c) * 4 + x] = sum over the kept samples k whose code in row j is x of d_values[k * v_stride + c]
 * k is the sample's rank in the ctx's kept list (its index when all samples are kept); x is 0 hom-ref, 1 het, 2 hom-alt, 3 missing,
 * the order of the per-variant counts.  From the four sums of a column a host derives a regression of the column on the genotype
 * (any missing-call policy), a genotypic model and per-genotype means without touching a genotype again.  d_values is a DEVICE
 * array of FP64, K x n_columns; v_stride is in doubles, >= n_columns (or K <= 1).  FP64 input is deliberate: a term is the value
 * itself (there is no product), so FP64 costs nothing in exactness and a host passes residualised phenotypes unrounded.
 * Rows are selected exactly as in pgenhip_genotype_counts / pgenhip_genotype_counts_at: by stride (record_stride >= R, or
 * n_variants <= 1), through d_variant_idx, or through d_record_off; records may start at any byte alignment; a gather that repeats
 * a row writes it twice.  The pad bits of a record's last byte and samples >= N are never read as samples.
 *   - Arithmetic: every addition is FP64; there are no f32 partial sums.  The ORDER of the additions is not fixed (tiles of one
 *     row combine through FP64 atomics).  With A_c = sum over all kept k of |d_values[k * v_stride + c]|, each of the four sums
 *     of (j, c) is within (K + 1) * 2^-53 * A_c of its exact value.  The bound is stated against A_c, not against the class's own
 *     sum, on purpose: an implementation may obtain one class as the column total minus the other three.  Sums whose every
 *     partial sum is an integer below 2^53 are exact whatever the order.  Non-finite values give unspecified results.  Two runs
 *     on the same input may differ in the last bits: bitwise run-to-run reproducibility is NOT promised.
 *   - The call overwrites exactly the 4 * n_columns * n_variants doubles d_sums[0 .. 4 * n_columns * n_variants); nothing else is
 *     written.  K == 0 writes zeros.  n_variants == 0 is a no-op.  There is no ACCUMULATE flag: rows are the unit a host blocks
 *     over, and each row's sums are complete after one call.
 *   - d_sums must be ORDINARY device memory (hipMalloc, pgenhip_device_malloc), not fine-grained or host-mapped memory: the
 *     kernel adds with hardware FP64 atomics, which such memory does not serve.
 *   - PGENHIP_ERR_BAD_ARG: n_columns == 0 or > PGENHIP_VSUM_MAX_COLUMNS; v_stride < n_columns with K > 1; d_values NULL with
 *     K > 0 and n_variants > 0; d_values or d_sums not 8-byte aligned; d_sums NULL with n_variants > 0; unknown flag bits or
 *     shape ids; a forced shape that does not apply (with a detail string: PGENHIP_VSUM_MFMA needs K >= 1).
 *     PGENHIP_ERR_TOO_LARGE, before any launch: byte offsets of 2^52 or more (v_stride * K * 8, n_variants * n_columns * 32,
 *     record_stride * n_variants as in pgenhip_decode_matrix).  A host with more than PGENHIP_VSUM_MAX_COLUMNS columns calls once
 *     per group of columns (d_values + first column of the group, the same v_stride).
 * Same launch contract as pgenhip_genotype_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable (the overwrite is a hipMemsetAsync ahead of the kernel where tiles of a row meet in atomics).  No work
 * counters: these launches do not count against PGENHIP_LAUNCHES_IN_FLIGHT.
 * flags: a shape (PGENHIP_VSUM_AUTO or a forced one). */
#define PGENHIP_VSUM_MAX_COLUMNS 16u
#define PGENHIP_VSUM_AUTO 0u
#define PGENHIP_VSUM_GENERAL 1u   /* a wave per (row, column), any K, any layout: the correctness baseline */
#define PGENHIP_VSUM_MFMA 2u      /* the samples of a row summed by the FP64 matrix core (v_mfma_f64_16x16x4_f64), all samples or a kept list, K >= 1: what AUTO takes */
#define PGENHIP_VSUM_SHAPE_MASK 0xFu
int pgenhip_variant_sums(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                         uint32_t n_variants, const double *d_values, uint64_t v_stride, uint32_t n_columns, double *d_sums,
                         uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_variant_sums_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                            const double *d_values, uint64_t v_stride, uint32_t n_columns, double *d_sums, uint32_t flags);

/* ---- per-variant logistic regression (device-resident, asynchronous on the ctx stream) ----
 * What pgenhip_variant_sums cannot give: a fit whose weights depend on the row's own coefficients.  For every selected row j a
 * logistic regression of d_y on X = [design, g] over the ctx's kept samples, g_k = t_j[x_j(k)] with x_j(k) the code of kept sample k
 * in row j (0 hom-ref, 1 het, 2 hom-alt, 3 missing) and t_j = d_code_values[4*j .. 4*j+3] (the table argument of pgenhip_sample_gram:
 * a DEVICE array of FP64 indexed by the row's position in the selection).  A NaN table entry leaves the samples with that code out of
 * row j's fit, so one kernel serves both policies for a missing call: a host passes the row's mean dosage for code 3 (mean
 * imputation) or NaN (the sample is dropped for that row).  The library does not interpret the table.
 * Rows are selected exactly as in pgenhip_variant_sums / pgenhip_variant_sums_at: by stride (record_stride >= R, or n_variants <= 1),
 * through d_variant_idx, or through d_record_off; records may start at any byte alignment; a gather that repeats a row writes it
 * twice.  The pad bits of a record's last byte and samples >= N are never read as samples.  d_design is a DEVICE array of FP64,
 * K x n_cov, indexed by the sample's rank in the kept list like d_values of pgenhip_variant_sums (x_stride in doubles, >= n_cov or
 * K <= 1; a host puts the intercept there as a column); d_y holds K values in [0, 1]; d_start the n_cov coefficients of the null
 * model (the fit without the genotype), from which every row starts.
 *   - The algorithm is fixed, so that a reference can restate it.  beta = (d_start, 0).  For it = 1 .. max_iter: over the included
 *     samples evaluate mu = 1 / (1 + e^-(X beta)), grad = X^T (y - mu) and H = X^T diag(mu (1 - mu)) X; take the Cholesky factor of
 *     H, where a pivot that is <= 0 or not finite ends the row as SINGULAR (the coefficients keep this beta, the SE is NaN);
 *     delta = H^-1 grad; if max |delta_i| <= tol the row is CONVERGED and reports THIS beta (not beta + delta), SE =
 *     sqrt((H^-1)[g][g]) from this H and it evaluations; else, if it == max_iter, the row is NOT_CONVERGED (the coefficients hold
 *     this beta, the SE is NaN); else beta += delta.  So max_iter evaluations take at most max_iter - 1 steps.  There is no step
 *     halving and no Firth penalty: a separated row ends as NOT_CONVERGED or SINGULAR.  A row with no included sample is SINGULAR.
 *   - Arithmetic: every product and every addition is FP64.  The ORDER of the additions is not fixed (samples are dealt to lanes);
 *     bitwise run-to-run and shape-to-shape reproducibility is NOT promised.  e^-eta overflowing to inf gives mu = 0, not NaN.
 *   - Outputs, per row j: d_coef[j * c_stride .. + n_cov] (c_stride in doubles, >= n_cov + 1 or n_variants <= 1): the covariates'
 *     coefficients, then the genotype's; d_se[j]: the genotype's standard error or NaN; d_status[j]: the evaluations done in the low
 *     8 bits and one of PGENHIP_LOGIT_CONVERGED / NOT_CONVERGED / SINGULAR.  d_coef rows may be used as working storage during the
 *     call; nothing outside the three outputs is written.  K == 0 writes SINGULAR for every row (d_design and d_y are not read).
 *     n_variants == 0 is a no-op.
 *   - PGENHIP_ERR_BAD_ARG, before any launch and with nothing written: n_cov == 0 or > PGENHIP_LOGIT_MAX_COVARIATES; max_iter == 0 or
 *     > PGENHIP_LOGIT_MAX_ITER; tol NaN or negative; x_stride < n_cov with K > 1; c_stride < n_cov + 1 with n_variants > 1; with
 *     n_variants > 0 a NULL d_code_values, d_start, d_coef, d_se or d_status, and with K > 0 as well a NULL d_design or d_y; a
 *     pointer to doubles that is not 8-byte aligned, d_status not 4-byte aligned; unknown flag bits or shape ids.
 *     PGENHIP_ERR_TOO_LARGE, before any launch: byte offsets of 2^52 or more (x_stride * K * 8, c_stride * n_variants * 8,
 *     record_stride * n_variants as in pgenhip_decode_matrix).
 * Same launch contract as pgenhip_variant_sums: device pointers only, no allocation, no synchronisation, one kernel queued on the
 * ctx stream, graph-capturable, no work counters (these launches do not count against PGENHIP_LAUNCHES_IN_FLIGHT), outputs in
 * ordinary device memory.  One row's samples are not split over blocks (the iteration needs no meeting across blocks): a call with
 * few rows of very long records uses few CUs.  PGENHIP_KNOB_LOGIT_BLOCKS forces the grid.
 * flags: a shape (PGENHIP_LOGIT_AUTO or a forced one). */
#define PGENHIP_LOGIT_MAX_COVARIATES 15u   /* design columns incl. the intercept; the genotype is the 16th */
#define PGENHIP_LOGIT_MAX_ITER 64u
#define PGENHIP_LOGIT_AUTO 0u
#define PGENHIP_LOGIT_GENERAL 1u   /* a block per row, one pass over the samples per row of H: the correctness baseline, any shape */
#define PGENHIP_LOGIT_FAST 2u      /* H's lower half in each lane's registers, one pass per evaluation, rows in groups: what AUTO takes */
#define PGENHIP_LOGIT_SHAPE_MASK 0xFu
/* d_status[j]: low 8 bits = evaluations done; then */
#define PGENHIP_LOGIT_CONVERGED     0x100u
#define PGENHIP_LOGIT_NOT_CONVERGED 0x200u
#define PGENHIP_LOGIT_SINGULAR      0x400u
int pgenhip_variant_logistic(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                             uint32_t n_variants, const double *d_code_values, const double *d_design, uint64_t x_stride,
                             uint32_t n_cov, const double *d_y, const double *d_start, uint32_t max_iter, double tol,
                             double *d_coef, uint64_t c_stride, double *d_se, uint32_t *d_status, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_variant_logistic_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                                const double *d_code_values, const double *d_design, uint64_t x_stride, uint32_t n_cov,
                                const double *d_y, const double *d_start, uint32_t max_iter, double tol, double *d_coef,
                                uint64_t c_stride, double *d_se, uint32_t *d_status, uint32_t flags);

/* ---- numeric genotype matrix (device-resident, asynchronous on the ctx stream) ----
 * The GT text with the fixed bytes removed: element (j, k) is the code pgenhip_decode_emit prints as the k-th field of row j,
 * mapped through a four-entry table.  Rows are selected exactly as in pgenhip_decode_emit / pgenhip_decode_emit_at; a gather that
 * repeats a row writes it twice.  k is the sample's rank in the ctx's kept list (its index when all samples are kept), c the
 * 2-bit code of that sample in that row (src/pfile.rs:172-175; the pad bits of a record's last byte are never read as samples).
 *   - elem_bytes is 1, 2 or 4.  code_values is a HOST pointer to four elements of elem_bytes bytes, the bit patterns written for
 *     codes 0, 1, 2, 3; it is read during the call and passed as kernel arguments (no device copy, no allocation; a captured
 *     graph keeps the patterns it was captured with).  NULL means 0, 1, 2 and all bits set (-1 as a signed integer).  The library
 *     does not interpret the elements: int8, uint8, fp16, bf16, fp32 and int32 are all "a size and four patterns", and results
 *     compare byte for byte.
 *   - Variant-major (default): element (j, k) at d_out + j*out_stride + k*elem_bytes, out_stride >= K*elem_bytes (or
 *     n_variants <= 1).  Sample-major (PGENHIP_MATRIX_SAMPLE_MAJOR): at d_out + k*out_stride + j*elem_bytes, out_stride >=
 *     n_variants*elem_bytes (or K <= 1).  out_stride is in bytes; d_out and out_stride must be multiples of elem_bytes, else
 *     PGENHIP_ERR_BAD_ARG.  Bytes of d_out outside the n_variants x K elements (row padding included) are not touched.
 *     n_variants == 0 or K == 0 writes nothing.
 *   - Shapes.  GENERAL applies always.  STREAM: all samples kept (no list, or the identity list), variant-major, any d_out /
 *     out_stride the contract allows.  TILE: all samples kept, sample-major, d_out and out_stride multiples of 16 bytes (its stores
 *     cover whole 128-byte lines when they are multiples of 128: pad the row pitch).  A forced shape that does not apply is
 *     PGENHIP_ERR_BAD_ARG with a detail string; AUTO takes STREAM / TILE where they apply and GENERAL everywhere else.
 *   - An offset that does not fit the kernels' index types (2^52 bytes or more) is PGENHIP_ERR_TOO_LARGE before any launch: the
 *     n_variants x K elements, out_stride times the output rows, record_stride times n_variants.  With d_variant_idx only record_stride
 *     itself is bounded: the row numbers live on the device, like d_record_off's offsets, and a record's address is 64-bit arithmetic.
 * Same launch contract as pgenhip_genotype_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable.
 * flags: a shape (low 4 bits) | orientation. */
#define PGENHIP_MATRIX_AUTO 0u
#define PGENHIP_MATRIX_GENERAL 1u     /* any K, any strides, both orientations: the correctness baseline */
#define PGENHIP_MATRIX_STREAM 2u      /* variant-major, all samples kept */
#define PGENHIP_MATRIX_TILE 3u        /* sample-major, all samples kept, 16-byte-aligned rows: tile transpose */
#define PGENHIP_MATRIX_SHAPE_MASK 0xFu
#define PGENHIP_MATRIX_SAMPLE_MAJOR 0x10u
int pgenhip_decode_matrix(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                          uint32_t n_variants, void *d_out, uint64_t out_stride, uint32_t elem_bytes,
                          const void *code_values, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_decode_matrix_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                             void *d_out, uint64_t out_stride, uint32_t elem_bytes, const void *code_values, uint32_t flags);

/* ---- windowed pairwise genotype tables / r^2 (device-resident, asynchronous on the ctx stream) ----
 * How two variants go together: for every pair of selected rows (i, i + d) with 0 <= i < n_left, 1 <= d <= window and
 * i + d < n_variants, the joint table of the two rows' codes over the ctx's kept samples, or the r^2 of that table.
 * Rows are selected exactly as in pgenhip_genotype_counts / pgenhip_genotype_counts_at: by stride (record_stride >= R, or
 * n_variants <= 1), through d_variant_idx, or through d_record_off; records may start at any byte alignment.  Samples >= N and the
 * pad bits of a record's last byte are never counted.  n_variants is the number of selected rows, n_left <= n_variants how many
 * leading rows own pairs (a host that streams blocks overlapping by `window` rows passes the block's own rows as n_left and computes
 * no pair twice), window = W >= 1.  The pair (i, i + d) has pair index p = i * W + (d - 1).
 *   - PGENHIP_PAIR_TABLE: sixteen u32 at d_out[16*p + 4*a + b], the number of kept samples with code a in row i and code b in row
 *     i + d (0 hom-ref, 1 het, 2 hom-alt, 3 missing: the order of the count entry points).  The sums over b are
 *     pgenhip_genotype_counts of row i, the sums over a those of row i + d, the whole table sums to K.  d_out must be 16-byte
 *     aligned (an entry is four 16-byte stores), else PGENHIP_ERR_BAD_ARG.
 *   - PGENHIP_PAIR_R2: one f32 at d_out[p], from the same table's cells with a, b in {0, 1, 2} (samples called in both rows):
 *     n = their sum, Sx = sum a*T, Sy = sum b*T, Sxx = sum a^2*T, Syy = sum b^2*T, Sxy = sum a*b*T and
 *     r^2 = (n*Sxy - Sx*Sy)^2 / ((n*Sxx - Sx^2) * (n*Syy - Sy^2)).  The three bracketed terms are exact 64-bit integers; each is
 *     converted to double, they are combined in double and the result is rounded once to f32.  A zero denominator (n == 0, or a
 *     row that is monomorphic among the jointly called samples) gives NaN.  This is the unphased genotype correlation; no byte or
 *     digit parity with another tool's r^2 is claimed.  d_out must be 4-byte aligned, else PGENHIP_ERR_BAD_ARG.
 *   - Entries with i + d >= n_variants are NOT touched, nor is anything outside the n_left * W entries: a fresh buffer keeps what
 *     it held there.  A gather that repeats a row pairs it with itself (a diagonal table).  K == 0 is valid: tables are all zero,
 *     r^2 is NaN.  n_left == 0 or n_variants <= 1 is a no-op.
 *   - PGENHIP_ERR_BAD_ARG: window == 0, n_left > n_variants, an unknown flag, and — when at least one pair exists — a NULL or
 *     misaligned d_out.  PGENHIP_ERR_TOO_LARGE before any launch when n_left * window * 64 >= 2^52.
 * Same launch contract as pgenhip_genotype_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable.  One pair's samples are not split over blocks: a call with few rows of very long records uses few CUs. */
#define PGENHIP_PAIR_TABLE 0u   /* 16 u32 per pair */
#define PGENHIP_PAIR_R2    1u   /* one f32 per pair */
int pgenhip_pair_stats(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                       uint32_t n_variants, uint32_t n_left, uint32_t window, void *d_out, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_pair_stats_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                          uint32_t n_left, uint32_t window, void *d_out, uint32_t flags);

/* ---- LD pruning: one bit per pair, and the greedy independent set of the graph they form (device-resident, asynchronous) ----
 * pgenhip_pair_mask: rows, pairs, n_left, window = W and the kept samples are exactly those of pgenhip_pair_stats / _at; the pair
 * (i, j = i + d) exists for i < n_left, 1 <= d <= W, j < n_variants.  An existing pair is an EDGE iff
 *   - the f32 value PGENHIP_PAIR_R2 defines for it compares > min_r2 (the same formula: exact u64 terms, doubles, one rounding;
 *     NaN is never an edge), and
 *   - d_key == NULL, or (d_key[j] - d_key[i]) mod 2^64 <= max_span.  d_key is a DEVICE array of u64 indexed by the row's position in
 *     the selection; the library does not interpret it.  A host passes (chromosome rank << 32) | POS: a pair across chromosomes, or
 *     out of order, is then never an edge, and with POS left 0 and max_span = 0 a window in variants still stops at chromosome ends.
 * With b = d - 1, an edge sets bit b & 31 of d_fwd[i * mask_stride + b / 32] and, when d_bwd != NULL, the same bit of
 * d_bwd[j * mask_stride + b / 32].  mask_stride is in u32 words, >= ceil(W / 32).  The call only ever SETS bits (integer OR, so any
 * order gives the same words), clears nothing, and writes nothing outside the words that hold an edge's bit: row padding and the
 * words of rows without an edge are untouched.  The caller zeroes the masks once and calls per block with d_fwd / d_bwd advanced by
 * block_row0 * mask_stride, so the halo rows of a block land on the next block's rows of d_bwd.  flags must be 0.
 *   - PGENHIP_ERR_BAD_ARG: window == 0, n_left > n_variants, min_r2 NaN, d_key not 8-byte aligned, unknown flags, and — when a pair
 *     exists — d_fwd NULL, a mask not 4-byte aligned, mask_stride < ceil(W / 32) when more than one mask row is addressed.
 *   - PGENHIP_ERR_TOO_LARGE before any launch when n_variants * mask_stride * 4 >= 2^52.
 * Launch contract as for pgenhip_pair_stats: device pointers only, no allocation, no synchronisation, one kernel on the ctx stream,
 * graph-capturable, masks in ordinary device memory; PGENHIP_KNOB_PAIR_BLOCKS forces its grid too.
 *
 * pgenhip_prune_resolve: the neighbours of row v are v + d for the bits d - 1 set in d_fwd's row v and v - d for the bits set in
 * d_bwd's row v (rows of mask_stride words each); only 1 <= d <= window and neighbours in [0, n_rows) count, bits that point outside
 * are ignored, never followed.  Row u BEATS v iff d_priority[u] > d_priority[v], or the two are equal and u < v (d_priority == NULL:
 * the lower index wins).  The answer S: take the rows in beating order; a row whose d_state byte the caller pre-set to KEPT or REMOVED
 * has that state; any other row is KEPT iff none of its neighbours that beat it is KEPT, else REMOVED.  S is unique.  One call
 *   (a) never changes a non-zero state and never writes a state that differs from S;
 *   (b) decides at least one row if any is undecided when it starts (a host loop ends after at most n_rows calls);
 *   (c) overwrites *d_undecided (DEVICE u64) with the exact number of rows still undecided when it ends.
 * The host loops call -> D2H of the counter -> repeat until the counter is 0.  n_rows == 0 writes 0 to the counter and nothing else
 * (a NULL d_undecided is accepted then, and nothing at all is written).
 * State bytes other than 0, 1, 2 give an unspecified result without any out-of-bounds access; so does a d_bwd that is not the
 * transpose of d_fwd (some consistent-looking result).  flags: a shape; every shape takes every legal call and ends at the same S.
 *   - PGENHIP_ERR_BAD_ARG: window == 0; with n_rows > 0 a NULL d_fwd / d_bwd / d_state / d_undecided; masks or d_priority not 4-byte
 *     aligned, d_undecided not 8-byte aligned; mask_stride < ceil(window / 32) with n_rows > 1; unknown flags or shapes.
 *   - PGENHIP_ERR_TOO_LARGE: n_rows * mask_stride * 4 >= 2^52.
 * Device pointers only, no allocation, no synchronisation; one 8-byte memset and one kernel on the ctx stream; graph-capturable. */
int pgenhip_pair_mask(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                      uint32_t n_variants, uint32_t n_left, uint32_t window, float min_r2, const uint64_t *d_key, uint64_t max_span,
                      uint32_t *d_fwd, uint32_t *d_bwd, uint64_t mask_stride, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_pair_mask_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants, uint32_t n_left,
                         uint32_t window, float min_r2, const uint64_t *d_key, uint64_t max_span, uint32_t *d_fwd, uint32_t *d_bwd,
                         uint64_t mask_stride, uint32_t flags);
#define PGENHIP_PRUNE_UNDECIDED 0u
#define PGENHIP_PRUNE_KEPT 1u
#define PGENHIP_PRUNE_REMOVED 2u
#define PGENHIP_PRUNE_AUTO 0u
#define PGENHIP_PRUNE_GENERAL 1u   /* a lane per row, one sweep per call: the correctness baseline */
#define PGENHIP_PRUNE_BLOCK 2u     /* a workgroup per range of rows, swept to a local fixed point in LDS */
int pgenhip_prune_resolve(pgenhip_ctx *ctx, const uint32_t *d_fwd, const uint32_t *d_bwd, uint64_t mask_stride, uint32_t window,
                          uint64_t n_rows, const uint32_t *d_priority, uint8_t *d_state, uint64_t *d_undecided, uint32_t flags);

/* ---- pairwise sample tables (device-resident, asynchronous on the ctx stream) ----
 * The transpose of pgenhip_pair_stats: pairs of kept SAMPLES, summed over the selected rows.  Rows are selected exactly as in
 * pgenhip_sample_counts / pgenhip_sample_counts_at (by stride with record_stride >= R or n_variants <= 1, through d_variant_idx, or
 * through d_record_off; any byte alignment; a gather that repeats a row counts it twice).  [a_begin, a_begin + a_count) and
 * [b_begin, b_begin + b_count) are ranges of RANKS in the ctx's kept list (a rank is the sample index when all samples are kept);
 * they may be equal, overlap, be disjoint or come in either order.  For a = a_begin + i and b = b_begin + l sixteen u32 go to
 *     d_out[16 * (i * b_count + l) + 4 * x + y] = the number of selected rows in which sample a has code x and sample b has code y
 * with codes 0 hom-ref, 1 het, 2 hom-alt, 3 missing (the order of the count entry points).  The sums over y are a's
 * pgenhip_sample_counts over the same rows, the sums over x are b's, a table sums to n_variants, T(a, a) is diagonal and
 * T(b, a)[y][x] == T(a, b)[x][y], so a host that covers K x K with rectangles needs the upper block triangle only.  The library
 * does not interpret the tables: KING kinship, IBS distances and X^T X are host arithmetic on them.  The pad bits of a record's
 * last byte and samples >= N are never read as samples.
 *   - Without PGENHIP_SPAIR_ACCUMULATE the call overwrites the 16 * a_count * b_count entries (zeros when n_variants == 0).  With it
 *     the counts are added to what d_out holds, so a host sums blocks of rows in place; n_variants == 0 is then a no-op.  Counts
 *     are exact integers, reproducible from run to run whatever order blocks combine in, and wrap modulo 2^32 only past 2^32 - 1
 *     counted rows.  Nothing outside the entries is written; a_count == 0 or b_count == 0 writes nothing and returns PGENHIP_OK.
 *   - PGENHIP_ERR_BAD_ARG: a range that ends past K; d_out NULL or not 16-byte aligned when at least one entry exists; unknown flag
 *     bits or shape ids.  PGENHIP_ERR_TOO_LARGE, before any launch: a_count * b_count * 64 >= 2^52, and the record byte offsets that
 *     pgenhip_decode_matrix refuses.
 * Same launch contract as pgenhip_sample_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable (the overwrite is a hipMemsetAsync ahead of the kernel).  The kernels use no work-queue counters, so these
 * launches do not count against PGENHIP_LAUNCHES_IN_FLIGHT.
 * flags: a shape (PGENHIP_SPAIR_AUTO or a forced one; both forced shapes take every legal call) | PGENHIP_SPAIR_ACCUMULATE. */
#define PGENHIP_SPAIR_AUTO 0u
#define PGENHIP_SPAIR_GENERAL 1u      /* a lane per pair, row by row: the correctness baseline */
#define PGENHIP_SPAIR_MFMA 2u         /* int8 matrix cores on 0/1 indicator vectors, 64 x 64 samples per block */
#define PGENHIP_SPAIR_SHAPE_MASK 0xFu
#define PGENHIP_SPAIR_ACCUMULATE 0x10u
int pgenhip_sample_pair_stats(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                              uint32_t n_variants, uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count,
                              uint32_t *d_out, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_sample_pair_stats_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                                 uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count, uint32_t *d_out,
                                 uint32_t flags);

/* ---- sample Gram matrix (device-resident, asynchronous on the ctx stream) ----
 * The weighted member of the family whose integer member is pgenhip_sample_pair_stats: Z^T Z in FP64, where every selected row has its
 * own value for each of the four codes.  Rows are selected exactly as in pgenhip_sample_pair_stats / _at (by stride with
 * record_stride >= R or n_variants <= 1, through d_variant_idx, or through d_record_off; any byte alignment; a gather that repeats a
 * row adds it twice).  [a_begin, a_begin + a_count) and [b_begin, b_begin + b_count) are ranges of RANKS in the ctx's kept list (a
 * rank is the sample index when all samples are kept); they may be equal, overlap, be disjoint or come in either order.  For
 * a = a_begin + i and b = b_begin + l
 *     d_out[i * out_stride + l] = sum over the selected rows j of t_j[x_j(a)] * t_j[x_j(b)]
 * where x_j(s) is the 2-bit code of sample s in row j (0 hom-ref, 1 het, 2 hom-alt, 3 missing) and t_j = d_code_values[4*j .. 4*j+3],
 * a DEVICE array of FP64 indexed by the row's POSITION IN THE SELECTION (as d_weights of pgenhip_sample_scores is).  The library
 * does not interpret the table: a standardised GRM ((0-2p)s, (1-2p)s, (2-2p)s, 0), a dominance GRM, a raw dosage cross-product
 * (0, 1, 2, 0) and the number of rows called in both samples (1, 1, 1, 0) are all "four doubles per row".  out_stride is in doubles,
 * >= b_count (or a_count <= 1).  The result is mathematically symmetric when the two ranges are equal; the library does not exploit
 * that, and a host covers K x K with the upper block triangle.  The pad bits of a record's last byte and samples >= N are never read
 * as samples.
 *   - Arithmetic.  Every product and every addition is FP64; there are no f32 partial sums.  The order of the additions is not fixed
 *     (rows are dealt to blocks and accumulator chains, which meet in atomics).  Each entry is within (n_variants + 2) * 2^-53 *
 *     A(a, b) of the exact sum, A(a, b) = sum over j of |t_j[x_j(a)] * t_j[x_j(b)]|: one rounding per product and n_variants - 1
 *     additions, to first order, with room to spare.  Sums whose every partial sum is an integer below 2^53 are exact in any order.
 *     Non-finite table entries give unspecified results.  Bitwise run-to-run reproducibility is not promised.
 *   - Without PGENHIP_GRAM_ACCUMULATE the call overwrites exactly the a_count x b_count entries (zeros when n_variants == 0).  With
 *     it the sums are added to what d_out holds, so a host sums blocks of rows in place; n_variants == 0 is then a no-op.  Row
 *     padding and everything else are not touched; a_count == 0 or b_count == 0 writes nothing and returns PGENHIP_OK.
 *   - d_out must be ORDINARY device memory (hipMalloc, pgenhip_device_malloc), not fine-grained or host-mapped memory: the
 *     kernel adds with hardware FP64 atomics, which such memory does not serve.
 *   - PGENHIP_ERR_BAD_ARG: a range that ends past K; d_code_values NULL with n_variants > 0, or not 8-byte aligned; d_out NULL or not
 *     8-byte aligned when at least one entry exists; out_stride < b_count with a_count > 1; unknown flag bits or shape ids; a forced
 *     shape that does not apply (both shapes take every legal call today).  PGENHIP_ERR_TOO_LARGE, before any launch:
 *     a_count * out_stride * 8 >= 2^52, n_variants * 32 >= 2^52, and the record byte offsets that pgenhip_decode_matrix refuses.
 *     Nothing is written or launched on a refusal.
 * Same launch contract as pgenhip_sample_pair_stats: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable (the overwrite is a zeroing memset ahead of the kernel).  The kernels use no work-queue counters, so these
 * launches do not count against PGENHIP_LAUNCHES_IN_FLIGHT.
 * flags: a shape (PGENHIP_GRAM_AUTO or a forced one) | PGENHIP_GRAM_ACCUMULATE. */
#define PGENHIP_GRAM_AUTO 0u
#define PGENHIP_GRAM_GENERAL 1u       /* a lane per pair, FP64 multiply-add along the rows: the correctness baseline */
#define PGENHIP_GRAM_MFMA 2u          /* FP64 matrix cores (v_mfma_f64_16x16x4_f64), 64 x 64 ranks per block: what AUTO takes */
/* 3u is reserved for a matrix-core form with f32 operands (not built; refused with PGENHIP_ERR_BAD_ARG) */
#define PGENHIP_GRAM_SHAPE_MASK 0xFu
#define PGENHIP_GRAM_ACCUMULATE 0x10u
int pgenhip_sample_gram(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                        uint32_t n_variants, const double *d_code_values, uint32_t a_begin, uint32_t a_count, uint32_t b_begin,
                        uint32_t b_count, double *d_out, uint64_t out_stride, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_sample_gram_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                           const double *d_code_values, uint32_t a_begin, uint32_t a_count, uint32_t b_begin, uint32_t b_count,
                           double *d_out, uint64_t out_stride, uint32_t flags);

/* ---- Gram product (device-resident, asynchronous on the ctx stream) ----
 * (Z^T Z) Q without Z^T Z: what an eigen-solver iterates (principal components) when the K x K matrix of pgenhip_sample_gram does not
 * fit.  Rows are selected exactly as in pgenhip_sample_gram / _at (by stride with record_stride >= R or n_variants <= 1, through
 * d_variant_idx, or through d_record_off; any byte alignment; a gather that repeats a row adds it twice).  With
 *     Z[j][k] = t_j[x_j(k)]
 * where x_j(k) is the 2-bit code, in selected row j, of the sample of rank k in the ctx's kept list (0 hom-ref, 1 het, 2 hom-alt,
 * 3 missing) and t_j = d_code_values[4*j .. 4*j+3] (the table argument of pgenhip_sample_gram: a DEVICE array of FP64 indexed by the
 * row's POSITION IN THE SELECTION, not interpreted by the library), the call computes over ALL K kept samples
 *     d_proj[j * n_columns + c] = P[j][c] = sum over k of Z[j][k] * d_q[k * q_stride + c]        (always overwritten)
 *     d_out[k * out_stride + c] = Y[k][c] = sum over j of Z[j][k] * P[j][c]
 * for c < n_columns <= PGENHIP_GAPPLY_MAX_COLUMNS.  q_stride and out_stride are in doubles, >= n_columns (or K <= 1).  d_proj, the
 * variants' projections, is a documented output: rows are the unit a host blocks over, as in pgenhip_variant_sums, and it is the only
 * intermediate, so no hidden scratch exists.  The pad bits of a record's last byte and samples >= N are never read as samples.
 *   - Arithmetic.  Every product and every addition is FP64; there are no f32 partial sums.  The order of the additions is not fixed
 *     (samples and rows are dealt to lanes, blocks and accumulator chains, which meet in atomics).  To first order, with room to
 *     spare: P[j][c] is within (K + 1) * 2^-53 * sum over k of |Z[j][k] * q[k][c]| of the exact sum, and Y[k][c] is within
 *     (n_variants + K + 4) * 2^-53 * B(k, c) of it, B(k, c) = sum over j of |Z[j][k]| * sum over k' of |Z[j][k'] * q[k'][c]|.  Sums
 *     whose every partial sum is an integer below 2^53 are exact in any order.  Non-finite input gives unspecified results.  Bitwise
 *     run-to-run reproducibility is not promised.
 *   - Without PGENHIP_GAPPLY_ACCUMULATE the call overwrites exactly the K x n_columns entries of d_out (zeros when n_variants == 0).
 *     With it Y is added to what d_out holds, so a host sums blocks of rows in place; n_variants == 0 is then a no-op.  Row padding
 *     and everything else are not touched.  K == 0 writes zeros to d_proj and nothing to d_out.
 *   - d_out and d_proj must be ORDINARY device memory (hipMalloc, pgenhip_device_malloc), not fine-grained or host-mapped memory:
 *     the kernels add with hardware FP64 atomics, which such memory does not serve.  d_q, d_proj and d_out must not overlap.
 *   - PGENHIP_ERR_BAD_ARG: n_columns 0 or above 16; q_stride < n_columns or out_stride < n_columns with K > 1; d_code_values, d_q,
 *     d_proj or d_out NULL or not 8-byte aligned where at least one element would be read or written; unknown flag bits or shape
 *     ids.  PGENHIP_ERR_TOO_LARGE, before any launch: K * q_stride * 8, K * out_stride * 8 or n_variants * n_columns * 8 of 2^52 or
 *     more, and the record byte offsets that pgenhip_decode_matrix refuses.  Nothing is written or launched on a refusal.  (With a
 *     32-bit n_variants and at most 16 columns n_variants * n_columns * 8 stays below 2^40: that refusal cannot be reached through
 *     this ABI version and no test can provoke it; it is stated, and checked, for the day either type widens.)
 * Same launch contract as pgenhip_sample_gram: device pointers only, no allocation, no synchronisation, queued on the ctx stream,
 * graph-capturable (zeroing memsets ahead of two kernels).  The kernels use no work-queue counters, so these launches do not count
 * against PGENHIP_LAUNCHES_IN_FLIGHT.
 * flags: a shape (PGENHIP_GAPPLY_AUTO or a forced one; both take every legal call) | PGENHIP_GAPPLY_ACCUMULATE. */
#define PGENHIP_GAPPLY_MAX_COLUMNS 16u
#define PGENHIP_GAPPLY_AUTO 0u
#define PGENHIP_GAPPLY_GENERAL 1u     /* correctness baseline, any shape */
#define PGENHIP_GAPPLY_MFMA 2u        /* v_mfma_f64_16x16x4_f64 in both passes */
#define PGENHIP_GAPPLY_SHAPE_MASK 0xFu
#define PGENHIP_GAPPLY_ACCUMULATE 0x10u
int pgenhip_gram_apply(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                       uint32_t n_variants, const double *d_code_values, const double *d_q, uint64_t q_stride,
                       uint32_t n_columns, double *d_proj, double *d_out, uint64_t out_stride, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_gram_apply_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                          const double *d_code_values, const double *d_q, uint64_t q_stride, uint32_t n_columns,
                          double *d_proj, double *d_out, uint64_t out_stride, uint32_t flags);

/* ---- packed records of the kept samples (device-resident, asynchronous on the ctx stream) ----
 * The selection written back as records: row j of the output is the mode-0x02 record of a K-sample file that holds the ctx's kept
 * samples of selected row j, so a host that puts the 12-byte header in front has a .pgen of the subset (src/pfile.rs:172-175 read
 * backwards).  Rows are selected exactly as in pgenhip_decode_emit / pgenhip_decode_emit_at: by stride (record_stride >= R, or
 * n_variants <= 1), through d_variant_idx, or through d_record_off; records may start at any byte alignment; a gather that repeats
 * a row writes it twice.
 *   - Row j is R_K = ceil(K / 4) bytes (pgenhip_packed_record_size) at d_out + j*out_stride: the code of kept sample k in byte k/4,
 *     bits 2*(k%4), LSB first; k is the sample's rank in the ctx's kept list (its index when all samples are kept).  The pad bits
 *     of the last byte are always written as zero, whatever the input's pad bits and code_map hold.  Samples >= N are never read
 *     as samples.
 *   - out_stride >= R_K (or n_variants <= 1); any alignment of d_out, any out_stride.  Bytes of d_out outside the n_variants x R_K
 *     record bytes (row padding included) are not touched.  n_variants == 0 or K == 0 writes nothing and is PGENHIP_OK.
 *   - code_map is a HOST pointer to four bytes, the 2-bit code written for input codes 0, 1, 2, 3; it is read during the call and
 *     passed as kernel arguments (no device copy, no allocation; a captured graph keeps the map it was captured with).  NULL is the
 *     identity; a value > 3 is PGENHIP_ERR_BAD_ARG.  The library does not interpret the map: {3, 2, 0, 1} is the PLINK 1 .bed coding
 *     with ALT as A1 (00 hom A1, 01 missing, 10 het, 11 hom A2).
 *   - Shapes (flags; anything else is PGENHIP_ERR_BAD_ARG).  GENERAL applies always: one output byte per lane, four gathered codes.
 *     DENSE: all samples kept (no list, or the identity list).  GATHER: the ctx was created with a kept list (an identity list
 *     counts) of K >= 1 samples.  A forced shape that does not apply is PGENHIP_ERR_BAD_ARG with a detail string, also on a call that
 *     would write nothing; AUTO takes DENSE or GATHER where they apply and GENERAL otherwise.
 *   - PGENHIP_ERR_TOO_LARGE before any launch for offsets of 2^52 bytes or more, as in pgenhip_decode_matrix: out_stride times
 *     n_variants, record_stride times n_variants without a gather, record_stride itself with d_variant_idx.
 * Same launch contract as pgenhip_genotype_counts: device pointers only, no allocation, no synchronisation, queued on the ctx
 * stream, graph-capturable.  Every output byte has one owner: no atomics and no work counters, so these launches do not count
 * against PGENHIP_LAUNCHES_IN_FLIGHT. */
#define PGENHIP_PACK_AUTO 0u
#define PGENHIP_PACK_GENERAL 1u   /* any K, any layout: the correctness baseline */
#define PGENHIP_PACK_DENSE 2u     /* all samples kept: a record copy between two byte phases */
#define PGENHIP_PACK_GATHER 3u    /* a kept list, K >= 1: output-driven, one output dword per lane */
uint32_t pgenhip_packed_record_size(const pgenhip_ctx *ctx);   /* ceil(K / 4); 0 for a NULL ctx */
int pgenhip_pack_records(pgenhip_ctx *ctx, const void *d_records, uint64_t record_stride, const uint32_t *d_variant_idx,
                         uint32_t n_variants, void *d_out, uint64_t out_stride, const uint8_t *code_map, uint32_t flags);
/* Same, with the record of row j at d_base + d_record_off[j] (DEVICE array of u64 byte offsets). */
int pgenhip_pack_records_at(pgenhip_ctx *ctx, const void *d_base, const uint64_t *d_record_off, uint32_t n_variants,
                            void *d_out, uint64_t out_stride, const uint8_t *code_map, uint32_t flags);

/* ---- GT text to records (device-resident, asynchronous on the ctx stream) ----
 * The inverse of pgenhip_decode_emit: for every line j of a text buffer the sample fields become the line's mode-0x02 record of the
 * ctx's N samples (sample s in byte s/4, bits 2*(s%4), LSB first; pad bits zero), so a host that puts the 12-byte header in front
 * of the rows has a .pgen of a VCF's GT calls.  The ctx must keep all samples (no list, or the identity list); a proper subset is
 * PGENHIP_ERR_BAD_ARG with a detail string: subsetting is pgenhip_pack_records' job.
 *
 * Grammar.  The sample region of line j is text[d_field_off[j], d_line_end[j]): a sequence of fields, each introduced by a '\t';
 * the tab at d_field_off[j] introduces sample 0.  A field's GT is its bytes up to the first ':', or the whole field.  An allele is
 * one or more bytes of 0-9, or the single byte '.'.  A GT is `A` (haploid) or `A S B` (diploid) with S one of '/' and '|'.
 *   - A GT of neither form (empty, three alleles, other bytes) sets BAD_CALL; otherwise a digit token other than exactly "0" and
 *     "1" ("2", "10", "01") sets ALLELE_RANGE.  In both cases the sample's code is 3 and the field sets no other flag.
 *   - Otherwise: diploid, both called: a + b; diploid with a '.': 3, and HALF_CALL if only one is; haploid: "0" 0, "1" 2, "." 3, and
 *     HAPLOID; a '|' sets PHASED (the phase is dropped).
 *   - Fields with ordinal >= N are ignored and set FIELD_COUNT; samples without a field get code 3 and set FIELD_COUNT.  A region
 *     that is empty or does not begin with a tab has no fields.
 * Shapes (flags & PGENHIP_PARSE_SHAPE_MASK; other bits and values are PGENHIP_ERR_BAD_ARG).  GENERAL takes fields of any width; a
 * block per line, so a call with few very long lines uses few CUs.  FIXED takes the lines this library's own emit path writes — a
 * region of exactly 4N bytes, every field `\t[01.][/|][01.]` — flat over the launch's bytes; any other line is declined as a whole:
 * PGENHIP_PARSE_DECLINED is its only flag and its record bytes are not touched.  AUTO
 * runs FIXED and then GENERAL on the declined lines: its records and flags equal GENERAL's bit for bit on every input.
 *   - Row j is the R = ceil(N / 4) bytes at d_out + j*out_stride, out_stride >= R or n_lines <= 1; d_out may have any alignment.
 *     d_line_flags[j] is always overwritten.  Nothing outside the n_lines x R record bytes and the n_lines flag words is written.
 *   - Nothing outside [d_text, d_text + text_len) is read: offsets past text_len are clamped to it, d_field_off[j] > d_line_end[j]
 *     is an empty region.  d_text may have any alignment.
 *   - n_lines == 0 is a no-op.  Refused before any launch, everything untouched: PGENHIP_ERR_BAD_ARG for a NULL pointer where an
 *     element would be touched, d_line_flags not 4-byte aligned, offset arrays not 8-byte aligned, a stride below R, unknown flag
 *     bits or shapes; PGENHIP_ERR_TOO_LARGE for out_stride * n_lines >= 2^52.  Malformed text is data, reported in the flags.
 * Same launch contract as pgenhip_pack_records: device pointers only, no allocation, no synchronisation, queued on the ctx stream
 * (a memset of the flag words and up to two kernels), graph-capturable, no work counters: not counted against
 * PGENHIP_LAUNCHES_IN_FLIGHT. */
#define PGENHIP_PARSE_AUTO 0u
#define PGENHIP_PARSE_GENERAL 1u
#define PGENHIP_PARSE_FIXED 2u
#define PGENHIP_PARSE_SHAPE_MASK 0xFu
/* per-line flag bits */
#define PGENHIP_PARSE_FIELD_COUNT  0x01u
#define PGENHIP_PARSE_BAD_CALL     0x02u
#define PGENHIP_PARSE_ALLELE_RANGE 0x04u
#define PGENHIP_PARSE_HALF_CALL    0x08u   /* informational */
#define PGENHIP_PARSE_HAPLOID      0x10u   /* informational */
#define PGENHIP_PARSE_PHASED       0x20u   /* informational */
#define PGENHIP_PARSE_DECLINED     0x40u   /* forced FIXED only: line not taken, its record bytes not touched */
int pgenhip_parse_gt(pgenhip_ctx *ctx, const void *d_text, uint64_t text_len,
                     const uint64_t *d_field_off, const uint64_t *d_line_end, uint32_t n_lines,
                     void *d_out, uint64_t out_stride, uint32_t *d_line_flags, uint32_t flags);

/* ---- sample-wise join of records (device-resident, asynchronous on the ctx stream) ----
 * The inverse of pgenhip_pack_records' sample selection: row j of the output is the mode-0x02 record of N_out = sum of the parts'
 * sample_count samples, the samples of part 0 first, then part 1, and so on: output sample start_p + s (s < n_p) is sample s of part
 * p's record for row j, the record at d_base + d_record_off[j] (ceil(n_p / 4) bytes, any alignment).  So a host that puts the 12-byte
 * header in front of the rows has a .pgen of several filesets' samples side by side.
 *   - A part whose d_record_off[j] is PGENHIP_JOIN_ABSENT has no record for row j: its n_p samples get code 3 and nothing of the
 *     part is read for that row.  Two rows may name the same record.
 *   - A part with a d_flip array has codes 0 and 2 exchanged in the rows with d_flip[j] != 0 (REF and ALT the other way round in
 *     that part); codes 1 and 3 stay.
 *   - The pad bits of the output's last byte are always written as zero.  The pad bits of a part's last record byte are never
 *     read as samples, whatever they hold.
 *   - The ctx must keep all samples (no list, or the identity list), as for pgenhip_parse_gt, and its sample count must equal the
 *     sum of the parts' sample_count (summed in 64 bits).  A part with sample_count 0 is legal: it adds nothing and its pointers are
 *     not touched.
 *   - Row j is the R = ceil(N_out / 4) bytes at d_out + j*out_stride, out_stride >= R or n_variants <= 1; d_out and the records
 *     may have any alignment.  Nothing outside the n_variants x R record bytes is written: row padding is untouched.
 *   - Of a part, only aligned 16-byte chunks that hold a byte of a present row's ceil(n_p / 4)-byte record may be loaded (the
 *     kernels as built load record bytes only), and its n_variants offsets and flip bytes.
 *   - n_variants == 0 or N_out == 0 writes nothing and is PGENHIP_OK.
 *   - Shapes (flags; other bits and values are PGENHIP_ERR_BAD_ARG).  GENERAL: a lane per output byte, the correctness baseline.
 *     STREAM: a lane per aligned 16-byte chunk of an output row, its source bytes read at the part's own bit phase.  Both take any
 *     part sizes; their bytes are equal.  AUTO takes STREAM.
 *   - Refused before any launch, d_out untouched.  PGENHIP_ERR_BAD_ARG, with a detail string: parts NULL; n_parts 0 or above
 *     PGENHIP_JOIN_MAX_PARTS; a part's reserved != 0; a sample sum other than the ctx's N; a ctx with a proper subset; a part with
 *     sample_count > 0 and a NULL d_base or d_record_off while n_variants > 0; a d_record_off not 8-byte aligned; d_out NULL where a
 *     byte would be written; out_stride < R with n_variants > 1; unknown flags.  PGENHIP_ERR_TOO_LARGE for out_stride * n_variants
 *     >= 2^52.
 * `parts` is a HOST array, read during the call and passed as kernel arguments (no device copy, no allocation; a captured graph
 * keeps the table it was captured with).  Same launch contract as pgenhip_pack_records: device pointers only, no allocation, no
 * synchronisation, queued on the ctx stream (one kernel), graph-capturable.  Every output byte has one owner: no atomics and no
 * work counters, so these launches do not count against PGENHIP_LAUNCHES_IN_FLIGHT. */
#define PGENHIP_JOIN_MAX_PARTS 8u
#define PGENHIP_JOIN_ABSENT UINT64_MAX
typedef struct pgenhip_join_part {
    const void *d_base;            /* DEVICE */
    const uint64_t *d_record_off;  /* DEVICE, n_variants byte offsets from d_base; PGENHIP_JOIN_ABSENT = no such row in this part */
    const uint8_t *d_flip;         /* DEVICE, n_variants bytes, or NULL (no row flipped) */
    uint32_t sample_count;         /* n_p; 0 is legal: the part adds nothing and its pointers are not touched */
    uint32_t reserved;             /* must be 0 */
} pgenhip_join_part;
#define PGENHIP_JOIN_AUTO 0u
#define PGENHIP_JOIN_GENERAL 1u   /* one lane per output byte: the correctness baseline */
#define PGENHIP_JOIN_STREAM 2u    /* output-driven: one aligned 16-byte chunk of an output row per lane */
int pgenhip_join_records(pgenhip_ctx *ctx, const pgenhip_join_part *parts, uint32_t n_parts, uint32_t n_variants,
                         void *d_out, uint64_t out_stride, uint32_t flags);

/* Pure host function: the lines of a block of VCF body text, for pgenhip_parse_gt.  Per complete line i < *n_lines (a line ends
 * with '\n'; with PGENHIP_VCF_LAST_BLOCK a non-empty remainder without one counts as a line that ends at text_len):
 *   line_start[i]  the line's first byte
 *   format_off[i]  the first byte of column format_col (columns are separated by '\t', column 0 starts the line)
 *   field_off[i]   the tab that ends that column; line_end[i] when the line has exactly format_col + 1 columns; UINT64_MAX (as
 *                  format_off[i] is then) when it has fewer, which the caller turns into an error
 *   line_end[i]    the offset of the '\n', or of a '\r' directly before it
 * Stops after max_lines lines (the arrays' length).  *consumed is the offset just past the last line reported, so the caller can
 * carry the remainder into its next block.  PGENHIP_ERR_BAD_ARG for a NULL array or counter, a NULL text with text_len != 0, or
 * unknown flags. */
#define PGENHIP_VCF_LAST_BLOCK 1u   /* a final line without '\n' counts */
int pgenhip_vcf_index_lines(const uint8_t *text, uint64_t text_len, uint32_t format_col, uint64_t max_lines, uint32_t flags,
                            uint64_t *line_start, uint64_t *format_off, uint64_t *field_off, uint64_t *line_end,
                            uint64_t *n_lines, uint64_t *consumed);

/* Launch-shape knobs of one ctx (tests force small grids to exercise ring re-use; A/B probes).
 * value 0 restores the built-in default of a knob unless noted. */
typedef enum pgenhip_knob {
    PGENHIP_KNOB_WIDE_BLOCKS_PER_CU = 1, /* stream kernel: resident blocks per CU (default: occupancy API; two on launches of up to 1 GB of text, and on launches of short rows, N < 1 916, of up to 3 GB) */
    PGENHIP_KNOB_WIDE_RANGES = 2,        /* stream kernel: work-queue ranges (write fronts of a launch), a power of two up to 64; default 0 = by shape (8 for rows of more than 16 KiB of text and for launches of more than 3 GB of short rows, N < 1 916, else 2) */
    PGENHIP_KNOB_FLAT_BLOCKS_PER_CU = 3, /* flat kernel: grid cap per CU (default 64) */
    PGENHIP_KNOB_SCAN_BLOCKS_PER_CU = 4, /* segment kernel: resident blocks per CU (default: 2 from ~0.6 % kept, else the occupancy API's 3) */
    /* 5 was the band override of round 1's three-segment gather kernel (removed) */
    PGENHIP_KNOB_PICK_BATCH_BYTES = 6,   /* short-record pick kernel: text bytes per batch (default 32768) */
    PGENHIP_KNOB_SCAN_XCD_MAP = 8,       /* segment kernels: 1 (default) all blocks of a row group on one XCD, -1 plain block map */
    PGENHIP_KNOB_SCAN_TWO_PASS = 9,      /* sparse keeps on long records: 1 (default) compact pass + all-samples pass, -1 single-pass segment kernel */
    PGENHIP_KNOB_SCAN_CHUNK_ROWS = 10,   /* two-pass path: rows per chunk (default: as many as the launch's 32-MiB compact-scratch slice holds) */
    PGENHIP_KNOB_ROWPICK_BLOCKS_PER_CU = 11, /* row-owner kernel: cap on resident blocks per CU (default: occupancy API) */
    PGENHIP_KNOB_SCAN_ROWPICK = 12,      /* kept subsets on long records, launches of many rows: 1 (default, and any value >= 0) the row-owner kernel where it measures ahead (text in one pass for 2-20 % kept and for records of barely more than one segment; compact pass of the two passes below 2 %), -1 never (segment kernels) */
    /* 13-15 selected flush forms AUTO never took (row-by-row full lines, 1 / 4 chunks per lane and step, five picks per chunk):
       retired, refused with PGENHIP_ERR_BAD_ARG, never reused */
    PGENHIP_KNOB_ALIGN_STORES = 16,      /* subset kernels (segment, row-owner, pick): 1 (default) lanes <-> chunks shifted so that every store instruction covers whole 128-byte lines, -1 from the run's first whole chunk */
    PGENHIP_KNOB_SCOUNT_SLICES = 17,     /* per-sample counts: row ranges per column tile, each summed by one block (default 0 = as many as fill the chip's resident blocks) */
    PGENHIP_KNOB_MATRIX_BLOCKS = 18,     /* genotype matrix kernels: grid size in blocks (default 0 = by shape: the work, capped at 8 blocks per CU, 4 for TILE); tests force small grids */
    PGENHIP_KNOB_PAIR_BLOCKS = 19,       /* pairwise kernel: grid size in blocks (default 0 = by shape: the tiles, capped at 16 one-wave blocks per CU); tests force small grids */
    PGENHIP_KNOB_PACK_BLOCKS = 20,       /* pack kernels: grid size in blocks (default 0 = by shape: the work, capped at 8 blocks per CU); tests force small grids */
    PGENHIP_KNOB_SCORE_SLICES = 21,      /* per-sample scores: row ranges per column tile, each summed by one block (default 0 = by shape: as many as fill the chip's resident blocks, of at least 512 rows each); tests put the row count on either side of every plan edge */
    PGENHIP_KNOB_SPAIR_SLICES = 22,      /* pairwise sample tables: row ranges per sample tile, each summed by one block (default 0 = by shape: as many as fill the chip's resident blocks, of at least 256 rows each); tests put the row count on either side of every slice edge */
    PGENHIP_KNOB_VSUM_BLOCKS = 23,       /* per-variant sums: grid size in blocks (default 0 = by shape: the work, capped at 8 blocks per CU); the MFMA shape also cuts the rows into that many slices, so tests force small grids and the multi-block combine */
    PGENHIP_KNOB_STORE_POLICY = 24,      /* stream kernel (row items, full lines through it, RUNS): how the text is stored. 0 (default) the measured rule: non-temporal write-through stores (sc1 nt: the line leaves the L2 with the store) on launches of more than 1 GB of text whose rows span several 16-KiB work items, or one and up to 4.5 GB; non-temporal stores elsewhere. 1 non-temporal stores everywhere, 2 write-through stores everywhere (tests force both at small sizes; A/B probes); other values are refused. The other emit kernels store as before whatever the value */
    PGENHIP_KNOB_GRAM_SLICES = 25,       /* sample Gram matrix: row ranges per rank tile, each summed by one block (default 0 = by shape: as many as fill the chip's resident blocks, of at least 256 rows each); tests put the row count on either side of every slice edge */
    PGENHIP_KNOB_GAPPLY_SAMPLE_SLICES = 26, /* Gram product, P pass: sample ranges per row tile, each summed by one block (default 0 = by shape: as many as fill the chip's resident blocks, of at least 4096 samples each); tests put the sample count on either side of every slice edge */
    PGENHIP_KNOB_GAPPLY_ROW_SLICES = 27, /* Gram product, Y pass: row ranges per sample tile, each summed by one block (default 0 = by shape: as many as fill the chip's resident blocks, of at least 256 rows each); tests put the row count on either side of every slice edge */
    PGENHIP_KNOB_WIDE_BURST = 28,        /* stream kernel (GT segments and full lines of long rows): plain store steps issued back to back, 1 or 2; default 0 = by shape (1 on launches of 9 GB of text and more in rows of more than 16 KiB, else 2) */
    PGENHIP_KNOB_PARSE_BLOCKS = 29,      /* GT text parse kernels: grid size in blocks (default 0 = by shape: the work, capped at 8 blocks per CU); tests force small grids */
    PGENHIP_KNOB_JOIN_BLOCKS = 30,       /* join kernels: grid size in blocks (default 0 = by shape: the work, capped at 8 blocks per CU); tests force small grids */
    PGENHIP_KNOB_PRUNE_BLOCKS = 31,      /* prune resolve kernels: grid size in blocks (default 0 = by shape); for the BLOCK shape thereby the rows of a workgroup's range; tests force small grids */
    PGENHIP_KNOB_LOGIT_BLOCKS = 32,      /* per-variant logistic regression: grid size in blocks (default 0 = by shape: a block per group of rows (FAST) or per row (GENERAL), capped at 8 blocks per CU); tests force small grids */
    PGENHIP_KNOB_RUNS_ROWS = 7       /* RUNS kernel: rows per work item (default: as many as one wide load / one span holds) */
} pgenhip_knob;
int pgenhip_tune(pgenhip_ctx *ctx, uint32_t knob, int32_t value);

/* Block until everything queued on the ctx stream has finished. */
int pgenhip_wait(pgenhip_ctx *ctx);

/* hipEvent pair on the ctx stream: start ... launches ... stop -> elapsed ms (stop synchronises). */
int pgenhip_timer_start(pgenhip_ctx *ctx);
int pgenhip_timer_stop(pgenhip_ctx *ctx, float *elapsed_ms);
/* Pipelined form: mark records the stop event without blocking; read returns the elapsed ms once
 * the stream has passed the mark (e.g. after pgenhip_wait). */
int pgenhip_timer_mark(pgenhip_ctx *ctx);
int pgenhip_timer_read(pgenhip_ctx *ctx, float *elapsed_ms);

/* ---- device / pinned memory for hosts that do not link HIP themselves --- */
int pgenhip_device_malloc(pgenhip_ctx *ctx, void **d_ptr, size_t bytes);
int pgenhip_device_free(pgenhip_ctx *ctx, void *d_ptr);
int pgenhip_host_malloc_pinned(pgenhip_ctx *ctx, void **h_ptr, size_t bytes);
int pgenhip_host_free_pinned(pgenhip_ctx *ctx, void *h_ptr);
/* asynchronous on the ctx stream (truly async only from/to pinned host memory) */
int pgenhip_memcpy_h2d(pgenhip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int pgenhip_memcpy_d2h(pgenhip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* bytes of the ctx's device that are free right now, and that it has (either pointer may be NULL, not both): what a host sizes
 * buffers that stay resident by, before it allocates them */
int pgenhip_device_memory(pgenhip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- synthetic records generated on the device --------- */
#define PGENHIP_SYNTH_DIRTY_PAD 1u
/* "hwe" value distribution instead of uniform codes: variant v has allele frequency
 * p = (655 + splitmix64((seed ^ 0x4D4146) + v) % 32113) / 65536 in [0.01, 0.5); sample s draws two alleles from
 * h = splitmix64(splitmix64((seed ^ 0x485745) + v) + s) (low two 16-bit fields < p * 65536) -> codes 0/1/2 in
 * Hardy-Weinberg proportions, and is missing (code 3) when h >> 32 < 4294967 (0.1 %).  Pad bits zero. */
#define PGENHIP_SYNTH_HWE 2u
/* record bytes of variant v = LE words splitmix64(seed + (v << 20) + word_idx), truncated to R;
 * pad bits of the last byte zeroed unless PGENHIP_SYNTH_DIRTY_PAD (the tests hold a CPU twin). */
int pgenhip_synth_records(pgenhip_ctx *ctx, void *d_dst, uint64_t record_stride,
                          uint64_t first_variant, uint32_t n_variants,
                          uint64_t seed, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
