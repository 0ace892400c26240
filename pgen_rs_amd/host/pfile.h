// pfile.h — C++ host restatement of pgen-rs's `Pfile` (src/pfile.rs:19-336) above the C ABI of
// include/pgen_hip.h.  Same names and argument meaning as the reference so a pgen-rs user finds
// what they expect; the per-variant decode/emit body (src/pfile.rs:165-190) is NOT here — it runs
// on the GPU through pgenhip_emit_lines.  The reference is compiled Rust and no Rust toolchain
// exists in this image, hence C++.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "csvlite.h"

namespace pgenhost {

// What the reference expresses as panic!/unwrap()/assert! (exit status 101).
struct PfileError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// An open file, closed when it goes out of scope.  close() is the checked close: a failed close (ENOSPC/EIO surfacing late) must
// not leave a truncated file behind an exit code 0.
class Fd {
  public:
    Fd(const std::string &path, int flags) : path_(path), fd_(::open(path.c_str(), flags, 0644))
    {
        if (fd_ < 0) throw PfileError(((flags & O_CREAT) ? "create " : "open ") + path + ": " + std::strerror(errno));
    }
    Fd(const Fd &) = delete;
    Fd &operator=(const Fd &) = delete;
    ~Fd()
    {
        if (fd_ >= 0) ::close(fd_);
    }
    int get() const { return fd_; }
    // all n bytes at the file's current position
    void write_all(const void *data, size_t n)
    {
        for (const char *p = static_cast<const char *>(data); n;) {
            const ssize_t w = ::write(fd_, p, n);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) throw PfileError("write " + path_ + ": " + std::strerror(errno));
            p += w;
            n -= (size_t)w;
        }
    }
    void close()
    {
        const int fd = fd_;
        fd_ = -1;
        if (::close(fd) != 0) throw PfileError("close " + path_ + ": " + std::strerror(errno));
    }

  private:
    std::string path_;
    int fd_;
};

struct OutputOptions {
    int n_gpus = 1;                         // variant ranges shard over devices 0..n_gpus-1 (no collective)
    int n_shards = 0;                       // 0 = one shard per GPU; > 0: that many variant ranges, dealt round-robin over the GPUs
    uint64_t block_text_bytes = 128ull << 20;  // VCF bytes produced (and record bytes read) per block and device: the unit of staging, D2H copy and file write.  End to end on the chr22 shape
                                               // (tmpfs): 512 / 256 / 128 / 64 MiB -> 2.87 / 2.56 / 2.47 / 2.39 s keeping everybody, 1.03 / 0.76 / 0.65 / 0.65 s
                                               // keeping 20 samples: pinning the staging buffers costs more than bigger launches give (profiles/r02_e2e.md)
    uint64_t launch_bytes = 2048ull << 20;     // text (or record) bytes one kernel launch covers: several consecutive blocks, staged and copied out block by block
    int write_threads = 1;                  // parallel pwrite()s per block and device
    int read_threads = 4;                   // parallel pread()s of one run of consecutive records (runs of >= 64 MiB)
    bool bgzf = false;                      // write BGZF (`.vcf.gz`) instead of plain text
    int bgzf_level = 6;                     // zlib level of the BGZF members (bgzip's default)
    int compress_threads = 0;               // deflate threads per device shard (0 = the host's cores, at most 32)
    int filter_threads = 0;                 // pieces the metadata walk is cut into (0 = by file size and host cores, 1 = serial like the reference)
    bool verbose = false;
};

// `matrix`: the element type of the output (.npy 'descr'), the bit patterns written for codes 0-3 and the orientation
struct MatrixOptions {
    uint32_t elem_bytes = 1;          // 1, 2 or 4
    std::string descr = "|i1";        // NumPy dtype string
    uint8_t values[16] = {0, 1, 2, 0xFF};   // four elements of elem_bytes bytes, little-endian
    bool sample_major = false;        // shape (K, V_kept) instead of (V_kept, K)
};

// `ld`: the window in kept variants, the r^2 floor of a printed pair, r^2 alone or the pair's table beside it
struct LdOptions {
    uint32_t window = 0;              // W >= 1: pairs (i, i + d), 1 <= d <= W, of the kept variants
    double min_r2 = 0.2;              // pairs below it (and NaN pairs) are not printed; 0 prints every pair with a defined r^2
    bool counts = false;              // --counts: N_OBS and the sixteen cells behind R2, r^2 from the table on the host
    uint64_t block_rows = 0;          // left rows per block (0: as many as fill block_text_bytes with their W entries each)
};

// `export`: the container written
struct ExportOptions {
    bool bed = false;                 // PLINK 1 .bed / .bim / .fam instead of .pgen / .pvar / .psam
};

// `prune`: the window in kept variants and / or in base pairs, the r^2 above which two variants do not both stay
struct PruneOptions {
    uint32_t window = 0;              // --window W (0: not given; then --window-kb sets W from the positions)
    uint64_t window_kb = 0;           // --window-kb KB (0: not given): pairs further apart than KB x 1000 base pairs are no edges
    bool has_window_kb = false;
    double min_r2 = 0.2;              // --r2: an edge is r^2 > min_r2 (as float32)
    bool with_export = false;         // --export: OUT.pgen / .pvar / .psam of the kept variants and samples beside the two lists
    uint64_t block_rows = 0;          // rows per block (0: as many as fill block_text_bytes with their records)
};

// `score`: how missing calls count and what is printed
struct ScoreOptions {
    bool mean_imputation = true;      // a missing call counts as the variant's mean dosage over the kept samples called (else as 0)
    bool average = false;             // --avg: <NAME>_AVG = SUM / DENOM instead of <NAME>_SUM
};

// A `score` weights file: tab-separated, a header line (a leading '#' allowed), then one row per variant: ID, effect allele, one
// weight per score.  read_score_weights throws a PfileError that names the line for a weight that is not a finite number (after
// rounding to f32), a row with another number of cells than the header, and an ID that occurs twice.
struct ScoreWeights {
    std::vector<std::string> names;          // the score columns' header cells
    std::vector<std::string> ids, alleles;   // per row
    std::vector<float> w;                    // rows x names.size(), rounded to f32 once, at parse time
    std::vector<size_t> lines;               // the file line each row starts on
};
ScoreWeights read_score_weights(const std::string &path);

// `assoc`: the per-sample value files
struct AssocOptions {
    std::string pheno_file;                 // --pheno: IID, then one quantitative phenotype per column
    std::vector<std::string> pheno_names;   // --pheno-name: the columns used (empty: all)
    std::string covar_file;                 // --covar: IID, then one covariate per column (empty: the intercept alone)
    bool logistic = false;                  // --logistic: case/control phenotypes, a logistic regression per variant on the device
    bool mean_imputation = true;            // --logistic: a missing call counts as the variant's mean dosage (else the sample is dropped for that variant)
    uint32_t max_iter = 25;                 // --logistic: evaluations per variant at most (1 .. PGENHIP_LOGIT_MAX_ITER)
    double tol = 1e-9;                      // --logistic: a fit has converged when no coefficient moves by more
};

// A `assoc` pheno / covar file: tab-separated, a header line (a leading '#' allowed), then one row per sample: IID, one value per
// column; NA, nan and empty cells are missing (NaN here).  read_value_table throws a PfileError that names the line for a cell
// that is not a number, a row with another number of cells than the header, and an IID that occurs twice.
struct ValueTable {
    std::vector<std::string> names;          // the value columns' header cells
    std::vector<std::string> iids;           // per row
    std::vector<double> x;                   // rows x names.size()
};
ValueTable read_value_table(const std::string &path);

// `kinship`: what is printed and how the kept samples are cut into rank tiles on the device
struct KinshipOptions {
    bool counts = false;              // --counts: the sixteen cells of the pair's table behind KINSHIP
    bool has_min = false;             // --min-kinship given
    double min_kinship = 0.0;         // with has_min: lines below it (and nan lines) are not printed
    uint32_t tile = 1024;             // ranks per square tile: one device buffer of 64 * tile^2 bytes per pair of tiles
    uint64_t block_rows = 0;          // variants per block (0: as many as fill block_text_bytes with their records)
};

// `grm`: the files written and how the kept samples are cut into rank tiles on the device
struct GrmOptions {
    bool rel = false;                 // --format rel: the full square as text instead of GCTA's binary lower triangle
    uint32_t tile = 1024;             // ranks per square tile: two device buffers of 8 * tile^2 bytes per pair of tiles
    uint64_t block_rows = 0;          // variants per block (0: as many as fill block_text_bytes with their records)
};

// `pca`: how many components, when the iteration stops, where it starts
struct PcaOptions {
    uint32_t pcs = 10;                // --pcs: principal components written, 1 .. 32 and <= kept samples
    double tol = 1e-6;                // --tol: stop when the largest residual norm of the first pcs Ritz pairs is <= tol * lambda_1
    uint32_t max_passes = 100;        // --max-passes: passes over the records at most (each is one product M Q)
    uint64_t seed = 1;                // --seed: of the Gaussian start matrix
    uint64_t block_rows = 0;          // variants per block (0: as many as fill block_text_bytes with their records)
};

struct OutputStats {
    uint64_t variants = 0, samples_kept = 0, header_bytes = 0, body_bytes = 0;   // header / body: bytes of VCF text
    uint64_t file_bytes = 0;                                                     // what the output file holds (BGZF: compressed)
    double seconds_filter = 0, seconds_body = 0, seconds_kernel = 0;
    uint64_t score_matched = 0, score_flipped = 0, score_skipped = 0;            // `score`: weights rows used, of them REF-effect rows, rows not used
    uint64_t assoc_dropped = 0;                                                  // `assoc`: kept samples dropped for a missing phenotype or covariate
    uint64_t logit_converged = 0, logit_not_converged = 0, logit_singular = 0;   // `assoc --logistic`: output lines per status
    uint64_t grm_skipped = 0;                                                    // `grm`: kept variants that add nothing (no call, or monomorphic among the kept samples)
    uint64_t pca_skipped = 0, pca_passes = 0;                                    // `pca`: kept variants that add nothing; passes over the records
    double pca_residual = 0;                                                     // `pca`: max over the written components of |M u - lambda u| / lambda_1 at the last pass
    bool pca_converged = true;                                                   // `pca`: the residual reached --tol within --max-passes
    uint64_t import_skipped = 0, import_half_call = 0, import_haploid = 0, import_phased = 0;   // `import`: multiallelic lines dropped; lines with a half call, a haploid call, a phased call
    uint64_t prune_kept = 0, prune_removed = 0, prune_edges = 0, prune_window = 0, prune_calls = 0, prune_mask_bytes = 0;   // `prune`: its JSON line
    double seconds_setup = 0;   // inside seconds_body: HIP runtime start, contexts, device and pinned allocations of the slowest shard, before its first block is staged
};

class Pfile {
  public:
    std::string pfile_prefix;  // src/pfile.rs:20-22
    uint32_t num_variants = 0;
    uint32_t num_samples = 0;
    // Variable-width storage modes (the reference refuses them at src/pfile.rs:53 and only validates
    // their tables in the dead `Pgen` type, src/pgen.rs): per-variant record type / length / file offset from the
    // header walk (pgenhip_vw_walk_index).  Empty for a fixed-width (0x02) file.
    uint8_t storage_mode = 0x02;
    std::shared_ptr<const std::vector<uint8_t>> vw_record_type;
    std::shared_ptr<const std::vector<uint32_t>> vw_record_len;
    std::shared_ptr<const std::vector<uint64_t>> vw_record_off;
    bool variable_width() const { return static_cast<bool>(vw_record_off); }
    // file offset of variant var_idx's record: src/pfile.rs:165 (u64), or the walked table
    uint64_t record_offset(uint64_t var_idx) const;

    std::string pgen_path() const { return pfile_prefix + ".pgen"; }  // :26-36
    std::string psam_path() const { return pfile_prefix + ".psam"; }
    std::string pvar_path() const { return pfile_prefix + ".pvar"; }

    // :38-76 — opens PREFIX.pgen and checks magic / storage mode 0x02 / flag byte 0x40; storage mode 0x10 goes through the
    // variable-width header walk (src/pgen.rs:21-258) and is accepted when the file holds its tables and they are sound;
    // every other mode is refused like the reference does (:53)
    static Pfile from_prefix(const std::string &pfile_prefix);

    // :196-200
    uint32_t variant_record_size() const;

    // :202-220 — (all leading '#' lines but the last, the last one = column names line)
    std::pair<std::string, std::string> read_pvar_header() const;

    // :248-268 — byte offset just after the '#' of the column-header line
    static uint64_t find_metadata_file_header_start(const std::string &file_contents);

    using IdxRecords = std::vector<std::pair<size_t, StringRecord>>;
    // :312-335 — rows (file order) whose predicate is true; all rows without a query
    // (filter_threads: 0 = as many pieces as the file size and the host's cores suggest, 1 = the reference's serial walk)
    static IdxRecords filter_metadata(TsvReader &reader, const std::optional<std::string> &query, int filter_threads = 0);

    // :111-128 — the kept variant and sample rows (.psam read first, .pvar filtered first) and the two header rows
    struct Selection {
        IdxRecords var_idx_rcds, sam_idx_rcs;
        StringRecord sam_header, var_header;
    };
    Selection select(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query, int filter_threads) const;

    // :78-102 — prints f_string evaluated on each kept row to `out` (stdout in the CLI)
    static void query_metadata(TsvReader &reader, const std::optional<std::string> &query, const std::string &f_string,
                               std::string &out);

    // :104-194 — header on the host, body lines assembled on the GPU(s)
    OutputStats output_vcf(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                           const std::string &filename, const OutputOptions &opt = OutputOptions()) const;

    // `freq` (not in the reference): per-variant genotype counts of the kept samples, one tab-separated line per kept variant
    // (CHROM POS ID REF ALT, then the counts of 0/0, 0/1, 1/1 and ./.) behind plink2 .gcount-style column names.  Variant and
    // sample selection are output_vcf's (filter_metadata); records are staged like output_vcf's and counted on the GPU(s)
    // (pgenhip_genotype_counts / _at); 16 bytes per variant come back.  filename empty: stdout.
    // Uses n_gpus, n_shards, block_text_bytes (bytes of records per block), read_threads and filter_threads of `opt`.
    OutputStats output_freq(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                            const std::string &filename, const OutputOptions &opt = OutputOptions()) const;

    // `sample-counts` (not in the reference): per-sample genotype counts over the kept variants, one tab-separated line per kept
    // sample in psam order (the IID column verbatim, then the counts of 0/0, 0/1, 1/1 and ./.).  Selection and staging are freq's;
    // each shard's blocks accumulate on the device (pgenhip_sample_counts / _at), 16 bytes per kept sample come back once per
    // shard and the host sums the shards in u64.  No kept variant or no kept sample: zero lines / the header alone, no device.
    // A psam without an IID column is vcf_header's error.  filename empty: stdout.
    OutputStats output_sample_counts(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                     const std::string &filename, const OutputOptions &opt = OutputOptions()) const;

    // `score` (not in the reference): polygenic scores of the kept samples, S[k, c] = sum over the matched variants of w[j, c] * dosage
    // (plink2 --score; no byte or digit parity with its .sscore is claimed).  The weights file's rows are matched by the .pvar ID
    // among the kept variants: effect allele == ALT uses the weight as is, == REF scores w * (2 - dosage) (-w on the device, the
    // constant sum of 2w added on the host in FP64), neither allele or an ID that is not kept skips the row; a matched ID that
    // occurs twice among the kept variants is an error that names the line, no matched row at all an error before any device is
    // touched.  Only the matched variants are staged (freq's block loop and shards); per block pgenhip_genotype_counts gives the
    // mean dosage of every row (mean imputation: miss[j] = (float)((c1 + 2 c2) / (c0 + c1 + c2)), 0 when nobody is called),
    // pgenhip_sample_scores adds the block into K x C doubles on the device, at most PGENHIP_SCORE_MAX_COLUMNS columns per launch,
    // and pgenhip_sample_counts accumulates the per-sample missing count; both come back once per shard and shards are summed in
    // FP64.  One line per kept sample in psam order: IID, ALLELE_CT = 2 (M - missing), DENOM (2 M under mean imputation, else
    // ALLELE_CT), then <NAME>_SUM per score (%.12g), or with average <NAME>_AVG = SUM / DENOM (nan when DENOM is 0).  No kept
    // sample: the header alone, no device.  filename empty: stdout.
    OutputStats output_score(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                             const std::string &weights_file, const std::string &filename, const ScoreOptions &sopt,
                             const OutputOptions &opt = OutputOptions()) const;

    // `assoc` (not in the reference): a linear regression of every chosen phenotype on every kept variant's ALT dosage with an
    // intercept and the covariates, over the kept samples that have every chosen phenotype and every covariate (complete cases); a
    // missing call counts as the variant's mean dosage over the called samples (mean imputation, as in `score`; plink2 --glm drops
    // the sample for that variant instead, so no digit parity with it is claimed).  The host orthonormalises [1, covariates]
    // (modified Gram-Schmidt, twice; stats.h holds this arithmetic) into Q and residualises every phenotype, r_p = y_p - Q Q' y_p; Q's columns and the r_p go up
    // once per shard as K x (m + P) doubles.  Per block (freq's block loop and shards) pgenhip_genotype_counts gives c0 .. c3 and
    // pgenhip_variant_sums, at most PGENHIP_VSUM_MAX_COLUMNS columns per launch, the four per-code sums S[v][x] of every column;
    // 16 + 32 (m + P) bytes per row come back.  With called = c0 + c1 + c2, mu = (c1 + 2 c2) / called, t_v = S[v][1] + 2 S[v][2]
    // + mu S[v][3], gg = c1 + 4 c2 + mu^2 c3 and denom = gg - sum over Q's columns of t_q^2: BETA = t_r / denom, rss = r'r -
    // t_r^2 / denom, SE = sqrt(rss / (n - m - 1) / denom), T_STAT = BETA / SE, P two-sided Student t.  One line per variant and
    // phenotype: CHROM POS ID REF ALT A1 PHENO OBS_CT MISS_CT A1_FREQ BETA SE T_STAT P (%.12g; NA where called == 0, denom <=
    // 1e-12 gg or rss <= 0).  Fewer than m + 2 complete samples or collinear covariates: an error before any device is touched.
    // No kept variant: the header alone.  filename empty: stdout.
    // With aopt.logistic the phenotypes are case/control columns (1 / 2 with a 2 present, or 0 / 1; another column, or one without a
    // case or without a control among the complete cases, is an error that names it) and every line is a logistic fit: the host
    // scales Q by sqrt(n) into the design, fits every phenotype's null model (stats.h), and per block pgenhip_genotype_counts gives
    // the code table (0, 1, 2 and the mean dosage, or NaN without mean imputation: the sample is dropped for that variant) and
    // pgenhip_variant_logistic, once per phenotype, the genotype's coefficient (log-odds per ALT allele), its standard error and a
    // status: CHROM POS ID REF ALT A1 PHENO OBS_CT MISS_CT A1_FREQ BETA SE Z_STAT P ITER STATUS, P = erfc(|Z| / sqrt 2) (Wald),
    // STATUS "." / NOT_CONVERGED / SINGULAR and NA in BETA .. P unless converged.  No Firth fallback, no step halving.
    OutputStats output_assoc(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                             const AssocOptions &aopt, const std::string &filename, const OutputOptions &opt = OutputOptions()) const;

    // `matrix` (not in the reference): the additive-coded genotype matrix of the kept variants and samples as a NumPy .npy file
    // (version 1.0, C order, data on a multiple of 64 bytes), decoded on the GPU(s) (pgenhip_decode_matrix / _at) block by block and
    // written with pwrite at offsets computed up front, so shards and blocks write independently; with sample_major a block is a
    // column band of the file.  Beside it FILE.variants (the ID column of the kept variants, one per line) and FILE.samples (IID).
    // Selection and staging are freq's.  No kept variant or no kept sample: a valid file with a zero dimension, no device.
    // Uses n_gpus, n_shards, block_text_bytes (bytes of matrix per block), read_threads and filter_threads of `opt`.
    OutputStats output_matrix(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &filename, const MatrixOptions &mopt, const OutputOptions &opt = OutputOptions()) const;

    // `ld` (not in the reference): r^2 of every pair of kept variants at most `window` kept variants apart, over the kept samples
    // (pgenhip_pair_stats / _at, the unphased genotype correlation over the samples called in both; no digit parity with plink2 is
    // claimed).  One tab-separated line per pair on one chromosome with r^2 >= min_r2, ordered by (first variant, distance):
    // CHROM_A POS_A ID_A CHROM_B POS_B ID_B R2 (%.6g), with counts also N_OBS and the table's cells T00 .. T33 (Tab = samples with
    // code a in A and b in B; 0 hom-ref, 1 het, 2 hom-alt, 3 missing).  Selection and staging are freq's; shards own contiguous
    // ranges of first variants and every block stages the `window` rows behind its own, so no pair is lost or repeated at a seam.
    // Fewer than two kept variants or no kept sample: the header alone, no device.  filename empty: stdout.
    OutputStats output_ld(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                          const std::string &filename, const LdOptions &ld, const OutputOptions &opt = OutputOptions()) const;

    // `export` (not in the reference): the kept variants and samples written back as a fixed-width (mode 0x02) OUT.pgen with OUT.pvar
    // and OUT.psam, or as PLINK 1 OUT.bed / .bim / .fam (variant-major, ALT as A1; no byte parity with plink2 is claimed).  The records
    // are packed on the GPU(s) (pgenhip_pack_records / _at) block by block and written with pwrite at 12 + j * R_K (3 + j * R_K for
    // .bed), so shards and blocks write independently.  The .pvar is the input's header lines verbatim and then each kept row's
    // fields joined by tabs; the .psam the input's bytes up to and including its column-header line, then the kept rows likewise.
    // .bim: CHROM ID 0 POS ALT REF (an ALT with a ',' is an error that names the variant); .fam: FID IID PAT MAT SEX -9, with 0 for a
    // column the .psam lacks and for a SEX other than 1 or 2.  Selection and staging are freq's.  A variable-width input whose kept
    // records are plain gives a fixed-width output.  No kept variant or no kept sample: valid files with a zero dimension, no
    // device.  out_prefix naming the input's own .pgen is refused before anything is opened for writing.
    // Uses n_gpus, n_shards, block_text_bytes (bytes of records per block), read_threads and filter_threads of `opt`.
    OutputStats output_export(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                              const std::string &out_prefix, const ExportOptions &eopt, const OutputOptions &opt = OutputOptions()) const;

    // `prune` (not in the reference): LD pruning of the kept variants.  One pass over the blocks (each with the W rows behind it) counts
    // every row (pgenhip_genotype_counts) and ORs its pairs' edges into two masks that stay on the device (pgenhip_pair_mask with keys
    // (CHROM rank by first appearance << 32) | POS; without --window-kb POS is left out and max_span is 0, so a window in variants
    // still stops at chromosome ends); then the priorities (minor-allele frequency among called alleles, host/prune_plan.h) go up,
    // pgenhip_prune_resolve runs until nothing is undecided, and one state byte per row comes back.  The more common variant of a
    // correlated pair stays, ties go to the earlier one; a monomorphic or uncalled variant has no r^2, hence no edge, and is kept.
    // Writes OUT.prune.in (the kept variants' IDs, one per line, in file order) and OUT.prune.out (the removed ones'), with --export
    // also OUT.pgen / .pvar / .psam of the kept variants and samples through `export`'s own path.  One device.  Fewer than two kept
    // variants or no kept sample: every variant is kept and no device is touched.  No parity with plink2 --indep-pairwise is claimed.
    OutputStats output_prune(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                             const std::string &out_prefix, const PruneOptions &popt, const OutputOptions &opt = OutputOptions()) const;

    // `kinship` (not in the reference): the joint genotype tables of every pair of kept samples over the kept variants
    // (pgenhip_sample_pair_stats / _at) and the KING-robust between-family kinship estimate from them.  The kept samples are cut into
    // square tiles of `tile` ranks; the device holds the upper block triangle of tables, one buffer per pair of tiles, overwritten by
    // the first block of variants and added to by the others (freq's block loop and shards; every staged block is used for every
    // pair of tiles before the next one is read); the buffers come back once per shard and the host adds the shards' u32 tables.
    // The whole triangle (32 K^2 bytes) must fit the device: out-of-core sample tiling is not built, and a triangle that does not
    // fit fails with the library's out-of-memory message.  One line per pair of ranks a < b, ordered by (a, b):
    // IID1 IID2 N HETHET IBS0 HET1 HET2 KINSHIP, all over the rows called in both samples (cells x, y in {0, 1, 2}): N their sum,
    // HETHET = T[1][1], IBS0 = T[0][2] + T[2][0], HET1 = T[1][0] + T[1][1] + T[1][2], HET2 = T[0][1] + T[1][1] + T[2][1],
    // KINSHIP = 0.5 - (HET1 + HET2 - 2 HETHET + 4 IBS0) / (4 min(HET1, HET2)) in double (%.6g; nan when min(HET1, HET2) == 0);
    // with counts also T00 .. T33.  No byte or digit parity with plink2's .kin0 or KING is claimed.  Fewer than two kept samples:
    // the header alone; no kept variant: every table is zero; neither touches a device.  filename empty: stdout.
    OutputStats output_kinship(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                               const std::string &filename, const KinshipOptions &kopt, const OutputOptions &opt = OutputOptions()) const;

    // `grm` (not in the reference): the genetic relationship matrix of the kept samples over the kept variants, GCTA's definition.
    // Per block of variants: pgenhip_genotype_counts, then on the host in double called = c0 + c1 + c2, p = (c1 + 2 c2) / (2 called),
    // s = 1 / sqrt(2p(1-p)) and the two tables G ((0-2p)s, (1-2p)s, (2-2p)s, 0) and N (1, 1, 1, 0), both all zero for a variant
    // with no call or with p == 0 or p == 1 (counted in grm_skipped); then pgenhip_sample_gram / _at twice for every pair of rank
    // tiles of the upper block triangle (kinship's tiling, block loop and shards; the shard's first block overwrites, the others
    // accumulate).  The host adds the shards' doubles in shard order.  GRM[a][b] = G[a][b] / N[a][b], the mean over the variants
    // called in both samples; nan where N == 0.  Both triangles (16 K^2 bytes) must fit the device and the host: out-of-core sample
    // tiling is not built.  grm-bin: out_prefix.grm.bin (little-endian f32, lower triangle with the diagonal, row a then b = 0..a),
    // .grm.N.bin (f32 N in the same order), .grm.id (FID<TAB>IID with FID = IID).  rel: out_prefix.rel (K lines of K tab-separated
    // %.17g values) and .rel.id (one IID per line).  No kept sample: empty files; no kept variant: every entry nan; neither touches
    // a device.  No byte or digit parity with plink2 or GCTA is claimed.
    OutputStats output_grm(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                           const std::string &out_prefix, const GrmOptions &gopt, const OutputOptions &opt = OutputOptions()) const;

    // `pca` (not in the reference): the leading principal components of the kept samples over the kept variants, without the K x K
    // matrix.  M = Z^T Z / V_used with Z[j][k] = grm's table G of variant j at the code of sample k: ((0-2p)s, (1-2p)s, (2-2p)s, 0), p
    // from a first pass of pgenhip_genotype_counts, so a missing call sits at the variant's mean (plink2 --pca's convention; grm's
    // G / N is pairwise-complete and differs wherever calls are missing).  A variant with no call or p of 0 or 1 is skipped
    // (pca_skipped); V_used counts the others.  Randomised subspace iteration with Rayleigh-Ritz in every pass: L = min(K, pcs + 10)
    // columns; Q starts as a seeded Gaussian K x L matrix (splitmix64 from the seed; per entry two draws u1 in (0, 1], u2 in [0, 1)
    // and the Box-Muller cosine sqrt(-2 ln u1) cos(2 pi u2), row-major), orthonormalised (linalg.h).  One pass: Y = M Q by
    // pgenhip_gram_apply / _at over freq's block loop and shards, 16 columns per call; the shard's first block overwrites, the
    // others accumulate; the host adds the shards in the order of their first variants; records are re-staged every pass.  Then
    // T = Q^T Y (symmetrised) = W Lambda W^T, U = Q W, r_i = Y w_i - lambda_i u_i; stop when max over i < pcs of |r_i| <= tol * lambda_1
    // or after max_passes passes (pca_converged false: the outputs are written all the same), else Q = orth(Y).
    // out_prefix.eigenval: pcs lines, %.17g.  out_prefix.eigenvec: "#IID<TAB>PC1 .. PCpcs", one line per kept sample, unit-norm
    // vectors, each with its largest-magnitude entry positive, %.17g.  No kept sample, no kept variant or no usable variant: the
    // header alone and an empty .eigenval (the first two touch no device).  No digit parity with plink2 is claimed.
    OutputStats output_pca(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                           const std::string &out_prefix, const PcaOptions &popt, const OutputOptions &opt = OutputOptions()) const;

    // the header part of output_vcf (:110-146) on its own: used by output_vcf and by the CPU tests
    std::string vcf_header(const IdxRecords &sam_idx_rcs, const StringRecord &sam_header) const;
};

// Synthetic PREFIX.{pgen,pvar,psam}: pvar rows "22\t{16050000+7i}\tsnp{i}\tA\tG\t100\tPASS\t.",
// psam "#IID\tSEX\tKEEP" with "S{i:06d}\tNA\t{keep}", records from pgenhip_synth_records on device 0.
void synth_pfile(const std::string &prefix, uint32_t variants, uint32_t samples, uint32_t keep_modulus, uint64_t seed);

// `import`: what becomes of lines that a biallelic hard-call file cannot hold
struct ImportOptions {
    bool skip_multiallelic = false;   // --skip-multiallelic: drop the lines whose ALT holds a ',' (and count them); without it their alleles >= 2 are an error
};

// VCF (plain text, or gzip / BGZF: one sequential zlib stream over concatenated members) to OUT_PREFIX.pgen (fixed-width, storage
// mode 0x02), .pvar (the ## lines but ##fileformat= and `##source=pgen-rs`, which `filter` adds itself; the columns in front of FORMAT,
// verbatim) and .psam (#IID SEX, NA).  Blocks of whole lines go through read -> pinned -> H2D -> pgenhip_parse_gt -> D2H -> pwrite at
// 12 + j*R; a reader thread fills and indexes block k + 1 (pgenhip_vcf_index_lines) while block k is on the device.  One device: the
// reader bounds the command.  A FORMAT other than GT / GT:..., a line with too few columns or fields, a call of another form than
// the grammar's or an allele other than 0, 1 and '.' is an error that names the input's line (1-based) and leaves no output file;
// half calls, haploid calls and phased calls are counted per line and warned about once each.  More than 2^32 - 1 variants is an
// error.  Uses block_text_bytes of `opt` (text bytes per block).
OutputStats import_vcf(const std::string &in_path, const std::string &out_prefix, const ImportOptions &iopt, const OutputOptions &opt = OutputOptions());

// whole-file read helper (metadata files are read once; the reference streams them through BufReader)
std::string read_file(const std::string &path);

}  // namespace pgenhost
