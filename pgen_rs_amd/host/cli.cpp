// cli.cpp — `pgen-hip`: the pgen-rs command-line surface (src/cli.rs:1-62, dispatch
// src/main.rs:92-127) on top of the MI355X engine.  Same subcommands, flags and defaults:
//
//   pgen-hip query  <PFILE_PREFIX> -f|--fstring <EXPR> [-i|--include <EXPR>] [-s|--samples]
//   pgen-hip filter <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [-o|--out <FILE>]
//
// `pgen-hip freq <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [-o|--out <FILE>]` (not in the reference): per-variant
// genotype counts of the kept samples with filter's selection, counted on the GPU; tab-separated to stdout or FILE.
// `pgen-hip sample-counts <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [-o|--out <FILE>]` (not in the reference): the
// other half, per-sample genotype counts over the kept variants (IID, then the four counts), same selection, staging and output.
// `pgen-hip matrix <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [--dtype i8|f16|f32] [--missing <X>] [--sample-major]
// -o|--out <FILE.npy>` (not in the reference): the additive-coded genotype matrix (0 / 1 / 2 alternate alleles, --missing for
// "./.") of the kept variants and samples as a NumPy .npy file, decoded on the GPU; FILE.npy.variants / FILE.npy.samples hold the ids.
// `pgen-hip export <PFILE_PREFIX> -o|--out <OUT_PREFIX> [--format pgen|bed] [--include-var <EXPR>] [--include-sam <EXPR>]` (not in the
// reference): the kept variants and samples written back as OUT_PREFIX.pgen / .pvar / .psam (fixed-width), or as PLINK 1 .bed / .bim /
// .fam; the records are packed on the GPU.
// `pgen-hip score <PFILE_PREFIX> --weights <FILE> [--no-mean-imputation] [--avg] [--include-var <EXPR>] [--include-sam <EXPR>]
// [-o|--out <FILE>]` (not in the reference): polygenic scores of the kept samples (plink2 --score), the weighted dosage sums of the
// variants FILE names among the kept ones, summed on the GPU in FP64.
// `pgen-hip kinship <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [--min-kinship <X>] [--counts] [-o|--out <FILE>]` (not in
// the reference): the joint genotype table of every pair of kept samples over the kept variants, counted on the GPU's int8 matrix
// cores, and the KING-robust kinship estimate from it.
// `pgen-hip grm <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [--format grm-bin|rel] -o|--out <OUT_PREFIX>` (not in the
// reference): the genetic relationship matrix of the kept samples over the kept variants (GCTA's definition), two FP64 Gram
// matrices per block of variants on the GPU's FP64 matrix cores.
// `pgen-hip pca <PFILE_PREFIX> [--include-var <EXPR>] [--include-sam <EXPR>] [--pcs <P>] [--tol <X>] [--max-passes <I>] [--seed <S>]
// -o|--out <OUT_PREFIX>` (not in the reference): the leading principal components of the kept samples by randomised subspace iteration,
// every pass one matrix-free Gram product (pgenhip_gram_apply) over the kept variants; the K x K matrix is never formed.
// `pgen-hip merge <PFILE_PREFIX> <PFILE_PREFIX> [...] -o|--out <OUT_PREFIX> [--union]` (not in the reference): two to eight filesets'
// samples side by side in one fileset, variants matched by (CHROM, POS, {REF, ALT}) with REF/ALT swaps flipped; the records are
// joined on the GPU (pgenhip_join_records).
// Additions (opt-in, not in the reference): --gpus <N>, --block-mib <M>, --launch-mib <M>, --filter-threads <T>, --stats, --dry-run
// (filter: write the VCF header only and report the body geometry; needs no GPU); BGZF output (`-o x.vcf.gz` or --bgzf,
// --bgzf-level <1-9>, --compress-threads <T>) and `pgen-hip bgzf <IN> <OUT>`, the same writer on a file.
// Exit codes: 0 ok; 2 usage error (clap's code); 101 where the reference would panic.
#include <cerrno>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <optional>
#include <string>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "bgzf.h"
#include "expr.h"
#include "merge.h"
#include "pfile.h"
#include "../../include/pgen_hip.h"
#include "stats.h"

using namespace pgenhost;

namespace {

// --dry-run: the VCF header alone, as text or as a complete BGZF file (header members + EOF marker)
void write_header_only(const std::string &out_file, const std::string &header, bool bgzf, int level)
{
    Fd f(out_file, O_WRONLY | O_CREAT | O_TRUNC);
    if (bgzf) {
        BgzfWriter w(f.get(), out_file, level, 1);
        w.write(header.data(), header.size());
        w.finish();
    } else {
        f.write_all(header.data(), header.size());
    }
    f.close();
}

void bgzf_file(const std::string &in, const std::string &out, int level, unsigned threads, size_t chunk)
{
    const Fd i(in, O_RDONLY);
    Fd o(out, O_WRONLY | O_CREAT | O_TRUNC);
    BgzfWriter w(o.get(), out, level, threads);
    std::vector<uint8_t> buf(chunk);
    for (;;) {
        size_t got = 0;
        while (got < buf.size()) {
            ssize_t r = read(i.get(), buf.data() + got, buf.size() - got);
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) throw PfileError("read " + in + ": " + std::strerror(errno));
            if (r == 0) break;
            got += (size_t)r;
        }
        if (!got) break;
        w.write(buf.data(), got);
    }
    w.finish();
    o.close();
}

const char *kUsage =
    "Usage: pgen-hip <COMMAND>\n\n"
    "Commands:\n"
    "  query   Queries the pgen, outputting to stdout\n"
    "  filter  Filters the pgen, outputting to a VCF\n"
    "  freq    Per-variant genotype counts of the kept samples, outputting to stdout\n"
    "  sample-counts  Per-sample genotype counts over the kept variants, outputting to stdout\n"
    "  score   Polygenic scores of the kept samples from a weights file, outputting to stdout\n"
    "  assoc   Linear regression of quantitative phenotypes (--logistic: logistic regression of case/control phenotypes) on every kept variant, outputting to stdout\n"
    "  matrix  Numeric genotype matrix of the kept variants and samples, outputting to a NumPy .npy file\n"
    "  ld      Pairwise r^2 of the kept variants inside a sliding window, outputting to stdout\n"
    "  prune   LD pruning of the kept variants: writes OUT.prune.in / OUT.prune.out, and with --export the pruned fileset\n"
    "  kinship Pairwise genotype tables and KING-robust kinship of the kept samples, outputting to stdout\n"
    "  grm     Genetic relationship matrix of the kept samples, outputting GCTA-style binary files or a text square\n"
    "  pca     Leading principal components of the kept samples, outputting .eigenval and .eigenvec files\n"
    "  export  Writes the kept variants and samples back as a .pgen (or PLINK 1 .bed) fileset\n"
    "  import  Reads a VCF's GT calls into a .pgen / .pvar / .psam fileset\n"
    "  help    Print this message\n\n"
    "query  <PFILE_PREFIX> -f, --fstring <QUERY_FSTRING> [-i, --include <QUERY>] [-s, --samples]\n"
    "filter <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--launch-mib <M>] [--write-threads <T>] [--read-threads <T>] [--filter-threads <T>] [--stats] [--dry-run]\n"
    "       [--bgzf] [--bgzf-level <1-9>] [--compress-threads <T>]   (BGZF `.vcf.gz`; implied by an OUT_FILE ending in .gz)\n"
    "freq   <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       one line per kept variant: CHROM POS ID REF ALT HOM_REF_CT HET_REF_ALT_CTS TWO_ALT_GENO_CTS MISSING_CT (plink2 .gcount\n"
    "       column names, diploid columns only; byte parity with plink2 is not claimed)\n"
    "sample-counts <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       one line per kept sample in psam order: IID HOM_REF_CT HET_CT HOM_ALT_CT MISSING_CT (the counts of 0/0, 0/1, 1/1 and\n"
    "       ./. over the kept variants; no byte parity with plink2's .scount / .smiss is claimed)\n"
    "score  <PFILE_PREFIX> --weights <FILE> [--no-mean-imputation] [--avg] [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       FILE: tab-separated with a header line: variant ID, effect allele, then one weight column per score (the header cell names it).\n"
    "       Rows are matched by ID among the kept variants; effect allele == ALT scores w * dosage, == REF w * (2 - dosage), another\n"
    "       allele or an ID that is not kept skips the row.  A missing call counts as the variant's mean dosage over the kept samples\n"
    "       (--no-mean-imputation: as 0).  One line per kept sample in psam order: IID ALLELE_CT DENOM <NAME>_SUM ... (--avg: <NAME>_AVG =\n"
    "       SUM / DENOM); weights are rounded to f32, sums are FP64; no byte or digit parity with plink2's .sscore is claimed\n"
    "assoc  <PFILE_PREFIX> --pheno <FILE> [--pheno-name <A,B,...>] [--covar <FILE>] [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       FILEs: tab-separated with a header line: IID, then one quantitative value per column; NA, nan and empty cells are missing.\n"
    "       A kept sample stays only with every chosen phenotype and every covariate.  Per variant and phenotype a linear regression on\n"
    "       the ALT dosage with an intercept and the covariates: CHROM POS ID REF ALT A1 PHENO OBS_CT MISS_CT A1_FREQ BETA SE T_STAT P\n"
    "       (NA where the fit is degenerate).  A missing call counts as the variant's mean dosage over the called samples (mean\n"
    "       imputation); plink2 --glm drops the sample for that variant instead, so no digit parity with plink2 is claimed\n"
    "assoc  --p-of <T_STAT> <DF>   the two-sided Student t P value of one statistic (no fileset, no device)\n"
    "assoc --logistic <PFILE_PREFIX> --pheno <FILE> [--pheno-name <A,B,...>] [--covar <FILE>] [--no-mean-imputation] [--max-iter <I>] [--tol <X>] [...as assoc]\n"
    "       case/control phenotypes: every value of a column 1 or 2 with a 2 present (control / case), or every value 0 or 1 (0 control).  Per\n"
    "       variant and phenotype a logistic regression on the ALT dosage with an intercept and up to 14 covariates, fitted on the device by\n"
    "       Newton's iteration from the null model, at most I evaluations (default 25, 1 .. 64), converged when no coefficient moves by more\n"
    "       than X (default 1e-9): CHROM POS ID REF ALT A1 PHENO OBS_CT MISS_CT A1_FREQ BETA SE Z_STAT P ITER STATUS.  BETA is the log-odds per\n"
    "       ALT allele, P = erfc(|Z| / sqrt 2) the Wald test; STATUS is . / NOT_CONVERGED / SINGULAR and BETA SE Z_STAT P are NA unless the fit\n"
    "       converged.  A missing call counts as the variant's mean dosage (--no-mean-imputation: the sample is dropped for that variant, as\n"
    "       plink2 does, and OBS_CT excludes it).  Not built: a Firth fallback, step halving (a separated variant ends NOT_CONVERGED or\n"
    "       SINGULAR), likelihood-ratio tests, per-genotype case/control counts, interaction terms, more than 14 covariates; no digit parity\n"
    "       with plink2 --glm is claimed\n"
    "assoc  --p-of-z <Z_STAT>      the two-sided normal (Wald) P value of one statistic (no fileset, no device)\n"
    "matrix <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [--dtype i8|f16|f32] [--missing <X>] [--sample-major]\n"
    "       -o, --out <OUT_FILE.npy> [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       NumPy .npy (version 1.0, C order) of shape (variants kept, samples kept), or (samples, variants) with --sample-major:\n"
    "       0 / 1 / 2 alternate alleles, --missing (default -1 for i8, nan for f16 / f32) for ./.; the kept variants' ID column in\n"
    "       OUT_FILE.npy.variants and the kept samples' IID column in OUT_FILE.npy.samples, one per line\n"
    "ld     <PFILE_PREFIX> --window <W> [--min-r2 <X>] [--counts] [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--block-rows <B>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       one line per pair of kept variants on one chromosome at most W kept variants apart with r^2 >= X (default 0.2; NaN pairs\n"
    "       are dropped): CHROM_A POS_A ID_A CHROM_B POS_B ID_B R2, ordered by first variant and distance; --counts appends N_OBS\n"
    "       and the pair's 4 x 4 genotype table T00 .. T33.  r^2 is the unphased genotype correlation over the kept samples called\n"
    "       in both variants; no digit parity with plink2 is claimed\n"
    "export <PFILE_PREFIX> -o, --out <OUT_PREFIX> [--format pgen|bed] [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       the kept variants and samples as OUT_PREFIX.pgen (fixed-width, storage mode 0x02), .pvar (the header lines and the kept\n"
    "       rows) and .psam; --format bed: PLINK 1 OUT_PREFIX.bed (variant-major, ALT as A1), .bim (CHROM ID 0 POS ALT REF) and .fam\n"
    "       (FID IID PAT MAT SEX -9; 0 for a missing column).  OUT_PREFIX must not name the input; no byte parity with plink2 is claimed\n"
    "import <IN.vcf[.gz]> -o, --out <OUT_PREFIX> [--skip-multiallelic] [--block-mib <M>] [--stats]\n"
    "       the VCF's biallelic GT hard calls as OUT_PREFIX.pgen (fixed-width, storage mode 0x02), .pvar (the ## lines but ##fileformat= and\n"
    "       `##source=pgen-rs`, which filter adds itself, and the columns in front of FORMAT, verbatim) and .psam (#IID SEX, with NA), so that\n"
    "       `filter` on OUT_PREFIX gives back a VCF that `filter` wrote.  GT must be the first FORMAT key; calls are 0, 1 and '.' with '/' or\n"
    "       '|' (the phase is dropped; a half call and a haploid '.' are missing, haploid 0 / 1 are 0/0 / 1/1; the lines with any of the three\n"
    "       are counted and warned about once each).  Any other call, another allele (what a multiallelic line holds: --skip-multiallelic\n"
    "       drops the lines whose ALT has a ',' and counts them), or a line with too few columns or fields is an error that names the input's line and leaves no\n"
    "       output file.  A gzip or BGZF input is inflated by one sequential zlib stream over its members (parallel inflate of BGZF members is\n"
    "       not built); one device is used whatever --gpus says: the reader, not the parse kernel, bounds this command.  Compressed .pgen\n"
    "       records and BCF are not read\n"
    "merge  <PFILE_PREFIX> <PFILE_PREFIX> [<PFILE_PREFIX> ...] -o, --out <OUT_PREFIX> [--union] [--block-mib <M>] [--read-threads <T>] [--stats] [--dry-run]\n"
    "       two to eight filesets' samples side by side (more: merge in stages) as OUT_PREFIX.pgen (fixed-width, storage mode 0x02), .pvar\n"
    "       and .psam: the inputs' samples in argument order (column lines byte-identical, no IID twice).  A variant is (CHROM, POS, {REF,\n"
    "       ALT}), strings compared verbatim; an input that has REF and ALT exchanged against the first input that holds the variant is\n"
    "       flipped (0/0 <-> 1/1), and that first input's .pvar row is written (a differing ID in a later input is counted, not an error).\n"
    "       Default: the variants every input holds, in the first input's order; --union: every variant, sorted by (CHROM by first\n"
    "       appearance, POS, first seen), an input that lacks one is ./. there.  Strand flips (A/G against T/C) are not detected; differing\n"
    "       columns are not harmonised; one device is used.  --dry-run matches and prints the counts as one JSON line, without a device or a file\n"
    "prune  <PFILE_PREFIX> (--window <W> | --window-kb <KB> [--window <W>]) --r2 <X> -o, --out <OUT_PREFIX> [--export]\n"
    "       [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [--block-mib <M>] [--block-rows <B>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       OUT_PREFIX.prune.in: the IDs of the kept variants that stay, one per line in file order; OUT_PREFIX.prune.out: the removed ones'.\n"
    "       Two kept variants on one chromosome, at most W variants apart (with --window-kb: at most KB x 1000 base pairs apart, and W\n"
    "       is then the most variants such a span holds, capped by --window), are linked when their unphased genotype r^2 over the kept\n"
    "       samples (ld's R2, as float32) is above X.  Variants are taken by minor-allele frequency among called alleles, the more common\n"
    "       first, ties to the earlier one; each stays unless a linked variant before it in that order stayed.  So no two variants that\n"
    "       stay inside a window have r^2 above X, and every removed variant has a kept, more common (or equally common, earlier) variant\n"
    "       inside its window with r^2 above X.  A monomorphic or uncalled variant has no r^2, hence no link, and stays; MAF filters are\n"
    "       not part of this.  --export also writes OUT_PREFIX.pgen / .pvar / .psam with the variants that stay and the kept samples, as\n"
    "       `export` would.  One device is used; the result does not depend on --block-rows.  No parity with plink2 --indep-pairwise is\n"
    "       claimed: its result depends on its window stepping.  Prints one JSON line: kept, removed, edges, window, resolve_calls, mask_bytes\n"
    "kinship <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [--min-kinship <X>] [--counts] [-o, --out <OUT_FILE>]\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--block-rows <B>] [--sample-tile <T>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       one line per pair of kept samples in psam order: IID1 IID2 N HETHET IBS0 HET1 HET2 KINSHIP over the kept variants called in\n"
    "       both samples; KINSHIP = 0.5 - (HET1 + HET2 - 2 HETHET + 4 IBS0) / (4 min(HET1, HET2)) is the KING-robust between-family\n"
    "       estimator (nan when min(HET1, HET2) is 0); --counts appends the pair's 4 x 4 genotype table T00 .. T33; --min-kinship drops\n"
    "       the lines below X and the nan lines.  The tables of all pairs (32 bytes x kept samples squared) are held on each device in\n"
    "       square tiles of T ranks (default 1024): out-of-core sample tiling is not built, and a sample set whose tables do not fit\n"
    "       fails with an out-of-memory error.  No byte or digit parity with plink2's .kin0 or KING is claimed\n"
    "grm    <PFILE_PREFIX> [--include-var <VAR_QUERY>] [--include-sam <SAM_QUERY>] [--format grm-bin|rel] -o, --out <OUT_PREFIX>\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--block-rows <B>] [--sample-tile <T>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       GRM[a][b] = G[a][b] / N[a][b] over the kept variants called in both samples (GCTA's definition; nan where N is 0):\n"
    "       G sums (x_a - 2p)(x_b - 2p) / (2p(1-p)) with p the variant's ALT frequency among the kept samples called, N counts the\n"
    "       variants; a variant with no call or with p of 0 or 1 adds to neither (--stats reports how many).  --format grm-bin (default):\n"
    "       OUT_PREFIX.grm.bin and .grm.N.bin (little-endian f32, lower triangle with the diagonal, row a then b = 0..a) and .grm.id\n"
    "       (FID IID with FID = IID); --format rel: OUT_PREFIX.rel (K lines of K tab-separated values, %.17g) and .rel.id.  Both matrices\n"
    "       (16 bytes x kept samples squared) are held on each device in square tiles of T ranks (default 1024) and on the host:\n"
    "       out-of-core sample tiling is not built, and a sample set whose matrices do not fit fails with an out-of-memory error.\n"
    "       Sums are FP64 in no fixed order; no byte or digit parity with plink2 or GCTA is claimed\n"
    "pca    <PFILE_PREFIX> [--include-sam <SAM_QUERY>] [--include-var <VAR_QUERY>] [--pcs <P>] [--tol <X>] [--max-passes <I>] [--seed <S>] -o, --out <OUT_PREFIX>\n"
    "       [--gpus <N>] [--shards <S>] [--block-mib <M>] [--block-rows <B>] [--read-threads <T>] [--filter-threads <T>] [--stats]\n"
    "       the P (default 10, 1 .. 32) leading principal components of M = Z^T Z / V_used, Z the kept variants' standardised genotypes\n"
    "       (x - 2p) / sqrt(2p(1-p)) with a missing call at the variant's mean (plink2 --pca's convention; grm's G / N is pairwise-complete\n"
    "       and differs wherever calls are missing); a variant with no call or with p of 0 or 1 is skipped (--stats reports how many).\n"
    "       The K x K matrix is never formed: randomised subspace iteration on min(K, P + 10) columns with Rayleigh-Ritz in every pass,\n"
    "       each pass one Gram product over all records, until the residuals of the P pairs are <= X * lambda_1 (default 1e-6) or after I\n"
    "       passes (default 100: a warning, exit 0, \"converged\": false under --stats beside passes and residual).  OUT_PREFIX.eigenval: P\n"
    "       lines; OUT_PREFIX.eigenvec: #IID PC1 .. PCP, one line per kept sample, unit-norm vectors, %.17g.  No digit parity with plink2 is claimed\n"
    "bgzf   <IN_FILE> <OUT_FILE> [--level <1-9>] [--threads <T>] [--chunk-mib <M>]\n";

[[noreturn]] void usage_error(const std::string &msg)
{
    std::fprintf(stderr, "error: %s\n\n%s", msg.c_str(), kUsage);
    std::exit(2);
}

struct Args {
    std::vector<std::string> positional;
    std::vector<std::pair<std::string, std::string>> options;  // name (without dashes) -> value ("" for flags)
    bool has(const std::string &n) const
    {
        for (const auto &o : options)
            if (o.first == n) return true;
        return false;
    }
    std::optional<std::string> get(const std::string &n) const
    {
        std::optional<std::string> v;
        for (const auto &o : options)
            if (o.first == n) v = o.second;
        return v;
    }
    // the value of an option the command cannot do without (shown: the option as the usage text words it); an empty one is none
    std::string required(const std::string &n, const char *shown) const
    {
        if (!has(n) || get(n)->empty()) usage_error(std::string("the following required arguments were not provided: ") + shown);
        return *get(n);
    }
    // --format: one of the command's two, the first when the option is absent
    std::string format(const std::string &first, const std::string &second) const
    {
        const std::string f = get("format").value_or(first);
        if (f != first && f != second) usage_error("invalid value '" + f + "' for '--format <FORMAT>' [possible values: " + first + ", " + second + "]");
        return f;
    }
};

// clap-style: long `--name value` / `--name=value`, short `-f value` / `-fvalue`, flags without values
Args parse(int argc, char **argv, int first, const std::vector<std::pair<std::string, char>> &valued,
           const std::vector<std::pair<std::string, char>> &flags)
{
    Args a;
    auto long_of_short = [&](char c, bool &is_flag) -> std::string {
        for (const auto &v : valued)
            if (v.second == c) { is_flag = false; return v.first; }
        for (const auto &f : flags)
            if (f.second == c) { is_flag = true; return f.first; }
        return std::string();
    };
    auto is_valued = [&](const std::string &n) {
        for (const auto &v : valued)
            if (v.first == n) return true;
        return false;
    };
    auto is_flag = [&](const std::string &n) {
        for (const auto &f : flags)
            if (f.first == n) return true;
        return false;
    };
    bool only_positional = false;
    for (int i = first; i < argc; i++) {
        std::string s = argv[i];
        if (only_positional || s.size() < 2 || s[0] != '-') {
            a.positional.push_back(s);
            continue;
        }
        if (s == "--") {
            only_positional = true;
            continue;
        }
        if (s[1] == '-') {
            std::string name = s.substr(2), value;
            const size_t eq = name.find('=');
            const bool inline_value = eq != std::string::npos;
            if (inline_value) {
                value = name.substr(eq + 1);
                name = name.substr(0, eq);
            }
            if (is_valued(name)) {
                if (!inline_value) {
                    if (i + 1 >= argc) usage_error("a value is required for '--" + name + "' but none was supplied");
                    value = argv[++i];
                }
                a.options.emplace_back(name, value);
            } else if (is_flag(name)) {
                a.options.emplace_back(name, "");
            } else {
                usage_error("unexpected argument '--" + name + "' found");
            }
        } else {
            bool flag = false;
            const std::string name = long_of_short(s[1], flag);
            if (name.empty()) usage_error(std::string("unexpected argument '-") + s[1] + "' found");
            if (flag) {
                a.options.emplace_back(name, "");
            } else {
                std::string value = s.substr(2);
                if (!value.empty() && value[0] == '=') value = value.substr(1);
                if (s.size() == 2) {
                    if (i + 1 >= argc) usage_error("a value is required for '-" + std::string(1, s[1]) + "' but none was supplied");
                    value = argv[++i];
                }
                a.options.emplace_back(name, value);
            }
        }
    }
    return a;
}

// the options filter and freq share
OutputOptions output_options(const Args &a)
{
    OutputOptions opt;
    if (auto f = a.get("filter-threads")) opt.filter_threads = std::max(1, std::atoi(f->c_str()));
    if (auto g = a.get("gpus")) opt.n_gpus = std::max(1, std::atoi(g->c_str()));
    if (auto sh = a.get("shards")) opt.n_shards = std::max(1, std::atoi(sh->c_str()));
    if (auto w = a.get("read-threads")) opt.read_threads = std::max(1, std::atoi(w->c_str()));
    if (auto m = a.get("block-mib")) opt.block_text_bytes = (uint64_t)std::max(1, std::atoi(m->c_str())) << 20;
    return opt;
}

// IEEE binary32 -> binary16 bits, round to nearest even; out_of_range: a finite value that does not stay finite
uint16_t f32_to_f16(float f, bool &out_of_range)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mant = x & 0x7FFFFFu;
    const int32_t exp = (int32_t)((x >> 23) & 0xFFu);
    out_of_range = false;
    if (exp == 0xFF) return (uint16_t)(sign | 0x7C00u | (mant ? 0x200u | (mant >> 13) : 0u));   // inf / nan (quiet)
    const int32_t e = exp - 127 + 15;
    if (e >= 0x1F) {
        out_of_range = true;
        return (uint16_t)(sign | 0x7C00u);
    }
    if (e <= 0) {   // subnormal or zero
        if (e < -10) return (uint16_t)sign;
        const uint32_t m = mant | 0x800000u;
        const uint32_t shift = (uint32_t)(14 - e);
        uint32_t h = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    uint32_t h = ((uint32_t)e << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    if (h >= 0x7C00u) out_of_range = true;
    return (uint16_t)(sign | h);
}

// --dtype / --missing of `matrix`: the element type and the four patterns (0, 1, 2, missing)
MatrixOptions matrix_options(const Args &a)
{
    MatrixOptions m;
    const std::string dtype = a.get("dtype").value_or("i8");
    const std::optional<std::string> missing = a.get("missing");
    m.sample_major = a.has("sample-major");
    std::memset(m.values, 0, sizeof m.values);
    if (dtype == "i8") {
        long v = -1;
        if (missing) {
            char *end = nullptr;
            errno = 0;
            v = std::strtol(missing->c_str(), &end, 10);
            if (missing->empty() || *end != '\0' || errno != 0 || v < -128 || v > 127)
                usage_error("invalid value '" + *missing + "' for '--missing <X>': i8 takes an integer in -128 .. 127");
        }
        m.elem_bytes = 1;
        m.descr = "|i1";
        const int8_t vals[4] = {0, 1, 2, (int8_t)v};
        std::memcpy(m.values, vals, 4);
    } else if (dtype == "f16" || dtype == "f32") {
        float v = std::nanf("");
        if (missing) {
            char *end = nullptr;
            errno = 0;
            v = std::strtof(missing->c_str(), &end);
            if (missing->empty() || *end != '\0' || (errno == ERANGE && std::isinf(v)))
                usage_error("invalid value '" + *missing + "' for '--missing <X>': " + dtype + " takes a number it can hold, inf or nan");
        }
        const float vals[4] = {0.0f, 1.0f, 2.0f, v};
        if (dtype == "f32") {
            m.elem_bytes = 4;
            m.descr = "<f4";
            std::memcpy(m.values, vals, 16);
        } else {
            m.elem_bytes = 2;
            m.descr = "<f2";
            for (int c = 0; c < 4; c++) {
                bool range = false;
                const uint16_t h = f32_to_f16(vals[c], range);
                if (range) usage_error("invalid value '" + *missing + "' for '--missing <X>': f16 takes a number it can hold, inf or nan");
                std::memcpy(m.values + 2 * c, &h, 2);
            }
        }
    } else {
        usage_error("invalid value '" + dtype + "' for '--dtype <DTYPE>' [possible values: i8, f16, f32]");
    }
    return m;
}

// the times that end every --stats line (OutputStats or MergeStats): the "seconds_*" members, seconds_main up to now
template <class Stats>
std::string seconds_json(const Stats &st, std::chrono::steady_clock::time_point t_main)
{
    char buf[200];
    std::snprintf(buf, sizeof buf, "\"seconds_filter\": %.6f, \"seconds_body\": %.6f, \"seconds_setup\": %.6f, \"seconds_kernel\": %.6f, \"seconds_main\": %.6f",
                  st.seconds_filter, st.seconds_body, st.seconds_setup, st.seconds_kernel, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main).count());
    return buf;
}

// --stats: one JSON line on stderr
void print_stats(const OutputStats &st, std::chrono::steady_clock::time_point t_main)
{
    std::fprintf(stderr, "{\"variants_kept\": %llu, \"samples_kept\": %llu, \"header_bytes\": %llu, \"body_bytes\": %llu, \"file_bytes\": %llu, %s}\n",
                 (unsigned long long)st.variants, (unsigned long long)st.samples_kept, (unsigned long long)st.header_bytes,
                 (unsigned long long)st.body_bytes, (unsigned long long)st.file_bytes, seconds_json(st, t_main).c_str());
}

// The arguments of a command that takes filter's selection: the options every such command has and --stats, beside the command's
// own valued options and flags, and exactly one positional argument, the fileset's prefix
struct SelectionArgs : Args {
    SelectionArgs(int argc, char **argv, std::vector<std::pair<std::string, char>> valued, std::vector<std::pair<std::string, char>> flags)
    {
        for (const char *name : {"include-var", "include-sam", "gpus", "shards", "block-mib", "read-threads", "filter-threads"}) valued.emplace_back(name, 0);
        valued.emplace_back("out", 'o');
        flags.emplace_back("stats", 0);
        static_cast<Args &>(*this) = parse(argc, argv, 2, valued, flags);
        if (positional.size() != 1) usage_error("the following required arguments were not provided: <PFILE_PREFIX>");
    }
    // the command's last step: the --stats line (behind the lines the command itself has printed)
    int done(const OutputStats &st, std::chrono::steady_clock::time_point t_main) const
    {
        if (has("stats")) print_stats(st, t_main);
        return 0;
    }
};

// `--name <PLACEHOLDER>` as a whole number in [lo, hi]; `what` ends the message for anything else
unsigned long long unsigned_value(const std::string &s, const char *name, const char *placeholder, unsigned long long lo, unsigned long long hi, const char *what)
{
    char *end = nullptr;
    errno = 0;
    const unsigned long long v = std::strtoull(s.c_str(), &end, 10);
    if (s.empty() || s[0] == '-' || *end != '\0' || errno != 0 || v < lo || v > hi)
        usage_error("invalid value '" + s + "' for '--" + name + " <" + placeholder + ">': " + what);
    return v;
}

// the same for a number in [lo, hi] (a NaN is in no range)
double double_value(const std::string &s, const char *name, const char *placeholder, double lo, double hi, const char *what)
{
    char *end = nullptr;
    errno = 0;
    const double v = std::strtod(s.c_str(), &end);
    if (s.empty() || *end != '\0' || errno != 0 || !(v >= lo && v <= hi))
        usage_error("invalid value '" + s + "' for '--" + name + " <" + placeholder + ">': " + what);
    return v;
}

constexpr unsigned long long kNoLimit = ~0ull;
uint64_t block_rows_value(const std::string &s) { return unsigned_value(s, "block-rows", "B", 1, kNoLimit, "a number of variants from 1"); }
uint64_t block_mib_value(const std::string &s) { return unsigned_value(s, "block-mib", "M", 1, 65536, "a number of MiB from 1 to 65536") << 20; }   // import, merge: bytes
uint32_t sample_tile_value(const std::string &s) { return (uint32_t)unsigned_value(s, "sample-tile", "T", 1, 65536, "a number of samples from 1 to 65536"); }

}  // namespace

int main(int argc, char **argv)
{
    const auto t_main = std::chrono::steady_clock::now();
    if (argc < 2) usage_error("a subcommand is required");
    const std::string cmd = argv[1];
    try {
        if (cmd == "help" || cmd == "--help" || cmd == "-h") {
            std::fputs(kUsage, stdout);
            return 0;
        }
        if (cmd == "--version" || cmd == "-V") {
            std::puts("pgen-hip 0.1.0 (MI355X engine for pgen-rs's filter/query surface)");
            return 0;
        }
        if (cmd == "query") {  // src/main.rs:95-113
            Args a = parse(argc, argv, 2, {{"fstring", 'f'}, {"include", 'i'}}, {{"samples", 's'}});
            if (a.positional.size() != 1) usage_error("the following required arguments were not provided: <PFILE_PREFIX>");
            if (!a.has("fstring")) usage_error("the following required arguments were not provided: --fstring <QUERY_FSTRING>");
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const std::string path = a.has("samples") ? pfile.psam_path() : pfile.pvar_path();
            const std::string data = read_file(path);
            TsvReader reader(data, Pfile::find_metadata_file_header_start(data));
            std::string out;
            Pfile::query_metadata(reader, a.get("include"), *a.get("fstring"), out);
            std::fwrite(out.data(), 1, out.size(), stdout);
            return 0;
        }
        if (cmd == "filter") {  // src/main.rs:114-124
            const SelectionArgs a(argc, argv, {{"launch-mib", 0}, {"write-threads", 0}, {"bgzf-level", 0}, {"compress-threads", 0}}, {{"dry-run", 0}, {"bgzf", 0}});
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            auto ends_with = [](const std::string &x, const char *suffix) { const size_t n = std::strlen(suffix); return x.size() >= n && x.compare(x.size() - n, n, suffix) == 0; };
            const bool bgzf = a.has("bgzf") || (a.get("out") && ends_with(*a.get("out"), ".gz"));
            const std::string out_file = a.get("out").value_or(pfile.pfile_prefix + (bgzf ? ".pgen-rs.vcf.gz" : ".pgen-rs.vcf"));  // :121-122
            const int bgzf_level = a.get("bgzf-level") ? std::atoi(a.get("bgzf-level")->c_str()) : 6;
            if (bgzf_level < 1 || bgzf_level > 9) usage_error("--bgzf-level takes 1 .. 9");
            OutputOptions opt = output_options(a);
            if (a.has("dry-run")) {
                // header + geometry only: the plumbing of BASELINE config 1 without touching a GPU
                const Pfile::Selection sel = pfile.select(a.get("include-sam"), a.get("include-var"), opt.filter_threads);
                const auto &vars = sel.var_idx_rcds, &sams = sel.sam_idx_rcs;
                const std::string header = pfile.vcf_header(sams, sel.sam_header);
                write_header_only(out_file, header, bgzf, bgzf_level);
                unsigned long long prefix = 0;
                for (const auto &v : vars) {
                    prefix += 2;
                    for (const auto &c : v.second) prefix += c.size() + 1;
                }
                const unsigned long long body = prefix + (unsigned long long)vars.size() * (4ull * sams.size() + 1ull);
                std::printf("{\"variants_kept\": %zu, \"samples_kept\": %zu, \"header_bytes\": %zu, \"prefix_bytes\": %llu, \"body_bytes\": %llu, \"file_bytes\": %llu}\n",
                            vars.size(), sams.size(), header.size(), prefix, body, (unsigned long long)header.size() + body);
                return 0;
            }
            opt.bgzf = bgzf;
            opt.bgzf_level = bgzf_level;
            if (auto c = a.get("compress-threads")) opt.compress_threads = std::max(1, std::atoi(c->c_str()));
            if (auto w = a.get("write-threads")) opt.write_threads = std::max(1, std::atoi(w->c_str()));
            if (auto m = a.get("launch-mib")) opt.launch_bytes = (uint64_t)std::max(1, std::atoi(m->c_str())) << 20;
            return a.done(pfile.output_vcf(a.get("include-sam"), a.get("include-var"), out_file, opt), t_main);  // :123
        }
        if (cmd == "freq") {
            const SelectionArgs a(argc, argv, {}, {});
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_freq(a.get("include-sam"), a.get("include-var"), a.get("out").value_or(""), output_options(a)), t_main);
        }
        if (cmd == "sample-counts") {
            const SelectionArgs a(argc, argv, {}, {});
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_sample_counts(a.get("include-sam"), a.get("include-var"), a.get("out").value_or(""), output_options(a)), t_main);
        }
        if (cmd == "score") {
            const SelectionArgs a(argc, argv, {{"weights", 0}}, {{"no-mean-imputation", 0}, {"avg", 0}});
            const std::string weights = a.required("weights", "--weights <FILE>");
            ScoreOptions s;
            s.mean_imputation = !a.has("no-mean-imputation");
            s.average = a.has("avg");
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const OutputStats st = pfile.output_score(a.get("include-sam"), a.get("include-var"), weights, a.get("out").value_or(""), s, output_options(a));
            if (a.has("stats"))
                std::fprintf(stderr, "{\"weights_matched\": %llu, \"weights_flipped\": %llu, \"weights_skipped\": %llu}\n",
                             (unsigned long long)st.score_matched, (unsigned long long)st.score_flipped, (unsigned long long)st.score_skipped);
            return a.done(st, t_main);
        }
        if (cmd == "assoc") {
            if (argc >= 3 && std::string(argv[2]) == "--p-of") {
                char *e1 = nullptr, *e2 = nullptr;
                const double t = argc == 5 ? std::strtod(argv[3], &e1) : 0.0, df = argc == 5 ? std::strtod(argv[4], &e2) : 0.0;
                if (argc != 5 || *argv[3] == '\0' || *e1 != '\0' || *argv[4] == '\0' || *e2 != '\0' || !(df > 0)) usage_error("--p-of takes a statistic and its degrees of freedom (> 0)");
                std::printf("%.17g\n", stats::student_t_two_sided_p(t, df));
                return 0;
            }
            if (argc >= 3 && std::string(argv[2]) == "--p-of-z") {
                char *e1 = nullptr;
                const double z = argc == 4 ? std::strtod(argv[3], &e1) : 0.0;
                if (argc != 4 || *argv[3] == '\0' || *e1 != '\0') usage_error("--p-of-z takes one statistic");
                std::printf("%.17g\n", stats::wald_p(z));
                return 0;
            }
            const SelectionArgs a(argc, argv, {{"pheno", 0}, {"pheno-name", 0}, {"covar", 0}, {"max-iter", 0}, {"tol", 0}}, {{"logistic", 0}, {"no-mean-imputation", 0}});
            if (!a.has("logistic"))   // the options of the logistic fit do not exist without it
                for (const char *name : {"no-mean-imputation", "max-iter", "tol"})
                    if (a.has(name)) usage_error(std::string("unexpected argument '--") + name + "' found");
            const std::string pheno = a.required("pheno", "--pheno <FILE>");
            if (a.has("covar") && a.get("covar")->empty()) usage_error("a value is required for '--covar <FILE>'");
            AssocOptions ao;
            ao.pheno_file = pheno;
            ao.covar_file = a.get("covar").value_or("");
            if (a.has("pheno-name")) {
                std::string name;
                for (const char ch : *a.get("pheno-name") + ",") {
                    if (ch != ',') {
                        name += ch;
                        continue;
                    }
                    if (name.empty()) usage_error("--pheno-name takes column names separated by commas");
                    ao.pheno_names.push_back(name);
                    name.clear();
                }
            }
            if (a.has("logistic")) {
                ao.logistic = true;
                ao.mean_imputation = !a.has("no-mean-imputation");
                if (a.has("max-iter")) ao.max_iter = (uint32_t)unsigned_value(*a.get("max-iter"), "max-iter", "I", 1, PGENHIP_LOGIT_MAX_ITER, "a number of evaluations from 1 to 64");
                if (a.has("tol")) {
                    char *end = nullptr;
                    ao.tol = std::strtod(a.get("tol")->c_str(), &end);
                    if (a.get("tol")->empty() || *end != '\0' || !(ao.tol >= 0.0) || std::isinf(ao.tol)) usage_error("invalid value '" + *a.get("tol") + "' for '--tol <X>': not a finite number >= 0");
                }
            }
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const OutputStats st = pfile.output_assoc(a.get("include-sam"), a.get("include-var"), ao, a.get("out").value_or(""), output_options(a));
            if (a.has("stats") && ao.logistic)
                std::fprintf(stderr, "{\"samples_dropped\": %llu, \"converged\": %llu, \"not_converged\": %llu, \"singular\": %llu}\n", (unsigned long long)st.assoc_dropped,
                             (unsigned long long)st.logit_converged, (unsigned long long)st.logit_not_converged, (unsigned long long)st.logit_singular);
            else if (a.has("stats")) std::fprintf(stderr, "{\"samples_dropped\": %llu}\n", (unsigned long long)st.assoc_dropped);
            return a.done(st, t_main);
        }
        if (cmd == "matrix") {
            const SelectionArgs a(argc, argv, {{"dtype", 0}, {"missing", 0}}, {{"sample-major", 0}});
            const std::string out = a.required("out", "--out <OUT_FILE.npy>");
            const MatrixOptions m = matrix_options(a);
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_matrix(a.get("include-sam"), a.get("include-var"), out, m, output_options(a)), t_main);
        }
        if (cmd == "export") {
            const SelectionArgs a(argc, argv, {{"format", 0}}, {});
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            ExportOptions e;
            e.bed = a.format("pgen", "bed") == "bed";
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_export(a.get("include-sam"), a.get("include-var"), out, e, output_options(a)), t_main);
        }
        if (cmd == "import") {
            Args a = parse(argc, argv, 2, {{"out", 'o'}, {"block-mib", 0}}, {{"skip-multiallelic", 0}, {"stats", 0}});
            if (a.positional.size() != 1) usage_error("the following required arguments were not provided: <IN.vcf[.gz]>");
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            ImportOptions io;
            io.skip_multiallelic = a.has("skip-multiallelic");
            OutputOptions opt;
            if (auto m = a.get("block-mib")) opt.block_text_bytes = block_mib_value(*m);
            const OutputStats st = import_vcf(a.positional[0], out, io, opt);
            if (a.has("stats"))
                std::fprintf(stderr,
                             "{\"variants\": %llu, \"samples\": %llu, \"skipped_multiallelic\": %llu, \"half_call_lines\": %llu, \"haploid_lines\": %llu, "
                             "\"phased_lines\": %llu, \"file_bytes\": %llu, %s}\n",
                             (unsigned long long)st.variants, (unsigned long long)st.samples_kept, (unsigned long long)st.import_skipped,
                             (unsigned long long)st.import_half_call, (unsigned long long)st.import_haploid, (unsigned long long)st.import_phased,
                             (unsigned long long)st.file_bytes, seconds_json(st, t_main).c_str());
            return 0;
        }
        if (cmd == "merge") {
            Args a = parse(argc, argv, 2, {{"out", 'o'}, {"block-mib", 0}, {"read-threads", 0}}, {{"union", 0}, {"stats", 0}, {"dry-run", 0}});
            if (a.positional.size() < 2) usage_error("merge takes at least two <PFILE_PREFIX> arguments");
            if (a.positional.size() > PGENHIP_JOIN_MAX_PARTS) usage_error("merge takes at most eight <PFILE_PREFIX> arguments: merge in stages");
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            MergeOptions mo;
            mo.with_union = a.has("union");
            mo.dry_run = a.has("dry-run");
            OutputOptions opt;
            if (auto m = a.get("block-mib")) opt.block_text_bytes = block_mib_value(*m);
            if (auto t = a.get("read-threads")) opt.read_threads = (int)unsigned_value(*t, "read-threads", "T", 1, 256, "a number of threads from 1 to 256");
            const MergeStats st = merge_pfiles(a.positional, out, mo, opt);
            if (mo.dry_run) {
                std::printf("{%s}\n", st.json_counts().c_str());
            } else if (a.has("stats")) {
                std::fprintf(stderr, "{%s, \"file_bytes\": %llu, %s}\n", st.json_counts().c_str(), (unsigned long long)st.file_bytes, seconds_json(st, t_main).c_str());
            }
            return 0;
        }
        if (cmd == "ld") {
            const SelectionArgs a(argc, argv, {{"window", 0}, {"min-r2", 0}, {"block-rows", 0}}, {{"counts", 0}});
            if (!a.has("window")) usage_error("the following required arguments were not provided: --window <W>");
            LdOptions ld;
            ld.window = (uint32_t)unsigned_value(*a.get("window"), "window", "W", 1, 0xFFFFFFFFull, "a number of variants from 1 to 4294967295");
            if (auto m = a.get("min-r2")) ld.min_r2 = double_value(*m, "min-r2", "X", 0.0, 1.0, "a number from 0 to 1");
            if (auto b = a.get("block-rows")) ld.block_rows = block_rows_value(*b);
            ld.counts = a.has("counts");
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_ld(a.get("include-sam"), a.get("include-var"), a.get("out").value_or(""), ld, output_options(a)), t_main);
        }
        if (cmd == "prune") {
            const SelectionArgs a(argc, argv, {{"window", 0}, {"window-kb", 0}, {"r2", 0}, {"block-rows", 0}}, {{"export", 0}});
            if (!a.has("window") && !a.has("window-kb")) usage_error("the following required arguments were not provided: --window <W> or --window-kb <KB>");
            if (!a.has("r2")) usage_error("the following required arguments were not provided: --r2 <X>");
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            PruneOptions po;
            if (auto w = a.get("window")) po.window = (uint32_t)unsigned_value(*w, "window", "W", 1, 0xFFFFFFFFull, "a number of variants from 1 to 4294967295");
            if (auto k = a.get("window-kb")) {
                po.window_kb = unsigned_value(*k, "window-kb", "KB", 0, 4294967ull, "a number of kilobases from 0 to 4294967");
                po.has_window_kb = true;
            }
            po.min_r2 = double_value(*a.get("r2"), "r2", "X", 0.0, 1.0, "a number from 0 to 1");
            if (auto b = a.get("block-rows")) po.block_rows = block_rows_value(*b);
            po.with_export = a.has("export");
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const OutputStats st = pfile.output_prune(a.get("include-sam"), a.get("include-var"), out, po, output_options(a));
            std::printf("{\"kept\": %llu, \"removed\": %llu, \"edges\": %llu, \"window\": %llu, \"resolve_calls\": %llu, \"mask_bytes\": %llu}\n",
                        (unsigned long long)st.prune_kept, (unsigned long long)st.prune_removed, (unsigned long long)st.prune_edges,
                        (unsigned long long)st.prune_window, (unsigned long long)st.prune_calls, (unsigned long long)st.prune_mask_bytes);
            std::fflush(stdout);
            return a.done(st, t_main);
        }
        if (cmd == "kinship") {
            const SelectionArgs a(argc, argv, {{"min-kinship", 0}, {"sample-tile", 0}, {"block-rows", 0}}, {{"counts", 0}});
            KinshipOptions k;
            if (auto m = a.get("min-kinship")) {
                k.min_kinship = double_value(*m, "min-kinship", "X", -DBL_MAX, DBL_MAX, "a finite number");
                k.has_min = true;
            }
            if (auto t = a.get("sample-tile")) k.tile = sample_tile_value(*t);
            if (auto b = a.get("block-rows")) k.block_rows = block_rows_value(*b);
            k.counts = a.has("counts");
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            return a.done(pfile.output_kinship(a.get("include-sam"), a.get("include-var"), a.get("out").value_or(""), k, output_options(a)), t_main);
        }
        if (cmd == "grm") {
            const SelectionArgs a(argc, argv, {{"format", 0}, {"sample-tile", 0}, {"block-rows", 0}}, {});
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            GrmOptions g;
            g.rel = a.format("grm-bin", "rel") == "rel";
            if (auto t = a.get("sample-tile")) g.tile = sample_tile_value(*t);
            if (auto b = a.get("block-rows")) g.block_rows = block_rows_value(*b);
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const OutputStats st = pfile.output_grm(a.get("include-sam"), a.get("include-var"), out, g, output_options(a));
            if (a.has("stats")) std::fprintf(stderr, "{\"variants_skipped\": %llu}\n", (unsigned long long)st.grm_skipped);
            return a.done(st, t_main);
        }
        if (cmd == "pca") {
            const SelectionArgs a(argc, argv, {{"pcs", 0}, {"tol", 0}, {"max-passes", 0}, {"seed", 0}, {"block-rows", 0}}, {});
            const std::string out = a.required("out", "--out <OUT_PREFIX>");
            PcaOptions p;
            if (auto v = a.get("pcs")) p.pcs = (uint32_t)unsigned_value(*v, "pcs", "P", 1, 32, "a number of components from 1 to 32");
            if (auto v = a.get("tol")) p.tol = double_value(*v, "tol", "X", 0.0, 1.0, "a number from 0 to 1");
            if (auto v = a.get("max-passes")) p.max_passes = (uint32_t)unsigned_value(*v, "max-passes", "I", 1, 1000000, "a number of passes from 1 to 1000000");
            if (auto v = a.get("seed")) p.seed = unsigned_value(*v, "seed", "S", 0, kNoLimit, "a whole number");
            if (auto b = a.get("block-rows")) p.block_rows = block_rows_value(*b);
            const Pfile pfile = Pfile::from_prefix(a.positional[0]);
            const OutputStats st = pfile.output_pca(a.get("include-sam"), a.get("include-var"), out, p, output_options(a));
            if (a.has("stats"))
                std::fprintf(stderr, "{\"variants_skipped\": %llu, \"passes\": %llu, \"residual\": %.6g, \"converged\": %s}\n", (unsigned long long)st.pca_skipped,
                             (unsigned long long)st.pca_passes, st.pca_residual, st.pca_converged ? "true" : "false");
            return a.done(st, t_main);
        }
        if (cmd == "bgzf") {
            // not in the reference: the BGZF writer of `filter ... -o x.vcf.gz` applied to a file (what `bgzip -c IN > OUT` does)
            Args a = parse(argc, argv, 2, {{"level", 0}, {"threads", 0}, {"chunk-mib", 0}}, {});
            if (a.positional.size() != 2) usage_error("bgzf <IN_FILE> <OUT_FILE> [--level <1-9>] [--threads <T>] [--chunk-mib <M>]");
            const int level = a.get("level") ? std::atoi(a.get("level")->c_str()) : 6;
            if (level < 1 || level > 9) usage_error("--level takes 1 .. 9");
            const unsigned threads = (unsigned)std::max(1, std::atoi(a.get("threads").value_or("8").c_str()));
            const size_t chunk = (size_t)std::max(1, std::atoi(a.get("chunk-mib").value_or("64").c_str())) << 20;
            bgzf_file(a.positional[0], a.positional[1], level, threads, chunk);
            return 0;
        }
        if (cmd == "synth") {
            // not in the reference: writes a synthetic PREFIX.{pgen,pvar,psam} triple of the SURVEY §8d shapes
            // (records from the device generator pgenhip_synth_records; KEEP column = the 1-in-M keep mask)
            Args a = parse(argc, argv, 2, {{"variants", 0}, {"samples", 0}, {"keep-modulus", 0}, {"seed", 0}}, {});
            if (a.positional.size() != 1 || !a.has("variants") || !a.has("samples"))
                usage_error("synth <PFILE_PREFIX> --variants <V> --samples <N> [--keep-modulus <M>] [--seed <S>]");
            synth_pfile(a.positional[0], (uint32_t)std::strtoul(a.get("variants")->c_str(), nullptr, 10),
                        (uint32_t)std::strtoul(a.get("samples")->c_str(), nullptr, 10),
                        (uint32_t)std::strtoul(a.get("keep-modulus").value_or("100").c_str(), nullptr, 10),
                        std::strtoull(a.get("seed").value_or("1346848078").c_str(), nullptr, 10));  // 0x5047454E "PGEN": seed_data of SURVEY.md 8(d) (round 2 had a typo here)
            return 0;
        }
        usage_error("unrecognized subcommand '" + cmd + "'");
    } catch (const PfileError &e) {
        std::fprintf(stderr, "pgen-hip: %s\n", e.what());
        return 101;
    } catch (const CsvError &e) {
        std::fprintf(stderr, "pgen-hip: %s\n", e.what());
        return 101;
    } catch (const ExprError &e) {
        std::fprintf(stderr, "pgen-hip: %s\n", e.what());
        return 101;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pgen-hip: %s\n", e.what());
        return 101;
    }
    return 0;
}
