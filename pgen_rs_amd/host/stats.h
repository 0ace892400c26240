// stats.h — the arithmetic of the commands in commands.cpp and assoc.cpp, in plain C++: numbers in, numbers out.  Nothing here touches a file, a
// device, a clock or a PfileError, so tests/stats_check.cpp runs all of it as a stand-alone program under AddressSanitizer and UBSan
// (tests/test_host_stats.py).  A condition a command words as an error comes back as a value.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pgenhost::stats {

// counts: a variant's genotype counts {hom ref, het, hom alt, missing}

// the mean ALT dosage over the called samples; 0 when nobody is called
double mean_dosage(const uint32_t counts[4]);

// The standardised genotype table of `grm` and `pca`: g[x] = (x - 2p) / sqrt(2p(1 - p)) and n[x] = 1 for the codes x = 0, 1, 2, both
// 0 for a missing call.  False, with both tables zero, when the variant adds nothing: no call, p == 0 or p == 1.
bool standardized_table(const uint32_t counts[4], double g[4], double n[4]);

// KING-robust kinship of a sample pair from its 4 x 4 table of code pairs (table[4 a + b]: variants where the first sample has code a
// and the second code b): 1/2 - ((het1 + het2 - 2 hethet) + 4 ibs0) / (4 min(het1, het2)), NaN when the smaller heterozygote count is 0
struct King {
    uint64_t n, hethet, ibs0, het1, het2;   // variants both have called; both het; opposite homozygotes; het in the first, in the second
    double kinship;
};
King king(const uint32_t table[16]);

// two-sided P of a Student t statistic with df degrees of freedom: I_{df / (df + t^2)}(df / 2, 1 / 2), the regularised incomplete
// beta function by a Lentz continued fraction (no library)
double student_t_two_sided_p(double t, double df);

// `assoc`'s design: the value columns the device sums per genotype code
struct AssocDesign {
    size_t n = 0, m = 0, P = 0;   // samples, intercept + covariates, phenotypes
    std::vector<double> values;   // n x (m + P), row-major: Q's m orthonormal columns, then the phenotypes residualised on them
    std::vector<double> rr;       // P: the residualised phenotypes' sums of squares
    double df = 0;                // n - m - 1
    size_t columns() const { return m + P; }
};
constexpr size_t kNoColumn = ~(size_t)0;

// Builds d from the covariates x (n x ncov, row-major) and the phenotypes y (n x P), n >= ncov + 3: the intercept and the covariates
// orthonormalised by modified Gram-Schmidt applied twice, the phenotypes with their parts along them taken out.  Returns kNoColumn,
// or the first column of [1, x] (0: the intercept, c: covariate c - 1) that is collinear with the columns before it; d is then
// unfinished.
size_t assoc_design(const std::vector<double> &x, const std::vector<double> &y, size_t n, size_t ncov, size_t P, AssocDesign &d);

// One line of `assoc`: the regression of phenotype p on a variant's mean-imputed dosage beside the design's m columns, from the
// variant's counts and its per-code sums S (columns() x 4: S[4 c + x] = the sum of value column c over the samples with code x)
struct AssocTest {
    bool has_freq;   // somebody is called: a1_freq exists
    double a1_freq;
    bool na;         // nobody called, a dosage (numerically) inside the span of the design, or no residual left: no estimate
    double beta, se, t, p;
};
AssocTest assoc_test(const AssocDesign &d, const uint32_t counts[4], const double *S, size_t p);

// ---- `assoc --logistic` ----
// How a case/control column is coded, from its n values v[0], v[stride], ... (NaN: missing, skipped): every value 1 or 2 with a 2
// present (control / case), else every value 0 or 1 (0 control), else neither
enum class BinaryCoding { kNone, kZeroOne, kOneTwo };
BinaryCoding binary_coding(const double *v, size_t n, size_t stride);
// 0 / 1 from a value of a column coded so
inline double binary_value(double v, BinaryCoding c) { return c == BinaryCoding::kOneTwo ? v - 1.0 : v; }

// The design the device iterates on: the n x m orthonormal columns of assoc_design scaled by sqrt(n), so that the first column is
// the constant 1 and coefficients are O(1); the genotype's coefficient and its standard error do not depend on the basis of the
// covariates' span.  Returns assoc_design's column report; x as there.
size_t logistic_design(const std::vector<double> &x, size_t n, size_t ncov, std::vector<double> &design);

// The null model: Newton's iteration on the design alone (n x m, row-major) from zero, the algorithm of the device's fit without the
// genotype: Cholesky of H = X^T diag(mu (1 - mu)) X, stop when max |delta| <= tol.  converged is false after max_iter evaluations
// or at a pivot that is <= 0 or not finite (a phenotype the covariates separate); beta then holds the last coefficients.
struct LogisticNull {
    bool converged;
    int evaluations;
    std::vector<double> beta;   // m
};
LogisticNull logistic_null(const std::vector<double> &design, size_t n, size_t m, const double *y, int max_iter, double tol);

// two-sided P of a Wald statistic: erfc(|z| / sqrt 2)
double wald_p(double z);

}  // namespace pgenhost::stats
