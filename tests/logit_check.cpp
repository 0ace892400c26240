// logit_check.cpp — a stand-alone program around the logistic arithmetic of pgen_rs_amd/host/stats.cpp (tests/test_variant_logistic.py
// compiles the two with g++ -fsanitize=address,undefined and runs the result; it is never loaded into Python, and it links neither HIP
// nor libpgen_hip.so).  It reads cases from the file named by argv[1] and prints one line per case, doubles as hexadecimal floats:
//   coding n, then n values (nan: missing)  -> coding <0 neither, 1 zero/one, 2 one/two>
//   null n ncov max_iter tol, x (n x ncov), y (n, 0 / 1)
//                                           -> null <collinear column, or -1 and then:> <1 if converged> <evaluations> beta[0..m)
//                                              eta[0..n): the design times beta, the fitted linear predictor, which does not depend
//                                              on the basis of the covariates' span
//   pz z                                    -> pz <two-sided normal P>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pgen_rs_amd/host/stats.h"

using namespace pgenhost;

static bool read_doubles(std::FILE *f, std::vector<double> &v)
{
    for (double &x : v)
        if (std::fscanf(f, "%lf", &x) != 1) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (!std::strcmp(kind, "coding")) {
            size_t n;
            if (std::fscanf(f, "%zu", &n) != 1) return 3;
            std::vector<double> v(n);
            if (!read_doubles(f, v)) return 3;
            std::printf("coding %d\n", (int)stats::binary_coding(v.data(), n, 1));
        } else if (!std::strcmp(kind, "null")) {
            size_t n, ncov;
            int max_iter;
            double tol;
            if (std::fscanf(f, "%zu %zu %d %lf", &n, &ncov, &max_iter, &tol) != 4) return 3;
            std::vector<double> x(n * ncov), y(n), design;
            if (!read_doubles(f, x) || !read_doubles(f, y)) return 3;
            const size_t bad = stats::logistic_design(x, n, ncov, design);
            if (bad != stats::kNoColumn) {
                std::printf("null %zu\n", bad);
                continue;
            }
            const size_t m = 1 + ncov;
            const stats::LogisticNull fit = stats::logistic_null(design, n, m, y.data(), max_iter, tol);
            std::printf("null -1 %d %d", (int)fit.converged, fit.evaluations);
            for (double b : fit.beta) std::printf(" %a", b);
            for (size_t k = 0; k < n; k++) {
                double eta = 0.0;
                for (size_t c = 0; c < m; c++) eta += design[k * m + c] * fit.beta[c];
                std::printf(" %a", eta);
            }
            std::printf("\n");
        } else if (!std::strcmp(kind, "pz")) {
            double z;
            if (std::fscanf(f, "%lf", &z) != 1) return 3;
            std::printf("pz %a\n", stats::wald_p(z));
        } else {
            return 4;
        }
    }
    std::fclose(f);
    return 0;
}
