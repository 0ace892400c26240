// stats_check.cpp — a stand-alone program around pgen_rs_amd/host/stats.cpp and linalg.cpp, the arithmetic of the host commands
// (tests/test_host_stats.py compiles the three with g++ -fsanitize=address,undefined and runs the result; it is never loaded into
// Python, and it links neither HIP nor libpgen_hip.so).  It reads cases from the file named by argv[1] and prints one line per
// case, doubles as hexadecimal floats (%a) so that the reader gets every bit:
//   table c0 c1 c2 c3                    -> table <1 if the variant counts> g[0..4) n[0..4) <mean dosage>
//   king t[0..16)                        -> king n hethet ibs0 het1 het2 <kinship>
//   tp t df                              -> tp <two-sided P>
//   assoc n ncov P V, x (n x ncov), y (n x P), then per variant 4 counts and (1 + ncov + P) x 4 per-code sums
//                                        -> assoc <collinear column, or -1 and then:> df rr[0..P), per variant and phenotype
//                                           <has_freq> <a1_freq> <na> <beta> <se> <t> <p>
//   start seed K L                       -> start <the K x L Gaussian start, row-major>
//   pca K L P seed tol max_passes, M (K x K)
//                                        -> pca <passes> <1 if converged> lambda[0..P) <the scaled vectors, K x P row-major>
//      the iteration of `pgen-hip pca` with the product Y = M Q done densely here
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pgen_rs_amd/host/linalg.h"
#include "../pgen_rs_amd/host/stats.h"

using namespace pgenhost;

static bool read_doubles(std::FILE *f, std::vector<double> &v)
{
    for (double &x : v)
        if (std::fscanf(f, "%lf", &x) != 1) return false;
    return true;
}

static bool read_u32s(std::FILE *f, uint32_t *v, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (std::fscanf(f, "%" SCNu32, &v[i]) != 1) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (!std::strcmp(kind, "table")) {
            uint32_t c[4];
            if (!read_u32s(f, c, 4)) return 3;
            double g[4], n[4];
            const bool used = stats::standardized_table(c, g, n);
            std::printf("table %d", (int)used);
            for (double x : g) std::printf(" %a", x);
            for (double x : n) std::printf(" %a", x);
            std::printf(" %a\n", stats::mean_dosage(c));
        } else if (!std::strcmp(kind, "king")) {
            uint32_t t[16];
            if (!read_u32s(f, t, 16)) return 3;
            const stats::King k = stats::king(t);
            std::printf("king %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %a\n", k.n, k.hethet, k.ibs0, k.het1, k.het2, k.kinship);
        } else if (!std::strcmp(kind, "tp")) {
            double t, df;
            if (std::fscanf(f, "%lf %lf", &t, &df) != 2) return 3;
            std::printf("tp %a\n", stats::student_t_two_sided_p(t, df));
        } else if (!std::strcmp(kind, "assoc")) {
            size_t n, ncov, P, V;
            if (std::fscanf(f, "%zu %zu %zu %zu", &n, &ncov, &P, &V) != 4) return 3;
            std::vector<double> x(n * ncov), y(n * P);
            if (!read_doubles(f, x) || !read_doubles(f, y)) return 3;
            stats::AssocDesign d;
            const size_t collinear = stats::assoc_design(x, y, n, ncov, P, d);
            std::vector<double> S((1 + ncov + P) * 4);
            if (collinear != stats::kNoColumn) {
                std::printf("assoc %zu\n", collinear);
            } else {
                std::printf("assoc -1 %a", d.df);
                for (double r : d.rr) std::printf(" %a", r);
            }
            for (size_t j = 0; j < V; j++) {
                uint32_t c[4];
                if (!read_u32s(f, c, 4) || !read_doubles(f, S)) return 3;
                if (collinear != stats::kNoColumn) continue;
                for (size_t p = 0; p < P; p++) {
                    const stats::AssocTest r = stats::assoc_test(d, c, S.data(), p);
                    std::printf(" %d %a %d %a %a %a %a", (int)r.has_freq, r.a1_freq, (int)r.na, r.beta, r.se, r.t, r.p);
                }
            }
            if (collinear == stats::kNoColumn) std::printf("\n");
        } else if (!std::strcmp(kind, "start")) {
            uint64_t seed;
            size_t K, L;
            if (std::fscanf(f, "%" SCNu64 " %zu %zu", &seed, &K, &L) != 3) return 3;
            std::vector<double> q;
            linalg::gaussian_start(seed, K, L, q);
            if (q.size() != K * L) return 4;
            std::printf("start");
            for (double v : q) std::printf(" %a", v);
            std::printf("\n");
        } else if (!std::strcmp(kind, "pca")) {
            size_t K, L, P, max_passes;
            uint64_t seed;
            double tol;
            if (std::fscanf(f, "%zu %zu %zu %" SCNu64 " %lf %zu", &K, &L, &P, &seed, &tol, &max_passes) != 6) return 3;
            std::vector<double> M(K * K), Q, Y(K * L), U, lambda;
            if (!read_doubles(f, M)) return 3;
            linalg::gaussian_start(seed, K, L, Q);
            linalg::qr_thin(Q, K, L);
            size_t passes = 0;
            bool converged = false;
            for (;;) {
                for (size_t k = 0; k < K; k++)
                    for (size_t c = 0; c < L; c++) {
                        double dot = 0.0;
                        for (size_t i = 0; i < K; i++) dot += M[k * K + i] * Q[i * L + c];
                        Y[k * L + c] = dot;
                    }
                passes++;
                const double worst = linalg::rayleigh_ritz(Q, Y, K, L, P, lambda, U);
                converged = worst <= tol * lambda[0];
                if (converged || passes >= max_passes) break;
                Q = Y;
                linalg::qr_thin(Q, K, L);
            }
            linalg::unit_columns_largest_positive(U, K, L, P);
            std::printf("pca %zu %d", passes, (int)converged);
            for (size_t i = 0; i < P; i++) std::printf(" %a", lambda[i]);
            for (size_t k = 0; k < K; k++)
                for (size_t i = 0; i < P; i++) std::printf(" %a", U[k * L + i]);
            std::printf("\n");
        } else {
            return 3;
        }
    }
    std::fclose(f);
    return 0;
}
