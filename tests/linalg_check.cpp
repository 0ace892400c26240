// linalg_check.cpp — a stand-alone program around pgen_rs_amd/host/linalg.cpp (tests/test_gram_apply.py compiles both with
// g++ -fsanitize=address,undefined and runs the result; it is never loaded into Python).  It reads cases from the file named by
// argv[1] ("qr K L" or "eig L", then the matrix row-major, any strtod format) and prints one line per case:
//   qr K L <|Q^T Q - I|_F> <|Q R - A|_F / |A|_F> <1 if R is upper triangular>
//   eig L <|W^T W - I|_F> <|W diag(lambda) W^T - T|_F / |T|_F> <1 if lambda descends and every eigenvector's largest entry is positive>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pgen_rs_amd/host/linalg.h"

using namespace pgenhost::linalg;

static double rel(double err, double norm) { return norm > 0.0 ? err / norm : err; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (!std::strcmp(kind, "qr")) {
            size_t K, L;
            if (std::fscanf(f, "%zu %zu", &K, &L) != 2) return 3;
            std::vector<double> a(K * L), r;
            for (double &x : a)
                if (std::fscanf(f, "%lf", &x) != 1) return 3;
            std::vector<double> q = a;
            qr_thin(q, K, L, &r);
            double orth = 0.0, recon = 0.0, norm = 0.0;
            for (size_t i = 0; i < L; i++)
                for (size_t j = 0; j < L; j++) {
                    double dot = 0.0;
                    for (size_t k = 0; k < K; k++) dot += q[k * L + i] * q[k * L + j];
                    dot -= i == j ? 1.0 : 0.0;
                    orth += dot * dot;
                }
            for (size_t k = 0; k < K; k++)
                for (size_t j = 0; j < L; j++) {
                    double qr = 0.0;
                    for (size_t i = 0; i < L; i++) qr += q[k * L + i] * r[i * L + j];
                    recon += (qr - a[k * L + j]) * (qr - a[k * L + j]);
                    norm += a[k * L + j] * a[k * L + j];
                }
            int upper = 1;
            for (size_t i = 0; i < L; i++)
                for (size_t j = 0; j < i; j++) upper &= r[i * L + j] == 0.0;
            std::printf("qr %zu %zu %.17g %.17g %d\n", K, L, std::sqrt(orth), rel(std::sqrt(recon), std::sqrt(norm)), upper);
        } else if (!std::strcmp(kind, "eig")) {
            size_t L;
            if (std::fscanf(f, "%zu", &L) != 1) return 3;
            std::vector<double> t(L * L), lambda, w;
            for (double &x : t)
                if (std::fscanf(f, "%lf", &x) != 1) return 3;
            jacobi_eigh(t, L, lambda, w);
            double orth = 0.0, recon = 0.0, norm = 0.0;
            for (size_t i = 0; i < L; i++)
                for (size_t j = 0; j < L; j++) {
                    double dot = 0.0, back = 0.0;
                    for (size_t k = 0; k < L; k++) {
                        dot += w[k * L + i] * w[k * L + j];
                        back += w[i * L + k] * lambda[k] * w[j * L + k];
                    }
                    dot -= i == j ? 1.0 : 0.0;
                    orth += dot * dot;
                    recon += (back - t[i * L + j]) * (back - t[i * L + j]);
                    norm += t[i * L + j] * t[i * L + j];
                }
            int ordered = 1;
            for (size_t i = 0; i < L; i++) {
                if (i + 1 < L) ordered &= lambda[i] >= lambda[i + 1];
                size_t big = 0;
                for (size_t k = 1; k < L; k++)
                    if (std::fabs(w[k * L + i]) > std::fabs(w[big * L + i])) big = k;
                ordered &= w[big * L + i] > 0.0;
            }
            std::printf("eig %zu %.17g %.17g %d\n", L, std::sqrt(orth), rel(std::sqrt(recon), std::sqrt(norm)), ordered);
        } else {
            return 3;
        }
    }
    std::fclose(f);
    return 0;
}
