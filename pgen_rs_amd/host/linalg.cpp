// linalg.cpp — Householder QR, cyclic Jacobi and the steps of the subspace iteration for `pgen-hip pca` (linalg.h).  Pure C++;
// tests/linalg_check.cpp and tests/stats_check.cpp run it under AddressSanitizer and UBSan as stand-alone programs.
#include "linalg.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace pgenhost::linalg {

void qr_thin(std::vector<double> &a, size_t K, size_t L, std::vector<double> *r)
{
    // reflector j: v_j (rows j .. K-1, stored in vs) and beta_j = 2 / v^T v (0: the column was already zero below and on the diagonal)
    std::vector<double> vs(K * L, 0.0), beta(L, 0.0);
    for (size_t j = 0; j < L; j++) {
        double below2 = 0.0;
        for (size_t i = j + 1; i < K; i++) below2 += a[i * L + j] * a[i * L + j];
        if (below2 == 0.0) continue;   // nothing to annihilate: H_j = I (as LAPACK's dlarfg), so a 1 x 1 input comes back untouched
        const double norm = std::sqrt(a[j * L + j] * a[j * L + j] + below2);
        const double alpha = a[j * L + j] >= 0.0 ? -norm : norm;   // the reflected column is alpha e_j: no cancellation in v_j
        for (size_t i = j; i < K; i++) vs[i * L + j] = a[i * L + j];
        vs[j * L + j] -= alpha;
        double vv = 0.0;
        for (size_t i = j; i < K; i++) vv += vs[i * L + j] * vs[i * L + j];
        if (vv == 0.0) continue;
        beta[j] = 2.0 / vv;
        a[j * L + j] = alpha;   // the reflected column, exactly
        for (size_t i = j + 1; i < K; i++) a[i * L + j] = 0.0;
        for (size_t c = j + 1; c < L; c++) {
            double dot = 0.0;
            for (size_t i = j; i < K; i++) dot += vs[i * L + j] * a[i * L + c];
            dot *= beta[j];
            for (size_t i = j; i < K; i++) a[i * L + c] -= dot * vs[i * L + j];
        }
    }
    if (r) {
        r->assign(L * L, 0.0);
        for (size_t i = 0; i < L; i++)
            for (size_t c = i; c < L; c++) (*r)[i * L + c] = a[i * L + c];
    }
    // Q = H_0 H_1 ... H_{L-1} applied to the first L columns of the identity
    std::fill(a.begin(), a.end(), 0.0);
    for (size_t i = 0; i < L; i++) a[i * L + i] = 1.0;
    for (size_t j = L; j-- > 0;) {
        if (beta[j] == 0.0) continue;
        for (size_t c = 0; c < L; c++) {
            double dot = 0.0;
            for (size_t i = j; i < K; i++) dot += vs[i * L + j] * a[i * L + c];
            dot *= beta[j];
            for (size_t i = j; i < K; i++) a[i * L + c] -= dot * vs[i * L + j];
        }
    }
}

void jacobi_eigh(const std::vector<double> &t, size_t L, std::vector<double> &lambda, std::vector<double> &w)
{
    std::vector<double> a(L * L);
    for (size_t i = 0; i < L; i++)
        for (size_t j = 0; j < L; j++) a[i * L + j] = i <= j ? t[i * L + j] : t[j * L + i];
    std::vector<double> v(L * L, 0.0);
    for (size_t i = 0; i < L; i++) v[i * L + i] = 1.0;
    double total = 0.0;
    for (double x : a) total += x * x;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (size_t i = 0; i < L; i++)
            for (size_t j = i + 1; j < L; j++) off += 2.0 * a[i * L + j] * a[i * L + j];
        if (!(std::sqrt(off) > 0x1p-52 * std::sqrt(total))) break;
        for (size_t p = 0; p + 1 < L; p++)
            for (size_t q = p + 1; q < L; q++) {
                const double apq = a[p * L + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * L + q] - a[p * L + p]) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
                for (size_t k = 0; k < L; k++) {   // columns p and q
                    const double akp = a[k * L + p], akq = a[k * L + q];
                    a[k * L + p] = c * akp - s * akq;
                    a[k * L + q] = s * akp + c * akq;
                }
                for (size_t k = 0; k < L; k++) {   // rows p and q
                    const double apk = a[p * L + k], aqk = a[q * L + k];
                    a[p * L + k] = c * apk - s * aqk;
                    a[q * L + k] = s * apk + c * aqk;
                }
                for (size_t k = 0; k < L; k++) {
                    const double vkp = v[k * L + p], vkq = v[k * L + q];
                    v[k * L + p] = c * vkp - s * vkq;
                    v[k * L + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<size_t> order(L);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return a[x * L + x] > a[y * L + y]; });
    lambda.assign(L, 0.0);
    w.assign(L * L, 0.0);
    for (size_t i = 0; i < L; i++) {
        const size_t src = order[i];
        lambda[i] = a[src * L + src];
        size_t big = 0;
        for (size_t k = 1; k < L; k++)
            if (std::fabs(v[k * L + src]) > std::fabs(v[big * L + src])) big = k;
        const double sign = v[big * L + src] < 0.0 ? -1.0 : 1.0;
        for (size_t k = 0; k < L; k++) w[k * L + i] = sign * v[k * L + src];
    }
}

namespace {

// splitmix64: the next state's output
uint64_t splitmix64(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

void gaussian_start(uint64_t seed, size_t K, size_t L, std::vector<double> &q)
{
    q.resize(K * L);
    uint64_t state = seed;
    for (double &x : q) {
        const double u1 = (double)((splitmix64(state) >> 11) + 1) * 0x1p-53, u2 = (double)(splitmix64(state) >> 11) * 0x1p-53;
        x = std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
    }
}

double rayleigh_ritz(const std::vector<double> &q, const std::vector<double> &y, size_t K, size_t L, size_t P, std::vector<double> &lambda,
                     std::vector<double> &u)
{
    std::vector<double> t(L * L), w;
    for (size_t a = 0; a < L; a++)
        for (size_t b = 0; b < L; b++) {
            double dot = 0.0;
            for (size_t k = 0; k < K; k++) dot += q[k * L + a] * y[k * L + b];
            t[a * L + b] = dot;
        }
    for (size_t a = 0; a < L; a++)
        for (size_t b = a + 1; b < L; b++) t[a * L + b] = t[b * L + a] = 0.5 * (t[a * L + b] + t[b * L + a]);
    jacobi_eigh(t, L, lambda, w);
    u.resize(K * L);
    double worst = 0.0;
    for (size_t i = 0; i < L; i++) {
        double rr = 0.0;
        for (size_t k = 0; k < K; k++) {
            double uk = 0.0, yw = 0.0;
            for (size_t a = 0; a < L; a++) {
                uk += q[k * L + a] * w[a * L + i];
                yw += y[k * L + a] * w[a * L + i];
            }
            u[k * L + i] = uk;
            const double r = yw - lambda[i] * uk;
            rr += r * r;
        }
        if (i < P) worst = std::max(worst, std::sqrt(rr));
    }
    return worst;
}

void unit_columns_largest_positive(std::vector<double> &u, size_t K, size_t L, size_t P)
{
    for (size_t i = 0; i < P; i++) {
        double ss = 0.0, big = 0.0;
        for (size_t k = 0; k < K; k++) {
            ss += u[k * L + i] * u[k * L + i];
            if (std::fabs(u[k * L + i]) > std::fabs(big)) big = u[k * L + i];
        }
        const double scale = (big < 0.0 ? -1.0 : 1.0) / (ss > 0.0 ? std::sqrt(ss) : 1.0);
        for (size_t k = 0; k < K; k++) u[k * L + i] *= scale;
    }
}

}  // namespace pgenhost::linalg
