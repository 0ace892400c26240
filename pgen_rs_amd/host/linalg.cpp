// linalg.cpp — Householder QR and cyclic Jacobi for `pgen-hip pca` (linalg.h).  Pure C++; tests/linalg_check.cpp runs it under
// AddressSanitizer and UBSan as a stand-alone program.
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

}  // namespace pgenhost::linalg
