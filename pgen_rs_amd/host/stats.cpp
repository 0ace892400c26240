// stats.cpp — the commands' arithmetic (stats.h).  Pure C++; tests/stats_check.cpp runs it under AddressSanitizer and UBSan as a
// stand-alone program.
#include "stats.h"

#include <algorithm>
#include <cmath>

namespace pgenhost::stats {

double mean_dosage(const uint32_t counts[4])
{
    const uint64_t c1 = counts[1], c2 = counts[2], called = counts[0] + c1 + c2;
    return called ? (double)(c1 + 2 * c2) / (double)called : 0.0;
}

bool standardized_table(const uint32_t counts[4], double g[4], double n[4])
{
    const uint64_t c0 = counts[0], c1 = counts[1], c2 = counts[2];
    const uint64_t called = c0 + c1 + c2, alt = c1 + 2 * c2;
    if (called == 0 || alt == 0 || alt == 2 * called) {   // no call, p == 0 or p == 1: the variant adds nothing
        for (int x = 0; x < 4; x++) g[x] = n[x] = 0.0;
        return false;
    }
    const double p = (double)alt / (2.0 * (double)called);
    const double s = 1.0 / std::sqrt(2.0 * p * (1.0 - p));
    g[0] = (0.0 - 2.0 * p) * s;
    g[1] = (1.0 - 2.0 * p) * s;
    g[2] = (2.0 - 2.0 * p) * s;
    g[3] = 0.0;
    n[0] = n[1] = n[2] = 1.0;
    n[3] = 0.0;
    return true;
}

King king(const uint32_t t[16])
{
    King k{0, t[5], (uint64_t)t[2] + t[8], (uint64_t)t[4] + t[5] + t[6], (uint64_t)t[1] + t[5] + t[9], 0.0};
    for (int x = 0; x < 3; x++)
        for (int y = 0; y < 3; y++) k.n += t[4 * x + y];
    const uint64_t hmin = std::min(k.het1, k.het2);
    k.kinship = hmin == 0 ? std::nan("") : 0.5 - ((double)(k.het1 + k.het2 - 2 * k.hethet) + 4.0 * (double)k.ibs0) / (4.0 * (double)hmin);
    return k;
}

namespace {

// ln Gamma(a + 1/2) - ln Gamma(a): the difference of two lgamma values loses 1e-16 of their size (6e6 at a = 5e5), so from a = 64 on
// the asymptotic series of the ratio itself
double lgamma_half_step(double a)
{
    if (a < 64.0) return std::lgamma(a + 0.5) - std::lgamma(a);
    const double i = 1.0 / a, i2 = i * i;
    return 0.5 * std::log(a) + i * (-1.0 / 8.0 + i2 * (1.0 / 192.0 + i2 * (-1.0 / 640.0 + i2 * (17.0 / 14336.0))));
}

// the continued fraction of the incomplete beta function by the modified Lentz method
double beta_cf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 100000; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

}  // namespace

double student_t_two_sided_p(double t, double df)
{
    if (std::isnan(t) || std::isnan(df) || df <= 0.0) return std::nan("");
    if (std::isinf(t)) return 0.0;
    if (t == 0.0) return 1.0;
    const double a = 0.5 * df, b = 0.5, t2 = t * t;
    const double x = df / (df + t2), y = t2 / (df + t2);                 // y = 1 - x without the cancellation
    // ln of x^a y^b / B(a, b): a ln x = -a log1p(t^2 / df); B(a, 1/2) = Gamma(a) sqrt(pi) / Gamma(a + 1/2)
    const double front = std::exp(lgamma_half_step(a) - 0.5 * std::log(M_PI) - a * std::log1p(t2 / df) + b * std::log(y));
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
    return 1.0 - front * beta_cf(b, a, y) / b;
}

size_t assoc_design(const std::vector<double> &x, const std::vector<double> &y, size_t n, size_t ncov, size_t P, AssocDesign &d)
{
    const size_t m = 1 + ncov, C = m + P;
    d.n = n;
    d.m = m;
    d.P = P;
    d.df = (double)(n - m - 1);
    d.values.assign(n * C, 0.0);
    d.rr.assign(P, 0.0);
    auto at = [&](size_t k, size_t c) -> double & { return d.values[k * C + c]; };
    auto project_out = [&](size_t c, size_t upto) {   // column c minus its parts along columns [0, upto), twice
        for (int pass = 0; pass < 2; pass++)
            for (size_t q = 0; q < upto; q++) {
                double dot = 0.0;
                for (size_t k = 0; k < n; k++) dot += at(k, q) * at(k, c);
                for (size_t k = 0; k < n; k++) at(k, c) -= dot * at(k, q);
            }
    };
    auto norm = [&](size_t c) {
        double ss = 0.0;
        for (size_t k = 0; k < n; k++) ss += at(k, c) * at(k, c);
        return std::sqrt(ss);
    };
    for (size_t c = 0; c < m; c++) {
        for (size_t k = 0; k < n; k++) at(k, c) = c == 0 ? 1.0 : x[k * ncov + (c - 1)];
        const double before = norm(c);
        project_out(c, c);
        const double after = norm(c);
        if (!(after > 1e-10 * before)) return c;
        for (size_t k = 0; k < n; k++) at(k, c) /= after;
    }
    for (size_t p = 0; p < P; p++) {
        for (size_t k = 0; k < n; k++) at(k, m + p) = y[k * P + p];
        project_out(m + p, m);
        for (size_t k = 0; k < n; k++) d.rr[p] += at(k, m + p) * at(k, m + p);
    }
    return kNoColumn;
}

AssocTest assoc_test(const AssocDesign &d, const uint32_t counts[4], const double *S, size_t p)
{
    const double c1 = counts[1], c2 = counts[2], c3 = counts[3];
    const bool called = (uint64_t)counts[0] + counts[1] + counts[2] != 0;
    const double mu = mean_dosage(counts);
    // t_c: the dot product of value column c with the dosages, a missing call at the mean
    auto tv = [&](size_t c) { return S[4 * c + 1] + 2.0 * S[4 * c + 2] + mu * S[4 * c + 3]; };
    const double gg = c1 + 4.0 * c2 + mu * mu * c3;
    double denom = gg;   // the dosages' sum of squares less their part along Q
    for (size_t q = 0; q < d.m; q++) denom -= tv(q) * tv(q);
    const double b = tv(d.m + p);
    const double rss = d.rr[p] - b * b / denom;
    AssocTest r{called, 0.5 * mu, false, 0.0, 0.0, 0.0, 0.0};
    r.na = !called || !(denom > 1e-12 * gg) || !(rss > 0);
    if (r.na) return r;
    r.beta = b / denom;
    r.se = std::sqrt(rss / d.df / denom);
    r.t = r.beta / r.se;
    r.p = student_t_two_sided_p(r.t, d.df);
    return r;
}

BinaryCoding binary_coding(const double *v, size_t n, size_t stride)
{
    bool zero_one = true, one_two = true, two = false;
    for (size_t k = 0; k < n; k++) {
        const double x = v[k * stride];
        if (std::isnan(x)) continue;
        zero_one = zero_one && (x == 0.0 || x == 1.0);
        one_two = one_two && (x == 1.0 || x == 2.0);
        two = two || x == 2.0;
    }
    if (one_two && two) return BinaryCoding::kOneTwo;
    return zero_one ? BinaryCoding::kZeroOne : BinaryCoding::kNone;
}

size_t logistic_design(const std::vector<double> &x, size_t n, size_t ncov, std::vector<double> &design)
{
    AssocDesign d;
    const size_t bad = assoc_design(x, std::vector<double>(), n, ncov, 0, d);
    if (bad != kNoColumn) return bad;
    const double scale = std::sqrt((double)n);
    design = std::move(d.values);
    for (double &v : design) v *= scale;
    return kNoColumn;
}

LogisticNull logistic_null(const std::vector<double> &design, size_t n, size_t m, const double *y, int max_iter, double tol)
{
    LogisticNull r{false, 0, std::vector<double>(m, 0.0)};
    std::vector<double> H(m * m), g(m);
    for (int it = 1; it <= max_iter; it++) {
        r.evaluations = it;
        std::fill(H.begin(), H.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        for (size_t k = 0; k < n; k++) {
            const double *xr = design.data() + k * m;
            double eta = 0.0;
            for (size_t c = 0; c < m; c++) eta += xr[c] * r.beta[c];
            const double mu = 1.0 / (1.0 + std::exp(-eta)), w = mu * (1.0 - mu), res = y[k] - mu;
            for (size_t a = 0; a < m; a++) {
                g[a] += xr[a] * res;
                const double wx = w * xr[a];
                for (size_t b = 0; b <= a; b++) H[a * m + b] += wx * xr[b];
            }
        }
        for (size_t j = 0; j < m; j++) {   // Cholesky in place, lower
            double piv = H[j * m + j];
            for (size_t k = 0; k < j; k++) piv -= H[j * m + k] * H[j * m + k];
            if (!(piv > 0.0) || std::isinf(piv)) return r;
            const double l = std::sqrt(piv);
            H[j * m + j] = l;
            for (size_t i = j + 1; i < m; i++) {
                double v = H[i * m + j];
                for (size_t k = 0; k < j; k++) v -= H[i * m + k] * H[j * m + k];
                H[i * m + j] = v / l;
            }
        }
        for (size_t i = 0; i < m; i++) {
            double v = g[i];
            for (size_t k = 0; k < i; k++) v -= H[i * m + k] * g[k];
            g[i] = v / H[i * m + i];
        }
        for (size_t i = m; i-- > 0;) {
            double v = g[i];
            for (size_t k = i + 1; k < m; k++) v -= H[k * m + i] * g[k];
            g[i] = v / H[i * m + i];
        }
        bool converged = true;
        for (size_t i = 0; i < m; i++) converged = converged && std::fabs(g[i]) <= tol;
        if (converged) {
            r.converged = true;
            return r;
        }
        for (size_t i = 0; i < m; i++) r.beta[i] += g[i];
    }
    return r;
}

double wald_p(double z) { return std::erfc(std::fabs(z) / std::sqrt(2.0)); }

}  // namespace pgenhost::stats
