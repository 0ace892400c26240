// linalg.h — the dense linear algebra `pgen-hip pca` needs on the host, in plain C++ (no device, no dependency): Householder QR of a
// tall K x L matrix, a cyclic Jacobi eigen-solver of a symmetric L x L matrix, and the steps of the subspace iteration around the
// product Y = M Q: its seeded start, the Rayleigh-Ritz step and the scaling of what is written.  Matrices are row-major
// std::vector<double>.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pgenhost::linalg {

// a (K x L, K >= L, row-major) = Q R by Householder reflections: a is overwritten with the thin Q (K x L, orthonormal columns whatever
// the rank of the input: a dependent column gets a direction orthogonal to the others) and r, when not null, with R (L x L upper
// triangle, row-major; its diagonal may have either sign)
void qr_thin(std::vector<double> &a, size_t K, size_t L, std::vector<double> *r = nullptr);

// Eigen-decomposition of the symmetric L x L matrix t (row-major; only its upper triangle with the diagonal is read) by cyclic Jacobi
// rotations: t = W diag(lambda) W^T, lambda in descending order, eigenvector i in COLUMN i of w (L x L, row-major), each with its
// largest-magnitude entry made positive.  Sweeps stop when the off-diagonal norm is below 2^-52 times the matrix norm, or after 60.
void jacobi_eigh(const std::vector<double> &t, size_t L, std::vector<double> &lambda, std::vector<double> &w);

// q = the K x L standard normal matrix of `seed`, row-major: splitmix64 from the state `seed`, two outputs per entry,
// u1 = ((o1 >> 11) + 1) 2^-53 in (0, 1], u2 = (o2 >> 11) 2^-53 in [0, 1), and the Box-Muller cosine sqrt(-2 ln u1) cos(2 pi u2)
void gaussian_start(uint64_t seed, size_t K, size_t L, std::vector<double> &q);

// The Rayleigh-Ritz step of Q (K x L, orthonormal columns) with Y = M Q: T = Q^T Y symmetrised = W diag(lambda) W^T (jacobi_eigh),
// u = Q W (K x L).  Returns the largest residual norm |Y w_i - lambda_i u_i| = |M u_i - lambda_i u_i| of the first P pairs.
double rayleigh_ritz(const std::vector<double> &q, const std::vector<double> &y, size_t K, size_t L, size_t P, std::vector<double> &lambda,
                     std::vector<double> &u);

// the first P columns of u (K x L) scaled to unit norm with the largest-magnitude entry positive (a zero column stays)
void unit_columns_largest_positive(std::vector<double> &u, size_t K, size_t L, size_t P);

}  // namespace pgenhost::linalg
