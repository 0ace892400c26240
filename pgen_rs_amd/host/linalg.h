// linalg.h — the dense linear algebra `pgen-hip pca` needs on the host, in plain C++ (no device, no dependency): Householder QR of a
// tall K x L matrix and a cyclic Jacobi eigen-solver of a symmetric L x L matrix.  Matrices are row-major std::vector<double>.
#pragma once
#include <cstddef>
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

}  // namespace pgenhost::linalg
