// gt_logit.hip — per-variant logistic regression for gfx950 (MI355X): for every selected row j a Newton iteration on
// X = [design, g], g_k = t_j[code of kept sample k in row j] (src/pfile.rs:172-183: sample s in byte s/4, bits 2*(s%4)), over the
// kept samples whose table entry is not NaN.  The algorithm is the one include/pgen_hip.h fixes (pgenhip_variant_logistic): start at
// (start, 0); per evaluation mu = 1 / (1 + e^-eta), grad = X^T (y - mu), H = X^T diag(mu (1 - mu)) X; Cholesky of H, delta = H^-1 grad;
// stop when max |delta_i| <= tol, else beta += delta; no step halving.  Every product and addition is FP64.  The order of the
// additions is not fixed (samples are dealt to lanes, lanes meet in a wave reduction), so two shapes may differ in the last bits.
//
// Unlike every other kernel here this one is compute-bound in FP64: a row costs, per evaluation and included sample, p FMAs for eta,
// an exp and a division, and p (p + 1) / 2 + p FMAs for the sums (p = n_cov + 1 <= 16), and it needs several evaluations whose
// weights depend on the row's own coefficients, so nothing is shared between rows but the design values.
//
// GENERAL: a block per row, the rest by grid stride; threads over the row's samples; one pass over the samples per row a of H, which
// sums H[a][0 .. a] and grad[a] (17 accumulators, each reduced on its own over the block); the solve in thread 0.  Any shape.
//
// FAST: every lane holds the lower half of H and the gradient in registers (p (p + 1) / 2 + p FP64 accumulators, all indices
// compile-time: the kernel is compiled for p rounded up to 4, 8, 12 or 16, plan::logit::bucket) and makes ONE pass over its samples
// per evaluation.  Up to 8 columns a wave owns a row.  Above that the accumulators do not fit 256 VGPRs (152 FP64 values at 16; at 12
// the compiler fits 90 only through AGPR copies at one wave per SIMD, and a VALU FMA cannot take an AGPR operand), so two waves share
// a row, each with half of H's entries (plan::logit::row_part) and all samples.  The block's four waves carry a group of 4 (or 2)
// rows through the evaluations together: they read the same design values at the same time, which the CU's L1 serves once, a
// converged row's waves idle, and the group ends when all its rows have ended.  The solve is one wave per row, a lane per row of H,
// in registers (logit_advance_wave); GENERAL keeps the one-lane solve on H in LDS, so the two shapes check each other's solve.  The
// loop over evaluations is bounded by max_iter <= 64 and every barrier is reached by all threads.  Record bytes are re-read per
// evaluation: 2 bits per sample next to 8 * n_cov bytes of design.
#include "gt_common.hip.h"
#include "kernels.h"
#include "launch_plan.h"

namespace pgenhip {

namespace {

using namespace plan::logit;   // kThreads, kWaves, kMaxP, kSums, bucket, waves_per_row, row_part, ... and the launch plan

constexpr uint32_t kHalf = kMaxP * (kMaxP + 1u) / 2u;   // the gradient's place behind the packed lower half of H
constexpr uint32_t kNoRow = 1u;                         // state of a slot without a row: ended, nothing to write

__device__ __forceinline__ uint32_t tri(uint32_t a, uint32_t b) { return a * (a + 1u) / 2u + b; }   // H[a][b], b <= a

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// mu = 1 / (1 + e^-eta); e^-eta = inf gives 0, not NaN
__device__ __forceinline__ double logistic(double eta) { return 1.0 / (1.0 + exp(-eta)); }

// One lane: the step after an evaluation.  sums holds the packed lower half of H and, at kHalf, the gradient; both are overwritten
// (H by its Cholesky factor, the gradient by delta).  Returns 0 when beta has moved on, else the row's final status word.
__device__ uint32_t logit_advance(double *sums, double *beta, uint32_t p, uint32_t it, uint32_t max_iter, double tol, double &se)
{
    double *H = sums, *d = sums + kHalf;
    se = __longlong_as_double(0x7FF8000000000000ll);
    for (uint32_t j = 0; j < p; j++) {
        double piv = H[tri(j, j)];
        for (uint32_t k = 0; k < j; k++) piv -= H[tri(j, k)] * H[tri(j, k)];
        if (!(piv > 0.0) || isinf(piv)) return PGENHIP_LOGIT_SINGULAR | it;
        const double l = sqrt(piv);
        H[tri(j, j)] = l;
        for (uint32_t i = j + 1u; i < p; i++) {
            double v = H[tri(i, j)];
            for (uint32_t k = 0; k < j; k++) v -= H[tri(i, k)] * H[tri(j, k)];
            H[tri(i, j)] = v / l;
        }
    }
    for (uint32_t i = 0; i < p; i++) {   // L z = grad
        double v = d[i];
        for (uint32_t k = 0; k < i; k++) v -= H[tri(i, k)] * d[k];
        d[i] = v / H[tri(i, i)];
    }
    for (uint32_t i = p; i-- > 0u;) {    // L^T delta = z
        double v = d[i];
        for (uint32_t k = i + 1u; k < p; k++) v -= H[tri(k, i)] * d[k];
        d[i] = v / H[tri(i, i)];
    }
    bool converged = true;
    for (uint32_t i = 0; i < p; i++) converged = converged && fabs(d[i]) <= tol;
    if (converged) {
        se = 1.0 / H[tri(p - 1u, p - 1u)];   // sqrt((H^-1)[g][g]): the last row of L^-1 is e_g / L[g][g]
        return PGENHIP_LOGIT_CONVERGED | it;
    }
    if (it == max_iter) return PGENHIP_LOGIT_NOT_CONVERGED | it;
    for (uint32_t i = 0; i < p; i++) beta[i] += d[i];
    return 0u;
}

__device__ void logit_write(const LogitArgs &a, uint64_t row, const double *beta, uint32_t p, double se, uint32_t status)
{
    double *dst = a.coef + row * a.c_stride;
    for (uint32_t i = 0; i < p; i++) dst[i] = beta[i];
    a.se[row] = se;
    a.status[row] = status;
}

__global__ __launch_bounds__(kThreads) void gt_logit_general_kernel(LogitArgs a)
{
    __shared__ double s_beta[kMaxP];
    __shared__ double s_sums[kSums];
    __shared__ double s_red[kWaves][kMaxP + 1u];
    __shared__ uint32_t s_state;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = a.sample_count, nc = a.n_cov, p = nc + 1u;
    for (uint64_t row = blockIdx.x; row < a.n_variants; row += gridDim.x) {
        const uint8_t *rec = row_record(a, row);
        double tab[4];
#pragma unroll
        for (uint32_t x = 0; x < 4u; x++) tab[x] = a.code_values[4u * row + x];
        if (tid < kMaxP) s_beta[tid] = tid < nc ? a.start[tid] : 0.0;
        if (tid == 0u) s_state = 0u;
        __syncthreads();
        for (uint32_t it = 1; it <= a.max_iter; it++) {
            for (uint32_t ra = 0; ra < p; ra++) {   // row ra of H and entry ra of the gradient
                double acc[kMaxP + 1u];
#pragma unroll
                for (uint32_t i = 0; i <= kMaxP; i++) acc[i] = 0.0;
                for (uint32_t s = tid; s < N; s += kThreads) {
                    const uint32_t code = (rec[s >> 2] >> (2u * (s & 3u))) & 3u;
                    const double gv = code == 0u ? tab[0] : code == 1u ? tab[1] : code == 2u ? tab[2] : tab[3];
                    bool kept;
                    const uint32_t k = kept_rank_of(a.kept_mask, a.kept_rank, s, kept);
                    if (!kept || gv != gv) continue;
                    const double *xr = a.design + (uint64_t)k * a.x_stride;
                    double x[kMaxP], eta = 0.0, xa = 0.0;
#pragma unroll
                    for (uint32_t c = 0; c < kMaxP; c++) {
                        x[c] = c < nc ? xr[c] : (c == nc ? gv : 0.0);
                        eta = fma(x[c], s_beta[c], eta);
                        xa = c == ra ? x[c] : xa;
                    }
                    const double mu = logistic(eta);
                    const double wx = mu * (1.0 - mu) * xa;
#pragma unroll
                    for (uint32_t c = 0; c < kMaxP; c++) acc[c] = fma(wx, x[c], acc[c]);
                    acc[kMaxP] = fma(xa, a.y[k] - mu, acc[kMaxP]);
                }
#pragma unroll
                for (uint32_t i = 0; i <= kMaxP; i++) {
                    const double v = wave_sum(acc[i]);
                    if (lane == 0u) s_red[wave][i] = v;
                }
                __syncthreads();
                if (tid <= kMaxP && (tid <= ra || tid == kMaxP)) {
                    double v = 0.0;
                    for (uint32_t w = 0; w < kWaves; w++) v += s_red[w][tid];
                    s_sums[tid == kMaxP ? kHalf + ra : tri(ra, tid)] = v;
                }
                __syncthreads();
            }
            if (tid == 0u) {
                double se;
                const uint32_t st = logit_advance(s_sums, s_beta, p, it, a.max_iter, a.tol, se);
                if (st) logit_write(a, row, s_beta, p, se, st);
                s_state = st;
            }
            __syncthreads();
            if (s_state != 0u) break;   // (block-uniform)
        }
        __syncthreads();
    }
}

// One evaluation's sums of one row over the lane's samples: the entries of H's lower half and of the gradient that PART owns
template <uint32_t P, uint32_t SPLIT, uint32_t PART>
__device__ __forceinline__ void logit_accumulate(const LogitArgs &a, const uint8_t *rec, const double (&tab)[4], const double *beta, uint32_t lane, double *sums)
{
    constexpr uint32_t kH = P * (P + 1u) / 2u;
    double H[kH], g[P];
#pragma unroll
    for (uint32_t i = 0; i < kH; i++) H[i] = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < P; c++) g[c] = 0.0;
    const uint32_t N = a.sample_count, nc = a.n_cov;
    for (uint32_t s = lane; s < N; s += 64u) {
        const uint32_t code = (rec[s >> 2] >> (2u * (s & 3u))) & 3u;
        const double gv = code == 0u ? tab[0] : code == 1u ? tab[1] : code == 2u ? tab[2] : tab[3];
        bool kept;
        const uint32_t k = kept_rank_of(a.kept_mask, a.kept_rank, s, kept);
        if (!kept || gv != gv) continue;
        const double *xr = a.design + (uint64_t)k * a.x_stride;
        double x[P], eta = 0.0;
#pragma unroll
        for (uint32_t c = 0; c < P; c++) {
            x[c] = c < nc ? xr[c] : (c == nc ? gv : 0.0);
            eta = fma(x[c], beta[c], eta);   // (LDS, the same address in every lane: a broadcast read, and no register copy of beta)
        }
        const double mu = logistic(eta);
        const double w = mu * (1.0 - mu), r = a.y[k] - mu;
#pragma unroll
        for (uint32_t ra = 0; ra < P; ra++) {
            if (row_part(ra, SPLIT) != PART) continue;
            g[ra] = fma(x[ra], r, g[ra]);
            const double wx = w * x[ra];
#pragma unroll
            for (uint32_t rb = 0; rb <= ra; rb++) H[ra * (ra + 1u) / 2u + rb] = fma(wx, x[rb], H[ra * (ra + 1u) / 2u + rb]);
        }
    }
#pragma unroll
    for (uint32_t ra = 0; ra < P; ra++) {
        if (row_part(ra, SPLIT) != PART) continue;
        const double gs = wave_sum(g[ra]);
        if (lane == 0u) sums[kHalf + ra] = gs;
#pragma unroll
        for (uint32_t rb = 0; rb <= ra; rb++) {
            const double hs = wave_sum(H[ra * (ra + 1u) / 2u + rb]);
            if (lane == 0u) sums[ra * (ra + 1u) / 2u + rb] = hs;
        }
    }
}

// logit_advance by one whole wave, in registers: lane i < p holds row i of H's lower half (r[k] = H[i][k], k <= i) and entry i of the
// gradient.  Column by column the pivot's lane broadcasts its row (shuffles) and the lanes below it finish their entry of that
// column; the two triangular solves move one value per (row, column) the same way.  The factor is logit_advance's operation for
// operation; the back substitution subtracts its terms in the opposite order.  The whole wave must be active.  Returns as
// logit_advance does, in every lane; on a final status the lanes write the row's outputs.
template <uint32_t P>
__device__ __forceinline__ uint32_t logit_advance_wave(const LogitArgs &a, uint64_t row, const double *sums, double *beta, uint32_t p, uint32_t it, uint32_t lane)
{
    const bool mine = lane < p;
    const uint32_t li = mine ? lane : 0u;
    double r[P], diag = 1.0;
#pragma unroll
    for (uint32_t k = 0; k < P; k++) r[k] = mine && k <= lane ? sums[tri(li, k)] : 0.0;
    double z = mine ? sums[kHalf + li] : 0.0;
    bool singular = false;
#pragma unroll
    for (uint32_t j = 0; j < P; j++) {
        if (j < p && !singular) {   // (wave-uniform)
            double v = r[j];
#pragma unroll
            for (uint32_t k = 0; k < j; k++) v -= r[k] * __shfl(r[k], (int)j, 64);   // lane j: its pivot; lanes below: their entry of column j
            const double piv = __shfl(v, (int)j, 64);
            if (!(piv > 0.0) || isinf(piv)) {
                singular = true;
            } else {
                const double l = sqrt(piv);
                r[j] = lane == j ? l : v / l;
                diag = lane == j ? l : diag;
            }
        }
    }
    uint32_t status = 0u;
    double se = __longlong_as_double(0x7FF8000000000000ll);
    if (singular) {
        status = PGENHIP_LOGIT_SINGULAR | it;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < P; j++) {   // L z = grad
            if (j < p) {
                if (lane == j) z = z / diag;
                const double zj = __shfl(z, (int)j, 64);
                if (lane > j) z -= r[j] * zj;
            }
        }
#pragma unroll
        for (uint32_t jj = 0; jj < P; jj++) {   // L^T delta = z, from the last row up: row j's lane hands L[j][i] * delta_j to lane i
            const uint32_t j = P - 1u - jj;
            if (j < p) {
                if (lane == j) z = z / diag;
#pragma unroll
                for (uint32_t i = 0; i < j; i++) {
                    const double t = __shfl(r[i] * z, (int)j, 64);
                    if (lane == i) z -= t;
                }
            }
        }
        const bool converged = __all(!mine || fabs(z) <= a.tol);
        if (converged) {
            se = 1.0 / __shfl(diag, (int)(p - 1u), 64);   // sqrt((H^-1)[g][g]): the last row of L^-1 is e_g / L[g][g]
            status = PGENHIP_LOGIT_CONVERGED | it;
        } else if (it == a.max_iter) {
            status = PGENHIP_LOGIT_NOT_CONVERGED | it;
        } else if (mine) {
            beta[li] += z;
        }
    }
    if (status) {
        if (mine) a.coef[row * a.c_stride + li] = beta[li];
        if (lane == 0u) {
            a.se[row] = se;
            a.status[row] = status;
        }
    }
    return status;
}

template <uint32_t P>
__global__ __launch_bounds__(kThreads) void gt_logit_fast_kernel(LogitArgs a)
{
    constexpr uint32_t SPLIT = waves_per_row(P), G = kWaves / SPLIT;
    __shared__ double s_beta[G][kMaxP];
    __shared__ double s_sums[G][kSums];
    __shared__ uint32_t s_state[G];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t slot = wave / SPLIT, part = wave % SPLIT;
    const uint32_t nc = a.n_cov, p = nc + 1u;
    const uint64_t V = a.n_variants, n_groups = groups(V, P);
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint64_t row = grp * G + slot;
        const bool live = row < V;
        const uint8_t *rec = row_record(a, live ? row : 0u);
        double tab[4];
#pragma unroll
        for (uint32_t x = 0; x < 4u; x++) tab[x] = a.code_values[4u * (live ? row : 0u) + x];
        if (part == 0u && lane < kMaxP) s_beta[slot][lane] = lane < nc ? a.start[lane] : 0.0;
        if (part == 0u && lane == 0u) s_state[slot] = live ? 0u : kNoRow;
        __syncthreads();
        for (uint32_t it = 1; it <= a.max_iter; it++) {
            if (s_state[slot] == 0u) {   // (wave-uniform)
                if (SPLIT == 1u || part == 0u) logit_accumulate<P, SPLIT, 0u>(a, rec, tab, s_beta[slot], lane, s_sums[slot]);
                else logit_accumulate<P, SPLIT, SPLIT - 1u>(a, rec, tab, s_beta[slot], lane, s_sums[slot]);
            }
            __syncthreads();
            if (part == 0u && s_state[slot] == 0u) {   // (wave-uniform)
                const uint32_t st = logit_advance_wave<P>(a, row, s_sums[slot], s_beta[slot], p, it, lane);
                if (lane == 0u) s_state[slot] = st;
            }
            __syncthreads();
            bool ended = true;
#pragma unroll
            for (uint32_t q = 0; q < G; q++) ended = ended && s_state[q] != 0u;
            if (ended) break;   // (block-uniform: read between two barriers)
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_gt_logit_general(const LogitArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0) return hipSuccess;
    hipLaunchKernelGGL(gt_logit_general_kernel, dim3(general_grid(a.n_variants, num_cus, blocks)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gt_logit_fast(const LogitArgs &a, int blocks, int num_cus, hipStream_t stream)
{
    if (a.n_variants == 0) return hipSuccess;
    const dim3 grid(fast_grid(a.n_variants, a.n_cov + 1u, num_cus, blocks));
    switch (bucket(a.n_cov + 1u)) {
        case 4u: hipLaunchKernelGGL(gt_logit_fast_kernel<4u>, grid, dim3(kThreads), 0, stream, a); break;
        case 8u: hipLaunchKernelGGL(gt_logit_fast_kernel<8u>, grid, dim3(kThreads), 0, stream, a); break;
        case 12u: hipLaunchKernelGGL(gt_logit_fast_kernel<12u>, grid, dim3(kThreads), 0, stream, a); break;
        default: hipLaunchKernelGGL(gt_logit_fast_kernel<16u>, grid, dim3(kThreads), 0, stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace pgenhip
