// bvcf_pca.hip.h — the dense symmetric eigensolver behind --pca (bvcf_pca_eigen): Householder tridiagonalisation and the
// back-transformation of the eigenvectors, in double
// Part of the gfx950 device code of libbvcf; see bvcf_device.hip.h for the kernel map.
//
// The matrix is the full symmetric n x n matrix in double, row-major with the leading dimension ld (n rounded up to 16
// doubles, so every row starts on a 128-byte line).  The algorithm is LAPACK's unblocked dsytd2 with dlarfg's reflectors,
// turned to rows: a symmetric matrix's column j below the diagonal is its row j behind it, and rows are what is contiguous.
// Step j = 0 .. n-2, with m = n - j - 1, x = A[j][j+1 .. n) and A22 = A[j+1 .. n)[j+1 .. n):
//   k_pca_house   one workgroup.  alpha = x_0, beta = -sign(alpha) ||x||, tau = (beta - alpha) / beta, v = x / (alpha - beta)
//                 with v_0 = 1, written over x: row j keeps v_j for the back-transformation.  d_j = A[j][j], e_j = beta.  When
//                 ||x[1:]|| = 0 the reflector is the identity: tau = 0, e_j = alpha, x stays.
//   k_pca_symv    p = tau A22 v: a wave per row of A22, lanes along the row.
//   k_pca_w       one workgroup.  w = p - (tau p^T v / 2) v.
//   k_pca_rank2   A22 -= v w^T + w v^T, elementwise; v_r w_c and w_r v_c are rounded separately and then added, so the
//                 update of (r, c) and of (c, r) are the same number and A22 stays exactly symmetric.
// and d_{n-1} = A[n-1][n-1] (k_pca_house with m = 0).  One launch per phase and step, in stream order: no device-wide barrier,
// no cooperative kernel.  The host solves the tridiagonal (d, e) (bvcf_pca_tri.h); then
//   k_pca_back    one workgroup per vector: u = H_0 H_1 .. H_{n-2} z, the reflectors H_j = I - tau_j v_j v_j^T applied in reverse
//                 order, u in registers (kPcaPerThread elements per thread); then u / ||u|| and the sign rule -- the component
//                 of largest magnitude positive, ties to the lowest index.
//   k_pca_expand  the packed float32 lower triangle, a run of rows at a time, into both halves of the double matrix.
//
// Determinism.  Every sum has one order: a thread adds its elements (index t, t + threads, ..) in ascending order, a wave
// adds its lanes by a fixed butterfly, a workgroup its waves in wave order.  Workgroup sizes are constants; the grids of
// k_pca_symv and k_pca_rank2 only decide which workgroup computes a row or an element, never how.  No atomics.
//
// The norms need no scaling: the entries start as float32 (|a| < 2^128, a^2 < 2^256) and an orthogonal similarity keeps every
// later entry within the matrix's Frobenius norm, at most n 2^128 -- squares and sums of n of them stay far inside double's
// range, and an entry too small for its square to register is too small to matter to a sum the others dominate.
//
// This is the memory-bound form: per step A22 is read once by k_pca_symv and read and written by k_pca_rank2, 24 m^2 bytes,
// 8 n^3 over all steps.  Not done: the blocked form (dsytrd's rank-2k update on the FP64 matrix cores), and reading only
// one triangle.
#pragma once

#include "bvcf_common.hip.h"

namespace bvcf_dev {

constexpr uint32_t kPcaWgThreads = 1024;  // the single-workgroup kernels
constexpr uint32_t kPcaWgWaves = kPcaWgThreads / kWave;
constexpr uint32_t kPcaPerThread = BVCF_PAIR_MAX_SAMPLES / kPcaWgThreads;  // k_pca_back: elements of u per thread
constexpr uint32_t kPcaRank2Rows = 8;     // rows of A22 per workgroup of k_pca_rank2 (kWgThreads columns wide)
static_assert(kPcaPerThread * kPcaWgThreads == BVCF_PAIR_MAX_SAMPLES, "a vector of the largest matrix fits the registers of one workgroup");

__device__ __forceinline__ double pca_wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// the sum over a workgroup of kPcaWgThreads threads, the same bits in every thread.  lds: kPcaWgWaves doubles
__device__ __forceinline__ double pca_block_sum(double v, double *lds) {
  v = pca_wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (uint32_t w = 0; w < kPcaWgWaves; w++) s += lds[w];
  __syncthreads();  // (the next sum writes lds again)
  return s;
}

// grid (ceil(n / kWgThreads), rows): row row0 + blockIdx.y of the packed triangle, src = the run's first element
__global__ __launch_bounds__(kWgThreads) void k_pca_expand(const float *__restrict__ src, uint32_t row0, uint32_t rows, double *__restrict__ A,
                                                           uint32_t ld, uint32_t n) {
  const uint32_t i = row0 + blockIdx.y, j = blockIdx.x * kWgThreads + threadIdx.x;
  if (blockIdx.y >= rows || i >= n || j > i) return;
  const uint64_t at = (uint64_t)i * (i + 1) / 2 - (uint64_t)row0 * (row0 + 1) / 2 + j;
  const double v = (double)src[at];
  A[(uint64_t)i * ld + j] = v;
  A[(uint64_t)j * ld + i] = v;
}

__global__ __launch_bounds__(kPcaWgThreads) void k_pca_house(double *__restrict__ A, uint32_t ld, uint32_t n, uint32_t j, double *__restrict__ d,
                                                             double *__restrict__ e, double *__restrict__ tau) {
  __shared__ double lds[kPcaWgWaves];
  const uint32_t m = n - j - 1, t = threadIdx.x;
  double *row = A + (uint64_t)j * ld + j;  // row[0] the diagonal, row[1 ..= m] is x
  if (t == 0) d[j] = row[0];
  if (m == 0) return;
  const double alpha = row[1];
  double s = 0.0;
  for (uint32_t i = 2 + t; i <= m; i += kPcaWgThreads) s += row[i] * row[i];
  const double xn2 = pca_block_sum(s, lds);
  if (xn2 == 0.0) {
    if (t == 0) {
      e[j] = alpha;
      tau[j] = 0.0;
    }
    return;
  }
  const double beta = -copysign(sqrt(alpha * alpha + xn2), alpha), div = alpha - beta;
  for (uint32_t i = 2 + t; i <= m; i += kPcaWgThreads) row[i] = row[i] / div;
  if (t == 0) {
    row[1] = 1.0;
    e[j] = beta;
    tau[j] = (beta - alpha) / beta;
  }
}

// grid ceil(m / kWavesPerWg): a wave per row r of A22
__global__ __launch_bounds__(kWgThreads) void k_pca_symv(const double *__restrict__ A, uint32_t ld, uint32_t n, uint32_t j,
                                                         const double *__restrict__ tau, double *__restrict__ p) {
  const uint32_t m = n - j - 1, lane = threadIdx.x & (kWave - 1);
  const uint32_t r = blockIdx.x * kWavesPerWg + threadIdx.x / kWave;
  if (r >= m) return;
  const double tj = tau[j];
  double s = 0.0;
  if (tj != 0.0) {
    const double *v = A + (uint64_t)j * ld + j + 1, *row = A + (uint64_t)(j + 1 + r) * ld + j + 1;
    for (uint32_t c = lane; c < m; c += kWave) s += row[c] * v[c];
    s = pca_wave_sum(s);
  }
  if (lane == 0) p[r] = tj * s;
}

__global__ __launch_bounds__(kPcaWgThreads) void k_pca_w(const double *__restrict__ A, uint32_t ld, uint32_t n, uint32_t j,
                                                         const double *__restrict__ tau, const double *__restrict__ p, double *__restrict__ w) {
  __shared__ double lds[kPcaWgWaves];
  const uint32_t m = n - j - 1, t = threadIdx.x;
  const double *v = A + (uint64_t)j * ld + j + 1;
  double s = 0.0;
  for (uint32_t i = t; i < m; i += kPcaWgThreads) s += p[i] * v[i];
  const double c = tau[j] * pca_block_sum(s, lds) / 2.0;
  for (uint32_t i = t; i < m; i += kPcaWgThreads) w[i] = p[i] - c * v[i];
}

// grid (ceil(m / kWgThreads), ceil(m / kPcaRank2Rows))
__global__ __launch_bounds__(kWgThreads) void k_pca_rank2(double *__restrict__ A, uint32_t ld, uint32_t n, uint32_t j, const double *__restrict__ tau,
                                                          const double *__restrict__ w) {
  const uint32_t m = n - j - 1, c = blockIdx.x * kWgThreads + threadIdx.x;
  if (c >= m || tau[j] == 0.0) return;
  const double *v = A + (uint64_t)j * ld + j + 1;
  const double vc = v[c], wc = w[c];
  const uint32_t r0 = blockIdx.y * kPcaRank2Rows;
#pragma unroll
  for (uint32_t k = 0; k < kPcaRank2Rows; k++) {
    const uint32_t r = r0 + k;
    if (r >= m) break;
    double *a = A + (uint64_t)(j + 1 + r) * ld + j + 1 + c;
    *a = __dsub_rn(*a, __dadd_rn(__dmul_rn(v[r], wc), __dmul_rn(w[r], vc)));
  }
}

// grid k: vector blockIdx.x.  z, u: [k][n]
__global__ __launch_bounds__(kPcaWgThreads) void k_pca_back(const double *__restrict__ A, uint32_t ld, uint32_t n, const double *__restrict__ tau,
                                                            const double *__restrict__ z, double *__restrict__ u_out) {
  __shared__ double lds[kPcaWgWaves];
  __shared__ double best_v[kPcaWgWaves];
  __shared__ uint32_t best_i[kPcaWgWaves];
  const uint32_t t = threadIdx.x;
  const double *zin = z + (uint64_t)blockIdx.x * n;
  double u[kPcaPerThread], vq[kPcaPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPcaPerThread; q++) {
    const uint32_t i = t + q * kPcaWgThreads;
    u[q] = i < n ? zin[i] : 0.0;
  }
  for (uint32_t j = n >= 2 ? n - 1 : 0; j-- > 0;) {
    const double tj = tau[j];
    if (tj == 0.0) continue;  // (the same for every thread)
    const double *row = A + (uint64_t)j * ld;
    double s = 0.0;
#pragma unroll
    for (uint32_t q = 0; q < kPcaPerThread; q++) {
      const uint32_t i = t + q * kPcaWgThreads;
      vq[q] = (i > j && i < n) ? row[i] : 0.0;
      s += vq[q] * u[q];
    }
    const double f = tj * pca_block_sum(s, lds);
#pragma unroll
    for (uint32_t q = 0; q < kPcaPerThread; q++) u[q] -= f * vq[q];
  }
  double s = 0.0;
#pragma unroll
  for (uint32_t q = 0; q < kPcaPerThread; q++) s += u[q] * u[q];
  const double nrm = sqrt(pca_block_sum(s, lds));
  // the component of largest magnitude, ties to the lowest index: a thread's indices ascend with q, so ">" keeps its first
  double bv = 0.0;
  uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t q = 0; q < kPcaPerThread; q++) {
    const uint32_t i = t + q * kPcaWgThreads;
    if (nrm > 0.0 && nrm < INFINITY) u[q] = u[q] / nrm;
    if (i < n && (bi == 0xFFFFFFFFu || fabs(u[q]) > fabs(bv))) {
      bv = u[q];
      bi = i;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off, kWave);
    const uint32_t oi = __shfl_xor(bi, off, kWave);
    if (oi != 0xFFFFFFFFu && (bi == 0xFFFFFFFFu || fabs(ov) > fabs(bv) || (fabs(ov) == fabs(bv) && oi < bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if ((t & (kWave - 1)) == 0) {
    best_v[t / kWave] = bv;
    best_i[t / kWave] = bi;
  }
  __syncthreads();
  bv = best_v[0];
  bi = best_i[0];
  for (uint32_t w = 1; w < kPcaWgWaves; w++) {
    const double ov = best_v[w];
    const uint32_t oi = best_i[w];
    if (oi != 0xFFFFFFFFu && (bi == 0xFFFFFFFFu || fabs(ov) > fabs(bv) || (fabs(ov) == fabs(bv) && oi < bi))) {
      bv = ov;
      bi = oi;
    }
  }
  const bool flip = bv < 0.0;
#pragma unroll
  for (uint32_t q = 0; q < kPcaPerThread; q++) {
    const uint32_t i = t + q * kPcaWgThreads;
    if (i < n) u_out[(uint64_t)blockIdx.x * n + i] = flip ? -u[q] : u[q];
  }
}

}  // namespace bvcf_dev
