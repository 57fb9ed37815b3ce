// The arithmetic the exhaustive registration kernels (icp.hip) and the grid ones (icp_grid.hip) have in common: the
// source transform, a kept pair's 29 terms, the fp64 wave sum, and a normal from a neighbour list (covariance, cyclic
// Jacobi, orientation).  Shared so that both paths round the same expressions in the same order: with the same
// neighbours and the same pairs their results are the same bits.
#pragma once
#include "common.hpp"

namespace lnr {

constexpr int kIcpBlockPts = 16;                      // source points per partial row
constexpr int kIcpRow = 32;                           // doubles per partial row: 27 sums, count, sum d^2, padding
constexpr int kIcpTerms = 29;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// ------------------------------------------------------------------ ICP
// One k_icp_update round on `stream` (icp.hip): the stages of both searches end their rounds with it.
void icp_launch_update(const double* partials, int32_t n_rows, int32_t n_src, int32_t round, int32_t max_iterations,
                       double rel_fitness, double rel_rmse, lnr_icp_state* state, hipStream_t stream);

// p = T s in fp64 (pd), rounded to fp32 for the search (pf).
__device__ __forceinline__ void icp_transform(const double (&T)[12], double sx, double sy, double sz, double (&pd)[3],
                                              float (&pf)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pd[r] = T[4 * r] * sx + T[4 * r + 1] * sy + T[4 * r + 2] * sz + T[4 * r + 3];
    pf[r] = (float)pd[r];
  }
}

__device__ __forceinline__ void icp_zero_terms(double* __restrict__ row) {
#pragma unroll
  for (int t = 0; t < kIcpTerms; ++t) row[t] = 0.0;
}

// The terms of a kept pair (p, q) with q's normal n: J^T J (upper triangle, row-major, 21), J^T r (6), 1, |p - q|^2;
// J = [p x n, n], r = (p - q) . n.
__device__ __forceinline__ void icp_pair_terms(double px, double py, double pz, double qx, double qy, double qz,
                                               double nx, double ny, double nz, double* __restrict__ row) {
  const double ex = px - qx, ey = py - qy, ez = pz - qz;
  const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
  const double r = ex * nx + ey * ny + ez * nz;
  int t = 0;
#pragma unroll
  for (int u = 0; u < 6; ++u)
#pragma unroll
    for (int v = u; v < 6; ++v) row[t++] = J[u] * J[v];
#pragma unroll
  for (int u = 0; u < 6; ++u) row[21 + u] = J[u] * r;
  row[27] = 1.0;
  row[28] = ex * ex + ey * ey + ez * ez;
}

// ------------------------------------------------------------------ normals
// Jacobi rotation annihilating a_pq of a symmetric 3x3; r is the third index.  (Numerical Recipes' jacobi.)
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // 0 when theta overflows
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  double x = arp, y = arq;
  arp = c * x - s * y, arq = s * x + c * y;
  x = v0p, y = v0q, v0p = c * x - s * y, v0q = s * x + c * y;
  x = v1p, y = v1q, v1p = c * x - s * y, v1q = s * x + c * y;
  x = v2p, y = v2q, v2p = c * x - s * y, v2q = s * x + c * y;
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix (a00 a01 a02; . a11 a12; . . a22).
__device__ __forceinline__ void smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22,
                                                double& nx, double& ny, double& nz) {
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  for (int sweep = 0; sweep < 12; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  // the column of the smallest diagonal entry (ties to the lower index), picked with 0 / 1 weights: selects between
  // the columns would be turned into an indexed private array
  const double w1 = (a11 < a00 && !(a22 < a11)) ? 1.0 : 0.0, w2 = (a22 < a00 && a22 < a11) ? 1.0 : 0.0;
  const double w0 = 1.0 - w1 - w2;
  const double x = w0 * v00 + w1 * v01 + w2 * v02, y = w0 * v10 + w1 * v11 + w2 * v12,
               z = w0 * v20 + w1 * v21 + w2 * v22;
  const double len = sqrt(x * x + y * y + z * z);
  nx = x / len, ny = y / len, nz = z / len;
}

// The covariance (a00 a01 a02 a11 a12 a22) of a wave's k neighbours about their mean: lane j < k (`has`) holds
// neighbour j.  Every lane of the wave calls it and ends with the same six numbers.
__device__ __forceinline__ void neighbour_covariance(bool has, double px, double py, double pz, int k, double (&a)[6]) {
  const double inv = 1.0 / (double)k;
  const double mx = wave_sum_f64(has ? px : 0.0) * inv, my = wave_sum_f64(has ? py : 0.0) * inv,
               mz = wave_sum_f64(has ? pz : 0.0) * inv;
  const double cx = has ? px - mx : 0.0, cy = has ? py - my : 0.0, cz = has ? pz - mz : 0.0;
  a[0] = wave_sum_f64(cx * cx) * inv, a[1] = wave_sum_f64(cx * cy) * inv, a[2] = wave_sum_f64(cx * cz) * inv;
  a[3] = wave_sum_f64(cy * cy) * inv, a[4] = wave_sum_f64(cy * cz) * inv, a[5] = wave_sum_f64(cz * cz) * inv;
}

// The normal of that covariance at the query (qx, qy, qz), written to o[0 .. 3): (0, 0, 1) for a zero covariance
// (or `fallback`) and for a non-finite eigenvector, turned so that normal . q <= 0.
__device__ __forceinline__ void write_normal(const double (&a)[6], bool fallback, float qx, float qy, float qz,
                                             float* __restrict__ o) {
  double nx = 0.0, ny = 0.0, nz = 1.0;
  const bool zero = a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0 && a[3] == 0.0 && a[4] == 0.0 && a[5] == 0.0;
  if (!zero && !fallback) smallest_eigvec(a[0], a[1], a[2], a[3], a[4], a[5], nx, ny, nz);
  if (!(isfinite(nx) && isfinite(ny) && isfinite(nz))) nx = 0.0, ny = 0.0, nz = 1.0;
  if (nx * (double)qx + ny * (double)qy + nz * (double)qz > 0.0) nx = -nx, ny = -ny, nz = -nz;
  o[0] = (float)nx, o[1] = (float)ny, o[2] = (float)nz;
}

}  // namespace lnr
