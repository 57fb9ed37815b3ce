// Registration on the cell grid of the cloud searches (cloud_grid.hpp): what icp.hip computes exhaustively, for clouds
// its O(n^2) kernels cannot take.  Same keys ((fp32 d^2, caller's index), every operation rounded), same sums
// (icp_math.hpp), so with the same inputs the results are icp.hip's bit for bit.
//
//   k_normals_from_knn      one wave per query, lane j its j-th neighbour from a list (lnr_knn_search's): the tail of
//                           k_cloud_normals.
//   k_icp_correspond_grid   one thread per source point: p = T s, the Chebyshev rings of p's cell as in k_nn_grid, but
//                           never beyond ring R = lnr_icp_grid_rings(threshold, cell): a target outside rings 0 .. R
//                           has a key above (R cell)^2 (1 - 2^-20) >= threshold^2 (the proof above k_nn_grid) and
//                           could not be a kept pair.  No pending list, no exhaustive pass.  The 29 terms go through
//                           LDS; one partial row per 16 consecutive source points, added in index order from 0.0:
//                           k_icp_correspond's rows.  k_icp_update (icp.hip) ends the round.
// Integer atomics only (the status word).
#include "cloud_grid.hpp"
#include "icp_math.hpp"

namespace lnr {

constexpr int kNormBlock = 256;                           // 4 waves, one query each
constexpr int kNormWaves = kNormBlock / kWave;
constexpr int kGridBlock = 64;                            // source points per block: 4 partial rows
constexpr int kGridRows = kGridBlock / kIcpBlockPts;
static_assert(kGridBlock % kIcpBlockPts == 0, "a block owns whole partial rows");
static_assert((2 * kNnMaxRings + 1) * (2 * kNnMaxRings + 1) <= kNnMaxColumns, "the widest ring the walk may take");

__global__ void __launch_bounds__(kNormBlock)
    k_normals_from_knn(const float* __restrict__ pts, int64_t n, const float* __restrict__ tgt, int64_t n_tgt,
                       const int32_t* __restrict__ idx, int32_t k, float* __restrict__ normals) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * kNormWaves + wid;
  if (q >= n) return;  // wave-uniform, and the kernel has no barrier
  const float qx = pts[q * 3], qy = pts[q * 3 + 1], qz = pts[q * 3 + 2];
  const bool has = lane < k;
  const int64_t raw = has ? (int64_t)idx[q * k + lane] : 0;
  const bool inside = raw >= 0 && raw < n_tgt;
  const bool bad = __ballot(has && !inside) != 0;  // an index outside the target is never followed
  const int64_t id = inside ? raw : 0;
  const double px = tgt[id * 3], py = tgt[id * 3 + 1], pz = tgt[id * 3 + 2];
  double cov[6];
  neighbour_covariance(has, px, py, pz, k, cov);
  if (lane != 0) return;
  write_normal(cov, bad, qx, qy, qz, normals + q * 3);
}

__global__ void __launch_bounds__(kGridBlock)
    k_icp_correspond_grid(const float* __restrict__ src, int32_t n_src, const float* __restrict__ tp,
                          const int64_t* __restrict__ tk, const int32_t* __restrict__ tperm, int64_t n_tgt,
                          const double* __restrict__ origin, double cell, const int32_t* __restrict__ dims,
                          const float* __restrict__ tgt_normals, float thr2, int32_t rings, int32_t round,
                          const lnr_icp_state* __restrict__ st, int32_t n_rows, double* __restrict__ partials,
                          int32_t* __restrict__ corr_idx, float* __restrict__ corr_d2, uint32_t* __restrict__ status) {
  if (round > 0 && st->converged) return;  // block-uniform
  __shared__ double terms[kGridBlock][kIcpTerms];
  const int64_t i = (int64_t)blockIdx.x * kGridBlock + threadIdx.x;
  const bool live = i < n_src;
  const int64_t ic = live ? i : (int64_t)n_src - 1;  // the tail repeats the last point and is masked below
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = st->T[e];
  double pd[3];
  float pf[3];
  icp_transform(T, src[ic * 3], src[ic * 3 + 1], src[ic * 3 + 2], pd, pf);
  const bool finite = isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]);
  if (live && !finite) atomicOr(status, LNR_CLOUD_NONFINITE);
  NnBest b = {kNoNnKey, 0};
  if (live && finite) {
    int64_t c[3], dim[3];
    int64_t r0 = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      dim[a] = min(max((int64_t)dims[a], (int64_t)1), (int64_t)1 << kCellBits);
      const double u = cell_coord(pf[a], origin[a], cell);
      c[a] = (int64_t)fmin(fmax(u, -1073741824.0), 1073741824.0);  // nan (a bad origin) -> the lower clamp
      r0 = max(r0, max(-c[a], c[a] - (dim[a] - 1)));               // rings below r0 miss the box
    }
    bool done = false;
    for (int64_t r = r0; r <= rings && !done; ++r) {
      const int64_t x0 = max(c[0] - r, (int64_t)0), x1 = min(c[0] + r, dim[0] - 1);
      const int64_t y0 = max(c[1] - r, (int64_t)0), y1 = min(c[1] + r, dim[1] - 1);
      const int64_t z0 = max(c[2] - r, (int64_t)0), z1 = min(c[2] + r, dim[2] - 1);
      int64_t next = 0;  // rows follow each other in key order: the next one starts no earlier than this one ends
      for (int64_t x = x0; x <= x1; ++x) {
        const int64_t lo = lower_bound(tk, next, n_tgt, cell_key(x, y0, 0));
        const int64_t kend = cell_key(x, y1, ((int64_t)1 << kCellBits) - 1);  // the row's largest key
        const int64_t hi = kend == kBadKey ? n_tgt : lower_bound(tk, lo, n_tgt, kend + 1);
        next = hi;
        if (lo == hi) continue;
        for (int64_t y = y0; y <= y1; ++y) {
          const bool rim = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
          if (rim) {
            if (z0 <= z1) nn_scan_run(tp, tk, tperm, lo, hi, x, y, z0, z1, pf[0], pf[1], pf[2], b);
          } else {  // inside the ring's square: its floor and its ceiling
            const int64_t zl = c[2] - r, zh = c[2] + r;
            if (zl >= 0 && zl < dim[2]) nn_scan_run(tp, tk, tperm, lo, hi, x, y, zl, zl, pf[0], pf[1], pf[2], b);
            if (r > 0 && zh >= 0 && zh < dim[2]) nn_scan_run(tp, tk, tperm, lo, hi, x, y, zh, zh, pf[0], pf[1], pf[2], b);
          }
        }
      }
      if (b.pair != kNoNnKey) {
        const double bound = (double)r * cell;
        const double best = (double)__uint_as_float((uint32_t)(b.pair >> 32));
        done = r >= 1 && best <= bound * bound * (1.0 - kNnMargin);
      }
    }
  }
  // every thread of the block is here again: the terms, then the rows
  const float d2 = __uint_as_float((uint32_t)(b.pair >> 32));
  const int64_t ci = (int64_t)(uint32_t)b.pair;
  const bool keep = live && b.pair != kNoNnKey && d2 < thr2 && ci < n_tgt;
  if (live) {
    if (corr_idx) corr_idx[i] = keep ? (int32_t)ci : -1;
    if (corr_d2) corr_d2[i] = keep ? d2 : 0.f;
  }
  double* row = terms[threadIdx.x];
  if (keep) {
    const int64_t j = b.pos;
    icp_pair_terms(pd[0], pd[1], pd[2], tp[j * 3], tp[j * 3 + 1], tp[j * 3 + 2], tgt_normals[ci * 3],
                   tgt_normals[ci * 3 + 1], tgt_normals[ci * 3 + 2], row);
  } else {
    icp_zero_terms(row);
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < kGridRows * kIcpRow / kGridBlock; ++pass) {
    const int e = pass * kGridBlock + threadIdx.x;
    const int lr = e / kIcpRow, t = e % kIcpRow;
    const int64_t grow = (int64_t)blockIdx.x * kGridRows + lr;
    if (grow >= n_rows) continue;
    double s = 0.0;
    if (t < kIcpTerms)
      for (int p = 0; p < kIcpBlockPts; ++p) s += terms[lr * kIcpBlockPts + p][t];
    partials[grow * kIcpRow + t] = s;
  }
}

static int64_t grid_rows(int64_t n_src) { return (n_src + kIcpBlockPts - 1) / kIcpBlockPts; }

}  // namespace lnr

using namespace lnr;

extern "C" int lnr_normals_from_knn(const float* pts, int64_t n, const float* tgt, int64_t n_tgt, const int32_t* idx,
                                    int32_t k, float* normals, void* stream) {
  LNR_REQUIRE(pts && tgt && idx && normals, "lnr_normals_from_knn: null pointer");
  LNR_REQUIRE(k >= 3 && k <= 64, "lnr_normals_from_knn: k=%d outside [3, 64]", k);
  LNR_REQUIRE(n >= 1 && n <= LNR_CLOUD_MAX_POINTS && n_tgt >= 1 && n_tgt <= LNR_CLOUD_MAX_POINTS,
              "lnr_normals_from_knn: bad sizes (n=%lld, n_tgt=%lld)", (long long)n, (long long)n_tgt);
  hipLaunchKernelGGL(k_normals_from_knn, dim3((unsigned)((n + kNormWaves - 1) / kNormWaves)), dim3(kNormBlock), 0,
                     as_stream(stream), pts, n, tgt, n_tgt, idx, k, normals);
  LNR_RETURN_LAUNCH("lnr_normals_from_knn");
}

extern "C" int32_t lnr_icp_grid_rings(float threshold, double cell) {
  if (!(threshold > 0.f) || !std::isfinite(threshold) || !(cell >= 1e-12) || !std::isfinite(cell)) return 0;
  const float thr2 = (float)((double)threshold * (double)threshold);
  if (!std::isfinite(thr2)) return 0;  // no ring bounds an infinite threshold
  for (int32_t r = 1; r <= kNnMaxRings; ++r) {
    const double bound = (double)r * cell;
    if (bound * bound * (1.0 - kNnMargin) >= (double)thr2) return r;
  }
  return 0;
}

extern "C" int64_t lnr_icp_grid_workspace_bytes(int64_t n_src) {
  if (n_src < 1 || n_src > LNR_ICP_MAX_POINTS) return 0;
  return grid_rows(n_src) * kIcpRow * (int64_t)sizeof(double);
}

extern "C" int lnr_icp_stage_grid(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                                  const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell,
                                  const int32_t* dims, const float* tgt_normals, float threshold,
                                  int32_t max_iterations, double rel_fitness, double rel_rmse, lnr_icp_state* state,
                                  void* workspace, int64_t ws_bytes, int32_t* corr_idx, float* corr_d2,
                                  uint32_t* status, void* stream) {
  LNR_REQUIRE(src && tgt_sorted && tgt_keys && tgt_perm && origin && dims && tgt_normals && state && workspace && status,
              "lnr_icp_stage_grid: null pointer");
  LNR_REQUIRE(n_src >= 1 && n_src <= LNR_ICP_MAX_POINTS && n_tgt >= 1 && n_tgt <= LNR_ICP_MAX_POINTS,
              "lnr_icp_stage_grid: bad sizes (n_src=%lld, n_tgt=%lld)", (long long)n_src, (long long)n_tgt);
  LNR_REQUIRE(threshold > 0.f && std::isfinite(threshold),
              "lnr_icp_stage_grid: threshold must be positive and finite");
  LNR_REQUIRE(max_iterations >= 0 && max_iterations <= 1000, "lnr_icp_stage_grid: max_iterations=%d outside [0, 1000]",
              max_iterations);
  LNR_REQUIRE(rel_fitness >= 0.0 && rel_rmse >= 0.0, "lnr_icp_stage_grid: negative convergence criterion");
  LNR_REQUIRE(cell >= 1e-12 && std::isfinite(cell), "lnr_icp_stage_grid: cell=%g outside [1e-12, inf)", cell);
  const int32_t rings = lnr_icp_grid_rings(threshold, cell);
  LNR_REQUIRE(rings >= 1, "lnr_icp_stage_grid: threshold=%g needs more than %d rings of cell=%g", (double)threshold,
              kNnMaxRings, cell);
  LNR_REQUIRE(ws_bytes >= lnr_icp_grid_workspace_bytes(n_src), "lnr_icp_stage_grid: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_icp_grid_workspace_bytes(n_src));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_icp_stage_grid: workspace not 8-byte aligned");
  const int64_t rows = grid_rows(n_src);
  const unsigned blocks = (unsigned)((n_src + kGridBlock - 1) / kGridBlock);
  const float thr2 = (float)((double)threshold * (double)threshold);
  for (int32_t round = 0; round <= max_iterations; ++round) {
    hipLaunchKernelGGL(k_icp_correspond_grid, dim3(blocks), dim3(kGridBlock), 0, as_stream(stream), src, (int32_t)n_src,
                       tgt_sorted, tgt_keys, tgt_perm, n_tgt, origin, cell, dims, tgt_normals, thr2, rings, round, state,
                       (int32_t)rows, static_cast<double*>(workspace), corr_idx, corr_d2, status);
    icp_launch_update(static_cast<const double*>(workspace), (int32_t)rows, (int32_t)n_src, round, max_iterations,
                      rel_fitness, rel_rmse, state, as_stream(stream));
  }
  LNR_RETURN_LAUNCH("lnr_icp_stage_grid");
}
