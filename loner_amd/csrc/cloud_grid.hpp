// The uniform grid of the cloud searches (cloud.hip: lnr_nn_search; lidar_map.hip: lnr_knn_search): cell keys, the
// fp32 search key and the search in the sorted keys.  Shared so that both searches order targets by the same bits.
#pragma once
#include "common.hpp"

namespace lnr {

constexpr int kCellBits = LNR_CLOUD_CELL_BITS;
constexpr int64_t kBadKey = LNR_CLOUD_BAD_KEY;
constexpr int kNnMaxRings = LNR_NN_MAX_RINGS;
constexpr int kNnMaxColumns = 81;                    // a ring cut to the box may not hold more columns than ring 4
constexpr double kNnMargin = 9.5367431640625e-07;    // 2^-20, see k_nn_grid
constexpr uint64_t kNoNnKey = ~(uint64_t)0;

__device__ __forceinline__ int64_t cell_key(int64_t ix, int64_t iy, int64_t iz) {
  return (ix << (2 * kCellBits)) | (iy << kCellBits) | iz;
}
// floor((double(p) - origin) / cell): one IEEE subtraction, one IEEE division (no reciprocal), as numpy computes it
__device__ __forceinline__ double cell_coord(float p, double origin, double cell) {
  return floor(__ddiv_rn(__dsub_rn((double)p, origin), cell));
}

// (d^2, index) as one integer: non-negative floats order like their bit patterns, ties go to the lower index.
__device__ __forceinline__ uint64_t nn_pair(float d2, uint32_t idx) {
  return ((uint64_t)__float_as_uint(d2) << 32) | idx;
}
// Every operation rounded on its own, in this order: contraction can never change the bits.
__device__ __forceinline__ float nn_dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The first position in [lo, hi) whose key is >= k (hi if none).
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ keys, int64_t lo, int64_t hi, int64_t k) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ one query's walk (k_nn_grid, k_icp_correspond_grid)
struct NnBest {
  uint64_t pair;  // nn_pair of the best so far
  int64_t pos;    // its sorted position
};

// One candidate: the index is only read when the distance does not lose outright.
__device__ __forceinline__ void nn_offer(float d2, int64_t j, const int32_t* __restrict__ tperm, NnBest& b) {
  if (__float_as_uint(d2) > (uint32_t)(b.pair >> 32)) return;  // d2 >= 0: bit order is value order
  const uint64_t pair = nn_pair(d2, (uint32_t)tperm[j]);
  if (pair < b.pair) b.pair = pair, b.pos = j;
}

// Cells z0 .. z1 of column (x, y): contiguous in key order.  [lo, hi) are the sorted positions of the column's row
// (x fixed, the ring's y range), so the search is short and stays in a few cache lines.  Only positions below hi <=
// n_tgt are read; a key is compared, never followed.
__device__ __forceinline__ void nn_scan_run(const float* __restrict__ tp, const int64_t* __restrict__ tk,
                                            const int32_t* __restrict__ tperm, int64_t lo, int64_t hi, int64_t x,
                                            int64_t y, int64_t z0, int64_t z1, float qx, float qy, float qz,
                                            NnBest& b) {
  const int64_t khi = cell_key(x, y, z1);
  for (int64_t j = lower_bound(tk, lo, hi, cell_key(x, y, z0)); j < hi && tk[j] <= khi; ++j)
    nn_offer(nn_dist2(qx, qy, qz, tp[j * 3], tp[j * 3 + 1], tp[j * 3 + 2]), j, tperm, b);
}

}  // namespace lnr
