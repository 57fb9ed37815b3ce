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

}  // namespace lnr
