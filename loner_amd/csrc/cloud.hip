// Map evaluation (analysis/evaluate_lidar_map.py, analysis/renderer_lidar.py): the voxel filter and the
// nearest-neighbour distances the reference hands to Open3D (voxel_down_sample, compute_point_cloud_distance), and the
// sums its metrics are made of.
//
//   k_cell_keys       one thread per point: key = ix << 42 | iy << 21 | iz, i_a = floor((double(p_a) - origin_a) / cell).
//                     Serves the voxel filter (cell = voxel) and the search grid.
//   k_voxel_heads     1 where a sorted key starts a run; the caller's inclusive scan numbers the voxels.
//   k_voxel_starts    the first sorted position of every voxel.
//   k_voxel_partial   one thread per chunk of at most kVoxChunk points of ONE voxel: an fp64 sum, front to back.  Voxels
//                     differ widely in load (1 768 points against a median of a few on a 1 m grid), so neither a
//                     thread nor a wave owns a voxel.
//   k_voxel_finish    one thread per voxel: its chunk sums in chunk order, the mean, one rounding to fp32.
//   k_nn_grid         one thread per query: Chebyshev rings of cells around the query's own.  Two binary searches in
//                     the sorted keys bound a row of the ring (x fixed), short ones inside it find each column's z-run
//                     (no dense table: a 100 m map at 0.1 m has 10^9 cells).
//   k_nn_brute        the queries the rings gave up on: a block lists its own, the target passes through LDS in tiles,
//                     every lane scans its share for four queries of its wave.
//   k_dist_stats_*    {sum, count above a threshold} of a distance array: one partial row per 4096 entries, then one
//                     block adds the rows.
// Integer atomics only (the status word); every floating-point sum has a shape fixed by the sizes and the data:
// results repeat bit for bit.
#include "cloud_grid.hpp"

namespace lnr {

constexpr int kCloudBlock = 256;
constexpr int kVoxChunk = LNR_CLOUD_VOXEL_CHUNK;
constexpr double kCellLimit = (double)(1 << kCellBits);
constexpr int kNnBrutePts = 4;                       // queries per wave and pass of the exhaustive scan
constexpr int kNnTile = 1024;                        // target points per LDS tile (12 KiB)
constexpr int kNnPerPass = kNnBrutePts * (kCloudBlock / kWave);  // queries per block and pass
constexpr int kNnBruteBlocks = 1024;                 // at most: four per CU
constexpr int kStatPer = 16;                         // entries per thread of a partial row
constexpr int kStatTile = kCloudBlock * kStatPer;    // 4096 entries per row

// ------------------------------------------------------------------ keys
__global__ void __launch_bounds__(kCloudBlock)
    k_cell_keys(const float* __restrict__ pts, int64_t n, const double* __restrict__ origin, double cell,
                int64_t* __restrict__ keys, uint32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t bad = 0;
  int64_t c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = pts[i * 3 + a];
    const double u = cell_coord(p, origin[a], cell);
    if (!isfinite(p)) bad |= LNR_CLOUD_NONFINITE;
    else if (!(u >= 0.0 && u < kCellLimit)) bad |= LNR_CLOUD_GRID_RANGE;  // a nan origin lands here
    c[a] = bad ? 0 : (int64_t)u;
  }
  keys[i] = bad ? kBadKey : cell_key(c[0], c[1], c[2]);
  if (bad) atomicOr(status, bad);
}

// ------------------------------------------------------------------ voxel filter
__global__ void __launch_bounds__(kCloudBlock)
    k_voxel_heads(const int64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ heads) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= n) return;
  heads[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// Voxel v (0-based) of sorted position i, or -1 for a scan entry that is no voxel number.
__device__ __forceinline__ int64_t voxel_of(const int64_t* __restrict__ scan, int64_t i, int64_t n_vox) {
  const int64_t v = scan[i] - 1;
  return (v >= 0 && v < n_vox) ? v : -1;
}

// starts[v] = the first sorted position of voxel v, starts[n_vox] = n.  The buffer was filled with n beforehand, so a
// voxel a malformed scan never starts is empty, not unbounded.
__global__ void __launch_bounds__(kCloudBlock)
    k_voxel_starts(const int64_t* __restrict__ scan, int64_t n, int64_t n_vox, int64_t* __restrict__ starts) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t v = voxel_of(scan, i, n_vox);
  if (v < 0) return;
  if (i == 0 || voxel_of(scan, i - 1, n_vox) != v) starts[v] = i;
}

__global__ void __launch_bounds__(kCloudBlock) k_fill_i64(int64_t* __restrict__ dst, int64_t n, int64_t value) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i < n) dst[i] = value;
}

// The partial-sum slot of chunk j of voxel v.  Strictly increasing over (v, j) in voxel order, because
// floor((s + c) / K) - floor(s / K) >= ceil(c / K) - 1 for a voxel of c points starting at s; below n_vox + n / K + 1.
__device__ __forceinline__ int64_t chunk_slot(int64_t v, int64_t start, int64_t j) { return v + start / kVoxChunk + j; }

__global__ void __launch_bounds__(kCloudBlock)
    k_voxel_partial(const float* __restrict__ pts, const int64_t* __restrict__ perm, const int64_t* __restrict__ scan,
                    int64_t n, int64_t n_vox, const int64_t* __restrict__ starts, int64_t n_slots,
                    double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t v = voxel_of(scan, i, n_vox);
  if (v < 0) return;
  const int64_t s = starts[v], e = min(starts[v + 1], n);
  if (i < s || i >= e || (i - s) % kVoxChunk != 0) return;  // only the first position of a chunk works
  const int64_t last = min(i + kVoxChunk, e);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t p = i; p < last; ++p) {
    const int64_t q = perm[p];
    if (q < 0 || q >= n) continue;
    sx += (double)pts[q * 3], sy += (double)pts[q * 3 + 1], sz += (double)pts[q * 3 + 2];
  }
  const int64_t slot = chunk_slot(v, s, (i - s) / kVoxChunk);
  if (slot >= n_slots) return;  // cannot happen for a scan of heads
  partial[slot * 3] = sx, partial[slot * 3 + 1] = sy, partial[slot * 3 + 2] = sz;
}

__global__ void __launch_bounds__(kCloudBlock)
    k_voxel_finish(const int64_t* __restrict__ starts, int64_t n, int64_t n_vox, int64_t n_slots,
                   const double* __restrict__ partial, float* __restrict__ means, int32_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (v >= n_vox) return;
  const int64_t s = starts[v], e = min(starts[v + 1], n);
  const int64_t cnt = max(e - s, (int64_t)0);
  const int64_t chunks = (cnt + kVoxChunk - 1) / kVoxChunk;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t j = 0; j < chunks; ++j) {
    const int64_t slot = chunk_slot(v, s, j);
    if (slot >= n_slots) break;
    sx += partial[slot * 3], sy += partial[slot * 3 + 1], sz += partial[slot * 3 + 2];
  }
  const double c = (double)cnt;
  means[v * 3] = (float)__ddiv_rn(sx, c), means[v * 3 + 1] = (float)__ddiv_rn(sy, c);
  means[v * 3 + 2] = (float)__ddiv_rn(sz, c);
  if (counts) counts[v] = (int32_t)cnt;
}

// ------------------------------------------------------------------ nearest neighbour
// (NnBest, nn_offer and nn_scan_run: cloud_grid.hpp, shared with icp_grid.hip)
__device__ __forceinline__ void nn_write(int64_t i, const NnBest& b, float qx, float qy, float qz,
                                         const float* __restrict__ tp, int32_t* __restrict__ idx,
                                         float* __restrict__ d2, double* __restrict__ dist) {
  const double ex = (double)qx - (double)tp[b.pos * 3], ey = (double)qy - (double)tp[b.pos * 3 + 1],
               ez = (double)qz - (double)tp[b.pos * 3 + 2];
  idx[i] = (int32_t)(uint32_t)b.pair;
  d2[i] = __uint_as_float((uint32_t)(b.pair >> 32));
  dist[i] = sqrt(ex * ex + ey * ey + ez * ez);
}

// Why a query may stop after ring r >= 1 once best <= (r cell)^2 (1 - 2^-20), best being its smallest fp32 d^2:
// a target t outside rings 0 .. r differs from the query q by at least r + 1 cells on some axis a, so the COMPUTED
// cell coordinates u = fl(fl(p_a - o_a) / cell) differ by more than r.  Each u carries two fp64 roundings, |u| is below
// 2^21 for a target and below 2^21 + r + 1 for a query that reaches it, so the exact coordinates differ by more than
// r - 2^-51 (2^22 + r + 1) >= r (1 - 2^-28), that is |t_a - q_a| > r cell (1 - 2^-28) and |t - q|^2 > (r cell)^2 (1 - 2^-27).
// (A query whose cell index was clamped lies farther out on that axis than its clamped cell: the bound only grows.)
// The fp32 key of t: each difference carries one rounding (2^-24 relative), its square two more, the two additions of
// non-negative terms one each: d2(t) >= |t - q|^2 (1 - 5.1 * 2^-24) (cell >= 1e-12 keeps (r cell)^2 far above the
// subnormals).  Together d2(t) > (r cell)^2 (1 - 2^-27 - 5.1 * 2^-24) > (r cell)^2 (1 - 2^-20) >= best: strictly
// larger, so t cannot win, not even a tie.  Ring 0 alone never stops a query: squares may underflow to d^2 = 0 for a
// neighbouring cell's point with a lower index.
__global__ void __launch_bounds__(kCloudBlock)
    k_nn_grid(const float* __restrict__ src, int64_t n_src, const float* __restrict__ tp,
              const int64_t* __restrict__ tk, const int32_t* __restrict__ tperm, int64_t n_tgt,
              const double* __restrict__ origin, double cell, const int32_t* __restrict__ dims,
              int32_t* __restrict__ idx, float* __restrict__ d2, double* __restrict__ dist,
              uint32_t* __restrict__ status, int32_t* __restrict__ pend) {
  const int64_t i = (int64_t)blockIdx.x * kCloudBlock + threadIdx.x;
  if (i >= n_src) return;
  const float qx = src[i * 3], qy = src[i * 3 + 1], qz = src[i * 3 + 2];
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
    atomicOr(status, LNR_CLOUD_NONFINITE);
    idx[i] = -1, d2[i] = INFINITY, dist[i] = INFINITY;
    return;
  }
  int64_t c[3], dim[3];
  const float q[3] = {qx, qy, qz};
  int64_t r0 = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    dim[a] = min(max((int64_t)dims[a], (int64_t)1), (int64_t)1 << kCellBits);
    const double u = cell_coord(q[a], origin[a], cell);
    c[a] = (int64_t)fmin(fmax(u, -1073741824.0), 1073741824.0);  // nan (a bad origin) -> the lower clamp
    r0 = max(r0, max(-c[a], c[a] - (dim[a] - 1)));               // rings below r0 miss the box
  }
  NnBest b = {kNoNnKey, 0};
  bool done = false;
  for (int64_t r = r0; r < r0 + kNnMaxRings && !done; ++r) {
    const int64_t x0 = max(c[0] - r, (int64_t)0), x1 = min(c[0] + r, dim[0] - 1);
    const int64_t y0 = max(c[1] - r, (int64_t)0), y1 = min(c[1] + r, dim[1] - 1);
    const int64_t z0 = max(c[2] - r, (int64_t)0), z1 = min(c[2] + r, dim[2] - 1);
    if ((x1 - x0 + 1) * (y1 - y0 + 1) > kNnMaxColumns) break;
    int64_t next = 0;  // rows follow each other in key order: the next one starts no earlier than this one ends
    for (int64_t x = x0; x <= x1; ++x) {
      // the row: x fixed, y in [y0, y1], every z; two searches in the whole array, the columns' stay inside it
      const int64_t lo = lower_bound(tk, next, n_tgt, cell_key(x, y0, 0));
      const int64_t kend = cell_key(x, y1, ((int64_t)1 << kCellBits) - 1);  // the row's largest key
      const int64_t hi = kend == kBadKey ? n_tgt : lower_bound(tk, lo, n_tgt, kend + 1);
      next = hi;
      if (lo == hi) continue;  // an empty row: most of a sparse grid
      for (int64_t y = y0; y <= y1; ++y) {
        const bool rim = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
        if (rim) {
          if (z0 <= z1) nn_scan_run(tp, tk, tperm, lo, hi, x, y, z0, z1, qx, qy, qz, b);
        } else {  // inside the ring's square: its floor and its ceiling
          const int64_t zl = c[2] - r, zh = c[2] + r;
          if (zl >= 0 && zl < dim[2]) nn_scan_run(tp, tk, tperm, lo, hi, x, y, zl, zl, qx, qy, qz, b);
          if (r > 0 && zh >= 0 && zh < dim[2]) nn_scan_run(tp, tk, tperm, lo, hi, x, y, zh, zh, qx, qy, qz, b);
        }
      }
    }
    const double bound = (double)r * cell;
    const bool covered = c[0] - r <= 0 && c[0] + r >= dim[0] - 1 && c[1] - r <= 0 && c[1] + r >= dim[1] - 1 &&
                         c[2] - r <= 0 && c[2] + r >= dim[2] - 1;
    if (b.pair != kNoNnKey) {
      const double best = (double)__uint_as_float((uint32_t)(b.pair >> 32));
      done = covered || (r >= 1 && best <= bound * bound * (1.0 - kNnMargin));
    }
  }
  if (done) {
    nn_write(i, b, qx, qy, qz, tp, idx, d2, dist);
    return;
  }
  const int32_t slot = atomicAdd(pend, 1);  // an integer count: the list's order is arbitrary, no result depends on it
  if (slot < n_src) pend[2 + slot] = (int32_t)i;
}

__device__ __forceinline__ uint64_t wave_min_pair(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, kWave);
    v = w < v ? w : v;
  }
  return v;
}

// The queries the rings left pending, from the list k_nn_grid appended them to (pend[0]: their number, pend[2 ..]: the
// queries, in no particular order: every query's answer is its own).  Pending queries cluster where one cloud has a
// surface the other lacks, so the list, not the query's block, hands out the work: a block takes kNnPerPass queries
// per pass, kNnBrutePts per wave, and in a pass the target goes through LDS in tiles that the four waves share (the
// layout of k_icp_correspond), every lane scanning its share of each tile.  Loop counts are block-uniform: a wave
// without a query in a pass still loads tiles and meets the barriers.
__global__ void __launch_bounds__(kCloudBlock)
    k_nn_brute(const float* __restrict__ src, int64_t n_src, const float* __restrict__ tp,
               const int32_t* __restrict__ tperm, int64_t n_tgt, const int32_t* __restrict__ pend,
               int32_t* __restrict__ idx, float* __restrict__ d2, double* __restrict__ dist) {
  __shared__ float tx[kNnTile], ty[kNnTile], tz[kNnTile];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t total = min((int64_t)pend[0], n_src);
  const int32_t* list = pend + 2;
  for (int64_t p0 = (int64_t)blockIdx.x * kNnPerPass; p0 < total; p0 += (int64_t)gridDim.x * kNnPerPass) {
    int64_t qi[kNnBrutePts];
    float q[kNnBrutePts][3];
    NnBest b[kNnBrutePts];
    float bd[kNnBrutePts];
    bool has[kNnBrutePts];
#pragma unroll
    for (int a = 0; a < kNnBrutePts; ++a) {
      const int64_t slot = p0 + wid * kNnBrutePts + a;
      has[a] = slot < total;                                           // wave-uniform
      qi[a] = min(max((int64_t)list[has[a] ? slot : p0], (int64_t)0), n_src - 1);  // absent: a repeat, not written
      q[a][0] = src[qi[a] * 3], q[a][1] = src[qi[a] * 3 + 1], q[a][2] = src[qi[a] * 3 + 2];
      b[a].pair = kNoNnKey, b[a].pos = -1;
      bd[a] = INFINITY;
    }
    for (int64_t base = 0; base < n_tgt; base += kNnTile) {
      const int cnt = (int)min((int64_t)kNnTile, n_tgt - base);
      __syncthreads();
      for (int j = threadIdx.x; j < cnt; j += kCloudBlock) {
        const float* p = tp + (base + j) * 3;
        tx[j] = p[0], ty[j] = p[1], tz[j] = p[2];
      }
      __syncthreads();
      if (!has[0]) continue;
      for (int j = lane; j < cnt; j += kWave) {
        const float x = tx[j], y = ty[j], z = tz[j];
#pragma unroll
        for (int a = 0; a < kNnBrutePts; ++a) {
          // the scan keeps (d2, position) and reads an index only at an exact tie: no global load on the common path
          const float v = nn_dist2(q[a][0], q[a][1], q[a][2], x, y, z);
          if (v < bd[a]) bd[a] = v, b[a].pos = base + j;
          else if (v == bd[a] && (b[a].pos < 0 || tperm[base + j] < tperm[b[a].pos])) b[a].pos = base + j;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < kNnBrutePts; ++a) {
      b[a].pair = b[a].pos >= 0 ? nn_pair(bd[a], (uint32_t)tperm[b[a].pos]) : kNoNnKey;
      const uint64_t best = wave_min_pair(b[a].pair);
      const uint64_t owners = __ballot(b[a].pair == best);
      const int owner = __ffsll((unsigned long long)owners) - 1;
      b[a].pos = __shfl(b[a].pos, owner, kWave);
      b[a].pair = best;
      if (lane != 0 || !has[a]) continue;
      if (best != kNoNnKey) nn_write(qi[a], b[a], q[a][0], q[a][1], q[a][2], tp, idx, d2, dist);
      else idx[qi[a]] = -1, d2[qi[a]] = INFINITY, dist[qi[a]] = INFINITY;  // every distance was nan
    }
  }
}

// ------------------------------------------------------------------ distance statistics
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// Block sum of (a, b): lane butterflies, then the waves in order.  Thread 0 holds the totals.
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double (*lds)[2]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  a = wave_sum_d(a), b = wave_sum_d(b);
  if (lane == 0) lds[wid][0] = a, lds[wid][1] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0.0, b = 0.0;
    for (int w = 0; w < kCloudBlock / kWave; ++w) a += lds[w][0], b += lds[w][1];
  }
}

__global__ void __launch_bounds__(kCloudBlock)
    k_dist_stats_rows(const double* __restrict__ dist, int64_t n, double threshold, double* __restrict__ rows) {
  __shared__ double lds[kCloudBlock / kWave][2];
  const int64_t base = (int64_t)blockIdx.x * kStatTile;
  double s = 0.0, c = 0.0;
#pragma unroll
  for (int k = 0; k < kStatPer; ++k) {
    const int64_t j = base + (int64_t)k * kCloudBlock + threadIdx.x;
    if (j < n) {
      const double v = dist[j];
      s += v;
      c += v > threshold ? 1.0 : 0.0;
    }
  }
  block_sum2_d(s, c, lds);
  if (threadIdx.x == 0) rows[2 * (int64_t)blockIdx.x] = s, rows[2 * (int64_t)blockIdx.x + 1] = c;
}

__global__ void __launch_bounds__(kCloudBlock)
    k_dist_stats_total(const double* __restrict__ rows, int64_t n_rows, double* __restrict__ out) {
  __shared__ double lds[kCloudBlock / kWave][2];
  double s = 0.0, c = 0.0;
  for (int64_t r = threadIdx.x; r < n_rows; r += kCloudBlock) s += rows[2 * r], c += rows[2 * r + 1];
  block_sum2_d(s, c, lds);
  if (threadIdx.x == 0) out[0] = s, out[1] = c;
}

static unsigned blocks_for(int64_t n) { return (unsigned)((n + kCloudBlock - 1) / kCloudBlock); }
static bool cloud_size_ok(int64_t n) { return n >= 1 && n <= LNR_CLOUD_MAX_POINTS; }
static bool cell_ok(double cell) { return cell >= 1e-12 && std::isfinite(cell); }
static int64_t voxel_slots(int64_t n, int64_t n_vox) { return n_vox + n / kVoxChunk + 1; }
static int64_t stat_rows(int64_t n) { return (n + kStatTile - 1) / kStatTile; }

}  // namespace lnr

using namespace lnr;

extern "C" int lnr_cloud_cell_keys(const float* pts, int64_t n, const double* origin, double cell, int64_t* keys,
                                   uint32_t* status, void* stream) {
  LNR_REQUIRE(pts && origin && keys && status, "lnr_cloud_cell_keys: null pointer");
  LNR_REQUIRE(cloud_size_ok(n), "lnr_cloud_cell_keys: n=%lld outside [1, 2^27]", (long long)n);
  LNR_REQUIRE(cell_ok(cell), "lnr_cloud_cell_keys: cell=%g outside [1e-12, inf)", cell);
  hipLaunchKernelGGL(k_cell_keys, dim3(blocks_for(n)), dim3(kCloudBlock), 0, as_stream(stream), pts, n, origin, cell,
                     keys, status);
  LNR_RETURN_LAUNCH("lnr_cloud_cell_keys");
}

extern "C" int lnr_voxel_heads(const int64_t* sorted_keys, int64_t n, int32_t* heads, void* stream) {
  LNR_REQUIRE(sorted_keys && heads, "lnr_voxel_heads: null pointer");
  LNR_REQUIRE(cloud_size_ok(n), "lnr_voxel_heads: n=%lld outside [1, 2^27]", (long long)n);
  hipLaunchKernelGGL(k_voxel_heads, dim3(blocks_for(n)), dim3(kCloudBlock), 0, as_stream(stream), sorted_keys, n,
                     heads);
  LNR_RETURN_LAUNCH("lnr_voxel_heads");
}

extern "C" int64_t lnr_voxel_workspace_bytes(int64_t n, int64_t n_vox) {
  if (!cloud_size_ok(n) || n_vox < 1 || n_vox > n) return 0;
  return ((n_vox + 1) + 3 * voxel_slots(n, n_vox)) * (int64_t)sizeof(double);
}

extern "C" int lnr_voxel_reduce(const float* pts, const int64_t* perm, const int64_t* head_scan, int64_t n,
                                int64_t n_vox, void* workspace, int64_t ws_bytes, float* means, int32_t* counts,
                                void* stream) {
  LNR_REQUIRE(pts && perm && head_scan && workspace && means, "lnr_voxel_reduce: null pointer");
  LNR_REQUIRE(cloud_size_ok(n) && n_vox >= 1 && n_vox <= n, "lnr_voxel_reduce: bad sizes (n=%lld, n_vox=%lld)",
              (long long)n, (long long)n_vox);
  LNR_REQUIRE(ws_bytes >= lnr_voxel_workspace_bytes(n, n_vox), "lnr_voxel_reduce: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_voxel_workspace_bytes(n, n_vox));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_voxel_reduce: workspace not 8-byte aligned");
  int64_t* starts = static_cast<int64_t*>(workspace);
  double* partial = reinterpret_cast<double*>(starts + n_vox + 1);
  const int64_t slots = voxel_slots(n, n_vox);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_fill_i64, dim3(blocks_for(n_vox + 1)), dim3(kCloudBlock), 0, s, starts, n_vox + 1, n);
  hipLaunchKernelGGL(k_voxel_starts, dim3(blocks_for(n)), dim3(kCloudBlock), 0, s, head_scan, n, n_vox, starts);
  hipLaunchKernelGGL(k_voxel_partial, dim3(blocks_for(n)), dim3(kCloudBlock), 0, s, pts, perm, head_scan, n, n_vox,
                     starts, slots, partial);
  hipLaunchKernelGGL(k_voxel_finish, dim3(blocks_for(n_vox)), dim3(kCloudBlock), 0, s, starts, n, n_vox, slots, partial,
                     means, counts);
  LNR_RETURN_LAUNCH("lnr_voxel_reduce");
}

extern "C" int64_t lnr_nn_workspace_bytes(int64_t n_src) {
  if (!cloud_size_ok(n_src)) return 0;
  return (n_src + 2) * (int64_t)sizeof(int32_t);
}

extern "C" int lnr_nn_search(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                             const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell,
                             const int32_t* dims, void* workspace, int64_t ws_bytes, int32_t* idx, float* d2,
                             double* dist, uint32_t* status, void* stream) {
  LNR_REQUIRE(src && tgt_sorted && tgt_keys && tgt_perm && origin && dims && workspace && idx && d2 && dist && status,
              "lnr_nn_search: null pointer");
  LNR_REQUIRE(cloud_size_ok(n_src) && cloud_size_ok(n_tgt), "lnr_nn_search: bad sizes (n_src=%lld, n_tgt=%lld)",
              (long long)n_src, (long long)n_tgt);
  LNR_REQUIRE(cell_ok(cell), "lnr_nn_search: cell=%g outside [1e-12, inf)", cell);
  LNR_REQUIRE(ws_bytes >= lnr_nn_workspace_bytes(n_src), "lnr_nn_search: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_nn_workspace_bytes(n_src));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_nn_search: workspace not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  int32_t* pend = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(k_fill_i64, dim3(1), dim3(kCloudBlock), 0, s, static_cast<int64_t*>(workspace), (int64_t)1,
                     (int64_t)0);
  hipLaunchKernelGGL(k_nn_grid, dim3(blocks_for(n_src)), dim3(kCloudBlock), 0, s, src, n_src, tgt_sorted, tgt_keys,
                     tgt_perm, n_tgt, origin, cell, dims, idx, d2, dist, status, pend);
  const int64_t passes = (n_src + kNnPerPass - 1) / kNnPerPass;
  hipLaunchKernelGGL(k_nn_brute, dim3((unsigned)(passes < kNnBruteBlocks ? passes : kNnBruteBlocks)), dim3(kCloudBlock), 0, s, src,
                     n_src, tgt_sorted, tgt_perm, n_tgt, pend, idx, d2, dist);
  LNR_RETURN_LAUNCH("lnr_nn_search");
}

extern "C" int64_t lnr_dist_stats_workspace_bytes(int64_t n) {
  if (!cloud_size_ok(n)) return 0;
  return 2 * stat_rows(n) * (int64_t)sizeof(double);
}

extern "C" int lnr_dist_stats(const double* dist, int64_t n, double threshold, void* workspace, int64_t ws_bytes,
                              double* out, void* stream) {
  LNR_REQUIRE(dist && workspace && out, "lnr_dist_stats: null pointer");
  LNR_REQUIRE(cloud_size_ok(n), "lnr_dist_stats: n=%lld outside [1, 2^27]", (long long)n);
  LNR_REQUIRE(ws_bytes >= lnr_dist_stats_workspace_bytes(n), "lnr_dist_stats: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_dist_stats_workspace_bytes(n));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_dist_stats: workspace not 8-byte aligned");
  const int64_t rows = stat_rows(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_dist_stats_rows, dim3((unsigned)rows), dim3(kCloudBlock), 0, s, dist, n, threshold,
                     static_cast<double*>(workspace));
  hipLaunchKernelGGL(k_dist_stats_total, dim3(1), dim3(kCloudBlock), 0, s, static_cast<const double*>(workspace), rows,
                     out);
  LNR_RETURN_LAUNCH("lnr_dist_stats");
}
