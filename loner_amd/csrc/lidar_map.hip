// The ground-truth LiDAR map (examples/fusion_portable/create_lidar_map.py, mask_gt_with_trajectory.py): every return
// moved to the world by the trajectory's pose at its own timestamp, and the statistical outlier filter the reference
// hands to Open3D (remove_statistical_outlier), which needs k nearest neighbours.
//
//   k_traj_transform   one thread per return: the trajectory interval of its timestamp (scipy's rule), R = R_i
//                      exp(alpha rel_rotvec_i) by Rodrigues in fp64, a linear translation, one rounding to fp32.
//   k_knn_grid         one wave per query: the k smallest (fp32 d^2, index) keys as a sorted list with one entry per
//                      lane (the ballot-and-shift insertion of k_cloud_normals); Chebyshev rings of cells as in
//                      k_nn_grid, the lanes taking a run of cells' points 64 at a time.
//   k_knn_brute        the queries the rings gave up on, from the pending list: one wave per query, the target through
//                      LDS in tiles shared by the block's four waves, the same key.
//   k_moments_*        {sum, count, sum of squared deviations from a centre} over the positive entries of an array:
//                      one partial row per 4096 entries, then one block adds the rows.
// Integer atomics only (the status word, the pending counter); every floating-point sum has a fixed shape: results
// repeat bit for bit.  Keys are compared, never followed; every index read from memory is clamped before it is used.
#include "cloud_grid.hpp"

namespace lnr {

constexpr int kMapBlock = 256;
constexpr int kMapWaves = kMapBlock / kWave;
constexpr int kKnnMaxK = LNR_KNN_MAX_K;
constexpr int kKnnTile = 1024;            // target points per LDS tile (16 KiB with their indices)
constexpr int kKnnBruteBlocks = 1024;     // at most: four per CU
constexpr int kMomPer = 16;               // entries per thread of a partial row
constexpr int kMomTile = kMapBlock * kMomPer;  // 4096 entries per row
static_assert(kKnnMaxK <= kWave, "the neighbour list holds one entry per lane");

// ------------------------------------------------------------------ trajectory transform
// searchsorted(traj_t, t, 'left'): the first j in [0, m) with traj_t[j] >= t (m if none).
__device__ __forceinline__ int64_t first_not_below(const double* __restrict__ ts, int64_t m, double t) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ts[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kMapBlock)
    k_traj_transform(const float* __restrict__ pts, const double* __restrict__ t, int64_t n,
                     const double* __restrict__ traj_t, const double* __restrict__ traj_xyz,
                     const double* __restrict__ traj_rot, const double* __restrict__ rel_rotvec, int64_t m,
                     double min_range, float* __restrict__ out, uint8_t* __restrict__ valid,
                     uint32_t* __restrict__ status) {
  const int64_t p = (int64_t)blockIdx.x * kMapBlock + threadIdx.x;
  if (p >= n) return;
  const double px = pts[p * 3], py = pts[p * 3 + 1], pz = pts[p * 3 + 2], tp = t[p];
  bool finite = isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(tp) && isfinite(min_range);
  const double range = sqrt((px * px + py * py) + pz * pz);
  // scipy's Slerp and interp1d raise outside [traj_t[0], traj_t[m - 1]]: never extrapolated
  const bool inside = finite && tp >= traj_t[0] && tp <= traj_t[m - 1];
  bool ok = inside && range > min_range;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (inside) {
    // i = searchsorted(left) - 1, a t on the first knot to interval 0; clamped: a table that is not increasing
    // gives a wrong interval, never an index outside it
    const int64_t i = min(max(first_not_below(traj_t, m, tp) - 1, (int64_t)0), m - 2);
    const double t0 = traj_t[i], t1 = traj_t[i + 1];
    const double alpha = (tp - t0) / (t1 - t0);
    const double vx = alpha * rel_rotvec[i * 3], vy = alpha * rel_rotvec[i * 3 + 1], vz = alpha * rel_rotvec[i * 3 + 2];
    // Rodrigues: exp([v]) = I + a [v] + b [v]^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 = 2 sin^2(th / 2) / th^2;
    // below 1e-4 rad the series a = 1 - th^2 / 6, b = 1 / 2 - th^2 / 24 (the next terms are below 1e-18)
    const double th2 = (vx * vx + vy * vy) + vz * vz;
    const double th = sqrt(th2);
    double a, b;
    if (th < 1e-4) {
      a = 1.0 - th2 / 6.0, b = 0.5 - th2 / 24.0;
    } else {
      const double sh = sin(0.5 * th);
      a = sin(th) / th, b = 2.0 * sh * sh / th2;
    }
    // q = exp([v]) p = p + a (v x p) + b v x (v x p)
    const double cx = vy * pz - vz * py, cy = vz * px - vx * pz, cz = vx * py - vy * px;
    const double dx = vy * cz - vz * cy, dy = vz * cx - vx * cz, dz = vx * cy - vy * cx;
    const double qx = px + (a * cx + b * dx), qy = py + (a * cy + b * dy), qz = pz + (a * cz + b * dz);
    const double* R = traj_rot + i * 9;
    const double* x0 = traj_xyz + i * 3;
    const double* x1 = traj_xyz + (i + 1) * 3;
    o0 = ((R[0] * qx + R[1] * qy) + R[2] * qz) + (x0[0] + alpha * (x1[0] - x0[0]));
    o1 = ((R[3] * qx + R[4] * qy) + R[5] * qz) + (x0[1] + alpha * (x1[1] - x0[1]));
    o2 = ((R[6] * qx + R[7] * qy) + R[8] * qz) + (x0[2] + alpha * (x1[2] - x0[2]));
    if (!(isfinite(o0) && isfinite(o1) && isfinite(o2))) finite = false, ok = false;  // a non-finite table entry
  }
  if (!finite) atomicOr(status, LNR_CLOUD_NONFINITE);
  out[p * 3] = ok ? (float)o0 : 0.f, out[p * 3 + 1] = ok ? (float)o1 : 0.f, out[p * 3 + 2] = ok ? (float)o2 : 0.f;
  valid[p] = ok ? 1 : 0;
}

// ------------------------------------------------------------------ k nearest neighbours
// The wave's neighbour list: lane l holds the l-th smallest key so far and its sorted position.
struct KnnList {
  uint64_t key;  // nn_pair, kNoNnKey = empty
  int32_t pos;   // the sorted position of that target
  uint64_t thr;  // the k-th smallest key (wave-uniform)
};

// Offers each lane's candidate (key = kNoNnKey: none).  The loop count comes from a ballot: wave-uniform.
__device__ __forceinline__ void knn_offer(uint64_t key, int32_t pos, int k, KnnList& l) {
  const int lane = threadIdx.x & 63;
  uint64_t m = __ballot(key < l.thr);
  while (m) {
    const int from = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const uint64_t c = __shfl(key, from, kWave);
    const int32_t cp = __shfl(pos, from, kWave);
    if (c >= l.thr) continue;  // the threshold fell since the ballot
    const uint64_t prev = __shfl_up(l.key, 1, kWave);
    const int32_t prevp = __shfl_up(l.pos, 1, kWave);
    if (l.key > c) {
      const bool here = lane == 0 || prev < c;
      l.key = here ? c : prev, l.pos = here ? cp : prevp;
    }
    l.thr = __shfl(l.key, k - 1, kWave);
  }
}

// The sorted positions [j0, j1) (wave-uniform), 64 at a time.  d2 is nan only for a non-finite target: no candidate.
__device__ __forceinline__ void knn_scan(const float* __restrict__ tp, const int32_t* __restrict__ tperm, int64_t j0,
                                         int64_t j1, float qx, float qy, float qz, int k, KnnList& l) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = j0; base < j1; base += kWave) {
    const int64_t j = base + lane;
    uint64_t key = kNoNnKey;
    if (j < j1) {
      const float d2 = nn_dist2(qx, qy, qz, tp[j * 3], tp[j * 3 + 1], tp[j * 3 + 2]);
      if (d2 == d2) key = nn_pair(d2, (uint32_t)tperm[j]);
    }
    knn_offer(key, (int32_t)j, k, l);
  }
}

// Cells z0 .. z1 of column (x, y): contiguous in key order, inside the row's positions [lo, hi).
__device__ __forceinline__ void knn_scan_run(const float* __restrict__ tp, const int64_t* __restrict__ tk,
                                             const int32_t* __restrict__ tperm, int64_t lo, int64_t hi, int64_t x,
                                             int64_t y, int64_t z0, int64_t z1, float qx, float qy, float qz, int k,
                                             KnnList& l) {
  const int64_t j0 = lower_bound(tk, lo, hi, cell_key(x, y, z0));
  const int64_t khi = cell_key(x, y, z1);
  const int64_t j1 = khi == kBadKey ? hi : lower_bound(tk, j0, hi, khi + 1);
  knn_scan(tp, tperm, j0, j1, qx, qy, qz, k, l);
}

// Row i of the outputs from the list: lanes 0 .. k - 1 write a neighbour each; mean_dist is the mean of the fp64
// distances to them (recomputed from the coordinates, as lnr_nn_search's dist), added in list order.  An empty entry
// (fewer than k targets with a finite key) gives idx -1 and inf.
__device__ __forceinline__ void knn_write(int64_t i, const KnnList& l, int k, float qx, float qy, float qz,
                                          const float* __restrict__ tp, int64_t n_tgt, int32_t* __restrict__ idx,
                                          float* __restrict__ d2, double* __restrict__ mean_dist) {
  const int lane = threadIdx.x & 63;
  const bool has = l.key != kNoNnKey;
  const int64_t pos = min(max((int64_t)l.pos, (int64_t)0), n_tgt - 1);
  const double ex = (double)qx - (double)tp[pos * 3], ey = (double)qy - (double)tp[pos * 3 + 1],
               ez = (double)qz - (double)tp[pos * 3 + 2];
  const double dist = has ? sqrt(ex * ex + ey * ey + ez * ez) : (double)INFINITY;
  if (lane < k) {
    idx[i * k + lane] = has ? (int32_t)(uint32_t)l.key : -1;
    d2[i * k + lane] = has ? __uint_as_float((uint32_t)(l.key >> 32)) : INFINITY;
  }
  if (!mean_dist) return;  // wave-uniform
  double s = 0.0;
  for (int a = 0; a < k; ++a) s += __shfl(dist, a, kWave);
  if (lane == 0) mean_dist[i] = __ddiv_rn(s, (double)k);
}

// Why a query may stop after ring r >= 1 once its list is full and kth <= (r cell)^2 (1 - 2^-20), kth being the fp32
// d^2 of its k-th smallest key (the proof above k_nn_grid, with "best" read as "k-th best"): a target t outside rings
// 0 .. r differs from the query q by at least r + 1 cells on some axis a, so the COMPUTED cell coordinates u =
// fl(fl(p_a - o_a) / cell) differ by more than r.  Each u carries two fp64 roundings, |u| is below 2^21 for a target
// and below 2^21 + r + 1 for a query that reaches it, so the exact coordinates differ by more than r (1 - 2^-28), that
// is |t - q|^2 > (r cell)^2 (1 - 2^-27).  (A query whose cell index was clamped lies farther out on that axis than its
// clamped cell: the bound only grows.)  The fp32 key of t loses at most 5.1 * 2^-24 relative (one rounding per
// difference, two per square, one per addition of non-negative terms; cell >= 1e-12 keeps (r cell)^2 far above the
// subnormals), so d2(t) > (r cell)^2 (1 - 2^-27 - 5.1 * 2^-24) > (r cell)^2 (1 - 2^-20) >= kth: strictly larger than
// every one of the k keys held, so t cannot enter the list, not even at a tie.  Ring 0 alone never stops a query:
// squares may underflow to d^2 = 0 for a neighbouring cell's point with a lower index.  Every cell is offered once
// (ring r visits the shell at Chebyshev distance r only), so no key enters the list twice.
// Everything that steers a loop here (the query, its cell, the rows' bounds, the list's threshold) is the same in all
// 64 lanes: the shuffles in knn_offer are always met by the whole wave.
__global__ void __launch_bounds__(kMapBlock)
    k_knn_grid(const float* __restrict__ src, int64_t n_src, const float* __restrict__ tp,
               const int64_t* __restrict__ tk, const int32_t* __restrict__ tperm, int64_t n_tgt,
               const double* __restrict__ origin, double cell, const int32_t* __restrict__ dims, int k,
               int32_t* __restrict__ idx, float* __restrict__ d2, double* __restrict__ mean_dist,
               uint32_t* __restrict__ status, int32_t* __restrict__ pend) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kMapWaves + wid;
  if (i >= n_src) return;  // the whole wave; the kernel has no barrier
  const float qx = src[i * 3], qy = src[i * 3 + 1], qz = src[i * 3 + 2];
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
    if (lane == 0) atomicOr(status, LNR_CLOUD_NONFINITE);
    if (lane < k) idx[i * k + lane] = -1, d2[i * k + lane] = INFINITY;
    if (mean_dist && lane == 0) mean_dist[i] = INFINITY;
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
  KnnList l = {kNoNnKey, 0, kNoNnKey};
  bool done = false;
  for (int64_t r = r0; r < r0 + kNnMaxRings && !done; ++r) {
    const int64_t x0 = max(c[0] - r, (int64_t)0), x1 = min(c[0] + r, dim[0] - 1);
    const int64_t y0 = max(c[1] - r, (int64_t)0), y1 = min(c[1] + r, dim[1] - 1);
    const int64_t z0 = max(c[2] - r, (int64_t)0), z1 = min(c[2] + r, dim[2] - 1);
    if ((x1 - x0 + 1) * (y1 - y0 + 1) > kNnMaxColumns) break;
    int64_t next = 0;  // rows follow each other in key order: the next one starts no earlier than this one ends
    for (int64_t x = x0; x <= x1; ++x) {
      const int64_t lo = lower_bound(tk, next, n_tgt, cell_key(x, y0, 0));
      const int64_t kend = cell_key(x, y1, ((int64_t)1 << kCellBits) - 1);  // the row's largest key
      const int64_t hi = kend == kBadKey ? n_tgt : lower_bound(tk, lo, n_tgt, kend + 1);
      next = hi;
      if (lo == hi) continue;  // an empty row: most of a sparse grid
      for (int64_t y = y0; y <= y1; ++y) {
        const bool rim = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
        if (rim) {
          if (z0 <= z1) knn_scan_run(tp, tk, tperm, lo, hi, x, y, z0, z1, qx, qy, qz, k, l);
        } else {  // inside the ring's square: its floor and its ceiling
          const int64_t zl = c[2] - r, zh = c[2] + r;
          if (zl >= 0 && zl < dim[2]) knn_scan_run(tp, tk, tperm, lo, hi, x, y, zl, zl, qx, qy, qz, k, l);
          if (r > 0 && zh >= 0 && zh < dim[2]) knn_scan_run(tp, tk, tperm, lo, hi, x, y, zh, zh, qx, qy, qz, k, l);
        }
      }
    }
    const double bound = (double)r * cell;
    const bool covered = c[0] - r <= 0 && c[0] + r >= dim[0] - 1 && c[1] - r <= 0 && c[1] + r >= dim[1] - 1 &&
                         c[2] - r <= 0 && c[2] + r >= dim[2] - 1;
    if (l.thr != kNoNnKey) {  // the list is full
      const double kth = (double)__uint_as_float((uint32_t)(l.thr >> 32));
      done = covered || (r >= 1 && kth <= bound * bound * (1.0 - kNnMargin));
    }
  }
  if (done) {
    knn_write(i, l, k, qx, qy, qz, tp, n_tgt, idx, d2, mean_dist);
    return;
  }
  if (lane != 0) return;
  const int32_t slot = atomicAdd(pend, 1);  // an integer count: the list's order is arbitrary, no result depends on it
  if (slot < n_src) pend[2 + slot] = (int32_t)i;
}

// The pending queries (pend[0]: their number, pend[2 ..]: the queries, in no particular order), a wave each; the
// target goes through LDS in tiles the block's waves share.  Loop counts are block-uniform: a wave without a query
// in a pass still loads tiles and meets the barriers, and offers nothing.
__global__ void __launch_bounds__(kMapBlock)
    k_knn_brute(const float* __restrict__ src, int64_t n_src, const float* __restrict__ tp,
                const int32_t* __restrict__ tperm, int64_t n_tgt, int k, const int32_t* __restrict__ pend,
                int32_t* __restrict__ idx, float* __restrict__ d2, double* __restrict__ mean_dist) {
  __shared__ float tx[kKnnTile], ty[kKnnTile], tz[kKnnTile];
  __shared__ int32_t ti[kKnnTile];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t total = min(max((int64_t)pend[0], (int64_t)0), n_src);
  const int32_t* list = pend + 2;
  for (int64_t p0 = (int64_t)blockIdx.x * kMapWaves; p0 < total; p0 += (int64_t)gridDim.x * kMapWaves) {
    const bool has = p0 + wid < total;  // wave-uniform
    const int64_t qi = min(max((int64_t)list[has ? p0 + wid : p0], (int64_t)0), n_src - 1);
    const float qx = src[qi * 3], qy = src[qi * 3 + 1], qz = src[qi * 3 + 2];
    KnnList l = {kNoNnKey, 0, kNoNnKey};
    for (int64_t base = 0; base < n_tgt; base += kKnnTile) {
      const int cnt = (int)min((int64_t)kKnnTile, n_tgt - base);
      __syncthreads();
      for (int j = threadIdx.x; j < cnt; j += kMapBlock) {
        const float* p = tp + (base + j) * 3;
        tx[j] = p[0], ty[j] = p[1], tz[j] = p[2], ti[j] = tperm[base + j];
      }
      __syncthreads();
      if (!has) continue;
      for (int j0 = 0; j0 < cnt; j0 += kWave) {
        const int j = j0 + lane;
        uint64_t key = kNoNnKey;
        if (j < cnt) {
          const float v = nn_dist2(qx, qy, qz, tx[j], ty[j], tz[j]);
          if (v == v) key = nn_pair(v, (uint32_t)ti[j]);
        }
        knn_offer(key, (int32_t)(base + j), k, l);
      }
    }
    if (has) knn_write(qi, l, k, qx, qy, qz, tp, n_tgt, idx, d2, mean_dist);
  }
}

// ------------------------------------------------------------------ moments
// Block sum of (a, b, c): lane butterflies, then the waves in order.  Thread 0 holds the totals.
__device__ __forceinline__ void block_sum3_d(double& a, double& b, double& c, double (*lds)[3]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a += __shfl_xor(a, o, kWave), b += __shfl_xor(b, o, kWave), c += __shfl_xor(c, o, kWave);
  }
  if (lane == 0) lds[wid][0] = a, lds[wid][1] = b, lds[wid][2] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0.0, b = 0.0, c = 0.0;
    for (int w = 0; w < kMapWaves; ++w) a += lds[w][0], b += lds[w][1], c += lds[w][2];
  }
}

__global__ void __launch_bounds__(kMapBlock)
    k_moments_rows(const double* __restrict__ v, int64_t n, double centre, const double* __restrict__ centre_dev,
                   double* __restrict__ rows) {
  __shared__ double lds[kMapWaves][3];
  const double mu = centre_dev ? centre_dev[0] : centre;
  const int64_t base = (int64_t)blockIdx.x * kMomTile;
  double s = 0.0, c = 0.0, q = 0.0;
#pragma unroll
  for (int e = 0; e < kMomPer; ++e) {
    const int64_t j = base + (int64_t)e * kMapBlock + threadIdx.x;
    if (j < n) {
      const double x = v[j];
      if (x > 0.0) s += x, c += 1.0, q += (x - mu) * (x - mu);
    }
  }
  block_sum3_d(s, c, q, lds);
  if (threadIdx.x == 0) {
    double* row = rows + 3 * (int64_t)blockIdx.x;
    row[0] = s, row[1] = c, row[2] = q;
  }
}

__global__ void __launch_bounds__(kMapBlock)
    k_moments_total(const double* __restrict__ rows, int64_t n_rows, double* __restrict__ out) {
  __shared__ double lds[kMapWaves][3];
  double s = 0.0, c = 0.0, q = 0.0;
  for (int64_t r = threadIdx.x; r < n_rows; r += kMapBlock) s += rows[3 * r], c += rows[3 * r + 1], q += rows[3 * r + 2];
  block_sum3_d(s, c, q, lds);
  if (threadIdx.x == 0) out[0] = s, out[1] = c, out[2] = q;
}

static unsigned map_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
static bool map_size_ok(int64_t n) { return n >= 1 && n <= LNR_CLOUD_MAX_POINTS; }
static int64_t moment_rows(int64_t n) { return (n + kMomTile - 1) / kMomTile; }

}  // namespace lnr

using namespace lnr;

extern "C" int lnr_trajectory_transform(const float* pts, const double* t, int64_t n, const double* traj_t,
                                        const double* traj_xyz, const double* traj_rot, const double* rel_rotvec,
                                        int64_t n_poses, double min_range, float* out, uint8_t* valid,
                                        uint32_t* status, void* stream) {
  LNR_REQUIRE(pts && t && traj_t && traj_xyz && traj_rot && rel_rotvec && out && valid && status,
              "lnr_trajectory_transform: null pointer");
  LNR_REQUIRE(map_size_ok(n), "lnr_trajectory_transform: n=%lld outside [1, 2^27]", (long long)n);
  LNR_REQUIRE(n_poses >= 2 && n_poses <= LNR_CLOUD_MAX_POINTS, "lnr_trajectory_transform: n_poses=%lld outside [2, 2^27]",
              (long long)n_poses);
  hipLaunchKernelGGL(k_traj_transform, dim3(map_blocks(n, kMapBlock)), dim3(kMapBlock), 0, as_stream(stream), pts, t, n,
                     traj_t, traj_xyz, traj_rot, rel_rotvec, n_poses, min_range, out, valid, status);
  LNR_RETURN_LAUNCH("lnr_trajectory_transform");
}

extern "C" int64_t lnr_knn_workspace_bytes(int64_t n_src) {
  if (!map_size_ok(n_src)) return 0;
  return (n_src + 2) * (int64_t)sizeof(int32_t);
}

extern "C" int lnr_knn_search(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                              const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell,
                              const int32_t* dims, int32_t k, void* workspace, int64_t ws_bytes, int32_t* idx,
                              float* d2, double* mean_dist, uint32_t* status, void* stream) {
  LNR_REQUIRE(src && tgt_sorted && tgt_keys && tgt_perm && origin && dims && workspace && idx && d2 && status,
              "lnr_knn_search: null pointer");
  LNR_REQUIRE(map_size_ok(n_src) && map_size_ok(n_tgt), "lnr_knn_search: bad sizes (n_src=%lld, n_tgt=%lld)",
              (long long)n_src, (long long)n_tgt);
  LNR_REQUIRE(k >= 1 && k <= kKnnMaxK && k <= n_tgt, "lnr_knn_search: k=%d outside [1, min(%d, n_tgt=%lld)]", (int)k,
              kKnnMaxK, (long long)n_tgt);
  LNR_REQUIRE(cell >= 1e-12 && std::isfinite(cell), "lnr_knn_search: cell=%g outside [1e-12, inf)", cell);
  LNR_REQUIRE(ws_bytes >= lnr_knn_workspace_bytes(n_src), "lnr_knn_search: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_knn_workspace_bytes(n_src));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_knn_search: workspace not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  int32_t* pend = static_cast<int32_t*>(workspace);
  LNR_REQUIRE(hipMemsetAsync(pend, 0, 2 * sizeof(int32_t), s) == hipSuccess, "lnr_knn_search: hipMemsetAsync failed");
  hipLaunchKernelGGL(k_knn_grid, dim3(map_blocks(n_src, kMapWaves)), dim3(kMapBlock), 0, s, src, n_src, tgt_sorted,
                     tgt_keys, tgt_perm, n_tgt, origin, cell, dims, (int)k, idx, d2, mean_dist, status, pend);
  const int64_t passes = (n_src + kMapWaves - 1) / kMapWaves;
  hipLaunchKernelGGL(k_knn_brute, dim3((unsigned)(passes < kKnnBruteBlocks ? passes : kKnnBruteBlocks)),
                     dim3(kMapBlock), 0, s, src, n_src, tgt_sorted, tgt_perm, n_tgt, (int)k, pend, idx, d2, mean_dist);
  LNR_RETURN_LAUNCH("lnr_knn_search");
}

extern "C" int64_t lnr_dist_moments_workspace_bytes(int64_t n) {
  if (!map_size_ok(n)) return 0;
  return 3 * moment_rows(n) * (int64_t)sizeof(double);
}

extern "C" int lnr_dist_moments(const double* v, int64_t n, double centre, const double* centre_dev, void* workspace,
                                int64_t ws_bytes, double* out, void* stream) {
  LNR_REQUIRE(v && workspace && out, "lnr_dist_moments: null pointer");
  LNR_REQUIRE(map_size_ok(n), "lnr_dist_moments: n=%lld outside [1, 2^27]", (long long)n);
  LNR_REQUIRE(ws_bytes >= lnr_dist_moments_workspace_bytes(n), "lnr_dist_moments: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_dist_moments_workspace_bytes(n));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_dist_moments: workspace not 8-byte aligned");
  const int64_t rows = moment_rows(n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_moments_rows, dim3((unsigned)rows), dim3(kMapBlock), 0, s, v, n, centre, centre_dev,
                     static_cast<double*>(workspace));
  hipLaunchKernelGGL(k_moments_total, dim3(1), dim3(kMapBlock), 0, s, static_cast<const double*>(workspace), rows, out);
  LNR_RETURN_LAUNCH("lnr_dist_moments");
}
