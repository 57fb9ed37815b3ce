// Frame-to-frame tracking (src/tracking/tracker.py:167-255): cloud normals and two-stage point-to-plane ICP, the work the
// reference hands to Open3D (estimate_normals, registration_icp with TransformationEstimationPointToPlane).
//
//   k_cloud_normals   one wave per point: its exact k nearest neighbours by (fp32 d^2, index), kept as a sorted list
//                     with one entry per lane; the cloud passes through LDS in tiles.  Covariance about the
//                     neighbours' mean and a cyclic Jacobi eigen-solve in fp64, normal towards the origin.
//   k_icp_correspond  one wave per kIcpPts source points: p = T s (fp64, rounded to fp32 for the search), every lane
//                     scans its share of each LDS tile of the target, a (d^2, index) minimum over the wave; the kept
//                     pairs' J^T J, J^T r, count and sum d^2 in fp64, one partial row per block (no atomics).
//   k_icp_update      one block: the partial rows added in a fixed order, fitness / rmse / convergence, and thread 0's
//                     6x6 Cholesky solve and T <- M(x) T.
// A stage is max_iterations + 1 rounds of (correspond, update) enqueued at once; every kernel of a round after the
// first returns at once when state->converged is set, so the stream needs no host decision.
// Every sum has a fixed shape (lane butterflies, then rows in index order): results repeat bit for bit.
#include "icp_math.hpp"

namespace lnr {

constexpr int kIcpBlock = 256;                        // 4 waves
constexpr int kIcpWaves = kIcpBlock / kWave;
constexpr int kIcpTile = 1024;                        // points of the searched cloud per LDS tile (12 KiB)
constexpr int kIcpPts = 4;                            // source points per wave
static_assert(kIcpPts * kIcpWaves == kIcpBlockPts, "one partial row per block");
constexpr int kIcpStripes = kIcpBlock / kIcpRow;      // 8 row stripes in the update's reduction
constexpr int64_t kNormalsMaxN = (int64_t)1 << 18;
constexpr uint64_t kNoKey = ~(uint64_t)0;

// (d^2, index) as one integer: non-negative floats order like their bit patterns, ties go to the lower index.
__device__ __forceinline__ uint64_t nn_key(float d2, uint32_t idx) {
  return ((uint64_t)__float_as_uint(d2) << 32) | idx;
}
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, kWave);
    v = w < v ? w : v;
  }
  return v;
}

// One tile of the cloud into LDS (x, y, z planes); entries past n are left unread by the callers.
__device__ __forceinline__ void load_tile(const float* __restrict__ pts, int64_t base, int cnt, float* tx, float* ty,
                                          float* tz) {
  for (int j = threadIdx.x; j < cnt; j += kIcpBlock) {
    const float* p = pts + (base + j) * 3;
    tx[j] = p[0], ty[j] = p[1], tz[j] = p[2];
  }
}

// ------------------------------------------------------------------ normals
__global__ void __launch_bounds__(kIcpBlock)
    k_cloud_normals(const float* __restrict__ pts, int32_t n, int32_t k, float* __restrict__ normals) {
  __shared__ float tx[kIcpTile], ty[kIcpTile], tz[kIcpTile];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * kIcpWaves + wid;
  const bool live = q < n;  // a dead wave still takes part in the barriers
  const int64_t qc = live ? q : n - 1;
  const float qx = pts[qc * 3], qy = pts[qc * 3 + 1], qz = pts[qc * 3 + 2];
  uint64_t list = kNoKey;  // lane l: the l-th smallest key so far
  uint64_t thr = kNoKey;   // the k-th smallest
  for (int64_t base = 0; base < n; base += kIcpTile) {
    const int cnt = (int)min((int64_t)kIcpTile, n - base);
    __syncthreads();
    load_tile(pts, base, cnt, tx, ty, tz);
    __syncthreads();
    for (int j0 = 0; j0 < cnt; j0 += kWave) {
      const int j = j0 + lane;
      uint64_t key = kNoKey;
      if (j < cnt) key = nn_key(dist2(qx, qy, qz, tx[j], ty[j], tz[j]), (uint32_t)(base + j));
      uint64_t m = __ballot(key < thr);
      while (m) {
        const int from = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t c = __shfl(key, from, kWave);
        if (c >= thr) continue;  // the threshold fell since the ballot
        const uint64_t prev = __shfl_up(list, 1, kWave);
        if (list > c) list = (lane == 0 || prev < c) ? c : prev;
        thr = __shfl(list, k - 1, kWave);
      }
    }
  }
  // lanes 0 .. k - 1 hold the neighbours (k <= n: every one is a point)
  const bool has = lane < k;
  const int64_t id = has ? (int64_t)(uint32_t)list : qc;
  const double px = pts[id * 3], py = pts[id * 3 + 1], pz = pts[id * 3 + 2];
  double cov[6];
  neighbour_covariance(has, px, py, pz, k, cov);
  if (!live || lane != 0) return;
  write_normal(cov, false, qx, qy, qz, normals + q * 3);
}

// ------------------------------------------------------------------ ICP
__global__ void k_icp_init(lnr_icp_state* __restrict__ st, lnr_icp_state init) { *st = init; }

__global__ void __launch_bounds__(kIcpBlock)
    k_icp_correspond(const float* __restrict__ src, int32_t n_src, const float* __restrict__ tgt,
                     const float* __restrict__ tgt_normals, int32_t n_tgt, float thr2, int32_t round,
                     const lnr_icp_state* __restrict__ st, double* __restrict__ partials,
                     int32_t* __restrict__ corr_idx, float* __restrict__ corr_d2) {
  if (round > 0 && st->converged) return;  // block-uniform
  __shared__ float tx[kIcpTile], ty[kIcpTile], tz[kIcpTile];
  __shared__ double terms[kIcpBlockPts][kIcpTerms];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t first = ((int64_t)blockIdx.x * kIcpWaves + wid) * kIcpPts;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = st->T[i];
  double pd[kIcpPts][3];
  float pf[kIcpPts][3], best[kIcpPts];
  uint32_t besti[kIcpPts];
#pragma unroll
  for (int a = 0; a < kIcpPts; ++a) {
    const int64_t i = min(first + a, (int64_t)n_src - 1);  // the tail repeats the last point and is masked below
    icp_transform(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], pd[a], pf[a]);
    best[a] = INFINITY;
    besti[a] = 0xFFFFFFFFu;
  }
  for (int64_t base = 0; base < n_tgt; base += kIcpTile) {
    const int cnt = (int)min((int64_t)kIcpTile, n_tgt - base);
    __syncthreads();
    load_tile(tgt, base, cnt, tx, ty, tz);
    __syncthreads();
    for (int j = lane; j < cnt; j += kWave) {
      const float x = tx[j], y = ty[j], z = tz[j];
#pragma unroll
      for (int a = 0; a < kIcpPts; ++a) {
        const float d2 = dist2(pf[a][0], pf[a][1], pf[a][2], x, y, z);
        if (d2 < best[a]) best[a] = d2, besti[a] = (uint32_t)(base + j);  // a lane's indices only grow: ties keep the lower
      }
    }
  }
#pragma unroll
  for (int a = 0; a < kIcpPts; ++a) {
    const uint64_t key = wave_min_u64(besti[a] == 0xFFFFFFFFu ? kNoKey : nn_key(best[a], besti[a]));
    if (lane != a) continue;
    const int64_t i = first + a;
    const float d2 = __uint_as_float((uint32_t)(key >> 32));
    const bool keep = i < n_src && key != kNoKey && d2 < thr2;
    double* row = terms[wid * kIcpPts + a];
    if (i < n_src) {
      if (corr_idx) corr_idx[i] = keep ? (int32_t)(uint32_t)key : -1;
      if (corr_d2) corr_d2[i] = keep ? d2 : 0.f;
    }
    if (!keep) {
      icp_zero_terms(row);
      continue;
    }
    const int64_t c = (int64_t)(uint32_t)key;
    icp_pair_terms(pd[a][0], pd[a][1], pd[a][2], tgt[c * 3], tgt[c * 3 + 1], tgt[c * 3 + 2], tgt_normals[c * 3],
                   tgt_normals[c * 3 + 1], tgt_normals[c * 3 + 2], row);
  }
  __syncthreads();
  if (threadIdx.x < kIcpRow) {
    double s = 0.0;
    if (threadIdx.x < kIcpTerms)
      for (int p = 0; p < kIcpBlockPts; ++p) s += terms[p][threadIdx.x];
    partials[(int64_t)blockIdx.x * kIcpRow + threadIdx.x] = s;
  }
}

// x of A x = -b for the symmetric positive definite A given by its upper triangle (21 entries, row-major); false when
// a pivot is not positive or anything is not finite.
__device__ __forceinline__ bool solve_spd6(const double* __restrict__ s, double x[6]) {
  double Lm[6][6];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double a = s[j * 6 - j * (j - 1) / 2 + (i - j)];  // A[j][i], j <= i
#pragma unroll
      for (int k = 0; k < j; ++k) a -= Lm[i][k] * Lm[j][k];
      if (i == j) {
        ok = ok && a > 0.0 && isfinite(a);
        Lm[i][i] = sqrt(ok ? a : 1.0);
      } else {
        Lm[i][j] = a / Lm[j][j];
      }
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = -s[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) a -= Lm[i][k] * y[k];
    y[i] = a / Lm[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double a = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) a -= Lm[k][i] * x[k];
    x[i] = a / Lm[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && isfinite(x[i]);
  return ok;
}

__global__ void __launch_bounds__(kIcpBlock)
    k_icp_update(const double* __restrict__ partials, int32_t n_rows, int32_t n_src, int32_t round,
                 int32_t max_iterations, double rel_fitness, double rel_rmse, lnr_icp_state* __restrict__ st) {
  if (round > 0 && st->converged) return;
  __shared__ double acc[kIcpStripes][kIcpRow];
  __shared__ double tot[kIcpRow];
  const int e = threadIdx.x % kIcpRow, stripe = threadIdx.x / kIcpRow;
  double s = 0.0;
  for (int r = stripe; r < n_rows; r += kIcpStripes) s += partials[(int64_t)r * kIcpRow + e];
  acc[stripe][e] = s;
  __syncthreads();
  if (threadIdx.x < kIcpRow) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kIcpStripes; ++k) t += acc[k][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double count = tot[27], sum_d2 = tot[28];
  const double fitness = count > 0.0 ? count / (double)n_src : 0.0;
  const double rmse = count > 0.0 ? sqrt(sum_d2 / count) : 0.0;
  int iterations = round == 0 ? 0 : st->iterations;
  bool converged = false;
  if (round > 0) converged = fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse;
  st->fitness = fitness;
  st->rmse = rmse;
  st->sum_d2 = sum_d2;
  st->n_corr = (int64_t)count;
#pragma unroll
  for (int i = 0; i < 27; ++i) st->sums[i] = tot[i];
  if (!converged && iterations < max_iterations) {
    double x[6];
    if (count >= 6.0 && solve_spd6(tot, x)) {
      const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
      // Rz(x2) Ry(x1) Rx(x0) | x3..5  (Open3D's TransformVector6dToMatrix4d)
      const double M[12] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3],
                            sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4],
                            -sb,     cb * sa,                cb * ca,                x[5]};
      double T[12], N[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = st->T[i];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          N[4 * r + c] = M[4 * r] * T[c] + M[4 * r + 1] * T[4 + c] + M[4 * r + 2] * T[8 + c] + (c == 3 ? M[4 * r + 3] : 0.0);
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 12; ++i) fin = fin && isfinite(N[i]);
      if (fin) {
#pragma unroll
        for (int i = 0; i < 12; ++i) st->T[i] = N[i];
      }
    }
    ++iterations;
  }
  st->iterations = iterations;
  st->converged = converged ? 1 : 0;
}

void icp_launch_update(const double* partials, int32_t n_rows, int32_t n_src, int32_t round, int32_t max_iterations,
                       double rel_fitness, double rel_rmse, lnr_icp_state* state, hipStream_t stream) {
  hipLaunchKernelGGL(k_icp_update, dim3(1), dim3(kIcpBlock), 0, stream, partials, n_rows, n_src, round, max_iterations,
                     rel_fitness, rel_rmse, state);
}

}  // namespace lnr

using namespace lnr;

extern "C" int lnr_cloud_normals(const float* pts, int64_t n, int32_t k, float* normals, void* stream) {
  LNR_REQUIRE(pts && normals, "lnr_cloud_normals: null pointer");
  LNR_REQUIRE(k >= 3 && k <= 64, "lnr_cloud_normals: k=%d outside [3, 64]", k);
  LNR_REQUIRE(n >= 1 && n >= k && n <= kNormalsMaxN, "lnr_cloud_normals: n=%lld outside [k=%d, 2^18]", (long long)n, k);
  hipLaunchKernelGGL(k_cloud_normals, dim3((unsigned)((n + kIcpWaves - 1) / kIcpWaves)), dim3(kIcpBlock), 0,
                     as_stream(stream), pts, (int32_t)n, k, normals);
  LNR_RETURN_LAUNCH("lnr_cloud_normals");
}

static int64_t icp_rows(int64_t n_src) { return (n_src + kIcpBlockPts - 1) / kIcpBlockPts; }

extern "C" int64_t lnr_icp_workspace_bytes(int64_t n_src) {
  if (n_src < 1 || n_src > LNR_ICP_MAX_POINTS) return 0;
  return icp_rows(n_src) * kIcpRow * (int64_t)sizeof(double);
}

extern "C" int lnr_icp_init(lnr_icp_state* state, const double* T0, void* stream) {
  LNR_REQUIRE(state && T0, "lnr_icp_init: null pointer");
  lnr_icp_state init = {};
  for (int i = 0; i < 16; ++i) {
    LNR_REQUIRE(std::isfinite(T0[i]), "lnr_icp_init: T0[%d] is not finite", i);
    init.T[i] = T0[i];
  }
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(1), 0, as_stream(stream), state, init);
  LNR_RETURN_LAUNCH("lnr_icp_init");
}

extern "C" int lnr_icp_stage(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals, int64_t n_tgt,
                             float threshold, int32_t max_iterations, double rel_fitness, double rel_rmse,
                             lnr_icp_state* state, void* workspace, int64_t ws_bytes, int32_t* corr_idx,
                             float* corr_d2, void* stream) {
  LNR_REQUIRE(src && tgt && tgt_normals && state && workspace, "lnr_icp_stage: null pointer");
  LNR_REQUIRE(n_src >= 1 && n_src <= LNR_ICP_MAX_POINTS && n_tgt >= 1 && n_tgt <= LNR_ICP_MAX_POINTS,
              "lnr_icp_stage: bad sizes (n_src=%lld, n_tgt=%lld)", (long long)n_src, (long long)n_tgt);
  LNR_REQUIRE(threshold > 0.f && std::isfinite(threshold), "lnr_icp_stage: threshold must be positive and finite");
  LNR_REQUIRE(max_iterations >= 0 && max_iterations <= 1000, "lnr_icp_stage: max_iterations=%d outside [0, 1000]",
              max_iterations);
  LNR_REQUIRE(rel_fitness >= 0.0 && rel_rmse >= 0.0, "lnr_icp_stage: negative convergence criterion");
  LNR_REQUIRE(ws_bytes >= lnr_icp_workspace_bytes(n_src), "lnr_icp_stage: workspace of %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)lnr_icp_workspace_bytes(n_src));
  LNR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "lnr_icp_stage: workspace not 8-byte aligned");
  const int64_t rows = icp_rows(n_src);
  const float thr2 = (float)((double)threshold * (double)threshold);
  for (int32_t round = 0; round <= max_iterations; ++round) {
    hipLaunchKernelGGL(k_icp_correspond, dim3((unsigned)rows), dim3(kIcpBlock), 0, as_stream(stream), src,
                       (int32_t)n_src, tgt, tgt_normals, (int32_t)n_tgt, thr2, round, state,
                       static_cast<double*>(workspace), corr_idx, corr_d2);
    icp_launch_update(static_cast<const double*>(workspace), (int32_t)rows, (int32_t)n_src, round, max_iterations,
                      rel_fitness, rel_rmse, state, as_stream(stream));
  }
  LNR_RETURN_LAUNCH("lnr_icp_stage");
}
