// Mesh extraction (analysis/mesher.py): the weight volume's scatter-max and indexed marching cubes.
//
//   k_splat_max   one thread per ray sample: point = o + d z (fp32), torch.bucketize against the float64 boundaries
//                 of each axis, atomic max of the weight's bit pattern into the volume (mesher.py:139-180)
//   k_mc_count    one thread per voxel: the crossed grid edges it owns (those leaving it in +x, +y, +z) and the
//                 triangles of the cell whose lower corner it is
//   k_mc_emit     one thread per voxel: its vertices, then its cell's triangles with vertex ids looked up through the
//                 scanned counts
// Conventions of the table, the ownership and the orders: loner_amd/mc_table.py, loner_amd/meshing.py.
#include "common.hpp"
#include "mc_table.hpp"

namespace lnr {

constexpr int kMeshBlock = 256;

// torch.bucketize(v, b, right=False): the first i with b[i] >= v, for b[0] <= v <= b[n - 1].  An arithmetic guess on
// the (near-uniform) boundaries, then corrected against them: the result is the binary search's.
__device__ __forceinline__ int bucket_of(const double* __restrict__ b, int n, double b0, double bl, double v) {
  float t = (float)(v - b0) * ((float)(n - 1) / (float)(bl - b0));
  t = fminf(fmaxf(ceilf(t), 0.f), (float)(n - 1));  // fmaxf drops the nan of a one-point or zero-width axis
  int i = (int)t;
  while (i > 0 && b[i - 1] >= v) --i;
  while (i < n - 1 && b[i] < v) ++i;
  return i;
}

__global__ void __launch_bounds__(kMeshBlock)
    k_splat_max(const float* __restrict__ rays, const float* __restrict__ z, const float* __restrict__ weights,
                const float* __restrict__ depth, const float* __restrict__ variance, int64_t n, int32_t S,
                const double* __restrict__ bx, int nx, const double* __restrict__ by, int ny,
                const double* __restrict__ bz, int nz, float depth_max, float var_max, int* __restrict__ volume) {
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= n) return;
  const float w = weights[i];
  if (!(w > 0.f)) return;  // weight 0 cannot raise a cell (nor can a nan: it never enters the volume)
  const int64_t r = i / S;
  if (!(depth[r] < depth_max)) return;
  if (var_max > 0.f && !(variance[r] < var_max)) return;
  const float* ray = rays + r * 13;
  const float zi = z[i];
  const double px = (double)(ray[0] + ray[3] * zi), py = (double)(ray[1] + ray[4] * zi),
               pz = (double)(ray[2] + ray[5] * zi);
  const double x0 = bx[0], x1 = bx[nx - 1], y0 = by[0], y1 = by[ny - 1], z0 = bz[0], z1 = bz[nz - 1];
  if (!(px >= x0 && px <= x1 && py >= y0 && py <= y1 && pz >= z0 && pz <= z1)) return;
  const int64_t cell = (int64_t)bucket_of(bx, nx, x0, x1, px) * nz + (int64_t)bucket_of(by, ny, y0, y1, py) * nx * nz +
                       bucket_of(bz, nz, z0, z1, pz);
  if (cell >= (int64_t)nx * ny * nz) return;  // the reference's "bucketize edge cases" (mesher.py:176)
  const int bits = __float_as_int(w);  // non-negative floats order like their bit patterns
  // cells only grow: a cell already at or above w needs no atomic
  if (__hip_atomic_load(volume + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= bits) return;
  atomicMax(volume + cell, bits);
}

struct McGrid {
  int nx, ny, nz;
  float level;
};

// Bit c = dx + 2 dy + 4 dz of the case: corner (ix + dx, iy + dy, iz + dz) is inside (value > level).
__device__ __forceinline__ int mc_case(const float* __restrict__ vol, const McGrid g, int64_t i) {
  const int64_t sx = (int64_t)g.ny * g.nz, sy = g.nz;
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) c |= (vol[i + (k & 1) * sx + ((k >> 1) & 1) * sy + (k >> 2)] > g.level) << k;
  return c;
}

__global__ void __launch_bounds__(kMeshBlock)
    k_mc_count(const float* __restrict__ vol, McGrid g, int64_t n, int32_t* __restrict__ vert_count,
               int32_t* __restrict__ tri_count) {
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= n) return;
  const int iz = (int)(i % g.nz), iy = (int)((i / g.nz) % g.ny), ix = (int)(i / ((int64_t)g.nz * g.ny));
  const bool hx = ix + 1 < g.nx, hy = iy + 1 < g.ny, hz = iz + 1 < g.nz;
  const bool in0 = vol[i] > g.level;
  int nv = 0;
  if (hx) nv += (vol[i + (int64_t)g.ny * g.nz] > g.level) != in0;
  if (hy) nv += (vol[i + g.nz] > g.level) != in0;
  if (hz) nv += (vol[i + 1] > g.level) != in0;
  vert_count[i] = nv;
  tri_count[i] = (hx && hy && hz) ? kMcTriCount[mc_case(vol, g, i)] : 0;
}

// The crossed-edge flags (bit a: the edge leaving voxel (ix, iy, iz) along axis a) of a voxel.
__device__ __forceinline__ int mc_owned(const float* __restrict__ vol, const McGrid g, int64_t i, int ix, int iy,
                                        int iz, float f0) {
  const bool in0 = f0 > g.level;
  int m = 0;
  if (ix + 1 < g.nx) m |= (int)((vol[i + (int64_t)g.ny * g.nz] > g.level) != in0);
  if (iy + 1 < g.ny) m |= (int)((vol[i + g.nz] > g.level) != in0) << 1;
  if (iz + 1 < g.nz) m |= (int)((vol[i + 1] > g.level) != in0) << 2;
  return m;
}

__global__ void __launch_bounds__(kMeshBlock)
    k_mc_emit(const float* __restrict__ vol, McGrid g, int64_t n, float sx, float sy, float sz,
              const int64_t* __restrict__ vert_offset, const int64_t* __restrict__ tri_offset, int64_t n_verts,
              int64_t n_faces, float* __restrict__ verts, int32_t* __restrict__ faces) {
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= n) return;
  const int iz = (int)(i % g.nz), iy = (int)((i / g.nz) % g.ny), ix = (int)(i / ((int64_t)g.nz * g.ny));
  const int64_t stride[3] = {(int64_t)g.ny * g.nz, g.nz, 1};
  const float f0 = vol[i];
  const int own = mc_owned(vol, g, i, ix, iy, iz, f0);
  if (own) {
    const float p[3] = {(float)ix * sx, (float)iy * sy, (float)iz * sz};
    const float sp[3] = {sx, sy, sz};
    int64_t v = vert_offset[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((own >> a) & 1)) continue;
      const float f1 = vol[i + stride[a]];
      const float t = (g.level - f0) / (f1 - f0);
      if (v < n_verts) {  // holds when the offsets are the scan of this volume's counts
        float* o = verts + v * 3;
        o[0] = p[0], o[1] = p[1], o[2] = p[2];
        o[a] = p[a] + t * sp[a];
      }
      ++v;
    }
  }
  if (!(ix + 1 < g.nx && iy + 1 < g.ny && iz + 1 < g.nz)) return;
  const int c = mc_case(vol, g, i);
  const int nt = kMcTriCount[c];
  if (nt == 0) return;
  const int64_t f = tri_offset[i];
  for (int k = 0; k < 3 * nt; ++k) {
    const int e = kMcTriTable[c][k];
    const int axis = e >> 2, j = e & 3;
    // the voxel that owns edge e: the two other axes, in increasing order, take the bits of j
    const int dx = axis == 0 ? 0 : (j & 1), dy = axis == 1 ? 0 : (axis == 0 ? (j & 1) : (j >> 1)),
              dz = axis == 2 ? 0 : (j >> 1);
    const int64_t o = i + dx * stride[0] + dy * stride[1] + dz;
    const int m = mc_owned(vol, g, o, ix + dx, iy + dy, iz + dz, vol[o]);
    const int64_t id = vert_offset[o] + __popc(m & ((1 << axis) - 1));
    if (f + k / 3 < n_faces) faces[f * 3 + k] = (int32_t)id;
  }
}

}  // namespace lnr

using namespace lnr;

extern "C" int lnr_volume_splat_max(const float* rays, const float* z, const float* weights, const float* depth,
                                    const float* variance, int64_t n_rays, int32_t n_samples, const double* bx,
                                    int32_t nx, const double* by, int32_t ny, const double* bz, int32_t nz,
                                    float depth_max, float var_max, float* volume, void* stream) {
  LNR_REQUIRE(rays && z && weights && depth && bx && by && bz && volume, "lnr_volume_splat_max: null pointer");
  LNR_REQUIRE(var_max <= 0.f || variance, "lnr_volume_splat_max: var_max > 0 needs variance");
  LNR_REQUIRE(n_rays >= 0 && n_samples >= 1, "lnr_volume_splat_max: bad sizes (n_rays=%lld, n_samples=%d)",
              (long long)n_rays, n_samples);
  LNR_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "lnr_volume_splat_max: bad grid %d x %d x %d", nx, ny, nz);
  const int64_t n = n_rays * n_samples;
  LNR_REQUIRE(n < ((int64_t)1 << 31) * kMeshBlock, "lnr_volume_splat_max: too many samples for one launch");
  if (n == 0) return LNR_OK;
  hipLaunchKernelGGL(k_splat_max, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0,
                     as_stream(stream), rays, z, weights, depth, variance, n, n_samples, bx, nx, by, ny, bz, nz,
                     depth_max, var_max, reinterpret_cast<int*>(volume));
  LNR_RETURN_LAUNCH("lnr_volume_splat_max");
}

static int mc_check(const char* who, const float* volume, int32_t nx, int32_t ny, int32_t nz, int64_t* n) {
  LNR_REQUIRE(volume != nullptr, "%s: null volume", who);
  LNR_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: bad grid %d x %d x %d", who, nx, ny, nz);
  *n = (int64_t)nx * ny * nz;
  LNR_REQUIRE(*n < ((int64_t)1 << 31) * kMeshBlock, "%s: grid too large for one launch", who);
  return LNR_OK;
}

extern "C" int lnr_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level,
                                        int32_t* vert_count, int32_t* tri_count, void* stream) {
  int64_t n;
  if (int e = mc_check("lnr_marching_cubes_count", volume, nx, ny, nz, &n)) return e;
  LNR_REQUIRE(vert_count && tri_count, "lnr_marching_cubes_count: null output");
  hipLaunchKernelGGL(k_mc_count, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0,
                     as_stream(stream), volume, McGrid{nx, ny, nz, level}, n, vert_count, tri_count);
  LNR_RETURN_LAUNCH("lnr_marching_cubes_count");
}

extern "C" int lnr_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, float sx,
                                       float sy, float sz, const int64_t* vert_offset, const int64_t* tri_offset,
                                       int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, void* stream) {
  int64_t n;
  if (int e = mc_check("lnr_marching_cubes_emit", volume, nx, ny, nz, &n)) return e;
  LNR_REQUIRE(vert_offset && tri_offset, "lnr_marching_cubes_emit: null offsets");
  LNR_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_verts < ((int64_t)1 << 31),
              "lnr_marching_cubes_emit: bad sizes (n_verts=%lld, n_faces=%lld)", (long long)n_verts,
              (long long)n_faces);
  LNR_REQUIRE((verts || n_verts == 0) && (faces || n_faces == 0), "lnr_marching_cubes_emit: null output");
  if (n_verts == 0 && n_faces == 0) return LNR_OK;
  hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0,
                     as_stream(stream), volume, McGrid{nx, ny, nz, level}, n, sx, sy, sz, vert_offset, tri_offset,
                     n_verts, n_faces, verts, faces);
  LNR_RETURN_LAUNCH("lnr_marching_cubes_emit");
}
