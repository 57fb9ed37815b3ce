// Mesh sampling (analysis/compute_metrics/maps/mesh_to_pcd.py, analysis/meshing.py:122): what the reference hands to
// Open3D's sample_points_uniformly and compute_vertex_normals.
//
//   k_face_areas      one thread per face: the cross product of its edges in fp64, area = |c| / 2, normal = c / |c|
//   k_sample_points   one block per 256 consecutive points.  Point i belongs to the first face t with bounds[t] > i.
//                     Threads 0 and 255 search the whole array for the block's first and last point; if the faces
//                     between them fit kMeshStage bounds these are staged in LDS and every thread searches there,
//                     otherwise every thread searches the global array between the two.  Both searches are the same
//                     upper bound over the same values: the same face.
//   k_vertex_normals  one thread per vertex: the cross products of its incident faces, recomputed and added in fp64 in
//                     the order of its row of the caller's inverted index, then normalised.
// Integer atomics only (the status word).  Every face index is tested before the load that uses it.  All geometry is
// fp64 from the fp32 vertices, one rounding per operation (-ffp-contract=off), in the order the header states.
#include "common.hpp"

namespace lnr {

constexpr int kMeshCloudBlock = 256;
constexpr int kMeshStage = 1024;  // bounds an LDS stage holds (8 KiB)
enum : uint32_t { kStreamMesh = 7 };

struct Tri {
  double v[3][3];
  bool ok;
};

// The corners of face f widened to fp64; ok = false (and nothing loaded from verts) when an index is outside
// [0, n_verts).
__device__ __forceinline__ Tri load_tri(const float* __restrict__ verts, int64_t n_verts,
                                        const int32_t* __restrict__ faces, int64_t f) {
  Tri t;
  const int32_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  t.ok = i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts;
  const int64_t id[3] = {t.ok ? i0 : 0, t.ok ? i1 : 0, t.ok ? i2 : 0};  // vertex 0 exists: n_verts >= 1
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) t.v[k][a] = (double)verts[id[k] * 3 + a];
  return t;
}

// c = e1 x e2, e1 = v1 - v0, e2 = v2 - v0
__device__ __forceinline__ void tri_cross(const Tri& t, double (&c)[3]) {
  const double e1x = t.v[1][0] - t.v[0][0], e1y = t.v[1][1] - t.v[0][1], e1z = t.v[1][2] - t.v[0][2];
  const double e2x = t.v[2][0] - t.v[0][0], e2y = t.v[2][1] - t.v[0][1], e2z = t.v[2][2] - t.v[0][2];
  c[0] = e1y * e2z - e1z * e2y;
  c[1] = e1z * e2x - e1x * e2z;
  c[2] = e1x * e2y - e1y * e2x;
}

__device__ __forceinline__ double norm3(const double (&c)[3]) {
  return __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

// c / |c| rounded to fp32, (0, 0, 1) for |c| = 0
__device__ __forceinline__ void store_unit(float* __restrict__ out, const double (&c)[3], double len) {
  const bool z = !(len > 0.0);
  out[0] = z ? 0.f : (float)__ddiv_rn(c[0], len);
  out[1] = z ? 0.f : (float)__ddiv_rn(c[1], len);
  out[2] = z ? 1.f : (float)__ddiv_rn(c[2], len);
}

__global__ void __launch_bounds__(kMeshCloudBlock)
    k_face_areas(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces, int64_t n_faces,
                 double* __restrict__ area, float* __restrict__ normal, uint32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * kMeshCloudBlock + threadIdx.x;
  if (f >= n_faces) return;
  const Tri t = load_tri(verts, n_verts, faces, f);
  double c[3] = {0.0, 0.0, 0.0};
  if (t.ok) tri_cross(t, c);
  else atomicOr(status, LNR_MESH_BAD_INDEX);
  const double len = norm3(c);
  area[f] = 0.5 * len;
  if (normal) store_unit(normal + f * 3, c, len);
}

// The first t in [lo, hi) with b[t] > i, hi if there is none.
template <class P>
__device__ __forceinline__ int64_t upper_bound(P b, int64_t lo, int64_t hi, int64_t i) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (b[mid] > i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kMeshCloudBlock)
    k_sample_points(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                    int64_t n_faces, const int64_t* __restrict__ bounds, int64_t first, int64_t count, uint32_t key,
                    float* __restrict__ points, int32_t* __restrict__ face_of, uint32_t* __restrict__ status) {
  __shared__ int64_t s_bounds[kMeshStage];
  __shared__ int64_t s_range[2];
  const int64_t base = (int64_t)blockIdx.x * kMeshCloudBlock;  // < count
  const int64_t k = base + threadIdx.x;
  const int64_t i = first + k;
  if (threadIdx.x == 0) s_range[0] = upper_bound(bounds, 0, n_faces, first + base);
  if (threadIdx.x == kMeshCloudBlock - 1)
    s_range[1] = upper_bound(bounds, 0, n_faces, first + min(base + kMeshCloudBlock, count) - 1);
  __syncthreads();
  // the block's faces lie in [t_lo, t_hi]; t_hi = n_faces says that its last point has no face
  const int64_t t_lo = s_range[0], t_hi = max(s_range[1], t_lo);
  const int64_t n_stage = min(t_hi, n_faces - 1) - t_lo + 1;  // entries of bounds worth a look (<= 0: none)
  int64_t t;
  if (n_stage <= kMeshStage) {  // block-uniform
    for (int64_t j = threadIdx.x; j < n_stage; j += kMeshCloudBlock) s_bounds[j] = bounds[t_lo + j];
    __syncthreads();
    t = t_lo + upper_bound(s_bounds, 0, max(n_stage, (int64_t)0), i);
  } else {
    t = upper_bound(bounds, t_lo, t_lo + n_stage, i);
  }
  if (k >= count) return;
  float* out = points + k * 3;
  uint32_t bad = 0;
  Tri tri;
  tri.ok = false;
  if (t >= n_faces) bad = LNR_MESH_NO_FACE;
  else {
    tri = load_tri(verts, n_verts, faces, t);
    if (!tri.ok) bad = LNR_MESH_BAD_INDEX;
  }
  if (bad) {
    atomicOr(status, bad);
    out[0] = 0.f, out[1] = 0.f, out[2] = 0.f;
    if (face_of) face_of[k] = -1;
    return;
  }
  const double r1 = (double)rand_uniform(key, kStreamMesh, (uint32_t)i, 0);
  const double r2 = (double)rand_uniform(key, kStreamMesh, (uint32_t)i, 1);
  const double s = __dsqrt_rn(r1);
  const double a = 1.0 - s, b = s * (1.0 - r2), c = s * r2;
#pragma unroll
  for (int x = 0; x < 3; ++x) out[x] = (float)((a * tri.v[0][x] + b * tri.v[1][x]) + c * tri.v[2][x]);
  if (face_of) face_of[k] = (int32_t)t;
}

__global__ void __launch_bounds__(kMeshCloudBlock)
    k_vertex_normals(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                     int64_t n_faces, const int64_t* __restrict__ corner_perm, const int64_t* __restrict__ row_start,
                     float* __restrict__ normals, uint32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * kMeshCloudBlock + threadIdx.x;
  if (v >= n_verts) return;
  const int64_t n_corners = 3 * n_faces;
  const int64_t lo = max(row_start[v], (int64_t)0), hi = min(row_start[v + 1], n_corners);
  double sum[3] = {0.0, 0.0, 0.0};
  uint32_t bad = 0;
  for (int64_t j = lo; j < hi; ++j) {
    const int64_t corner = corner_perm[j];
    if (corner < 0 || corner >= n_corners) continue;
    const Tri t = load_tri(verts, n_verts, faces, corner / 3);
    if (!t.ok) {
      bad = LNR_MESH_BAD_INDEX;
      continue;
    }
    double c[3];
    tri_cross(t, c);
    sum[0] += c[0], sum[1] += c[1], sum[2] += c[2];
  }
  if (bad) atomicOr(status, bad);
  store_unit(normals + v * 3, sum, norm3(sum));
}

}  // namespace lnr

using namespace lnr;

static int mesh_check(const char* who, const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                      const uint32_t* status) {
  LNR_REQUIRE(verts && faces && status, "%s: null pointer", who);
  LNR_REQUIRE(n_verts >= 1 && n_verts < ((int64_t)1 << 31), "%s: n_verts=%lld outside [1, 2^31)", who,
              (long long)n_verts);
  LNR_REQUIRE(n_faces >= 1 && n_faces <= LNR_CLOUD_MAX_POINTS, "%s: n_faces=%lld outside [1, %d]", who,
              (long long)n_faces, LNR_CLOUD_MAX_POINTS);
  return LNR_OK;
}

static dim3 mesh_grid(int64_t n) { return dim3((unsigned)((n + kMeshCloudBlock - 1) / kMeshCloudBlock)); }

extern "C" int lnr_mesh_face_areas(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                   double* area, float* normal, uint32_t* status, void* stream) {
  if (int e = mesh_check("lnr_mesh_face_areas", verts, n_verts, faces, n_faces, status)) return e;
  LNR_REQUIRE(area != nullptr, "lnr_mesh_face_areas: null area");
  hipLaunchKernelGGL(k_face_areas, mesh_grid(n_faces), dim3(kMeshCloudBlock), 0, as_stream(stream), verts, n_verts,
                     faces, n_faces, area, normal, status);
  LNR_RETURN_LAUNCH("lnr_mesh_face_areas");
}

extern "C" int lnr_mesh_sample_points(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                      const int64_t* bounds, int64_t first, int64_t count, uint32_t key, float* points,
                                      int32_t* face_of, uint32_t* status, void* stream) {
  if (int e = mesh_check("lnr_mesh_sample_points", verts, n_verts, faces, n_faces, status)) return e;
  LNR_REQUIRE(bounds != nullptr, "lnr_mesh_sample_points: null bounds");
  LNR_REQUIRE(first >= 0 && count >= 0 && first <= LNR_CLOUD_MAX_POINTS && count <= LNR_CLOUD_MAX_POINTS - first,
              "lnr_mesh_sample_points: first=%lld, count=%lld outside 0 <= first, 0 <= count, first + count <= %d",
              (long long)first, (long long)count, LNR_CLOUD_MAX_POINTS);
  if (count == 0) return LNR_OK;
  LNR_REQUIRE(points != nullptr, "lnr_mesh_sample_points: null points");
  hipLaunchKernelGGL(k_sample_points, mesh_grid(count), dim3(kMeshCloudBlock), 0, as_stream(stream), verts, n_verts,
                     faces, n_faces, bounds, first, count, key, points, face_of, status);
  LNR_RETURN_LAUNCH("lnr_mesh_sample_points");
}

extern "C" int lnr_mesh_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                       const int64_t* corner_perm, const int64_t* row_start, float* normals,
                                       uint32_t* status, void* stream) {
  if (int e = mesh_check("lnr_mesh_vertex_normals", verts, n_verts, faces, n_faces, status)) return e;
  LNR_REQUIRE(corner_perm && row_start && normals, "lnr_mesh_vertex_normals: null pointer");
  hipLaunchKernelGGL(k_vertex_normals, mesh_grid(n_verts), dim3(kMeshCloudBlock), 0, as_stream(stream), verts,
                     n_verts, faces, n_faces, corner_perm, row_start, normals, status);
  LNR_RETURN_LAUNCH("lnr_mesh_vertex_normals");
}
