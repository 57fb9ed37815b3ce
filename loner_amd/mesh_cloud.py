"""A triangle mesh as a point cloud, and its vertex normals, on the GPU (the reference's
analysis/compute_metrics/maps/mesh_to_pcd.py and the compute_vertex_normals of analysis/meshing.py:122, without Open3D).

    face_areas               lnr_mesh_face_areas: area (F,) float64 and, on request, unit normals (F, 3) float32
    sample_bounds            Open3D's allocation of N points to the faces: bounds[t] = floor(cum[t] / cum[-1] N + 0.5),
                             cum = torch.cumsum(area) in float64; face t owns the points [bounds[t - 1], bounds[t])
    sample_points_uniformly  Open3D's sample_points_uniformly: areas, bounds, lnr_mesh_sample_points
    vertex_normals           Open3D's compute_vertex_normals: a stable sort of the corners by vertex, the rows' starts,
                             lnr_mesh_vertex_normals
    mesh_to_cloud            mesh_to_pcd.py: sample_points_uniformly, then map_eval.voxel_down_sample
    evaluate_mesh            mesh_to_cloud, then map_eval.compare_point_clouds against a ground-truth cloud
    face_areas_ref, sample_bounds_ref, sample_points_ref, vertex_normals_ref
                             float64 numpy restatements with the kernels' operation order: the tests' oracle (validated
                             on their own in tests/test_mesh_cloud_ref.py) and what a host without a GPU runs

Every public GPU call reads the status word back once, at its end; a face index outside [0, n_verts) raises
RuntimeError there.

Deviations from the reference:
  * the draws are the project's counter generator (stream 7), not Open3D's std::mt19937: point i depends on (key, i)
    alone, so a run repeats bit for bit and a chunked run equals the whole one;
  * points are float32 (Open3D holds float64), computed in float64 and rounded once;
  * at most 2^27 points and faces (the voxel filter's limit; the reference's 5 10^7 fit).
"""
import numpy as np
import torch

from . import _lib as L

STREAM_MESH = 7  # kStreamMesh (csrc/mesh_cloud.hip); 1 to 6 are the samplers' and the ray selection's


# ---------------------------------------------------------------------------------------------- numpy restatements
def _mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def rand_u32(key, stream, a, b):
    """The counter generator of csrc/common.hpp on uint64 arrays holding uint32 values."""
    m = np.uint64(0xFFFFFFFF)
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    h = _mix32((np.uint64(key) & m) ^ ((np.uint64(stream) * np.uint64(0x9E3779B9)) & m))
    h = _mix32(h ^ a)
    return _mix32(h ^ ((b * np.uint64(0x85EBCA6B) + np.uint64(0x632BE5AB)) & m))


def rand_uniform(key, stream, a, b):
    """rand_uniform of csrc/common.hpp: the top 24 bits times 2^-24, float32."""
    return ((rand_u32(key, stream, a, b) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _mesh_ref(verts, faces):
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    return v, f, ((f >= 0) & (f < len(v))).all(axis=1)


def _cross_ref(v, f, ok):
    """The faces' unnormalised cross products in the kernels' operation order; zero for a face with a bad index."""
    g = np.where(ok[:, None], f, 0)
    v0, v1, v2 = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    c = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), axis=1)
    return np.where(ok[:, None], c, 0.0)


def _unit_ref(c):
    """c / |c| with |c| = sqrt((x^2 + y^2) + z^2), rounded to float32; (0, 0, 1) for |c| = 0.  Returns (unit, |c|)."""
    n = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    with np.errstate(all="ignore"):
        u = (c / n[:, None]).astype(np.float32)
    u[~(n > 0)] = (0.0, 0.0, 1.0)
    return u, n


def face_areas_ref(verts, faces, return_normals=False):
    """``lnr_mesh_face_areas`` in float64 numpy: area (F,) float64[, normals (F, 3) float32]."""
    v, f, ok = _mesh_ref(verts, faces)
    unit, n = _unit_ref(_cross_ref(v, f, ok))
    return (0.5 * n, unit) if return_normals else 0.5 * n


def sample_bounds_ref(area_or_cum, n, cum=None):
    """bounds[t] = int64(floor(cum[t] / cum[-1] * n + 0.5)); ``cum`` given: that scan (the device's, say) instead of
    numpy's sequential cumsum of the areas."""
    cum = np.cumsum(np.asarray(area_or_cum, np.float64)) if cum is None else np.asarray(cum, np.float64)
    return np.floor(cum / cum[-1] * float(n) + 0.5).astype(np.int64)


def sample_points_ref(verts, faces, bounds, key=0, first=0, count=None, return_weights=False):
    """``lnr_mesh_sample_points`` in float64 numpy: (points (count, 3) float32, face_of (count,) int32[, the
    barycentric weights (count, 3) float64]).  ``count=None``: up to bounds[-1]."""
    v, f, ok = _mesh_ref(verts, faces)
    bounds = np.asarray(bounds, np.int64)
    count = int(bounds[-1]) - first if count is None else int(count)
    i = np.arange(first, first + count, dtype=np.int64)
    t = np.searchsorted(bounds, i, side="right")  # the first face with bounds[t] > i
    good = t < len(f)
    good[good] = ok[t[good]]
    tg = np.where(good, t, 0)
    g = np.where(good[:, None], f[tg], 0)
    r1 = rand_uniform(key, STREAM_MESH, i, 0).astype(np.float64)
    r2 = rand_uniform(key, STREAM_MESH, i, 1).astype(np.float64)
    s = np.sqrt(r1)
    a, b, c = 1.0 - s, s * (1.0 - r2), s * r2
    p = ((a[:, None] * v[g[:, 0]] + b[:, None] * v[g[:, 1]]) + c[:, None] * v[g[:, 2]]).astype(np.float32)
    p[~good] = 0.0
    face_of = np.where(good, t, -1).astype(np.int32)
    return (p, face_of, np.stack((a, b, c), axis=1)) if return_weights else (p, face_of)


def vertex_rows_ref(faces, n_verts):
    """The inverted index of ``vertex_normals``: (corner_perm, row_start); corners with a bad index go past the last
    row."""
    flat = np.asarray(faces).reshape(-1).astype(np.int64)
    keys = np.where((flat >= 0) & (flat < n_verts), flat, n_verts)
    perm = np.argsort(keys, kind="stable")
    return perm, np.searchsorted(keys[perm], np.arange(n_verts + 1), side="left")


def vertex_normals_ref(verts, faces):
    """``lnr_mesh_vertex_normals`` in float64 numpy: every vertex adds its incident faces' cross products in the order
    of its row (ascending corner index), then normalises; (n_verts, 3) float32."""
    v, f, ok = _mesh_ref(verts, faces)
    c = _cross_ref(v, f, ok)
    perm, start = vertex_rows_ref(f, len(v))
    length = start[1:] - start[:-1]
    total = np.zeros((len(v), 3), np.float64)
    for k in range(int(length.max()) if len(length) else 0):
        rows = np.nonzero(length > k)[0]
        total[rows] += c[perm[start[rows] + k] // 3]
    return _unit_ref(total)[0]


# ---------------------------------------------------------------------------------------------- GPU
def _mesh(verts, faces, what):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32 (n_verts, 3) vertices")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: expected int32 (n_faces, 3) faces")
    if verts.shape[0] < 1 or faces.shape[0] < 1:
        raise ValueError(f"{what}: an empty mesh")
    return verts.contiguous(), faces.contiguous()


def _status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _raise_status(status, what):
    bits = int(status.item())
    if bits & L.MESH_BAD_INDEX:
        raise RuntimeError(f"{what}: a face index is outside [0, n_verts)")
    if bits & L.MESH_NO_FACE:
        raise RuntimeError(f"{what}: a point index has no face (bounds end early, or the mesh has no area)")


def _face_areas(v, f, status, normals=None):
    area = torch.empty(f.shape[0], dtype=torch.float64, device=v.device)
    L.call("lnr_mesh_face_areas", v, v.shape[0], f, f.shape[0], area, normals, status, L.stream(v.device))
    return area


def face_areas(verts, faces, return_normals=False):
    """Area (F,) float64 of every face[, and its unit normal (F, 3) float32, (0, 0, 1) for a face without area]."""
    v, f = _mesh(verts, faces, "face_areas")
    status = _status(v.device)
    normals = torch.empty(f.shape[0], 3, dtype=torch.float32, device=v.device) if return_normals else None
    area = _face_areas(v, f, status, normals)
    _raise_status(status, "face_areas")
    return (area, normals) if return_normals else area


def sample_bounds(area, n):
    """bounds (F,) int64 on the device from the areas (F,) float64; no host read."""
    cum = torch.cumsum(area, 0)
    return torch.floor(cum / cum[-1] * float(n) + 0.5).to(torch.int64)


def _sample(v, f, bounds, first, count, key, status, return_faces):
    points = torch.empty(count, 3, dtype=torch.float32, device=v.device)
    face_of = torch.empty(count, dtype=torch.int32, device=v.device) if return_faces else None
    L.call("lnr_mesh_sample_points", v, v.shape[0], f, f.shape[0], bounds, first, count, int(key) & 0xFFFFFFFF, points,
           face_of, status, L.stream(v.device))
    return points, face_of


def sample_points_uniformly(verts, faces, number_of_points, key=0, return_faces=False, first=0, count=None):
    """Open3D's sample_points_uniformly on a device mesh: points (count, 3) float32[, face_of (count,) int32], the
    points ``first .. first + count`` of the ``number_of_points`` the mesh gets (default: all of them)."""
    v, f = _mesh(verts, faces, "sample_points_uniformly")
    n, first = int(number_of_points), int(first)
    count = n - first if count is None else int(count)
    if not (1 <= n <= L.CLOUD_MAX_POINTS and 0 <= first and 0 <= count and first + count <= n):
        raise ValueError(f"sample_points_uniformly: number_of_points={n}, first={first}, count={count} outside "
                         f"1 <= number_of_points <= 2^27, 0 <= first, first + count <= number_of_points")
    status = _status(v.device)
    bounds = sample_bounds(_face_areas(v, f, status), n)
    points, face_of = _sample(v, f, bounds, first, count, key, status, return_faces)
    _raise_status(status, "sample_points_uniformly")
    return (points, face_of) if return_faces else points


def vertex_rows(faces, n_verts):
    """The inverted index lnr_mesh_vertex_normals reads: corner_perm (3F,) int64, the stable argsort of the corners by
    vertex, and row_start (n_verts + 1,) int64, the exclusive scan of the vertices' corner counts (read off the sorted
    keys by a search, which needs no host read).  Corners with a bad index sort past the last row."""
    flat = faces.reshape(-1).to(torch.int64)
    keys = torch.where((flat >= 0) & (flat < n_verts), flat, n_verts)
    skeys, perm = torch.sort(keys, stable=True)
    return perm, torch.searchsorted(skeys, torch.arange(n_verts + 1, dtype=torch.int64, device=faces.device))


def vertex_normals(verts, faces):
    """Open3D's compute_vertex_normals on a device mesh: (n_verts, 3) float32 unit normals, area-weighted; (0, 0, 1)
    for a vertex no face with area touches."""
    v, f = _mesh(verts, faces, "vertex_normals")
    status = _status(v.device)
    perm, row_start = vertex_rows(f, v.shape[0])
    normals = torch.empty(v.shape[0], 3, dtype=torch.float32, device=v.device)
    L.call("lnr_mesh_vertex_normals", v, v.shape[0], f, f.shape[0], perm, row_start, normals, status,
           L.stream(v.device))
    _raise_status(status, "vertex_normals")
    return normals


def mesh_to_cloud(verts, faces, resolution, number_of_points=50_000_000, key=0):
    """mesh_to_pcd.py: ``number_of_points`` uniform samples of the mesh, voxel-filtered at ``resolution``."""
    from .map_eval import voxel_down_sample
    return voxel_down_sample(sample_points_uniformly(verts, faces, number_of_points, key), resolution)


def evaluate_mesh(verts, faces, gt, f_score_threshold=0.1, voxel_size=0.05, number_of_points=50_000_000, **kw):
    """The map metrics of a mesh against a ground-truth device cloud: ``mesh_to_cloud`` at ``voxel_size``, then
    ``map_eval.compare_point_clouds`` (``kw``: its align, align_max_points, cell, timer, return_distances; key)."""
    from .map_eval import compare_point_clouds
    est = mesh_to_cloud(verts, faces, voxel_size, number_of_points, kw.pop("key", 0))
    return compare_point_clouds(est, gt, f_score_threshold, voxel_size, **kw)
