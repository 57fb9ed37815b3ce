"""Map evaluation on the GPU (the reference's analysis/renderer_lidar.py and analysis/evaluate_lidar_map.py, without
Open3D): render the trained map as a point cloud and compare it with a ground-truth cloud.

    voxel_down_sample        Open3D's voxel_down_sample: lnr_cloud_cell_keys, a stable sort, lnr_voxel_heads, a scan,
                             lnr_voxel_reduce (``voxel_filter`` also returns counts and keys)
    uniform_down_sample      points[::k]
    NearestGrid, nearest_distances
                             Open3D's compute_point_cloud_distance: the target sorted into a uniform grid
                             (lnr_cloud_cell_keys + sort), lnr_nn_search per query cloud
    distance_stats           {sum, count above a threshold} of a distance array (lnr_dist_stats)
    compare_point_clouds     evaluate_lidar_map.compare_point_clouds: voxel filter, 10 point-to-plane ICP iterations
                             at 0.125 m (``tracking.cloud_normals`` / ``tracking.icp``), accuracy, completion, Chamfer
                             distance, precision, recall, F-score; ``write_statistics`` writes its YAML
    LidarMapRenderer         renderer_lidar.py: a synthetic sweep from every n-th pose through ``evaluate.DepthRenderer``,
                             kept where variance and depth pass, voxel-filtered, moved to the world, merged, filtered
    write_pcd, read_pcd      PCD v0.7, x y z float32
    voxel_down_sample_ref, nearest_distances_ref, compare_point_clouds_ref
                             float64 numpy / scipy restatements: the tests' oracle (validated on their own in
                             tests/test_map_eval_ref.py) and what a host without a GPU runs

Deviations from the reference:
  * output order of the voxel filter: ascending cell key (x, then y, then z); Open3D's is that of an unordered map;
  * points are float32 (Open3D holds float64): a voxel's mean is summed in float64 and rounded once, an aligned or
    posed cloud is transformed in float64 and rounded once;
  * the alignment clouds are capped at ``align_max_points`` = 2^16 points (reference: 10^6) and at most 2^17 with the
    default exhaustive search, whose two kernels are O(n^2); ``align_search="grid"`` (the same transform bit for bit)
    takes the reference's 10^6;
  * only the target's normals are estimated: point-to-plane ICP reads no others.
"""
import os

import numpy as np
import torch

from . import _lib as L

# compare_point_clouds' search cell in voxels: the fastest of 1, 2, 4, 8 at 2^17 points a side, build included
# (tools/map_eval_demo.py, profiles/map_eval_demo.json)
DEFAULT_CELL_VOXELS = 4
ALIGN_MAX_POINTS = 1 << 17
ALIGN_MAX_POINTS_GRID = 1_000_000  # with align_search="grid": the reference's cap
ALIGN_KNN = 30


# ---------------------------------------------------------------------------------------------- numpy restatements
def cell_indices_ref(points, origin, cell):
    """lnr_cloud_cell_keys' indices: floor((float64(p) - origin) / cell), (n, 3) float64."""
    return np.floor((np.asarray(points, np.float32).astype(np.float64) - np.asarray(origin, np.float64)) / float(cell))


def cell_keys_ref(idx):
    i = np.asarray(idx).astype(np.int64)
    return (i[:, 0] << (2 * L.CLOUD_CELL_BITS)) | (i[:, 1] << L.CLOUD_CELL_BITS) | i[:, 2]


def voxel_down_sample_ref(points, voxel_size, return_counts=False, return_keys=False):
    """Open3D's voxel_down_sample in float64 numpy: origin = min - voxel / 2, one point per occupied voxel, the mean
    of its points (rounded to float32 once), in ascending key order."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise RuntimeError("voxel_down_sample: a coordinate is nan or inf")
    origin = p.min(axis=0).astype(np.float64) - float(voxel_size) / 2
    idx = cell_indices_ref(p, origin, voxel_size)
    if not ((idx >= 0) & (idx < 2 ** L.CLOUD_CELL_BITS)).all():
        raise RuntimeError("voxel_down_sample: the grid exceeds 2^21 cells on an axis")
    keys, inv, counts = np.unique(cell_keys_ref(idx), return_inverse=True, return_counts=True)
    sums = np.zeros((len(keys), 3), np.float64)
    np.add.at(sums, inv.reshape(-1), p.astype(np.float64))
    out = [(sums / counts[:, None]).astype(np.float32)]
    if return_counts:
        out.append(counts.astype(np.int32))
    if return_keys:
        out.append(keys)
    return out[0] if len(out) == 1 else tuple(out)


def nn_key_ref(src, tgt, block=256):
    """The search key of lnr_nn_search emulated in numpy: d2 = dx dx + dy dy + dz dz in float32, every operation
    rounded, the minimum by (d2, index).  Returns (idx int32, d2 float32).  O(n m)."""
    s, t = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    idx = np.empty(len(s), np.int32)
    d2 = np.empty(len(s), np.float32)
    for a in range(0, len(s), block):
        d = s[a:a + block, None, :] - t[None, :, :]
        d *= d
        k = (d[..., 0] + d[..., 1]) + d[..., 2]
        j = np.argmin(k, axis=1)  # the first of equal minima: the lower index
        idx[a:a + block] = j
        d2[a:a + block] = k[np.arange(len(j)), j]
    return idx, d2


def nearest_distances_ref(src, tgt, fp32_key=False):
    """compute_point_cloud_distance in float64: (dist, idx) of each source point's nearest target by a k-d tree.  With
    ``fp32_key`` the winner is chosen as the kernel chooses it (``nn_key_ref``) and (dist, idx, d2) is returned, dist
    being the float64 distance to that winner."""
    s, t = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    if not fp32_key:
        from scipy.spatial import cKDTree
        dist, idx = cKDTree(t).query(s, k=1)
        return dist, idx.astype(np.int32)
    idx, d2 = nn_key_ref(src, tgt)
    return np.sqrt(((s - t[idx]) ** 2).sum(axis=1)), idx, d2


def transform_points_ref(points, T):
    """T (4, 4) applied to float32 points in float64, term by term, rounded to float32 once."""
    p = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    q = p[:, 0:1] * T[:3, 0] + p[:, 1:2] * T[:3, 1] + p[:, 2:3] * T[:3, 2] + T[:3, 3]
    return q.astype(np.float32)


def alignment_skip(n, cap):
    return n // cap if n > cap else 1


def statistics(sum_acc, n_acc, false_pos, sum_comp, n_comp, false_neg):
    """The reference's dict from the two sums and the two counts above the threshold (recall = TP / (TP + FN) with TP
    taken from accuracy, and the + 1e-8, as written there)."""
    accuracy, completion = sum_acc / n_acc, sum_comp / n_comp
    tp = n_acc - false_pos
    precision = tp / (tp + false_pos)
    recall = tp / (tp + false_neg) if tp + false_neg else 0.0
    return {"accuracy": float(accuracy), "completion": float(completion),
            "chamfer_distance": float(accuracy + completion), "recall": float(recall), "precision": float(precision),
            "f-score": float(2 * (precision * recall) / (precision + recall + 1e-8)), "num_points": int(n_acc)}


def _check_align_cap(cap, search="brute"):
    if search not in ("brute", "grid"):
        raise ValueError(f"align_search={search!r} is not one of ('brute', 'grid')")
    if search == "grid":
        if not 1 <= int(cap) <= ALIGN_MAX_POINTS_GRID:
            raise ValueError(f"align_max_points={cap} outside [1, {ALIGN_MAX_POINTS_GRID}] (align_search='grid')")
    elif not 1 <= int(cap) <= ALIGN_MAX_POINTS:
        raise ValueError(f"align_max_points={cap} outside [1, 2^17]")


def compare_point_clouds_ref(est, gt, f_score_threshold=0.1, voxel_size=0.05, align=True, align_max_points=1 << 16,
                             return_distances=False, align_search="brute"):
    """compare_point_clouds in float64 numpy / scipy, on ``tracking.normals_reference`` / ``icp_reference``.
    ``align_search`` only sets the cap ``align_max_points`` is checked against."""
    from . import tracking as TR
    _check_align_cap(align_max_points, align_search)
    e, g = voxel_down_sample_ref(est, voxel_size), voxel_down_sample_ref(gt, voxel_size)
    T = np.eye(4)
    if align:
        ae, ag = e[::alignment_skip(len(e), align_max_points)], g[::alignment_skip(len(g), align_max_points)]
        T = TR.icp_reference(ae, ag, TR.normals_reference(ag, ALIGN_KNN), 0.125, 10, 1e-12, 1e-12)["T"]
        e = transform_points_ref(e, T)
    acc, _ = nearest_distances_ref(e, g)
    comp, _ = nearest_distances_ref(g, e)
    stats = statistics(acc.sum(), len(acc), int((acc > f_score_threshold).sum()), comp.sum(), len(comp),
                       int((comp > f_score_threshold).sum()))
    return (stats, acc, comp, T) if return_distances else stats


# ---------------------------------------------------------------------------------------------- files
def write_statistics(stats, output_dir, id_str=None):
    """``<output_dir>/metrics/statistics{_id}.yaml``: the flat dict as YAML, keys sorted (yaml.dump's layout)."""
    d = os.path.join(output_dir, "metrics")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"statistics{'_' + str(id_str) if id_str is not None else ''}.yaml")
    with open(path, "w") as f:
        for k in sorted(stats):
            f.write(f"{k}: {stats[k]!r}\n")
    return path


def write_pcd(path, points):
    """Binary PCD v0.7 with fields x y z, float32."""
    p = np.ascontiguousarray(torch.as_tensor(points).detach().cpu().numpy(), "<f4").reshape(-1, 3)
    header = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\n"
              f"COUNT 1 1 1\nWIDTH {len(p)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(p)}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(p.tobytes())


def read_pcd(path):
    """x, y, z of a PCD v0.7 file (DATA binary or ascii; x y z must be 4-byte floats) as (n, 3) float32."""
    with open(path, "rb") as f:
        raw = f.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if line and not line.startswith("#"):
            k, *v = line.split()
            head[k] = v
            if k == "DATA":
                break
    fields, sizes, types = head["FIELDS"], [int(s) for s in head["SIZE"]], head["TYPE"]
    counts = [int(c) for c in head.get("COUNT", ["1"] * len(fields))]
    n = int(head["POINTS"][0])
    cols = [fields.index(a) for a in "xyz"]
    if any(sizes[c] != 4 or types[c] != "F" or counts[c] != 1 for c in cols):
        raise ValueError("read_pcd: x y z must be float32")
    if head["DATA"][0] == "ascii":
        start = np.cumsum([0] + counts)
        rows = np.array([ln.split() for ln in raw[pos:].decode("ascii").splitlines() if ln.strip()][:n], dtype=object)
        return np.stack([rows[:, start[c]].astype(np.float32) for c in cols], axis=1)
    if head["DATA"][0] != "binary":
        raise ValueError(f"read_pcd: DATA {head['DATA'][0]} is not supported")
    offs = np.cumsum([0] + [s * c for s, c in zip(sizes, counts)])
    rec = np.frombuffer(raw, np.uint8, n * int(offs[-1]), pos).reshape(n, int(offs[-1]))
    return np.stack([rec[:, offs[c]:offs[c] + 4].copy().view("<f4")[:, 0] for c in cols], axis=1).astype(np.float32)


def scan_world_points(scans, stride=1):
    """The world points of synthetic scans (dicts of directions (3, P), distances (P,), pose (4, 4)): every
    ``stride``-th point of each, float32 (n, 3) on the CPU."""
    out = []
    for s in scans:
        p = (s["directions"][:, ::stride] * s["distances"][::stride]).t().double()
        T = torch.as_tensor(s["pose"]).double()
        out.append((p @ T[:3, :3].t() + T[:3, 3]).float())
    return torch.cat(out).contiguous()


# ---------------------------------------------------------------------------------------------- GPU
def _cloud(points, what):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or \
            points.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 (n, 3) tensor")
    if points.shape[0] < 1:
        raise ValueError(f"{what}: an empty cloud")
    return points.contiguous()


def _raise_status(bits, what):
    if bits & L.CLOUD_NONFINITE:
        raise RuntimeError(f"{what}: a coordinate is nan or inf")
    if bits & L.CLOUD_GRID_RANGE:
        raise RuntimeError(f"{what}: the grid exceeds 2^21 cells on an axis")


def _cell_keys(pts, origin, cell, status):
    keys = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    L.call("lnr_cloud_cell_keys", pts, pts.shape[0], origin, float(cell), keys, status, L.stream(pts.device))
    return keys


def voxel_filter(points, voxel_size, return_keys=False):
    """The voxel filter of a device cloud: (means (m, 3) float32, counts (m,) int32[, keys (m,) int64]) in ascending
    key order.  One host read (the voxel count and the status word) sizes the outputs; non-finite input and a grid
    over 2^21 cells per axis raise RuntimeError there."""
    pts = _cloud(points, "voxel_down_sample")
    dev, n = pts.device, pts.shape[0]
    s = L.stream(dev)
    origin = pts.min(dim=0).values.double() - float(voxel_size) / 2
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    skeys, perm = torch.sort(_cell_keys(pts, origin, voxel_size, status), stable=True)
    heads = torch.empty(n, dtype=torch.int32, device=dev)
    L.call("lnr_voxel_heads", skeys, n, heads, s)
    scan = torch.cumsum(heads, 0)  # int64
    n_vox, bits = torch.stack((scan[-1], status[0].to(torch.int64))).tolist()
    _raise_status(bits, "voxel_down_sample")
    ws = torch.empty(int(L.lib().lnr_voxel_workspace_bytes(n, n_vox)) // 8, dtype=torch.float64, device=dev)
    means = torch.empty(n_vox, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(n_vox, dtype=torch.int32, device=dev)
    L.call("lnr_voxel_reduce", pts, perm, scan, n, n_vox, ws, ws.numel() * 8, means, counts, s)
    return (means, counts, skeys[heads.bool()]) if return_keys else (means, counts)


def voxel_down_sample(points, voxel_size, return_counts=False):
    """Open3D's voxel_down_sample of a float32 (n, 3) device cloud; see ``voxel_filter``."""
    means, counts = voxel_filter(points, voxel_size)
    return (means, counts) if return_counts else means


def uniform_down_sample(points, k):
    """Open3D's uniform_down_sample: every k-th point."""
    return points[::int(k)]


def default_cell(lo, hi, n):
    """A search cell for a surface cloud of n points in the box [lo, hi]: about two points per occupied cell, and no
    more than 2^20 cells on an axis."""
    e = [max(float(b) - float(a), 0.0) for a, b in zip(lo, hi)]
    area = e[0] * e[1] + e[1] * e[2] + e[0] * e[2]
    cell = (2.0 * area / n) ** 0.5 if area > 0 else (max(e) / n if max(e) > 0 else 1.0)
    return max(cell, max(e) / 2 ** 20, 1e-6)


class NearestGrid:
    """A target cloud sorted into a uniform grid of ``cell`` metres for ``lnr_nn_search``.  ``cell=None`` reads the
    target's box back once and takes ``default_cell``.  The result of a query does not depend on the cell size."""

    def __init__(self, tgt, cell=None):
        t = _cloud(tgt, "nearest_distances")
        dev = t.device
        lo, hi = t.min(dim=0).values, t.max(dim=0).values
        if cell is None:
            box = torch.stack((lo, hi)).tolist()
            if not np.isfinite(box).all():
                raise RuntimeError("nearest_distances: a coordinate is nan or inf")
            cell = default_cell(box[0], box[1], t.shape[0])
        self.cell = float(cell)
        self.n = t.shape[0]
        self.origin = lo.double()
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        keys = _cell_keys(t, self.origin, self.cell, self.status)
        # the cell of the largest coordinate, by the kernel's own arithmetic; lnr_nn_search clamps what is left of a nan
        top = torch.floor((hi.double() - self.origin) / self.cell)
        self.dims = (torch.nan_to_num(top, nan=0.0).clamp(0, 2 ** L.CLOUD_CELL_BITS - 1) + 1).to(torch.int32)
        self.keys, perm = torch.sort(keys, stable=True)
        self.points = t[perm].contiguous()
        self.perm = perm.to(torch.int32)

    def query(self, src, check=True):
        """(dist float64, idx int32, d2 float32) per point of ``src``.  ``check`` reads the status word (a
        synchronisation); with ``check=False`` the caller reads ``self.status`` later."""
        q = _cloud(src, "nearest_distances")
        dev, n = q.device, q.shape[0]
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        ws = torch.empty(int(L.lib().lnr_nn_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=dev)
        L.call("lnr_nn_search", q, n, self.points, self.keys, self.perm, self.n, self.origin, self.cell, self.dims,
               ws, ws.numel() * 8, idx, d2, dist, self.status, L.stream(dev))
        if check:
            _raise_status(int(self.status.item()), "nearest_distances")
        return dist, idx, d2


def nearest_distances(src, tgt, cell=None):
    """Open3D's ``src.compute_point_cloud_distance(tgt)`` on device clouds: (dist (n,) float64, idx (n,) int32, d2 (n,)
    float32), the target point with the smallest (float32 squared distance, index) for each source point."""
    return NearestGrid(tgt, cell).query(src)


def distance_stats(dist, threshold, out=None):
    """out[0] = sum(dist), out[1] = count(dist > threshold), float64 on the device (lnr_dist_stats)."""
    dev, n = dist.device, dist.shape[0]
    out = torch.empty(2, dtype=torch.float64, device=dev) if out is None else out
    ws = torch.empty(int(L.lib().lnr_dist_stats_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    L.call("lnr_dist_stats", dist, n, float(threshold), ws, ws.numel() * 8, out, L.stream(dev))
    return out


def transform_points(points, T):
    """T (4, 4) applied to a float32 device cloud in float64, term by term, rounded to float32 once."""
    Tm = torch.as_tensor(np.asarray(T, np.float64)).to(points.device)
    p = points.double()
    q = p[:, 0:1] * Tm[:3, 0] + p[:, 1:2] * Tm[:3, 1] + p[:, 2:3] * Tm[:3, 2] + Tm[:3, 3]
    return q.float().contiguous()


def align_clouds(est, gt, align_max_points=1 << 16, search="brute"):
    """The reference's alignment step on filtered device clouds: uniform down-sampling to the cap, normals (k = 30) of
    the target, one point-to-plane ICP stage (0.125 m, 10 iterations, 1e-12 / 1e-12), est onto gt.  Returns T (4, 4)
    float64 and the stage's state.  ``search="grid"``: normals and correspondences on the cell grid
    (``tracking.cloud_normals_grid``, lnr_icp_stage_grid), the same T bit for bit, with the cap at
    ALIGN_MAX_POINTS_GRID."""
    from . import tracking as TR
    _check_align_cap(align_max_points, search)
    ae = uniform_down_sample(est, alignment_skip(est.shape[0], align_max_points)).contiguous()
    ag = uniform_down_sample(gt, alignment_skip(gt.shape[0], align_max_points)).contiguous()
    if ag.shape[0] < ALIGN_KNN:
        raise RuntimeError(f"compare_point_clouds: {ag.shape[0]} alignment points are fewer than k={ALIGN_KNN}")
    normals = TR.cloud_normals_grid(ag, ALIGN_KNN) if search == "grid" else TR.cloud_normals(ag, ALIGN_KNN)
    T, res = TR.icp(ae, ag, normals, [TR.IcpStage(0.125, 10, 1e-12, 1e-12)], search=search)
    if res[-1]["status"]:
        _raise_status(res[-1]["status"], "compare_point_clouds")
    return T, res[-1]


def compare_point_clouds(est, gt, f_score_threshold=0.1, voxel_size=0.05, align=True, align_max_points=1 << 16,
                         cell=None, timer=None, return_distances=False, align_search="brute"):
    """evaluate_lidar_map.compare_point_clouds on float32 (n, 3) device clouds; returns the reference's dict (accuracy,
    completion, chamfer_distance, recall, precision, f-score, num_points).  ``cell``: the search grid's cell, default
    DEFAULT_CELL_VOXELS x voxel_size.  Both directions' sums and counts come back in one copy.  ``align_search``:
    ``align_clouds``' search; with "grid" ``align_max_points`` may reach ALIGN_MAX_POINTS_GRID."""
    from .meshing import _NoTimer
    timer = timer or _NoTimer()
    _check_align_cap(align_max_points, align_search)
    with timer("voxel_filter"):
        e, g = voxel_down_sample(est, voxel_size), voxel_down_sample(gt, voxel_size)
    T = np.eye(4)
    if align:
        with timer("align"):
            T, _ = align_clouds(e, g, align_max_points, align_search)
            e = transform_points(e, T)
    cell = DEFAULT_CELL_VOXELS * float(voxel_size) if cell is None else float(cell)
    with timer("search"):
        ge, gg = NearestGrid(e, cell), NearestGrid(g, cell)
        acc = gg.query(e, check=False)[0]
        comp = ge.query(g, check=False)[0]
    with timer("stats"):
        out = torch.empty(5, dtype=torch.float64, device=e.device)
        distance_stats(acc, f_score_threshold, out[0:2])
        distance_stats(comp, f_score_threshold, out[2:4])
        out[4] = (ge.status | gg.status)[0]
        sa, fp, sc, fn, bits = out.tolist()
    _raise_status(int(bits), "compare_point_clouds")
    stats = statistics(sa, acc.shape[0], int(fp), sc, comp.shape[0], int(fn))
    return (stats, acc, comp, T) if return_distances else stats


class LidarMapRenderer:
    """renderer_lidar.py on a ``loner_amd.step.FieldState``: the map as the cloud a synthetic lidar would see.  The
    sweep is ``meshing.build_lidar_directions`` at the reference's 0.1 degrees; depth and variance come from
    ``evaluate.DepthRenderer`` (Model.forward(testing=True)) times the cube's scale; a return is kept iff variance <
    var_threshold and depth < ray_range[1] - 0.25.  Rays that fail the 1 m filter are dropped with their directions,
    as ``meshing.Mesher`` drops them."""

    def __init__(self, state, world_cube, ray_range, lidar_vertical_fov, vertical_resolution=0.1,
                 horizontal_resolution=0.1, n_samples=2048, chunk=4096, var_threshold=1e-2):
        from .evaluate import DepthRenderer
        from .meshing import build_lidar_directions
        self.state = state
        self.world_cube = world_cube
        self.ray_range = (float(ray_range[0]), float(ray_range[1]))
        self.var_threshold = float(var_threshold)
        self.scale = float(np.float32(world_cube.scale_factor.reshape(-1)[0].item()))
        self.renderer = DepthRenderer(state, n_samples=n_samples, chunk=chunk)
        self.directions = build_lidar_directions(lidar_vertical_fov, vertical_resolution, horizontal_resolution)
        self._dirs_dev = self.directions.t().contiguous().to(state.device)

    def sweep(self, pose, key):
        """The rendered sweep before the filter: (directions (R, 3), depth (R,), variance (R,)) on the device, depth
        and variance in metres (times the scale factor, float32)."""
        from .evaluate import scan_window
        dev = self.state.device
        scan = dict(directions=self.directions, distances=torch.ones(self.directions.shape[1]))
        pose = torch.as_tensor(pose).detach().to("cpu", torch.float32)
        win = scan_window(scan, pose, self.world_cube, self.ray_range, dev)
        rays, _, valid = win.build_all()
        dirs = self._dirs_dev
        if not win.all_valid:
            keep = valid.bool()
            rays, dirs = rays[keep].contiguous(), dirs[keep]
        depth, _, variance = self.renderer.render(rays, key)
        scale = torch.tensor(self.scale, dtype=torch.float32, device=dev)
        return dirs, depth * scale, variance * scale

    def filter(self, dirs, depth, variance):
        """Sensor-frame points directions x depth of the returns the reference keeps."""
        dev = depth.device
        good = (variance < torch.tensor(self.var_threshold, dtype=torch.float32, device=dev)) & \
               (depth < torch.tensor(self.ray_range[1] - 0.25, dtype=torch.float32, device=dev))
        return (dirs * depth[:, None])[good].contiguous()

    def render_scan(self, pose, key):
        """One pose's sweep as sensor-frame points (m, 3) float32 on the device."""
        return self.filter(*self.sweep(pose, key))

    def render(self, poses, voxel_size, skip_step=5, key=0):
        """The reference's loop over ``poses[::skip_step]``: each sweep voxel-filtered, moved to the world by its pose,
        all of them concatenated and filtered again (``voxel_size=None``: no filter).  Sweep k renders with
        lnr_step_key(key, k)."""
        clouds = []
        for k, pose in enumerate(poses[::skip_step]):
            pts = self.render_scan(pose, L.step_key(key, k))
            if pts.shape[0] == 0:
                continue
            if voxel_size is not None:
                pts = voxel_down_sample(pts, voxel_size)
            clouds.append(transform_points(pts, torch.as_tensor(pose).detach().cpu().double().numpy()))
        if not clouds:
            return torch.zeros(0, 3, dtype=torch.float32, device=self.state.device)
        cloud = torch.cat(clouds)
        return voxel_down_sample(cloud, voxel_size) if voxel_size is not None else cloud
