"""The ground-truth LiDAR map on the GPU (the reference's examples/fusion_portable/create_lidar_map.py and
mask_gt_with_trajectory.py, without Open3D, rosbag or pandas): every return moved to the world by the trajectory's
pose at its own timestamp, voxel-filtered, merged, optionally cleaned by the statistical outlier filter; and a
ground-truth cloud masked by that map.

    trajectory_table         TUM rows (t x y z qx qy qz qw) -> the table lnr_trajectory_transform reads (scipy, host)
    normalise_point_times    create_lidar_map.py:95-100 in float64
    scan_points_and_times    one scan's returns beyond min_range and their absolute times, or None where the reference
                             drops the scan (:65-66, :102-103)
    deskew_points            lnr_trajectory_transform: (world points, valid mask)
    knn                      lnr_knn_search on a ``map_eval.NearestGrid``: (idx, d2, mean distance)
    dist_moments             lnr_dist_moments
    remove_statistical_outlier
                             Open3D's filter from knn's mean distances and two lnr_dist_moments passes
    build_lidar_map          create_lidar_map.py:62-135
    mask_cloud               mask_gt_with_trajectory.py:86-98
    deskew_points_ref, knn_key_ref, knn_ref, remove_statistical_outlier_ref, build_lidar_map_ref, mask_cloud_ref
                             float64 numpy / scipy restatements: the tests' oracle (validated on their own in
                             tests/test_lidar_map_ref.py) and what a host without a GPU runs

Deviations from the reference:
  * times are float64 (reference: float128): an absolute time near 1.7e9 s resolves 2.4e-7 s, 2.4e-7 of a 1 s
    trajectory interval;
  * points are float32, moved in float64 and rounded once (Open3D holds float64);
  * a return whose time lies before the trajectory's first pose is dropped (the reference only tests the last time of
    a scan against the trajectory's end, and scipy raises on an earlier one); a scan without a return beyond
    ``min_range`` is dropped (the reference indexes an empty array);
  * the voxel filter's output order is ascending cell key (map_eval), so is the merged map's;
  * the outlier rule is Open3D's as its source is recalled (Open3D is not installed where this was written).
"""
import numpy as np
import torch

from . import _lib as L
from . import map_eval as ME

# knn's default cell is KNN_CELL_FACTOR x default_cell x sqrt(k): the fastest of 0.5, 1, 2, 4, 8 for k = 20 on a
# voxel-filtered surface cloud of 2^17 points, grid build included (tools/lidar_map_demo.py,
# profiles/lidar_map_demo.json: 3.76, 2.93, 2.03, 3.11, 6.24 ms)
KNN_CELL_FACTOR = 2.0
KNN_CELL_FACTORS = (0.5, 1.0, 2.0, 4.0, 8.0)


# ---------------------------------------------------------------------------------------------- the trajectory
class TrajectoryTable:
    """float64 numpy arrays t (M,), xyz (M, 3), rot (M, 9), rel (M - 1, 3); ``device(dev)`` uploads them once."""

    def __init__(self, t, xyz, rot, rel):
        self.t, self.xyz, self.rot, self.rel = t, xyz, rot, rel
        self._dev = {}

    def __len__(self):
        return len(self.t)

    def device(self, dev):
        key = str(torch.device(dev))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                   for a in (self.t, self.xyz, self.rot, self.rel))
        return self._dev[key]


def trajectory_table(tum):
    """The kernel's table from TUM rows (M, 8): t x y z qx qy qz qw.  Rotations are scipy's (``Rotation.from_quat``
    normalises), rel[i] the rotation vector of R_i^-1 R_{i+1} as ``Slerp`` computes it."""
    from scipy.spatial.transform import Rotation
    tum = np.asarray(tum, np.float64)
    if tum.ndim != 2 or tum.shape[1] != 8 or tum.shape[0] < 2:
        raise ValueError("trajectory_table: expected (M, 8) TUM rows with M >= 2")
    if not np.isfinite(tum).all():
        raise ValueError("trajectory_table: a value is nan or inf")
    t = np.ascontiguousarray(tum[:, 0])
    if not (np.diff(t) > 0).all():
        raise ValueError("trajectory_table: timestamps must be strictly increasing")
    rot = Rotation.from_quat(tum[:, 4:8])
    rel = (rot[:-1].inv() * rot[1:]).as_rotvec().reshape(-1, 3)
    return TrajectoryTable(t, np.ascontiguousarray(tum[:, 1:4]), rot.as_matrix().reshape(-1, 9), rel)


def normalise_point_times(ts, stamp):
    """create_lidar_map.py:95-100 on one scan's per-point times (float64; the reference holds float128): nanoseconds
    to seconds when the last one exceeds 1e7; offsets from the scan's stamp when the first is below 1e-2, otherwise
    times re-based so that the first equals the stamp."""
    ts = np.array(ts, np.float64).reshape(-1)
    if ts[-1] > 1e7:
        ts *= 1e-9
    if ts[0] < 1e-2:
        ts += float(stamp)
    else:
        ts = ts - ts[0] + float(stamp)
    return ts


def _range(p):
    p = p.astype(np.float64)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def scan_points_and_times(scan, table, min_range=0.5):
    """(points (m, 3) float32, times (m,) float64) of the scan's returns with range > ``min_range``, in the sensor
    frame and absolute seconds, or None where the reference drops the scan: its stamp outside the trajectory (:65-66),
    a normalised time beyond the trajectory's end (:102-103), or no return left.  ``scan``: directions (3, P),
    distances (P,), time, optionally timestamps (P,); without them every return carries the scan's stamp."""
    stamp = float(scan["time"])
    if stamp < table.t[0] or stamp > table.t[-1]:
        return None
    d = torch.as_tensor(scan["directions"]).detach().cpu().float()
    r = torch.as_tensor(scan["distances"]).detach().cpu().float()
    p = (d * r).t().contiguous().numpy()  # float32 products, as scan_world_points forms them
    keep = _range(p) > float(min_range)
    if not keep.any():
        return None
    ts = scan.get("timestamps")
    ts = np.zeros(len(p)) if ts is None else torch.as_tensor(ts).detach().cpu().double().numpy().reshape(-1)
    if len(ts) != len(p):
        raise ValueError(f"build_lidar_map: {len(ts)} timestamps for {len(p)} returns")
    ts = normalise_point_times(ts[keep], stamp)
    if ts.max() > table.t[-1]:
        return None
    return np.ascontiguousarray(p[keep]), ts


# ---------------------------------------------------------------------------------------------- numpy restatements
def deskew_points_ref(points, times, table, min_range=0.5, dtype=np.float32):
    """lnr_trajectory_transform in float64 numpy, operation by operation: (out (n, 3) float32, valid (n,) bool).
    ``dtype=np.float64`` returns the points before their rounding."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(times, np.float64).reshape(-1)
    T, m = table.t, len(table.t)
    with np.errstate(all="ignore"):
        finite = np.isfinite(p).all(axis=1) & np.isfinite(t)
        inside = finite & (t >= T[0]) & (t <= T[-1])
        ok = inside & (_range(p) > float(min_range))
        i = np.clip(np.searchsorted(T, t, "left") - 1, 0, m - 2)
        alpha = (t - T[i]) / (T[i + 1] - T[i])
        v = alpha[:, None] * table.rel[i]
        vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        th2 = (vx * vx + vy * vy) + vz * vz
        th = np.sqrt(th2)
        sh = np.sin(0.5 * th)
        a = np.where(th < 1e-4, 1.0 - th2 / 6.0, np.sin(th) / th)
        b = np.where(th < 1e-4, 0.5 - th2 / 24.0, 2.0 * sh * sh / th2)
        cx, cy, cz = vy * pz - vz * py, vz * px - vx * pz, vx * py - vy * px
        dx, dy, dz = vy * cz - vz * cy, vz * cx - vx * cz, vx * cy - vy * cx
        qx, qy, qz = px + (a * cx + b * dx), py + (a * cy + b * dy), pz + (a * cz + b * dz)
        R, x0, x1 = table.rot[i], table.xyz[i], table.xyz[i + 1]
        out = np.stack([((R[:, 3 * r] * qx + R[:, 3 * r + 1] * qy) + R[:, 3 * r + 2] * qz) +
                        (x0[:, r] + alpha * (x1[:, r] - x0[:, r])) for r in range(3)], axis=1)
        ok &= np.isfinite(out).all(axis=1)
        out = np.where(ok[:, None], out, 0.0).astype(dtype)
    return out, ok


def knn_key_ref(src, tgt, k, block=256):
    """The search key of lnr_knn_search emulated in numpy (``map_eval.nn_key_ref``'s arithmetic): the k smallest
    (float32 d2, index) per source point, ascending.  Returns (idx (n, k) int32, d2 (n, k) float32).  O(n m log m)."""
    s, t = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    if not 1 <= k <= len(t):
        raise ValueError(f"knn: k={k} outside [1, {len(t)}]")
    idx = np.empty((len(s), k), np.int32)
    d2 = np.empty((len(s), k), np.float32)
    for a in range(0, len(s), block):
        d = s[a:a + block, None, :] - t[None, :, :]
        d *= d
        key = (d[..., 0] + d[..., 1]) + d[..., 2]
        j = np.argsort(key, axis=1, kind="stable")[:, :k]  # stable: equal d2 in index order
        idx[a:a + block] = j
        d2[a:a + block] = np.take_along_axis(key, j, axis=1)
    return idx, d2


def knn_ref(src, tgt, k):
    """(dist (n, k) float64, idx (n, k)) by a k-d tree in float64."""
    from scipy.spatial import cKDTree
    dist, idx = cKDTree(np.asarray(tgt, np.float64)).query(np.asarray(src, np.float64), k=k)
    return dist.reshape(len(dist), -1), idx.reshape(len(idx), -1)


def outlier_threshold_ref(a, std_ratio):
    """mu + std_ratio s of the mean distances a: mu = sum_{a>0} a / n, s = sqrt(sum_{a>0} (a - mu)^2 / (n - 1))."""
    a = np.asarray(a, np.float64)
    n, pos = len(a), a[a > 0]
    mu = pos.sum() / n
    return mu + float(std_ratio) * np.sqrt(((pos - mu) ** 2).sum() / (n - 1))


def remove_statistical_outlier_ref(points, nb_neighbors=20, std_ratio=1.5, return_distances=False):
    """Open3D's remove_statistical_outlier in float64: a_i = the mean distance to the ``nb_neighbors`` nearest points,
    itself included; keep i iff 0 < a_i < mu + std_ratio s.  Returns (kept points, kept indices int64)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if len(p) < 2:
        raise ValueError("remove_statistical_outlier: fewer than 2 points")
    if nb_neighbors < 1 or not std_ratio > 0:
        raise ValueError("remove_statistical_outlier: nb_neighbors < 1 or std_ratio <= 0")
    a = knn_ref(p, p, min(int(nb_neighbors), len(p)))[0].mean(axis=1)
    thr = outlier_threshold_ref(a, std_ratio)
    ind = np.flatnonzero((a > 0) & (a < thr)).astype(np.int64)
    return (p[ind], ind, a, thr) if return_distances else (p[ind], ind)


def mask_cloud_ref(gt, reconstructed, dist_threshold=0.1, transform=None):
    g = np.asarray(gt, np.float32).reshape(-1, 3)
    r = np.asarray(reconstructed, np.float32).reshape(-1, 3)
    if transform is not None:
        r = ME.transform_points_ref(r, transform)
    keep = ME.nearest_distances_ref(g, r)[0] < float(dist_threshold)
    return g[keep], keep


def build_lidar_map_ref(scans, tum, voxel_size=0.05, min_range=0.5, outlier_filter=False):
    """build_lidar_map on the float64 restatements; (n, 3) float32 numpy."""
    table = trajectory_table(tum)
    clouds = []
    for scan in scans:
        pt = scan_points_and_times(scan, table, min_range)
        if pt is None:
            continue
        w, valid = deskew_points_ref(pt[0], pt[1], table, min_range)
        if valid.any():
            clouds.append(ME.voxel_down_sample_ref(w[valid], voxel_size))
    if not clouds:
        return np.zeros((0, 3), np.float32)
    cloud = ME.voxel_down_sample_ref(np.concatenate(clouds), voxel_size)
    return remove_statistical_outlier_ref(cloud)[0] if outlier_filter else cloud


# ---------------------------------------------------------------------------------------------- GPU
def deskew_points(points, times, table, min_range=0.5, check=True):
    """Sensor-frame returns (n, 3) float32 on the device and their absolute times (n,) float64 -> (world points (n, 3)
    float32, valid (n,) bool).  An invalid return (range not > ``min_range``, a time outside the trajectory, a
    non-finite input) comes back as (0, 0, 0).  ``check`` reads the status word once and raises RuntimeError on a
    non-finite input."""
    pts = ME._cloud(points, "deskew_points")
    dev, n = pts.device, pts.shape[0]
    t = torch.as_tensor(times)
    if t.dtype != torch.float64 or t.dim() != 1 or t.shape[0] != n:
        raise ValueError("deskew_points: expected float64 times, one per point")
    t = t.to(dev).contiguous()
    if not isinstance(table, TrajectoryTable):
        raise ValueError("deskew_points: expected a trajectory_table")
    tt, xyz, rot, rel = table.device(dev)
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("lnr_trajectory_transform", pts, t, n, tt, xyz, rot, rel, len(table), float(min_range), out, valid, status,
           L.stream(dev))
    if check:
        ME._raise_status(int(status.item()), "deskew_points")
    return out, valid.bool()


def default_knn_cell(lo, hi, n, k):
    """A search cell for k neighbours in a surface cloud: ``map_eval.default_cell`` (two points per occupied cell)
    times sqrt(k), so that the points per cell follow k, times the measured KNN_CELL_FACTOR."""
    return KNN_CELL_FACTOR * ME.default_cell(lo, hi, n) * float(k) ** 0.5


def knn_grid(tgt, k, cell=None):
    """A ``map_eval.NearestGrid`` of ``tgt`` with ``default_knn_cell`` (one read of the target's box)."""
    t = ME._cloud(tgt, "knn")
    if cell is None:
        box = torch.stack((t.min(dim=0).values, t.max(dim=0).values)).tolist()
        if not np.isfinite(box).all():
            raise RuntimeError("knn: a coordinate is nan or inf")
        cell = default_knn_cell(box[0], box[1], t.shape[0], k)
    return ME.NearestGrid(t, cell)


def knn(src, tgt_or_grid, k, cell=None, check=True):
    """The exact k nearest targets of every source point by (float32 d2, index): (idx (n, k) int32 in the target's
    own order, d2 (n, k) float32, mean_dist (n,) float64), rows ascending.  ``tgt_or_grid``: a float32 (m, 3) device
    cloud or a ``map_eval.NearestGrid`` of one; the result does not depend on the cell.  ``check`` reads the status
    word (a synchronisation); with ``check=False`` the caller reads ``grid.status`` later."""
    q = ME._cloud(src, "knn")
    k = int(k)
    grid = tgt_or_grid if isinstance(tgt_or_grid, ME.NearestGrid) else None
    n_tgt = grid.n if grid else ME._cloud(tgt_or_grid, "knn").shape[0]
    if not 1 <= k <= min(L.KNN_MAX_K, n_tgt):
        raise ValueError(f"knn: k={k} outside [1, min({L.KNN_MAX_K}, {n_tgt} targets)]")
    if grid is None:
        grid = knn_grid(tgt_or_grid, k, cell)
    dev, n = q.device, q.shape[0]
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib().lnr_knn_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=dev)
    L.call("lnr_knn_search", q, n, grid.points, grid.keys, grid.perm, grid.n, grid.origin, grid.cell, grid.dims, k,
           ws, ws.numel() * 8, idx, d2, mean, grid.status, L.stream(dev))
    if check:
        ME._raise_status(int(grid.status.item()), "knn")
    return idx, d2, mean


def dist_moments(v, centre=0.0, out=None):
    """Over the entries v > 0 of a float64 device array: out[0] = sum, out[1] = count, out[2] = sum (v - centre)^2.
    ``centre``: a float, or a 1-element float64 device tensor (no host round trip)."""
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.dim() != 1 or v.shape[0] < 1:
        raise ValueError("dist_moments: expected a non-empty float64 (n,) tensor")
    dev, n = v.device, v.shape[0]
    out = torch.empty(3, dtype=torch.float64, device=dev) if out is None else out
    ws = torch.empty(int(L.lib().lnr_dist_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    on_dev = isinstance(centre, torch.Tensor)
    if on_dev and (centre.dtype != torch.float64 or centre.numel() != 1):
        raise ValueError("dist_moments: a device centre is one float64")
    L.call("lnr_dist_moments", v.contiguous(), n, 0.0 if on_dev else float(centre),
           centre.contiguous() if on_dev else None, ws, ws.numel() * 8, out, L.stream(dev))
    return out


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=1.5, return_distances=False):
    """Open3D's remove_statistical_outlier on a float32 (n, 3) device cloud: (kept points, kept indices int64,
    ascending).  The mean distances come from ``knn`` (itself included), the mean and the deviation from two
    lnr_dist_moments passes whose centre stays on the device.  Two host reads: the cloud's box (the search cell) and
    {kept count, status word}, which sizes the output."""
    pts = ME._cloud(points, "remove_statistical_outlier")
    n = pts.shape[0]
    if n < 2:
        raise ValueError("remove_statistical_outlier: fewer than 2 points")
    if nb_neighbors < 1 or not std_ratio > 0:
        raise ValueError("remove_statistical_outlier: nb_neighbors < 1 or std_ratio <= 0")
    k = min(int(nb_neighbors), n)
    grid = knn_grid(pts, k)
    a = knn(pts, grid, k, check=False)[2]
    mu = (dist_moments(a)[0] / n).reshape(1)
    thr = mu + float(std_ratio) * torch.sqrt(dist_moments(a, mu)[2] / (n - 1))
    keep = (a > 0) & (a < thr)
    pos = torch.cumsum(keep, 0)
    count, bits = torch.stack((pos[-1], grid.status[0].to(torch.int64))).tolist()
    ME._raise_status(bits, "remove_statistical_outlier")
    # compaction without another synchronisation: kept point i goes to slot pos[i] - 1, the others to a spare slot
    ind = torch.empty(count + 1, dtype=torch.int64, device=pts.device)
    ind.scatter_(0, torch.where(keep, pos - 1, count), torch.arange(n, device=pts.device))
    ind = ind[:count]
    return (pts[ind], ind, a, thr) if return_distances else (pts[ind], ind)


def build_lidar_map(scans, tum, voxel_size=0.05, min_range=0.5, outlier_filter=False, device="cuda", timer=None):
    """create_lidar_map.py on scan dicts (directions (3, P), distances (P,), time, optional per-point timestamps) and
    TUM rows: each kept scan's returns at their own interpolated poses, voxel-filtered; the scans merged and filtered
    again; optionally remove_statistical_outlier(20, 1.5).  Returns (n, 3) float32 on the device."""
    from .meshing import _NoTimer
    timer = timer or _NoTimer()
    table = trajectory_table(tum)
    clouds = []
    for scan in scans:
        with timer("prepare"):
            pt = scan_points_and_times(scan, table, min_range)
        if pt is None:
            continue
        with timer("deskew"):
            w, valid = deskew_points(torch.from_numpy(pt[0]).to(device), torch.from_numpy(pt[1]).to(device), table,
                                     min_range)
            w = w[valid]
        if w.shape[0]:
            with timer("voxel_filter_scan"):
                clouds.append(ME.voxel_down_sample(w, voxel_size))
    if not clouds:
        return torch.zeros(0, 3, dtype=torch.float32, device=device)
    with timer("voxel_filter_merged"):
        cloud = ME.voxel_down_sample(torch.cat(clouds), voxel_size)
    if outlier_filter:
        with timer("outlier_filter"):
            cloud = remove_statistical_outlier(cloud)[0]
    return cloud


def mask_cloud(gt, reconstructed, dist_threshold=0.1, transform=None, cell=None):
    """mask_gt_with_trajectory.py:86-98 on device clouds: (the points of ``gt`` whose nearest point of
    ``reconstructed`` is closer than ``dist_threshold``, the mask (n,) bool).  ``transform`` (4, 4) moves
    ``reconstructed`` first."""
    g, r = ME._cloud(gt, "mask_cloud"), ME._cloud(reconstructed, "mask_cloud")
    if transform is not None:
        r = ME.transform_points(r, transform)
    keep = ME.NearestGrid(r, cell).query(g)[0] < float(dist_threshold)
    return g[keep], keep
