"""Frame-to-frame ICP tracking on the GPU (src/tracking/tracker.py:167-255): LiDAR odometry without Open3D.

    frame_point_cloud   Frame.build_point_cloud's index logic (src/common/frame.py:105-146)
    cloud_normals       lnr_cloud_normals: Open3D's estimate_normals() with its default KNN(30)
    cloud_normals_grid  the same normals from the grid kNN (lnr_knn_search + lnr_normals_from_knn): any cloud size
    IcpSolver           lnr_icp_init / lnr_icp_stage around a device-resident lnr_icp_state; ``search="grid"`` runs
                        lnr_icp_stage_grid on a ``GridTarget`` instead (the same states, bit for bit)
    Tracker             track(scan): cloud, normals, the ICP schedule against the previous frame, pose chaining,
                        motion compensation and sky rays (``loner_amd.preprocess``)
    normals_reference, icp_reference
                        numpy / scipy float64 restatements of the two kernels' contracts (include/loner_amd.h); the GPU
                        tests compare against them, tests/test_tracking_ref.py validates them on their own.

Open3D itself is not a dependency and is not compared against: parity is to the restatements, which follow
registration_icp's loop (evaluate, update, evaluate, compare the two evaluations) and
TransformationEstimationPointToPlane's normal equations.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from . import lidar_map as LM
from . import map_eval as ME
from . import preprocess as PP

N_SUMS = 27  # J^T J upper triangle (21, row-major) + J^T r (6)
SEARCHES = ("brute", "grid")
# A grid stage's cell is max(ICP_CELL_FACTOR x map_eval.default_cell, threshold (1 + 2^-10) / LNR_NN_MAX_RINGS).
# 0.5 is the fastest of ICP_CELL_FACTORS for the default schedule at 5e3, 3.5e4 and 1e5 points a side, builds included
# (tools/registration_bench.py, profiles/registration_grid.json, DESIGN.md 7e: 26.8, 29.9, 50.2, 131, 299 ms at 1e5).
# A scan is far denser near the sensor than default_cell's two points per cell assumes, and one thread walks a cell.
ICP_CELL_FACTOR = 0.5
ICP_CELL_FACTORS = (0.5, 1.0, 2.0, 4.0, 8.0)
NORMALS_CHUNK = 1 << 18  # queries per lnr_knn_search call of cloud_normals_grid: bounds the (n, k) temporaries


def check_search(search, what="search"):
    if search not in SEARCHES:
        raise ValueError(f"{what}={search!r} is not one of {SEARCHES}")
    return search


# ---------------------------------------------------------------------------------------------- settings
@dataclass
class IcpStage:
    threshold: float
    max_iterations: int = 10
    relative_fitness: float = 1e-8
    relative_rmse: float = 1e-8


def _default_schedule():
    return [IcpStage(1.5), IcpStage(0.125)]


@dataclass
class TrackerSettings:
    """cfg/defaults.yaml:135-164 (``tracker:``)."""
    scan_duration: float = 0.9
    schedule: list = field(default_factory=_default_schedule)
    downsample_type: str = "UNIFORM"
    target_uniform_point_count: int = 5000
    knn: int = 30
    motion_compensation: bool = True
    compute_sky_rays: bool = False
    search: str = "brute"  # "grid": normals and correspondences on the cell grid (the same results; any cloud size)

    def __post_init__(self):
        check_search(self.search, "tracker search")
        if self.downsample_type == "VOXEL":
            raise NotImplementedError("tracker downsample type VOXEL is not built; use UNIFORM or None")
        if self.downsample_type not in (None, "UNIFORM"):
            raise ValueError(f"Unrecognized downsample type {self.downsample_type}")
        self.schedule = [s if isinstance(s, IcpStage) else IcpStage(**s) for s in self.schedule]

    @classmethod
    def from_dict(cls, d):
        """From the reference's ``tracker:`` YAML layout; missing keys keep the defaults."""
        d = d or {}
        icp = d.get("icp") or {}
        kw = {}
        if "scan_duration" in icp:
            kw["scan_duration"] = icp["scan_duration"]
        if "schedule" in icp:
            kw["schedule"] = [IcpStage(float(s["threshold"]), int(s.get("max_iterations", 10)),
                                       float(s.get("relative_fitness", 1e-8)), float(s.get("relative_rmse", 1e-8)))
                              for s in icp["schedule"]]
        ds = icp.get("downsample") or {}
        if "type" in ds:
            kw["downsample_type"] = ds["type"]
        if "target_uniform_point_count" in ds:
            kw["target_uniform_point_count"] = int(ds["target_uniform_point_count"])
        mc = d.get("motion_compensation") or {}
        if "enabled" in mc:
            kw["motion_compensation"] = bool(mc["enabled"])
        if "compute_sky_rays" in d:
            kw["compute_sky_rays"] = bool(d["compute_sky_rays"])
        return cls(**kw)


# ---------------------------------------------------------------------------------------------- the cloud
def frame_indices(timestamps=None, n_points=None, scan_duration=None, target_points=None):
    """(start, final, step) of Frame.build_point_cloud: the middle ``scan_duration`` share of the sweep by
    timestamp (all points without timestamps, without a share, or for a sweep of at most 1e-3 s), and
    ``step = (final - start) // target_points``, 1 if that is 0."""
    if timestamps is not None:
        n_points = int(timestamps.shape[0])
    start, final = 0, int(n_points)
    if timestamps is not None and scan_duration is not None and n_points > 0:
        ts = timestamps
        sweep = float(ts[-1] - ts[0])
        if sweep > 1e-3:
            per_scan = scan_duration * sweep
            middle = (ts[0] + ts[-1]) / 2
            start = int(torch.argmax((ts - middle >= -per_scan / 2).float()))
            if bool(ts[-1] < middle + per_scan / 2):
                final = n_points
            else:
                final = int(torch.argmax((ts - middle >= per_scan / 2).float()))
    step = 1 if target_points is None else (final - start) // int(target_points)
    return start, final, max(step, 1)


def frame_point_cloud(directions, distances, timestamps=None, scan_duration=None, target_points=None):
    """The ICP cloud of a scan, (n, 3) fp32 on the scan's device: ``directions`` (3, P) times ``distances`` (P,) over
    ``[start:final:step]`` of ``frame_indices``.  Reading the indices synchronises when the timestamps live on the
    GPU."""
    start, final, step = frame_indices(timestamps, distances.shape[0], scan_duration, target_points)
    pts = directions[:, start:final:step] * distances[start:final:step]
    return pts.t().to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------- float64 restatements
def normals_reference(points, k=30):
    """lnr_cloud_normals in float64: exact k nearest neighbours (the point itself included), covariance about their
    mean, unit eigenvector of the smallest eigenvalue, turned towards the origin; (0, 0, 1) for a zero covariance."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float64)
    _, idx = cKDTree(p).query(p, k=k)
    nb = p[idx.reshape(len(p), k)]
    c = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c) / k
    _, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0].copy()
    nrm[~cov.reshape(len(p), -1).any(axis=1)] = (0.0, 0.0, 1.0)
    nrm[np.einsum("ni,ni->n", nrm, p) > 0] *= -1.0
    return nrm


def transform_from_vector6(x):
    """Open3D's TransformVector6dToMatrix4d: rotation Rz(x2) Ry(x1) Rx(x0), translation x3..5."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    M = np.eye(4)
    M[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    M[:3, 3] = x[3:6]
    return M


def point_to_plane_terms(p, q, n):
    """Per-pair terms (m, 27) of the point-to-plane normal equations, float64: the upper triangle of J^T J (row-major)
    and J^T r, with J = [p x n, n] and r = (p - q) . n."""
    p, q, n = (np.asarray(a, np.float64) for a in (p, q, n))
    J = np.concatenate([np.cross(p, n), n], axis=1)
    r = np.einsum("ni,ni->n", p - q, n)
    iu = np.triu_indices(6)
    return np.concatenate([J[:, iu[0]] * J[:, iu[1]], J * r[:, None]], axis=1)


def solve_update(sums):
    """x of J^T J x = -J^T r from the 27 sums, or None when the matrix is not positive definite."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    x = np.linalg.solve(A, -np.asarray(sums[21:27]))
    return x if np.isfinite(x).all() else None


def icp_reference(src, tgt, tgt_normals, threshold, max_iterations=10, relative_fitness=1e-8, relative_rmse=1e-8,
                  T0=None):
    """One lnr_icp_stage in float64 with a k-d tree: max_iterations + 1 rounds of (correspond, update).  Returns a dict
    with T, fitness, rmse, n_corr, iterations, converged, sums and the last evaluation's corr_idx / corr_d."""
    from scipy.spatial import cKDTree
    s, t, tn = (np.asarray(a, np.float64) for a in (src, tgt, tgt_normals))
    tree = cKDTree(t)
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    out = dict(iterations=0, converged=False)
    fitness = rmse = 0.0
    for rnd in range(max_iterations + 1):
        p = s @ T[:3, :3].T + T[:3, 3]
        d, idx = tree.query(p, k=1)
        keep = d < threshold
        m = int(keep.sum())
        sums = point_to_plane_terms(p[keep], t[idx[keep]], tn[idx[keep]]).sum(axis=0)
        prev = (fitness, rmse)
        fitness = m / len(s) if m else 0.0
        rmse = float(np.sqrt((d[keep] ** 2).sum() / m)) if m else 0.0
        out.update(fitness=fitness, rmse=rmse, n_corr=m, sums=sums, corr_idx=np.where(keep, idx, -1), corr_d=d)
        if rnd > 0 and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            out["converged"] = True
            break
        if out["iterations"] < max_iterations:
            x = solve_update(sums) if m >= 6 else None
            if x is not None:
                T = transform_from_vector6(x) @ T
            out["iterations"] += 1
    out["T"] = T
    return out


def icp_schedule_reference(src, tgt, tgt_normals, schedule, T0=None):
    """The stages of ``schedule`` (IcpStage) chained on T; returns (T, per-stage results)."""
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    res = []
    for st in schedule:
        r = icp_reference(src, tgt, tgt_normals, st.threshold, st.max_iterations, st.relative_fitness,
                          st.relative_rmse, T)
        T = r["T"]
        res.append(r)
    return T, res


# ---------------------------------------------------------------------------------------------- GPU
def cloud_normals(points, k=30, out=None):
    """Normals (n, 3) fp32 of the device cloud ``points`` (n, 3) fp32 (lnr_cloud_normals)."""
    if out is None:
        out = torch.empty_like(points)
    L.call("lnr_cloud_normals", points, points.shape[0], int(k), out, L.stream(points.device))
    return out


def cloud_normals_grid(points, k=30, cell=None, out=None):
    """``cloud_normals`` for a cloud of any size up to LNR_CLOUD_MAX_POINTS: the exact k nearest neighbours from the
    grid search (``lidar_map.knn``), then lnr_normals_from_knn.  The lists are those lnr_cloud_normals finds, so the
    normals are its normals bit for bit, whatever ``cell`` is (default: ``lidar_map.default_knn_cell``, one read of
    the cloud's box).  Queries run NORMALS_CHUNK at a time.  The search's status word is read once at the end (a
    synchronisation): a nan or inf coordinate raises RuntimeError, as the box read does with ``cell=None``."""
    pts = ME._cloud(points, "cloud_normals_grid")
    n, k = pts.shape[0], int(k)
    if not 3 <= k <= min(64, n):
        raise ValueError(f"cloud_normals_grid: k={k} outside [3, min(64, {n} points)]")
    if out is None:
        out = torch.empty_like(pts)
    grid = LM.knn_grid(pts, k, cell)
    s = L.stream(pts.device)
    for a in range(0, n, NORMALS_CHUNK):
        q = pts[a:a + NORMALS_CHUNK]
        idx = LM.knn(q, grid, k, check=False)[0]
        L.call("lnr_normals_from_knn", q, q.shape[0], pts, n, idx, k, out[a:a + NORMALS_CHUNK], s)
    ME._raise_status(int(grid.status.item()), "cloud_normals_grid")
    return out


def icp_grid_rings_ref(threshold, cell):
    """lnr_icp_grid_rings in Python: the smallest R in 1 .. LNR_NN_MAX_RINGS with (R cell)^2 (1 - 2^-20) >= thr2, thr2
    the float32 square of the float32 threshold; 0 if there is none or an argument is out of range."""
    with np.errstate(over="ignore", invalid="ignore"):
        thr, cell = np.float32(threshold), float(cell)
        if not (np.isfinite(thr) and thr > 0 and np.isfinite(cell) and cell >= 1e-12):
            return 0
        thr2 = float(np.float32(float(thr) * float(thr)))
    if not np.isfinite(thr2):
        return 0
    for r in range(1, L.NN_MAX_RINGS + 1):
        bound = float(r) * cell
        if bound * bound * (1.0 - 2.0 ** -20) >= thr2:
            return r
    return 0


def icp_grid_cell(threshold, lo, hi, n, factor=None):
    """The cell of a grid stage: ``factor`` (default ICP_CELL_FACTOR) x ``map_eval.default_cell`` of the target's box,
    and never so small that the threshold would need more than LNR_NN_MAX_RINGS rings."""
    factor = ICP_CELL_FACTOR if factor is None else float(factor)
    floor = float(np.float32(threshold)) * (1.0 + 2.0 ** -10) / L.NN_MAX_RINGS
    return max(factor * ME.default_cell(lo, hi, n), floor)


class GridTarget:
    """An ICP target for ``search="grid"``: the cloud, its normals, and one ``map_eval.NearestGrid`` per distinct cell,
    each built when a stage first asks for it.  The cloud's box is read back once (a synchronisation)."""

    def __init__(self, tgt, normals):
        self.points = ME._cloud(tgt, "GridTarget")
        self.normals = ME._cloud(normals, "GridTarget normals")
        if self.normals.shape != self.points.shape:
            raise ValueError("GridTarget: one normal per point")
        self.n = self.points.shape[0]
        self._box = None
        self._grids = {}

    @property
    def box(self):
        if self._box is None:
            box = torch.stack((self.points.min(dim=0).values, self.points.max(dim=0).values)).tolist()
            if not np.isfinite(box).all():
                raise RuntimeError("GridTarget: a coordinate is nan or inf")
            self._box = box
        return self._box

    def cell_for(self, threshold, factor=None):
        return icp_grid_cell(threshold, self.box[0], self.box[1], self.n, factor)

    def grid(self, cell):
        cell = float(cell)
        if cell not in self._grids:
            self._grids[cell] = ME.NearestGrid(self.points, cell)
        return self._grids[cell]


STATE_BYTES = ctypes.sizeof(L.IcpState)


def _state_dict(raw, status=0):
    s = L.IcpState.from_buffer_copy(bytes(raw))
    return dict(status=int(status), T=np.array(s.T, np.float64).reshape(4, 4), fitness=float(s.fitness), rmse=float(s.rmse),
                sum_d2=float(s.sum_d2), sums=np.array(s.sums, np.float64), n_corr=int(s.n_corr),
                iterations=int(s.iterations), converged=bool(s.converged))


class IcpSolver:
    """The ICP schedule on one device: state, per-stage snapshots and the workspace are allocated once (the workspace
    grows with the largest source cloud seen).  ``run`` only enqueues; ``read`` is the one synchronisation (with
    ``search="grid"`` a target given as a tensor is wrapped in a ``GridTarget``, whose box is one more read).  The
    status word (LNR_CLOUD_NONFINITE, LNR_CLOUD_GRID_RANGE; grid stages only) is cleared by ``init`` and snapshot with
    every stage."""

    def __init__(self, device, max_stages=4):
        self.device = torch.device(device)
        self.state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=self.device)
        self.snap = torch.zeros(max_stages, STATE_BYTES, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(0, dtype=torch.float64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.status_snap = torch.zeros(max_stages, dtype=torch.int32, device=self.device)
        self.n_stages = 0

    def init(self, T0=None):
        T = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
        arr = (ctypes.c_double * 16)(*T.reshape(-1).tolist())
        L.call("lnr_icp_init", self.state, arr, L.stream(self.device))
        self.status.zero_()
        self.n_stages = 0

    def stage(self, src, tgt, tgt_normals, st, corr_idx=None, corr_d2=None, search="brute", cell=None):
        """One stage from the state's T.  ``search="grid"``: ``tgt`` is a ``GridTarget`` (``tgt_normals`` is then
        ignored) or a cloud that is wrapped in one; ``cell`` overrides ``GridTarget.cell_for(threshold)``."""
        check_search(search)
        grid = search == "grid"
        need = int((L.lib().lnr_icp_grid_workspace_bytes if grid else L.lib().lnr_icp_workspace_bytes)(src.shape[0]))
        if self.ws.numel() * 8 < need:
            self.ws = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        crit = (float(st.threshold), int(st.max_iterations), float(st.relative_fitness), float(st.relative_rmse))
        if grid:
            gt = tgt if isinstance(tgt, GridTarget) else GridTarget(tgt, tgt_normals)
            g = gt.grid(gt.cell_for(st.threshold) if cell is None else cell)
            L.call("lnr_icp_stage_grid", src, src.shape[0], g.points, g.keys, g.perm, g.n, g.origin, g.cell, g.dims,
                   gt.normals, *crit, self.state, self.ws, self.ws.numel() * 8, corr_idx, corr_d2, self.status,
                   L.stream(self.device))
            self.status |= g.status  # what the target's own keys reported
        else:
            L.call("lnr_icp_stage", src, src.shape[0], tgt, tgt_normals, tgt.shape[0], *crit, self.state, self.ws,
                   self.ws.numel() * 8, corr_idx, corr_d2, L.stream(self.device))
        if self.n_stages >= self.snap.shape[0]:
            self.snap = torch.cat([self.snap, torch.zeros_like(self.snap)])
            self.status_snap = torch.cat([self.status_snap, torch.zeros_like(self.status_snap)])
        self.snap[self.n_stages].copy_(self.state)
        self.status_snap[self.n_stages:self.n_stages + 1].copy_(self.status)
        self.n_stages += 1

    def run(self, src, tgt, tgt_normals, schedule, T0=None, search="brute"):
        self.init(T0)
        if check_search(search) == "grid" and not isinstance(tgt, GridTarget):
            tgt = GridTarget(tgt, tgt_normals)  # one box, one grid per distinct cell for the whole schedule
        for st in schedule:
            self.stage(src, tgt, tgt_normals, st, search=search)

    def read(self):
        """The state after each stage run since ``init``, with the status word as it stood then (one device-to-host
        copy)."""
        n = self.n_stages
        raw = torch.cat([self.snap[:n].reshape(-1), self.status_snap[:n].view(torch.uint8)]).cpu().numpy()
        status = raw[n * STATE_BYTES:].view(np.int32)
        return [_state_dict(raw[i * STATE_BYTES:(i + 1) * STATE_BYTES], status[i]) for i in range(n)]


def icp(src, tgt, tgt_normals, schedule, T0=None, solver=None, search="brute"):
    """Run ``schedule`` on device clouds; returns (T (4, 4) float64, per-stage state dicts).  ``search``: "brute"
    (lnr_icp_stage) or "grid" (lnr_icp_stage_grid; ``tgt`` may be a ``GridTarget``): the same states bit for bit."""
    solver = solver or IcpSolver(src.device)
    solver.run(src, tgt, tgt_normals, schedule, T0, search=search)
    res = solver.read()
    return (res[-1]["T"] if res else (np.eye(4) if T0 is None else np.asarray(T0, np.float64))), res


class Tracker:
    """Frame-to-frame ICP odometry (Tracker.track_frame, src/tracking/tracker.py:167-255)."""

    def __init__(self, settings=None, device="cuda", initial_pose=None):
        self.settings = settings or TrackerSettings()
        self.device = torch.device(device)
        self._solver = IcpSolver(self.device, max_stages=max(1, len(self.settings.schedule)))
        self._ref_points = None  # with search="grid": a GridTarget
        self._ref_normals = None
        self._ref_pose = np.eye(4) if initial_pose is None else PP._np(initial_pose).copy()
        self._ref_time = None
        self.frame_count = 0

    @property
    def reference_pose(self):
        return self._ref_pose.copy()

    def _cloud(self, scan):
        s = self.settings
        ts = scan.get("timestamps")
        target = s.target_uniform_point_count if s.downsample_type == "UNIFORM" else None
        # the index logic runs where the scan lives (no synchronisation for a host scan), the cloud on the device
        start, final, step = frame_indices(ts, scan["distances"].shape[0], s.scan_duration, target)
        dirs = scan["directions"].to(self.device, torch.float32)
        dist = scan["distances"].to(self.device, torch.float32)
        pts = (dirs[:, start:final:step] * dist[start:final:step]).t().contiguous()
        return pts, dirs, dist

    def track(self, scan, time=None):
        """Estimate the pose of ``scan`` (dict: directions (3, P), distances (P,), optional timestamps (P,) and
        sky_directions) and make it the reference for the next one.  ``time``: the scan's middle time on the clock of
        its timestamps (default: the mean of the first and last timestamp, or the frame count without timestamps).
        With motion compensation the scan's directions and distances are replaced by the compensated device tensors;
        with sky rays on, its sky_directions (3, Q) too.  Returns pose (4, 4) float64, fitness, rmse, iterations (one
        entry per stage) and n_points."""
        s = self.settings
        ts = scan.get("timestamps")
        if time is None:
            time = float(ts[0] / 2.0 + ts[-1] / 2.0) if ts is not None and ts.numel() else float(self.frame_count)
        pts, dirs, dist = self._cloud(scan)
        if pts.shape[0] < s.knn:
            raise RuntimeError(f"Tracker: a cloud of {pts.shape[0]} points is smaller than knn={s.knn}")
        grid = s.search == "grid"
        normals = cloud_normals_grid(pts, s.knn) if grid else cloud_normals(pts, s.knn)
        if self._ref_points is None:
            pose = self._ref_pose.copy()
            res = []
        else:
            T, res = icp(pts, self._ref_points, self._ref_normals, s.schedule, solver=self._solver, search=s.search)
            pose = self._ref_pose @ T
            if s.motion_compensation and ts is not None:
                dp3 = dirs.t().contiguous()
                dist = dist.clone() if dist is scan["distances"] else dist
                PP.motion_compensate(dp3, dist, ts.to(self.device, torch.float32).contiguous(),
                                     (self._ref_pose, pose), (self._ref_time, time), pose)
                scan["directions"] = dp3.t()
                scan["distances"] = dist
        if s.compute_sky_rays:
            d = scan["directions"].to(self.device, torch.float32)
            scan["sky_directions"] = PP.sky_rays(d.t().contiguous(), pose).t()
        self._ref_points, self._ref_normals = (GridTarget(pts, normals) if grid else pts), normals
        self._ref_pose, self._ref_time = pose, float(time)
        self.frame_count += 1
        last = res[-1] if res else None
        return dict(pose=pose.copy(), fitness=last["fitness"] if last else 1.0, rmse=last["rmse"] if last else 0.0,
                    iterations=[r["iterations"] for r in res], n_points=int(pts.shape[0]))
