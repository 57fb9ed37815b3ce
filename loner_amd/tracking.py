"""Frame-to-frame ICP tracking on the GPU (src/tracking/tracker.py:167-255): LiDAR odometry without Open3D.

    frame_point_cloud   Frame.build_point_cloud's index logic (src/common/frame.py:105-146)
    cloud_normals       lnr_cloud_normals: Open3D's estimate_normals() with its default KNN(30)
    IcpSolver           lnr_icp_init / lnr_icp_stage around a device-resident lnr_icp_state
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
from . import preprocess as PP

N_SUMS = 27  # J^T J upper triangle (21, row-major) + J^T r (6)


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

    def __post_init__(self):
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


STATE_BYTES = ctypes.sizeof(L.IcpState)


def _state_dict(raw):
    s = L.IcpState.from_buffer_copy(bytes(raw))
    return dict(T=np.array(s.T, np.float64).reshape(4, 4), fitness=float(s.fitness), rmse=float(s.rmse),
                sum_d2=float(s.sum_d2), sums=np.array(s.sums, np.float64), n_corr=int(s.n_corr),
                iterations=int(s.iterations), converged=bool(s.converged))


class IcpSolver:
    """The ICP schedule on one device: state, per-stage snapshots and the workspace are allocated once (the workspace
    grows with the largest source cloud seen).  ``run`` only enqueues; ``read`` is the one synchronisation."""

    def __init__(self, device, max_stages=4):
        self.device = torch.device(device)
        self.state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=self.device)
        self.snap = torch.zeros(max_stages, STATE_BYTES, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(0, dtype=torch.float64, device=self.device)
        self.n_stages = 0

    def init(self, T0=None):
        T = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
        arr = (ctypes.c_double * 16)(*T.reshape(-1).tolist())
        L.call("lnr_icp_init", self.state, arr, L.stream(self.device))
        self.n_stages = 0

    def stage(self, src, tgt, tgt_normals, st, corr_idx=None, corr_d2=None):
        need = int(L.lib().lnr_icp_workspace_bytes(src.shape[0]))
        if self.ws.numel() * 8 < need:
            self.ws = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        L.call("lnr_icp_stage", src, src.shape[0], tgt, tgt_normals, tgt.shape[0], float(st.threshold),
               int(st.max_iterations), float(st.relative_fitness), float(st.relative_rmse), self.state, self.ws,
               self.ws.numel() * 8, corr_idx, corr_d2, L.stream(self.device))
        if self.n_stages >= self.snap.shape[0]:
            self.snap = torch.cat([self.snap, torch.zeros_like(self.snap)])
        self.snap[self.n_stages].copy_(self.state)
        self.n_stages += 1

    def run(self, src, tgt, tgt_normals, schedule, T0=None):
        self.init(T0)
        for st in schedule:
            self.stage(src, tgt, tgt_normals, st)

    def read(self):
        """The state after each stage run since ``init`` (one device-to-host copy)."""
        raw = self.snap[:self.n_stages].cpu().numpy()
        return [_state_dict(r) for r in raw]


def icp(src, tgt, tgt_normals, schedule, T0=None, solver=None):
    """Run ``schedule`` on device clouds; returns (T (4, 4) float64, per-stage state dicts)."""
    solver = solver or IcpSolver(src.device)
    solver.run(src, tgt, tgt_normals, schedule, T0)
    res = solver.read()
    return (res[-1]["T"] if res else (np.eye(4) if T0 is None else np.asarray(T0, np.float64))), res


class Tracker:
    """Frame-to-frame ICP odometry (Tracker.track_frame, src/tracking/tracker.py:167-255)."""

    def __init__(self, settings=None, device="cuda", initial_pose=None):
        self.settings = settings or TrackerSettings()
        self.device = torch.device(device)
        self._solver = IcpSolver(self.device, max_stages=max(1, len(self.settings.schedule)))
        self._ref_points = None
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
        normals = cloud_normals(pts, s.knn)
        if self._ref_points is None:
            pose = self._ref_pose.copy()
            res = []
        else:
            T, res = icp(pts, self._ref_points, self._ref_normals, s.schedule, solver=self._solver)
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
        self._ref_points, self._ref_normals = pts, normals
        self._ref_pose, self._ref_time = pose, float(time)
        self.frame_count += 1
        last = res[-1] if res else None
        return dict(pose=pose.copy(), fitness=last["fitness"] if last else 1.0, rmse=last["rmse"] if last else 0.0,
                    iterations=[r["iterations"] for r in res], n_points=int(pts.shape[0]))
