"""The numpy / scipy restatements of loner_amd.lidar_map on their own (CPU only): they are the oracle of
tests/test_gpu_lidar_map.py.  The deskew against scipy's Slerp and np.interp, the float32 search key against a k-d
tree, the outlier rule on a plane with scattered points, the timestamp and scan-drop rules on hand-made cases."""
import numpy as np
import pytest
import torch

from loner_amd import _lib as L
from loner_amd import lidar_map as LM


def trajectory(m=9, seed=3, t0=1.7e9):
    """TUM rows: m poses 0.5 .. 1.5 s apart, rotations up to about 1 rad and a few metres between them."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    t = t0 + np.cumsum(rng.uniform(0.5, 1.5, m))
    xyz = np.cumsum(rng.uniform(-2, 2, (m, 3)), axis=0)
    rot = Rotation.identity()
    quats = []
    for _ in range(m):
        v = rng.normal(size=3)
        rot = rot * Rotation.from_rotvec(v / np.linalg.norm(v) * rng.uniform(0.2, 1.0))
        quats.append(rot.as_quat())
    return np.column_stack([t, xyz, np.array(quats)])


def plane_with_outliers(seed=11):
    """A 64 x 64 plane at 0.1 m spacing, jittered by 2 cm, then 64 points scattered 0.5 .. 5 m above it."""
    rng = np.random.default_rng(seed)
    g = np.arange(64) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    plane = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(4096)], axis=1) + rng.uniform(-0.02, 0.02, (4096, 3))
    out = np.column_stack([rng.uniform(0, 6.3, (64, 2)), rng.uniform(0.5, 5.0, 64)])
    return np.concatenate([plane, out]).astype(np.float32)


def scipy_deskew(tum, p, t):
    from scipy.spatial.transform import Rotation, Slerp
    R = Slerp(tum[:, 0], Rotation.from_quat(tum[:, 4:8]))(t).as_matrix()
    x = np.stack([np.interp(t, tum[:, 0], tum[:, 1 + a]) for a in range(3)], axis=1)
    return np.einsum("nij,nj->ni", R, p.astype(np.float64)) + x


def test_deskew_matches_scipy():
    tum = trajectory()
    table = LM.trajectory_table(tum)
    assert len(table) == 9 and table.rot.shape == (9, 9) and table.rel.shape == (8, 3)
    assert 0.8 < np.linalg.norm(table.rel, axis=1).max() <= 1.0  # up to about 1 rad between poses
    rng = np.random.default_rng(0)
    t = np.concatenate([rng.uniform(tum[0, 0], tum[-1, 0], 3000), tum[:, 0]])  # random times and every knot
    p = (rng.normal(size=(len(t), 3)) * 20).astype(np.float32)
    out, valid = LM.deskew_points_ref(p, t, table, 0.5, dtype=np.float64)
    assert valid.all()
    assert np.abs(out - scipy_deskew(tum, p, t)).max() <= 1e-12
    # on a knot the pose is the knot's
    i = 4
    Rm = table.rot[i].reshape(3, 3)
    o, _ = LM.deskew_points_ref(p[:5], np.full(5, tum[i, 0]), table, 0.5, dtype=np.float64)
    assert np.abs(o - (p[:5].astype(np.float64) @ Rm.T + tum[i, 1:4])).max() <= 1e-12
    # the rounded form is the float64 one rounded once
    o32, _ = LM.deskew_points_ref(p, t, table, 0.5)
    assert o32.dtype == np.float32 and np.array_equal(o32, out.astype(np.float32))


def test_deskew_small_angles_and_interval_rule():
    from scipy.spatial.transform import Rotation
    tum = trajectory(5)
    # nearly equal rotations: the series branch
    q = Rotation.from_rotvec([[0.3, 0.1, -0.2]] * 5) * Rotation.from_rotvec(np.arange(5)[:, None] * [[1e-6, -2e-6, 5e-7]])
    tum[:, 4:8] = q.as_quat()
    table = LM.trajectory_table(tum)
    assert np.linalg.norm(table.rel, axis=1).max() < 1e-4
    rng = np.random.default_rng(1)
    t = rng.uniform(tum[0, 0], tum[-1, 0], 500)
    p = (rng.normal(size=(500, 3)) * 20).astype(np.float32)
    out, valid = LM.deskew_points_ref(p, t, table, 0.5, dtype=np.float64)
    assert valid.all() and np.abs(out - scipy_deskew(tum, p, t)).max() <= 1e-12
    # searchsorted(left) - 1 with the first knot in interval 0: scipy's own rule
    T = table.t
    probe = np.concatenate([T, np.nextafter(T, np.inf)[:-1], np.nextafter(T, -np.inf)[1:]])
    i = np.clip(np.searchsorted(T, probe, "left") - 1, 0, len(T) - 2)
    want = np.searchsorted(T, probe) - 1
    want[probe == T[0]] = 0
    np.testing.assert_array_equal(i, want)


def test_deskew_validity():
    tum = trajectory()
    table = LM.trajectory_table(tum)
    mid = 0.5 * (tum[2, 0] + tum[3, 0])
    p = np.array([[3, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0.5, 0, 2.0 ** -10], [3, 0, 0], [3, 0, 0], [np.nan, 0, 0],
                  [3, 0, 0], [3, 0, 0], [3, 0, 0]], np.float32)
    t = np.array([mid, mid, mid, mid, np.nextafter(tum[0, 0], -np.inf), np.nextafter(tum[-1, 0], np.inf), mid, np.nan,
                  tum[0, 0], tum[-1, 0]])
    out, valid = LM.deskew_points_ref(p, t, table, 0.5)
    # range exactly 0.5 is not > 0.5 (strict); just outside either end is never extrapolated; the ends are inside
    np.testing.assert_array_equal(valid, [1, 0, 0, 1, 0, 0, 0, 0, 1, 1])
    assert (out[~valid] == 0).all() and np.isfinite(out).all()
    for bad in (tum[:1], tum[:, :7], tum[::-1]):
        with pytest.raises(ValueError):
            LM.trajectory_table(bad)
    nan = tum.copy()
    nan[3, 2] = np.nan
    with pytest.raises(ValueError, match="nan or inf"):
        LM.trajectory_table(nan)


def test_knn_key_matches_kdtree_and_orders_duplicates():
    rng = np.random.default_rng(4)
    g = np.arange(40) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    t = (np.stack([x.reshape(-1), y.reshape(-1), np.zeros(1600)], axis=1) + rng.uniform(-0.03, 0.03, (1600, 3)))
    t = t.astype(np.float32)
    s = np.concatenate([t[::7], (rng.uniform(0, 4, (200, 3)) * (1, 1, 0.2)).astype(np.float32)])
    idx, d2 = LM.knn_key_ref(s, t, 20)
    assert idx.shape == (len(s), 20) and idx.dtype == np.int32 and d2.dtype == np.float32
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    dist, tree = LM.knn_ref(s, t, 20)
    np.testing.assert_array_equal(np.sort(idx, axis=1), np.sort(tree, axis=1))  # the same neighbour sets
    np.testing.assert_allclose(np.sqrt(d2.astype(np.float64)), dist, rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(idx[: len(t[::7]), 0], np.arange(len(t))[::7])  # a target finds itself first
    # k = 1 is map_eval's key
    from loner_amd import map_eval as ME
    i1, k1 = ME.nn_key_ref(s, t)
    np.testing.assert_array_equal(idx[:, 0], i1)
    np.testing.assert_array_equal(d2[:, 0].view(np.uint32), k1.view(np.uint32))
    # duplicates: ascending indices
    same = np.repeat(t[5:6], 50, axis=0)
    idx, d2 = LM.knn_key_ref(s[:10], same, 8)
    np.testing.assert_array_equal(idx, np.tile(np.arange(8), (10, 1)))
    two = np.concatenate([same[:3], t[9:10], same[:3]])
    idx, _ = LM.knn_key_ref(t[5:6], two, 7)
    np.testing.assert_array_equal(idx[0], [0, 1, 2, 4, 5, 6, 3])
    for k in (0, 8):
        with pytest.raises(ValueError):
            LM.knn_key_ref(s[:10], two, k)


def test_statistical_outlier_filter():
    p = plane_with_outliers()
    kept, ind, a, thr = LM.remove_statistical_outlier_ref(p, 20, 1.5, return_distances=True)
    assert ind.dtype == np.int64 and (np.diff(ind) > 0).all() and np.array_equal(kept, p[ind])
    assert set(range(4096)) <= set(ind.tolist())  # every plane point stays
    assert (ind >= 4096).sum() <= 4               # at least 60 of the 64 scattered points go
    # the rule, from its parts
    n = len(p)
    mu = a.sum() / n
    assert thr == pytest.approx(mu + 1.5 * np.sqrt(((a - mu) ** 2).sum() / (n - 1)), rel=1e-13)
    np.testing.assert_array_equal(ind, np.flatnonzero(a < thr))
    assert (a > 0).all()
    # a duplicated cloud: every mean distance is 0 and nothing is kept (0 < a fails)
    _, none = LM.remove_statistical_outlier_ref(np.zeros((5, 3), np.float32), 3, 1.5)
    assert len(none) == 0
    # more neighbours than points: all of them
    _, few = LM.remove_statistical_outlier_ref(p[:10], 20, 1.5)
    want = LM.knn_ref(p[:10], p[:10], 10)[0].mean(axis=1)
    np.testing.assert_array_equal(few, np.flatnonzero(want < LM.outlier_threshold_ref(want, 1.5)))
    with pytest.raises(ValueError):
        LM.remove_statistical_outlier_ref(p[:1])


def test_normalise_point_times():
    stamp = 1.7e9
    # offsets in seconds from the stamp
    np.testing.assert_array_equal(LM.normalise_point_times([0.0, 0.05, 0.1], stamp), stamp + np.array([0.0, 0.05, 0.1]))
    # offsets in nanoseconds
    np.testing.assert_array_equal(LM.normalise_point_times([0, 5e7, 1e8], stamp),
                                  stamp + np.array([0.0, 5e7, 1e8]) * 1e-9)
    # absolute seconds of another clock: re-based on the first
    got = LM.normalise_point_times([500.0, 500.05, 500.1], stamp)
    np.testing.assert_array_equal(got, np.array([500.0, 500.05, 500.1]) - 500.0 + stamp)
    # absolute nanoseconds: scaled, then re-based
    ns = np.array([1.6e18, 1.6e18 + 5e7])
    np.testing.assert_array_equal(LM.normalise_point_times(ns, stamp), ns * 1e-9 - ns[0] * 1e-9 + stamp)
    # a first offset of exactly 1e-2 is not below 1e-2: re-based
    np.testing.assert_array_equal(LM.normalise_point_times([1e-2, 2e-2], 10.0), np.array([1e-2, 2e-2]) - 1e-2 + 10.0)
    ts = np.array([0.0, 0.1])
    LM.normalise_point_times(ts, 1.0)
    np.testing.assert_array_equal(ts, [0.0, 0.1])  # the input is not modified


def test_scan_drop_rules():
    tum = trajectory()
    table = LM.trajectory_table(tum)
    first, last = tum[0, 0], tum[-1, 0]
    d = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0]])
    r = torch.tensor([2.0, 0.4, 3.0, 0.5])  # ranges 2, 0.4, 3, 0.5: the second and the fourth are not > 0.5

    def scan(time, ts=None):
        s = dict(directions=d, distances=r, time=time)
        if ts is not None:
            s["timestamps"] = torch.tensor(ts, dtype=torch.float64)
        return s

    p, t = LM.scan_points_and_times(scan(first + 1.0, [0.0, 0.01, 0.02, 0.03]), table, 0.5)
    np.testing.assert_array_equal(p, [[2, 0, 0], [0, 0, 3]])
    np.testing.assert_array_equal(t, first + 1.0 + np.array([0.0, 0.02]))
    # without per-point times: the stamp
    p, t = LM.scan_points_and_times(scan(first + 1.0), table, 0.5)
    np.testing.assert_array_equal(t, [first + 1.0] * 2)
    # the rules read the returns that pass the range test: their first time, 0.02, is not below 1e-2: re-based
    p, t = LM.scan_points_and_times(scan(first + 1.0, [0.02, 0.0, 0.05, 0.03]), table, 0.5)
    np.testing.assert_array_equal(t, np.array([0.02, 0.05]) - 0.02 + (first + 1.0))
    # :65-66 the stamp outside the trajectory
    assert LM.scan_points_and_times(scan(first - 1e-3), table, 0.5) is None
    assert LM.scan_points_and_times(scan(last + 1e-3), table, 0.5) is None
    assert LM.scan_points_and_times(scan(first), table, 0.5) is not None
    assert LM.scan_points_and_times(scan(last), table, 0.5) is not None
    # :102-103 a time beyond the trajectory's end
    assert LM.scan_points_and_times(scan(last - 0.01, [0.0, 0.0, 0.02, 0.0]), table, 0.5) is None
    assert LM.scan_points_and_times(scan(last - 0.01, [0.0, 0.02, 0.005, 0.02]), table, 0.5) is not None
    # no return beyond the minimum range
    assert LM.scan_points_and_times(scan(first + 1.0), table, 3.0) is None
    with pytest.raises(ValueError, match="timestamps"):
        LM.scan_points_and_times(scan(first + 1.0, [0.0, 0.1]), table, 0.5)


def test_build_and_mask_ref():
    tum = trajectory()
    table = LM.trajectory_table(tum)
    rng = np.random.default_rng(8)
    scans = []
    for s in range(3):
        d = rng.normal(size=(3, 400))
        d /= np.linalg.norm(d, axis=0)
        scans.append(dict(directions=torch.from_numpy(d).float(), distances=torch.from_numpy(rng.uniform(0.3, 9, 400)).float(),
                          time=float(tum[1 + 2 * s, 0]), timestamps=torch.linspace(0, 0.1, 400, dtype=torch.float64)))
    scans.append(dict(scans[0], time=float(tum[-1, 0]) + 5.0))  # dropped
    cloud = LM.build_lidar_map_ref(scans, tum, voxel_size=0.5, min_range=0.5)
    parts = []
    for s in scans[:3]:
        p, t = LM.scan_points_and_times(s, table, 0.5)
        w, v = LM.deskew_points_ref(p, t, table, 0.5)
        assert v.all() and len(p) < 400
        parts.append(w)
    from loner_amd import map_eval as ME
    want = ME.voxel_down_sample_ref(np.concatenate([ME.voxel_down_sample_ref(w, 0.5) for w in parts]), 0.5)
    np.testing.assert_array_equal(cloud, want)
    assert LM.build_lidar_map_ref(scans[3:], tum).shape == (0, 3)
    # the mask: strictly below the threshold, after the optional transform
    gt = np.array([[0, 0, 0], [0.05, 0, 0], [0.1, 0, 0], [1, 0, 0]], np.float32)
    rec = np.zeros((1, 3), np.float32)
    kept, mask = LM.mask_cloud_ref(gt, rec, 0.1)
    np.testing.assert_array_equal(mask, [1, 1, 0, 0])  # float32(0.1) > 0.1: not below
    np.testing.assert_array_equal(kept, gt[:2])
    T = np.eye(4)
    T[0, 3] = 1.0
    np.testing.assert_array_equal(LM.mask_cloud_ref(gt, rec, 0.1, T)[1], [0, 0, 0, 1])


def test_header_declares_the_new_functions():
    for name in ("lnr_trajectory_transform", "lnr_knn_workspace_bytes", "lnr_knn_search",
                 "lnr_dist_moments_workspace_bytes", "lnr_dist_moments"):
        assert name in L.FUNCTIONS, name
    assert L.KNN_MAX_K == 64
    f = L.FUNCTIONS["lnr_knn_search"]
    assert [n for _, n in f.params][:10] == ["src", "n_src", "tgt_sorted", "tgt_keys", "tgt_perm", "n_tgt", "origin",
                                             "cell", "dims", "k"]
    assert L.lib().lnr_knn_workspace_bytes(0) == 0 and L.lib().lnr_knn_workspace_bytes(100) == 408
    assert L.lib().lnr_dist_moments_workspace_bytes(4097) == 48
