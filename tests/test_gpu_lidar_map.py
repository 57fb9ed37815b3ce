"""The ground-truth LiDAR map on the GPU (loner_amd.lidar_map): the trajectory deskew, the grid k-nearest-neighbour
search, the statistical outlier filter, build_lidar_map and mask_cloud against their numpy / scipy restatements
(validated on their own in tests/test_lidar_map_ref.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CELLS = (0.1, 0.25, 0.37, 2.0, 50.0)
KS = (1, 20, 64)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def ME(L):
    from loner_amd import map_eval
    return map_eval


@pytest.fixture(scope="module")
def LM(L):
    from loner_amd import lidar_map
    return lidar_map


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ulps(a, b):
    """Distance of float32 arrays in units in the last place (on the ordered-integer line, so across zero too)."""
    def line(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


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
    """The cloud of tests/test_lidar_map_ref.py: a jittered 64 x 64 plane, then 64 points 0.5 .. 5 m above it."""
    rng = np.random.default_rng(seed)
    g = np.arange(64) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    plane = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(4096)], axis=1) + rng.uniform(-0.02, 0.02, (4096, 3))
    out = np.column_stack([rng.uniform(0, 6.3, (64, 2)), rng.uniform(0.5, 5.0, 64)])
    return np.concatenate([plane, out]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- deskew
def check_deskew(LM, p, t, table, min_range=0.5):
    want, wvalid = LM.deskew_points_ref(p, t, table, min_range)
    out, valid = LM.deskew_points(dev(p), dev(t), table, min_range, check=False)
    assert out.dtype == torch.float32 and valid.dtype == torch.bool and tuple(out.shape) == p.shape
    np.testing.assert_array_equal(host(valid), wvalid)
    got = host(out)
    # float64 on both sides: the error of either is far below half a float32 ulp, so only the final rounding (and,
    # through it, sin and cos in their last place) can differ
    u = ulps(got, want)
    print(f"deskew n={len(p)}: {int((u > 0).sum())} of {u.size} coordinates differ, max {int(u.max())} ulp")
    assert u.max() <= 1
    assert (u > 0).sum() <= 1e-3 * u.size
    assert (got[~wvalid] == 0).all()
    out2, valid2 = LM.deskew_points(dev(p), dev(t), table, min_range, check=False)
    assert torch.equal(out, out2) and torch.equal(valid, valid2)
    return out, valid


def test_deskew_matches_reference(LM):
    tum = trajectory()
    table = LM.trajectory_table(tum)
    rng = np.random.default_rng(0)
    n = 5000
    t = rng.uniform(tum[0, 0], tum[-1, 0], n)
    p = (rng.normal(size=(n, 3)) * 20).astype(np.float32)
    t[:9] = tum[:, 0]                                                           # exactly on the knots
    t[9], t[10] = np.nextafter(tum[0, 0], -np.inf), np.nextafter(tum[-1, 0], np.inf)  # just outside both ends
    t[11], t[12] = tum[0, 0] - 3.0, tum[-1, 0] + 3.0
    p[20], p[21], p[22] = (0.5, 0, 0), (0, 0.25, 0), (0, 0, 0)                  # at or below min_range
    p[23] = (0.5, 0, 2.0 ** -10)                                                # just above it
    p[30, 1] = np.nan
    out, valid = check_deskew(LM, p, t, table)
    v = host(valid)
    assert not v[9:13].any() and not v[20:23].any() and v[23] and not v[30] and v[:9].all()
    assert v.sum() == n - 8
    with pytest.raises(RuntimeError, match="nan or inf"):
        LM.deskew_points(dev(p), dev(t), table)
    # without the nan the status stays clear; a nan time raises too
    p[30, 1] = 1.0
    LM.deskew_points(dev(p), dev(t), table)
    t[40] = np.nan
    with pytest.raises(RuntimeError, match="nan or inf"):
        LM.deskew_points(dev(p), dev(t), table)


def test_deskew_small_cases(LM):
    tum = trajectory()
    two = LM.trajectory_table(tum[3:5])
    t = np.array([0.25 * tum[3, 0] + 0.75 * tum[4, 0]])
    p = np.array([[4.0, -7.0, 1.5]], np.float32)
    _, valid = check_deskew(LM, p, t, two)  # n = 1, M = 2
    assert bool(valid[0])
    # nearly equal rotations: the series branch
    from scipy.spatial.transform import Rotation
    q = Rotation.from_rotvec([[0.3, 0.1, -0.2]] * 9) * Rotation.from_rotvec(np.arange(9)[:, None] * [[1e-6, -2e-6, 5e-7]])
    slow = tum.copy()
    slow[:, 4:8] = q.as_quat()
    rng = np.random.default_rng(1)
    check_deskew(LM, (rng.normal(size=(777, 3)) * 20).astype(np.float32), rng.uniform(tum[0, 0], tum[-1, 0], 777),
                 LM.trajectory_table(slow))
    with pytest.raises(ValueError):
        LM.deskew_points(dev(p), dev(t.astype(np.float32)), two)
    with pytest.raises(ValueError):
        LM.deskew_points(dev(p.astype(np.float64)), dev(t), two)
    with pytest.raises(ValueError):
        LM.deskew_points(dev(p), dev(np.zeros(2)), two)


# ---------------------------------------------------------------------------------------------- k nearest neighbours
@pytest.fixture(scope="module")
def search_case(ME, LM):
    """The search case of tests/test_gpu_map_eval.py.  Targets: the filtered quad cloud with a 3 m ball carved out (4 000).
    Sources (at most 6 000): canteen points, the ball's centre, 64 points up to 200 m outside the targets' box, 100 of
    the targets.  The reference for k = 64 is computed once; a smaller k is its prefix."""
    from loner_amd import synthetic as syn
    clouds = {k: ME.scan_world_points(syn.make_window(k, 4), stride=8).numpy() for k in ("quad", "canteen")}
    rng = np.random.default_rng(21)
    t = ME.voxel_down_sample_ref(clouds["quad"], 0.5)
    centre = t[len(t) // 2].astype(np.float64) + (0.0, 0.0, 1.0)
    t = t[np.linalg.norm(t - centre, axis=1) > 3.0]
    t = t[rng.permutation(len(t))[:4000]]  # unsorted: the caller's order is not the grid's
    lo, hi = t.min(axis=0), t.max(axis=0)
    side = rng.integers(0, 2, (64, 3))
    far = np.where(side, hi + rng.uniform(0, 200, (64, 3)), lo - rng.uniform(0, 200, (64, 3)))
    far[:32, 1] = rng.uniform(lo[1], hi[1], 32)  # half of them beside the box, not off a corner
    c = clouds["canteen"]
    s = np.concatenate([c[:: len(c) // 5800][:5800], centre[None], far, t[::40]]).astype(np.float32)
    assert len(s) <= 6000 and len(t) == 4000
    idx, d2 = LM.knn_key_ref(s, t, max(KS))
    return dict(src=s, tgt=t, idx=idx, d2=d2, src_dev=dev(s), tgt_dev=dev(t))


def check_knn(case, k, idx, d2, mean):
    idx, d2, mean = host(idx), host(d2), host(mean)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and mean.dtype == np.float64
    assert idx.shape == (len(case["src"]), k) and d2.shape == idx.shape and mean.shape == (len(case["src"]),)
    np.testing.assert_array_equal(idx, case["idx"][:, :k])
    np.testing.assert_array_equal(d2.view(np.uint32), case["d2"][:, :k].view(np.uint32))
    s, t = case["src"].astype(np.float64), case["tgt"].astype(np.float64)
    # the float64 distances to those winners, added in list order as the kernel adds them
    want = np.add.accumulate(np.sqrt(((s[:, None, :] - t[idx]) ** 2).sum(axis=2)), axis=1)[:, -1] / k
    np.testing.assert_allclose(mean, want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("cell", CELLS)
def test_knn_matches_reference(ME, LM, search_case, cell):
    case = search_case
    grid = ME.NearestGrid(case["tgt_dev"], cell)
    for k in KS:
        idx, d2, mean = LM.knn(case["src_dev"], grid, k)
        check_knn(case, k, idx, d2, mean)
        idx2, d22, mean2 = LM.knn(case["src_dev"], case["tgt_dev"], k, cell)
        assert torch.equal(idx, idx2) and torch.equal(d2, d22) and torch.equal(mean, mean2)
        if k == 1:  # the single-nearest search, bit for bit
            dist, i1, k1 = grid.query(case["src_dev"])
            assert torch.equal(idx[:, 0], i1) and torch.equal(d2[:, 0], k1) and torch.equal(mean, dist)


def test_knn_default_cell_and_small_targets(ME, LM, search_case):
    case = search_case
    s = case["src_dev"]
    for k in (1, 20):
        grid = LM.knn_grid(case["tgt_dev"], k)
        print(f"default cell for k={k}: {grid.cell:.3f} m, dims {host(grid.dims)}")
        check_knn(case, k, *LM.knn(s, case["tgt_dev"], k))
    # a target of exactly k points: every row is the whole target, by distance
    for k in (1, 5, 64):
        few = case["tgt_dev"][100:100 + k].contiguous()
        idx, d2, _ = LM.knn(s, few, k, 0.25)
        ri, rd = LM.knn_key_ref(case["src"], case["tgt"][100:100 + k], k)
        np.testing.assert_array_equal(host(idx), ri)
        np.testing.assert_array_equal(host(d2).view(np.uint32), rd.view(np.uint32))
    # a target of identical points: indices 0 .. k - 1
    same = case["tgt_dev"][3:4].repeat(200, 1).contiguous()
    for cell in (None, 0.25):
        for k in (1, 20, 64):
            idx, d2, _ = LM.knn(s, same, k, cell)
            assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device="cuda").expand(len(s), k))
            assert bool((d2 == d2[:, :1]).all())
    # one source
    idx, d2, mean = LM.knn(s[11:12].contiguous(), case["tgt_dev"], 20, 0.37)
    np.testing.assert_array_equal(host(idx)[0], case["idx"][11, :20])
    np.testing.assert_array_equal(host(d2)[0], case["d2"][11, :20])
    # a query that is a target finds itself first, at distance 0
    idx, d2, _ = LM.knn(case["tgt_dev"], case["tgt_dev"], 3)
    assert torch.equal(idx[:, 0], torch.arange(4000, dtype=torch.int32, device="cuda")) and float(d2[:, 0].max()) == 0.0


def test_knn_error_contract(ME, LM, L):
    d = torch.device("cuda")
    pts = torch.rand(100, 3, device=d)
    for k in (0, 65, 101):
        with pytest.raises(ValueError, match="k="):
            LM.knn(pts, pts, k)
    with pytest.raises(ValueError, match="k="):
        LM.knn(pts, pts[:10].contiguous(), 11)
    with pytest.raises(ValueError, match="float32"):
        LM.knn(pts.double(), pts, 3)
    with pytest.raises(ValueError, match="float32"):
        LM.knn(pts, pts.double(), 3)
    with pytest.raises(ValueError, match="empty"):
        LM.knn(pts[:0], pts, 3)
    with pytest.raises(ValueError, match="empty"):
        LM.knn(pts, pts[:0], 1)
    # the C ABI refuses the same
    grid = ME.NearestGrid(pts, 0.1)
    s = L.stream(d)
    idx = torch.empty(100, 64, dtype=torch.int32, device=d)
    d2 = torch.empty(100, 64, device=d)
    mean = torch.empty(100, dtype=torch.float64, device=d)
    need = int(L.lib().lnr_knn_workspace_bytes(100))
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=d)
    args = lambda k, n_tgt=100, cell=0.1, nbytes=need, out=idx: (  # noqa: E731
        "lnr_knn_search", pts, 100, grid.points, grid.keys, grid.perm, n_tgt, grid.origin, cell, grid.dims, k, ws, nbytes,
        out, d2, mean, grid.status, s)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match="k="):
            L.call(*args(k))
    with pytest.raises(RuntimeError, match="k="):
        L.call(*args(11, n_tgt=10))
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call(*args(1, n_tgt=0))
    with pytest.raises(RuntimeError, match="cell="):
        L.call(*args(3, cell=0.0))
    with pytest.raises(RuntimeError, match="workspace of"):
        L.call(*args(3, nbytes=need - 4))
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call(*args(3, out=None))
    assert L.lib().lnr_knn_workspace_bytes(0) == 0 and L.lib().lnr_dist_moments_workspace_bytes(0) == 0
    # a non-finite query: its row is -1 / inf and the status word says so
    bad = pts.clone()
    bad[17, 1] = float("nan")
    idx, d2, mean = LM.knn(bad, grid, 4, check=False)
    assert int(grid.status.item()) & L.CLOUD_NONFINITE
    assert bool((idx[17] == -1).all()) and bool(torch.isinf(d2[17]).all()) and bool(torch.isinf(mean[17]))
    assert int(idx[16].min()) >= 0 and int(idx[18].min()) >= 0
    with pytest.raises(RuntimeError, match="nan or inf"):
        LM.knn(bad, pts, 4)
    with pytest.raises(RuntimeError, match="nan or inf"):
        LM.knn(pts, bad, 4)


# ---------------------------------------------------------------------------------------------- outlier filter
def test_dist_moments(LM):
    rng = np.random.default_rng(2)
    for n in (1, 4096, 4097, 10000):
        v = rng.uniform(0, 0.2, n)
        v[rng.integers(0, n, n // 10)] = 0.0  # zeros: left out of all three sums
        c = 0.07
        pos = v[v > 0]
        want = np.array([pos.sum(), len(pos), ((pos - c) ** 2).sum()])
        out = host(LM.dist_moments(dev(v), c))
        assert out[1] == want[1]
        np.testing.assert_allclose(out, want, rtol=1e-13, atol=0)
        # the centre from the device: the same bits
        out2 = host(LM.dist_moments(dev(v), torch.tensor([c], dtype=torch.float64, device="cuda")))
        assert np.array_equal(out, out2)
    with pytest.raises(ValueError):
        LM.dist_moments(dev(v.astype(np.float32)))


def test_statistical_outlier_filter(LM):
    p = plane_with_outliers()
    _, want, a_ref, thr_ref = LM.remove_statistical_outlier_ref(p, 20, 1.5, return_distances=True)
    # no mean distance near the threshold: the kept set does not hang on the last digits
    margin = np.abs(a_ref - thr_ref).min() / thr_ref
    print(f"threshold {thr_ref:.6f}, nearest mean distance {margin:.2e} of it away")
    assert margin > 1e-4
    kept, ind, a, thr = LM.remove_statistical_outlier(dev(p), 20, 1.5, return_distances=True)
    assert ind.dtype == torch.int64 and kept.dtype == torch.float32
    np.testing.assert_array_equal(host(ind), want)
    np.testing.assert_array_equal(host(kept), p[want])
    # the float32 key may choose another neighbour at a near-tie: its rounding is <= 4e-7 in d^2, 2e-7 in d
    np.testing.assert_allclose(host(a), a_ref, rtol=1e-6, atol=0)
    assert float(thr) == pytest.approx(thr_ref, rel=1e-6)
    kept2, ind2 = LM.remove_statistical_outlier(dev(p), 20, 1.5)
    assert torch.equal(ind, ind2) and torch.equal(kept, kept2)
    # more neighbours than points: all of them
    _, few = LM.remove_statistical_outlier(dev(p[:10]), 20, 1.5)
    np.testing.assert_array_equal(host(few), LM.remove_statistical_outlier_ref(p[:10], 20, 1.5)[1])
    # identical points: every mean distance is 0, nothing is kept
    kept0, ind0 = LM.remove_statistical_outlier(torch.zeros(5, 3, device="cuda"), 3, 1.5)
    assert tuple(kept0.shape) == (0, 3) and tuple(ind0.shape) == (0,)
    with pytest.raises(ValueError):
        LM.remove_statistical_outlier(dev(p[:1]))
    with pytest.raises(ValueError):
        LM.remove_statistical_outlier(dev(p), 65)
    bad = p.copy()
    bad[5, 0] = np.inf
    with pytest.raises(RuntimeError, match="nan or inf"):
        LM.remove_statistical_outlier(dev(bad))


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def map_case():
    """Three quad scans strided to about 5 000 returns each, per-point times over 0.1 s of a moving trajectory, and one
    scan after the trajectory's end."""
    from loner_amd import synthetic as syn
    from scipy.spatial.transform import Rotation
    poses = syn.keyframe_poses("quad", 7, None)
    tum = np.array([[1.7e9 + 0.5 * i, *T[:3, 3], *Rotation.from_matrix(T[:3, :3]).as_quat()]
                    for i, T in enumerate(poses)])
    scans = []
    for i, s in enumerate(syn.make_window("quad", 3, seed=4, poses=poses[1:6:2])):
        stride = max(s["distances"].shape[0] // 5000, 1)
        d, r = s["directions"][:, ::stride].contiguous(), s["distances"][::stride].contiguous()
        assert 4000 <= r.shape[0] <= 7000
        scans.append(dict(directions=d, distances=r, time=float(tum[1 + 2 * i, 0]),
                          timestamps=torch.linspace(0.0, 0.1, r.shape[0], dtype=torch.float64)))
    scans.append(dict(scans[0], time=float(tum[-1, 0]) + 1.0))
    return scans, tum


def covered(a, b, tol):
    """The fraction of a's points without a point of b within tol."""
    from scipy.spatial import cKDTree
    return float((cKDTree(b.astype(np.float64)).query(a.astype(np.float64))[0] > tol).mean())


def test_build_lidar_map_end_to_end(ME, LM, map_case):
    scans, tum = map_case
    voxel = 0.1
    cloud = LM.build_lidar_map(scans, tum, voxel_size=voxel, min_range=0.5)
    assert cloud.is_cuda and cloud.dtype == torch.float32 and cloud.shape[0] > 5000
    # the same public functions by hand: bit for bit
    table = LM.trajectory_table(tum)
    parts = []
    for s in scans[:3]:
        p, t = LM.scan_points_and_times(s, table, 0.5)
        w, valid = LM.deskew_points(dev(p), dev(t), table, 0.5)
        assert bool(valid.all())
        parts.append(ME.voxel_down_sample(w, voxel))
    assert LM.scan_points_and_times(scans[3], table, 0.5) is None
    merged = torch.cat(parts)
    assert torch.equal(cloud, ME.voxel_down_sample(merged, voxel)) and cloud.shape[0] < merged.shape[0]
    assert torch.equal(cloud, LM.build_lidar_map(scans, tum, voxel_size=voxel, min_range=0.5))
    # the deskew moved the returns: one pose per scan gives another cloud
    rigid = [dict(s, timestamps=None) for s in scans]
    assert not torch.equal(cloud, LM.build_lidar_map(rigid, tum, voxel_size=voxel))
    # the float64 restatement: a 1-ulp deskew difference can move a return across a voxel face, so the clouds agree
    # point for point within 1e-3 voxel up to 0.1 % of them
    ref = LM.build_lidar_map_ref(scans, tum, voxel_size=voxel, min_range=0.5)
    got = host(cloud)
    miss = covered(got, ref, 1e-3 * voxel), covered(ref, got, 1e-3 * voxel)
    print(f"{len(got)} points (reference {len(ref)}); without a partner within 1e-3 voxel: {miss}")
    assert max(miss) <= 1e-3
    # with the outlier filter: what remove_statistical_outlier keeps of that cloud
    filtered = LM.build_lidar_map(scans, tum, voxel_size=voxel, min_range=0.5, outlier_filter=True)
    assert torch.equal(filtered, LM.remove_statistical_outlier(cloud)[0]) and 0 < filtered.shape[0] < cloud.shape[0]
    assert tuple(LM.build_lidar_map(scans[3:], tum).shape) == (0, 3)


def test_mask_cloud(ME, LM, map_case):
    scans, tum = map_case
    rec = host(LM.build_lidar_map(scans[:2], tum, voxel_size=0.2))
    table = LM.trajectory_table(tum)
    gt = np.concatenate([LM.deskew_points_ref(*LM.scan_points_and_times(s, table, 0.5), table)[0] for s in scans[:3]])
    thr = 0.1
    T = np.eye(4)
    T[:3, 3] = (0.03, -0.02, 0.01)
    for tf in (None, T):
        kept_ref, mask_ref = LM.mask_cloud_ref(gt, rec, thr, tf)
        moved = rec if tf is None else ME.transform_points_ref(rec, tf)
        dist = ME.nearest_distances_ref(gt, moved)[0]
        assert np.abs(dist - thr).min() > 1e-6 * thr  # no distance on the threshold: the mask is exact
        assert 0 < mask_ref.sum() < len(gt)
        kept, mask = LM.mask_cloud(dev(gt), dev(rec), thr, tf)
        np.testing.assert_array_equal(host(mask), mask_ref)
        np.testing.assert_array_equal(host(kept), kept_ref)
