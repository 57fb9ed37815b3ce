"""Map evaluation on the GPU (loner_amd.map_eval): the voxel filter, the grid nearest-neighbour search, the distance
statistics, compare_point_clouds and LidarMapRenderer against their numpy / scipy restatements (validated on their own
in tests/test_map_eval_ref.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CELLS = (0.1, 0.25, 0.37, 2.0, 50.0)


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


@pytest.fixture(scope="module")
def clouds(ME):
    """World points of four synthetic scans, strided: 3e4 .. 7e4 points each, float32 numpy."""
    from loner_amd import synthetic as syn
    out = {k: ME.scan_world_points(syn.make_window(k, 4), stride=8).numpy() for k in ("quad", "canteen")}
    for k, v in out.items():
        print(f"{k}: {len(v)} points")
        assert 3e4 <= len(v) <= 7e4
    return out


# ---------------------------------------------------------------------------------------------- voxel filter
def check_voxel(ME, p, voxel):
    rm, rc, rk = ME.voxel_down_sample_ref(p, voxel, return_counts=True, return_keys=True)
    m, c, k = ME.voxel_filter(dev(p), voxel, return_keys=True)
    assert m.dtype == torch.float32 and c.dtype == torch.int32 and k.dtype == torch.int64
    np.testing.assert_array_equal(host(k), rk)  # the voxel set and its order
    np.testing.assert_array_equal(host(c), rc)
    # the float64 error of either sum is far below half a float32 ulp: only the final rounding can differ
    assert ulps(host(m), rm).max() <= 1
    return m, c, k, rc


@pytest.mark.parametrize("voxel", [0.05, 1.0])
def test_voxel_filter_matches_reference(ME, L, clouds, voxel):
    p = clouds["quad"]
    m, c, k, rc = check_voxel(ME, p, voxel)
    print(f"voxel {voxel}: {len(rc)} voxels, max {rc.max()} points, median {np.median(rc)}")
    if voxel == 1.0:
        assert rc.max() > 2 * L.CLOUD_VOXEL_CHUNK  # at least three chunks in one voxel: the split path
    # again: bit for bit
    m2, c2 = ME.voxel_down_sample(dev(p), voxel, return_counts=True)
    assert torch.equal(m, m2) and torch.equal(c, c2)
    # a permuted input: the same voxels and counts; a sum in another order may round the other way
    perm = np.random.default_rng(5).permutation(len(p))
    m3, c3, k3 = ME.voxel_filter(dev(p[perm]), voxel, return_keys=True)
    assert torch.equal(k, k3) and torch.equal(c, c3)
    assert ulps(host(m3), host(m)).max() <= 1


def test_voxel_filter_edge_cases(ME):
    rng = np.random.default_rng(9)
    one = np.array([[1.5, -2.25, 3.0]], np.float32)
    m, c, _, _ = check_voxel(ME, one, 0.3)
    np.testing.assert_array_equal(host(m), one)
    # all points in one voxel
    m, c, _, _ = check_voxel(ME, (rng.uniform(0, 0.01, (100, 3)) + 7).astype(np.float32), 1.0)
    assert tuple(m.shape) == (1, 3) and int(c[0]) == 100
    # duplicated points, more than two chunks of one: the mean of copies is the point itself
    pt = np.array([[0.1, -0.2, 0.3], [5.0, 5.0, 5.0]], np.float32)
    m, c, _, _ = check_voxel(ME, np.repeat(pt, [130, 3], axis=0), 0.5)
    np.testing.assert_array_equal(host(m), pt)
    np.testing.assert_array_equal(host(c), [130, 3])
    # negative coordinates
    check_voxel(ME, rng.uniform(-50, -10, (3000, 3)).astype(np.float32), 0.7)
    # points exactly on voxel faces: multiples of 0.125 at voxel 0.25 (origin and quotients exact in float64)
    g = np.arange(-8, 9, dtype=np.float32) * 0.125
    faces = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    m, c, _, rc = check_voxel(ME, faces, 0.25)
    assert len(rc) == 9 ** 3 and rc.max() == 8 and rc.min() == 1


# ---------------------------------------------------------------------------------------------- nearest neighbour
@pytest.fixture(scope="module")
def search_case(ME, clouds):
    """Targets: the filtered quad cloud with a 3 m ball carved out (at most 4 000).  Sources (at most 6 000): canteen
    points, the ball's centre, 64 points up to 200 m outside the targets' box, 100 of the targets."""
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
    from scipy.spatial import cKDTree
    dist, _ = cKDTree(t.astype(np.float64)).query(s.astype(np.float64))
    idx, d2 = ME.nn_key_ref(s, t)
    assert dist[5800] > 2.9  # the ball's centre
    return dict(src=s, tgt=t, dist=dist, idx=idx, d2=d2, src_dev=dev(s), tgt_dev=dev(t))


def check_search(case, dist, idx, d2):
    dist, idx, d2 = host(dist), host(idx), host(d2)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and d2.dtype == np.float32
    np.testing.assert_array_equal(idx, case["idx"])
    np.testing.assert_array_equal(d2.view(np.uint32), case["d2"].view(np.uint32))
    # the key's rounding is <= 4e-7 in d^2, hence 2e-7 in d: the winner is the k-d tree's up to that
    assert (np.abs(dist - case["dist"]) <= 1e-6 * case["dist"]).all()
    s, t = case["src"].astype(np.float64), case["tgt"].astype(np.float64)
    np.testing.assert_allclose(dist, np.sqrt(((s - t[idx]) ** 2).sum(axis=1)), rtol=1e-15, atol=0)


@pytest.mark.parametrize("cell", CELLS)
def test_nearest_matches_reference(ME, search_case, cell):
    case = search_case
    dist, idx, d2 = ME.nearest_distances(case["src_dev"], case["tgt_dev"], cell)
    check_search(case, dist, idx, d2)
    dist2, idx2, d22 = ME.nearest_distances(case["src_dev"], case["tgt_dev"], cell)
    assert torch.equal(dist, dist2) and torch.equal(idx, idx2) and torch.equal(d2, d22)


def test_nearest_default_cell_and_small_targets(ME, search_case):
    case = search_case
    grid = ME.NearestGrid(case["tgt_dev"])
    print(f"default cell {grid.cell:.3f} m, dims {host(grid.dims)}")
    check_search(case, *grid.query(case["src_dev"]))
    s = case["src_dev"]
    # a target of one point
    dist, idx, _ = ME.nearest_distances(s, case["tgt_dev"][7:8].contiguous(), 0.25)
    assert int(idx.abs().max()) == 0
    want = np.sqrt(((case["src"].astype(np.float64) - case["tgt"][7].astype(np.float64)) ** 2).sum(axis=1))
    np.testing.assert_allclose(host(dist), want, rtol=1e-15)
    # a target of identical points: the lowest index
    same = case["tgt_dev"][3:4].repeat(200, 1).contiguous()
    for cell in (None, 0.25):
        dist, idx, _ = ME.nearest_distances(s, same, cell)
        assert int(idx.abs().max()) == 0
    # one source
    dist, idx, d2 = ME.nearest_distances(s[11:12].contiguous(), case["tgt_dev"], 0.37)
    assert int(idx[0]) == case["idx"][11] and host(d2)[0] == case["d2"][11]


# ---------------------------------------------------------------------------------------------- errors
def test_error_contract(ME, L):
    d = torch.device("cuda")
    s = L.stream(d)
    pts = torch.rand(100, 3, device=d)
    origin = torch.zeros(3, dtype=torch.float64, device=d)
    keys = torch.empty(100, dtype=torch.int64, device=d)
    status = torch.zeros(1, dtype=torch.int32, device=d)
    heads = torch.empty(100, dtype=torch.int32, device=d)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_cloud_cell_keys", pts, 100, None, 0.1, keys, status, s)
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="cell="):
            L.call("lnr_cloud_cell_keys", pts, 100, origin, cell, keys, status, s)
    for n in (0, (1 << 27) + 1):
        with pytest.raises(RuntimeError, match="outside"):
            L.call("lnr_cloud_cell_keys", pts, n, origin, 0.1, keys, status, s)
        with pytest.raises(RuntimeError, match="outside"):
            L.call("lnr_voxel_heads", keys, n, heads, s)
        assert L.lib().lnr_voxel_workspace_bytes(n, 1) == 0 and L.lib().lnr_dist_stats_workspace_bytes(n) == 0
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_voxel_heads", None, 100, heads, s)
    scan = torch.arange(1, 101, dtype=torch.int64, device=d)
    perm = torch.arange(100, dtype=torch.int64, device=d)
    need = int(L.lib().lnr_voxel_workspace_bytes(100, 100))
    assert need > 0 and L.lib().lnr_voxel_workspace_bytes(100, 101) == 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=d)
    means = torch.empty(100, 3, device=d)
    with pytest.raises(RuntimeError, match="workspace of"):
        L.call("lnr_voxel_reduce", pts, perm, scan, 100, 100, ws, need - 8, means, None, s)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_voxel_reduce", pts, perm, scan, 100, 100, None, need, means, None, s)
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call("lnr_voxel_reduce", pts, perm, scan, 100, 101, ws, need, means, None, s)
    dims = torch.ones(3, dtype=torch.int32, device=d)
    idx = torch.empty(100, dtype=torch.int32, device=d)
    d2 = torch.empty(100, device=d)
    dist = torch.empty(100, dtype=torch.float64, device=d)
    perm32 = perm.int()
    nn_need = int(L.lib().lnr_nn_workspace_bytes(100))
    assert 0 < nn_need <= need and L.lib().lnr_nn_workspace_bytes(0) == 0
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_nn_search", pts, 100, pts, keys, perm32, 100, origin, 0.1, None, ws, need, idx, d2, dist, status,
               s)
    with pytest.raises(RuntimeError, match="cell="):
        L.call("lnr_nn_search", pts, 100, pts, keys, perm32, 100, origin, 0.0, dims, ws, need, idx, d2, dist, status,
               s)
    with pytest.raises(RuntimeError, match="bad sizes"):
        L.call("lnr_nn_search", pts, 100, pts, keys, perm32, 0, origin, 0.1, dims, ws, need, idx, d2, dist, status, s)
    with pytest.raises(RuntimeError, match="workspace of"):
        L.call("lnr_nn_search", pts, 100, pts, keys, perm32, 100, origin, 0.1, dims, ws, nn_need - 4, idx, d2, dist,
               status, s)
    out = torch.empty(2, dtype=torch.float64, device=d)
    with pytest.raises(RuntimeError, match="workspace of"):
        L.call("lnr_dist_stats", dist, 100, 0.1, ws, 8, out, s)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_dist_stats", dist, 100, 0.1, ws, need, None, s)
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_grid_limit_and_nan_raise(ME, L):
    far = torch.tensor([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0]], device="cuda")
    with pytest.raises(RuntimeError, match="2\\^21"):
        ME.voxel_down_sample(far, 0.05)
    assert tuple(ME.voxel_down_sample(far, 1.0).shape) == (2, 3)
    bad = torch.rand(50, 3, device="cuda")
    bad[17, 1] = float("nan")
    with pytest.raises(RuntimeError, match="nan or inf"):
        ME.voxel_down_sample(bad, 0.05)
    ok = torch.rand(50, 3, device="cuda")
    with pytest.raises(RuntimeError, match="nan or inf"):
        ME.nearest_distances(bad, ok, 0.1)
    with pytest.raises(RuntimeError, match="nan or inf"):
        ME.nearest_distances(ok, bad, 0.1)
    with pytest.raises(RuntimeError, match="nan or inf"):
        ME.nearest_distances(ok, bad)
    with pytest.raises(RuntimeError, match="2\\^21"):
        ME.nearest_distances(ok, far, 0.05)
    # the default cell fits any box; the status word reports, the outputs stay defined
    dist, idx, _ = ME.nearest_distances(ok, far)
    assert int(idx.max()) == 0 and float(dist.max()) < 2.0
    torch.cuda.synchronize()


def test_distance_stats(ME):
    rng = np.random.default_rng(2)
    for n in (1, 4096, 4097, 70001):
        d = rng.uniform(0, 0.2, n)
        out = host(ME.distance_stats(dev(d), 0.1))
        assert out[1] == (d > 0.1).sum()
        assert out[0] == pytest.approx(d.sum(), rel=1e-13)
        assert np.array_equal(out, host(ME.distance_stats(dev(d), 0.1)))


# ---------------------------------------------------------------------------------------------- compare_point_clouds
def lattice(n=20, dz=0.0):
    g = np.arange(n, dtype=np.float64) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, dz)], axis=1).astype(np.float32)


def test_compare_lattice(ME):
    a, b = dev(lattice()), dev(lattice(dz=0.07))
    s = ME.compare_point_clouds(a, b, f_score_threshold=0.1, voxel_size=0.05, align=False)
    assert set(s) == {"accuracy", "completion", "chamfer_distance", "recall", "precision", "f-score", "num_points"}
    assert s["num_points"] == 400
    assert s["accuracy"] == pytest.approx(0.07, rel=1e-6) and s["completion"] == pytest.approx(0.07, rel=1e-6)
    assert s["chamfer_distance"] == pytest.approx(0.14, rel=1e-6)
    assert s["precision"] == 1.0 and s["recall"] == 1.0 and s["f-score"] == pytest.approx(1.0, abs=1e-8)
    s = ME.compare_point_clouds(a, b, f_score_threshold=0.05, voxel_size=0.05, align=False)
    assert s["precision"] == 0.0 and s["recall"] == 0.0 and s["f-score"] == 0.0
    with pytest.raises(ValueError, match="2\\^17"):
        ME.compare_point_clouds(a, b, align_max_points=(1 << 17) + 1)


def test_compare_unaligned_matches_reference(ME, clouds):
    p = clouds["quad"]
    est, gt = p[0::2], p[1::2]
    thr, voxel = 0.1, 0.05
    ref, acc, comp, _ = ME.compare_point_clouds_ref(est, gt, thr, voxel, align=False, return_distances=True)
    # inputs for which no reference distance sits on the threshold: the counts are then exact
    assert np.abs(acc - thr).min() > 1e-6 * thr and np.abs(comp - thr).min() > 1e-6 * thr
    got = ME.compare_point_clouds(dev(est), dev(gt), thr, voxel, align=False)
    print(ref, got)
    assert got["num_points"] == ref["num_points"]
    for k in ("accuracy", "completion", "chamfer_distance"):
        assert got[k] == pytest.approx(ref[k], rel=1e-6)
    for k in ("precision", "recall", "f-score"):  # from equal counts
        assert got[k] == pytest.approx(ref[k], rel=1e-12)
    assert 0.0 < ref["precision"] < 1.0 and 0.0 < ref["recall"] < 1.0


def test_compare_aligned_matches_reference(ME, clouds):
    est = clouds["canteen"][::2]
    a = np.deg2rad(0.3)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (0.02 / np.sqrt(3),) * 3
    gt = ME.transform_points_ref(est, T)
    assert np.abs(est).max() < 48  # the bound below: float32 coordinates below 64 m
    thr, voxel, tol = 0.1, 0.05, 1e-5
    ref, racc, rcomp, rT = ME.compare_point_clouds_ref(est, gt, thr, voxel, align=True, return_distances=True)
    got, acc, comp, gT = ME.compare_point_clouds(dev(est), dev(gt), thr, voxel, align=True, return_distances=True)
    raw = ME.compare_point_clouds(dev(est), dev(gt), thr, voxel, align=False)
    acc, comp = host(acc), host(comp)
    print("reference", ref, "\ngpu      ", got, "\nunaligned", raw, "\n|T - T_ref| max", np.abs(gT - rT).max())
    # float32 rounding of the transformed coordinates (<= 3.3e-6 m of displacement at 32 m) plus the transform
    # agreement of DESIGN.md 7e (1e-7 m); the nearest distance is 1-Lipschitz in the point
    for k in ("accuracy", "completion", "chamfer_distance"):
        assert abs(got[k] - ref[k]) <= tol, (k, got[k], ref[k])
    assert got["num_points"] == ref["num_points"] == len(acc)
    fp, fn = int((acc > thr).sum()), int((comp > thr).sum())
    rfp, rfn = int((racc > thr).sum()), int((rcomp > thr).sum())
    assert abs(fp - rfp) <= int((np.abs(racc - thr) <= tol).sum())
    assert abs(fn - rfn) <= int((np.abs(rcomp - thr) <= tol).sum())
    want = ME.statistics(acc.sum(), len(acc), fp, comp.sum(), len(comp), fn)
    for k in ("precision", "recall", "f-score"):  # the device's sums and counts are those of its distance arrays
        assert got[k] == pytest.approx(want[k], rel=1e-12)
    assert got["accuracy"] < raw["accuracy"]


# ---------------------------------------------------------------------------------------------- LidarMapRenderer
def _state(S_):
    st = S_.FieldState(S_.StepConfig(), device="cuda:0", table_init=0.5, seed=7)
    torch.manual_seed(3)
    with torch.no_grad():
        st.params[2048:3072].mul_(8.0)  # a sigma head with contrast: surfaces along the rays
        st.occ.normal_(0, 2)
    st.refresh_shadow()
    return st


def test_lidar_map_renderer_end_to_end(ME, L):
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    st = _state(S_)
    wc, rr = syn.world_cube("canteen"), syn.SENSORS["canteen"]["ray_range"]
    poses = [torch.from_numpy(p.astype(np.float32)) for p in syn.keyframe_poses("canteen", 2, None)]
    r = ME.LidarMapRenderer(st, wc, rr, (-22.5, 22.5), vertical_resolution=2.0, horizontal_resolution=2.0,
                            n_samples=256, chunk=2048)
    _, _, var = r.sweep(poses[0], L.step_key(5, 0))
    r.var_threshold = float(np.median(host(var)))  # so that the variance filter cuts
    voxel = 0.5
    sweeps = []
    for k, pose in enumerate(poses):
        key = L.step_key(5, k)
        dirs, depth, var = (host(t) for t in r.sweep(pose, key))
        assert 0 < len(depth) <= 23 * 180
        good = (var < np.float32(r.var_threshold)) & (depth < np.float32(rr[1] - 0.25))
        assert 0 < good.sum() < len(good)
        want = (dirs * depth[:, None])[good]
        pts = r.render_scan(pose, key)
        np.testing.assert_array_equal(host(pts), want)  # the filter: float32 products, nothing to round differently
        rm, rc, rk = ME.voxel_down_sample_ref(want, voxel, return_counts=True, return_keys=True)
        m, c, kk = ME.voxel_filter(pts, voxel, return_keys=True)
        np.testing.assert_array_equal(host(kk), rk)
        np.testing.assert_array_equal(host(c), rc)
        assert ulps(host(m), rm).max() <= 1
        Tp = pose.double().numpy()
        w = ME.transform_points(m, Tp)
        np.testing.assert_array_equal(host(w), ME.transform_points_ref(host(m), Tp))  # the same float64 terms
        sweeps.append(host(w))
    cloud = r.render(poses, voxel, skip_step=1, key=5)
    assert cloud.is_cuda and cloud.dtype == torch.float32
    merged = np.concatenate(sweeps)
    rm, rk = ME.voxel_down_sample_ref(merged, voxel, return_keys=True)
    assert len(rm) < len(merged)  # the sweeps overlap: the final filter merges
    assert tuple(cloud.shape) == rm.shape and ulps(host(cloud), rm).max() <= 1
    assert torch.equal(cloud, r.render(poses, voxel, skip_step=1, key=5))
    assert not torch.equal(cloud, r.render(poses, voxel, skip_step=1, key=6))
    # inside the world cube
    scale = float(wc.scale_factor.reshape(-1)[0])
    shift = wc.shift.reshape(-1).numpy().astype(np.float64)
    assert (np.abs((host(cloud).astype(np.float64) + shift) / scale) <= 1.0).all()
    # without a voxel size: the first pose's kept returns, moved to the world
    first = r.render_scan(poses[0], L.step_key(5, 0))
    assert torch.equal(r.render(poses, None, skip_step=2, key=5), ME.transform_points(first, poses[0].double().numpy()))
