"""Registration on the cell grid (lnr_normals_from_knn, lnr_icp_stage_grid; ``search="grid"``) against the exhaustive
kernels of the same library, bit for bit wherever both can run, and against float64 numpy above their limits.
Small clouds: tests/test_gpu_tracking.py's two scans a small motion apart (about 1517 points, no multiple of 64 or 16);
large ones: four full synthetic scans."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("quad", "canteen")
DEV = "cuda:0"


def _rel_pose():
    y, p = np.deg2rad(2.0), np.deg2rad(0.5)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = (0.4, 0.04, 0.02)
    return T


REL = _rel_pose()


def _pose_error(T, ref):
    d = np.linalg.inv(ref) @ T
    ang = np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(d[:3, 3])), float(ang)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """tests/test_gpu_tracking.py's recipe: two clouds, the float64 normals of the target, the float64 schedule."""
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    base = syn.keyframe_poses(kind, 1, None)[0]
    win = syn.make_window(kind, 2, seed=3, poses=[base, base @ REL])
    tgt, src = (TR.frame_point_cloud(w["directions"], w["distances"], target_points=1500).numpy() for w in win)
    assert 1400 < len(src) < 1700 and len(tgt) % 64 != 0
    nrm = TR.normals_reference(tgt, 30)
    T, _ = TR.icp_schedule_reference(src, tgt, nrm, TR.TrackerSettings().schedule)
    for a in (tgt, src, nrm, T):
        a.setflags(write=False)
    return dict(tgt=tgt, src=src, nrm32=nrm.astype(np.float32), T=T)


@functools.lru_cache(maxsize=None)
def _chain(n=5):
    from loner_amd import synthetic as syn
    base = syn.keyframe_poses("quad", 1, None)[0]
    poses = [base]
    for _ in range(n - 1):
        poses.append(poses[-1] @ REL)
    return poses, syn.make_window("quad", n, seed=3, poses=poses)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached arrays are read-only


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- 1. normals, bitwise
@pytest.mark.parametrize("kind", KINDS)
def test_normals_equal_the_exhaustive_kernel(kind):
    from loner_amd import tracking as TR
    pts = _dev(_case(kind)["tgt"])
    for k in (3, 30, 64):
        want = _bytes(TR.cloud_normals(pts, k))
        for cell in (None, 0.05, 50.0):  # the default; nearly every query through the kNN's exhaustive list; one cell
            got = TR.cloud_normals_grid(pts, k, cell)
            assert _bytes(got) == want, (kind, k, cell)
        assert _bytes(TR.cloud_normals_grid(pts, k)) == want  # and again


def test_normals_small_clouds_equal_the_exhaustive_kernel():
    from loner_amd import tracking as TR
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(70, 3)).astype(np.float32) * np.float32([3, 2, 0.5]) + np.float32([0, 0, 4])
    for p, k in ((pts, 64), (pts[:5], 5)):
        for cell in (None, 0.05, 50.0):
            assert _bytes(TR.cloud_normals_grid(_dev(p), k, cell)) == _bytes(TR.cloud_normals(_dev(p), k)), (k, cell)
    same = _dev(np.tile(np.float32([[1, 2, 3]]), (9, 1)))
    out = TR.cloud_normals_grid(same, 4)
    np.testing.assert_array_equal(out.cpu().numpy(), np.tile(np.float32([[0, 0, -1]]), (9, 1)))
    assert _bytes(out) == _bytes(TR.cloud_normals(same, 4))
    buf = torch.zeros(9, 3, device=DEV)
    assert TR.cloud_normals_grid(same, 4, out=buf) is buf and _bytes(buf) == _bytes(out)
    with pytest.raises(ValueError, match="k=10"):
        TR.cloud_normals_grid(same, 10)
    bad = pts.copy()
    bad[11, 2] = np.nan
    for cell in (None, 0.5):  # the box read refuses the first, the search's status word the second
        with pytest.raises(RuntimeError, match="nan or inf"):
            TR.cloud_normals_grid(_dev(bad), 30, cell)


# ---------------------------------------------------------------------------------------------- 2. normals above 2^18
def test_normals_above_the_exhaustive_limit():
    from loner_amd import lidar_map as LM
    from loner_amd import map_eval as ME
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    n, k = (1 << 18) + 77, 30
    cloud = ME.scan_world_points(syn.make_window("quad", 4, seed=3))
    assert cloud.shape[0] >= n
    pts = cloud[:n].contiguous().to(DEV)
    assert n > TR.NORMALS_CHUNK  # more than one chunk of queries
    with pytest.raises(RuntimeError, match="2\\^18"):
        TR.cloud_normals(pts, k)
    grid = LM.knn_grid(pts, k)
    a = TR.cloud_normals_grid(pts, k)
    b = TR.cloud_normals_grid(pts, k, 2 * grid.cell)
    assert _bytes(a) == _bytes(b)
    out = a.cpu().numpy().astype(np.float64)
    p64 = pts.cpu().numpy().astype(np.float64)
    assert (np.einsum("ni,ni->n", out, p64) <= 0).all()
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() <= 1e-5
    rows = np.random.default_rng(11).choice(n, 4096, replace=False)
    idx = LM.knn(pts[torch.from_numpy(rows).to(DEV)], grid, k)[0].cpu().numpy()
    nb = p64[idx]
    c = nb - nb.mean(axis=1, keepdims=True)
    lam, v = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c) / k)
    clear = (lam[:, 1] - lam[:, 0]) > 1e-4 * lam[:, 2]
    dots = np.abs(np.einsum("ni,ni->n", out[rows], v[:, :, 0]))
    print(f"rows excluded {(~clear).sum()} of 4096, min |dot| on the rest {dots[clear].min():.12f}")
    assert (~clear).sum() <= 0.01 * len(rows)
    assert dots[clear].min() >= 1 - 1e-6


# ---------------------------------------------------------------------------------------------- 3. one round, bitwise
def _round(solver, src, tgt, nrm, T0, stage, **kw):
    idx = torch.full((src.shape[0],), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((src.shape[0],), -1.0, dtype=torch.float32, device=DEV)
    solver.init(T0)
    solver.stage(src, tgt, nrm, stage, idx, d2, **kw)
    return _bytes(solver.state), _bytes(idx), _bytes(d2), int((idx >= 0).sum())


@pytest.mark.parametrize("kind", KINDS)
def test_one_round_equals_the_exhaustive_stage(kind):
    from loner_amd import _lib as L
    from loner_amd import tracking as TR
    c = _case(kind)
    away = np.eye(4)
    away[0, 3] = 30.0
    starts = dict(identity=np.eye(4), converged=c["T"], away=away @ c["T"])
    src_all, tgt, nrm = _dev(c["src"]), _dev(c["tgt"]), _dev(c["nrm32"])
    target = TR.GridTarget(tgt, nrm)
    solver = TR.IcpSolver(DEV)
    kept = {}
    for n_src in (src_all.shape[0], 1, 15, 17, 255, 257):
        src = src_all[:n_src].contiguous()
        for at, T0 in starts.items():
            for thr in (1.5, 0.125):
                stage = TR.IcpStage(thr, 0, 1e-8, 1e-8)
                want = _round(solver, src, tgt, nrm, T0, stage)
                kept[(n_src, at, thr)] = want[3]
                floor = thr * (1 + 2.0 ** -10)
                for cell, rings in ((floor / 4, 4), (floor, 1), (50.0, 1)):
                    assert L.lib().lnr_icp_grid_rings(thr, cell) == rings
                    got = _round(solver, src, target, None, T0, stage, search="grid", cell=cell)
                    assert got == want, (kind, n_src, at, thr, cell, got[3], want[3])
                    assert solver.read()[-1]["status"] == 0
    n = src_all.shape[0]
    print(kind, {k: v for k, v in kept.items() if k[0] == n})
    assert kept[(n, "converged", 1.5)] > 0.5 * n  # the comparison is not one of empty sets
    assert kept[(n, "away", 0.125)] < kept[(n, "converged", 0.125)]  # moved away: queries outside the box, fewer pairs


# ---------------------------------------------------------------------------------------------- 4. schedules, bitwise
@pytest.mark.parametrize("kind", KINDS)
def test_schedules_equal_the_exhaustive_schedule(kind):
    from loner_amd import tracking as TR
    c = _case(kind)
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    nrm = TR.cloud_normals(tgt, 30)
    sched = TR.TrackerSettings().schedule
    brute, grid = TR.IcpSolver(DEV), TR.IcpSolver(DEV)
    Tb, rb = TR.icp(src, tgt, nrm, sched, solver=brute)
    target = TR.GridTarget(tgt, nrm)
    Tg, rg = TR.icp(src, target, None, sched, solver=grid, search="grid")
    cells = [target.cell_for(st.threshold) for st in sched]
    assert sorted(target._grids) == sorted(set(cells))  # one grid per distinct cell, shared by the stages that use it
    assert _bytes(grid.snap[:2]) == _bytes(brute.snap[:2])
    assert Tg.tobytes() == Tb.tobytes() and [r["iterations"] for r in rg] == [r["iterations"] for r in rb]
    assert all(r["status"] == 0 for r in rg + rb)
    Tt, _ = TR.icp(src, tgt, nrm, sched, search="grid")  # a tensor target is wrapped
    assert Tt.tobytes() == Tb.tobytes()
    # two stages on two cells (at 1517 points the default rule gives both stages one cell: 2 x default_cell is 4 m)
    floors = [st.threshold * (1 + 2.0 ** -10) for st in sched]
    assert floors[0] != floors[1]
    grid.init()
    for st, cell in zip(sched, floors):
        grid.stage(src, target, None, st, search="grid", cell=cell)
    assert set(floors) <= set(target._grids)
    assert _bytes(grid.snap[:2]) == _bytes(brute.snap[:2])
    # a loose stage converges early; the rounds after it are no-ops
    loose = TR.IcpStage(1.5, 10, 1e-2, 1e-2)
    TR.icp(src, tgt, nrm, [loose], solver=brute)
    _, (a,) = TR.icp(src, target, None, [loose], solver=grid, search="grid")
    assert a["converged"] and 0 < a["iterations"] < 10
    assert _bytes(grid.snap[:1]) == _bytes(brute.snap[:1])
    raw = _bytes(grid.snap[:1])
    _, (b,) = TR.icp(src, target, None, [TR.IcpStage(1.5, a["iterations"], 1e-2, 1e-2)], solver=grid, search="grid")
    assert b["iterations"] == a["iterations"] and _bytes(grid.snap[:1]) == raw
    # grid and exhaustive stages chain on one state
    TR.icp(src, tgt, nrm, sched, solver=brute)
    for first, second in (("grid", "brute"), ("brute", "grid")):
        grid.init()
        grid.stage(src, target if first == "grid" else tgt, nrm, sched[0], search=first)
        grid.stage(src, target if second == "grid" else tgt, nrm, sched[1], search=second)
        assert _bytes(grid.snap[:2]) == _bytes(brute.snap[:2]), (first, second)


# ---------------------------------------------------------------------------------------------- 5. tracker
def _track(settings, win):
    from loner_amd import tracking as TR
    tr = TR.Tracker(settings, DEV)
    return [tr.track(dict(directions=w["directions"], distances=w["distances"])) for w in win]


def test_tracker_grid_equals_brute_and_tracks_full_scans():
    from loner_amd import tracking as TR
    poses, win = _chain()
    brute = _track(TR.TrackerSettings(target_uniform_point_count=1500), win)
    grid = _track(TR.TrackerSettings(target_uniform_point_count=1500, search="grid"), win)
    for b, g in zip(brute, grid):
        assert set(g) == set(b)
        assert g["pose"].tobytes() == b["pose"].tobytes()
        assert (g["fitness"], g["rmse"], g["iterations"], g["n_points"]) == \
               (b["fitness"], b["rmse"], b["iterations"], b["n_points"])
    full = _track(TR.TrackerSettings(downsample_type=None, search="grid"), win)
    assert all(f["n_points"] == w["distances"].shape[0] for f, w in zip(full, win))
    assert full[0]["n_points"] > 50000
    truth = np.linalg.inv(poses[0]) @ poses[-1]
    ft, fr = _pose_error(full[-1]["pose"], truth)
    bt, br = _pose_error(brute[-1]["pose"], truth)
    print(f"drift after {len(win)} scans: full scans ({full[0]['n_points']} points, grid) {ft * 1e3:.3f} mm "
          f"{fr:.4f} deg; 1500 points (brute) {bt * 1e3:.3f} mm {br:.4f} deg")
    assert all(len(f["iterations"]) == 2 for f in full[1:])
    assert ft <= bt and fr <= br  # more points should not track worse, in translation or in rotation


# ---------------------------------------------------------------------------------------------- 6. alignment
def _aligned_pair(est):
    from loner_amd import map_eval as ME
    a = np.deg2rad(0.3)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (0.02 / np.sqrt(3),) * 3
    return est, ME.transform_points_ref(est, T)


def test_alignment_grid_equals_brute():
    """tests/test_gpu_map_eval.py::test_compare_aligned_matches_reference's case: both searches can run."""
    from loner_amd import map_eval as ME
    from loner_amd import synthetic as syn
    est, gt = _aligned_pair(ME.scan_world_points(syn.make_window("canteen", 4), stride=8).numpy()[::2])
    e, g = _dev(est), _dev(gt)
    sb, _, _, Tb = ME.compare_point_clouds(e, g, 0.1, 0.05, align=True, return_distances=True)
    sg, _, _, Tg = ME.compare_point_clouds(e, g, 0.1, 0.05, align=True, return_distances=True, align_search="grid")
    assert sg == sb and Tg.tobytes() == Tb.tobytes()
    assert not np.array_equal(Tb, np.eye(4))


def test_alignment_above_the_exhaustive_cap():
    from loner_amd import map_eval as ME
    from loner_amd import synthetic as syn
    est, gt = _aligned_pair(ME.scan_world_points(syn.make_window("quad", 4)).numpy())
    assert np.abs(est).max() < 64
    thr, voxel, tol, cap = 0.1, 0.05, 1e-5, 1_000_000
    e, g = _dev(est), _dev(gt)
    with pytest.raises(ValueError, match="2\\^17"):
        ME.compare_point_clouds(e, g, thr, voxel, align_max_points=cap)
    got, acc, comp, gT = ME.compare_point_clouds(e, g, thr, voxel, align=True, align_max_points=cap,
                                                 return_distances=True, align_search="grid")
    assert acc.shape[0] > 1 << 17 and comp.shape[0] > 1 << 17  # both alignment clouds are above the old cap, unstrided
    raw = ME.compare_point_clouds(e, g, thr, voxel, align=False)
    ref, racc, rcomp, rT = ME.compare_point_clouds_ref(est, gt, thr, voxel, align=True, align_max_points=cap,
                                                       return_distances=True, align_search="grid")
    acc, comp = acc.cpu().numpy(), comp.cpu().numpy()
    print("filtered", len(acc), len(comp), "\nreference", ref, "\ngpu      ", got, "\nunaligned", raw,
          "\n|T - T_ref| max", np.abs(gT - rT).max())
    for k in ("accuracy", "completion", "chamfer_distance"):
        assert abs(got[k] - ref[k]) <= tol, (k, got[k], ref[k])
    assert got["num_points"] == ref["num_points"] == len(acc)
    fp, fn = int((acc > thr).sum()), int((comp > thr).sum())
    rfp, rfn = int((racc > thr).sum()), int((rcomp > thr).sum())
    assert abs(fp - rfp) <= int((np.abs(racc - thr) <= tol).sum())
    assert abs(fn - rfn) <= int((np.abs(rcomp - thr) <= tol).sum())
    want = ME.statistics(acc.sum(), len(acc), fp, comp.sum(), len(comp), fn)
    for k in ("precision", "recall", "f-score"):
        assert got[k] == pytest.approx(want[k], rel=1e-12)
    assert got["accuracy"] < raw["accuracy"]


# ---------------------------------------------------------------------------------------------- 7. error contract
def test_bad_arguments_are_refused_before_any_launch():
    from loner_amd import _lib as L
    from loner_amd import map_eval as ME
    from loner_amd import tracking as TR
    rng = np.random.default_rng(2)
    pts = _dev(rng.uniform(0, 4, size=(40, 3)).astype(np.float32))
    out = torch.zeros(40, 3, device=DEV)
    idx = torch.zeros(40, 30, dtype=torch.int32, device=DEV)
    s = L.stream(pts.device)
    args = [pts, 40, pts, 40, idx, 30, out, s]
    L.call("lnr_normals_from_knn", *args)  # the good call
    big = L.CLOUD_MAX_POINTS + 1
    for pos, bad, msg in ((0, None, "null pointer"), (2, None, "null pointer"), (4, None, "null pointer"),
                          (6, None, "null pointer"), (5, 2, "k=2"), (5, 65, "k=65"), (1, 0, "bad sizes"),
                          (3, 0, "bad sizes"), (1, big, "bad sizes"), (3, big, "bad sizes")):
        a = list(args)
        a[pos] = bad
        with pytest.raises(RuntimeError, match=msg):
            L.call("lnr_normals_from_knn", *a)
    # an index outside the target is never followed: its row gets the fallback, the other rows their normals
    good = TR.cloud_normals_grid(pts, 30)
    from loner_amd import lidar_map as LM
    lists = LM.knn(pts, pts, 30)[0]
    lists[3, 7], lists[9, 0] = 40, -1
    L.call("lnr_normals_from_knn", pts, 40, pts, 40, lists, 30, out, s)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[[3, 9]], np.float32([[0, 0, -1], [0, 0, -1]]))  # z > 0: turned to the origin
    keep = np.ones(40, bool)
    keep[[3, 9]] = False
    np.testing.assert_array_equal(got[keep], good.cpu().numpy()[keep])

    g = ME.NearestGrid(pts, 1.0)
    state = torch.zeros(TR.STATE_BYTES, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = int(L.lib().lnr_icp_grid_workspace_bytes(40))
    assert need == 3 * 32 * 8
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    L.call("lnr_icp_init", state, (ctypes.c_double * 16)(*np.eye(4).reshape(-1)), s)
    args = [pts, 40, g.points, g.keys, g.perm, 40, g.origin, g.cell, g.dims, out, 1.5, 10, 1e-8, 1e-8, state, ws, need,
            None, None, status, s]
    L.call("lnr_icp_stage_grid", *args)  # the good call
    before = _bytes(state)
    nulls = [(p, None, "null pointer") for p in (0, 2, 3, 4, 6, 8, 9, 14, 15, 19)]
    for pos, bad, msg in nulls + [(1, 0, "bad sizes"), (5, 0, "bad sizes"), (1, L.ICP_MAX_POINTS + 1, "bad sizes"),
                                  (5, L.ICP_MAX_POINTS + 1, "bad sizes"), (16, need - 8, "workspace"),
                                  (15, ctypes.c_void_p(ws.data_ptr() + 4), "aligned"), (10, 0.0, "threshold"),
                                  (10, float("nan"), "threshold"), (10, float("inf"), "threshold"),
                                  (11, -1, "max_iterations"), (12, -1e-9, "negative"), (13, -1e-9, "negative"),
                                  (7, 1.5 / 4, "rings"), (7, 0.0, "cell"), (7, float("nan"), "cell")]:
        a = list(args)
        a[pos] = bad
        with pytest.raises(RuntimeError, match=msg):
            L.call("lnr_icp_stage_grid", *a)
    torch.cuda.synchronize()
    assert _bytes(state) == before and int(status.item()) == 0  # nothing ran
    with pytest.raises(RuntimeError, match="rings"):
        TR.IcpSolver(DEV).stage(pts, TR.GridTarget(pts, out), None, TR.IcpStage(1.5), search="grid", cell=0.1)
    with pytest.raises(ValueError, match="kdtree"):
        TR.IcpSolver(DEV).stage(pts, pts, out, TR.IcpStage(1.5), search="kdtree")


def test_a_nan_source_point_has_no_pair():
    from loner_amd import _lib as L
    from loner_amd import tracking as TR
    c = _case("quad")
    src = c["src"].copy()
    src[5, 1] = np.nan
    src[600] = np.inf
    src, tgt, nrm = _dev(src), _dev(c["tgt"]), _dev(c["nrm32"])
    solver = TR.IcpSolver(DEV)
    idx = torch.full((src.shape[0],), -7, dtype=torch.int32, device=DEV)
    solver.init()
    solver.stage(src, TR.GridTarget(tgt, nrm), None, TR.IcpStage(1.5), idx, search="grid")
    st = solver.read()[-1]
    assert st["status"] == L.CLOUD_NONFINITE
    idx = idx.cpu().numpy()
    assert idx[5] == -1 and idx[600] == -1 and (idx >= 0).sum() == st["n_corr"] > 0.5 * len(idx)
    assert np.isfinite(st["T"]).all() and st["iterations"] > 0
    # the exhaustive stage drops the same two points: the same state
    brute = TR.IcpSolver(DEV)
    brute.init()
    brute.stage(src, tgt, nrm, TR.IcpStage(1.5))
    assert _bytes(brute.state) == _bytes(solver.state)
    solver.init()
    assert int(solver.status.item()) == 0  # init clears the word
