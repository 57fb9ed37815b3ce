"""Frame-to-frame tracking on the GPU (loner_amd.tracking): lnr_cloud_normals and lnr_icp_stage against their float64
restatements (validated on their own in tests/test_tracking_ref.py), the schedule's determinism and its no-op rounds,
and Tracker end to end.  Clouds: two synthetic scans a small motion apart, about 1517 points each (no multiple of 64,
more than one LDS tile of 1024)."""
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
    """Host side of one scene, computed once: the two clouds, the reference's normals and its schedule result."""
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    base = syn.keyframe_poses(kind, 1, None)[0]
    win = syn.make_window(kind, 2, seed=3, poses=[base, base @ REL])
    tgt, src = (TR.frame_point_cloud(w["directions"], w["distances"], target_points=1500).numpy() for w in win)
    assert 1400 < len(src) < 1700 and len(tgt) % 64 != 0
    nrm = TR.normals_reference(tgt, 30)
    T, res = TR.icp_schedule_reference(src, tgt, nrm, TR.TrackerSettings().schedule)
    for a in (tgt, src, nrm, T):
        a.setflags(write=False)
    return dict(tgt=tgt, src=src, nrm=nrm, nrm32=nrm.astype(np.float32), T=T, res=res)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached arrays are read-only


# ---------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("kind", KINDS)
def test_normals_match_the_reference(kind):
    from scipy.spatial import cKDTree
    from loner_amd import tracking as TR
    c = _case(kind)
    pts = c["tgt"]
    out = TR.cloud_normals(_dev(pts), 30).cpu().numpy().astype(np.float64)
    p64 = pts.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=31)
    clear = (d[:, 30] - d[:, 29]) > 1e-4 * d[:, 30]  # the 30th and 31st neighbours cannot swap in fp32
    dots = np.abs(np.einsum("ni,ni->n", out, c["nrm"]))
    print(f"{kind}: ambiguous {1 - clear.mean():.4f}, min |dot| on the rest {dots[clear].min():.9f}, "
          f"on all {dots.min():.6f}")
    assert 1 - clear.mean() <= 0.03
    assert dots[clear].min() >= 1 - 1e-4
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() <= 1e-5
    assert (np.einsum("ni,ni->n", out, p64) <= 0).all()


def test_normals_small_clouds_and_k_range():
    """k = 3, 30 and 64 on a cloud smaller than a tile, k = n (every point is every point's neighbour); coincident
    points give (0, 0, 1) turned towards the origin."""
    from loner_amd import tracking as TR
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(70, 3)).astype(np.float32) * np.float32([3, 2, 0.5]) + np.float32([0, 0, 4])
    for k in (3, 30, 64):
        out = TR.cloud_normals(_dev(pts), k).cpu().numpy().astype(np.float64)
        ref = TR.normals_reference(pts, k)
        assert np.abs(np.einsum("ni,ni->n", out, ref)).min() >= 1 - 1e-4, k
    out = TR.cloud_normals(_dev(pts[:5]), 5).cpu().numpy().astype(np.float64)
    ref = TR.normals_reference(pts[:5], 5)
    assert np.abs(out @ ref[0]).min() >= 1 - 1e-6  # one covariance for all five
    same = np.tile(np.float32([[1, 2, 3]]), (9, 1))
    np.testing.assert_array_equal(TR.cloud_normals(_dev(same), 4).cpu().numpy(), np.tile(np.float32([[0, 0, -1]]), (9, 1)))


# ---------------------------------------------------------------------------------------------- one correspond round
def _clear_threshold(d, near):
    """A float32 threshold at or just above ``near`` that no distance of d lies within 1e-4 relative of."""
    for j in range(200):
        thr = float(np.float32(near * (1 + 5e-4 * j)))
        if np.abs(d - thr).min() > 1e-4 * thr:
            return thr
    raise AssertionError("no clear threshold")


def _one_round(solver, src, tgt, nrm, T0, thr, max_iterations=0):
    from loner_amd import tracking as TR
    idx = torch.full((src.shape[0],), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((src.shape[0],), -1.0, dtype=torch.float32, device=DEV)
    solver.init(T0)
    solver.stage(src, tgt, nrm, TR.IcpStage(thr, max_iterations, 1e-8, 1e-8), idx, d2)
    return solver.read()[-1], idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("near", (1.5, 0.125))
@pytest.mark.parametrize("at", ("identity", "converged"))
@pytest.mark.parametrize("kind", KINDS)
def test_correspond_round(kind, at, near):
    from scipy.spatial import cKDTree
    from loner_amd import tracking as TR
    c = _case(kind)
    T0 = np.eye(4) if at == "identity" else c["T"]
    src64, tgt64, n64 = c["src"].astype(np.float64), c["tgt"].astype(np.float64), c["nrm32"].astype(np.float64)
    p = src64 @ T0[:3, :3].T + T0[:3, 3]
    d, nn = cKDTree(tgt64).query(p, k=2)
    thr = _clear_threshold(d[:, 0], near)
    assert np.abs(d[:, 0] - thr).min() > 1e-4 * thr
    keep_ref = d[:, 0] < thr
    st, idx, d2 = _one_round(TR.IcpSolver(DEV), _dev(c["src"]), _dev(c["tgt"]), _dev(c["nrm32"]), T0, thr)
    # which pairs are kept, and with whom
    keep = idx >= 0
    assert (idx[~keep] == -1).all() and (d2[~keep] == 0).all()
    np.testing.assert_array_equal(keep, keep_ref)
    assert st["n_corr"] == int(keep_ref.sum()) and st["iterations"] == 0 and not st["converged"]
    clear = (d[:, 1] - d[:, 0]) > 1e-5 * d[:, 0]
    assert (idx[keep & clear] == nn[keep & clear, 0]).all()
    second = keep & ~clear
    assert ((idx[second] == nn[second, 0]) | (idx[second] == nn[second, 1])).all()
    assert second.sum() <= 0.005 * len(p)
    # the search's own d^2: p rounded to fp32 moves by at most delta = 1e-5 m (half an ulp of 128 m per axis), so d^2
    # by 2 d delta + delta^2; the fp32 arithmetic adds a few 1e-7 relative
    dk, delta = d[keep, 0], 1e-5
    assert (np.abs(d2[keep] - dk ** 2) <= 2 * dk * delta + delta ** 2 + 1e-6 * dk ** 2).all()
    # the sums, against float64 sums over the GPU's own pairs
    terms = TR.point_to_plane_terms(p[keep], tgt64[idx[keep]], n64[idx[keep]])
    ref, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    err = np.abs(st["sums"] - ref) / scale
    print(f"{kind} {at} thr {thr:.6f}: kept {keep.sum()} of {len(p)}, near ties {second.sum()}, "
          f"max sum error {err.max():.3e} of sum |term|")
    assert (np.abs(st["sums"] - ref) <= 1e-5 * scale).all()
    dd = ((p[keep] - tgt64[idx[keep]]) ** 2).sum(axis=1)
    assert st["fitness"] == keep.sum() / len(p)
    # both sides are float64; p = T s is rounded in a different order (a few ulp of 128 m, 5e-14 m), which a pair at
    # d = 2 mm feels as 5e-11 of its d^2
    assert abs(st["sum_d2"] - dd.sum()) <= 1e-9 * dd.sum()
    assert abs(st["rmse"] - np.sqrt(dd.sum() / keep.sum())) <= 1e-9 * st["rmse"]
    np.testing.assert_array_equal(st["T"], T0)


# ---------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("kind", KINDS)
def test_update_from_given_sums(kind):
    """The sums of round 0 (a stage with no update allowed), then a stage with one update from the same start: its T
    is numpy's solve and M(x) T."""
    from loner_amd import tracking as TR
    c = _case(kind)
    solver = TR.IcpSolver(DEV)
    src, tgt, nrm = _dev(c["src"]), _dev(c["tgt"]), _dev(c["nrm32"])
    rng = np.random.default_rng(7)
    T0 = TR.transform_from_vector6(rng.normal(size=6) * [0.01, 0.01, 0.01, 0.1, 0.1, 0.1])
    st0, _, _ = _one_round(solver, src, tgt, nrm, T0, 1.5)
    st1, _, _ = _one_round(solver, src, tgt, nrm, T0, 1.5, max_iterations=1)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = st0["sums"][:21]
    A = A + np.triu(A, 1).T
    x = np.linalg.solve(A, -st0["sums"][21:])
    want = TR.transform_from_vector6(x) @ T0
    diff = np.abs(st1["T"] - want).max() / np.abs(want).max()
    print(f"{kind}: update differs from numpy's by {diff:.3e} relative, cond {np.linalg.cond(A):.3e}")
    assert diff <= 1e-12
    assert st1["iterations"] == 1
    np.testing.assert_array_equal(st1["T"][3], [0, 0, 0, 1])


def test_update_without_correspondences():
    from loner_amd import tracking as TR
    c = _case("quad")
    T0 = c["T"]
    st, idx, _ = _one_round(TR.IcpSolver(DEV), _dev(c["src"]), _dev(c["tgt"]), _dev(c["nrm32"]), T0, 1e-6,
                            max_iterations=3)
    assert (idx == -1).all()
    assert st["T"].tobytes() == np.ascontiguousarray(T0).tobytes()
    assert st["fitness"] == 0.0 and st["rmse"] == 0.0 and st["n_corr"] == 0 and st["sum_d2"] == 0.0
    assert np.isfinite(st["sums"]).all() and np.isfinite(st["T"]).all()
    assert st["converged"] and st["iterations"] == 1  # the second evaluation equals the first


# ---------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("kind", KINDS)
def test_schedule_matches_the_reference(kind):
    from loner_amd import tracking as TR
    c = _case(kind)
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    nrm = TR.cloud_normals(tgt, 30)
    sched = TR.TrackerSettings().schedule
    solver = TR.IcpSolver(DEV)
    T, res = TR.icp(src, tgt, nrm, sched, solver=solver)
    raw = solver.snap[:2].cpu().numpy().tobytes()
    et, er = _pose_error(T, REL)
    rt, rr = _pose_error(c["T"], REL)
    dt, dr = _pose_error(T, c["T"])
    print(f"{kind}: GPU {et * 1e3:.3f} mm {er:.4f} deg, reference {rt * 1e3:.3f} mm {rr:.4f} deg, "
          f"GPU vs reference {dt * 1e3:.4f} mm {dr:.5f} deg; iterations GPU {[r['iterations'] for r in res]} "
          f"reference {[r['iterations'] for r in c['res']]}")
    assert et <= 2 * rt and er <= 2 * rr
    assert all(0 < r["iterations"] <= 10 for r in res)
    # the same schedule again: bit-identical states
    TR.icp(src, tgt, nrm, sched, solver=solver)
    assert solver.snap[:2].cpu().numpy().tobytes() == raw


@pytest.mark.parametrize("kind", KINDS)
def test_rounds_after_convergence_are_no_ops(kind):
    from loner_amd import tracking as TR
    c = _case(kind)
    src, tgt, nrm = _dev(c["src"]), _dev(c["tgt"]), _dev(c["nrm32"])
    loose = TR.IcpStage(1.5, 10, 1e-2, 1e-2)
    _, (a,) = TR.icp(src, tgt, nrm, [loose])
    assert a["converged"] and 0 < a["iterations"] < 10
    _, (b,) = TR.icp(src, tgt, nrm, [TR.IcpStage(1.5, a["iterations"], 1e-2, 1e-2)])
    assert b["iterations"] == a["iterations"]
    assert a["T"].tobytes() == b["T"].tobytes()
    assert (a["fitness"], a["rmse"], a["n_corr"]) == (b["fitness"], b["rmse"], b["n_corr"])
    assert a["sums"].tobytes() == b["sums"].tobytes()


# ---------------------------------------------------------------------------------------------- Tracker
@functools.lru_cache(maxsize=None)
def _chain(n=5):
    from loner_amd import synthetic as syn
    base = syn.keyframe_poses("quad", 1, None)[0]
    poses = [base]
    for _ in range(n - 1):
        poses.append(poses[-1] @ REL)
    return poses, syn.make_window("quad", n, seed=3, poses=poses)


def test_tracker_end_to_end():
    from loner_amd import tracking as TR
    poses, win = _chain()
    settings = TR.TrackerSettings(target_uniform_point_count=1500)
    tr = TR.Tracker(settings, DEV)
    got, ref_pose, ref = [], np.eye(4), []
    prev = None
    for w in win:
        scan = dict(directions=w["directions"], distances=w["distances"])
        out = tr.track(scan)
        got.append(out)
        # the numpy pipeline on the same cloud
        pts = TR.frame_point_cloud(w["directions"], w["distances"], target_points=1500).numpy()
        nrm = TR.normals_reference(pts, 30)
        if prev is not None:
            T, _ = TR.icp_schedule_reference(pts, prev[0], prev[1], settings.schedule)
            ref_pose = ref_pose @ T
        ref.append(ref_pose)
        prev = (pts, nrm)
        assert set(out) == {"pose", "fitness", "rmse", "iterations", "n_points"}
        assert out["pose"].shape == (4, 4) and out["pose"].dtype == np.float64
        assert isinstance(out["fitness"], float) and isinstance(out["rmse"], float)
        assert isinstance(out["n_points"], int) and out["n_points"] == len(pts)
        assert isinstance(out["iterations"], list) and all(isinstance(i, int) for i in out["iterations"])
    np.testing.assert_array_equal(got[0]["pose"], np.eye(4))
    assert got[0]["iterations"] == [] and all(len(g["iterations"]) == 2 for g in got[1:])
    truth = np.linalg.inv(poses[0]) @ poses[-1]
    gt, gr = _pose_error(got[-1]["pose"], truth)
    rt, rr = _pose_error(ref[-1], truth)
    print(f"drift after {len(win)} scans: GPU {gt * 1e3:.3f} mm {gr:.4f} deg, numpy {rt * 1e3:.3f} mm {rr:.4f} deg")
    assert gt <= 2 * rt and gr <= 2 * rr
    assert tr.frame_count == 5


def test_tracker_motion_compensation_and_initial_pose():
    from loner_amd import preprocess as PP
    from loner_amd import tracking as TR
    poses, win = _chain()
    start = poses[0]
    tr = TR.Tracker(TR.TrackerSettings(target_uniform_point_count=1500), DEV, initial_pose=start)
    scans = []
    for i, w in enumerate(win[:2]):
        P = w["distances"].shape[0]
        ts = torch.linspace(0.0, 0.1, P, dtype=torch.float64).float() + 0.1 * i
        scans.append(dict(directions=w["directions"].clone(), distances=w["distances"].clone(), timestamps=ts))
    o0 = tr.track(scans[0])
    np.testing.assert_array_equal(o0["pose"], start)
    assert torch.equal(scans[0]["directions"], win[0]["directions"])  # the first frame is not compensated
    o1 = tr.track(scans[1])
    # 90 % of the sweep, then every (n // 1500)-th point
    s, f, step = TR.frame_indices(scans[1]["timestamps"], scan_duration=0.9, target_points=1500)
    assert o1["n_points"] == len(range(s, f, step)) and 0.88 < (f - s) / len(scans[1]["timestamps"]) < 0.92
    et, er = _pose_error(np.linalg.inv(start) @ o1["pose"], REL)
    assert et < 0.05 and er < 0.5  # it tracked (the accuracy itself is test_schedule_matches_the_reference's)
    dirs = win[1]["directions"].t().contiguous().to(DEV)
    dist = win[1]["distances"].clone().to(DEV)
    t0 = float(scans[0]["timestamps"][0] / 2.0 + scans[0]["timestamps"][-1] / 2.0)
    t1 = float(scans[1]["timestamps"][0] / 2.0 + scans[1]["timestamps"][-1] / 2.0)
    PP.motion_compensate(dirs, dist, scans[1]["timestamps"].to(DEV), (start, o1["pose"]), (t0, t1), o1["pose"])
    assert scans[1]["directions"].shape == win[1]["directions"].shape
    assert torch.equal(scans[1]["directions"], dirs.t()) and torch.equal(scans[1]["distances"], dist)
    assert not torch.equal(scans[1]["distances"].cpu(), win[1]["distances"])


def test_tracker_sky_rays():
    from loner_amd import preprocess as PP
    from loner_amd import tracking as TR
    _, win = _chain()
    tr = TR.Tracker(TR.TrackerSettings(target_uniform_point_count=1500, compute_sky_rays=True), DEV)
    scan = dict(directions=win[0]["directions"], distances=win[0]["distances"])
    out = tr.track(scan)
    want = PP.sky_rays(win[0]["directions"].t().contiguous().to(DEV), out["pose"])
    assert want.shape[0] > 0 and scan["sky_directions"].shape == (3, want.shape[0])
    assert torch.equal(scan["sky_directions"], want.t())


# ---------------------------------------------------------------------------------------------- ABI errors
def test_bad_arguments_are_refused_before_any_launch():
    from loner_amd import _lib as L
    from loner_amd import tracking as TR
    pts = torch.zeros(40, 3, device=DEV)
    out = torch.zeros(40, 3, device=DEV)
    s = L.stream(pts.device)
    assert L.lib().lnr_cloud_normals(None, 40, 30, L.ptr(out), s) < 0
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_cloud_normals", None, 40, 30, out, s)
    with pytest.raises(RuntimeError, match="n=20"):
        L.call("lnr_cloud_normals", pts, 20, 30, out, s)  # k > n
    for k in (2, 65):
        with pytest.raises(RuntimeError, match="outside"):
            L.call("lnr_cloud_normals", pts, 40, k, out, s)
    with pytest.raises(RuntimeError, match="2\\^18"):
        L.call("lnr_cloud_normals", pts, (1 << 18) + 1, 30, out, s)
    state = torch.zeros(TR.STATE_BYTES, dtype=torch.uint8, device=DEV)
    need = int(L.lib().lnr_icp_workspace_bytes(40))
    assert need > 0 and L.lib().lnr_icp_workspace_bytes(0) == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    args = [pts, 40, pts, out, 40, 1.5, 10, 1e-8, 1e-8, state, ws, need, None, None, s]
    L.call("lnr_icp_init", state, (ctypes.c_double * 16)(*np.eye(4).reshape(-1)), s)
    L.call("lnr_icp_stage", *args)  # the good call
    for pos, bad, msg in ((11, need - 8, "workspace"), (0, None, "null pointer"), (9, None, "null pointer"),
                          (1, 0, "bad sizes"), (5, 0.0, "threshold"), (6, -1, "max_iterations")):
        a = list(args)
        a[pos] = bad
        with pytest.raises(RuntimeError, match=msg):
            L.call("lnr_icp_stage", *a)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_icp_init", state, None, s)
    with pytest.raises(RuntimeError, match="not finite"):
        L.call("lnr_icp_init", state, (ctypes.c_double * 16)(*([float("nan")] * 16)), s)
    torch.cuda.synchronize()
