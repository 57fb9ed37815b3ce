"""Per-keyframe scan preprocessing on the GPU (loner_amd.preprocess) against the numpy oracle
(oracle/preprocess.py): motion compensation (sensors.py:169-231) and sky rays
(fdt_optimize_implicit_map_utils.py:38-77)."""
import numpy as np
import pytest
import torch

from oracle import preprocess as opre

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import preprocess
    return preprocess


def _pose(yaw, pitch, t):
    from scipy.spatial.transform import Rotation
    m = np.eye(4)
    m[:3, :3] = Rotation.from_euler("zy", [yaw, pitch]).as_matrix()
    m[:3, 3] = t
    return m


def test_motion_compensate_vs_oracle(P):
    from loner_amd import synthetic as syn
    scan = syn.make_window("quad", 1, seed=4)[0]
    dirs = scan["directions"].numpy().astype(np.float64)
    dists = scan["distances"].numpy().astype(np.float64)
    n = dists.shape[0]
    ts = np.linspace(0, 0.1, n)
    start, end = _pose(0.3, 0.02, [1.0, 2.0, 0.5]), _pose(0.45, -0.01, [1.8, 2.3, 0.6])
    d_dev = torch.from_numpy(dirs.T.astype(np.float32)).cuda().contiguous()
    r_dev = torch.from_numpy(dists.astype(np.float32)).cuda()
    t_dev = torch.from_numpy(ts.astype(np.float32)).cuda()
    P.motion_compensate(d_dev, r_dev, t_dev, (start, end), (0.0, 0.1), end)
    torch.cuda.synchronize()
    idx = np.arange(0, n, 97)
    od, orr = opre.motion_compensate(dirs[:, idx], dists[idx], ts[idx], start, end, 0.0, 0.1, end)
    np.testing.assert_allclose(d_dev.cpu().numpy()[idx].T, od, atol=2e-5)
    np.testing.assert_allclose(r_dev.cpu().numpy()[idx], orr, rtol=2e-5, atol=2e-5)
    # identity motion leaves the scan unchanged
    d2 = torch.from_numpy(dirs.T.astype(np.float32)).cuda().contiguous()
    r2 = torch.from_numpy(dists.astype(np.float32)).cuda()
    P.motion_compensate(d2, r2, t_dev, (start, start), (0.0, 0.1), start)
    np.testing.assert_allclose(d2.cpu().numpy(), dirs.T, atol=2e-6)
    np.testing.assert_allclose(r2.cpu().numpy(), dists, rtol=2e-6)


@pytest.mark.parametrize("kind", ["quad", "forest", "canteen"])
def test_sky_rays_vs_oracle(P, kind):
    from loner_amd import synthetic as syn
    scan = syn.make_window(kind, 1, seed=2)[0]
    dirs = scan["directions"].numpy()
    pose = scan["pose"].numpy()
    got = P.sky_rays(torch.from_numpy(dirs.T.copy()).cuda(), pose).cpu().numpy().T
    ref = opre.sky_rays(dirs, pose[:3, :3])
    # 1-degree bins from float32 atan2: a point on a bin's rounding edge may land one bin over
    assert abs(got.shape[1] - ref.shape[1]) <= max(3, 0.01 * ref.shape[1]), (got.shape, ref.shape)
    if ref.shape[1]:
        # every GPU direction has an oracle direction within float32 rounding, and vice versa
        dots = got.T @ ref
        assert np.mean(dots.max(1) > 1 - 1e-6) > 0.99 and np.mean(dots.max(0) > 1 - 1e-6) > 0.99
        assert np.allclose(np.linalg.norm(got, axis=0), 1, atol=1e-5)


# ------------------------------------------------------------------ exact cases (tests/kernel_cases.py)
def _sky_call(dirs, pose, cap=None, guard=8):
    """lnr_sky_rays through the C ABI: (count, out (cap + guard, 3) prefilled with NaN)."""
    from loner_amd import _lib as L
    d = torch.from_numpy(np.ascontiguousarray(dirs.T)).cuda()
    sp = L.SkyParams()
    for i in range(9):
        sp.rot[i] = float(np.asarray(pose)[:3, :3].reshape(-1)[i])
    sp.top_rows, sp.horizon_deg = 3, 10.0
    cap = int(L.lib().lnr_sky_rays_capacity()) if cap is None else cap
    out = torch.full((cap + guard, 3), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    L.call("lnr_sky_rays", d, d.shape[0], L.ctypes.byref(sp), out, cap, cnt, L.stream())
    torch.cuda.synchronize()
    return int(cnt.item()), out.cpu().numpy()


@pytest.mark.parametrize("case", ["full", "partial"])
def test_sky_rays_exact(P, case):
    """A scan built from chosen integer bins, each direction at its bin's centre (fp32 atan2 cannot flip the
    rounding): theta = -180 and 180 (the == 360 -> 0 wrap) or part of the azimuth (theta.min() > -180), phi.min() > 0,
    single-bin holes (closed), 3 x 3 holes (kept), holes at each image border, the forced top rows, a tilted pose.
    The count equals the oracle's and the directions match it in order (both row-major) to 1e-6; no candidate is
    within 1e-3 degrees of the horizon threshold (tests/test_kernel_cases_ref.py)."""
    import kernel_cases as C
    dirs, _ = C.sky_scan(case)
    ref = opre.sky_rays(dirs, C.SKY_POSE[:3, :3])
    n, out = _sky_call(dirs, C.SKY_POSE)
    assert n == ref.shape[1], (n, ref.shape)
    np.testing.assert_allclose(out[:n], ref.T, atol=1e-6, rtol=0)
    assert np.all(np.isnan(out[n:]))
    got = P.sky_rays(torch.from_numpy(np.ascontiguousarray(dirs.T)).cuda(), C.SKY_POSE).cpu().numpy()
    np.testing.assert_array_equal(got, out[:n])
    # cap below the count: the count is still the total, and nothing is written past cap
    cap = n // 2
    n2, out2 = _sky_call(dirs, C.SKY_POSE, cap=cap)
    assert n2 == n
    np.testing.assert_array_equal(out2[:cap], out[:cap])
    assert np.all(np.isnan(out2[cap:]))


def test_sky_rays_one_point(P):
    """A one-point scan: a one-row image, forced occupied by the top rows: no sky rays."""
    import kernel_cases as C
    dirs = C.bin_directions([30], [60])
    assert opre.sky_rays(dirs, C.SKY_POSE[:3, :3]).shape[1] == 0
    n, out = _sky_call(dirs, C.SKY_POSE)
    assert n == 0 and np.all(np.isnan(out))
    assert P.sky_rays(torch.from_numpy(np.ascontiguousarray(dirs.T)).cuda(), C.SKY_POSE).shape == (0, 3)


@pytest.mark.parametrize("name", ["general", "identity_rotation", "near_pi"])
def test_motion_compensate_every_point(P, name):
    """Every point of n = 1000 (no multiple of the 256-thread block) against the vectorised float64 restatement of
    the oracle (kernel_cases.motion_compensate_vec, equal to the per-point oracle: tests/test_kernel_cases_ref.py),
    at the tolerances of test_motion_compensate_vs_oracle: timestamps below t0 and above t1 (extrapolation), a
    target pose that is neither end, equal rotations with a translation (the identity flag), a relative rotation
    of pi - 1e-3."""
    import kernel_cases as C
    c = C.motion_case(name)
    d_dev = torch.from_numpy(c["dirs"].T.astype(np.float32)).cuda().contiguous()
    r_dev = torch.from_numpy(c["dists"].astype(np.float32)).cuda()
    t_dev = torch.from_numpy(c["ts"].astype(np.float32)).cuda()
    mc = P.motion_comp_params(c["start"], c["end"], c["t"][0], c["t"][1], c["target"])
    assert mc.identity == (1 if name == "identity_rotation" else 0)
    P.motion_compensate(d_dev, r_dev, t_dev, (c["start"], c["end"]), c["t"], c["target"])
    torch.cuda.synchronize()
    od, orr = C.motion_compensate_vec(c["dirs"], c["dists"], c["ts"], c["start"], c["end"], c["t"][0], c["t"][1],
                                      c["target"])
    got_d, got_r = d_dev.cpu().numpy().T, r_dev.cpu().numpy()
    print(f"motion {name}: worst |ddir| {np.abs(got_d - od).max():.2e}, worst |ddist| / dist "
          f"{(np.abs(got_r - orr) / orr).max():.2e}")
    np.testing.assert_allclose(got_d, od, atol=2e-5)
    np.testing.assert_allclose(got_r, orr, rtol=2e-5, atol=2e-5)
