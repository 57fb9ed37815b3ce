"""Mesh extraction on the GPU (loner_amd.meshing): lnr_volume_splat_max and lnr_marching_cubes_count / _emit against
their numpy restatements (validated on their own in tests/test_meshing_ref.py), and Mesher end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib
    _lib.lib()
    return _lib


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _state(S_):
    st = S_.FieldState(S_.StepConfig(), device="cuda:0", table_init=0.5, seed=7)
    torch.manual_seed(3)
    with torch.no_grad():
        st.params[2048:3072].mul_(8.0)  # a sigma head with contrast: surfaces along the rays
        st.occ.normal_(0, 2)
    st.refresh_shadow()
    return st


@pytest.fixture(scope="module")
def rendered(L):
    """96 canteen rays x 64 samples rendered as the Mesher renders them; everything the splat reads, on the GPU."""
    from loner_amd import evaluate as E
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    st = _state(S_)
    scan = syn.make_window("canteen", 1, seed=5)[0]
    keep = torch.arange(0, scan["distances"].shape[0], 97)[:96]
    scan = dict(directions=scan["directions"][:, keep].contiguous(), distances=scan["distances"][keep].contiguous(),
                pose=scan["pose"])
    rr = syn.SENSORS["canteen"]["ray_range"]
    win = E.scan_window(scan, scan["pose"], syn.world_cube("canteen"), rr, "cuda:0")
    rays, _, _ = win.build_all()
    R, S = rays.shape[0], 64
    dev = rays.device
    z = torch.empty(R, S, dtype=torch.float32, device=dev)
    w = torch.empty(R, S, dtype=torch.float32, device=dev)
    enc = torch.empty(st.cfg.n_levels, R * S, dtype=torch.int32, device=dev)
    depth, opacity, var = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(3))
    key, s = L.step_key(21, 0), L.stream(dev)
    L.call("lnr_sample_ogm", rays, R, S, st.occ, st.cfg.occ_res, st.cfg.perturb, None, None, key, 0, z, None, s)
    L.call("lnr_hashgrid_fwd_rays", L.ctypes.byref(st.desc), rays, z, R, S, st.table_f16, enc, R * S, None, 0, s)
    L.call("lnr_field_render", st.mlp_f16, enc, R * S, rays, z, R, S, 0, st.cfg.raw_noise_std, None, key, 0, depth,
           opacity, var, w, s)
    depth_max = (rr[1] - 0.25) / win.scale
    # a 13 x 9 x 7 grid over the 15 % .. 85 % quantiles of the sample points: samples fall outside on every axis
    rn, zn = host(rays), host(z)
    pts = (rn[:, None, 0:3] + rn[:, None, 3:6] * zn[:, :, None]).reshape(-1, 3).astype(np.float64)
    bounds = [np.linspace(np.quantile(pts[:, a], 0.15), np.quantile(pts[:, a], 0.85), n)
              for a, n in enumerate((13, 9, 7))]
    for a in range(3):
        assert (pts[:, a] < bounds[a][0]).any() and (pts[:, a] > bounds[a][-1]).any()
    return dict(rays=rays, z=z, w=w, depth=depth, var=var, depth_max=depth_max, bounds=bounds)


def _splat(L, d, var_max, rows=None, volume=None):
    dev = d["rays"].device
    b = [torch.from_numpy(x).to(dev) for x in d["bounds"]]
    n = [len(x) for x in d["bounds"]]
    vol = torch.zeros(n[0] * n[1] * n[2], dtype=torch.float32, device=dev) if volume is None else volume
    sl = slice(None) if rows is None else rows
    rays, z, w = d["rays"][sl].contiguous(), d["z"][sl].contiguous(), d["w"][sl].contiguous()
    L.call("lnr_volume_splat_max", rays, z, w, d["depth"][sl].contiguous(), d["var"][sl].contiguous(), rays.shape[0],
           z.shape[1], b[0], n[0], b[1], n[1], b[2], n[2], d["depth_max"], var_max, vol, L.stream(dev))
    return vol


@pytest.mark.parametrize("with_variance", [False, True])
def test_splat_matches_reference(L, rendered, with_variance):
    from loner_amd import meshing as M
    d = rendered
    var = host(d["var"])
    var_max = float(np.median(var)) if with_variance else 0.0
    if with_variance:
        assert 0 < (var < np.float32(var_max)).sum() < len(var)
    got = host(_splat(L, d, var_max))
    ref = M.splat_max_ref(host(d["rays"]), host(d["z"]), host(d["w"]), host(d["depth"]), var, *d["bounds"],
                          depth_max=d["depth_max"], var_max=var_max)
    frac = float((ref > 0).mean())
    print(f"non-zero cells: {frac:.3f} (gpu {float((got > 0).mean()):.3f}), zero-weight samples "
          f"{float((host(d['w']) == 0).mean()):.3f}")
    np.testing.assert_array_equal(got, ref)  # a maximum of identical floats has no rounding
    assert 0.05 < frac < 0.95, frac
    # the rays in two calls: the same volume, bit for bit
    vol = _splat(L, d, var_max, slice(0, 40))
    vol = _splat(L, d, var_max, slice(40, None), volume=vol)
    assert torch.equal(vol, torch.from_numpy(got).to(vol.device))


def test_splat_error_contract(L, rendered):
    d = rendered
    dev = d["rays"].device
    b = torch.from_numpy(d["bounds"][0]).to(dev)
    vol = torch.zeros(8, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.call("lnr_volume_splat_max", d["rays"], d["z"], d["w"], d["depth"], None, 96, 64, b, 2, b, 2, None, 2,
               1.0, 0.0, vol, L.stream(dev))
    with pytest.raises(RuntimeError, match="bad grid"):
        L.call("lnr_volume_splat_max", d["rays"], d["z"], d["w"], d["depth"], None, 96, 64, b, 0, b, 2, b, 2,
               1.0, 0.0, vol, L.stream(dev))
    with pytest.raises(RuntimeError, match="needs variance"):
        L.call("lnr_volume_splat_max", d["rays"], d["z"], d["w"], d["depth"], None, 96, 64, b, 2, b, 2, b, 2,
               1.0, 0.5, vol, L.stream(dev))


def _mc_volumes():
    from loner_amd import meshing as M
    rng = np.random.default_rng(11)
    return {
        "sphere": (M.sphere_volume(24, 8.0), 0.0, (1.0, 1.0, 1.0)),
        "binary": ((rng.uniform(size=(8, 8, 8)) < 0.5).astype(np.float32), 0.5, (1.0, 1.0, 1.0)),
        "float": (rng.normal(size=(9, 12, 7)).astype(np.float32), 0.1, (0.5, 1.0, 2.0)),
    }


@pytest.mark.parametrize("name", ["sphere", "binary", "float"])
def test_marching_cubes_matches_reference(L, name):
    from loner_amd import meshing as M
    vol, level, sp = _mc_volumes()[name]
    rv, rf = M.marching_cubes_ref(vol, level, sp)
    verts, faces = M.marching_cubes(torch.from_numpy(vol).cuda(), level, sp)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert len(rf) > 0
    np.testing.assert_array_equal(host(faces), rf)
    np.testing.assert_allclose(host(verts), rv, rtol=1e-6, atol=1e-6 * np.abs(rv).max())


def test_marching_cubes_all_outside(L):
    from loner_amd import meshing as M
    verts, faces = M.marching_cubes(torch.zeros(5, 6, 7, device="cuda"), 0.5)
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3)


def test_mesher_end_to_end(L, tmp_path):
    from loner_amd import meshing as M
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    st = _state(S_)
    poses = [torch.from_numpy(p.astype(np.float32)) for p in syn.keyframe_poses("canteen", 2, None)]
    bound = [[-20, 30], [-12, 20], [-2, 6]]
    mesher = M.Mesher(st, poses, syn.world_cube("canteen"), syn.SENSORS["canteen"]["ray_range"], resolution=2.0,
                      marching_cubes_bound=bound, level_set=0, lidar_vertical_fov=(-22.5, 22.5), chunk=2048,
                      vertical_resolution=2.0, horizontal_resolution=2.0)
    assert [len(b) for b in mesher.xyz] == [25, 16, 4]
    verts, faces = mesher.get_mesh(skip_step=1, key=5)
    assert 0 < mesher.n_rays <= 2 * 23 * 180
    assert verts.is_cuda and verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert len(verts) > 0 and len(faces) > 0
    vol = host(mesher.volume())
    assert vol.shape == (25, 16, 4)
    rv, rf = M.marching_cubes_ref(vol, 0.0, mesher.spacing())
    np.testing.assert_array_equal(host(faces), rf)
    want = mesher.to_world(rv)
    v = host(verts)
    np.testing.assert_allclose(v, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    # inside the bound, up to float32 rounding of a coordinate of at most 30 m (eps 1.2e-7 x 30 x a few operations)
    lo, hi = np.array(bound, np.float64).T
    assert (v >= lo - 1e-4).all() and (v <= hi + 1e-4).all()
    # the same key again: bitwise the same mesh
    verts2, faces2 = mesher.get_mesh(skip_step=1, key=5)
    assert torch.equal(verts, verts2) and torch.equal(faces, faces2)
    M.write_ply(tmp_path / "mesh.ply", verts, faces)
    assert (tmp_path / "mesh.ply").stat().st_size > 13 * len(faces)
