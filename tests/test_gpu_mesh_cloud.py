"""Mesh sampling and vertex normals on the GPU (loner_amd.mesh_cloud) against their float64 numpy restatements
(validated on their own in tests/test_mesh_cloud_ref.py): equal bits wherever the operation order is fixed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
ONE = (np.array([[0.25, -1, 2], [3, 0.5, 2.5], [-1, 4, 0.125]], np.float32), np.array([[0, 1, 2]], np.int32))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loner_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def MC(L):
    from loner_amd import mesh_cloud
    return mesh_cloud


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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    i = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(i), b.view(i))


@pytest.fixture(scope="module")
def sphere():
    from loner_amd import meshing as M
    v, f = M.marching_cubes_ref(M.sphere_volume(24, 8.0), 0)
    assert v.shape == (1248, 3) and f.shape == (2492, 3)
    return v, f


def two_faces():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, -3, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1]], np.int32)


def degenerate_mesh():
    """Six faces: a point, a proper one, a segment (two equal corners), a proper one, collinear corners, a point."""
    v = np.array([[0, 0, 0], [1.5, 0, 0], [0, 2.5, 0.5], [3, 0, 0], [-1, -1, 4], [0.5, 0.25, 7]], np.float32)
    f = np.array([[4, 4, 4], [0, 1, 2], [1, 1, 2], [2, 4, 5], [0, 1, 3], [5, 5, 5]], np.int32)
    return v, f


def big_and_small(sphere):
    """The sphere mesh scaled by 1e-3, one face of 4 x 10^3 times its whole area, the small sphere again."""
    sv, sf = sphere
    small = sv * np.float32(1e-3)
    big = np.array([[0, 0, 5], [2, 0, 5], [0, 3, 5]], np.float32)
    v = np.concatenate((small, big, small + np.float32(1.0)))
    f = np.concatenate((sf, [[len(sv), len(sv) + 1, len(sv) + 2]], sf + len(sv) + 3)).astype(np.int32)
    return v, f


# ---------------------------------------------------------------------------------------------- areas, face normals
@pytest.mark.parametrize("mesh", ["sphere", "octahedron", "degenerate"])
def test_face_areas(MC, sphere, mesh):
    v, f = {"sphere": sphere, "octahedron": (OCTA_V, OCTA_F), "degenerate": degenerate_mesh()}[mesh]
    ra, rn = MC.face_areas_ref(v, f, return_normals=True)
    a, n = MC.face_areas(dev(v), dev(f), return_normals=True)
    assert a.dtype == torch.float64 and n.dtype == torch.float32 and n.shape == (len(f), 3)
    same_bits(host(a), ra)
    print(f"{mesh}: normals differ by at most {ulps(host(n), rn).max()} ulp")
    assert ulps(host(n), rn).max() <= 1
    if mesh == "degenerate":
        np.testing.assert_array_equal(ra > 0, [False, True, False, True, False, False])
        np.testing.assert_array_equal(host(n)[[0, 2, 4, 5]], [[0, 0, 1]] * 4)
    same_bits(host(MC.face_areas(dev(v), dev(f))), ra)  # without normals


# ---------------------------------------------------------------------------------------------- the scan
def test_scan_and_bounds(MC, sphere):
    v, f = sphere
    area = MC.face_areas(dev(v), dev(f))
    cum = host(torch.cumsum(area, 0))
    seq = np.cumsum(host(area))
    bound = (len(f) - 1) * 2.0 ** -53 * host(area).sum()  # any order of summation
    print(f"device scan against the sequential one: {np.abs(cum - seq).max():.3g} (bound {bound:.3g})")
    assert np.abs(cum - seq).max() <= bound
    for n in (1, 300, 200000, (1 << 20) + 3, 50_000_000):
        b = host(MC.sample_bounds(area, n))
        assert b.dtype == np.int64
        np.testing.assert_array_equal(b, MC.sample_bounds_ref(None, n, cum=cum))
        assert b[-1] == n and (np.diff(b) >= 0).all()


# ---------------------------------------------------------------------------------------------- the sampler
def check_sample(MC, v, f, n, key=0):
    """The device's points and faces against the restatement fed the device's bounds; returns the device's."""
    dv, df = dev(v), dev(f)
    bounds = host(MC.sample_bounds(MC.face_areas(dv, df), n))
    rp, rf = MC.sample_points_ref(v, f, bounds, key=key)
    p, face_of = MC.sample_points_uniformly(dv, df, n, key=key, return_faces=True)
    assert p.dtype == torch.float32 and p.shape == (n, 3) and face_of.dtype == torch.int32
    np.testing.assert_array_equal(host(face_of), rf)
    same_bits(host(p), rp)
    assert (rf >= 0).all()
    return p, face_of, bounds


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_one_face(MC, n):
    check_sample(MC, *ONE, n, key=n)


def test_two_faces(MC):
    _, face_of, bounds = check_sample(MC, *two_faces(), 8)
    np.testing.assert_array_equal(bounds, [2, 8])
    np.testing.assert_array_equal(host(face_of), [0, 0, 1, 1, 1, 1, 1, 1])


@pytest.mark.parametrize("n", [300, 200000, (1 << 20) + 3])
def test_sphere(MC, sphere, n):
    _, face_of, bounds = check_sample(MC, *sphere, n, key=5)
    span = np.searchsorted(bounds, min(255, n - 1), side="right") - np.searchsorted(bounds, 0, side="right") + 1
    print(f"n = {n}: the first block spans {span} faces")
    if n == 300:
        assert span > 1024  # more than the LDS stage holds: the search in global memory
    else:
        assert span < 64


def test_blocks_inside_one_face(MC, sphere):
    v, f = big_and_small(sphere)
    _, face_of, bounds = check_sample(MC, v, f, 3000, key=2)
    per_face = np.bincount(host(face_of), minlength=len(f))
    big = len(sphere[1])
    assert per_face[big] >= 2990 and (per_face == 0).sum() >= len(f) - 12


@pytest.mark.parametrize("where", [0, 1, 2])
def test_zero_area_faces_get_no_point(MC, where):
    v, f = two_faces()
    v = np.concatenate((v, [[5, 5, 5]])).astype(np.float32)
    f = np.insert(f, where, [[4, 4, 4]], axis=0).astype(np.int32)
    _, face_of, _ = check_sample(MC, v, f, 1000)
    np.testing.assert_array_equal(np.bincount(host(face_of), minlength=3), np.insert([250, 750], where, 0))


def test_chunks_runs_and_keys(MC, sphere):
    v, f = sphere
    dv, df = dev(v), dev(f)
    n = 5000
    p, face_of = MC.sample_points_uniformly(dv, df, n, key=9, return_faces=True)
    # uneven cuts, the first of them inside a face's run
    fo = host(face_of)
    inside = np.nonzero(fo[:-1] == fo[1:])[0] + 1
    cut = int(inside[inside > 1000][0])
    assert fo[cut - 1] == fo[cut] and cut % 256 != 0
    parts = [MC.sample_points_uniformly(dv, df, n, key=9, return_faces=True, first=a, count=b - a)
             for a, b in ((0, cut), (cut, 1300), (1300, n))]
    same_bits(host(torch.cat([q for q, _ in parts])), host(p))
    np.testing.assert_array_equal(host(torch.cat([q for _, q in parts])), fo)
    p2, f2 = MC.sample_points_uniformly(dv, df, n, key=9, return_faces=True)
    assert torch.equal(p, p2) and torch.equal(face_of, f2)
    p3, f3 = MC.sample_points_uniformly(dv, df, n, key=10, return_faces=True)
    assert torch.equal(face_of, f3) and not torch.equal(p, p3)
    assert MC.sample_points_uniformly(dv, df, n, key=9, first=n).shape == (0, 3)


# ---------------------------------------------------------------------------------------------- guards
@pytest.mark.parametrize("bad", ["n_verts", -1])
def test_bad_index(MC, L, bad):
    v, f = two_faces()
    f = f.copy()
    f[1, 1] = len(v) if bad == "n_verts" else -1
    dv, df = dev(v), dev(f)
    s = L.stream(dv.device)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    area = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    normal = torch.full((2, 3), -1.0, dtype=torch.float32, device="cuda")
    L.call("lnr_mesh_face_areas", dv, len(v), df, 2, area, normal, status, s)
    assert int(status.item()) == L.MESH_BAD_INDEX
    np.testing.assert_array_equal(host(area), [1.0, 0.0])
    np.testing.assert_array_equal(host(normal), [[0, 0, 1], [0, 0, 1]])
    bounds = MC.sample_bounds(area, 300)
    np.testing.assert_array_equal(host(bounds), [300, 300])
    status.zero_()
    points = torch.empty(300, 3, dtype=torch.float32, device="cuda")
    face_of = torch.empty(300, dtype=torch.int32, device="cuda")
    L.call("lnr_mesh_sample_points", dv, len(v), df, 2, bounds, 0, 300, 0, points, face_of, status, s)
    assert int(status.item()) == 0 and (host(face_of) == 0).all()  # the bad face is never reached
    # bounds that do hand it points: zeros, face -1, the status bit; a point past the last bound: the other bit
    wrong = dev(np.array([100, 299], np.int64))
    L.call("lnr_mesh_sample_points", dv, len(v), df, 2, wrong, 0, 300, 0, points, face_of, status, s)
    assert int(status.item()) == L.MESH_BAD_INDEX | L.MESH_NO_FACE
    np.testing.assert_array_equal(host(face_of), [0] * 100 + [-1] * 200)
    np.testing.assert_array_equal(host(points)[100:], 0)
    normals = torch.empty(len(v), 3, dtype=torch.float32, device="cuda")
    status.zero_()
    perm, rows = MC.vertex_rows(df, len(v))
    L.call("lnr_mesh_vertex_normals", dv, len(v), df, 2, perm, rows, normals, status, s)
    assert int(status.item()) == L.MESH_BAD_INDEX
    same_bits(host(normals), MC.vertex_normals_ref(v, f))
    for call in (lambda: MC.face_areas(dv, df), lambda: MC.sample_points_uniformly(dv, df, 10),
                 lambda: MC.vertex_normals(dv, df)):
        with pytest.raises(RuntimeError, match="face index"):
            call()


def test_argument_errors(MC, L):
    v, f = two_faces()
    dv, df = dev(v), dev(f)
    lib, s = L.lib(), L.stream(dv.device)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    area = torch.zeros(2, dtype=torch.float64, device="cuda")
    bounds = dev(np.array([2, 8], np.int64))
    points = torch.zeros(8, 3, dtype=torch.float32, device="cuda")
    normals = torch.zeros(4, 3, dtype=torch.float32, device="cuda")
    perm, rows = MC.vertex_rows(df, 4)
    P = L.ptr
    top = L.CLOUD_MAX_POINTS
    refused = [
        lib.lnr_mesh_face_areas(None, 4, P(df), 2, P(area), None, P(status), s),
        lib.lnr_mesh_face_areas(P(dv), 4, None, 2, P(area), None, P(status), s),
        lib.lnr_mesh_face_areas(P(dv), 4, P(df), 2, None, None, P(status), s),
        lib.lnr_mesh_face_areas(P(dv), 4, P(df), 2, P(area), None, None, s),
        lib.lnr_mesh_face_areas(P(dv), 4, P(df), 0, P(area), None, P(status), s),
        lib.lnr_mesh_face_areas(P(dv), 0, P(df), 2, P(area), None, P(status), s),
        lib.lnr_mesh_face_areas(P(dv), 4, P(df), top + 1, P(area), None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, None, 0, 8, 0, P(points), None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, P(bounds), 0, 8, 0, None, None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 0, P(bounds), 0, 8, 0, P(points), None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, P(bounds), top - 7, 8, 0, P(points), None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, P(bounds), -1, 8, 0, P(points), None, P(status), s),
        lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, P(bounds), 0, -1, 0, P(points), None, P(status), s),
        lib.lnr_mesh_vertex_normals(P(dv), 4, P(df), 2, None, P(rows), P(normals), P(status), s),
        lib.lnr_mesh_vertex_normals(P(dv), 4, P(df), 2, P(perm), None, P(normals), P(status), s),
        lib.lnr_mesh_vertex_normals(P(dv), 4, P(df), 2, P(perm), P(rows), None, P(status), s),
        lib.lnr_mesh_vertex_normals(P(dv), 4, P(df), 0, P(perm), P(rows), P(normals), P(status), s),
    ]
    assert refused == [L.ERR_ARG] * len(refused)
    assert b"lnr_mesh_vertex_normals" in lib.lnr_last_error()
    assert lib.lnr_mesh_sample_points(P(dv), 4, P(df), 2, P(bounds), 8, 0, 0, None, None, P(status), s) == 0  # nothing
    assert int(status.item()) == 0
    for call in (lambda: MC.sample_points_uniformly(dv, df, 0), lambda: MC.sample_points_uniformly(dv, df, top + 1),
                 lambda: MC.sample_points_uniformly(dv, df, 8, first=4, count=5),
                 lambda: MC.face_areas(dv, df.long()), lambda: MC.face_areas(dv.double(), df)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------- vertex normals
@pytest.mark.parametrize("mesh", ["sphere", "octahedron"])
def test_vertex_normals(MC, sphere, mesh):
    v, f = sphere if mesh == "sphere" else (OCTA_V, OCTA_F)
    v = np.concatenate((v, [[40, 40, 40]])).astype(np.float32)  # an isolated vertex
    ref = MC.vertex_normals_ref(v, f)
    n = MC.vertex_normals(dev(v), dev(f))
    assert n.dtype == torch.float32 and n.shape == (len(v), 3)
    print(f"{mesh}: vertex normals differ by at most {ulps(host(n), ref).max()} ulp")
    assert ulps(host(n), ref).max() <= 1
    np.testing.assert_array_equal(host(n)[-1], [0, 0, 1])
    if mesh == "octahedron":
        np.testing.assert_array_equal(host(n)[:-1], OCTA_V)
    assert torch.equal(n, MC.vertex_normals(dev(v), dev(f)))
    perm = np.random.default_rng(3).permutation(len(f))
    n2 = MC.vertex_normals(dev(v), dev(f[perm]))
    print(f"{mesh}: with the faces permuted, at most {ulps(host(n2), host(n)).max()} ulp")
    assert ulps(host(n2), host(n)).max() <= 1
    # the rows the kernel walks are the restatement's
    dp, dr = MC.vertex_rows(dev(f), len(v))
    rp, rr = MC.vertex_rows_ref(f, len(v))
    np.testing.assert_array_equal(host(dp), rp)
    np.testing.assert_array_equal(host(dr), rr)


# ---------------------------------------------------------------------------------------------- end to end
def test_mesh_to_cloud_end_to_end(MC):
    from loner_amd import map_eval as ME
    from loner_amd import meshing as M
    verts, faces = M.marching_cubes(dev(M.sphere_volume(24, 8.0)), 0.0)
    v, f = host(verts), host(faces)
    assert v.shape == (1248, 3) and f.shape == (2492, 3)
    n, res = 200000, 0.5
    bounds = host(MC.sample_bounds(MC.face_areas(verts, faces), n))
    rp, _ = MC.sample_points_ref(v, f, bounds, key=4)
    rm, rc, rk = ME.voxel_down_sample_ref(rp, res, return_counts=True, return_keys=True)
    cloud = MC.mesh_to_cloud(verts, faces, res, number_of_points=n, key=4)
    assert cloud.dtype == torch.float32 and cloud.shape == (len(rk), 3)
    m, c, k = ME.voxel_filter(MC.sample_points_uniformly(verts, faces, n, key=4), res, return_keys=True)
    assert torch.equal(m, cloud)
    np.testing.assert_array_equal(host(k), rk)
    np.testing.assert_array_equal(host(c), rc)
    assert ulps(host(m), rm).max() <= 1


def test_evaluate_mesh_on_a_sphere(MC):
    """The marching-cubes sphere against 20000 points of the analytic one.  Not aligned: a sphere has no unique
    alignment onto itself, and none is needed."""
    from loner_amd import meshing as M
    verts, faces = M.marching_cubes(dev(M.sphere_volume(24, 8.0)), 0.0)
    k = np.arange(20000) + 0.5
    z = 1.0 - 2.0 * k / 20000
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    gt = (11.5 + 8.0 * np.stack((r * np.cos(phi), r * np.sin(phi), z), axis=1)).astype(np.float32)
    voxel = 0.25
    stats = MC.evaluate_mesh(verts, faces, dev(gt), f_score_threshold=0.5, voxel_size=voxel, number_of_points=200000,
                             align=False)
    print(stats)
    assert set(stats) == {"accuracy", "completion", "chamfer_distance", "recall", "precision", "f-score", "num_points"}
    assert all(np.isfinite(x) for x in stats.values())
    # a sample is within 0.0144 + 3 / 64 = 0.0613 of the sphere (tests/test_mesh_cloud_ref.py); a voxel's mean and its
    # nearest neighbour in the other cloud add at most the voxel size
    assert stats["accuracy"] < 0.0613 + voxel and stats["completion"] < 0.0613 + voxel
    assert stats["precision"] == 1.0 and stats["recall"] == 1.0
