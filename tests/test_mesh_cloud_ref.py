"""The float64 numpy restatements of loner_amd.mesh_cloud (the GPU tests' oracle) on cases worked by hand, and the PLY
reader and writer of loner_amd.meshing.  No GPU."""
import numpy as np
import pytest

from loner_amd import mesh_cloud as MC
from loner_amd import meshing as M
from oracle import rng as orng

RIGHT = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)


def two_faces():
    """Coplanar triangles of areas 1 and 3."""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, -3, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1]], np.int32)


@pytest.fixture(scope="module")
def sphere():
    v, f = M.marching_cubes_ref(M.sphere_volume(24, 8.0), 0)
    assert v.shape == (1248, 3) and f.shape == (2492, 3)
    return v, f


def test_right_triangle():
    area, normal = MC.face_areas_ref(*RIGHT, return_normals=True)
    assert area.dtype == np.float64 and normal.dtype == np.float32
    np.testing.assert_array_equal(area, [0.5])
    np.testing.assert_array_equal(normal, [[0, 0, 1]])


def test_bounds_and_faces_of_two_triangles():
    v, f = two_faces()
    area = MC.face_areas_ref(v, f)
    np.testing.assert_array_equal(area, [1.0, 3.0])
    bounds = MC.sample_bounds_ref(area, 8)
    np.testing.assert_array_equal(bounds, [2, 8])
    np.testing.assert_array_equal(MC.sample_bounds_ref(None, 8, cum=np.array([1.0, 4.0])), [2, 8])
    p, face_of = MC.sample_points_ref(v, f, bounds)
    np.testing.assert_array_equal(face_of, [0, 0, 1, 1, 1, 1, 1, 1])
    assert p.shape == (8, 3) and p.dtype == np.float32 and (p[:, 2] == 0).all()
    assert (p[:2, 1] >= 0).all() and (p[2:, 1] <= 0).all()
    # chunks are the whole run's rows; a point index past the last bound has no face
    q, fq = MC.sample_points_ref(v, f, bounds, first=1, count=5)
    np.testing.assert_array_equal(q, p[1:6])
    np.testing.assert_array_equal(fq, face_of[1:6])
    z, fz = MC.sample_points_ref(v, f, bounds, first=7, count=2)
    np.testing.assert_array_equal(fz, [1, -1])
    np.testing.assert_array_equal(z[1], 0)
    # another key moves the points, not the allocation
    p2, f2 = MC.sample_points_ref(v, f, bounds, key=1)
    np.testing.assert_array_equal(f2, face_of)
    assert (p2 != p).any()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_zero_area_face_gets_no_point(where):
    v, f = two_faces()
    v = np.concatenate((v, [[5, 5, 5]])).astype(np.float32)
    flat = np.array([[4, 4, 4]], np.int32)  # a face collapsed to a point
    k = {"first": 0, "middle": 1, "last": 2}[where]
    f = np.insert(f, k if k < 2 else 2, flat, axis=0)
    area = MC.face_areas_ref(v, f)
    assert area[k] == 0 and (np.delete(area, k) > 0).all()
    bounds = MC.sample_bounds_ref(area, 100)
    assert bounds[-1] == 100
    _, face_of = MC.sample_points_ref(v, f, bounds)
    assert len(face_of) == 100 and (face_of != k).all() and (face_of >= 0).all()
    np.testing.assert_array_equal(np.bincount(face_of, minlength=3), np.insert([25, 75], k, 0))


def test_bad_index_is_a_face_without_area():
    v, f = two_faces()
    for bad in (len(v), -1):
        g = f.copy()
        g[1, 2] = bad
        area, normal = MC.face_areas_ref(v, g, return_normals=True)
        np.testing.assert_array_equal(area, [1.0, 0.0])
        np.testing.assert_array_equal(normal[1], [0, 0, 1])
        _, face_of = MC.sample_points_ref(v, g, MC.sample_bounds_ref(area, 10))
        assert (face_of == 0).all()
        assert np.isfinite(MC.vertex_normals_ref(v, g)).all()


def test_weights_and_planes(sphere):
    v, f = sphere
    area = MC.face_areas_ref(v, f)
    p, face_of, w = MC.sample_points_ref(v, f, MC.sample_bounds_ref(area, 20000), key=3, return_weights=True)
    assert (w >= 0).all()
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 2.0 ** -52
    _, normal = MC.face_areas_ref(v, f, return_normals=True)
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    v0 = v[f[face_of, 0]].astype(np.float64)
    off = np.abs(((p.astype(np.float64) - v0) * normal[face_of].astype(np.float64)).sum(axis=1))
    print(f"largest distance from the face's plane: {off.max():.3g} of extent {extent:.3g}")
    assert off.max() <= 1e-6 * extent


def test_generator_equals_the_oracle():
    r = np.random.default_rng(0)
    key, i, b = (r.integers(0, 2 ** 32, 1000, dtype=np.uint64) for _ in range(3))
    for k in range(1000):
        assert MC.rand_u32(int(key[k]), MC.STREAM_MESH, i[k], b[k]) == orng.rand_u32(int(key[k]), 7, i[k], b[k])
    np.testing.assert_array_equal(MC.rand_u32(12345, 7, i, b), orng.rand_u32(12345, 7, i, b))
    u = MC.rand_uniform(12345, 7, i, b)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    np.testing.assert_array_equal(u, orng.uniform(12345, 7, i, b))


@pytest.mark.parametrize("key", [0, 1, 12345])
def test_uniform_on_one_triangle(key):
    n = 65536
    _, _, w = MC.sample_points_ref(*RIGHT, np.array([n]), key=key, return_weights=True)
    # a barycentric coordinate of a uniform point has mean 1/3 and variance 1/18
    sigma = np.sqrt(1.0 / 18.0) / np.sqrt(n)
    dev = np.abs(w.mean(axis=0) - 1.0 / 3.0) / sigma
    # the four midpoint sub-triangles hold a quarter of the area each: a corner's where its weight is above 1/2
    counts = np.array([(w[:, k] > 0.5).sum() for k in range(3)] + [(w <= 0.5).all(axis=1).sum()])
    assert counts.sum() == n
    chi2 = float(((counts - n / 4.0) ** 2 / (n / 4.0)).sum())
    print(f"key {key}: means off by {dev} sigma, chi2 {chi2:.2f}")
    assert (dev <= 5).all()
    assert chi2 < 16.3  # the 0.999 quantile at 3 degrees of freedom


def test_sphere_samples_and_normals(sphere):
    v, f = sphere
    area = MC.face_areas_ref(v, f)
    assert (area > 0).all()
    n = 200000
    bounds = MC.sample_bounds_ref(area, n)
    p, face_of = MC.sample_points_ref(v, f, bounds, key=0)
    per_face = np.bincount(face_of, minlength=len(f))
    print(f"points per face: {per_face.min()} .. {per_face.max()}")
    assert len(p) == n and per_face.min() >= 3 and per_face.max() <= 177
    # the stratified allocation: every face within one point of its share
    assert np.abs(per_face - area / area.sum() * n).max() <= 1.0
    c = np.float64((24 - 1) / 2.0)
    dv = np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - 8.0).max()
    dp = np.abs(np.linalg.norm(p.astype(np.float64) - c, axis=1) - 8.0).max()
    print(f"radius error: vertices {dv:.4f}, samples {dp:.4f}")
    # a chord of at most sqrt(3) cells on a radius of 8 has a sagitta of 8 - sqrt(64 - 3 / 4) < 3 / 64
    assert dp <= dv + 3.0 / 64.0
    nv = MC.vertex_normals_ref(v, f).astype(np.float64)
    assert np.abs(np.linalg.norm(nv, axis=1) - 1.0).max() < 1e-6
    radial = v.astype(np.float64) - c
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (nv * radial).sum(axis=1)
    print(f"normal . radial >= {dots.min():.4f}")
    assert dots.min() >= 0.99
    valence = np.bincount(f.reshape(-1), minlength=len(v))
    assert 4 <= valence.min() and valence.max() <= 9


def test_octahedron_normals_are_the_axes():
    area, fn = MC.face_areas_ref(OCTA_V, OCTA_F, return_normals=True)
    np.testing.assert_allclose(area, np.sqrt(3.0) / 2.0, rtol=1e-15)
    assert ((fn * OCTA_V[OCTA_F].mean(axis=1)) .sum(axis=1) > 0).all()  # wound outwards
    np.testing.assert_array_equal(MC.vertex_normals_ref(OCTA_V, OCTA_F), OCTA_V)
    # an isolated vertex
    v = np.concatenate((OCTA_V, [[9, 9, 9]])).astype(np.float32)
    np.testing.assert_array_equal(MC.vertex_normals_ref(v, OCTA_F)[-1], [0, 0, 1])
    # the row order: corners in ascending index, whatever the order of the faces
    perm, start = MC.vertex_rows_ref(OCTA_F, 6)
    assert start[0] == 0 and start[-1] == 24 and (np.diff(start) == 4).all()
    for k in range(6):
        row = perm[start[k]:start[k + 1]]
        assert (np.diff(row) > 0).all() and (OCTA_F.reshape(-1)[row] == k).all()


# ---------------------------------------------------------------------------------------------- PLY
def old_ply_bytes(v, f):
    """The file ``write_ply`` wrote before it knew normals, spelled out."""
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
            f"property float z\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    body = v.astype("<f4").tobytes() + b"".join(b"\x03" + row.astype("<i4").tobytes() for row in f)
    return head.encode("ascii") + body


def test_ply_round_trip(tmp_path, sphere):
    v, f = sphere
    n = MC.vertex_normals_ref(v, f)
    path = str(tmp_path / "a.ply")
    M.write_ply(path, v, f)
    assert open(path, "rb").read() == old_ply_bytes(v, f)
    rv, rf, rn = M.read_ply(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32 and rn is None
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rf, f)
    M.write_ply(path, v, f, n)
    rv, rf, rn = M.read_ply(path)
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rf, f)
    np.testing.assert_array_equal(rn, n)
    with pytest.raises(ValueError):
        M.write_ply(path, v, f, n[:-1])


def other_ply(path, v, f, n, fmt, real, colours, index="int"):
    """A PLY as Open3D writes it: double or float coordinates, optional normals and uchar colours."""
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
    head = [f"ply\nformat {fmt} 1.0\ncomment Created by Open3D\nelement vertex {len(v)}\n"]
    head += [f"property {real} {a}\n" for a in names]
    head += [f"property uchar {a}\n" for a in ("red", "green", "blue")] if colours else []
    head += [f"element face {len(f)}\nproperty list uchar {index} vertex_indices\nend_header\n"]
    cols = np.concatenate((v, n), axis=1) if n is not None else v
    rgb = (np.arange(len(v) * 3).reshape(-1, 3) % 251).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write("".join(head).encode("ascii"))
        if fmt == "ascii":
            for k in range(len(v)):
                row = [repr(float(x)) for x in cols[k]] + ([str(int(c)) for c in rgb[k]] if colours else [])
                fh.write((" ".join(row) + "\n").encode("ascii"))
            for row in f:
                fh.write(("3 " + " ".join(str(int(i)) for i in row) + "\n").encode("ascii"))
        else:
            r = "<f8" if real == "double" else "<f4"
            dt = [(a, r) for a in names] + ([(a, "u1") for a in ("red", "green", "blue")] if colours else [])
            rec = np.zeros(len(v), dtype=dt)
            for k, a in enumerate(names):
                rec[a] = cols[:, k]
            if colours:
                for k, a in enumerate(("red", "green", "blue")):
                    rec[a] = rgb[:, k]
            frec = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<u4" if index == "uint" else "<i4", (3,))])
            frec["n"], frec["i"] = 3, f
            fh.write(rec.tobytes() + frec.tobytes())


@pytest.mark.parametrize("fmt", ["binary_little_endian", "ascii"])
@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("normals,colours,index", [(False, False, "int"), (True, True, "uint"), (True, False, "int"),
                                                   (False, True, "int")])
def test_read_ply_other_writers(tmp_path, fmt, real, normals, colours, index):
    v, f = OCTA_V * np.float32(1.1), OCTA_F
    n = MC.vertex_normals_ref(v, f) if normals else None
    path = str(tmp_path / "o.ply")
    other_ply(path, v, f, n, fmt, real, colours, index)
    rv, rf, rn = M.read_ply(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rf, f)
    if normals:
        np.testing.assert_array_equal(rn, n)
    else:
        assert rn is None


@pytest.mark.parametrize("old,new", [
    ("format binary_little_endian 1.0", "format binary_big_endian 1.0"),
    ("property float z", "property int z"),
    ("property list uchar int vertex_indices", "property list uchar float vertex_indices"),
    ("property list uchar int vertex_indices", "property list int int vertex_indices"),
    ("element face", "element edge"),
    ("property float y", "property list uchar float y"),
])
def test_read_ply_names_the_line_it_refuses(tmp_path, old, new):
    path = str(tmp_path / "bad.ply")
    M.write_ply(path, OCTA_V, OCTA_F)
    raw = open(path, "rb").read()
    assert old.encode() in raw
    open(path, "wb").write(raw.replace(old.encode(), new.encode(), 1))
    with pytest.raises(ValueError) as e:
        M.read_ply(path)
    line = next(ln for ln in raw.replace(old.encode(), new.encode(), 1).decode("latin1").splitlines() if new in ln)
    assert line in str(e.value), str(e.value)


def test_read_ply_refuses_a_quad_and_a_short_file(tmp_path):
    path = str(tmp_path / "q.ply")
    M.write_ply(path, OCTA_V, OCTA_F)
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-5])
    with pytest.raises(ValueError):
        M.read_ply(path)
    cut = len(raw) - 13 * len(OCTA_F)
    open(path, "wb").write(raw[:cut] + b"\x04" + raw[cut + 1:])
    with pytest.raises(ValueError):
        M.read_ply(path)
