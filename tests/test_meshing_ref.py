"""Mesh extraction, CPU side (loner_amd.meshing / loner_amd.mc_table): the generated marching-cubes table and the
conventions of the numpy restatements that the GPU kernels are tested against (tests/test_gpu_meshing.py)."""
import os

import numpy as np
import pytest

from loner_amd import mc_table as T
from loner_amd import meshing as M


def _directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def _assert_closed(faces, n_verts):
    """Every undirected edge occurs in exactly two triangles, once in each direction."""
    e = _directed_edges(faces)
    assert (e[:, 0] != e[:, 1]).all()
    code = e[:, 0] * n_verts + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    back = e[:, 1] * n_verts + e[:, 0]
    assert np.array_equal(np.sort(code), np.sort(back)), "a directed edge has no opposite"


def _euler(verts, faces):
    e = np.sort(_directed_edges(faces), axis=1)
    n_edges = len(np.unique(e[:, 0] * len(verts) + e[:, 1]))
    used = len(np.unique(faces))
    assert used == len(verts)  # no vertex without a triangle
    return len(verts) - n_edges + len(faces)


def _signed_volume_area(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0
    return vol, area


def torus_volume(n=32, major=9.0, minor=4.0):
    g = np.arange(n, dtype=np.float32) - np.float32((n - 1) / 2.0)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    q = np.sqrt(x ** 2 + y ** 2) - np.float32(major)
    return (np.float32(minor) - np.sqrt(q ** 2 + z ** 2)).astype(np.float32)


def test_table_header_matches_generator():
    with open(T.HEADER_PATH) as f:
        assert f.read() == T.header_text(), "csrc/mc_table.hpp is stale: run python -m loner_amd.mc_table"


def test_table_shape():
    assert T.TRI_TABLE.shape == (256, 3 * T.MAX_TRIS) and T.TRI_COUNT.shape == (256,)
    assert T.TRI_COUNT[0] == 0 and T.TRI_COUNT[255] == 0 and (T.TRI_COUNT[1:255] > 0).all()
    for case in range(256):
        n = 3 * int(T.TRI_COUNT[case])
        assert (T.TRI_TABLE[case, :n] >= 0).all() and (T.TRI_TABLE[case, :n] < 12).all()
        assert (T.TRI_TABLE[case, n:] == -1).all()
        # every table edge is crossed in this case
        for e in T.TRI_TABLE[case, :n]:
            lo = T.EDGE_OFFSET[e]
            hi = lo.copy()
            hi[T.EDGE_AXIS[e]] += 1
            ca, cb = lo[0] + 2 * lo[1] + 4 * lo[2], hi[0] + 2 * hi[1] + 4 * hi[2]
            assert ((case >> ca) & 1) != ((case >> cb) & 1)


def test_closedness_random_binary_volumes():
    seen = np.zeros(256, np.int64)
    for shape in ((6, 6, 6), (5, 7, 4)):
        for fill in (0.2, 0.5, 0.8):
            for seed in range(6):
                rng = np.random.default_rng(1000 * seed + int(100 * fill) + shape[1])
                vol = np.zeros(tuple(s + 2 for s in shape), np.float32)
                vol[1:-1, 1:-1, 1:-1] = rng.uniform(size=shape) < fill
                verts, faces = M.marching_cubes_ref(vol, 0.5)
                assert len(faces) > 0
                _assert_closed(faces, len(verts))
                seen += M.case_histogram(vol, 0.5)
    assert (seen > 0).all(), f"configurations never seen: {np.flatnonzero(seen == 0)}"


def test_sphere():
    r = 8.0
    verts, faces = M.marching_cubes_ref(M.sphere_volume(24, r), 0.0)
    _assert_closed(faces, len(verts))
    assert _euler(verts, faces) == 2
    vol, area = _signed_volume_area(verts, faces)
    assert vol > 0  # normals point outwards
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.03, vol
    assert abs(area / (4.0 * np.pi * r ** 2) - 1) < 0.03, area


def test_torus():
    verts, faces = M.marching_cubes_ref(torus_volume(), 0.0)
    _assert_closed(faces, len(verts))
    assert _euler(verts, faces) == 0
    assert _signed_volume_area(verts, faces)[0] > 0


def test_non_cubic_dimensions():
    rng = np.random.default_rng(7)
    vol = rng.normal(size=(9, 12, 7)).astype(np.float32)
    sp = (0.5, 1.0, 2.0)
    verts, faces = M.marching_cubes_ref(vol, 0.1, sp)
    assert len(verts) > 0 and len(faces) > 0
    assert faces.dtype == np.int32 and verts.dtype == np.float32
    assert faces.min() >= 0 and faces.max() < len(verts)
    hi = (np.array(vol.shape) - 1) * np.array(sp)
    assert (verts >= 0).all() and (verts <= hi + 1e-6).all()
    # the vertex count is the number of crossed grid edges
    ins = vol > 0.1
    n_cross = (ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum()
    assert len(verts) == n_cross


def _ray(origin, direction):
    r = np.zeros(13, np.float32)
    r[0:3], r[3:6] = origin, direction
    return r


def test_splat_ref_boundaries_and_layout():
    bx, by, bz = np.linspace(0.0, 1.0, 3), np.linspace(0.0, 1.5, 4), np.linspace(-1.0, 1.0, 5)
    nx, ny, nz = 3, 4, 5
    # one ray per sample point: origin = the point, z = 0
    pts = np.array([
        [0.0, 0.0, -1.0],                      # exactly on b[0] of every axis: bucket 0
        [1.0, 1.5, 1.0],                       # exactly on b[n - 1]: bucket n - 1
        [np.nextafter(np.float32(1.0), np.float32(2.0)), 0.5, 0.0],   # just outside x: dropped
        [0.5, np.nextafter(np.float32(0.0), np.float32(-1.0)), 0.0],  # just below y: dropped
        [0.25, 0.75, 0.25],                    # x bucket 1, y bucket 2, z bucket 3
        [0.5, 0.5, 0.5],                       # on boundaries: x bucket 1, y bucket 1, z bucket 3
    ], np.float32)
    rays = np.stack([_ray(p, (0, 0, 1)) for p in pts])
    z = np.zeros((len(pts), 1), np.float32)
    w = np.arange(1, len(pts) + 1, dtype=np.float32).reshape(-1, 1) / 8
    depth = np.zeros(len(pts), np.float32)
    vol = M.splat_max_ref(rays, z, w, depth, None, bx, by, bz, depth_max=1.0)
    cell = lambda x, y, zz: x * nz + y * nx * nz + zz  # noqa: E731  (the reference's formula)
    want = np.zeros(nx * ny * nz, np.float32)
    want[cell(0, 0, 0)] = w[0, 0]
    # (2, 3, 4) -> 2 * 5 + 3 * 15 + 4 = 59 = the last cell
    want[cell(nx - 1, ny - 1, nz - 1)] = w[1, 0]
    want[cell(1, 2, 3)] = w[4, 0]
    want[cell(1, 1, 3)] = w[5, 0]
    assert cell(nx - 1, ny - 1, nz - 1) == nx * ny * nz - 1
    np.testing.assert_array_equal(vol, want)
    # the (nx, ny, nz) view after the reference's reshape + transpose
    v3 = vol.reshape(ny, nx, nz).transpose(1, 0, 2)
    assert v3[1, 2, 3] == w[4, 0] and v3[0, 0, 0] == w[0, 0] and v3[2, 3, 4] == w[1, 0]


def test_splat_ref_ray_tests_and_max():
    bx = by = bz = np.linspace(0.0, 1.0, 3)
    rays = np.stack([_ray((0.1, 0.1, 0.1), (0, 0, 1))] * 4)
    z = np.zeros((4, 2), np.float32)
    w = np.array([[0.2, 0.7], [0.9, 0.0], [0.95, 0.1], [0.3, 0.5]], np.float32)
    depth = np.array([0.1, 2.0, 0.1, 0.1], np.float32)       # ray 1 fails depth < depth_max
    var = np.array([0.1, 0.1, 5.0, 0.1], np.float32)        # ray 2 fails the variance test
    vol = M.splat_max_ref(rays, z, w, depth, var, bx, by, bz, depth_max=1.0, var_max=1.0)
    assert vol.max() == np.float32(0.7) and (vol > 0).sum() == 1
    vol = M.splat_max_ref(rays, z, w, depth, var, bx, by, bz, depth_max=1.0, var_max=0.0)
    assert vol.max() == np.float32(0.95)
    # accumulation across calls keeps the maximum
    vol2 = M.splat_max_ref(rays[:1], z[:1], w[:1], depth[:1], None, bx, by, bz, 1.0, volume=vol.copy())
    np.testing.assert_array_equal(vol2, vol)


def test_bucketize_ref_is_torch_bucketize():
    import torch
    rng = np.random.default_rng(3)
    b = np.linspace(-0.3, 0.41, 57)
    v = np.concatenate([rng.uniform(-0.3, 0.41, 500), b]).astype(np.float32)
    got = M.bucketize_ref(v, b)
    want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(b)).numpy()
    np.testing.assert_array_equal(got, want)


def test_lidar_directions():
    d = M.build_lidar_directions((-22.5, 22.5), 2.5, 10.0)
    assert d.shape == (3, 18 * 36)
    n = d.norm(dim=0)
    assert float((n - 1).abs().max()) < 1e-6
    # the first row is the lowest elevation, azimuth 0 first
    np.testing.assert_allclose(d[:, 0].numpy(), [np.cos(np.deg2rad(22.5)), 0, -np.sin(np.deg2rad(22.5))], atol=1e-6)
    np.testing.assert_allclose(d[:, 9].numpy(), [0, np.cos(np.deg2rad(22.5)), -np.sin(np.deg2rad(22.5))], atol=1e-6)


def test_write_ply_roundtrip(tmp_path):
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(11, 3)).astype(np.float32)
    faces = rng.integers(0, 11, size=(7, 3)).astype(np.int32)
    path = os.path.join(tmp_path, "m.ply")
    M.write_ply(path, verts, faces)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert "element vertex 11" in lines and "element face 7" in lines
    v = np.frombuffer(body, "<f4", count=33).reshape(11, 3)
    rec = np.frombuffer(body, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=7, offset=33 * 4)
    assert len(body) == 33 * 4 + 7 * 13
    np.testing.assert_array_equal(v, verts)
    assert (rec["n"] == 3).all()
    np.testing.assert_array_equal(rec["i"], faces)
