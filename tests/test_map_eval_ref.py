"""The numpy / scipy restatements of loner_amd.map_eval on hand-computed cases (CPU only): they are the oracle of
tests/test_gpu_map_eval.py, so they are checked on their own here."""
import numpy as np
import pytest
import torch

from loner_amd import map_eval as ME
from loner_amd import synthetic as syn


def lattice(n=20, dz=0.0):
    g = np.arange(n, dtype=np.float64) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, dz)], axis=1).astype(np.float32)


def test_voxel_hand_case():
    p = np.zeros((5, 3), np.float32)
    p[:, 0] = [0.0, 0.4, 0.5, 1.4, 1.5]
    idx = ME.cell_indices_ref(p, p.min(axis=0).astype(np.float64) - 0.5, 1.0)
    np.testing.assert_array_equal(idx[:, 0], [0, 0, 1, 1, 2])  # origin -0.5
    means, counts, keys = ME.voxel_down_sample_ref(p, 1.0, return_counts=True, return_keys=True)
    np.testing.assert_allclose(means[:, 0], [0.2, 0.95, 1.5], rtol=2e-7)
    np.testing.assert_array_equal(means[:, 1:], 0.0)
    np.testing.assert_array_equal(counts, [2, 2, 1])
    np.testing.assert_array_equal(keys, np.array([0, 1, 2], np.int64) << 42)
    # the order of the input does not matter, the order of the output is the keys'
    m2 = ME.voxel_down_sample_ref(p[[4, 2, 0, 3, 1]], 1.0)
    np.testing.assert_allclose(m2, means, rtol=2e-7)


def test_voxel_order_and_limits():
    p = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    means, keys = ME.voxel_down_sample_ref(p, 0.5, return_keys=True)
    np.testing.assert_array_equal(means, p[[3, 0, 1, 2]])  # ascending x, then y, then z
    assert (np.diff(keys) > 0).all()
    with pytest.raises(RuntimeError, match="2\\^21"):
        ME.voxel_down_sample_ref(np.array([[0, 0, 0], [1e6, 0, 0]], np.float32), 0.05)
    with pytest.raises(RuntimeError, match="nan or inf"):
        ME.voxel_down_sample_ref(np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32), 0.05)


def test_lattice_statistics():
    a, b = lattice(), lattice(dz=0.07)
    s = ME.compare_point_clouds_ref(a, b, f_score_threshold=0.1, voxel_size=0.05, align=False)
    assert s["num_points"] == 400
    assert s["accuracy"] == pytest.approx(0.07, rel=1e-6) and s["completion"] == pytest.approx(0.07, rel=1e-6)
    assert s["chamfer_distance"] == pytest.approx(0.14, rel=1e-6)
    assert s["precision"] == 1.0 and s["recall"] == 1.0
    assert s["f-score"] == pytest.approx(1.0, abs=1e-8)
    s = ME.compare_point_clouds_ref(a, b, f_score_threshold=0.05, voxel_size=0.05, align=False)
    assert s["precision"] == 0.0 and s["recall"] == 0.0 and s["f-score"] == 0.0
    assert s["accuracy"] == pytest.approx(0.07, rel=1e-6)


def test_statistics_formulas():
    # 10 estimated points, 3 of them far; 8 true points, 2 of them far: TP = 7 (from accuracy), FP = 3, FN = 2
    s = ME.statistics(1.0, 10, 3, 2.0, 8, 2)
    assert s["accuracy"] == pytest.approx(0.1) and s["completion"] == pytest.approx(0.25)
    assert s["chamfer_distance"] == pytest.approx(0.35)
    assert s["precision"] == pytest.approx(0.7) and s["recall"] == pytest.approx(7 / 9)
    assert s["f-score"] == pytest.approx(2 * 0.7 * (7 / 9) / (0.7 + 7 / 9 + 1e-8))
    assert ME.alignment_skip(10, 4) == 2 and ME.alignment_skip(4, 4) == 1 and ME.alignment_skip(3, 4) == 1
    with pytest.raises(ValueError, match="2\\^17"):
        ME.compare_point_clouds_ref(lattice(), lattice(), align_max_points=(1 << 17) + 1)


@pytest.mark.parametrize("kind", ["quad", "canteen"])
def test_fp32_key_picks_the_kdtree_neighbour(kind):
    pts = ME.scan_world_points(syn.make_window(kind, 4), stride=2).numpy()  # both spread over all four scans
    src, tgt = pts[1::(len(pts) - 1) // 4000][:4000], pts[0::len(pts) // 6000][:6000]
    assert len(src) == 4000 and len(tgt) == 6000
    dist, idx = ME.nearest_distances_ref(src, tgt)
    d32, i32, key = ME.nearest_distances_ref(src, tgt, fp32_key=True)
    assert int((i32 != idx).sum()) == 0
    np.testing.assert_array_equal(d32, dist)
    # the key is the squared distance up to fp32 rounding (5 roundings of 2^-24)
    np.testing.assert_allclose(key.astype(np.float64), dist ** 2, rtol=4e-7, atol=1e-30)


def test_fp32_key_ties_go_to_the_lower_index():
    tgt = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [1, 0, 0]], np.float32)
    idx, d2 = ME.nn_key_ref(np.zeros((1, 3), np.float32), tgt)
    assert idx[0] == 0 and d2[0] == 1.0


def test_transform_points_ref():
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    np.testing.assert_array_equal(ME.transform_points_ref(np.array([[1, 0, 0], [0, 2, 5]], np.float32), T),
                                  [[1, 3, 3], [-1, 2, 8]])


def test_pcd_round_trip(tmp_path):
    p = np.random.default_rng(3).normal(size=(1001, 3)).astype(np.float32) * 30
    ME.write_pcd(tmp_path / "a.pcd", torch.from_numpy(p))
    raw = (tmp_path / "a.pcd").read_bytes()
    assert raw.startswith(b"# .PCD v0.7") and b"\nDATA binary\n" in raw and len(raw) > 12 * 1001
    np.testing.assert_array_equal(ME.read_pcd(tmp_path / "a.pcd"), p)
    # an ascii file with a further field before x y z
    with open(tmp_path / "b.pcd", "w") as f:
        f.write("VERSION 0.7\nFIELDS intensity x y z\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH 2\nHEIGHT 1\n"
                "POINTS 2\nDATA ascii\n9 1 2 3\n8 4 5.5 6\n")
    np.testing.assert_array_equal(ME.read_pcd(tmp_path / "b.pcd"), [[1, 2, 3], [4, 5.5, 6]])


def test_write_statistics(tmp_path):
    s = ME.compare_point_clouds_ref(lattice(), lattice(dz=0.07), align=False)
    path = ME.write_statistics(s, tmp_path, id_str="t1")
    assert path.endswith("metrics/statistics_t1.yaml")
    got = dict(line.split(": ") for line in open(path).read().splitlines())
    assert set(got) == set(s) and int(got["num_points"]) == 400 and float(got["accuracy"]) == s["accuracy"]
    assert ME.write_statistics(s, tmp_path).endswith("metrics/statistics.yaml")
