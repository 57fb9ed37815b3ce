"""Build a ground-truth LiDAR map (GPU box): synthetic quad scans get per-point timestamps over a moving trajectory and
a sprinkle of ghost returns; loner_amd.lidar_map.build_lidar_map deskews, filters and merges them and runs the
statistical outlier filter; a denser cloud is then masked by that map (mask_cloud).  Per-stage times by device events.

Then time the k-nearest-neighbour search (HIP events, the median of five runs after a warm-up) on the voxel-filtered
quad cloud at about 2^17 points, querying the cloud against itself:
  * lnr_knn_search, k = 20, at the default cell times each of KNN_CELL_FACTORS (grid build timed apart): the fastest
    total is what lidar_map.KNN_CELL_FACTOR should be;
  * the yardstick: tracking.cloud_normals(k = 20), the only other kNN of the library (exhaustive, plus an eigen-solve);
  * k = 1 against lnr_nn_search on the same grid (one wave per query against one thread per query).

    python tools/lidar_map_demo.py [--scans 16] [--voxel 0.05] [--json profiles/lidar_map_demo.json] [--pcd map.pcd]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 5
SCAN_PERIOD = 0.1


def timed(fn, runs=RUNS):
    """Median, minimum and maximum milliseconds of ``fn`` over ``runs`` runs after one warm-up (HIP events)."""
    fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def filtered_to(ME, points, target):
    """``points`` voxel-filtered at the voxel size (bisected) that leaves about ``target`` points."""
    lo, hi = 0.005, 2.0
    for _ in range(14):
        mid = (lo * hi) ** 0.5
        n = ME.voxel_down_sample(points, mid).shape[0]
        lo, hi = (mid, hi) if n > target else (lo, mid)
    voxel = (lo * hi) ** 0.5
    return ME.voxel_down_sample(points, voxel), voxel


def timed_scans(syn, n_scans, ghost_fraction, seed):
    """(scans, tum): quad scans measured by a sensor that keeps moving along the trajectory (one pose more than scans).
    The scene is cast from the pose at each scan's stamp; return j is then taken at its own time, spread over the
    SCAN_PERIOD after the stamp, so its sensor-frame point is the pose at that time inverted on the world point: only a
    deskew with the same trajectory puts the returns back on the surfaces.  ``ghost_fraction`` of the returns get a
    random range."""
    from scipy.spatial.transform import Rotation, Slerp
    rng = np.random.default_rng(seed)
    poses = syn.keyframe_poses("quad", n_scans + 1, None)
    t0 = 1.7e9
    tum = np.array([[t0 + SCAN_PERIOD * i, *T[:3, 3], *Rotation.from_matrix(T[:3, :3]).as_quat()]
                    for i, T in enumerate(poses)])
    slerp = Slerp(tum[:, 0], Rotation.from_quat(tum[:, 4:8]))
    scans = []
    for i, s in enumerate(syn.make_window("quad", n_scans, seed=1000, poses=poses[:n_scans])):
        n = s["distances"].shape[0]
        ts = np.linspace(0.0, SCAN_PERIOD * (1 - 1e-6), n)
        world = (s["directions"].double() * s["distances"].double()).t().numpy() @ poses[i][:3, :3].T + poses[i][:3, 3]
        at = tum[i, 0] + ts
        x = np.stack([np.interp(at, tum[:, 0], tum[:, 1 + a]) for a in range(3)], axis=1)
        p = slerp(at).inv().apply(world - x)
        r = np.linalg.norm(p, axis=1)
        d = p / r[:, None]
        ghosts = rng.permutation(n)[: int(ghost_fraction * n)]
        r[ghosts] = rng.uniform(1.0, 40.0, len(ghosts))
        scans.append(dict(directions=torch.from_numpy(d.T.copy()).float(), distances=torch.from_numpy(r).float(),
                          time=float(tum[i, 0]), timestamps=torch.from_numpy(ts)))
    return scans, tum


def knn_benchmark(ME, LM, TR, cloud, k=20):
    n = cloud.shape[0]
    box = torch.stack((cloud.min(dim=0).values, cloud.max(dim=0).values)).tolist()
    base = ME.default_cell(box[0], box[1], n) * k ** 0.5
    rec = {"points": int(n), "k": k, "cell_factor_1_m": round(base, 5), "grid": {}}
    first = None
    for f in LM.KNN_CELL_FACTORS:
        cell = f * base
        grid = ME.NearestGrid(cloud, cell)
        idx, d2, _ = LM.knn(cloud, grid, k)
        first = (idx, d2) if first is None else first
        rec["grid"][str(f)] = {"cell_m": round(cell, 5),
                               "same_result": bool(torch.equal(idx, first[0]) and torch.equal(d2, first[1])),
                               "build": timed(lambda: ME.NearestGrid(cloud, cell)),
                               "search": timed(lambda: LM.knn(cloud, grid, k, check=False))}
    total = {f: g["build"]["median_ms"] + g["search"]["median_ms"] for f, g in rec["grid"].items()}
    best = min(total, key=total.get)
    rec["fastest_factor"] = float(best)
    rec["grid_total_median_ms"] = round(total[best], 4)
    rec["module_factor"] = LM.KNN_CELL_FACTOR
    rec["module_factor_total_median_ms"] = round(total[str(LM.KNN_CELL_FACTOR)], 4)
    normals = torch.empty_like(cloud)
    rec["cloud_normals"] = timed(lambda: TR.cloud_normals(cloud, k, normals), runs=3)
    rec["normals_over_grid"] = round(rec["cloud_normals"]["median_ms"] / rec["module_factor_total_median_ms"], 2)
    # k = 1 against the single-nearest search, on the grid of map_eval's own default cell
    grid = ME.NearestGrid(cloud)
    one = timed(lambda: LM.knn(cloud, grid, 1, check=False))
    nn = timed(lambda: grid.query(cloud, check=False))
    i1, d1, m1 = LM.knn(cloud, grid, 1)
    dist, i2, d2 = grid.query(cloud)
    rec["k1"] = {"cell_m": round(grid.cell, 5), "knn": one, "nn_search": nn,
                 "knn_over_nn": round(one["median_ms"] / nn["median_ms"], 2),
                 "same_result": bool(torch.equal(i1[:, 0], i2) and torch.equal(d1[:, 0], d2) and torch.equal(m1, dist))}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--ghost-fraction", type=float, default=0.002)
    ap.add_argument("--dist-threshold", type=float, default=0.1)
    ap.add_argument("--pcd", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "lidar_map_demo.json"))
    ap.add_argument("--no-knn-benchmark", action="store_true")
    args = ap.parse_args()
    from loner_amd import lidar_map as LM
    from loner_amd import map_eval as ME
    from loner_amd import meshing as M
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    dev = torch.device("cuda", 0)
    scans, tum = timed_scans(syn, args.scans, args.ghost_fraction, seed=7)
    rec = {"scans": len(scans), "returns": int(sum(s["distances"].shape[0] for s in scans)), "voxel_m": args.voxel,
           "min_range_m": args.min_range, "ghost_fraction": args.ghost_fraction}
    LM.build_lidar_map(scans[:2], tum, args.voxel, args.min_range, outlier_filter=True, device=dev)  # warm-up
    timer = M.StageTimer()
    cloud = LM.build_lidar_map(scans, tum, args.voxel, args.min_range, outlier_filter=True, device=dev, timer=timer)
    unfiltered = LM.build_lidar_map(scans, tum, args.voxel, args.min_range, device=dev)
    # the denser cloud: twice the scans of the same scene, cast from standing poses, no ghosts
    dense = ME.scan_world_points(syn.make_window("quad", 2 * args.scans, seed=1000)).to(dev)
    LM.mask_cloud(dense[:1000].contiguous(), cloud, args.dist_threshold)  # warm-up
    with timer("mask_cloud"):
        kept, mask = LM.mask_cloud(dense, cloud, args.dist_threshold)
    rec.update(map_points=int(cloud.shape[0]), map_points_before_outlier_filter=int(unfiltered.shape[0]),
               dense_points=int(dense.shape[0]), dense_points_kept=int(kept.shape[0]))
    rec["stage_ms"] = {k: round(v, 4) for k, v in timer.times_ms().items()}
    print("stage_ms", rec["stage_ms"])
    if args.pcd:
        ME.write_pcd(args.pcd, cloud)
    if not args.no_knn_benchmark:
        big, voxel = filtered_to(ME, ME.scan_world_points(syn.make_window("quad", 32, seed=1000)).to(dev), 1 << 17)
        rec["knn"] = dict(voxel_m=round(voxel, 5), **knn_benchmark(ME, LM, TR, big))
        print("knn", json.dumps(rec["knn"]))
    print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
