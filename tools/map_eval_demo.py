"""Evaluate a trained map (GPU box): optimise the sigma field on a synthetic quad window as tools/mesh_demo.py does,
render the map as a point cloud (loner_amd.map_eval.LidarMapRenderer), take the synthetic scans' own world points as
the ground-truth cloud, and print the reference's seven statistics (compare_point_clouds) with event-timed stage times.

Then time the nearest-neighbour search on voxel-filtered synthetic surface clouds of about 2^15 and 2^17 points a side,
both directions, HIP events, the median of five runs after a warm-up:
  * the grid search (lnr_nn_search; the grid build and the sort timed apart) at cell = 1, 2, 4, 8 x voxel;
  * the yardstick: the brute-force tile scan of lnr_icp_stage (identity T, max_iterations = 0, a threshold above the
    cloud's extent, corr_idx / corr_d2 requested), whose indices the grid search must reproduce.

    python tools/map_eval_demo.py [--steps 300] [--skip-step 5] [--resolution 0.25] [--voxel 0.1]
                                  [--json profiles/map_eval_demo.json] [--pcd map.pcd]
                                  [--align-search grid --align-max-points 1000000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL_FACTORS = (1, 2, 4, 8)
RUNS = 5


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


class BruteForce:
    """Nearest neighbours by the ICP correspondence kernel; state, workspace and outputs allocated once."""

    def __init__(self, TR, src, tgt, extent):
        self.TR, self.src, self.tgt = TR, src, tgt
        self.normals = torch.zeros_like(tgt)  # read by the kernel's sums, which nobody looks at
        self.solver = TR.IcpSolver(src.device)
        self.stage = TR.IcpStage(2.0 * extent + 1.0, 0)
        self.idx = torch.empty(src.shape[0], dtype=torch.int32, device=src.device)
        self.d2 = torch.empty(src.shape[0], dtype=torch.float32, device=src.device)

    def __call__(self):
        self.solver.init()
        self.solver.stage(self.src, self.tgt, self.normals, self.stage, self.idx, self.d2)
        self.solver.n_stages = 0
        return self.idx, self.d2


def search_benchmark(ME, TR, a, b, voxel):
    """Both directions between the filtered clouds a and b: grid search per cell factor, and the brute force."""
    extent = float(torch.cat((a, b)).abs().max()) * 2
    rec = {"n_a": int(a.shape[0]), "n_b": int(b.shape[0]), "voxel_m": round(voxel, 5), "grid": {}}
    ab, ba = BruteForce(TR, a, b, extent), BruteForce(TR, b, a, extent)
    rec["brute_force"] = timed(lambda: (ab(), ba()))
    (bi_ab, bd_ab), (bi_ba, _) = ab(), ba()
    for f in CELL_FACTORS:
        cell = f * voxel
        ga, gb = ME.NearestGrid(a, cell), ME.NearestGrid(b, cell)
        _, i_ab, d_ab = gb.query(a)
        _, i_ba, _ = ga.query(b)
        rec["grid"][str(f)] = {
            "cell_m": round(cell, 5),
            "matches_brute_force": bool(torch.equal(i_ab, bi_ab) and torch.equal(i_ba, bi_ba) and
                                        torch.equal(d_ab, bd_ab)),
            "build": timed(lambda: (ME.NearestGrid(a, cell), ME.NearestGrid(b, cell))),
            "search": timed(lambda: (gb.query(a, check=False), ga.query(b, check=False))),
        }
    best = min(rec["grid"], key=lambda k: rec["grid"][k]["search"]["median_ms"] + rec["grid"][k]["build"]["median_ms"])
    g = rec["grid"][best]
    rec["fastest_factor"] = int(best)
    rec["grid_total_median_ms"] = round(g["search"]["median_ms"] + g["build"]["median_ms"], 4)
    rec["brute_over_grid"] = round(rec["brute_force"]["median_ms"] / rec["grid_total_median_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--skip-step", type=int, default=5)
    ap.add_argument("--resolution", type=float, default=0.25, help="sweep resolution in degrees (reference: 0.1)")
    ap.add_argument("--n-samples", type=int, default=512)
    ap.add_argument("--voxel", type=float, default=0.1, help="voxel size of the rendered cloud and of the comparison")
    ap.add_argument("--var-threshold", type=float, default=1e-2)
    ap.add_argument("--f-score-threshold", type=float, default=0.1)
    ap.add_argument("--pcd", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "map_eval_demo.json"))
    ap.add_argument("--no-search-benchmark", action="store_true")
    ap.add_argument("--align-search", default="brute", choices=("brute", "grid"),
                    help="the alignment's search; grid lifts the cap on the alignment clouds to 10^6 points")
    ap.add_argument("--align-max-points", type=int, default=1 << 16)
    args = ap.parse_args()
    import bench
    from loner_amd import map_eval as ME
    from loner_amd import meshing as M
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    from loner_amd.rays import RayWindow
    dev = torch.device("cuda", 0)
    wc, rr = syn.world_cube("quad"), syn.SENSORS["quad"]["ray_range"]
    scans = syn.make_window("quad", 16, seed=1000)
    window = RayWindow(scans, wc, rr, n_lidar=512, device=dev)
    st = S_.FieldState(S_.StepConfig(loss=S_.LossConfig.from_dict(bench.LOSS_PRESETS["default"])), device=dev)
    eng = S_.StepEngine(st, window.n_slots, seed=5)
    for it in range(args.steps):
        if it % 32 == 0:
            st.reset_optimizer()
        eng.step_window(window, global_step=it, iteration_idx=it % 32)
    del eng
    rec = {"steps": args.steps, "sweep_resolution_deg": args.resolution, "n_samples": args.n_samples,
           "voxel_m": args.voxel, "var_threshold": args.var_threshold}

    renderer = ME.LidarMapRenderer(st, wc, rr, syn.SENSORS["quad"]["fov"], args.resolution, args.resolution,
                                   n_samples=args.n_samples, var_threshold=args.var_threshold)
    poses = [s["pose"] for s in scans]
    renderer.render(poses[:1], args.voxel, 1, key=0)  # warm-up: code objects, allocator
    timer = M.StageTimer()
    with timer("render_map"):
        est = renderer.render(poses, args.voxel, args.skip_step, key=0)
    gt = ME.scan_world_points(scans).to(dev)
    rec.update(poses=len(poses[::args.skip_step]), rays_per_sweep=int(renderer.directions.shape[1]),
               rendered_points=int(est.shape[0]), ground_truth_points=int(gt.shape[0]))
    if args.pcd:
        ME.write_pcd(args.pcd, est)
    align = dict(align_search=args.align_search, align_max_points=args.align_max_points)
    rec.update(align)
    ME.compare_point_clouds(est, gt, args.f_score_threshold, args.voxel, **align)  # warm-up
    stats = ME.compare_point_clouds(est, gt, args.f_score_threshold, args.voxel, timer=timer, **align)
    rec["statistics"] = stats
    rec["stage_ms"] = {k: round(v, 4) for k, v in timer.times_ms().items()}
    rec["voxel_filter_gt"] = dict(points=int(gt.shape[0]), voxel_m=args.voxel,
                                  **timed(lambda: ME.voxel_down_sample(gt, args.voxel)))
    for k in ("accuracy", "completion", "chamfer_distance", "recall", "precision", "f-score", "num_points"):
        print(f"{k:18s} {stats[k]}")
    print("stage_ms", rec["stage_ms"])

    if not args.no_search_benchmark:
        # surface clouds of two disjoint halves of a denser window, filtered to the two sizes
        dense = syn.make_window("quad", 32, seed=1000)
        a_all = ME.scan_world_points(dense[0::2]).to(dev)
        b_all = ME.scan_world_points(dense[1::2]).to(dev)
        rec["search"] = {}
        for name, target in (("2^15", 1 << 15), ("2^17", 1 << 17)):
            a, va = filtered_to(ME, a_all, target)
            b = ME.voxel_down_sample(b_all, va)
            r = search_benchmark(ME, TR, a, b, va)
            rec["search"][name] = r
            print(name, json.dumps(r))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
