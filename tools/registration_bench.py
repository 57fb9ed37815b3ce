"""Registration, exhaustive against grid search (GPU box): cloud normals (k = 30) and the default two-stage ICP schedule
between two synthetic quad scans a small motion apart, at about 5 000, 2^15 and a full scan's points; the grid path's
cell factor swept over tracking.ICP_CELL_FACTORS; then the grid path alone on what the exhaustive one cannot take: a
tracker step on full scans and the alignment of two clouds of 1.9e5 points.  HIP events, medians of five runs after
a warm-up, the two paths alternating; the grid times include the grid builds (a fresh GridTarget per run).

    python tools/registration_bench.py [--json profiles/registration_grid.json]
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


def rel_pose():
    y, p = np.deg2rad(2.0), np.deg2rad(0.5)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = (0.4, 0.04, 0.02)
    return T


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, runs=RUNS):
    """Median milliseconds of each of ``fns`` (name -> callable): one warm-up each, then ``runs`` rounds in which
    every one runs once, in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            times[k].append(once(fn))
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "registration_grid.json"))
    ap.add_argument("--no-brute-above", type=int, default=1 << 18, help="skip the exhaustive path above this size")
    args = ap.parse_args()
    from loner_amd import map_eval as ME
    from loner_amd import synthetic as syn
    from loner_amd import tracking as TR
    dev = torch.device("cuda", 0)
    base = syn.keyframe_poses("quad", 1, None)[0]
    win = syn.make_window("quad", 2, seed=3, poses=[base, base @ rel_pose()])
    sched = TR.TrackerSettings().schedule
    default_factor = TR.ICP_CELL_FACTOR
    rec = dict(device=torch.cuda.get_device_name(0), runs=RUNS, knn=30, default_cell_factor=default_factor,
               schedule=[[s.threshold, s.max_iterations] for s in sched], sizes=[])
    brute_solver, grid_solver = TR.IcpSolver(dev), TR.IcpSolver(dev)
    for target in (5000, 1 << 15, None):
        tgt, src = (TR.frame_point_cloud(w["directions"], w["distances"], target_points=target).to(dev) for w in win)
        n = int(tgt.shape[0])
        with_brute = n <= args.no_brute_above
        out_b, out_g = torch.empty_like(tgt), torch.empty_like(tgt)
        fns = {"normals_grid_ms": lambda: TR.cloud_normals_grid(tgt, 30, out=out_g)}
        if with_brute:
            fns["normals_brute_ms"] = lambda: TR.cloud_normals(tgt, 30, out=out_b)
        row = dict(n_src=int(src.shape[0]), n_tgt=n, **alternate(fns))
        if with_brute:
            row["normals_bitwise_equal"] = bool(torch.equal(out_b, out_g))
        nrm = out_g

        def grid_run(factor):
            def run():  # IcpSolver.run with the stages' cells from ``factor``: a fresh target, its box, its grids
                target = TR.GridTarget(tgt, nrm)
                grid_solver.init()
                for st in sched:
                    grid_solver.stage(src, target, None, st, search="grid", cell=target.cell_for(st.threshold, factor))
            return run

        fns = {f"schedule_grid_c{c:g}_ms": grid_run(c) for c in TR.ICP_CELL_FACTORS}
        if with_brute:
            fns["schedule_brute_ms"] = lambda: brute_solver.run(src, tgt, nrm, sched)
        row.update(alternate(fns))
        row["schedule_grid_ms"] = row[f"schedule_grid_c{default_factor:g}_ms"]
        grid_solver.run(src, TR.GridTarget(tgt, nrm), None, sched, search="grid")
        res = grid_solver.read()
        row["iterations"] = [r["iterations"] for r in res]
        box = TR.GridTarget(tgt, nrm).box
        row["cells_m"] = {f"{c:g}": [round(TR.icp_grid_cell(s.threshold, box[0], box[1], n, c), 5) for s in sched]
                          for c in TR.ICP_CELL_FACTORS}
        if with_brute:
            brute_solver.run(src, tgt, nrm, sched)
            row["schedule_bitwise_equal"] = bool(torch.equal(brute_solver.snap[:2], grid_solver.snap[:2]))
        rec["sizes"].append(row)
        print(json.dumps(row), flush=True)

    # the grid path alone: one tracker step on full scans (cloud, normals, schedule, the read of the result)
    scans = [dict(directions=w["directions"].to(dev), distances=w["distances"].to(dev)) for w in win]
    settings = TR.TrackerSettings(downsample_type=None, search="grid")

    def track_pair():
        tr = TR.Tracker(settings, dev)
        for s in scans:
            out = tr.track(dict(s))
        return out

    def first_only():
        TR.Tracker(settings, dev).track(dict(scans[0]))

    t = alternate({"track_two_scans_ms": track_pair, "track_first_scan_ms": first_only})
    out = track_pair()
    rec["tracker_full_scans"] = dict(n_points=out["n_points"], iterations=out["iterations"], fitness=out["fitness"],
                                     rmse=out["rmse"], **t,
                                     second_scan_ms=round(t["track_two_scans_ms"] - t["track_first_scan_ms"], 4))
    print(json.dumps(rec["tracker_full_scans"]), flush=True)

    # and the alignment above the exhaustive cap: four full scans against themselves moved, voxel 0.05 m
    est = ME.scan_world_points(syn.make_window("quad", 4))
    a = np.deg2rad(0.3)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (0.02 / np.sqrt(3),) * 3
    gt = torch.from_numpy(ME.transform_points_ref(est.numpy(), T)).to(dev)
    e, g = ME.voxel_down_sample(est.to(dev), 0.05), ME.voxel_down_sample(gt, 0.05)
    t = alternate({"align_grid_ms": lambda: ME.align_clouds(e, g, ME.ALIGN_MAX_POINTS_GRID, "grid"),
                   "normals_grid_ms": lambda: TR.cloud_normals_grid(g, ME.ALIGN_KNN)})
    Tg, st = ME.align_clouds(e, g, ME.ALIGN_MAX_POINTS_GRID, "grid")
    rec["alignment"] = dict(n_est=int(e.shape[0]), n_gt=int(g.shape[0]), iterations=st["iterations"],
                            fitness=st["fitness"], rmse=st["rmse"],
                            transform_error_vs_generating_motion=float(np.abs(Tg - T).max()), **t)
    print(json.dumps(rec["alignment"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
