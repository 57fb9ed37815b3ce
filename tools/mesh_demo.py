"""Mesh a trained map (GPU box): optimise the sigma field on a synthetic quad window as
tests/test_gpu_eval.py::test_training_learns_the_map does, extract the mesh with loner_amd.meshing.Mesher, write a
PLY and report event-timed stage times next to a bytes-moved estimate per stage, and the share of mesh vertices
within one ``resolution`` of the synthetic scene's true surfaces (information, not a gate).

    python tools/mesh_demo.py [--steps 300] [--skip-step 4] [--resolution 0.2] [--level-set 0]
                                 [--ply mesh.ply] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUAD_BOUND = [[-5, 50], [-25, 15], [-3, 10]]  # the quad bounding box (cfg/newer_college/quad.yaml:8-14)


def surface_distance(scene, pts):
    """Distance (metres) from points (N, 3) to the nearest surface of a synthetic.Scene (ground plane and boxes)."""
    d = np.abs(pts[:, 2] - scene.ground_z)
    for b in scene.boxes:
        lo, hi = b[0], b[1]
        out = np.maximum(np.maximum(lo - pts, pts - hi), 0.0)          # > 0 outside, per axis
        d_out = np.linalg.norm(out, axis=1)
        d_in = np.min(np.minimum(pts - lo, hi - pts), axis=1)          # > 0 inside: distance to the nearest face
        d = np.minimum(d, np.where(d_out > 0, d_out, np.maximum(d_in, 0.0)))
    return d


def traffic_model(n_samples_total, n_levels, n_voxels, n_verts, n_faces):
    """Bytes each stage must move (compulsory traffic, caches assumed to hold the re-read neighbours):
      render   per ray sample: z written and read twice (4 + 8), the level-major encoding written and read
               (2 x 4 n_levels), sigma staged in the weights buffer then overwritten by the weights (4 + 4 + 4);
               the hash-table gathers are served from cache and not counted
      splat    per ray sample: z and weight read (8); the atomics touch only cells a sample can raise
      count    per voxel: the value read once (4), two int32 counts written (8)
      scan     per voxel and count array: int32 read, int64 scan written, both read and the int64 offset written (36)
      emit     per voxel: the value and two int64 offsets read (20); per vertex 12 written, per face 12 written"""
    return {
        "render": n_samples_total * (12 + 8 * n_levels + 12),
        "splat": n_samples_total * 8,
        "count": n_voxels * 12,
        "scan": n_voxels * 2 * 36,
        "emit": n_voxels * 20 + n_verts * 12 + n_faces * 12,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--skip-step", type=int, default=4)
    ap.add_argument("--resolution", type=float, default=0.2)
    ap.add_argument("--level-set", type=float, default=0.0, help="iso level of the weight volume (reference: 0)")
    ap.add_argument("--ply", default="mesh_demo.ply")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import bench
    from loner_amd import evaluate as E
    from loner_amd import meshing as M
    from loner_amd import step as S_
    from loner_amd import synthetic as syn
    from loner_amd.rays import RayWindow
    dev = torch.device("cuda", 0)
    wc, rr = syn.world_cube("quad"), syn.SENSORS["quad"]["ray_range"]
    scans = syn.make_window("quad", 16, seed=1000)
    window = RayWindow(scans, wc, rr, n_lidar=512, device=dev)
    held = syn.make_window("quad", 1, seed=77, start=3)[0]
    sub = torch.arange(0, held["distances"].shape[0], 29)
    held = dict(directions=held["directions"][:, sub].contiguous(), distances=held["distances"][sub].contiguous(),
                pose=held["pose"])
    st = S_.FieldState(S_.StepConfig(loss=S_.LossConfig.from_dict(bench.LOSS_PRESETS["default"])), device=dev)
    eng = S_.StepEngine(st, window.n_slots, seed=5)
    rend = E.DepthRenderer(st, n_samples=512, chunk=4096)
    rec = {"steps": args.steps, "l1_before_m": float(E.compute_l1_depth(rend, held, held["pose"], wc, rr, key=1))}
    for it in range(args.steps):
        if it % 32 == 0:
            st.reset_optimizer()
        eng.step_window(window, global_step=it, iteration_idx=it % 32)
    rec["l1_after_m"] = float(E.compute_l1_depth(rend, held, held["pose"], wc, rr, key=1))
    del rend, eng

    def mesh(timer):
        m = M.Mesher(st, [s["pose"] for s in scans], wc, rr, resolution=args.resolution,
                     marching_cubes_bound=QUAD_BOUND, level_set=args.level_set,
                     lidar_vertical_fov=syn.SENSORS["quad"]["fov"], timer=timer)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces = m.get_mesh(skip_step=args.skip_step, key=0)
        torch.cuda.synchronize()
        return m, verts, faces, time.perf_counter() - t0

    mesh(None)  # warm-up: code objects, allocator
    timer = M.StageTimer()
    m, verts, faces, wall = mesh(timer)
    times = timer.times_ms()
    n_vox = int(m.results.numel())
    n_samples_total = m.n_rays * m.S
    model = traffic_model(n_samples_total, st.cfg.n_levels, n_vox, len(verts), len(faces))
    rec.update(level_set=args.level_set, resolution=args.resolution, grid=[len(b) for b in m.xyz], voxels=n_vox,
               poses=len(m.poses[::args.skip_step]), rays=m.n_rays,
               n_samples=m.S, ray_samples=n_samples_total, vertices=len(verts), faces=len(faces),
               nonzero_cells=float((m.results > 0).float().mean()), wall_s=wall,
               stage_ms={k: round(v, 4) for k, v in times.items()},
               stage_bytes=model,
               stage_gb_per_s={k: round(model[k] / (times[k] * 1e-3) / 1e9, 1) for k in model if times.get(k)})
    scene = syn.make_scene("quad", np.random.default_rng(1234))
    v = verts.cpu().numpy().astype(np.float64)
    if len(v):
        d = surface_distance(scene, v)
        rec["share_within_resolution"] = float((d <= args.resolution).mean())
        rec["share_within_3_resolutions"] = float((d <= 3 * args.resolution).mean())
        rec["median_surface_distance_m"] = float(np.median(d))
    M.write_ply(args.ply, verts, faces)
    rec["ply"] = os.path.basename(args.ply)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
