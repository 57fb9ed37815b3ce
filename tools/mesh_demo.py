"""Mesh a trained map (GPU box): optimise the sigma field on a synthetic quad window as
tests/test_gpu_eval.py::test_training_learns_the_map does, extract the mesh with loner_amd.meshing.Mesher, write a
PLY and report event-timed stage times next to a bytes-moved estimate per stage, and the share of mesh vertices
within one ``resolution`` of the synthetic scene's true surfaces (information, not a gate).  The PLY carries vertex
normals (loner_amd.mesh_cloud.vertex_normals).

With --eval the mesh is then scored as the reference's mesh_to_pcd.py + evaluate_lidar_map.py score one: sampled into
--eval-points points (loner_amd.mesh_cloud), voxel-filtered at --voxel and compared with the synthetic scans' own world
points as tools/map_eval_demo.py compares its rendered cloud; the seven statistics are printed, not gated.  Each stage
is timed with HIP events, the median of five runs after a warm-up; the sampling kernel alternates with its yardstick,
the same computation composed from torch ops (``torch_sample_points``), whose points must equal the kernel's bit for
bit.  The record goes to --eval-json.

    python tools/mesh_demo.py [--steps 300] [--skip-step 4] [--resolution 0.2] [--level-set 0]
                                 [--ply mesh.ply] [--json out.json]
                                 [--eval] [--eval-points 50000000] [--voxel 0.1]
                                 [--eval-json profiles/mesh_cloud_demo.json]
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


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def timed(*fns, runs=5):
    """Median, minimum and maximum milliseconds of each of ``fns`` over ``runs`` rounds after one warm-up round; the
    functions alternate within a round."""
    for fn in fns:
        fn()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ms[k].append(event_ms(fn)[0])
    out = [{"median_ms": round(float(np.median(m)), 4), "min_ms": round(min(m), 4), "max_ms": round(max(m), 4)}
           for m in ms]
    return out[0] if len(out) == 1 else out


def torch_uniform(key, stream, a, b):
    """rand_uniform of csrc/common.hpp on int64 tensors holding uint32 values, widened to float64."""
    m = 0xFFFFFFFF

    def mix(x):
        x = x ^ (x >> 16)
        x = (x * 0x7FEB352D) & m
        x = x ^ (x >> 15)
        x = (x * 0x846CA68B) & m  # wraps in int64; the low 32 bits are the product's
        return x ^ (x >> 16)

    h = mix(torch.full_like(a, (key & m) ^ ((stream * 0x9E3779B9) & m)))
    h = mix(h ^ a)
    h = mix(h ^ ((b * 0x85EBCA6B + 0x632BE5AB) & m))
    return (h >> 8).double() * 2.0 ** -24


def torch_sample_points(verts, faces, bounds, n, key):
    """lnr_mesh_sample_points composed from torch ops: the search, the gathers and the float64 arithmetic in the
    kernel's order."""
    i = torch.arange(n, dtype=torch.int64, device=verts.device)
    t = torch.searchsorted(bounds, i, right=True)
    f = faces[t].long()
    v = verts.double()
    r1 = torch_uniform(key, 7, i, torch.zeros_like(i))
    r2 = torch_uniform(key, 7, i, torch.ones_like(i))
    s = torch.sqrt(r1)
    a, b, c = (1.0 - s)[:, None], (s * (1.0 - r2))[:, None], (s * r2)[:, None]
    return ((a * v[f[:, 0]] + b * v[f[:, 1]]) + c * v[f[:, 2]]).float()


def evaluate(args, verts, faces, normals, scans, dev):
    """--eval: the mesh's statistics and the stage times of mesh_cloud at args.eval_points points."""
    from loner_amd import _lib as L
    from loner_amd import map_eval as ME
    from loner_amd import mesh_cloud as MC
    from loner_amd import meshing as M
    n, key = args.eval_points, 0
    rec = {"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "points": n, "voxel_m": args.voxel}
    valence = torch.bincount(faces.reshape(-1).long(), minlength=verts.shape[0])
    rec["valence"] = {"min": int(valence.min()), "max": int(valence.max())}
    gt = ME.scan_world_points(scans).to(dev)
    timer = M.StageTimer()
    stats = MC.evaluate_mesh(verts, faces, gt, args.f_score_threshold, args.voxel, n, key=key, timer=timer)
    rec["statistics"] = stats
    rec["compare_stage_ms"] = {k: round(v, 4) for k, v in timer.times_ms().items()}
    for k in ("accuracy", "completion", "chamfer_distance", "recall", "precision", "f-score", "num_points"):
        print(f"{k:18s} {stats[k]}")

    status = torch.zeros(1, dtype=torch.int32, device=dev)
    area = MC.face_areas(verts, faces)
    bounds = MC.sample_bounds(area, n)
    points = MC.sample_points_uniformly(verts, faces, n, key)
    yard = torch_sample_points(verts, faces, bounds, n, key)
    rec["torch_composition_equals_kernel"] = bool(torch.equal(points.view(torch.int32), yard.view(torch.int32)))
    del yard
    perm, rows = MC.vertex_rows(faces, verts.shape[0])
    stage = {}
    stage["areas"] = timed(lambda: MC._face_areas(verts, faces, status))
    stage["scan_bounds"] = timed(lambda: MC.sample_bounds(area, n))
    stage["sample_kernel"], stage["sample_torch_ops"] = timed(
        lambda: MC._sample(verts, faces, bounds, 0, n, key, status, False),
        lambda: torch_sample_points(verts, faces, bounds, n, key))
    stage["voxel_filter"] = timed(lambda: ME.voxel_down_sample(points, args.voxel))
    stage["mesh_to_cloud"] = timed(lambda: MC.mesh_to_cloud(verts, faces, args.voxel, n, key))
    flat = faces.reshape(-1).long()
    skeys = torch.sort(flat, stable=True)[0]
    ids = torch.arange(verts.shape[0] + 1, dtype=torch.int64, device=dev)
    stage["normals_sort"] = timed(lambda: torch.sort(flat, stable=True))
    stage["normals_row_start"] = timed(lambda: torch.searchsorted(skeys, ids))
    stage["normals_bincount"] = timed(lambda: torch.bincount(flat, minlength=verts.shape[0]))
    out = torch.empty_like(verts)
    stage["normals_kernel"] = timed(lambda: L.call("lnr_mesh_vertex_normals", verts, verts.shape[0], faces,
                                                   faces.shape[0], perm, rows, out, status, L.stream(dev)))
    stage["vertex_normals"] = timed(lambda: MC.vertex_normals(verts, faces))
    assert int(status.item()) == 0 and torch.equal(out, normals)
    rec["stage"] = stage
    rec["cloud_points"] = int(MC.mesh_to_cloud(verts, faces, args.voxel, n, key).shape[0])
    # what the sampler must move: 12 B written per point (the mesh and the bounds are read once and stay in cache)
    written = 12 * n
    rec["sample_bytes_written"] = written
    rec["sample_gb_per_s"] = round(written / (stage["sample_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
    rec["sample_share_of_8_tb_per_s"] = round(rec["sample_gb_per_s"] / 8000.0, 4)
    rec["torch_ops_over_kernel"] = round(stage["sample_torch_ops"]["median_ms"] /
                                         stage["sample_kernel"]["median_ms"], 2)
    print(json.dumps(rec), flush=True)
    if args.eval_json:
        with open(args.eval_json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--skip-step", type=int, default=4)
    ap.add_argument("--resolution", type=float, default=0.2)
    ap.add_argument("--level-set", type=float, default=0.0, help="iso level of the weight volume (reference: 0)")
    ap.add_argument("--ply", default="mesh_demo.ply")
    ap.add_argument("--json", default=None)
    ap.add_argument("--eval", action="store_true", help="sample the mesh into a cloud and score it")
    ap.add_argument("--eval-points", type=int, default=50_000_000, help="samples of the mesh (reference: 5 10^7)")
    ap.add_argument("--voxel", type=float, default=0.1, help="voxel size of the sampled cloud and of the comparison")
    ap.add_argument("--f-score-threshold", type=float, default=0.1)
    ap.add_argument("--eval-json", default=os.path.join(ROOT, "profiles", "mesh_cloud_demo.json"))
    args = ap.parse_args()
    import bench
    from loner_amd import evaluate as E
    from loner_amd import mesh_cloud as MC
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
    normals = MC.vertex_normals(verts, faces) if len(v) and len(faces) else None
    M.write_ply(args.ply, verts, faces, normals)
    rec["ply"] = os.path.basename(args.ply)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    if args.eval:
        evaluate(args, verts, faces, normals, scans, dev)


if __name__ == "__main__":
    main()
