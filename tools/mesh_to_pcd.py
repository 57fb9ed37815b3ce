"""A triangle-mesh PLY as the point cloud the map metrics are computed on (GPU box): the command line of the
reference's analysis/compute_metrics/maps/mesh_to_pcd.py.  The mesh is read with loner_amd.meshing.read_ply, sampled
into --points points and voxel-filtered at RESOLUTION (loner_amd.mesh_cloud.mesh_to_cloud), and written next to the
PLY as ``<ply minus .ply>_sampled.pcd`` (loner_amd.map_eval.write_pcd).  The reference's unused lidar-to-camera
transform is not carried over.

    python tools/mesh_to_pcd.py PLY RESOLUTION [--points 50000000] [--key 0]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply_path")
    ap.add_argument("resolution", type=float)
    ap.add_argument("--points", type=int, default=50_000_000, help="samples of the mesh (reference: 5 10^7)")
    ap.add_argument("--key", type=int, default=0, help="key of the sampler's draws")
    args = ap.parse_args()
    from loner_amd import map_eval as ME
    from loner_amd import mesh_cloud as MC
    from loner_amd import meshing as M
    if not args.ply_path.endswith(".ply"):
        ap.error(f"{args.ply_path}: expected a .ply file")
    dev = torch.device("cuda", 0)
    verts, faces, _ = M.read_ply(args.ply_path)
    print(f"{args.ply_path}: {len(verts)} vertices, {len(faces)} faces")
    cloud = MC.mesh_to_cloud(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), args.resolution,
                             args.points, args.key)
    out = args.ply_path[:-len(".ply")] + "_sampled.pcd"
    ME.write_pcd(out, cloud)
    print(f"{out}: {cloud.shape[0]} points ({args.points} samples, voxel {args.resolution} m)")


if __name__ == "__main__":
    main()
