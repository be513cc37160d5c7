#!/usr/bin/env python3
"""Scores a mesh against a reference surface: accuracy (mesh -> reference), completeness (reference -> mesh), Chamfer,
Hausdorff and precision / recall / F-score at thresholds (the Tanks-and-Temples measure), from area-weighted samples
of both surfaces and exact point-to-mesh distances (ngp_amd.mesh.mesh_distance).  GPU only.  Prints one JSON line:
the metrics, V / F of both meshes and the milliseconds of reading, sampling, grid build and query of each direction.

  python tools/eval_mesh.py --mesh lego.ply --ref lego_gt.ply --thresholds 0.005 0.01
  python tools/eval_mesh.py --mesh proxy.ply --ref_proxy --thresholds 0.005 0.01    # against the analytic proxy scene

Against a point-cloud reference (a laser scan, --ref_points) the mesh is stood for by its surface samples or its
vertices, moved by --init_transform, cropped by --crop (Open3D's SelectionPolygonVolume JSON, in the reference's frame)
and registered by --align: `tnt` runs the three ICP stages of the Tanks-and-Temples protocol and scores both clouds
down-sampled at dtau / 2 (ngp_amd.cloud.tnt_score), `icp` one point-to-point ICP at 20 dtau on the full clouds, `none`
nothing.  The JSON line then holds cloud_distance's metrics with dtau among the thresholds, the refined transform,
fitness / rmse / time per stage and the points kept by crop and down-sampling.

  python tools/eval_mesh.py --mesh barn.ply --ref_points Barn.ply --init_transform Barn_trans.txt --crop Barn.json \
      --align tnt --dtau 0.01 --save_transform Barn_refined.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngp_amd  # noqa: F401
from ngp_amd import cloud, mesh, synthetic


def proxy_reference(resolution, device):
    """the surface of the analytic proxy scene: synthetic.analytic_sigma is SIGMA_IN inside the solids and 0 outside,
    so its surface is the level SIGMA_IN / 2 of the field sampled on a lattice over [-0.5, 0.5]^3 (marching cubes
    puts each vertex half-way between an inside and an outside sample: within half a lattice spacing of the solid)"""
    lo, hi = [-0.5] * 3, [0.5] * 3
    n, axes = mesh.lattice_axes(lo, hi, resolution, device)
    vol = synthetic.analytic_sigma(torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)).contiguous()
    return mesh.marching_cubes(vol, synthetic.SIGMA_IN / 2, mesh.lattice_spacing(lo, hi, n), lo)


def score_against_points(args, va, fa, dev, t0):
    """the --ref_points route: prints the JSON line"""
    gt = torch.from_numpy(cloud.read_ply_points(args.ref_points)[0]).to(dev)
    if args.recon_from == "vertices":
        recon = va
    else:
        recon = mesh.sample_surface(va, fa, args.samples, seed=args.seed)[0]
    init = np.loadtxt(args.init_transform).reshape(4, 4) if args.init_transform else np.eye(4)
    crop = cloud.CropVolume.from_json(args.crop) if args.crop else None
    thresholds = ([args.dtau] if args.dtau is not None else []) + [t for t in args.thresholds if t != args.dtau]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    align = args.align or "none"
    stats = {}
    if align == "tnt":
        res = cloud.tnt_score(recon, gt, args.dtau, init=init, crop=crop, with_scale=args.with_scale,
                              thresholds=thresholds, stats=stats)
        T, stages, points, out = np.array(res["transform"]), res["stages"], res["points"], res["metrics"]
    else:
        T, stages = init, []
        b = cloud._keep(gt, crop)
        if align == "icp":
            step, info = cloud.icp(cloud._keep(cloud.transform_points(recon, T), crop), b, 20 * args.dtau,
                                   with_scale=args.with_scale)
            T = step @ T
            stages = [{k: info[k] for k in ("fitness", "inlier_rmse", "iterations", "ms_per_iteration")}]
        a = cloud._keep(cloud.transform_points(recon, T), crop)
        points = dict(recon=int(recon.shape[0]), recon_cropped=int(a.shape[0]), recon_scored=int(a.shape[0]),
                      gt=int(gt.shape[0]), gt_cropped=int(b.shape[0]), gt_scored=int(b.shape[0]))
        out = cloud.cloud_distance(a, b, thresholds=thresholds, max_dist=args.max_dist, stats=stats)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if args.dtau is not None:
        out["fscore_dtau"] = out["fscore"][0]
    if args.save_transform:
        np.savetxt(args.save_transform, T)
    times = {"read_ms": 1e3 * (t1 - t0), "distance_ms": 1e3 * (t2 - t1)}
    for side in ("a_to_b", "b_to_a"):
        times[f"{side}_build_ms"] = stats[side]["build_ms"]
        times[f"{side}_query_ms"] = stats[side]["query_ms"]
    print(json.dumps({**out, "V": int(va.shape[0]), "F": int(fa.shape[0]), "align": align, "dtau": args.dtau,
                      "transform": T.tolist(), "stages": stages, "points": points,
                      **{k: round(x, 3) for k, x in times.items()},
                      "cell_ref": stats["a_to_b"]["cell"], "cell_mesh": stats["b_to_a"]["cell"]}))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Distance metrics between a mesh and a reference mesh.",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--mesh", required=True, help="PLY of the mesh to score (triangles)")
    ref = ap.add_mutually_exclusive_group(required=True)
    ref.add_argument("--ref", help="PLY of the reference mesh (triangles)")
    ref.add_argument("--ref_proxy", action="store_true",
                     help="the reference is the surface of the analytic proxy scene (ngp_amd.synthetic)")
    ref.add_argument("--ref_points", help="PLY of a reference point cloud (a scan; faces, if any, are ignored)")
    ap.add_argument("--ref_resolution", type=int, default=512, help="lattice points per axis of --ref_proxy")
    ap.add_argument("--samples", type=int, default=1_000_000, help="surface samples per mesh")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="distances for precision / recall / F-score")
    ap.add_argument("--max_dist", type=float, help="clip distances here (default: nothing is clipped)")
    ap.add_argument("--seed", type=int, default=0)
    pc = ap.add_argument_group("with --ref_points")
    pc.add_argument("--recon_from", choices=["samples", "vertices"], help="what stands for the mesh: --samples surface "
                    "samples (default) or its vertices")
    pc.add_argument("--init_transform", help="text file of a 4x4 matrix: reference ~ matrix * mesh")
    pc.add_argument("--crop", help="JSON of an Open3D SelectionPolygonVolume in the reference's frame")
    pc.add_argument("--align", choices=["none", "icp", "tnt"], help="registration before scoring (default none)")
    pc.add_argument("--dtau", type=float, help="the distance threshold of the protocol (needed by icp and tnt)")
    pc.add_argument("--with_scale", action="store_true", help="let the registration estimate a scale")
    pc.add_argument("--save_transform", help="write the refined 4x4 matrix here")
    args = ap.parse_args(argv)
    cloud_flags = {k: getattr(args, k) for k in ("recon_from", "init_transform", "crop", "align", "dtau", "with_scale",
                                                 "save_transform")}
    if args.ref_points is None and any(cloud_flags.values()):
        ap.error("--" + next(k for k, v in cloud_flags.items() if v) + " needs --ref_points")
    if args.ref_points is not None:
        if args.align in ("icp", "tnt") and not (args.dtau is not None and args.dtau > 0):
            ap.error(f"--align {args.align} needs --dtau > 0")
        if args.dtau is not None and not args.dtau > 0:
            ap.error("--dtau must be > 0")
    if args.samples < 1:
        ap.error("--samples must be >= 1")
    if args.max_dist is not None and not args.max_dist >= 0:
        ap.error("--max_dist must be >= 0")
    if args.ref_resolution < 2:
        ap.error("--ref_resolution must be >= 2")

    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    v, f, _ = mesh.read_ply(args.mesh)
    va, fa = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    if args.ref_points is not None:
        return score_against_points(args, va, fa, dev, t0)
    if args.ref_proxy:
        vb, fb = proxy_reference(args.ref_resolution, dev)
    else:
        v, f, _ = mesh.read_ply(args.ref)
        vb, fb = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    stats = {}
    out = mesh.mesh_distance(va, fa, vb, fb, n_samples=args.samples, thresholds=args.thresholds,
                             max_dist=args.max_dist, seed=args.seed, stats=stats)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    times = {"read_ms": 1e3 * (t1 - t0), "distance_ms": 1e3 * (t2 - t1), "sample_ms": stats["sample_ms"]}
    for side in ("a_to_b", "b_to_a"):
        times[f"{side}_build_ms"] = stats[side]["build_ms"]
        times[f"{side}_query_ms"] = stats[side]["query_ms"]
    print(json.dumps({**out, "V": int(va.shape[0]), "F": int(fa.shape[0]), "V_ref": int(vb.shape[0]),
                      "F_ref": int(fb.shape[0]), "samples": args.samples,
                      **{k: round(x, 3) for k, x in times.items()},
                      "cell_ref": stats["a_to_b"]["cell"], "cell_mesh": stats["b_to_a"]["cell"]}))


if __name__ == "__main__":
    main()
