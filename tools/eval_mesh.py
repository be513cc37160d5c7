#!/usr/bin/env python3
"""Scores a mesh against a reference surface: accuracy (mesh -> reference), completeness (reference -> mesh), Chamfer,
Hausdorff and precision / recall / F-score at thresholds (the Tanks-and-Temples measure), from area-weighted samples
of both surfaces and exact point-to-mesh distances (ngp_amd.mesh.mesh_distance).  GPU only.  Prints one JSON line:
the metrics, V / F of both meshes and the milliseconds of reading, sampling, grid build and query of each direction.

  python tools/eval_mesh.py --mesh lego.ply --ref lego_gt.ply --thresholds 0.005 0.01
  python tools/eval_mesh.py --mesh proxy.ply --ref_proxy --thresholds 0.005 0.01    # against the analytic proxy scene
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngp_amd  # noqa: F401
from ngp_amd import mesh, synthetic


def proxy_reference(resolution, device):
    """the surface of the analytic proxy scene: synthetic.analytic_sigma is SIGMA_IN inside the solids and 0 outside,
    so its surface is the level SIGMA_IN / 2 of the field sampled on a lattice over [-0.5, 0.5]^3 (marching cubes
    puts each vertex half-way between an inside and an outside sample: within half a lattice spacing of the solid)"""
    lo, hi = [-0.5] * 3, [0.5] * 3
    n, axes = mesh.lattice_axes(lo, hi, resolution, device)
    vol = synthetic.analytic_sigma(torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)).contiguous()
    return mesh.marching_cubes(vol, synthetic.SIGMA_IN / 2, mesh.lattice_spacing(lo, hi, n), lo)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Distance metrics between a mesh and a reference mesh.",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--mesh", required=True, help="PLY of the mesh to score (triangles)")
    ref = ap.add_mutually_exclusive_group(required=True)
    ref.add_argument("--ref", help="PLY of the reference mesh (triangles)")
    ref.add_argument("--ref_proxy", action="store_true",
                     help="the reference is the surface of the analytic proxy scene (ngp_amd.synthetic)")
    ap.add_argument("--ref_resolution", type=int, default=512, help="lattice points per axis of --ref_proxy")
    ap.add_argument("--samples", type=int, default=1_000_000, help="surface samples per mesh")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="distances for precision / recall / F-score")
    ap.add_argument("--max_dist", type=float, help="clip distances here (default: nothing is clipped)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
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
