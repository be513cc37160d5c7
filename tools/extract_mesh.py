#!/usr/bin/env python3
"""Extracts a triangle mesh from a trained checkpoint and writes it as binary PLY (the reference's extract_mesh.py:
density on a dense lattice, marching cubes, PLY).  GPU only.  Prints one JSON line: V, F and the milliseconds of the
density pass, marching cubes, the device->host copy and the PLY write (each timed around a device synchronise).

  python tools/extract_mesh.py --ckpt ckpts/lego.ckpt --scale 0.5 --out lego.ply --resolution 256 --normals
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
from ngp_amd import ckpt, mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_dataset import build_model  # noqa: E402  (the model the checkpoints of tools/train_dataset.py come from)

REFERENCE_CALL = "--bbox -1 -0.3 -1 1 0.15 1 --resolution 512 128 512 --level 10 --reference_spacing"


def main(argv=None):
    ap = argparse.ArgumentParser(
        description="Mesh of the level set sigma = level of a trained model.  The reference's own call is "
                    f"`{REFERENCE_CALL}`.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="checkpoint ({'state_dict': {'model.<key>': ...}})")
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--out", required=True, help="PLY file to write")
    ap.add_argument("--resolution", type=int, nargs="+", default=[512], help="one int, or nx ny nz")
    ap.add_argument("--bbox", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="lattice box (default: the model's [xyz_min, xyz_max])")
    ap.add_argument("--level", type=float, default=10.0)
    ap.add_argument("--normals", action="store_true", help="per-vertex normals -grad(sigma)/|grad(sigma)|")
    ap.add_argument("--reference_spacing", action="store_true",
                    help="place vertices as the reference does (spacing extent/n instead of extent/(n-1))")
    ap.add_argument("--chunk", type=int, default=128 ** 3)
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes 1 or 3 values")
    res = args.resolution[0] if len(args.resolution) == 1 else tuple(args.resolution)

    dev = torch.device("cuda", 0)
    model = build_model(args.scale, dev)
    ckpt.load_ckpt(model, args.ckpt, prefixes_to_ignore=['embedding_a', 'msk_model'])
    lo = args.bbox[:3] if args.bbox else model.xyz_min.reshape(3).tolist()
    hi = args.bbox[3:] if args.bbox else model.xyz_max.reshape(3).tolist()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = mesh.density_volume(model, lo, hi, res, args.chunk)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    verts, faces = mesh.marching_cubes(vol, args.level, mesh.lattice_spacing(lo, hi, vol.shape, args.reference_spacing),
                                       lo)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    nrm = mesh.vertex_normals(model, verts, args.chunk) if args.normals else None
    torch.cuda.synchronize()
    t_n = time.perf_counter()
    v, f = verts.cpu(), faces.cpu()
    nrm = None if nrm is None else nrm.cpu()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    mesh.write_ply(args.out, v, f, nrm)
    t4 = time.perf_counter()
    times = {"density_ms": 1e3 * (t1 - t0), "mc_ms": 1e3 * (t2 - t1), "normals_ms": 1e3 * (t_n - t2),
             "d2h_ms": 1e3 * (t3 - t_n), "ply_ms": 1e3 * (t4 - t3)}
    print(json.dumps({"V": int(v.shape[0]), "F": int(f.shape[0]), "lattice": list(vol.shape),
                      **{k: round(x, 3) for k, x in times.items()}}))


if __name__ == "__main__":
    main()
