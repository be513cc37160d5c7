#!/usr/bin/env python3
"""Extracts a triangle mesh from a trained checkpoint and writes it as binary PLY (the reference's extract_mesh.py:
density on a dense lattice, marching cubes, PLY).  GPU only.  Prints one JSON line: V, F and the milliseconds of the
density pass, marching cubes, the cleaning, the simplification, the normals, the colours, the device->host copy and
the PLY write (each timed around a device synchronise), what the cleaning found and removed, and what the
simplification did (cell, k, probes, clusters, V_in, V_out, F_in, F_out, degenerate, duplicate, probe_ms, emit_ms).
--report_distance adds simplify_distance: how far the simplification moved the surface (mesh.mesh_distance between the
cleaned and the simplified mesh: accuracy, completeness, hausdorff, each also in cells).

  python tools/extract_mesh.py --ckpt ckpts/lego.ckpt --scale 0.5 --out lego.ply --resolution 256 --normals
  python tools/extract_mesh.py --ckpt ckpts/lego.ckpt --scale 0.5 --out lego.ply --keep_largest 1 --colors
  python tools/extract_mesh.py --ckpt ckpts/lego.ckpt --scale 0.5 --out lego.ply --keep_largest 1 --target_faces 100000
  python tools/extract_mesh.py --ckpt ckpts/lego.ckpt --scale 0.5 --out lego.ply --target_faces 100000 --report_distance
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


def simplify_distance(cleaned, simplified, cell, n_samples):
    """accuracy (simplified -> cleaned), completeness (cleaned -> simplified) and hausdorff between the mesh that went
    into simplify_mesh and the one that came out, each also in units of the chosen cell; None for an empty mesh"""
    if cell is None or cleaned[1].shape[0] == 0 or simplified[1].shape[0] == 0:
        return None
    d = mesh.mesh_distance(*simplified, *cleaned, n_samples=n_samples)
    out = {k: d[k] for k in ("accuracy", "completeness", "hausdorff")}
    out.update({k + "_cells": d[k] / cell for k in ("accuracy", "completeness", "hausdorff")})
    out.update(cell=cell, samples=n_samples)
    return out


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
    ap.add_argument("--keep_largest", type=int, metavar="K",
                    help="keep only the K connected pieces with the most faces (floater removal)")
    ap.add_argument("--min_faces", type=int, metavar="M", help="keep only the connected pieces with at least M faces")
    simplify = ap.add_mutually_exclusive_group()
    simplify.add_argument("--simplify_cell", type=float, metavar="X",
                          help="merge the vertices of each cubic cell of edge X (from the lattice's corner) into one")
    simplify.add_argument("--target_faces", type=int, metavar="N",
                          help="simplify with the smallest cell found that leaves at most N faces")
    ap.add_argument("--placement", choices=("quadric", "mean"), default="quadric",
                    help="where a merged vertex goes: the quadric minimiser of its faces' planes, or the mean")
    ap.add_argument("--report_distance", action="store_true",
                    help="with --simplify_cell / --target_faces: how far the simplification moved the surface "
                         "(simplify_distance in the JSON line)")
    ap.add_argument("--distance_samples", type=int, default=1_000_000, metavar="N",
                    help="surface samples per mesh of --report_distance")
    ap.add_argument("--colors", action="store_true",
                    help="per-vertex RGB rendered from the trained appearance field (PLY red green blue)")
    ap.add_argument("--embed_a", action="store_true",
                    help="the checkpoint was trained with appearance codes (--embed_a): --colors renders with the code of training image 0")
    ap.add_argument("--embed_a_len", type=int, default=4, help="length of an appearance code")
    ap.add_argument("--use_skybox", action="store_true",
                    help="the checkpoint was trained with --use_skybox: the model is built with the skybox so that it loads "
                         "(the mesh and its colours do not look at the background)")
    ap.add_argument("--chunk", type=int, default=128 ** 3)
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes 1 or 3 values")
    if args.simplify_cell is not None and not args.simplify_cell > 0:
        ap.error("--simplify_cell must be positive")
    if args.target_faces is not None and args.target_faces < 0:
        ap.error("--target_faces must be >= 0")
    if args.report_distance and args.simplify_cell is None and args.target_faces is None:
        ap.error("--report_distance needs --simplify_cell or --target_faces")
    if args.distance_samples < 1:
        ap.error("--distance_samples must be >= 1")
    res = args.resolution[0] if len(args.resolution) == 1 else tuple(args.resolution)

    dev = torch.device("cuda", 0)
    model = build_model(args.scale, dev, args.embed_a, args.embed_a_len, use_skybox=args.use_skybox)
    ckpt.load_ckpt(model, args.ckpt, prefixes_to_ignore=['embedding_a', 'msk_model'])
    more = {}
    if args.embed_a:
        table = ckpt.extract_model_state_dict(args.ckpt, model_name='embedding_a')['weight']
        if table.dim() != 2 or table.shape[1] != args.embed_a_len:
            raise SystemExit(f"--embed_a_len {args.embed_a_len}: the checkpoint's table is {tuple(table.shape)}")
        more["embedding_a"] = table[0:1].to(dev).float().contiguous()
    lo = args.bbox[:3] if args.bbox else model.xyz_min.reshape(3).tolist()
    hi = args.bbox[3:] if args.bbox else model.xyz_max.reshape(3).tolist()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol = mesh.density_volume(model, lo, hi, res, args.chunk)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    spacing = mesh.lattice_spacing(lo, hi, vol.shape, args.reference_spacing)
    verts, faces = mesh.marching_cubes(vol, args.level, spacing, lo)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    stats = {"components": None, "V_removed": 0, "F_removed": 0}
    if args.keep_largest is not None or args.min_faces is not None:
        verts, faces = mesh.clean_mesh(verts, faces, keep_largest=args.keep_largest, min_faces=args.min_faces,
                                       stats=stats)
    torch.cuda.synchronize()
    t_c = time.perf_counter()
    simplified = {}
    if args.simplify_cell is not None or args.target_faces is not None:
        cleaned = (verts, faces)
        verts, faces = mesh.simplify_mesh(verts, faces, cell=args.simplify_cell, target_faces=args.target_faces,
                                          origin=lo, placement=args.placement, stats=simplified)
    torch.cuda.synchronize()
    t_s = time.perf_counter()
    report = {}
    t_r = t_s
    if args.report_distance:     # on a clock of its own: simplify_ms and normals_ms mean what they mean without the flag
        report["simplify_distance"] = simplify_distance(cleaned, (verts, faces), simplified["cell"],
                                                        args.distance_samples)
        torch.cuda.synchronize()
        t_r = time.perf_counter()
        report["simplify_distance_ms"] = round(1e3 * (t_r - t_s), 3)
    nrm = mesh.vertex_normals(model, verts, args.chunk) if args.normals or args.colors else None
    torch.cuda.synchronize()
    t_n = time.perf_counter()
    rgb = mesh.vertex_colors(model, verts, nrm, 2 * max(spacing), **more) if args.colors else None
    torch.cuda.synchronize()
    t_k = time.perf_counter()
    v, f = verts.cpu(), faces.cpu()
    nrm = None if nrm is None or not args.normals else nrm.cpu()
    rgb = None if rgb is None else rgb.cpu()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    mesh.write_ply(args.out, v, f, nrm, rgb)
    t4 = time.perf_counter()
    times = {"density_ms": 1e3 * (t1 - t0), "mc_ms": 1e3 * (t2 - t1), "normals_ms": 1e3 * (t_n - t_r),
             "d2h_ms": 1e3 * (t3 - t_k), "ply_ms": 1e3 * (t4 - t3), "clean_ms": 1e3 * (t_c - t2),
             "colors_ms": 1e3 * (t_k - t_n), "simplify_ms": 1e3 * (t_s - t_c)}
    print(json.dumps({"V": int(v.shape[0]), "F": int(f.shape[0]), "lattice": list(vol.shape),
                      **{k: round(x, 3) for k, x in times.items()},
                      **{k: stats[k] for k in ("components", "V_removed", "F_removed")},
                      **{k: round(x, 3) if isinstance(x, float) and k.endswith("_ms") else x
                         for k, x in simplified.items()}, **report}))


if __name__ == "__main__":
    main()
