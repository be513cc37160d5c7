#!/usr/bin/env python3
"""The record of profiles/cloud_eval.txt: ngp_amd.cloud on surface samples of the analytic proxy scene.  Target 2^22
points, 2^20 queries (another seed): grid build and query time of nearest_points under HIP events, the chosen cell and
the points per occupied cell, the time per ICP iteration from a small known offset, and for scale a plain-torch brute
force at 2^14 x 2^14 and scipy's cKDTree on the host at the full size.  GPU only; prints one JSON line per item.

  python tools/cloud_eval_bench.py [--target 4194304] [--queries 1048576] [--resolution 256]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngp_amd  # noqa: F401
from ngp_amd import cloud, mesh


def _eval_mesh_tool():
    spec = importlib.util.spec_from_file_location("tool_eval_mesh", os.path.join(ROOT, "tools", "eval_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(fn, repeats):
    """-> (result, [ms]) with HIP events around each call"""
    out, ms = None, []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1), 3))
    return out, ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--target", type=int, default=1 << 22)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--resolution", type=int, default=256, help="lattice of the proxy surface")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no_host_tree", action="store_true", help="skip scipy's cKDTree")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    verts, faces = _eval_mesh_tool().proxy_reference(args.resolution, dev)
    target, _ = mesh.sample_surface(verts, faces, args.target, seed=1)
    queries, _ = mesh.sample_surface(verts, faces, args.queries, seed=2)
    torch.cuda.synchronize()

    grid, build = _timed(lambda: cloud.PointGrid(target), args.repeats)
    print(json.dumps(dict(item="grid", points=grid.n, cell=grid.cell, dims=grid.dims, occupied=grid.occupied,
                          points_per_occupied_cell=round(grid.n / grid.occupied, 3), build_ms=build)))
    order = grid.sort_queries(queries)
    sorted_q = queries[order].contiguous()
    d2 = torch.empty(args.queries, device=dev)
    index = torch.empty(args.queries, dtype=torch.int32, device=dev)
    max_dist = float(np.float32(2.0))
    _, sort_ms = _timed(lambda: queries[grid.sort_queries(queries)].contiguous(), args.repeats)
    _, kernel = _timed(lambda: grid.launch(sorted_q, max_dist, d2=d2, index=index), args.repeats)
    _, unsorted = _timed(lambda: grid.launch(queries, max_dist, d2=d2, index=index), 2)
    _, whole = _timed(lambda: cloud.nearest_points(queries, grid), args.repeats)
    print(json.dumps(dict(item="nearest", queries=args.queries, sort_ms=sort_ms, kernel_ms=kernel,
                          kernel_unsorted_queries_ms=unsorted, nearest_points_ms=whole,
                          mean_dist=float(torch.sqrt(d2).double().mean()))))

    # ICP from a known small offset: 1 degree about z through the centre, 0.005 along x
    a = np.deg2rad(1.0)
    T0 = np.eye(4)
    T0[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T0[0, 3] = 0.005
    moved = cloud.transform_points(queries, np.linalg.inv(T0))
    T, info = cloud.icp(moved, None, 0.05, max_iter=20, grid=grid)
    print(json.dumps(dict(item="icp", iterations=info["iterations"], fitness=info["fitness"],
                          inlier_rmse=info["inlier_rmse"], iteration_ms=[round(x, 3) for x in info["iteration_ms"]],
                          error=float(np.abs(T - T0).max()))))

    # for scale: a plain-torch brute force at 2^14 x 2^14
    small_q, small_t = queries[:1 << 14], target[:1 << 14]
    _, brute = _timed(lambda: torch.cdist(small_q, small_t).min(1), args.repeats)
    _, ours = _timed(lambda: cloud.nearest_points(small_q, small_t), args.repeats)
    print(json.dumps(dict(item="brute_force_16384x16384", torch_cdist_min_ms=brute, nearest_points_ms=ours)))

    if not args.no_host_tree:
        from scipy.spatial import cKDTree
        tq, tt = queries.cpu().numpy(), target.cpu().numpy()
        t0 = time.perf_counter()
        tree = cKDTree(tt)
        t1 = time.perf_counter()
        dist, _ = tree.query(tq, workers=16)
        t2 = time.perf_counter()
        worst = float(np.abs(dist - torch.sqrt(d2).cpu().numpy()).max())   # d2: the last launch took the queries as given
        print(json.dumps(dict(item="host_ckdtree", build_ms=round(1e3 * (t1 - t0), 1),
                              query_ms_16_workers=round(1e3 * (t2 - t1), 1), worst_difference=worst)))


if __name__ == "__main__":
    main()
