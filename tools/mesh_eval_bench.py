#!/usr/bin/env python3
"""Times mesh evaluation (M4) on a proxy export and scores the export against the analytic scene: the record of
profiles/mesh_eval.txt.  Trains the lego proxy for --steps steps (or loads --ckpt), extracts the mesh at --resolution,
cleans it (keep_largest=1) and simplifies it (--target_faces), then prints one JSON line per measurement:

  score     mesh_distance of the raw, the cleaned and the simplified export against the proxy's own surface
            (tools/eval_mesh.py --ref_proxy), with the stage times of the last of --repeats warm calls
  simplify  mesh_distance between the cleaned and the simplified export (what --report_distance reports)
  brute     for scale: every one of 2^14 samples against every one of 2^14 faces in plain torch (the same closest-point
            sequence, chunked), beside closest_on_mesh on the same inputs, and whether the two agree

Times are host clocks around device synchronisation, after one warm-up call of every shape.  GPU only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngp_amd
from ngp_amd import ckpt, mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_mesh import proxy_reference  # noqa: E402
from train_dataset import build_model  # noqa: E402

DEV = torch.device("cuda", 0)


def train_proxy(steps):
    """the fixture of tests/test_mesh_simplify_gpu.py: the lego proxy from analytic rays, 4096 rays per step"""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    torch.manual_seed(3)
    model = ngp_amd.networks.NGP(scale=0.5).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    scene = LegoProxy(n_images=40, img_wh=(200, 200), device=DEV)
    tr = NGPTrainer(model, lr=1e-2)
    gen = torch.Generator(device=DEV).manual_seed(4)
    for _ in range(steps):
        img, pix = scene.sample_batch(4096, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=128)
        tr.step(o, d, gt)
    tr.wait()
    torch.cuda.synchronize()
    return model


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def torch_brute_d2(p, a, b, c, chunk=512):
    """the closest-point sequence of include/ngp_hip.h M4 in eager torch: p (n,3) against all faces (a, b, c (F,3))
    -> the smallest d2 per point (ties and degenerate faces are not its business: it is here for its time)"""
    out = torch.empty(p.shape[0], device=p.device)
    ab, ac = (b - a)[None], (c - a)[None]
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        ap, bp, cp = q - a[None], q - b[None], q - c[None]
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1 / ((va + vb) + vc)
        x = (a[None] + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        qs = [a[None], b[None], a[None] + ab * (d1 / (d1 - d3))[..., None], c[None],
              a[None] + ac * (d2 / (d2 - d6))[..., None],
              b[None] + (c - b)[None] * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]]
        for k in range(5, -1, -1):
            x = torch.where(conds[k][..., None], qs[k], x)
        e = q - x
        out[s:s + chunk] = torch.nan_to_num(_dot(e, e), nan=float("inf")).amin(1)
    return out


def timed(fn, repeats):
    """-> (result of the last call, milliseconds of each of `repeats` calls after one warm-up)"""
    fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(round(1e3 * (time.perf_counter() - t0), 3))
    return out, ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", help="a proxy checkpoint (scale 0.5); default: train one here")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--ref_resolution", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--target_faces", type=int, default=100000)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.005, 0.01, 0.02])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)

    if args.ckpt:
        model = build_model(0.5, DEV, False, 4)
        ckpt.load_ckpt(model, args.ckpt, prefixes_to_ignore=['embedding_a', 'msk_model'])
    else:
        model = train_proxy(args.steps)
    lo = model.xyz_min.reshape(3).tolist()
    raw = mesh.extract_mesh(model, resolution=args.resolution, level=10.0)
    cleaned = mesh.clean_mesh(*raw, keep_largest=1)
    sstats = {}
    simplified = mesh.simplify_mesh(*cleaned, target_faces=args.target_faces, origin=lo, stats=sstats)
    ref = proxy_reference(args.ref_resolution, DEV)

    def measure(kind, name, a, b):
        stats = {}
        out, ms = timed(lambda: mesh.mesh_distance(*a, *b, n_samples=args.samples, thresholds=args.thresholds,
                                                   stats=stats), args.repeats)
        sides = {}
        for side, target in (("a_to_b", b), ("b_to_a", a)):
            s = stats[side]
            sides[side] = dict(cell=s["cell"], dims=s["dims"], references=s["references"], probes=s["probes"],
                               references_per_face=round(s["references"] / max(target[1].shape[0], 1), 3),
                               build_ms=round(s["build_ms"], 3), query_ms=round(s["query_ms"], 3))
        print(json.dumps({"kind": kind, "mesh": name, "V": a[0].shape[0], "F": a[1].shape[0], "V_ref": b[0].shape[0],
                          "F_ref": b[1].shape[0], "samples": args.samples, **out, "mesh_distance_ms": ms,
                          "sample_ms": round(stats["sample_ms"], 3), **sides}), flush=True)

    for name, m in (("raw", raw), ("cleaned", cleaned), ("simplified", simplified)):
        measure("score", name, m, ref)
    print(json.dumps({"kind": "simplification", **{k: sstats[k] for k in ("cell", "k", "F_in", "F_out")}}), flush=True)
    measure("simplify", "simplified_vs_cleaned", simplified, cleaned)

    n = 1 << 14
    pts, _ = mesh.sample_surface(*cleaned, n, seed=1)
    sub_f = ref[1][:n].contiguous()
    a, b, c = (ref[0][sub_f[:, k].long()] for k in range(3))
    brute, brute_ms = timed(lambda: torch_brute_d2(pts, a, b, c), args.repeats)
    stats = {}
    (d2, _), grid_ms = timed(lambda: mesh.closest_on_mesh(pts, ref[0], sub_f, stats=stats, squared=True), args.repeats)
    print(json.dumps({"kind": "brute", "points": n, "faces": int(sub_f.shape[0]), "torch_brute_ms": brute_ms,
                      "closest_on_mesh_ms": grid_ms, "build_ms": round(stats["build_ms"], 3),
                      "query_ms": round(stats["query_ms"], 3), "d2_equal": int((d2 == brute).sum()),
                      "d2_max_abs_diff": float((d2 - brute).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
