#!/usr/bin/env python3
"""Per-step time of the normal_mono recipe on the proxy scene with its analytic normals (scale 0.5).

Three legs, one process each (--leg), to be alternated by the caller in one job:
  default   the default recipe, no normals
  module    NGPTrainer(loss_kwargs={'normal_mono': True}) with step(target={'normal': ...}): model(...), VolumeRenderer,
            RefLoss, the distortion pair, NeRFLoss and torch's element-wise normal term as separate launches, exact
            gradient norm
  fused     NGPTrainer(normal_mono=True) with step(normals=...): the fused field and ngp_render_loss_fused_nrm

Prints one JSON line: the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows).  --solo instead times ngp_render_loss_fused_nrm alone against
ngp_render_loss_fused on the same marched batch of the scene (HIP events, median of 50 launches) at 2048 and 8192 rays.

  python tools/normal_step_bench.py --leg fused --rays 8192
  python tools/normal_step_bench.py --solo
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
from ngp_amd._lib import call
from ngp_amd import vren
from ngp_amd.custom_functions import RayMarcher
from ngp_amd.networks import NGP
from ngp_amd.rendering import MAX_SAMPLES, intersect_scene
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG, CLASSES = 200, 20, 7


def make_model():
    model = NGP(scale=0.5).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


def median_us(fn, n=50, warm=10):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(sorted(us)[len(us) // 2], 2)


@torch.no_grad()
def solo():
    """both tail entries on one marched batch of the scene's analytic occupancy, with random field outputs"""
    torch.manual_seed(20220806)
    model = make_model()
    scene = LegoProxy(n_images=N_IMG, img_wh=(WH, WH), device=DEV)
    model.density_grid.copy_(scene.occupancy_from_analytic(model))
    vren.packbits(model.density_grid.view(-1), 0.5, model.density_bitfield)
    gen = torch.Generator(device=DEV).manual_seed(7)
    out = {}
    for nr in (2048, 8192):
        img, pix = scene.sample_batch(nr, generator=gen)
        o, d = scene.rays(img, pix)
        normals = scene.ground_truth_normals(o, d, n_quad=64).contiguous()
        hits_t = intersect_scene(model, o.contiguous(), d.contiguous())
        rays_a, xyzs, dirs, deltas, ts, _ = RayMarcher.apply(o, d, hits_t[:, 0], model.density_bitfield, model.cascades,
                                                             model.scale, 0.0, model.grid_size, MAX_SAMPLES)
        n = xyzs.shape[0]
        R = lambda *s: torch.rand(*s, device=DEV, generator=gen)
        sig, rgbs, dsig, nrm, sem = R(n) * 40, R(n, 3), R(n, 3) - 0.5, R(n, 3) - 0.5, R(n, CLASSES) * 4 - 2
        gt = R(nr, 3)
        E = lambda *s: torch.empty(*s, device=DEV)
        total = torch.empty(nr, dtype=torch.int64, device=DEV)
        acc = E(12)
        outs = (E(nr), E(nr), E(nr, 3), E(nr, 3), E(nr, CLASSES), E(n), E(nr), E(nr, 3))
        d_sig, d_rgb, d_np = E(n), E(n, 3), E(n, 3)
        head = (sig, rgbs, dsig, None, nrm, 3, sem, CLASSES, dirs, deltas, ts, rays_a, gt, None)
        plain = lambda: call("render_loss_fused", *head, 1e-4, CLASSES, nr, 2e-4, 3e-4, total, acc[4:6].view(torch.int64),
                             *outs, acc[:4], d_sig, d_rgb)
        nrmf = lambda: call("render_loss_fused_nrm", *head, normals, 1e-3, 1e-4, CLASSES, nr, 2e-4, 3e-4, total,
                            acc[6:8].view(torch.int64), *outs, acc[:5], d_sig, d_rgb, acc[8:12].view(torch.int32), d_np)
        out[f"samples_{nr}"] = n
        out[f"rays_with_a_normal_{nr}"] = int((normals != 0).any(-1).sum())
        out[f"render_loss_fused_us_{nr}"] = median_us(plain)
        out[f"render_loss_fused_nrm_us_{nr}"] = median_us(nrmf)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("default", "module", "fused"), default="fused")
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    if args.solo:
        return solo()
    torch.manual_seed(20220806)
    model = make_model()
    scene = LegoProxy(n_images=N_IMG, img_wh=(WH, WH), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    batches = []
    for _ in range(16):     # resident batches: the loop times the step, not the ground-truth quadrature
        img, pix = scene.sample_batch(args.rays, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt.contiguous(), scene.ground_truth_normals(o, d, n_quad=64).contiguous()))
    kw = dict(lr=1e-2)
    if args.leg == "default":
        tr = NGPTrainer(model, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2])
    elif args.leg == "fused":
        tr = NGPTrainer(model, normal_mono=True, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], normals=b[3])
    else:
        tr = NGPTrainer(model, loss_kwargs={"normal_mono": True}, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], target={"normal": b[3]})
    k = 0
    for _ in range(args.warmup):
        step(batches[k % len(batches)])
        k += 1
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, _ = step(batches[k % len(batches)])
            k += 1
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    tr.wait()
    print(json.dumps({"leg": args.leg, "rays": args.rays, "steps_total": k, "loss": float(loss),
                      "ms_per_step_median": round(sorted(windows)[len(windows) // 2], 4),
                      "ms_per_step_windows": [round(w, 4) for w in windows],
                      "fused_loss": tr.recipe.fused_loss, "normal_mono": tr.recipe.normal_mono, "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
