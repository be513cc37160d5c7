#!/usr/bin/env python3
"""Per-step time of the semantic + normal_mono + depth_mono recipe on the proxy scene with its labels, normals and depths
(scale 0.5).

Three legs, one process each (--leg), to be alternated by the caller in one job:
  default   the default recipe, no targets
  module    NGPTrainer(loss_kwargs={'semantic': True, 'normal_mono': True, 'depth_mono': True, 'scale': 0.5}) with
            step(target={'label', 'normal', 'depth'}): model(...), VolumeRenderer, RefLoss, the distortion pair, NeRFLoss's
            cross-entropy, normal and depth terms and compute_scale_and_shift's torch reductions (with a host read of the
            determinant in every step) as separate launches, exact gradient norm
  multi     NGPTrainer(multi_terms=('semantic', 'normal_mono', 'depth_mono')) with step(labels=, normals=, depths=): the
            fused field and ngp_render_loss_fused_multi (the label count, the fit kernel, then the tail)

Prints one JSON line: the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows).  --solo instead times ngp_render_loss_fused_multi alone (all three terms:
three launches) against ngp_render_loss_fused and against the three single entries on the same marched batch of the scene
(HIP events, median of 50 calls) at 2048 and 8192 rays.

  python tools/multi_step_bench.py --leg multi --rays 8192
  python tools/multi_step_bench.py --solo
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


def mono_depths(scene, o, d):
    """25 (0.37 D + 0.11) where the ray has a depth, 0 (invalid) elsewhere"""
    D = scene.ground_truth_depths(o, d, n_quad=64)
    return torch.where(D > 0, 25.0 * (0.37 * D + 0.11), torch.zeros_like(D)).contiguous()


def targets(scene, o, d, gen):
    """the scene's labels (0-4, 256), its normals with a random direction where it has none (every target non-zero: where the
    module states the same loss) and its monocular depths"""
    lab = scene.ground_truth_labels(o, d, n_quad=64).to(torch.int64).contiguous()
    nrm = scene.ground_truth_normals(o, d, n_quad=64)
    rnd = torch.nn.functional.normalize(torch.randn(nrm.shape, device=DEV, generator=gen), dim=-1)
    nrm = torch.where((nrm != 0).any(-1, keepdim=True), nrm, rnd).contiguous()
    return lab, nrm, mono_depths(scene, o, d)


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
    """the five tail entries on one marched batch of the scene's analytic occupancy, with random field outputs"""
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
        labels, normals, depths = targets(scene, o, d, gen)
        hits_t = intersect_scene(model, o.contiguous(), d.contiguous())
        rays_a, xyzs, dirs, deltas, ts, _ = RayMarcher.apply(o, d, hits_t[:, 0], model.density_bitfield, model.cascades,
                                                             model.scale, 0.0, model.grid_size, MAX_SAMPLES)
        n = xyzs.shape[0]
        R = lambda *s: torch.rand(*s, device=DEV, generator=gen)
        sig, rgbs, dsig, nrm, sem = R(n) * 40, R(n, 3), R(n, 3) - 0.5, R(n, 3) - 0.5, R(n, CLASSES) * 4 - 2
        gt = R(nr, 3)
        E = lambda *s: torch.empty(*s, device=DEV)
        total = torch.empty(nr, dtype=torch.int64, device=DEV)
        acc = E(40)
        outs = (E(nr), E(nr), E(nr, 3), E(nr, 3), E(nr, CLASSES), E(n), E(nr), E(nr, 3))
        d_sig, d_rgb, d_sem, d_np = E(n), E(n, 3), E(n, CLASSES), E(n, 3)
        sem_ws = torch.empty(8, dtype=torch.int32, device=DEV)
        head = (sig, rgbs, dsig, None, nrm, 3, sem, CLASSES, dirs, deltas, ts, rays_a, gt, None)
        plain = lambda: call("render_loss_fused", *head, 1e-4, CLASSES, nr, 2e-4, 3e-4, total, acc[4:6].view(torch.int64),
                             *outs, acc[:4], d_sig, d_rgb)
        depf = lambda: call("render_loss_fused_dep", *head, depths, 1.0, 0.5, 1e-4, CLASSES, nr, 2e-4, 3e-4, total,
                            acc[6:8].view(torch.int64), *outs, acc[:5], d_sig, d_rgb, acc[8:26].view(torch.int32))
        semf = lambda: call("render_loss_fused_sem", *head, labels, 4e-2, 1e-1, 1e-4, CLASSES, nr, 2e-4, 3e-4, total,
                            acc[6:8].view(torch.int64), *outs, acc[:6], d_sig, d_rgb, sem_ws, d_sem)
        nrmf = lambda: call("render_loss_fused_nrm", *head, normals, 1e-3, 1e-4, CLASSES, nr, 2e-4, 3e-4, total,
                            acc[6:8].view(torch.int64), *outs, acc[:5], d_sig, d_rgb, acc[8:12].view(torch.int32), d_np)
        multi = lambda: call("render_loss_fused_multi", *head, 7, labels, 4e-2, 1e-1, normals, 1e-3, depths, 1.0, 0.5, 1e-4,
                             CLASSES, nr, 2e-4, 3e-4, total, acc[8:10].view(torch.int64), *outs, acc[:8], d_sig, d_rgb,
                             acc[10:40].view(torch.int32), d_sem, d_np)
        out[f"samples_{nr}"] = n
        out[f"rays_with_a_depth_{nr}"] = int((depths > 0).sum())
        out[f"render_loss_fused_us_{nr}"] = median_us(plain)
        out[f"render_loss_fused_sem_us_{nr}"] = median_us(semf)
        out[f"render_loss_fused_nrm_us_{nr}"] = median_us(nrmf)
        out[f"render_loss_fused_dep_us_{nr}"] = median_us(depf)
        out[f"render_loss_fused_multi_us_{nr}"] = median_us(multi)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("default", "module", "multi"), default="multi")
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
        batches.append((o, d, gt.contiguous()) + targets(scene, o, d, gen))
    kw = dict(lr=1e-2)
    if args.leg == "default":
        tr = NGPTrainer(model, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2])
    elif args.leg == "multi":
        tr = NGPTrainer(model, multi_terms=("semantic", "normal_mono", "depth_mono"), **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], labels=b[3], normals=b[4], depths=b[5])
    else:
        tr = NGPTrainer(model, loss_kwargs={"semantic": True, "normal_mono": True, "depth_mono": True, "scale": 0.5}, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], target={"label": b[3], "normal": b[4], "depth": b[5]})
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
                      "fused_loss": tr.recipe.fused_loss, "multi_terms": list(tr.recipe.multi_terms), "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
