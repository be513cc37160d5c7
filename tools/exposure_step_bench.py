#!/usr/bin/env python3
"""Per-step time of the HDR-NeRF recipe (use_exposure) on the proxy scene shown at five exposure times.

Two legs, ALTERNATED window by window in one process on one trainer (same model, same batches, same clocks):
  layered   the launch-per-operation tone-mapper: the three tonemapper_net_i modules composed as
            NGP.log_radiance_to_rgb composed them before the fused kernels (slice, add of ln(exposure), ones-padding,
            two linear launches a channel forward; act_bwd, linear_bwd_weight, linear_bwd_input per layer backward)
  fused     ngp_tonemap_fwd / ngp_tonemap_bwd (networks._ToneMapFn)

Prints one JSON line: per leg the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows).  --solo instead times both routes of the tone-mapper alone, forward and
backward (HIP events, median of 50), at the sample count of a steady-state batch of this scene (read from a step after the
warm-up).

  python tools/exposure_step_bench.py --rays 8192
  python tools/exposure_step_bench.py --solo
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngp_amd  # noqa: F401
from ngp_amd.datasets.colmap import _HDR_EXPOSURES
from ngp_amd.datasets.export import HDR_UNIT_EXPOSURE_RGB
from ngp_amd.networks import NGP
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG = 200, 20


def layered_tonemap(self, log_radiances, **kwargs):
    """the tone-mapper module by module"""
    out = []
    for i in range(3):
        inp = log_radiances[:, i:i + 1]
        if 'exposure' in kwargs:
            inp = inp + torch.log(kwargs['exposure'])
        out.append(getattr(self, f'tonemapper_net_{i}')(inp))
    return torch.cat(out, 1)


def set_leg(model, leg):
    if leg == "layered":
        model.log_radiance_to_rgb = types.MethodType(layered_tonemap, model)
    elif "log_radiance_to_rgb" in model.__dict__:
        del model.log_radiance_to_rgb


def median(v):
    return sorted(v)[len(v) // 2]


def solo(model, n):
    """both routes of the tone-mapper alone at n samples: forward, and forward + backward minus forward"""
    lr = (torch.rand(n, 3, device=DEV) * 12 - 6).requires_grad_(True)
    e = torch.tensor(list(_HDR_EXPOSURES["chair"].values()), device=DEV)[torch.randint(5, (n, 1), device=DEV)]
    g = torch.randn(n, 3, device=DEV)
    out = {"samples": n}
    for leg in ("layered", "fused"):
        set_leg(model, leg)

        def fwd():
            with torch.no_grad():
                model.log_radiance_to_rgb(lr, exposure=e)

        def both():
            model.log_radiance_to_rgb(lr, exposure=e).backward(g)

        for name, fn in (("fwd", fwd), ("fwd_bwd", both)):
            for _ in range(10):
                fn()
            us = []
            for _ in range(50):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            out[f"{leg}_{name}_us"] = round(median(us), 2)
        out[f"{leg}_bwd_us"] = round(out[f"{leg}_fwd_bwd_us"] - out[f"{leg}_fwd_us"], 2)
    set_leg(model, "fused")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5, help="windows per leg")
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(20220806)
    model = NGP(scale=0.5, rgb_act="None").to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    scene = LegoProxy(n_images=N_IMG, img_wh=(WH, WH), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    times = torch.tensor(list(_HDR_EXPOSURES["chair"].values()), device=DEV)
    c = (1.0 - HDR_UNIT_EXPOSURE_RGB) / HDR_UNIT_EXPOSURE_RGB
    batches = []
    for _ in range(16):     # resident batches: the loop times the step, not the ground-truth quadrature
        img, pix = scene.sample_batch(args.rays, generator=gen)
        o, d = scene.rays(img, pix)
        radiance, _ = scene.ground_truth(o, d, n_quad=64)
        e = times[torch.randint(5, (args.rays, 1), device=DEV, generator=gen)]
        x = radiance * e
        batches.append((o, d, (x / (x + c)).contiguous(), e.contiguous()))   # export.hdr_response on the device
    tr = NGPTrainer(model, lr=1e-2, use_exposure=True, unit_exposure_rgb=HDR_UNIT_EXPOSURE_RGB)
    step = lambda b: tr.step(b[0], b[1], b[2], exposure=b[3])
    k = 0
    for _ in range(args.warmup):
        _, res = step(batches[k % len(batches)])
        k += 1
    if args.solo:
        tr.wait()
        torch.cuda.synchronize()
        return solo(model, int(res["total_samples"]))
    windows = {"layered": [], "fused": []}
    samples = []
    for w in range(2 * args.windows):
        leg = ("layered", "fused")[w % 2]
        set_leg(model, leg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, res = step(batches[k % len(batches)])
            k += 1
        torch.cuda.synchronize()
        windows[leg].append((time.perf_counter() - t0) / args.steps * 1e3)
        samples.append(int(res["total_samples"]))
    tr.wait()
    print(json.dumps({"rays": args.rays, "steps_total": k, "loss": float(loss), "samples_last": int(np.median(samples)),
                      **{f"{leg}_ms_per_step_median": round(median(v), 4) for leg, v in windows.items()},
                      **{f"{leg}_ms_per_step_windows": [round(x, 4) for x in v] for leg, v in windows.items()},
                      "fused_loss": tr.recipe.fused_loss, "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
