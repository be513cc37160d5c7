#!/usr/bin/env python3
"""Per-step time of the embed_a recipe on the proxy scene (scale 8, exponential stepping, random background, E = 8).

Three legs, one process each (--leg):
  none     the same recipe without appearance codes
  tensor   the route that needs nothing of appearance.py: the codes are an external nn.Parameter (n_imgs, E), indexed per
           ray and passed as embedding_a= (render() expands them per sample with torch operations, autograd sums their
           gradient), stepped by their own torch.optim.Adam(lr, eps=1e-8)
  fused    NGPTrainer(model, embedding_a=nn.Embedding): ngp_embed_a_fwd / ngp_embed_a_bwd, the table in the flat store

Prints one JSON line: the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows), and the sample count of the last step (the legs train different
models, so their occupancy grids and sample counts differ).  --solo instead times the two kernels alone (HIP events, median of
50 launches) on 8192 rays / about 440 k samples, with every ray of another image (all_images) and with all rays of one
image (same_image).

  python tools/embed_a_step_bench.py --leg fused --rays 8192
  rocprofv3 --kernel-trace --stats -d out -- python tools/embed_a_step_bench.py --leg fused --windows 1
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
from ngp_amd.networks import NGP
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG, E = 200, 20, 8


def solo():
    n_rays, n_imgs, Kp = 8192, 100, 160
    gen = torch.Generator(device=DEV).manual_seed(11)
    counts = torch.randint(0, 109, (n_rays,), device=DEV, generator=gen)      # mean 54 samples a ray
    starts = torch.cumsum(counts, 0) - counts
    rays_a = torch.stack([torch.randperm(n_rays, device=DEV, generator=gen), starts, counts], 1).contiguous()
    n = int(counts.sum())
    weight = torch.randn(n_imgs, E, device=DEV)
    rgb_in = torch.zeros(n, Kp, device=DEV)
    dfeat = torch.randn(n, 128 + E, device=DEV)
    d_weight = torch.zeros(n_imgs, E, device=DEV)
    out = {"rays": n_rays, "samples": n, "E": E}
    for tag, idx in (("all_images", torch.randint(n_imgs, (n_rays,), device=DEV, generator=gen)),
                     ("same_image", torch.full((n_rays,), 7, dtype=torch.int64, device=DEV))):
        fwd = lambda: call("embed_a_fwd", weight, n_imgs, E, idx, rays_a, n_rays, rgb_in[:, 144:], Kp, Kp - 144)
        bwd = lambda: call("embed_a_bwd", dfeat[:, 128:], 128 + E, E, idx, rays_a, n_rays, n_imgs, d_weight)
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
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
            us.sort()
            out[f"embed_a_{name}_us_{tag}"] = {"median": round(us[len(us) // 2], 2), "min": round(us[0], 2),
                                               "max": round(us[-1], 2)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("none", "tensor", "fused"), default="fused")
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    if args.solo:
        return solo()
    torch.manual_seed(20220806)
    model = (NGP(scale=8.0) if args.leg == "none" else NGP(scale=8.0, embed_a=True, embed_a_len=E)).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    scene = LegoProxy(n_images=N_IMG, img_wh=(WH, WH), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    batches = []
    for _ in range(16):     # resident batches: the loop times the step, not the ground-truth quadrature
        img, pix = scene.sample_batch(args.rays, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt.contiguous(), img.to(torch.int64).contiguous()))
    kw = dict(lr=1e-2, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    emb = torch.nn.Embedding(N_IMG, E).to(DEV)
    if args.leg == "none":
        tr = NGPTrainer(model, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2])
    elif args.leg == "fused":
        tr = NGPTrainer(model, embedding_a=emb, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], img_idxs=b[3])
    else:
        codes = torch.nn.Parameter(emb.weight.detach().clone())
        opt = torch.optim.Adam([codes], lr=1e-2, eps=1e-8)
        tr = NGPTrainer(model, **kw)

        def step(b):
            opt.zero_grad(set_to_none=True)
            tr.render_kwargs["embedding_a"] = codes[b[3]]
            out = tr.step(b[0], b[1], b[2])
            opt.step()
            return out

    k = 0
    for _ in range(args.warmup):
        step(batches[k % len(batches)])
        k += 1
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, res = step(batches[k % len(batches)])
            k += 1
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    tr.wait()
    print(json.dumps({"leg": args.leg, "rays": args.rays, "steps_total": k, "loss": float(loss),
                      "samples_last_step": int(res["total_samples"]),
                      "ms_per_step_median": round(sorted(windows)[len(windows) // 2], 4),
                      "ms_per_step_windows": [round(w, 4) for w in windows],
                      "fused_loss": tr.recipe.fused_loss, "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
