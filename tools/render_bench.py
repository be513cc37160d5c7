#!/usr/bin/env python3
"""Test-time rendering throughput: trains the lego-proxy scene briefly, then renders full frames
through render(test_time=True) (rendering.py:46-133 semantics).  GPU only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngp_amd
from ngp_amd.networks import NGP
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer
from ngp_amd.metrics import psnr
from ngp_amd.rendering import render

ap = argparse.ArgumentParser()
ap.add_argument("--train-steps", type=int, default=600)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--wh", type=int, default=800)
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.manual_seed(20220806)
model = NGP(scale=0.5).to(dev).add_occupancy_grid()
scene = LegoProxy(img_wh=(args.wh, args.wh), device=dev)
tr = NGPTrainer(model, lr=1e-2)
gen = torch.Generator(device=dev).manual_seed(1)
for i in range(args.train_steps):
    img, pix = scene.sample_batch(8192, generator=gen)
    o, d = scene.rays(img, pix)
    gt, _ = scene.ground_truth(o, d, n_quad=128)
    tr.step(o, d, gt)
tr.wait()
torch.cuda.synchronize()

n = args.wh * args.wh
pix = torch.arange(n, device=dev)
times = []
for f in range(args.frames + 1):
    img = torch.full((n,), f % scene.poses.shape[0], dtype=torch.long, device=dev)
    o, d = scene.rays(img, pix)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = render(model, o, d, test_time=True, exp_step_factor=0.0, T_threshold=1e-2)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
gt, _ = scene.ground_truth(o[::16], d[::16], n_quad=256)
t = sum(times[1:]) / args.frames
print(json.dumps({"frame": f"{args.wh}x{args.wh}", "ms_per_frame": t * 1e3, "rays_per_s": n / t,
                  "samples_per_frame": int(out["total_samples"]), "psnr_subsampled": float(psnr(out["rgb"][::16], gt)),
                  "opaque_frac": float((out["opacity"] > 0.5).float().mean())}))
