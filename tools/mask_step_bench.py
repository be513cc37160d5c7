#!/usr/bin/env python3
"""Per-step time of the embed_msk recipe on the proxy scene (scale 8, exponential stepping, random background).

Three legs, one process each (--leg):
  default   the default recipe, no mask
  layered   the route that needs no mask field in the package: a module assembled from tinycudann.Encoding +
            nn.Sequential with its own torch Adam, its output passed as mask= under loss_kwargs={'embed_msk': True}
            (the NeRFLoss module and torch autograd replace the fused tail, the exact norm replaces the norm bound)
  fused     NGPTrainer(model, msk_model=implicit_mask()): ngp_mask_field_fwd / _bwd and the masked fused tail

Prints one JSON line: the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows).  --solo instead times the two mask kernels alone (HIP events,
median of 50 launches) at 2048 and 8192 rows.

  python tools/mask_step_bench.py --leg fused --rays 8192
  rocprofv3 --kernel-trace --stats -d out -- python tools/mask_step_bench.py --leg fused --windows 1
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
from ngp_amd import tinycudann as tcnn
from ngp_amd._lib import call
from ngp_amd.implicit_mask import implicit_mask
from ngp_amd.networks import NGP
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG = 200, 20


class LayeredMask(torch.nn.Module):
    """the mask field as separate launches: grid encoding, two linear layers, two activations"""

    def __init__(self):
        super().__init__()
        ref = implicit_mask()
        self.mask_encoder = tcnn.Encoding(3, ref.mask_encoder.encoding_config)
        self.mask_net = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.ReLU(), torch.nn.Linear(64, 1),
                                            torch.nn.Sigmoid())

    def forward(self, uvi):
        return self.mask_net(self.mask_encoder(uvi))


def solo():
    msk = implicit_mask().to(DEV)
    l1, l2 = msk.mask_net[0], msk.mask_net[2]
    out = {}
    for n in (2048, 8192):
        uvi = torch.rand(n, 3, device=DEV) - 0.5
        mask, g = torch.empty(n, device=DEV), torch.randn(n, device=DEV)
        grads = [torch.zeros_like(p) for p in (msk.mask_encoder.params, l1.weight, l1.bias, l2.weight, l2.bias)]
        fwd = lambda: call("mask_field_fwd", msk.mask_encoder.desc, msk.mask_encoder.params, l1.weight, l1.bias, l2.weight,
                           l2.bias, uvi, n, mask)
        bwd = lambda: call("mask_field_bwd", msk.mask_encoder.desc, msk.mask_encoder.params, l1.weight, l1.bias, l2.weight,
                           uvi, mask, g, n, *grads)
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
            out[f"mask_field_{name}_us_{n}"] = round(sorted(us)[len(us) // 2], 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("default", "layered", "fused"), default="fused")
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    if args.solo:
        return solo()
    torch.manual_seed(20220806)
    model = NGP(scale=8.0).to(DEV)
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
        uvi = implicit_mask.uvi(torch.stack([pix // WH, pix % WH], -1), img, (WH, WH), N_IMG)
        batches.append((o, d, gt.contiguous(), uvi))
    kw = dict(lr=1e-2, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    opt = None
    if args.leg == "default":
        tr = NGPTrainer(model, **kw)
        step = lambda b: tr.step(b[0], b[1], b[2])
    elif args.leg == "fused":
        tr = NGPTrainer(model, msk_model=implicit_mask().to(DEV), **kw)
        step = lambda b: tr.step(b[0], b[1], b[2], uvi=b[3])
    else:
        msk = LayeredMask().to(DEV)
        opt = torch.optim.Adam(msk.parameters(), lr=1e-2, eps=1e-8)
        tr = NGPTrainer(model, loss_kwargs={"embed_msk": True}, **kw)

        def step(b):
            opt.zero_grad(set_to_none=True)
            out = tr.step(b[0], b[1], b[2], mask=msk(b[3]), step=tr.global_step)
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
            loss, _ = step(batches[k % len(batches)])
            k += 1
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    tr.wait()
    print(json.dumps({"leg": args.leg, "rays": args.rays, "steps_total": k, "loss": float(loss),
                      "ms_per_step_median": round(sorted(windows)[len(windows) // 2], 4),
                      "ms_per_step_windows": [round(w, 4) for w in windows],
                      "fused_loss": tr.recipe.fused_loss, "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
