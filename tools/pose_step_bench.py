#!/usr/bin/env python3
"""Per-step time of pose refinement (optimize_ext) on the proxy scene, and the solo times of its three kernels.

  python tools/pose_step_bench.py --rays 2048 8192          # legs alternated in one job: none | torch | kernels
  python tools/pose_step_bench.py --solo --rays 8192        # ngp_pose_rays_fwd / _bwd and ngp_sh_bwd_dirs alone

Legs: `none` trains with the dataset's rays (no refiner: the default step); `torch` forms the rays and ties the samples to
dR, dT with torch operations (axisangle_to_R, get_rays, repeat_interleave, indexing; their autograd chain is the adjoint);
`kernels` is pose.PoseRefiner.  Both pose legs run NGPTrainer's pose step and the field's dL/dx and dL/dd routes, so the
difference between them is the ray / pose part alone.  Each leg trains its own model from the same seed; windows of
`--window` steps are timed with HIP events, legs alternated window by window.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngp_amd  # noqa: F401
from ngp_amd._lib import call
from ngp_amd.datasets.ray_utils import axisangle_to_R, get_rays
from ngp_amd.networks import NGP
from ngp_amd.pose import PoseRefiner
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"


class TorchPoseRefiner(PoseRefiner):
    """the same interface on torch operations"""

    def _rays(self, img, pix):
        c2w = torch.cat([axisangle_to_R(self.dR[img]) @ self.poses[img][..., :3],
                         (self.poses[img][..., 3] + self.dT[img])[..., None]], -1)
        return get_rays(self.directions[pix], c2w)

    def rays(self, img_idxs, pix_idxs):
        o, d = self._rays(img_idxs, pix_idxs)
        return o.contiguous(), d.contiguous()

    def attach_samples(self, xyzs, dirs, ts, rays_a, img_idxs, pix_idxs):
        o, d = self._rays(img_idxs, pix_idxs)
        ray_of = torch.repeat_interleave(rays_a[:, 0], rays_a[:, 2], output_size=ts.shape[0])
        return o[ray_of] + ts[:, None] * d[ray_of], d[ray_of]


def build_model():
    torch.manual_seed(20220806)
    model = NGP(scale=0.5).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


class Leg:
    def __init__(self, kind, scene, n_rays):
        self.kind, self.scene, self.n_rays = kind, scene, n_rays
        self.model = build_model()
        self.ref = None
        if kind != "none":
            self.ref = (PoseRefiner if kind == "kernels" else TorchPoseRefiner)(scene.poses, scene.directions).to(DEV)
        self.tr = NGPTrainer(self.model, lr=1e-2, **({} if self.ref is None else {"pose_refiner": self.ref, "pose_lr": 1e-5}))
        self.gen = torch.Generator(device=DEV).manual_seed(7)
        self.samples = 0

    def step(self):
        img, pix = self.scene.sample_batch(self.n_rays, generator=self.gen)
        o, d = self.scene.rays(img, pix)
        gt, _ = self.scene.ground_truth(o, d, n_quad=64)
        if self.ref is None:
            _, res = self.tr.step(o, d, gt)
        else:
            _, res = self.tr.step(None, None, gt, img_idxs=img, pix_idxs=pix)
        self.samples = res["total_samples"]

    def window(self, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            self.step()
        self.tr.wait()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps


def steps_bench(n_rays, warmup, windows, window):
    scene = LegoProxy(n_images=20, img_wh=(200, 200), device=DEV)
    legs = [Leg(k, scene, n_rays) for k in ("none", "torch", "kernels")]
    for leg in legs:
        for _ in range(warmup):
            leg.step()
        leg.tr.wait()
    torch.cuda.synchronize()
    ms = {leg.kind: [] for leg in legs}
    for _ in range(windows):
        for leg in legs:
            ms[leg.kind].append(round(leg.window(window), 4))
    out = {"rays": n_rays, "warmup": warmup, "window": window}
    for leg in legs:
        v = sorted(ms[leg.kind])
        out[leg.kind] = {"ms_per_step_median": v[len(v) // 2], "windows": ms[leg.kind], "last_samples": int(leg.samples)}
    return out


def solo(n_rays, reps=50):
    """the three kernels alone on the samples of one marched batch of the warmed-up proxy model"""
    scene = LegoProxy(n_images=20, img_wh=(200, 200), device=DEV)
    leg = Leg("kernels", scene, n_rays)
    for _ in range(320):
        leg.step()
    leg.tr.wait()
    from ngp_amd.rendering import render
    out = {"rays": n_rays}
    for pattern in ("random", "one_image"):
        img, pix = scene.sample_batch(n_rays, generator=leg.gen)
        if pattern == "one_image":
            img = torch.full_like(img, 3)
        ref = leg.ref
        with torch.no_grad():
            o, d = ref.rays(img, pix)
            res = render(leg.model, o, d)
        n = int(res["total_samples"])
        ts, rays_a = res["ts"].contiguous(), res["rays_a"].contiguous()
        g_x, g_dir = torch.randn(n, 3, device=DEV), torch.randn(n, 3, device=DEV)
        dy = torch.randn(n, 16, device=DEV)
        dirs = torch.repeat_interleave(d[rays_a[:, 0]], rays_a[:, 2], 0).contiguous()
        acc = torch.zeros(2, ref.dR.shape[0], 3, device=DEV)
        o2, d2, gd = torch.empty_like(o), torch.empty_like(d), torch.empty(n, 3, device=DEV)
        n_imgs, n_pix = ref.poses.shape[0], ref.directions.shape[0]
        jobs = {"pose_rays_fwd": lambda: call("pose_rays_fwd", ref.poses, ref.dR.detach(), ref.dT.detach(), ref.directions, img,
                                              pix, n_imgs, n_pix, n_rays, o2, d2),
                "pose_rays_bwd": lambda: call("pose_rays_bwd", g_x, g_dir, ts, rays_a, ref.poses, ref.dR.detach(), ref.directions,
                                              img, pix, n_imgs, n_pix, n_rays, n, acc[0], acc[1]),
                "sh_bwd_dirs": lambda: call("sh_bwd_dirs", dirs, dy, 16, n, gd)}
        res_p = {"samples": n}
        for name, fn in jobs.items():
            for _ in range(5):
                fn()
            times = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            times.sort()
            res_p[name + "_us_median"] = round(times[len(times) // 2], 2)
        out[pattern] = res_p
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--warmup", type=int, default=320)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    if args.solo:
        print(json.dumps({"solo": [solo(n) for n in args.rays]}))
    else:
        print(json.dumps({"steps": [steps_bench(n, args.warmup, args.windows, args.window) for n in args.rays]}))


if __name__ == "__main__":
    main()
