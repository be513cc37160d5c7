#!/usr/bin/env python3
"""Per-step time of the skybox recipe (use_skybox) on the proxy scene composited over the analytic sky.

Three legs, ALTERNATED window by window in one process on one trainer (same model, same batches, same clocks), all past
the warm-up:
  default   the default recipe: no skybox in the step (the model's skybox network idles)
  module    render_kwargs={'use_skybox': True}: the launch-per-operation route (model(...), VolumeRenderer, forward_skybox
            module by module, RefLoss, nerf_loss_and_grads, the distortion pair, composite_train_bw)
  fused     NGPTrainer(use_skybox=True): ngp_skybox_fwd, ngp_render_loss_fused_sky, ngp_skybox_bwd

Prints one JSON line: per leg the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows), and per leg the calls of the library's C entries in one step (counted
in two extra steps per leg behind the timed windows; the kernels torch launches itself are not among them).  --solo instead
times the two sky kernels alone at --rays rays, and ngp_render_loss_fused_sky against ngp_render_loss_fused on the same
marched batch of the scene (HIP events, median of 50).

  python tools/sky_step_bench.py --rays 8192
  python tools/sky_step_bench.py --solo
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
from ngp_amd import _lib
from ngp_amd.networks import NGP
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG = 200, 20
LEGS = ("default", "module", "fused")


def set_leg(tr, leg):
    tr.recipe.use_skybox = leg == "fused"
    tr.render_kwargs = {"use_skybox": True} if leg == "module" else {}


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps=50, warm=10):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(median(us), 2)


def solo(model, tr, batch, n_rays):
    """the sky kernels alone, both routes of the skybox at n_rays rays, and the two tail entries on one marched batch"""
    d = torch.randn(n_rays, 3, device=DEV)
    g = torch.randn(n_rays, 3, device=DEV)
    out = {"rays": n_rays}
    for leg, fwd in (("module", model.forward_skybox), ("fused", model.skybox_rgb)):
        def f():
            with torch.no_grad():
                fwd(d)

        def both():
            fwd(d).backward(g)
        out[f"sky_{leg}_fwd_us"] = timed(f)
        out[f"sky_{leg}_fwd_bwd_us"] = timed(both)
        out[f"sky_{leg}_bwd_us"] = round(out[f"sky_{leg}_fwd_bwd_us"] - out[f"sky_{leg}_fwd_us"], 2)
    # the two tail entries on the arguments of one step of this trainer (captured from the step itself)
    _lib.CAPTURE = {"render_loss_fused": [], "render_loss_fused_sky": []}
    for leg in ("default", "fused"):
        set_leg(tr, leg)
        tr.step(*batch)
    torch.cuda.synchronize()
    cap, _lib.CAPTURE = _lib.CAPTURE, None
    for name, calls in cap.items():
        args = calls[-1]
        out[f"{name}_us"] = timed(lambda: _lib.call(name, *args))
    out["samples"] = int(cap["render_loss_fused_sky"][-1][0].shape[0])
    print(json.dumps(out))


def entry_calls(tr, leg, batches, k):
    """{C entry: calls} of one step of the leg (the second of two steps)"""
    set_leg(tr, leg)
    tr.step(*batches[k % len(batches)])
    _lib.PROFILE = {name[4:]: [] for name in _lib.PROTOS}
    tr.step(*batches[(k + 1) % len(batches)])
    tr.wait()
    torch.cuda.synchronize()
    prof, _lib.PROFILE = _lib.PROFILE, None
    return {name: len(v) for name, v in sorted(prof.items()) if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=320, help="steps before the first window; the skybox joins at step 256")
    ap.add_argument("--windows", type=int, default=5, help="windows per leg")
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(20220806)
    model = NGP(scale=0.5, use_skybox=True).to(DEV)
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
        gt, _ = scene.ground_truth(o, d, n_quad=64, sky=True)
        batches.append((o, d, gt.contiguous()))
    tr = NGPTrainer(model, lr=1e-2, use_skybox=True)
    if args.warmup < tr.warmup_steps:
        raise SystemExit(f"--warmup must reach the end of the trainer's warm-up ({tr.warmup_steps} steps): the legs are "
                         "compared past it")
    k = 0
    for _ in range(args.warmup):
        tr.step(*batches[k % len(batches)])
        k += 1
    if args.solo:
        tr.wait()
        torch.cuda.synchronize()
        return solo(model, tr, batches[k % len(batches)], args.rays)
    windows = {leg: [] for leg in LEGS}
    samples = []
    for w in range(len(LEGS) * args.windows):
        leg = LEGS[w % len(LEGS)]
        set_leg(tr, leg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, res = tr.step(*batches[k % len(batches)])
            k += 1
        torch.cuda.synchronize()
        windows[leg].append((time.perf_counter() - t0) / args.steps * 1e3)
        samples.append(int(res["total_samples"]))
    tr.wait()
    # six steps without an occupancy-grid update among them: the entries of the steady state
    tr.global_step = tr.global_step // tr.update_interval * tr.update_interval + 1
    calls = {leg: entry_calls(tr, leg, batches, k) for leg in LEGS}
    print(json.dumps({"rays": args.rays, "steps_total": k, "loss": float(loss), "samples_last": median(samples),
                      **{f"{leg}_ms_per_step_median": round(median(v), 4) for leg, v in windows.items()},
                      **{f"{leg}_ms_per_step_windows": [round(x, 4) for x in v] for leg, v in windows.items()},
                      **{f"{leg}_entry_calls_per_step": sum(c.values()) for leg, c in calls.items()},
                      "entry_calls": calls, "norm_bound": tr.norm_bound}))


if __name__ == "__main__":
    main()
