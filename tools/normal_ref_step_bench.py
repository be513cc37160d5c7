#!/usr/bin/env python3
"""Per-step time of the normal_ref recipe on the proxy scene.

Three legs, ALTERNATED window by window in one process on one trainer (same model, same batches, same clocks), all past
the warm-up:
  default   the default recipe: no normal_ref term in the step
  module    loss_kwargs={'normal_ref': True}: the launch-per-operation route (differentiable normals by create_graph=True,
            the density MLP's second order on torch ops, VolumeRenderer, _RefLossInputs, RefLoss, the NeRFLoss module)
  fused     NGPTrainer(normal_ref=True): the fused field node with second-order normals (ngp_grid_bwd_bwd_input,
            ngp_density_head_bwd2 and four products), the fused tail and ngp_normal_ref_tail

Prints one JSON line: per leg the median and the values of --windows windows of --steps steps, each between two device
synchronisations (as bench.py counts its windows), and per leg the calls of the library's C entries in one step (counted
in two extra steps per leg behind the timed windows; the kernels torch launches itself are not among them).  --solo instead
times, on the arguments of one fused step (a steady-state batch's sample count; HIP events, median of 50),
ngp_density_head_bwd2, ngp_normal_ref_tail and the whole second-order share of _FieldFn.backward: the seven entry calls
from ngp_grid_bwd_bwd_input to the density table's ngp_grid_bwd_param, one behind the other, and each of them alone.

  python tools/normal_ref_step_bench.py --rays 8192
  python tools/normal_ref_step_bench.py --solo
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
SHARE = ("grid_bwd_bwd_input", "linear_fwd", "density_head_bwd2", "linear_bwd_weight", "linear_bwd_input", "grid_bwd_param")


def set_leg(tr, leg):
    tr.recipe.normal_ref = leg == "fused"
    tr.model.second_order_normals = leg == "fused"
    tr.model.differentiable_normals = leg == "module"
    tr.loss_kwargs = {"normal_ref": True} if leg == "module" else {}
    tr.recipe.fused_loss = leg != "module"


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


def solo(model, tr, batch):
    """the two new entries alone and the second-order share of the field's backward, on one fused step's own arguments"""
    set_leg(tr, "fused")
    tr.step(*batch)
    _lib.CAPTURE = {name: [] for name in SHARE + ("normal_ref_tail",)}
    tr.step(*batch)
    tr.wait()
    torch.cuda.synchronize()
    cap, _lib.CAPTURE = _lib.CAPTURE, None
    xe = model.xyz_encoder.desc
    cap["grid_bwd_param"] = [a for a in cap["grid_bwd_param"] if a[0] is xe]      # (the colour table's scatter is the other one)
    order = [("grid_bwd_bwd_input", 0), ("linear_fwd", 0), ("density_head_bwd2", 0), ("linear_bwd_weight", 0),
             ("linear_bwd_weight", 1), ("linear_bwd_input", 0), ("grid_bwd_param", 0)]
    counts = {name: len(v) for name, v in cap.items()}
    if counts != {"grid_bwd_bwd_input": 1, "linear_fwd": 1, "density_head_bwd2": 1, "linear_bwd_weight": 2,
                  "linear_bwd_input": 1, "grid_bwd_param": 1, "normal_ref_tail": 1}:
        raise SystemExit(f"a fused step's second-order share is not the seven calls this tool replays: {counts}")
    out = {"rays": int(batch[0].shape[0]), "samples": int(cap["density_head_bwd2"][0][5])}
    for k, (name, i) in enumerate(order):
        args = cap[name][i]
        out[f"share_{k}_{name}_us"] = timed(lambda: _lib.call(name, *args))
    out["second_order_share_us"] = timed(lambda: [_lib.call(name, *cap[name][i]) for name, i in order])
    out["density_head_bwd2_us"] = out["share_2_density_head_bwd2_us"]
    tail = cap["normal_ref_tail"][0]
    out["normal_ref_tail_us"] = timed(lambda: _lib.call("normal_ref_tail", *tail))
    tr.flat_grad.zero_()          # (the replays added to the gradient sinks)
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
    ap.add_argument("--warmup", type=int, default=320, help="steps before the first window, on the default recipe")
    ap.add_argument("--windows", type=int, default=5, help="windows per leg")
    ap.add_argument("--solo", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(20220806)
    model = NGP(scale=0.5).to(DEV)
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
        batches.append((o, d, gt.contiguous()))
    tr = NGPTrainer(model, lr=1e-2, normal_ref=True)
    if args.warmup < tr.warmup_steps:
        raise SystemExit(f"--warmup must reach the end of the trainer's warm-up ({tr.warmup_steps} steps): the legs are "
                         "compared past it")
    k = 0
    set_leg(tr, "default")
    for _ in range(args.warmup):
        tr.step(*batches[k % len(batches)])
        k += 1
    if args.solo:
        tr.wait()
        torch.cuda.synchronize()
        return solo(model, tr, batches[k % len(batches)])
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
