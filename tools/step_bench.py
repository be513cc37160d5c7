#!/usr/bin/env python3
"""Per-step time of a training recipe on the proxy scene (20 views of 200 x 200), and the solo times of its kernels.

  python tools/step_bench.py <recipe> [--leg L] [--rays N] [--steps N] [--warmup N] [--windows N] [--solo]

<recipe> is a field of recipe.Recipe; SPECS below holds one spec per recipe, which says only what differs between them: the
model, the targets of a batch, the legs and how each trains, the warm-up, the protocol and the --solo body.  Everything else
exists once.  Three protocols, each printing one JSON line:

  process   one process per leg (--leg), to be alternated by the caller in one job: the median and the values of --windows
            windows of --steps steps, each between two device synchronisations (as bench.py counts its windows)
            (semantic, normal_mono, depth_mono, multi_terms, masked, embed_a)
  alternate the legs alternated window by window in one process on ONE trainer (same model, same batches, same clocks), the
            same windows per leg; use_skybox and normal_ref add the calls of the library's C entries in one step of each leg
            (counted in two extra steps per leg behind the timed windows; the kernels torch launches itself are not among them)
            (use_skybox, normal_ref, use_exposure)
  models    the legs alternated window by window, each training its own model from the same seed on batches it draws itself,
            windows timed with HIP events; takes several --rays (pose)

--solo times the recipe's kernels alone instead (HIP events, median of 50 calls).

  python tools/step_bench.py multi_terms --leg multi --rays 8192
  python tools/step_bench.py use_skybox --solo
  rocprofv3 --kernel-trace --stats -d out -- python tools/step_bench.py embed_a --leg fused --windows 1
"""
import argparse
import inspect
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngp_amd  # noqa: F401
from ngp_amd import _lib, vren
from ngp_amd import tinycudann as tcnn
from ngp_amd.custom_functions import RayMarcher
from ngp_amd.datasets.colmap import _HDR_EXPOSURES
from ngp_amd.datasets.export import HDR_UNIT_EXPOSURE_RGB
from ngp_amd.datasets.ray_utils import axisangle_to_R, get_rays
from ngp_amd.implicit_mask import implicit_mask
from ngp_amd.networks import NGP
from ngp_amd.pose import PoseRefiner
from ngp_amd.rendering import MAX_SAMPLES, TAIL_LAYOUT, intersect_scene, render
from ngp_amd.synthetic import LegoProxy
from ngp_amd.trainer import NGPTrainer

DEV = "cuda"
WH, N_IMG = 200, 20
call = _lib.call


# ---------------------------------------------------------------------------------------------- what exists once
def make_model(scale=0.5, **ngp):
    torch.manual_seed(20220806)
    return NGP(scale=scale, **ngp).to(DEV).add_occupancy_grid()


def make_scene():
    return LegoProxy(n_images=N_IMG, img_wh=(WH, WH), device=DEV)


def make_batches(spec, scene, n_rays):
    """16 resident batches (o, d, gt, the recipe's targets as step()'s keywords): the loop times the step, not the
    ground-truth quadrature"""
    gen = torch.Generator(device=DEV).manual_seed(7)
    batches = []
    for _ in range(16):
        img, pix = scene.sample_batch(n_rays, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64, **spec.ground_truth)
        gt, more = spec.targets(scene, img, pix, o, d, gt, gen)
        batches.append((o, d, gt.contiguous(), more))
    return batches


class Stepper:
    """walks the resident batches: run(step, n) takes n steps and returns the last one's (loss, results)"""

    def __init__(self, batches):
        self.batches, self.k = batches, 0

    def run(self, step, n):
        out = None
        for _ in range(n):
            out = step(self.batches[self.k % len(self.batches)])
            self.k += 1
        return out

    def window(self, step, n):
        """-> ms per step of n steps between two device synchronisations, the last step's (loss, results)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.run(step, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, out


def median(v):
    return sorted(v)[len(v) // 2]


def windows_json(windows, prefix=""):
    return {f"{prefix}ms_per_step_median": round(median(windows), 4), f"{prefix}ms_per_step_windows": [round(w, 4) for w in windows]}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_us(fn, n=50, warm=10):
    """-> the sorted times of n calls behind `warm` untimed ones (HIP events round the Python call)"""
    for _ in range(warm):
        fn()
    return sorted(event_ms(fn) * 1e3 for _ in range(n))


def median_us(fn, n=50, warm=10):
    return round(median(timed_us(fn, n, warm)), 2)


def fwd_bwd_us(out, key, fwd, g):
    """out[key_fwd_us], out[key_fwd_bwd_us] and their difference out[key_bwd_us] of the differentiable fwd()"""
    def f():
        with torch.no_grad():
            fwd()
    out[f"{key}_fwd_us"] = median_us(f)
    out[f"{key}_fwd_bwd_us"] = median_us(lambda: fwd().backward(g))
    out[f"{key}_bwd_us"] = round(out[f"{key}_fwd_bwd_us"] - out[f"{key}_fwd_us"], 2)


def entry_calls(spec, tr, leg, stepper):
    """{C entry: calls} of one step of the leg (the second of two steps)"""
    spec.set_leg(tr, leg)
    k = stepper.k
    stepper.run(spec.step(tr), 1)
    _lib.PROFILE = {name[4:]: [] for name in _lib.PROTOS}
    stepper.run(spec.step(tr), 1)
    stepper.k = k
    tr.wait()
    torch.cuda.synchronize()
    prof, _lib.PROFILE = _lib.PROFILE, None
    return {name: len(v) for name, v in sorted(prof.items()) if v}


# ---------------------------------------------------------------------------------------------- the three protocols
def run_process(spec, args):
    if args.solo:
        return spec.solo(args)
    model, scene = make_model(spec.scale, **spec.ngp(args.leg)), make_scene()
    stepper = Stepper(make_batches(spec, scene, args.rays))
    tr, step = spec.leg(args.leg, model)
    stepper.run(step, args.warmup)
    windows = []
    for _ in range(args.windows):
        ms, (loss, res) = stepper.window(step, args.steps)
        windows.append(ms)
    tr.wait()
    return {"leg": args.leg, "rays": args.rays, "steps_total": stepper.k, "loss": float(loss), **windows_json(windows),
            **spec.report(tr, res), "norm_bound": tr.norm_bound}


def run_alternate(spec, args):
    model, scene = make_model(spec.scale, **spec.ngp(None)), make_scene()
    stepper = Stepper(make_batches(spec, scene, args.rays))
    tr = spec.trainer(model)
    if spec.past_warmup and args.warmup < tr.warmup_steps:
        raise SystemExit(f"--warmup must reach the end of the trainer's warm-up ({tr.warmup_steps} steps): the legs are "
                         "compared past it")
    step = spec.step(tr)
    spec.set_leg(tr, spec.warm_leg)
    warm = stepper.run(step, args.warmup)
    if args.solo:
        tr.wait()
        torch.cuda.synchronize()
        return spec.solo(args, model, tr, stepper.batches[stepper.k % 16], int(warm[1]["total_samples"]))
    windows = {leg: [] for leg in spec.legs}
    samples = []
    for w in range(len(spec.legs) * args.windows):
        leg = spec.legs[w % len(spec.legs)]
        spec.set_leg(tr, leg)
        ms, (loss, res) = stepper.window(step, args.steps)
        windows[leg].append(ms)
        samples.append(int(res["total_samples"]))
    tr.wait()
    out = {"rays": args.rays, "steps_total": stepper.k, "loss": float(loss), "samples_last": median(samples)}
    for leg, v in windows.items():
        out.update(windows_json(v, leg + "_"))
    if spec.entry_report:
        # two steps per leg without an occupancy-grid update among them: the entries of the steady state
        tr.global_step = tr.global_step // tr.update_interval * tr.update_interval + 1
        calls = {leg: entry_calls(spec, tr, leg, stepper) for leg in spec.legs}
        out.update({f"{leg}_entry_calls_per_step": sum(c.values()) for leg, c in calls.items()}, entry_calls=calls)
    return {**out, **spec.report(tr, res), "norm_bound": tr.norm_bound}


def run_models(spec, args):
    if args.solo:
        return {"solo": [spec.solo(args, n) for n in args.rays]}
    runs = []
    for n_rays in args.rays:
        scene = make_scene()
        legs = [spec.Leg(k, scene, n_rays) for k in spec.legs]
        for leg in legs:
            leg.run(args.warmup)
        torch.cuda.synchronize()
        ms = {leg.kind: [] for leg in legs}
        for _ in range(args.windows):
            for leg in legs:
                ms[leg.kind].append(round(event_ms(lambda: leg.run(args.steps)) / args.steps, 4))
        out = {"rays": n_rays, "warmup": args.warmup, "steps": args.steps}
        for leg in legs:
            out[leg.kind] = {"ms_per_step_median": median(ms[leg.kind]), "windows": ms[leg.kind], "last_samples": int(leg.samples)}
        runs.append(out)
    return {"steps": runs}


# ---------------------------------------------------------------------------------------------- the recipes
class Spec:
    """what a recipe's row may say; the defaults are those of most rows"""
    legs = ("default", "module", "fused")
    protocol = staticmethod(run_process)
    scale = 0.5
    warmup = 64
    rays = dict(default=8192)        # --rays
    ground_truth = {}                # LegoProxy.ground_truth's keywords beside n_quad
    trainer_kw = {}                  # NGPTrainer's keywords of every leg, beside lr
    # run_alternate's:
    past_warmup = False              # refuses a --warmup short of the trainer's own warm-up
    entry_report = False             # reports the C entry calls of one step per leg
    warm_leg = "fused"               # the leg the warm-up trains

    def ngp(self, leg):
        """NGP's keywords beside scale"""
        return {}

    def targets(self, scene, img, pix, o, d, gt, gen):
        """-> (the colour target, step()'s keywords that carry the recipe's other targets)"""
        return gt, {}

    def plain(self, model, **kw):
        """the trainer and step of a leg without the recipe"""
        tr = NGPTrainer(model, lr=1e-2, **self.trainer_kw, **kw)
        return tr, lambda b: tr.step(*b[:3])

    def step(self, tr):
        """the step of a trainer with the recipe"""
        return lambda b: tr.step(*b[:3], **b[3])

    def report(self, tr, res):
        return {"fused_loss": tr.recipe.fused_loss}


def mono_depths(scene, o, d):
    """25 (0.37 D + 0.11) where the ray has a depth, 0 (invalid) elsewhere"""
    D = scene.ground_truth_depths(o, d, n_quad=64)
    return torch.where(D > 0, 25.0 * (0.37 * D + 0.11), torch.zeros_like(D)).contiguous()


class TailSpec(Spec):
    """a term of the fused render + loss tail (or all three).  module: NGPTrainer(loss_kwargs=...) with step(target=...):
    model(...), VolumeRenderer, RefLoss, the distortion pair and the NeRFLoss module as separate launches, exact gradient norm;
    the last leg: the trainer's own option with step(labels=, normals=, depths=), the fused field and the recipe's tail entry.
    --solo times the named tail entries alone on one marched batch of the scene at 2048 and 8192 rays"""
    TARGET = {"labels": "label", "normals": "normal", "depths": "depth"}   # step()'s keyword -> the key of target=
    classes = 7
    loss_kwargs = {}
    entries = ()                     # of TAIL_LAYOUT, timed by --solo
    counted = ()                     # the targets whose valid rays --solo reports

    def __init__(self, name, option):
        self.name, self.option = name, option

    def leg(self, leg, model):
        if leg == "default":
            return self.plain(model)
        if leg == "module":
            tr, _ = self.plain(model, loss_kwargs=self.loss_kwargs)
            return tr, lambda b: tr.step(*b[:3], target={self.TARGET[k]: v for k, v in b[3].items()})
        tr, _ = self.plain(model, **{self.name: self.option})
        return tr, self.step(tr)

    def report(self, tr, res):
        v = getattr(tr.recipe, self.name)
        return {"fused_loss": tr.recipe.fused_loss, self.name: list(v) if isinstance(v, tuple) else v}

    @torch.no_grad()
    def solo(self, args):
        """the tail entries on one marched batch of the scene's analytic occupancy, with random field outputs"""
        C = self.classes
        model, scene = make_model(self.scale, **self.ngp(None)), make_scene()
        model.density_grid.copy_(scene.occupancy_from_analytic(model))
        vren.packbits(model.density_grid.view(-1), 0.5, model.density_bitfield)
        gen = torch.Generator(device=DEV).manual_seed(7)
        out = {}
        for nr in (2048, 8192):
            img, pix = scene.sample_batch(nr, generator=gen)
            o, d = scene.rays(img, pix)
            _, t = self.targets(scene, img, pix, o, d, None, gen)
            hits_t = intersect_scene(model, o.contiguous(), d.contiguous())
            rays_a, xyzs, dirs, deltas, ts, _ = RayMarcher.apply(o, d, hits_t[:, 0], model.density_bitfield, model.cascades,
                                                                 model.scale, 0.0, model.grid_size, MAX_SAMPLES)
            n = xyzs.shape[0]
            R = lambda *s: torch.rand(*s, device=DEV, generator=gen)
            sig, rgbs, dsig, nrm, sem = R(n) * 40, R(n, 3), R(n, 3) - 0.5, R(n, 3) - 0.5, R(n, C) * 4 - 2
            gt = R(nr, 3)
            E = lambda *s: torch.empty(*s, device=DEV)
            total = torch.empty(nr, dtype=torch.int64, device=DEV)
            outs = (E(nr), E(nr), E(nr, 3), E(nr, 3), E(nr, C), E(n), E(nr), E(nr, 3))
            d_sig, d_rgb, d_sem, d_np = E(n), E(n, 3), E(n, C), E(n, 3)
            sem_a, nrm_a, dep_a = (t.get("labels"), 4e-2, 1e-1), (t.get("normals"), 1e-3), (t.get("depths"), 1.0, 0.5)
            out[f"samples_{nr}"] = n
            if "normals" in self.counted:
                out[f"rays_with_a_normal_{nr}"] = int((t["normals"] != 0).any(-1).sum())
            if "depths" in self.counted:
                out[f"rays_with_a_depth_{nr}"] = int((t["depths"] > 0).sum())
            head = (sig, rgbs, dsig, None, nrm, 3, sem, C, dirs, deltas, ts, rays_a, gt, None)
            for entry in self.entries:
                lay = TAIL_LAYOUT[entry]
                acc = E(lay.acc)
                own_ws = torch.empty(lay.ws_ints, dtype=torch.int32, device=DEV)      # (of the entry that keeps none in acc)
                own_in, grads = {"default": ((), ()), "sem": (sem_a, (d_sem,)), "nrm": (nrm_a, (d_np,)), "dep": (dep_a, ()),
                                 "multi": ((7,) + sem_a + nrm_a + dep_a, (d_sem, d_np))}[entry]
                name = "render_loss_fused" + ("" if entry == "default" else "_" + entry)

                def fn():   # slices the accumulator in the timed call, as rendering._RenderLossFn does in every step
                    wsp = () if not lay.ws_ints else (own_ws if lay.ws_at is None else acc[lay.ws_at:].view(torch.int32),)
                    call(name, *head, *own_in, 1e-4, C, nr, 2e-4, 3e-4, total, acc[lay.vr_at:lay.vr_at + 2].view(torch.int64),
                         *outs, acc[:lay.n_terms], d_sig, d_rgb, *wsp, *grads)
                out[f"{name}_us_{nr}"] = median_us(fn)
        return out


class Semantic(TailSpec):
    """the render_semantic recipe on the labelled scene (5 classes: four parts and sky; the labels are 0..4 or 256, the only
    values torch's cross-entropy takes here without a device assert), on ngp_render_loss_fused_sem"""
    classes = 5
    trainer_kw = {"num_classes": 5}
    loss_kwargs = {"semantic": True}
    entries = ("default", "sem")

    def ngp(self, leg):
        return {"classes": 5}

    def targets(self, scene, img, pix, o, d, gt, gen):
        return gt, {"labels": scene.ground_truth_labels(o, d, n_quad=64)}


class NormalMono(TailSpec):
    """the normal_mono recipe on the scene's analytic normals, on ngp_render_loss_fused_nrm"""
    loss_kwargs = {"normal_mono": True}
    entries = ("default", "nrm")
    counted = ("normals",)

    def targets(self, scene, img, pix, o, d, gt, gen):
        return gt, {"normals": scene.ground_truth_normals(o, d, n_quad=64).contiguous()}


class DepthMono(TailSpec):
    """the depth_mono recipe on the scene's depths as a monocular map, on ngp_render_loss_fused_dep (the fit kernel, then the
    tail); the module leg is compute_scale_and_shift's torch reductions, with a host read of the determinant in every step"""
    loss_kwargs = {"depth_mono": True, "scale": 0.5}
    entries = ("default", "dep")
    counted = ("depths",)

    def targets(self, scene, img, pix, o, d, gt, gen):
        return gt, {"depths": mono_depths(scene, o, d)}


class MultiTerms(TailSpec):
    """semantic + normal_mono + depth_mono together, on ngp_render_loss_fused_multi (the label count, the fit kernel, then the
    tail); --solo times it against ngp_render_loss_fused and the three single entries"""
    legs = ("default", "module", "multi")
    loss_kwargs = {"semantic": True, "normal_mono": True, "depth_mono": True, "scale": 0.5}
    entries = ("default", "sem", "nrm", "dep", "multi")
    counted = ("depths",)

    def targets(self, scene, img, pix, o, d, gt, gen):
        """the scene's labels (0-4, 256), its normals with a random direction where it has none (every target non-zero: where
        the module states the same loss) and its monocular depths"""
        lab = scene.ground_truth_labels(o, d, n_quad=64).to(torch.int64).contiguous()
        nrm = scene.ground_truth_normals(o, d, n_quad=64)
        rnd = torch.nn.functional.normalize(torch.randn(nrm.shape, device=DEV, generator=gen), dim=-1)
        nrm = torch.where((nrm != 0).any(-1, keepdim=True), nrm, rnd).contiguous()
        return gt, {"labels": lab, "normals": nrm, "depths": mono_depths(scene, o, d)}


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


class Masked(Spec):
    """the embed_msk recipe (scale 8, exponential stepping, random background).  layered: the route that needs no mask field in
    the package, a module assembled from tinycudann.Encoding + nn.Sequential with its own torch Adam, its output passed as
    mask= under loss_kwargs={'embed_msk': True} (the NeRFLoss module and torch autograd replace the fused tail, the exact norm
    the norm bound); fused: NGPTrainer(model, msk_model=implicit_mask()), ngp_mask_field_fwd / _bwd and the masked fused tail.
    --solo times the two mask kernels alone at 2048 and 8192 rows"""
    legs = ("default", "layered", "fused")
    scale = 8.0
    trainer_kw = dict(exp_step_factor=1 / 256, render_kwargs={"random_bg": True})

    def targets(self, scene, img, pix, o, d, gt, gen):
        return gt, {"uvi": implicit_mask.uvi(torch.stack([pix // WH, pix % WH], -1), img, (WH, WH), N_IMG)}

    def leg(self, leg, model):
        if leg == "default":
            return self.plain(model)
        if leg == "fused":
            tr, _ = self.plain(model, msk_model=implicit_mask().to(DEV))
            return tr, self.step(tr)
        msk = LayeredMask().to(DEV)
        opt = torch.optim.Adam(msk.parameters(), lr=1e-2, eps=1e-8)
        tr, _ = self.plain(model, loss_kwargs={"embed_msk": True})

        def step(b):
            opt.zero_grad(set_to_none=True)
            out = tr.step(*b[:3], mask=msk(b[3]["uvi"]), step=tr.global_step)
            opt.step()
            return out
        return tr, step

    def solo(self, args):
        msk = implicit_mask().to(DEV)
        l1, l2 = msk.mask_net[0], msk.mask_net[2]
        out = {}
        for n in (2048, 8192):
            uvi = torch.rand(n, 3, device=DEV) - 0.5
            mask, g = torch.empty(n, device=DEV), torch.randn(n, device=DEV)
            grads = [torch.zeros_like(p) for p in (msk.mask_encoder.params, l1.weight, l1.bias, l2.weight, l2.bias)]
            out[f"mask_field_fwd_us_{n}"] = median_us(lambda: call(
                "mask_field_fwd", msk.mask_encoder.desc, msk.mask_encoder.params, l1.weight, l1.bias, l2.weight, l2.bias, uvi, n,
                mask))
            out[f"mask_field_bwd_us_{n}"] = median_us(lambda: call(
                "mask_field_bwd", msk.mask_encoder.desc, msk.mask_encoder.params, l1.weight, l1.bias, l2.weight, uvi, mask, g, n,
                *grads))
        return out


class EmbedA(Spec):
    """the embed_a recipe (scale 8, exponential stepping, random background, E = 8).  none: the same recipe without appearance
    codes; tensor: the route that needs nothing of appearance.py, the codes an external nn.Parameter (n_imgs, E), indexed per
    ray and passed as embedding_a= (render() expands them per sample with torch operations, autograd sums their gradient),
    stepped by their own torch.optim.Adam(lr, eps=1e-8); fused: NGPTrainer(model, embedding_a=nn.Embedding), ngp_embed_a_fwd /
    _bwd, the table in the flat store.  The legs train different models, so their sample counts differ (samples_last_step).
    --solo times the two kernels alone on 8192 rays / about 440 k samples, with every ray of another image (all_images) and
    with all rays of one image (same_image)"""
    legs = ("none", "tensor", "fused")
    scale = 8.0
    trainer_kw = dict(exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    E = 8

    def ngp(self, leg):
        return {} if leg == "none" else {"embed_a": True, "embed_a_len": self.E}

    def targets(self, scene, img, pix, o, d, gt, gen):
        return gt, {"img_idxs": img.to(torch.int64).contiguous()}

    def leg(self, leg, model):
        emb = torch.nn.Embedding(N_IMG, self.E).to(DEV)
        if leg == "none":
            return self.plain(model)
        if leg == "fused":
            tr, _ = self.plain(model, embedding_a=emb)
            return tr, self.step(tr)
        codes = torch.nn.Parameter(emb.weight.detach().clone())
        opt = torch.optim.Adam([codes], lr=1e-2, eps=1e-8)
        tr, plain = self.plain(model)

        def step(b):
            opt.zero_grad(set_to_none=True)
            tr.render_kwargs["embedding_a"] = codes[b[3]["img_idxs"]]
            out = plain(b)
            opt.step()
            return out
        return tr, step

    def report(self, tr, res):
        return {"samples_last_step": int(res["total_samples"]), "fused_loss": tr.recipe.fused_loss}

    def solo(self, args):
        n_rays, n_imgs, Kp, E = 8192, 100, 160, self.E
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
                us = timed_us(fn)
                out[f"embed_a_{name}_us_{tag}"] = {"median": round(median(us), 2), "min": round(us[0], 2), "max": round(us[-1], 2)}
        return out


class Alternated(Spec):
    """three legs on one trainer: default, the default recipe; module, the launch-per-operation route; fused, the trainer's
    own option"""
    protocol = staticmethod(run_alternate)
    warmup = 320
    past_warmup = True
    entry_report = True

    def report(self, tr, res):
        return {}


class Skybox(Alternated):
    """the skybox recipe on the scene composited over the analytic sky; the skybox joins at step 256.  default: no skybox in
    the step (the model's skybox network idles); module: render_kwargs={'use_skybox': True} (model(...), VolumeRenderer,
    forward_skybox module by module, RefLoss, nerf_loss_and_grads, the distortion pair, composite_train_bw); fused:
    NGPTrainer(use_skybox=True), ngp_skybox_fwd, ngp_render_loss_fused_sky, ngp_skybox_bwd.  --solo times the two sky kernels
    alone at --rays rays, and ngp_render_loss_fused_sky against ngp_render_loss_fused on the same marched batch"""
    ground_truth = {"sky": True}

    def ngp(self, leg):
        return {"use_skybox": True}

    def trainer(self, model):
        return NGPTrainer(model, lr=1e-2, use_skybox=True)

    def set_leg(self, tr, leg):
        tr.recipe.use_skybox = leg == "fused"
        tr.render_kwargs = {"use_skybox": True} if leg == "module" else {}

    def solo(self, args, model, tr, batch, samples):
        d = torch.randn(args.rays, 3, device=DEV)
        g = torch.randn(args.rays, 3, device=DEV)
        out = {"rays": args.rays}
        for leg, fwd in (("module", model.forward_skybox), ("fused", model.skybox_rgb)):
            fwd_bwd_us(out, f"sky_{leg}", lambda: fwd(d), g)
        # the two tail entries on the arguments of one step of this trainer (captured from the step itself)
        _lib.CAPTURE = {"render_loss_fused": [], "render_loss_fused_sky": []}
        for leg in ("default", "fused"):
            self.set_leg(tr, leg)
            self.step(tr)(batch)
        torch.cuda.synchronize()
        cap, _lib.CAPTURE = _lib.CAPTURE, None
        for name, calls in cap.items():
            a = calls[-1]
            out[f"{name}_us"] = median_us(lambda: call(name, *a))
        out["samples"] = int(cap["render_loss_fused_sky"][-1][0].shape[0])
        return out


class NormalRef(Alternated):
    """the normal_ref recipe; the warm-up trains the default recipe.  module: loss_kwargs={'normal_ref': True} (differentiable
    normals by create_graph=True, the density MLP's second order on torch ops, VolumeRenderer, _RefLossInputs, RefLoss, the
    NeRFLoss module); fused: NGPTrainer(normal_ref=True), the fused field node with second-order normals
    (ngp_grid_bwd_bwd_input, ngp_density_head_bwd2 and four products), the fused tail and ngp_normal_ref_tail.  --solo times,
    on the arguments of one fused step, ngp_density_head_bwd2, ngp_normal_ref_tail and the whole second-order share of
    _FieldFn.backward: the seven entry calls from ngp_grid_bwd_bwd_input to the density table's ngp_grid_bwd_param, one behind
    the other, and each of them alone"""
    warm_leg = "default"
    SHARE = [("grid_bwd_bwd_input", 0), ("linear_fwd", 0), ("density_head_bwd2", 0), ("linear_bwd_weight", 0),
             ("linear_bwd_weight", 1), ("linear_bwd_input", 0), ("grid_bwd_param", 0)]

    def trainer(self, model):
        return NGPTrainer(model, lr=1e-2, normal_ref=True)

    def set_leg(self, tr, leg):
        tr.recipe.normal_ref = leg == "fused"
        tr.model.second_order_normals = leg == "fused"
        tr.model.differentiable_normals = leg == "module"
        tr.loss_kwargs = {"normal_ref": True} if leg == "module" else {}
        tr.recipe.fused_loss = leg != "module"

    def solo(self, args, model, tr, batch, samples):
        self.set_leg(tr, "fused")
        step = self.step(tr)
        step(batch)
        _lib.CAPTURE = {name: [] for name in dict(self.SHARE)} | {"normal_ref_tail": []}
        step(batch)
        tr.wait()
        torch.cuda.synchronize()
        cap, _lib.CAPTURE = _lib.CAPTURE, None
        xe = model.xyz_encoder.desc
        cap["grid_bwd_param"] = [a for a in cap["grid_bwd_param"] if a[0] is xe]      # (the colour table's scatter is the other one)
        counts = {name: len(v) for name, v in cap.items()}
        if counts != {"grid_bwd_bwd_input": 1, "linear_fwd": 1, "density_head_bwd2": 1, "linear_bwd_weight": 2,
                      "linear_bwd_input": 1, "grid_bwd_param": 1, "normal_ref_tail": 1}:
            raise SystemExit(f"a fused step's second-order share is not the seven calls this tool replays: {counts}")
        out = {"rays": int(batch[0].shape[0]), "samples": int(cap["density_head_bwd2"][0][5])}
        for k, (name, i) in enumerate(self.SHARE):
            a = cap[name][i]
            out[f"share_{k}_{name}_us"] = median_us(lambda: call(name, *a))
        out["second_order_share_us"] = median_us(lambda: [call(name, *cap[name][i]) for name, i in self.SHARE])
        out["density_head_bwd2_us"] = out["share_2_density_head_bwd2_us"]
        tail = cap["normal_ref_tail"][0]
        out["normal_ref_tail_us"] = median_us(lambda: call("normal_ref_tail", *tail))
        tr.flat_grad.zero_()          # (the replays added to the gradient sinks)
        return out


def layered_tonemap(self, log_radiances, **kwargs):
    """the tone-mapper module by module"""
    out = []
    for i in range(3):
        inp = log_radiances[:, i:i + 1]
        if 'exposure' in kwargs:
            inp = inp + torch.log(kwargs['exposure'])
        out.append(getattr(self, f'tonemapper_net_{i}')(inp))
    return torch.cat(out, 1)


class Exposure(Spec):
    """the HDR-NeRF recipe on the scene shown at five exposure times, two legs on one trainer.  layered: the launch-per-operation
    tone-mapper, the three tonemapper_net_i modules composed as NGP.log_radiance_to_rgb composed them before the fused
    kernels (slice, add of ln(exposure), ones-padding, two linear launches a channel forward; act_bwd, linear_bwd_weight,
    linear_bwd_input per layer backward); fused: ngp_tonemap_fwd / ngp_tonemap_bwd (networks._ToneMapFn).  --solo times both
    routes of the tone-mapper alone, forward and backward, at the sample count of a steady-state batch (read from a step after
    the warm-up)"""
    legs = ("layered", "fused")
    protocol = staticmethod(run_alternate)

    def ngp(self, leg):
        return {"rgb_act": "None"}

    def targets(self, scene, img, pix, o, d, gt, gen):
        times = torch.tensor(list(_HDR_EXPOSURES["chair"].values()), device=DEV)
        c = (1.0 - HDR_UNIT_EXPOSURE_RGB) / HDR_UNIT_EXPOSURE_RGB
        e = times[torch.randint(5, (gt.shape[0], 1), device=DEV, generator=gen)]
        x = gt * e
        return x / (x + c), {"exposure": e.contiguous()}     # export.hdr_response on the device

    def trainer(self, model):
        return NGPTrainer(model, lr=1e-2, use_exposure=True, unit_exposure_rgb=HDR_UNIT_EXPOSURE_RGB)

    def set_leg(self, tr, leg):
        if leg == "layered":
            tr.model.log_radiance_to_rgb = types.MethodType(layered_tonemap, tr.model)
        elif "log_radiance_to_rgb" in tr.model.__dict__:
            del tr.model.log_radiance_to_rgb

    def solo(self, args, model, tr, batch, n):
        lr = (torch.rand(n, 3, device=DEV) * 12 - 6).requires_grad_(True)
        e = torch.tensor(list(_HDR_EXPOSURES["chair"].values()), device=DEV)[torch.randint(5, (n, 1), device=DEV)]
        g = torch.randn(n, 3, device=DEV)
        out = {"samples": n}
        for leg in self.legs:
            self.set_leg(tr, leg)
            fwd_bwd_us(out, leg, lambda: model.log_radiance_to_rgb(lr, exposure=e), g)
        self.set_leg(tr, "fused")
        return out


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


class PoseLeg:
    """one leg of the pose recipe: its own model from the same seed, trained on batches it draws itself"""

    def __init__(self, kind, scene, n_rays):
        self.kind, self.scene, self.n_rays = kind, scene, n_rays
        self.model = make_model()
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

    def run(self, steps):
        for _ in range(steps):
            self.step()
        self.tr.wait()


class Pose(Spec):
    """pose refinement (optimize_ext).  none trains with the dataset's rays (no refiner: the default step); torch forms the
    rays and ties the samples to dR, dT with torch operations (axisangle_to_R, get_rays, repeat_interleave, indexing; their
    autograd chain is the adjoint); kernels is pose.PoseRefiner.  Both pose legs run NGPTrainer's pose step and the field's
    dL/dx and dL/dd routes, so the difference between them is the ray / pose part alone.  --solo times ngp_pose_rays_fwd / _bwd
    and ngp_sh_bwd_dirs alone on the samples of one marched batch of the model after 320 steps"""
    legs = ("none", "torch", "kernels")
    protocol = staticmethod(run_models)
    warmup = 320
    rays = dict(nargs="+", default=[2048, 8192])
    Leg = PoseLeg

    def solo(self, args, n_rays):
        scene = make_scene()
        leg = PoseLeg("kernels", scene, n_rays)
        leg.run(320)
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
            out[pattern] = {"samples": n, **{name + "_us_median": median_us(fn, warm=5) for name, fn in jobs.items()}}
        return out


SPECS = {   # recipe.Recipe's option fields
    "semantic": Semantic("semantic", True),
    "normal_mono": NormalMono("normal_mono", True),
    "depth_mono": DepthMono("depth_mono", True),
    "multi_terms": MultiTerms("multi_terms", ("semantic", "normal_mono", "depth_mono")),
    "use_exposure": Exposure(),
    "use_skybox": Skybox(),
    "normal_ref": NormalRef(),
    "masked": Masked(),
    "embed_a": EmbedA(),
    "pose": Pose(),
}


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="recipe", required=True, metavar="recipe", help=" | ".join(SPECS))
    for name, spec in SPECS.items():
        one = spec.protocol is run_process
        doc = [inspect.cleandoc(c.__doc__) for c in (type(spec), TailSpec, Alternated) if isinstance(spec, c)]
        if not one:
            doc.append("legs, alternated window by window: {" + ",".join(spec.legs) + "}")
        p = sub.add_parser(name, formatter_class=argparse.RawDescriptionHelpFormatter, description="\n\n".join(doc))
        if one:
            p.add_argument("--leg", choices=spec.legs, default=spec.legs[-1])
        p.add_argument("--rays", type=int, **spec.rays)
        p.add_argument("--steps", type=int, default=40, help="steps per window")
        p.add_argument("--warmup", type=int, default=spec.warmup, help="steps before the first window")
        p.add_argument("--windows", type=int, default=5, help="windows" if one else "windows per leg")
        p.add_argument("--solo", action="store_true")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    spec = SPECS[args.recipe]
    print(json.dumps(spec.protocol(spec, args)))


if __name__ == "__main__":
    main()
