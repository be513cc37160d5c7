#!/usr/bin/env python3
"""Trains on a scene directory with the reference's recipe and evaluates the test split (what
`python train.py --root_dir ... --dataset_name nerf|nsvf|colmap|tnt|nerfpp` + validation do in the
reference: train.py:82-392).  GPU only.

  python tools/train_dataset.py --root_dir /data/nerf_synthetic/lego --num_epochs 20
  python tools/train_dataset.py --root_dir /data/tnt/Playground --dataset_name tnt --scale 8 --exp_step_factor 0.00390625
  python tools/train_dataset.py --make_proxy /tmp/proxy --downsample 0.25 --num_epochs 2   # no dataset at hand
  python tools/train_dataset.py --root_dir /data/tnt/Playground --dataset_name tnt --scale 8 --exp_step_factor 0.00390625 \
      --random_bg --embed_msk --save_dir out --ckpt_path out/playground.ckpt   # transient mask: out/mask_NNN.png per image
  python tools/train_dataset.py --root_dir /data/tnt/Playground --dataset_name tnt --scale 8 --exp_step_factor 0.00390625 \
      --random_bg --embed_a --embed_a_len 8 --embed_msk --ckpt_path out/playground.ckpt   # the reference's Playground recipe
  python tools/train_dataset.py --make_proxy /tmp/proxy --downsample 0.125 --num_epochs 2 --optimize_ext --pose_lr 1e-4 \
      --perturb_poses 0.02 0.5 --ckpt_path out/poses.ckpt   # pose refinement from perturbed poses: errors before / after
  python tools/train_dataset.py --make_proxy /tmp/proxy_sem --dataset_name tnt --downsample 0.125 --num_epochs 2 \
      --render_semantic --num_classes 5 --ckpt_path out/sem.ckpt   # semantic head on the labelled proxy: accuracy, mIoU
      # (--scale must enclose the cameras, here it defaults to 2: the sky term puts density at the far end of the volume on rays labelled 4)
  python tools/train_dataset.py --make_proxy /tmp/proxy_nrm --dataset_name tnt --downsample 0.125 --num_epochs 2 \
      --normal_mono --ckpt_path out/nrm.ckpt   # normal head on the proxy's analytic normal maps: held-out angle in degrees
  python tools/train_dataset.py --make_proxy /tmp/proxy_dep --dataset_name tnt --downsample 0.125 --num_epochs 2 \
      --depth_mono --ckpt_path out/dep.ckpt   # depth_mono term on the proxy's depth maps (right up to scale and shift): held-out abs-rel
  python tools/train_dataset.py --make_proxy /tmp/proxy_all --dataset_name tnt --downsample 0.125 --num_epochs 2 \
      --multi_terms semantic normal_mono depth_mono --num_classes 5   # the three terms together on one fused tail
  python tools/train_dataset.py --make_proxy /tmp/proxy_hdr --dataset_name colmap --downsample 0.1 --num_epochs 3 \
      --steps_per_epoch 200 --use_exposure   # HDR-NeRF recipe on the multi-exposure proxy: held-out PSNR at unseen exposures
  python tools/train_dataset.py --make_proxy /tmp/proxy_sky --dataset_name tnt --downsample 0.125 --num_epochs 3 \
      --steps_per_epoch 200 --use_skybox --ckpt_path out/sky.ckpt   # skybox recipe on the proxy over the analytic sky: held-out
      # PSNR, and test_sky_psnr over the held-out pixels that see only sky
  python tools/train_dataset.py --make_proxy /tmp/proxy_ref --dataset_name tnt --downsample 0.1 --proxy_views 34 \
      --num_epochs 3 --steps_per_epoch 200 --batch_size 2048 --normal_ref   # normal_ref terms on the fused field and tail:
      # held-out PSNR, and test_normal_agree_deg_mean between the predicted and the density normals
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngp_amd  # noqa: F401
from ngp_amd import ckpt
from ngp_amd.appearance import FrameEmbedding
from ngp_amd.datasets import dataset_dict, write_synthetic_dataset
from ngp_amd.evaluation import depth_summary, evaluate_split, normal_summary, semantic_summary
from ngp_amd.implicit_mask import implicit_mask
from ngp_amd.metrics import psnr
from ngp_amd.networks import NGP
from ngp_amd.pose import PoseRefiner, perturb_poses, pose_errors
from ngp_amd.recipe import conflicts
from ngp_amd.rendering import MULTI_TERMS
from ngp_amd.trainer import NGPTrainer


def build_model(scale, device, embed_a=False, embed_a_len=4, num_classes=7, use_exposure=False, use_skybox=False):
    more = dict(embed_a=True, embed_a_len=embed_a_len) if embed_a else {}
    if use_skybox:   # skybox_dir_encoder and skybox_rgb_net (train.py:97)
        more["use_skybox"] = True
    if use_exposure:   # log-radiance and the three tone-mappers (train.py:99)
        more["rgb_act"] = "None"
    model = NGP(scale=scale, classes=num_classes, **more).to(device).add_occupancy_grid()
    return model


def labels_of_split(ds):
    """makes ds.labels[k] the label image of ds's k-th image.  The tnt loader reads the labels of its split; the colmap
    loader, as upstream, reads those of ALL registered frames while rays and poses are cut to the split (train: frame
    i with i % 8 != 0, test: i % 8 == 0), so BaseDataset would pair image k of the split with the labels of frame k.  Here
    the rows of the split's frames are kept; any other mismatch is an error.  Idempotent."""
    n_img, n_lab = len(ds.poses), ds.labels.shape[0]
    if n_lab == n_img:
        return ds
    keep = None
    if type(ds).__name__ == "ColmapDataset" and ds.split in ("train", "test") and "HDR-NeRF" not in ds.root_dir:
        keep = [i for i in range(n_lab) if (i % 8 != 0) == (ds.split == "train")]
    if keep is None or len(keep) != n_img:
        raise ValueError(f"{n_lab} label images for the {n_img} images of the {ds.split} split: cannot tell which belongs to which")
    ds.labels = ds.labels[torch.as_tensor(keep, device=ds.labels.device)].contiguous()
    return ds


def cameras_outside(train_set, scale):
    """largest |coordinate| of a training camera if it lies outside the model's volume [-scale, scale]^3, else None"""
    far = float(torch.as_tensor(train_set.poses)[:, :, 3].abs().max())
    return far if far > scale else None


def train(model, train_set, num_epochs, steps_per_epoch, batch_size, lr, log_every=0, exp_step_factor=0.0,
          render_kwargs=None, msk_model=None, embedding_a=None, pose_refiner=None, pose_lr=1e-6, semantic=False,
          num_classes=7, normal_mono=False, lambda_normal_mono=None, depth_mono=False, lambda_depth_mono=None,
          multi_terms=(), use_exposure=False, use_skybox=False, normal_ref=False):
    """the reference's schedule (NGPTrainer) fed by the dataset's own sampler, one batch ahead; msk_model: the transient
    mask field of --embed_msk, fed with the sampler's pixel coordinates and image indices; embedding_a: the appearance
    table of --embed_a, fed with the sampler's image indices; pose_refiner: the per-image corrections of --optimize_ext, fed
    with the sampler's image and pixel indices (the trainer then forms the rays itself, and nothing is marched ahead);
    semantic: the semantic head of --render_semantic, fed with the sampler's labels (num_classes of them); normal_mono:
    the normal head of --normal_mono, fed with the sampler's normals (lambda_normal_mono: the term's weight instead of
    NeRFLoss's 1e-3); depth_mono: the depth_mono term of --depth_mono, fed with the sampler's depths (lambda_depth_mono: the
    term's weight instead of NeRFLoss's 1); the trainer then carries `terms_log`, the loss terms of every step as device
    tensors (read after the run: nothing is read while it trains); multi_terms: the terms of --multi_terms, together on one
    tail (NGPTrainer(multi_terms=...)): the sampler feeds each named term as its own flag would, and `terms_log` holds the
    8 terms of every step; use_exposure: the HDR-NeRF recipe of --use_exposure, fed with the sampler's exposure times and the
    dataset's unit_exposure_rgb (`terms_log` then holds the 5 terms of every step); use_skybox: the skybox recipe of
    --use_skybox (NGPTrainer(use_skybox=True): the skybox joins from the end of the warm-up on); normal_ref: the normal_ref
    terms of --normal_ref (NGPTrainer(normal_ref=True), alone or with multi_terms): `terms_log` then holds the 6 (with
    multi_terms 10) terms of every step, the two ref terms last"""
    train_set.batch_size = batch_size
    multi_terms = tuple(multi_terms or ())
    if multi_terms and (semantic or normal_mono or depth_mono):
        raise ValueError("multi_terms names the terms itself: not together with semantic, normal_mono or depth_mono")
    semantic = semantic or "semantic" in multi_terms
    normal_mono = normal_mono or "normal_mono" in multi_terms
    depth_mono = depth_mono or "depth_mono" in multi_terms
    if depth_mono:
        if not hasattr(train_set, "depths_2d"):
            raise ValueError("--depth_mono needs per-pixel depths: the dataset has none (the tnt layout reads depth/*.npy "
                             "when loaded with depth_mono=True)")
        dev = next(model.parameters()).device
        train_set.depths_2d = train_set.depths_2d.to(dev)   # the sampler indexes them where the pixel indices are drawn
    if normal_mono:
        if not hasattr(train_set, "normals"):
            raise ValueError("--normal_mono needs per-pixel normals: the dataset has none (the tnt layout reads "
                             "normal/*.npy when loaded with normal_mono=True)")
        dev = next(model.parameters()).device
        train_set.normals = train_set.normals.to(dev)   # the sampler indexes them where the pixel indices are drawn
    if semantic:
        if not hasattr(train_set, "labels"):
            raise ValueError("--render_semantic needs per-pixel labels: the dataset has none (tnt / colmap layouts read "
                             "semantic/*.pgm when loaded with use_sem=True)")
        labels_of_split(train_set)
        dev = next(model.parameters()).device
        train_set.labels = train_set.labels.to(dev)   # the sampler indexes them where the pixel indices are drawn
    more = {} if embedding_a is None else {"embedding_a": embedding_a}
    if pose_refiner is not None:
        more.update(pose_refiner=pose_refiner, pose_lr=pose_lr)
    if semantic or num_classes != 7:
        more.update(num_classes=num_classes)
    if use_exposure:
        if train_set.rays.shape[-1] != 4:
            raise ValueError("--use_exposure needs an exposure time per ray: the dataset has none (the colmap loader reads "
                             "them for the HDR-NeRF layouts)")
        more.update(use_exposure=True, unit_exposure_rgb=train_set.unit_exposure_rgb)
    more.update(use_skybox=use_skybox, normal_ref=normal_ref, multi_terms=multi_terms)
    if not multi_terms:
        more.update(semantic=semantic, normal_mono=normal_mono, depth_mono=depth_mono)
    trainer = NGPTrainer(model, lr=lr, num_epochs=num_epochs, steps_per_epoch=steps_per_epoch,
                         exp_step_factor=exp_step_factor, render_kwargs=render_kwargs, msk_model=msk_model, **more)
    if lambda_normal_mono is not None:
        trainer.loss_fn.lambda_normal_mono = float(lambda_normal_mono)
    if lambda_depth_mono is not None:
        trainer.loss_fn.lambda_depth_mono = float(lambda_depth_mono)
    trainer.terms_log = []
    n_imgs = len(train_set.poses)

    def next_batch():
        s = train_set[0]
        if pose_refiner is not None:
            idx = torch.as_tensor(s["img_idxs"], device=s["rgb"].device).to(torch.int64).reshape(-1)
            idx = idx.expand(s["rgb"].shape[0]).contiguous()
            uvi = None
            if msk_model is not None:
                uvi = implicit_mask.uvi(s["uv"], s["img_idxs"], train_set.img_wh, n_imgs).to(idx.device)
            return None, None, s["rgb"].contiguous(), uvi, idx, s["pix_idxs"].to(torch.int64).contiguous(), None, None, None, None
        o, d = train_set.batch_rays(s)
        uvi = None
        if msk_model is not None:
            uvi = implicit_mask.uvi(s["uv"], s["img_idxs"], train_set.img_wh, n_imgs).to(o.device)
        idx = None
        if embedding_a is not None:   # one index per ray (the same_image strategy draws ONE image per batch)
            idx = torch.as_tensor(s["img_idxs"], device=o.device).to(torch.int64).reshape(-1).expand(o.shape[0]).contiguous()
        lab = s["label"].to(o.device, torch.int64).contiguous() if semantic else None
        nrm = s["normal"].to(o.device, torch.float32).contiguous() if normal_mono else None
        dep = s["depth"].to(o.device, torch.float32).reshape(-1).contiguous() if depth_mono else None
        exp = s["exposure"].to(o.device, torch.float32).contiguous() if use_exposure else None
        return o.contiguous(), d.contiguous(), s["rgb"].contiguous(), uvi, idx, None, lab, nrm, dep, exp

    import gc
    gc.collect()
    gc.freeze()   # model, dataset and trainer live for the whole run: keep full collections cheap
    cur = next_batch()
    total = num_epochs * steps_per_epoch
    t0 = time.perf_counter()
    for i in range(total):
        nxt = next_batch() if i + 1 < total else None
        more = {k: v for k, v in zip(("img_idxs", "pix_idxs", "labels", "normals", "depths", "exposure"), cur[4:]) if v is not None}
        ahead = None if nxt is None or pose_refiner is not None else nxt[:2]
        loss, res = trainer.step(*cur[:3], next_rays=ahead, uvi=cur[3], **more)
        if depth_mono or multi_terms or use_exposure or normal_ref:
            trainer.terms_log.append(res["loss_terms"])
        if log_every and (i + 1) % log_every == 0:
            torch.cuda.synchronize()
            print(json.dumps({"step": i + 1, "loss": float(loss), "train_psnr": float(psnr(res["rgb"].detach(), cur[2])),
                              "rays_per_s": batch_size * (i + 1) / (time.perf_counter() - t0)}), flush=True)
        cur = nxt
    trainer.wait()
    return trainer


def _save_rgb(save_dir, img_wh):
    """on_image callback of evaluate_split: writes each clamped rgb image as <save_dir>/NNN.png"""
    w, h = img_wh

    def save(i, rgb, results):
        from PIL import Image
        os.makedirs(save_dir, exist_ok=True)
        Image.fromarray((rgb.reshape(h, w, 3).cpu().numpy() * 255 + 0.5).astype("uint8")).save(
            os.path.join(save_dir, f"{i:03d}.png"))
    return save


@torch.no_grad()
def mask_images(msk_model, img_wh, n_imgs, device, save_dir=None, chunk=131072):
    """the mask field over every pixel of every training image, in chunks -> mean mask of each image; with save_dir
    also <save_dir>/mask_NNN.png = (uint8)(clip(mask, 0, 1) * 255), so that one can see what was masked"""
    w, h = img_wh
    pix = torch.arange(w * h, device=device)
    uv = torch.stack([pix // w, pix % w], -1)
    means = []
    for i in range(n_imgs):
        parts = []
        for a in range(0, w * h, chunk):
            idx = torch.full((min(chunk, w * h - a),), i, device=device)
            parts.append(msk_model(implicit_mask.uvi(uv[a:a + chunk], idx, img_wh, n_imgs))[:, 0])
        m = torch.cat(parts)
        means.append(float(m.mean()))
        if save_dir:
            from PIL import Image
            os.makedirs(save_dir, exist_ok=True)
            Image.fromarray((m.clamp(0, 1) * 255).to(torch.uint8).reshape(h, w).cpu().numpy()).save(
                os.path.join(save_dir, f"mask_{i:03d}.png"))
    return means


def evaluate(model, test_set, chunk=131072, save_dir=None, exp_step_factor=0.0):
    """per-image PSNR of the test split through render(test_time=True) (train.py:347-392)"""
    return evaluate_split(model, test_set, chunk, on_image=_save_rgb(save_dir, test_set.img_wh) if save_dir else None,
                          exp_step_factor=exp_step_factor)["psnr"]


# flag -> the trainer's option (or the condition of recipe.py) it stands for
FLAG_OPTIONS = dict({f: f for f in ("use_exposure", "normal_mono", "depth_mono", "multi_terms", "use_skybox", "normal_ref")},
                    embed_msk="msk_model", optimize_ext="pose_refiner", render_semantic="semantic")
# flag -> (the --dataset_name layouts --make_proxy can write its scene in, what that scene is)
PROXY_LAYOUTS = {
    "normal_ref": (("tnt",), "the scene in the tnt layout"),
    "multi_terms": (("tnt",), "a scene with labels, normal and depth maps (the layout that carries all three)"),
    "depth_mono": (("tnt",), "a scene with depth maps (the layout that carries depth/*.npy)"),
    "normal_mono": (("tnt",), "a scene with normal maps (the layout that carries normal/*.npy)"),
    "use_skybox": (("tnt",), "the scene over the analytic sky (the layout whose images carry their background)"),
    "use_exposure": (("colmap",), "the HDR-NeRF synthetic layout (the loader that reads it)"),
    "render_semantic": (("tnt", "colmap"), "a labelled scene (the layouts that carry semantic/*.pgm)"),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir")
    ap.add_argument("--dataset_name", default="nerf", choices=sorted(dataset_dict))
    ap.add_argument("--make_proxy", help="write the analytic lego-proxy scene to this directory first and train on it")
    ap.add_argument("--downsample", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=None,
                    help="half-width of the model's volume; default 0.5, and 2 with --make_proxy --render_semantic (the "
                         "exported cameras sit at radius 0.83 and the sky term needs them inside the volume)")
    ap.add_argument("--exp_step_factor", type=float, default=0.0, help="1/256 for unbounded scenes (opt.py)")
    ap.add_argument("--random_bg", action="store_true")
    ap.add_argument("--embed_msk", action="store_true",
                    help="train the transient mask field beside the scene (the reference's --embed_msk)")
    ap.add_argument("--embed_a", action="store_true",
                    help="train one appearance code per training image (the reference's --embed_a); the test split is "
                         "evaluated with the code of image 0")
    ap.add_argument("--embed_a_len", type=int, default=4, help="length of an appearance code, 1 to 32")
    ap.add_argument("--optimize_ext", action="store_true",
                    help="train a per-image rotation dR and translation dT beside the scene (the reference's --optimize_ext); "
                         "the test split is rendered with the dataset's test poses")
    ap.add_argument("--pose_lr", type=float, default=1e-6, help="constant learning rate of dR, dT (the reference's 1e-6)")
    ap.add_argument("--perturb_poses", type=float, nargs=2, metavar=("SIGMA_T", "DEG"),
                    help="with --optimize_ext: start from training poses translated by N(0, SIGMA_T^2) per axis and rotated by "
                         "DEG degrees about random axes (seeded); the JSON line reports the pose errors before and after")
    ap.add_argument("--batch_size", type=int, default=8192)
    ap.add_argument("--num_epochs", type=int, default=20)
    ap.add_argument("--steps_per_epoch", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--save_dir")
    ap.add_argument("--ckpt_path")
    ap.add_argument("--render_semantic", action="store_true",
                    help="load per-pixel labels (semantic/*.pgm, use_sem=True) and train the semantic head on them (the "
                         "reference's --render_semantic); the JSON line gains test_sem_acc_mean and test_sem_miou_mean.  "
                         "Choose --scale so that the volume encloses the cameras: the sky term rewards depth on rays labelled 4")
    ap.add_argument("--num_classes", type=int, default=7, help="classes of the semantic head, 1 to 16")
    ap.add_argument("--normal_mono", action="store_true",
                    help="load per-pixel normal maps (normal/*.npy of the tnt layout) and train the predicted-normal head on "
                         "them (the reference's --normal_mono); the JSON line gains test_normal_deg_mean")
    ap.add_argument("--depth_mono", action="store_true",
                    help="load per-pixel monocular depth maps (depth/*.npy of the tnt layout) and train with NeRFLoss's "
                         "depth_mono term (the reference's --depth_mono); the JSON line gains test_depth_absrel_mean")
    ap.add_argument("--lambda_depth_mono", type=float, default=None, help="weight of the depth_mono term (NeRFLoss: 1)")
    ap.add_argument("--multi_terms", nargs="+", choices=MULTI_TERMS, default=(),
                    help="train several of the semantic, normal_mono and depth_mono terms together on one fused tail "
                         "(the reference's street-scene recipes set --render_semantic and --normal_mono together and add "
                         "depth_mono): each named term loads its maps and reports its metrics as its own flag does; the "
                         "JSON line gains loss_terms (8) and every optional term's mean over the first and last ten steps")
    ap.add_argument("--use_exposure", action="store_true",
                    help="the reference's HDR-NeRF recipe (--use_exposure): a model with rgb_act='None' and three tone-mappers, "
                         "fed with the exposure time of every ray (the colmap loader reads them for the HDR-NeRF layouts) and "
                         "regularised at unit exposure; the test split is rendered at each image's own exposure.  The JSON line "
                         "gains unit_exposure_rgb_pred and the term's mean over the first and last ten steps.  With "
                         "--make_proxy DIR --dataset_name colmap the multi-exposure proxy goes to DIR/HDR-NeRF/syndata/chair")
    ap.add_argument("--use_skybox", action="store_true",
                    help="the reference's skybox recipe (--use_skybox): a model with the skybox network, which colours the "
                         "background by view direction from the end of the warm-up on; the test split is rendered with it.  With "
                         "--make_proxy DIR --dataset_name tnt the proxy is written over the analytic sky, with the opacity of "
                         "every pixel in opacity/*.npy.  Whenever the scene directory has those, the JSON line gains "
                         "test_sky_psnr, the PSNR over the held-out pixels whose opacity is below 0.01")
    ap.add_argument("--proxy_views", type=int, default=108, help="views of the scene --make_proxy writes")
    ap.add_argument("--normal_ref", action="store_true",
                    help="the reference's normal_ref terms (--normal_ref: Ref-NeRF's Rp and Ro regularisers) on the fused field "
                         "node and the fused tail (NGPTrainer(normal_ref=True)); alone or with --multi_terms, --embed_a and "
                         "--random_bg.  The JSON line gains the two terms' means over the first and the last ten steps and "
                         "test_normal_agree_deg_mean, the mean angle over the held-out pixels with opacity above 0.5 "
                         "between the rendered predicted normal and the rendered density normal")
    args = ap.parse_args(argv)
    args.multi_terms = tuple(t for t in MULTI_TERMS if t in args.multi_terms)
    # what combines is the trainer's to say (recipe.py's table): everything goes with --embed_a and --random_bg
    given = {opt: "--" + flag for flag, opt in FLAG_OPTIONS.items() if getattr(args, flag)}
    for opt, refused in conflicts(given):
        ap.error(f"{given[opt]} does not combine with {given[refused]}")
    for flag, (layouts, what) in PROXY_LAYOUTS.items():
        if args.make_proxy and getattr(args, flag) and args.dataset_name not in layouts:
            ap.error(f"--make_proxy with --{flag} writes {what}: --dataset_name {' or '.join(layouts)}")
    if not 1 <= args.num_classes <= 16:
        ap.error("--num_classes must lie in [1, 16]")
    if args.scale is None:
        args.scale = 2.0 if args.make_proxy and (args.render_semantic or "semantic" in args.multi_terms) else 0.5
    if not 1 <= args.embed_a_len <= 32:
        ap.error("--embed_a_len must lie in [1, 32]")
    if args.perturb_poses and not args.optimize_ext:
        ap.error("--perturb_poses needs --optimize_ext")
    return args


def make_labelled_proxy(root, fmt, scene, n_quad=256):
    """the analytic proxy with per-pixel labels in the tnt or colmap layout, every 8th view held out"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=n_quad)
    labels = export.render_scene_labels(scene, range(n), n_quad=n_quad)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    if fmt == "colmap":
        return export.export_colmap(root, images, c2w, K, labels=labels)
    return export.export_tnt(root, images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)], labels=labels)


def make_proxy_with_normals(root, scene, n_quad=256):
    """the analytic proxy with per-pixel world-space normals in the tnt layout, every 8th view held out"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=n_quad)
    normals = export.render_scene_normals(scene, range(n), n_quad=n_quad)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    return export.export_tnt(root, images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)], normals=normals)


def make_tnt_proxy(root, scene, n_quad=256):
    """the analytic proxy's images alone in the tnt layout, every 8th view held out (--normal_ref needs no map)"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=n_quad)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    return export.export_tnt(root, images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)])


PROXY_DEPTH_SCALE, PROXY_DEPTH_SHIFT = 0.37, 0.11


def make_proxy_with_depths(root, scene, n_quad=256):
    """the analytic proxy with per-pixel monocular depth maps in the tnt layout, every 8th view held out: the files hold
    25 (0.37 D + 0.11) with D the scene's expected distance, so they are right up to a scale and a shift, which the term's
    fit has to absorb; a pixel without depth stays 0"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=n_quad)
    D = export.render_scene_depths(scene, range(n), n_quad=n_quad)
    depths = np.where(D > 0, 25.0 * (PROXY_DEPTH_SCALE * D + PROXY_DEPTH_SHIFT), 0.0).astype(np.float32)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    return export.export_tnt(root, images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)], depths=depths)


def make_proxy_with_all_maps(root, scene, n_quad=256):
    """the analytic proxy with labels, world-space normals and monocular depth maps (as make_proxy_with_depths writes them)
    together in the tnt layout, every 8th view held out"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=n_quad)
    labels = export.render_scene_labels(scene, range(n), n_quad=n_quad)
    normals = export.render_scene_normals(scene, range(n), n_quad=n_quad)
    D = export.render_scene_depths(scene, range(n), n_quad=n_quad)
    depths = np.where(D > 0, 25.0 * (PROXY_DEPTH_SCALE * D + PROXY_DEPTH_SHIFT), 0.0).astype(np.float32)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    return export.export_tnt(root, images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)], labels=labels,
                             normals=normals, depths=depths)


def make_hdr_proxy(root, scene, n_quad=256):
    """the analytic proxy as an HDR-NeRF synthetic scene under <root>/HDR-NeRF/syndata/chair (the loader reads layout, split
    and exposure table from the path): the scene's 35 views, taken as linear radiance, at three training and two held-out
    exposures (export.export_hdr_nerf_syn) -> that directory"""
    from ngp_amd.datasets import export
    if scene.poses.shape[0] != 35:
        raise ValueError(f"the synthetic HDR-NeRF split is fixed at 35 poses: the scene has {scene.poses.shape[0]}")
    radiance = export.render_scene_views(scene, range(35), rgba=False, n_quad=n_quad)
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    return export.export_hdr_nerf_syn(os.path.join(root, "HDR-NeRF", "syndata", "chair"), radiance, c2w, K, scene="chair")


def make_sky_proxy(root, scene, n_quad=256):
    """the analytic proxy composited over synthetic.analytic_sky (a background that depends on the view direction) in
    the tnt layout, every 8th view held out, with the scene's opacity of every pixel in opacity/<stem>.npy (float32, h x w)"""
    from ngp_amd.datasets import export
    n = scene.poses.shape[0]
    w, h = scene.img_wh
    pix = torch.arange(w * h, device=scene.device)
    images, opacities = [], []
    for i in range(n):
        o, d = scene.rays(torch.full((w * h,), i, dtype=torch.long, device=scene.device), pix)
        rgb, opacity = scene.ground_truth(o, d, n_quad=n_quad, sky=True)
        images.append((rgb.clamp(0, 1).reshape(h, w, 3).cpu().numpy() * 255.0 + 0.5).astype(np.uint8))
        opacities.append(opacity.reshape(h, w).cpu().numpy().astype(np.float32))
    c2w = scene.poses.cpu().numpy().astype("float64")
    K = scene.K.cpu().numpy().astype("float64")
    split_of = [1 if i % 8 == 0 else 0 for i in range(n)]
    export.export_tnt(root, np.stack(images), c2w, K, split_of)
    os.makedirs(os.path.join(root, "opacity"), exist_ok=True)
    for i in range(n):
        np.save(os.path.join(root, "opacity", f"{split_of[i]}_{i:08d}.npy"), opacities[i])
    return root


def opacity_maps(test_set, root):
    """the opacity map of every image of the split from <root>/opacity/<image stem>.npy (make_sky_proxy writes them), as
    (n_images, h*w) float32 on the split's device, or None when the scene has none or they do not fit the images"""
    paths = [os.path.join(root, "opacity", os.path.splitext(os.path.basename(p))[0] + ".npy") for p in getattr(test_set, "imgs", [])]
    if not paths or not all(os.path.exists(p) for p in paths):
        return None
    maps = np.stack([np.load(p).reshape(-1) for p in paths]).astype(np.float32)
    w, h = test_set.img_wh
    return torch.from_numpy(maps).to(test_set.rays.device) if maps.shape[1] == w * h else None


class SkyPsnr:
    """on_image callback of evaluate_split: the squared error over the pixels whose ground-truth opacity is below
    `below`, pooled over the split (on the device: one read-back, in value())"""

    def __init__(self, test_set, opacity, below=0.01, then=None):
        self.gt, self.sky, self.then = test_set.rays, opacity < below, then
        self.sq = torch.zeros((), dtype=torch.float64, device=opacity.device)
        self.n = torch.zeros((), dtype=torch.float64, device=opacity.device)

    def __call__(self, i, rgb, results):
        m = self.sky[i].to(rgb.device)
        err = (rgb - self.gt[i][..., :3].to(rgb.device)) ** 2
        self.sq += err[m].sum().double().to(self.sq.device)
        self.n += 3.0 * m.sum().double().to(self.n.device)
        if self.then is not None:
            self.then(i, rgb, results)

    def value(self):
        """(PSNR in dB, number of pixels); (None, 0) without a sky pixel"""
        n = float(self.n)
        return (float(-10.0 * torch.log10(self.sq / self.n)), int(n / 3)) if n else (None, 0)


def multi_terms_summary(terms_log, k=10):
    """{term: (mean over the first k steps, over the last k steps)} for terms[4:8] of train()'s terms_log"""
    t = torch.stack([v.detach() for v in terms_log]).cpu()
    k = max(1, min(k, len(t) // 2))
    names = ("CELoss", "sky_depth", "normal_mono", "depth_mono")
    return {nm: (float(t[:k, 4 + i].mean()), float(t[-k:, 4 + i].mean())) for i, nm in enumerate(names)}


def normal_ref_summary(terms_log, k=10):
    """{term: (mean over the first k steps, over the last k steps)} for the last two entries of train()'s terms_log"""
    t = torch.stack([v.detach() for v in terms_log]).cpu()
    k = max(1, min(k, len(t) // 2))
    return {nm: (float(t[:k, i].mean()), float(t[-k:, i].mean())) for nm, i in (("normal_ref_rp", -2), ("normal_ref_ro", -1))}


class NormalAgreement:
    """evaluate_split's on_image callback: the angle between results['normal_pred'] and results['normal_raw'] (both
    normalised by the test-time renderer) pooled over the held-out pixels whose opacity is above `threshold`; `then`: the
    callback to run behind it"""

    def __init__(self, threshold=0.5, then=None):
        self.threshold, self.then = threshold, then
        self.deg, self.n = 0.0, 0

    def __call__(self, i, rgb, results):
        keep = results["opacity"].reshape(-1) > self.threshold
        cos = (results["normal_pred"] * results["normal_raw"]).sum(-1).clamp(-1.0, 1.0)[keep]
        self.deg = self.deg + torch.rad2deg(torch.acos(cos)).double().sum()
        self.n = self.n + keep.sum()
        if self.then is not None:
            self.then(i, rgb, results)

    def value(self):
        """(mean angle in degrees, number of pixels); (None, 0) without a pixel"""
        n = int(self.n)
        return (float(self.deg) / n, n) if n else (None, 0)


def terms_summary(terms_log, k=10):
    """(number of loss terms, mean of the last term over the first k steps, over the last k steps) of train()'s terms_log"""
    t = torch.stack([v.detach() for v in terms_log]).cpu()
    k = max(1, min(k, len(t) // 2))
    return t.shape[1], float(t[:k, -1].mean()), float(t[-k:, -1].mean())


def main():
    args = parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(20220806)
    root = args.root_dir
    if args.make_proxy:
        from ngp_amd.synthetic import LegoProxy
        wh = int(800 * args.downsample)
        hdr = args.dataset_name == "colmap" and args.use_exposure
        scene = LegoProxy(n_images=35 if hdr else args.proxy_views, img_wh=(wh, wh), device=dev)
        if hdr:
            root = make_hdr_proxy(args.make_proxy, scene)
            args.downsample = 1.0
        elif args.multi_terms:
            root = make_proxy_with_all_maps(args.make_proxy, scene)
            args.downsample = 1.0   # (these layouts are written at the size they are read at)
        elif args.render_semantic:
            root = make_labelled_proxy(args.make_proxy, args.dataset_name, scene)
            args.downsample = 1.0
        elif args.normal_mono:
            root = make_proxy_with_normals(args.make_proxy, scene)
            args.downsample = 1.0
        elif args.depth_mono:
            root = make_proxy_with_depths(args.make_proxy, scene)
            args.downsample = 1.0
        elif args.use_skybox:
            root = make_sky_proxy(args.make_proxy, scene)
            args.downsample = 1.0
        elif args.normal_ref:
            root = make_tnt_proxy(args.make_proxy, scene)
            args.downsample = 1.0
        else:
            root = write_synthetic_dataset(args.make_proxy, scene, n_train=100, n_test=8, rgba=False)
    loader = dataset_dict[args.dataset_name]
    with_sem = args.render_semantic or "semantic" in args.multi_terms
    with_nrm = args.normal_mono or "normal_mono" in args.multi_terms
    with_dep = args.depth_mono or "depth_mono" in args.multi_terms
    flag = "--multi_terms" if args.multi_terms else None
    sem = dict(use_sem=True, num_classes=args.num_classes) if with_sem else {}
    if with_nrm:
        sem["normal_mono"] = True
    if with_dep:
        sem["depth_mono"] = True
    train_set = loader(root, "train", args.downsample, device=dev, **sem)
    test_set = loader(root, "test", args.downsample, device=dev, **sem)
    if with_sem and not hasattr(train_set, "labels"):
        raise SystemExit(f"{flag or '--render_semantic'}: {root} holds no labels (semantic/*.pgm) for the {args.dataset_name} loader")
    if with_nrm and not hasattr(train_set, "normals"):
        raise SystemExit(f"{flag or '--normal_mono'}: {root} holds no normal maps (normal/*.npy) for the {args.dataset_name} loader")
    if with_dep and not hasattr(train_set, "depths_2d"):
        raise SystemExit(f"{flag or '--depth_mono'}: {root} holds no depth maps (depth/*.npy) for the {args.dataset_name} loader")
    if args.use_exposure and train_set.rays.shape[-1] != 4:
        print(f"--use_exposure: the {args.dataset_name} loader found no exposure times in {root} (the colmap loader reads "
              "them for the HDR-NeRF layouts)", file=sys.stderr)
        raise SystemExit(2)
    if with_sem:
        labels_of_split(train_set)
        if hasattr(test_set, "labels"):
            labels_of_split(test_set)
        far = cameras_outside(train_set, args.scale)
        if far is not None:
            print(f"warning: --render_semantic with cameras outside the volume (a camera coordinate of {far:.2f}, --scale "
                  f"{args.scale}): the sky term rewards depth on rays labelled 4 and puts density at the far end of the volume, "
                  "between the scene and the cameras opposite; held-out PSNR suffers.  Choose --scale so that the volume "
                  "encloses the cameras.", file=sys.stderr)
    model = build_model(args.scale, dev, args.embed_a, args.embed_a_len, args.num_classes, args.use_exposure, args.use_skybox)
    unit_pred0 = None
    if args.use_exposure:
        with torch.no_grad():
            unit_pred0 = model.log_radiance_to_rgb(torch.zeros(1, 3, device=dev), exposure=torch.ones(1, 1, device=dev))
    msk_model = implicit_mask().to(dev) if args.embed_msk else None
    embedding_a = FrameEmbedding(args.embed_a_len, train_set.poses).to(dev) if args.embed_a else None
    pose_refiner = true_poses = None
    if args.optimize_ext:
        true_poses = torch.as_tensor(train_set.poses, dtype=torch.float32)
        start = perturb_poses(true_poses, *args.perturb_poses, seed=20220806) if args.perturb_poses else true_poses
        pose_refiner = PoseRefiner(start, train_set.directions).to(dev)
    t0 = time.perf_counter()
    trainer = train(model, train_set, args.num_epochs, args.steps_per_epoch, args.batch_size, args.lr, log_every=500,
          exp_step_factor=args.exp_step_factor, render_kwargs={"random_bg": True} if args.random_bg else None,
          msk_model=msk_model, embedding_a=embedding_a, pose_refiner=pose_refiner, pose_lr=args.pose_lr,
          semantic=args.render_semantic, num_classes=args.num_classes, normal_mono=args.normal_mono,
                    depth_mono=args.depth_mono, lambda_depth_mono=args.lambda_depth_mono, multi_terms=args.multi_terms,
                    use_exposure=args.use_exposure, use_skybox=args.use_skybox, normal_ref=args.normal_ref)
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    more = {}
    if embedding_a is not None:   # train.py:153-154: the test split is rendered with the code of training image 0
        more["embedding_a"] = embedding_a(0).detach()
    if with_sem or args.num_classes != 7:
        more["num_classes"] = args.num_classes
    if args.use_skybox:   # the held-out images are rendered over the skybox (render(test_time=True, use_skybox=True))
        more["use_skybox"] = True
    on_image = _save_rgb(args.save_dir, test_set.img_wh) if args.save_dir else None
    opacity = opacity_maps(test_set, root)
    sky_psnr = None
    if opacity is not None:
        on_image = sky_psnr = SkyPsnr(test_set, opacity, then=on_image)
    # (always measured: a run without --normal_ref is what the term's effect is read against)
    on_image = agree = NormalAgreement(then=on_image)
    res = evaluate_split(model, test_set, on_image=on_image, exp_step_factor=args.exp_step_factor, **more)
    psnrs, ssims = res["psnr"], res["ssim"]
    if args.ckpt_path:
        ckpt.save_ckpt(model, args.ckpt_path, msk_model=msk_model, pose_refiner=pose_refiner,
                       **({} if embedding_a is None else {"embedding_a": embedding_a}))
    out = {"train_s": t_train, "test_psnr_mean": sum(psnrs) / len(psnrs), "test_psnr": psnrs,
           "test_ssim_mean": sum(ssims) / len(ssims), "test_ssim": ssims,
           "steps": args.num_epochs * args.steps_per_epoch, "img_wh": train_set.img_wh}
    out["test_normal_agree_deg_mean"], out["test_normal_agree_pixels"] = agree.value()
    if args.normal_ref:
        out.update(normal_ref=True, loss_terms=int(trainer.terms_log[0].numel()))
        for nm, (first, last) in normal_ref_summary(trainer.terms_log).items():
            out[f"{nm}_term_first"], out[f"{nm}_term_last"] = first, last
    if args.use_skybox:
        out["use_skybox"] = True
    if sky_psnr is not None:   # over the held-out pixels that see only background
        out["test_sky_psnr"], out["test_sky_pixels"] = sky_psnr.value()
    if "sem_acc" in res:
        acc, miou = semantic_summary(res)   # accuracy over all valid pixels; images without a valid label take no part
        out.update(test_sem_acc_mean=acc, test_sem_acc=res["sem_acc"], test_sem_miou_mean=miou,
                   test_sem_miou=res["sem_miou"], test_sem_valid=res["sem_valid"],
                   num_classes=args.num_classes)
    if "normal_deg" in res:   # mean over the held-out images that have pixels with a normal
        out.update(test_normal_deg_mean=normal_summary(res), test_normal_deg=res["normal_deg"])
    if "depth_absrel" in res:   # mean over the held-out images that have pixels with a depth
        out.update(test_depth_absrel_mean=depth_summary(res), test_depth_absrel=res["depth_absrel"])
    if args.depth_mono:
        n_terms, first, last = terms_summary(trainer.terms_log)
        out.update(loss_terms=n_terms, depth_mono_term_first=first, depth_mono_term_last=last,
                   lambda_depth_mono=trainer.loss_fn.lambda_depth_mono)
    if args.use_exposure:   # the test images were rendered at their own exposures (evaluate_split), never seen in training
        with torch.no_grad():
            unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=dev), exposure=torch.ones(1, 1, device=dev))
        n_terms, first, last = terms_summary(trainer.terms_log)
        out.update(use_exposure=True, loss_terms=n_terms, unit_exposure_rgb=train_set.unit_exposure_rgb,
                   unit_exposure_rgb_init=unit_pred0[0].tolist(), unit_exposure_rgb_pred=unit[0].tolist(),
                   unit_exposure_term_first=first, unit_exposure_term_last=last)
    if args.multi_terms:
        out.update(loss_terms=int(trainer.terms_log[0].numel()), multi_terms=list(args.multi_terms),
                   lambda_depth_mono=trainer.loss_fn.lambda_depth_mono)
        for nm, (first, last) in multi_terms_summary(trainer.terms_log).items():
            out[f"{nm}_term_first"], out[f"{nm}_term_last"] = first, last
    if pose_refiner is not None:   # mean translation (scene units) and rotation (degrees) error against the dataset's poses
        before = pose_errors(pose_refiner.poses.cpu(), true_poses.cpu())
        after = pose_errors(pose_refiner.refined_poses().detach().cpu(), true_poses.cpu())
        out.update(pose_t_err_before=before[0], pose_rot_err_deg_before=before[1], pose_t_err_after=after[0],
                   pose_rot_err_deg_after=after[1], pose_lr=args.pose_lr)
    if msk_model is not None:
        means = mask_images(msk_model, train_set.img_wh, len(train_set.poses), dev, save_dir=args.save_dir)
        out["mask_mean"] = sum(means) / len(means)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
