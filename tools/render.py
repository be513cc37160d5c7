#!/usr/bin/env python3
"""Renders a frame series from a trained checkpoint (the reference's render.py:50-218): rgb / depth / normal /
semantic frames as PNG files and the depth points as points.npy, along the test split's poses or the dataset's own
camera path.  GPU only.  The 8-bit frames are packed on the device (ngp_frame_pack), so one byte per channel crosses to
the host.  Prints one JSON line: frames, the seconds spent rendering, on the metrics, packing, resizing, copying
device->host and encoding PNGs, and, when the split has ground truth, mean and per-image PSNR / SSIM.  No video is written: the frame directory is
what a video encoder takes.  --anti_aliasing_factor S renders int(H*S) x int(W*S) rays per frame, packs them to 8 bits
and brings them back to W x H with Pillow's bicubic filter on the device (ngp_resize_bicubic_u8), as the reference's
render.py:150-156 does on the host; PSNR / SSIM are then those of the anti-aliased 8-bit frame.

  python tools/render.py --ckpt ckpts/lego.ckpt --root_dir /data/nerf_synthetic/lego --out_dir frames --render_rgb
  python tools/render.py --ckpt ckpts/tnt.ckpt --root_dir /data/tnt/Playground --dataset_name tnt --scale 8 \\
      --exp_step_factor 0.00390625 --render_traj --render_rgb --render_depth --render_normal --out_dir frames
  python tools/render.py --ckpt ckpts/lego.ckpt --root_dir /data/nerf_synthetic/lego --out_dir frames --render_rgb \\
      --anti_aliasing_factor 2
  python tools/render.py --ckpt ckpts/tnt.ckpt --root_dir /data/tnt/Playground --dataset_name tnt --scale 8 \\
      --exp_step_factor 0.00390625 --render_rgb --embed_a --embed_a_len 8 --out_dir frames   # appearance codes
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = {"rgb": "rgb", "depth": "depth", "normal": "normal", "normal_raw": "normal-raw", "semantic": "semantic"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(
        description="Frame series of a trained model: NNN-rgb.png, NNN-depth.png, NNN-normal.png, NNN-normal-raw.png, "
                    "NNN-semantic.png and points.npy (float32 (frames, H, W, 3)) in --out_dir.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="checkpoint ({'state_dict': {'model.<key>': ...}})")
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--root_dir", required=True)
    ap.add_argument("--dataset_name", default="nerf", help="nerf, nsvf, colmap, tnt or nerfpp")
    ap.add_argument("--downsample", type=float, default=1.0)
    ap.add_argument("--exp_step_factor", type=float, default=0.0, help="1/256 for unbounded scenes (opt.py)")
    ap.add_argument("--num_classes", type=int, default=7)
    ap.add_argument("--chunk_size", type=int, default=131072, help="rays per render() call")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--render_rgb", action="store_true", help="render rgb series")
    ap.add_argument("--render_depth", action="store_true", help="render depth series (Turbo of depth / (2 * scale))")
    ap.add_argument("--render_normal", action="store_true", help="render normal series (predicted and raw)")
    ap.add_argument("--render_semantic", action="store_true", help="render semantic segmentation series")
    ap.add_argument("--render_points", action="store_true", help="render depth points (points.npy)")
    ap.add_argument("--render_traj", action="store_true",
                    help="follow the dataset's own camera path (render_traj_rays) instead of the test poses")
    ap.add_argument("--anti_aliasing_factor", type=float, default=1.0,
                    help="render rgb / depth / normal frames on an int(H*S) x int(W*S) lattice and resize the 8-bit "
                         "frames back with Pillow's bicubic filter, on the device; 1 to 8")
    ap.add_argument("--embed_a", action="store_true",
                    help="the checkpoint was trained with appearance codes (--embed_a): every frame is rendered with a code picked by --embed_a_mode")
    ap.add_argument("--embed_a_len", type=int, default=4, help="length of an appearance code")
    ap.add_argument("--embed_a_mode", choices=("mean", "nearest", "index"), default="mean",
                    help="code of a frame: mean of the two training cameras nearest to the frame's pose, the nearest "
                         "one, or training image <frame number>; needs the train split's poses")
    ap.add_argument("--use_exposure", action="store_true",
                    help="the checkpoint was trained with --use_exposure (log-radiance and three tone-mappers): every frame "
                         "is rendered at its test item's exposure time, or at --exposure")
    ap.add_argument("--exposure", type=float, default=None, metavar="T",
                    help="with --use_exposure: render every frame at T seconds instead of the items' own exposures")
    ap.add_argument("--use_skybox", action="store_true",
                    help="the checkpoint was trained with --use_skybox (skybox_dir_encoder and skybox_rgb_net): every frame is "
                         "rendered over the skybox's colour of its rays")
    ap.add_argument("--aa_host_check", action="store_true",
                    help="with --anti_aliasing_factor and --render_rgb: also copy the fine 8-bit rgb frame to the host, "
                         "resize it with Pillow, require equality with the device result and report host_route_s")
    args = ap.parse_args(argv)
    if not 1.0 <= args.anti_aliasing_factor <= 8.0:
        ap.error("--anti_aliasing_factor must lie in [1, 8]")
    if args.anti_aliasing_factor > 1.0 and (args.render_semantic or args.render_points or args.render_traj):
        ap.error("--anti_aliasing_factor does not go with --render_semantic (labels do not average), --render_points "
                 "or --render_traj (the camera path's rays come from the loader at one ray per pixel)")
    if args.aa_host_check and not (args.anti_aliasing_factor > 1.0 and args.render_rgb):
        ap.error("--aa_host_check needs --anti_aliasing_factor above 1 and --render_rgb")
    if args.exposure is not None and not args.use_exposure:
        ap.error("--exposure needs --use_exposure")
    if args.use_skybox and args.use_exposure:
        ap.error("--use_skybox does not go with --use_exposure (no recipe trains both)")
    if args.exposure is not None and not args.exposure > 0:
        ap.error("--exposure must be positive (seconds)")
    if args.chunk_size <= 0:
        ap.error("--chunk_size must be positive")
    if not (args.render_rgb or args.render_depth or args.render_normal or args.render_semantic or args.render_points):
        ap.error("nothing to render: give at least one of --render_rgb --render_depth --render_normal "
                 "--render_semantic --render_points")
    return args


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    import ngp_amd  # noqa: F401
    from ngp_amd import ckpt
    from ngp_amd.datasets import dataset_dict
    from ngp_amd.evaluation import frame_images, image_metrics, render_image, render_rays
    from ngp_amd.imaging import resize_u8, supersampled_size
    from ngp_amd.networks import NGP

    if args.dataset_name not in dataset_dict:
        raise SystemExit(f"unknown --dataset_name {args.dataset_name}; known: {sorted(dataset_dict)}")
    dev = torch.device("cuda", 0)
    more = dict(embed_a=True, embed_a_len=args.embed_a_len) if args.embed_a else {}
    if args.use_exposure:
        more["rgb_act"] = "None"
    if args.use_skybox:
        more["use_skybox"] = True
    model = NGP(scale=args.scale, classes=args.num_classes, **more).to(dev)
    ckpt.load_ckpt(model, args.ckpt, prefixes_to_ignore=['embedding_a', 'msk_model', 'density_grid', 'grid_coords'])
    test_set = dataset_dict[args.dataset_name](args.root_dir, "test", args.downsample, device=dev,
                                               render_traj=args.render_traj, num_classes=args.num_classes)
    w, h = test_set.img_wh
    directions = test_set.directions.to(dev)
    frame_embed = None
    if args.embed_a:   # render.py:91-93 of the reference: the table over the TRAINING poses
        from ngp_amd.appearance import FrameEmbedding
        train_set = dataset_dict[args.dataset_name](args.root_dir, "train", args.downsample, device=dev)
        frame_embed = FrameEmbedding(args.embed_a_len, train_set.poses.to(dev), args.ckpt).to(dev)
    if args.render_traj:
        if getattr(test_set, "render_traj_rays", None) is None or getattr(test_set, "render_c2w", None) is None:
            raise SystemExit(f"--render_traj: the {args.dataset_name} loader found no camera path for {args.root_dir} "
                             "(no render_traj_rays); render the test poses instead")
        traj_rays = test_set.render_traj_rays                # the loader's own rays; the poses only rotate the normals
        poses = test_set.render_c2w.to(dev)
        have_gt = False
    else:
        poses = test_set.poses.to(dev)
        have_gt = len(test_set.rays) > 0

    want = [k for k, on in (("rgb", args.render_rgb), ("depth", args.render_depth), ("normal", args.render_normal),
                            ("normal_raw", args.render_normal), ("semantic", args.render_semantic)) if on]
    aa = args.anti_aliasing_factor
    fine_h, fine_w = supersampled_size(h, w, aa) if aa > 1.0 else (h, w)
    packed = want if aa == 1.0 or not have_gt or "rgb" in want else want + ["rgb"]   # the metrics need the 8-bit rgb
    os.makedirs(args.out_dir, exist_ok=True)
    t = {"render_s": 0.0, "metrics_s": 0.0, "pack_s": 0.0, "resize_s": 0.0, "d2h_s": 0.0, "png_s": 0.0}
    host_route_s = 0.0
    psnrs, ssims, points = [], [], []
    render_kwargs = {"exp_step_factor": args.exp_step_factor, "num_classes": args.num_classes}
    if args.use_skybox:
        render_kwargs["use_skybox"] = True

    def tick():
        torch.cuda.synchronize()
        return time.perf_counter()

    for i in range(len(poses)):
        item = test_set[i] if have_gt else {}
        gt = item["rgb"].to(dev) if have_gt else None      # a split kept on the host is copied outside the stages
        if args.use_exposure:   # one exposure time per frame, every sample's
            seconds = args.exposure
            if seconds is None:
                if "exposure" not in item:
                    raise SystemExit(f"--use_exposure: frame {i} carries no exposure time; give --exposure T")
                seconds = float(item["exposure"])
            render_kwargs["exposure"] = torch.full((1, 1), float(seconds), device=dev)
        if frame_embed is not None:
            with torch.no_grad():
                key = i % len(frame_embed.poses) if args.embed_a_mode == "index" else poses[i]
                render_kwargs["embedding_a"] = frame_embed(key, mode=args.embed_a_mode)
        t0 = tick()
        if args.render_traj:
            rays = traj_rays[i][:, :6].to(dev)
            results = render_rays(model, rays[:, :3], rays[:, 3:6], args.chunk_size, **render_kwargs)
        elif aa > 1.0:
            results = render_image(model, None, poses[i], args.chunk_size, anti_aliasing_factor=aa, K=test_set.K,
                                   img_wh=(w, h), **render_kwargs)
        else:
            results = render_image(model, directions, poses[i], args.chunk_size, **render_kwargs)
        t1 = tick()
        t["render_s"] += t1 - t0
        if aa == 1.0:
            if have_gt:
                p, q, _ = image_metrics(results["rgb"], gt, (w, h))
            tm = tick()
            images = frame_images(results, poses[i], args.scale, args.num_classes, want, img_wh=(w, h)) if want else {}
            t2 = tick()
            t["metrics_s"] += tm - t1
            t["pack_s"] += t2 - tm
        else:
            # the fine frame is packed to 8 bits, then resized; the anti-aliased 8-bit frame is what is kept, so it is
            # what PSNR / SSIM are taken on
            fine = frame_images(results, poses[i], args.scale, args.num_classes, packed, img_wh=(fine_w, fine_h)) \
                if packed else {}
            tp = tick()
            images = {k: resize_u8(v, (w, h)) for k, v in fine.items()}
            tr = tick()
            if have_gt:
                p, q, _ = image_metrics(images["rgb"].reshape(h * w, 3).float() / 255, gt, (w, h))
            t2 = tick()
            t["pack_s"] += tp - t1
            t["resize_s"] += tr - tp
            t["metrics_s"] += t2 - tr
            if args.aa_host_check:           # the route the device resize replaces: the fine frame to the host, Pillow
                host = np.asarray(Image.fromarray(fine["rgb"].cpu().numpy()).resize((w, h), Image.Resampling.BICUBIC))
                host_route_s += time.perf_counter() - t2
                if not np.array_equal(host, images["rgb"].cpu().numpy()):
                    raise SystemExit(f"--aa_host_check: frame {i}: the device resize differs from Pillow's")
                t2 = tick()
            images = {k: v for k, v in images.items() if k in want}
        if have_gt:
            psnrs.append(p)
            ssims.append(q)
        images = {k: v.cpu().numpy() for k, v in images.items()}
        if args.render_points:
            points.append(results["points"].reshape(h, w, 3).cpu().numpy())
        t3 = tick()
        for k, img in images.items():
            Image.fromarray(img).save(os.path.join(args.out_dir, f"{i:03d}-{FILES[k]}.png"))
        t4 = time.perf_counter()
        t["d2h_s"] += t3 - t2
        t["png_s"] += t4 - t3
    if args.render_points:
        np.save(os.path.join(args.out_dir, "points.npy"), np.stack(points).astype(np.float32))
    line = {"frames": len(poses), "img_wh": [w, h], "outputs": want + (["points"] if args.render_points else []),
            **{k: round(v, 4) for k, v in t.items()}}
    if aa > 1.0:
        line.update(anti_aliasing_factor=aa, supersampled_wh=[fine_w, fine_h])
        if have_gt:
            line["metrics_on"] = "antialiased_u8"
        if args.aa_host_check:
            line["host_route_s"] = round(host_route_s, 4)
    if have_gt and psnrs:
        p, s = torch.stack(psnrs).tolist(), torch.stack(ssims).tolist()
        line.update(psnr_mean=sum(p) / len(p), psnr=p, ssim_mean=sum(s) / len(s), ssim=s)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
