#!/usr/bin/env python3
"""Renders one equirectangular panorama around a point from a trained checkpoint (the reference's
render_panorama.py:87-136): rgb.png, opacity.png and mask.png (and depth.png) in --out_dir.  GPU only.  Column u looks
theta = (u - W/2 + 0.5) 2 pi / W away from --v_forward toward --v_right, row v phi = (v - H/2 + 0.5) pi / H toward
--v_down; the three vectors depend on the dataset's axes.  The 8-bit images are packed on the device (ngp_frame_pack);
with --anti_aliasing_factor S the panorama is rendered at int(H*S) x int(W*S) and brought back with Pillow's bicubic
filter on the device (ngp_resize_bicubic_u8).  Prints one JSON line: the sizes and the seconds of each stage.

  python tools/render_panorama.py --ckpt ckpts/tnt.ckpt --scale 8 --exp_step_factor 0.00390625 --out_dir pano \\
      --pano_hw 512 1024 --v_forward 0 0 1 --v_down 0 1 0 --v_right 1 0 0
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(
        description="Equirectangular panorama of a trained model: rgb.png, opacity.png, mask.png and, with "
                    "--render_depth, depth.png in --out_dir.",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="checkpoint ({'state_dict': {'model.<key>': ...}})")
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--pano_hw", type=int, nargs=2, required=True, metavar=("H", "W"), help="panorama size")
    ap.add_argument("--v_forward", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"),
                    help="world direction of the panorama's centre column")
    ap.add_argument("--v_down", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"),
                    help="world direction of the bottom pole")
    ap.add_argument("--v_right", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"),
                    help="world direction a quarter turn right of the centre column")
    ap.add_argument("--origin", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                    help="the point the panorama is taken around")
    ap.add_argument("--pano_radius", type=float, default=0.0, help="rays start this far from --origin, along themselves")
    ap.add_argument("--exp_step_factor", type=float, default=0.0, help="1/256 for unbounded scenes (opt.py)")
    ap.add_argument("--num_classes", type=int, default=7)
    ap.add_argument("--chunk_size", type=int, default=131072, help="rays per render() call")
    ap.add_argument("--anti_aliasing_factor", type=float, default=1.0,
                    help="render int(H*S) x int(W*S) rays and resize the 8-bit images back with Pillow's bicubic filter, "
                         "on the device; 1 to 8")
    ap.add_argument("--embed_a", action="store_true",
                    help="the checkpoint was trained with appearance codes (--embed_a): the panorama is rendered with the code of training image 0")
    ap.add_argument("--embed_a_len", type=int, default=4, help="length of an appearance code")
    ap.add_argument("--use_skybox", action="store_true",
                    help="the checkpoint was trained with --use_skybox: the panorama is rendered over the skybox's colour of "
                         "its rays (mask.png still marks the pixels without opacity)")
    ap.add_argument("--render_depth", action="store_true", help="also write depth.png (Turbo of depth / (2 * scale))")
    ap.epilog = ("mask.png is 255 where the opacity BYTE is 0 and 0 elsewhere: the reference compares the uint8 opacity "
                 "image with 0.5 (render_panorama.py:126-133), so only fully transparent pixels are marked.")
    args = ap.parse_args(argv)
    if min(args.pano_hw) <= 0:
        ap.error("--pano_hw must be positive")
    if args.chunk_size <= 0:
        ap.error("--chunk_size must be positive")
    if not 1.0 <= args.anti_aliasing_factor <= 8.0:
        ap.error("--anti_aliasing_factor must lie in [1, 8]")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    from PIL import Image
    import ngp_amd  # noqa: F401
    from ngp_amd import ckpt
    from ngp_amd.evaluation import frame_images, render_rays
    from ngp_amd.imaging import panorama_rays, resize_u8, supersampled_size
    from ngp_amd.networks import NGP

    dev = torch.device("cuda", 0)
    build = dict(embed_a=True, embed_a_len=args.embed_a_len) if args.embed_a else {}
    if args.use_skybox:
        build["use_skybox"] = True
    model = NGP(scale=args.scale, classes=args.num_classes, **build).to(dev)
    ckpt.load_ckpt(model, args.ckpt, prefixes_to_ignore=['embedding_a', 'msk_model', 'density_grid', 'grid_coords'])
    more = {}
    if args.embed_a:   # render_panorama.py:80-85 of the reference: the code of training image 0
        table = ckpt.extract_model_state_dict(args.ckpt, model_name='embedding_a')['weight']
        if table.dim() != 2 or table.shape[1] != args.embed_a_len:
            raise SystemExit(f"--embed_a_len {args.embed_a_len}: the checkpoint's table is {tuple(table.shape)}")
        more["embedding_a"] = table[0:1].to(dev).float().contiguous()
    if args.use_skybox:
        more["use_skybox"] = True
    H, W = args.pano_hw
    aa = args.anti_aliasing_factor
    fine_h, fine_w = supersampled_size(H, W, aa) if aa > 1.0 else (H, W)
    want = ["rgb", "opacity"] + (["depth"] if args.render_depth else [])

    def tick():
        torch.cuda.synchronize()
        return time.perf_counter()

    t0 = tick()
    rays_o, rays_d = panorama_rays(fine_h, fine_w, args.v_forward, args.v_down, args.v_right, origin=args.origin,
                                   radius=args.pano_radius, device=dev)
    t1 = tick()
    results = render_rays(model, rays_o, rays_d, args.chunk_size, exp_step_factor=args.exp_step_factor,
                          num_classes=args.num_classes, **more)
    t2 = tick()
    images = frame_images(results, None, args.scale, args.num_classes, want, img_wh=(fine_w, fine_h))
    t3 = tick()
    if aa > 1.0:
        images = {k: resize_u8(v, (W, H)) for k, v in images.items()}
    t4 = tick()
    images = {k: v.cpu().numpy() for k, v in images.items()}
    t5 = tick()
    os.makedirs(args.out_dir, exist_ok=True)
    images["mask"] = ((images["opacity"] == 0) * 255).astype("uint8")
    for k, img in images.items():
        Image.fromarray(img).save(os.path.join(args.out_dir, f"{k}.png"))
    t6 = time.perf_counter()
    line = {"pano_hw": [H, W], "outputs": sorted(images), "rays": fine_h * fine_w,
            "transparent_pixels": int((images["opacity"] == 0).sum()),
            "rays_s": round(t1 - t0, 4), "render_s": round(t2 - t1, 4), "pack_s": round(t3 - t2, 4),
            "resize_s": round(t4 - t3, 4), "d2h_s": round(t5 - t4, 4), "png_s": round(t6 - t5, 4)}
    if aa > 1.0:
        line.update(anti_aliasing_factor=aa, supersampled_hw=[fine_h, fine_w])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
