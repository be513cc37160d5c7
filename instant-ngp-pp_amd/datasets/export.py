"""Writers for the on-disk formats the loaders read, so that synthetic scenes can stand in for the
datasets this repository cannot ship (no NeRF-Synthetic / T&T / mip-NeRF-360 files exist here or on
the GPU box).  Generic writers take images (n,h,w,3|4) uint8, camera-to-world poses (n,3,4) in
[right down front] axes and a 3x3 pinhole matrix; `write_synthetic_dataset` renders the analytic
lego-proxy scene and writes it as a NeRF-Synthetic directory."""
import json
import math
import os

import numpy as np
import torch

from . import colmap_utils as cu


def _save_png(arr, path):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr, {2: "L", 3: "RGB", 4: "RGBA"}[arr.shape[2] if arr.ndim == 3 else 2]).save(path)


def _label_u8(label):
    """one label image for the 8-bit PGM writer: 256, the reference's ignore_index, does not fit and is stored as 255
    (ignored as well by the fused semantic tail for every class count it takes, and mapped back by nothing)"""
    label = np.asarray(label)
    if label.dtype == np.uint8:
        return label
    if (label < 0).any():
        raise ValueError("negative labels cannot be written to a .pgm")
    return np.minimum(label, 255).astype(np.uint8)


def _homog(c2w):
    m = np.eye(4)
    m[:3, :4] = c2w
    return m


def export_blender(root, images, c2w, camera_angle_x, splits):
    """NeRF-Synthetic: splits = {"train": [frame indices], ...}; poses are stored in Blender axes"""
    for split, idxs in splits.items():
        frames = []
        for k, i in enumerate(idxs):
            _save_png(images[i], os.path.join(root, split, f"r_{k}.png"))
            m = _homog(c2w[i])
            m[:3, 1:3] *= -1
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": m.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": camera_angle_x, "frames": frames}, f)
    return root


def export_tnt(root, images, c2w, K, split_of, img_dir="images", labels=None, depths=None, camera_path=None,
               flat_intrinsics=False, normals=None):
    """T&T / NSVF layout: split_of[i] in {0,1,2} is the file-name prefix of frame i.
    normals (n,h,w,3) float, world space, (0,0,0) = no normal -> normal/*.npy as float32 (the loader rescales translations
    only: no rotation applies),
    labels (n,h,w) uint8 or wider integers (256 and above are stored as 255) -> semantic/*.pgm, depths (n,h,w) float -> depth/*.npy,
    camera_path (m,3,4) -> camera_path/pose/<5 digits>.txt"""
    os.makedirs(os.path.join(root, "pose"), exist_ok=True)
    K4 = np.eye(4)
    K4[:3, :3] = K
    np.savetxt(os.path.join(root, "intrinsics.txt"), K4.reshape(1, 16) if flat_intrinsics else K4)
    for i in range(len(images)):
        stem = f"{split_of[i]}_{i:08d}"
        _save_png(images[i], os.path.join(root, img_dir, stem + ".png"))
        np.savetxt(os.path.join(root, "pose", stem + ".txt"), _homog(c2w[i]))
        if labels is not None:
            _save_png(_label_u8(labels[i]), os.path.join(root, "semantic", stem + ".pgm"))
        if depths is not None:
            os.makedirs(os.path.join(root, "depth"), exist_ok=True)
            np.save(os.path.join(root, "depth", stem + ".npy"), depths[i])
        if normals is not None:
            os.makedirs(os.path.join(root, "normal"), exist_ok=True)
            np.save(os.path.join(root, "normal", stem + ".npy"), np.asarray(normals[i], dtype=np.float32))
    if camera_path is not None:
        os.makedirs(os.path.join(root, "camera_path", "pose"), exist_ok=True)
        for j, pose in enumerate(camera_path):
            np.savetxt(os.path.join(root, "camera_path", "pose", f"path_{j:05d}.txt"), _homog(pose))
    return root


def export_nsvf(root, images, c2w, K, split_of, bbox):
    """NSVF layout = the T&T one with rgb/ and bbox.txt"""
    export_tnt(root, images, c2w, K, split_of, img_dir="rgb")
    np.savetxt(os.path.join(root, "bbox.txt"), np.asarray(bbox, dtype=np.float64).reshape(1, -1))
    return root


def export_nerfpp(root, images, c2w, K, splits):
    """NeRF++ layout: <split>/{rgb,pose,intrinsics}/, 16 numbers per text file"""
    K4 = np.eye(4)
    K4[:3, :3] = K
    for split, idxs in splits.items():
        for sub in ("rgb", "pose", "intrinsics"):
            os.makedirs(os.path.join(root, split, sub), exist_ok=True)
        for i in idxs:
            _save_png(images[i], os.path.join(root, split, "rgb", f"{i:05d}.png"))
            np.savetxt(os.path.join(root, split, "pose", f"{i:05d}.txt"), _homog(c2w[i]).reshape(1, 16))
            np.savetxt(os.path.join(root, split, "intrinsics", f"{i:05d}.txt"), K4.reshape(1, 16))
    return root


def _write_colmap_sparse(root, hw, c2w, K, names, points=None, model="PINHOLE", order=None):
    """sparse/0/{cameras,images,points3D}.bin: ONE camera (id 1) of size hw = (h, w), world-to-camera poses, records
    stored in `order`"""
    h, w = hw
    os.makedirs(os.path.join(root, "sparse", "0"), exist_ok=True)
    if model == "PINHOLE":
        params = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    elif model == "SIMPLE_RADIAL":
        params = [K[0, 0], K[0, 2], K[1, 2], 0.0]
    elif model == "OPENCV":
        params = [K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.0, 0.0, 0.0, 0.0]
    else:
        params = [0.0] * cu.CAMERA_MODELS[cu.CAMERA_MODEL_IDS[model]][1]
    cu.write_cameras_binary({1: cu.Camera(1, model, w, h, np.array(params, dtype=np.float64))},
                            os.path.join(root, "sparse/0/cameras.bin"))
    records = {}
    for i in (range(len(names)) if order is None else order):
        w2c = np.linalg.inv(_homog(c2w[i]))
        records[i + 1] = cu.Image(i + 1, cu.rotmat2qvec(w2c[:3, :3]), w2c[:3, 3], 1, names[i],
                                  np.zeros((0, 2)), np.zeros(0, dtype=np.int64))
    cu.write_images_binary(records, os.path.join(root, "sparse/0/images.bin"))
    points = np.zeros((1, 3)) if points is None else np.asarray(points, dtype=np.float64)
    cloud = {j + 1: cu.Point3D(j + 1, p, np.array([128, 128, 128], dtype=np.uint8), 0.5,
                               np.array([1], dtype=np.int32), np.array([0], dtype=np.int32)) for j, p in enumerate(points)}
    cu.write_points3d_binary(cloud, os.path.join(root, "sparse/0/points3D.bin"))


def export_colmap(root, images, c2w, K, names=None, points=None, model="PINHOLE", labels=None, shuffle_seed=None):
    """COLMAP layout: sparse/0/*.bin with ONE camera (id 1) and world-to-camera poses, images/<name>.
    `shuffle_seed` stores the image records in a permuted order (COLMAP registers images in
    reconstruction order, not name order — the loader has to sort)."""
    n, h, w = images.shape[0], images.shape[1], images.shape[2]
    names = names or [f"frame_{i:04d}.png" for i in range(n)]
    order = list(range(n))
    if shuffle_seed is not None:
        order = list(np.random.default_rng(shuffle_seed).permutation(n))
    _write_colmap_sparse(root, (h, w), c2w, K, names, points, model, order)
    for i in order:
        _save_png(images[i], os.path.join(root, "images", names[i]))
        if labels is not None:
            _save_png(_label_u8(labels[i]), os.path.join(root, "semantic", os.path.splitext(names[i])[0] + ".pgm"))
    return root


HDR_UNIT_EXPOSURE_RGB = 0.73   # what ColmapDataset sets for the synthetic HDR-NeRF scenes


def hdr_response(radiance, seconds, unit_rgb=HDR_UNIT_EXPOSURE_RGB):
    """the camera response of export_hdr_nerf_syn: sigmoid(ln(radiance * seconds) + logit(unit_rgb)), 0 at zero
    radiance.  Unit radiance at unit exposure maps to unit_rgb, and a tone-mapper (a sigmoid of a function of
    ln radiance + ln seconds) can represent it."""
    x = np.asarray(radiance, dtype=np.float64) * float(seconds)
    return x / (x + (1.0 - unit_rgb) / unit_rgb)


def export_hdr_nerf_syn(root, radiance_images, c2w, K, scene='chair'):
    """The HDR-NeRF synthetic layout ColmapDataset._hdr_split reads (`root` must end in HDR-NeRF/syndata/<scene>: the
    loader takes the layout, the split rule and the exposure table from the path): sparse/0/*.bin with the 35
    registered frames in name order, train/NNN_e.png = the last 18 poses at exposures e in {0, 2, 4}, test/NNN_e.png =
    the first 17 poses at e in {1, 3}: exposures never seen in training, HDR-NeRF's protocol.  Nothing else is written
    into either directory (the loader globs *[024].png and *[13].png).
    radiance_images (35, h, w, 3): linear radiance, float, or uint8 (taken as value / 255); the 8-bit image at exposure e
    is hdr_response(radiance, colmap._HDR_EXPOSURES[scene][e])."""
    from .colmap import _HDR_EXPOSURES
    radiance = np.asarray(radiance_images)
    if radiance.ndim != 4 or radiance.shape[0] != 35 or radiance.shape[3] != 3:
        raise ValueError(f"the synthetic HDR-NeRF split is fixed at 35 poses of (h, w, 3): got {radiance.shape}")
    if scene not in _HDR_EXPOSURES:
        raise ValueError(f"no exposure table for scene {scene!r}: known {sorted(_HDR_EXPOSURES)}")
    parts = [p for p in os.path.normpath(str(root)).split(os.sep) if p]
    if parts[-1] != scene or 'syndata' not in parts or 'HDR-NeRF' not in parts:
        raise ValueError(f"root must end in HDR-NeRF/syndata/{scene} (the loader reads the layout from the path): got {root}")
    if radiance.dtype == np.uint8:
        radiance = radiance.astype(np.float64) / 255.0
    times = _HDR_EXPOSURES[scene]
    _write_colmap_sparse(root, radiance.shape[1:3], c2w, K, [f"{i:03d}.png" for i in range(35)])
    for split, poses, digits in (("test", range(17), (1, 3)), ("train", range(17, 35), (0, 2, 4))):
        for i in poses:
            for e in digits:
                img = (hdr_response(radiance[i], times[e]) * 255.0 + 0.5).astype(np.uint8)
                _save_png(img, os.path.join(root, split, f"{i:03d}_{e}.png"))
    return root


@torch.no_grad()
def render_scene_views(scene, idxs, rgba=True, n_quad=256):
    """uint8 views of an analytic scene (synthetic.LegoProxy): rgba=True stores un-premultiplied
    colour + alpha = accumulated opacity (what Blender writes; loaders blend it on white);
    rgba=False stores the scene composited on black, the background the renderer adds for synthetic
    scenes (rendering.py:231-232)."""
    w, h = scene.img_wh
    pix = torch.arange(w * h, device=scene.device)
    out = []
    for i in idxs:
        o, d = scene.rays(torch.full((w * h,), int(i), dtype=torch.long, device=scene.device), pix)
        rgb, opacity = scene.ground_truth(o, d, n_quad=n_quad)
        if rgba:
            a = opacity.clamp(0, 1)[:, None]
            colour = torch.where(a > 1e-6, rgb / a.clamp(min=1e-6), torch.zeros_like(rgb)).clamp(0, 1)
            img = torch.cat([colour, a], -1).reshape(h, w, 4)
        else:
            img = rgb.clamp(0, 1).reshape(h, w, 3)
        out.append((img.cpu().numpy() * 255.0 + 0.5).astype(np.uint8))
    return np.stack(out)


@torch.no_grad()
def render_scene_labels(scene, idxs, n_quad=256):
    """per-pixel classes of an analytic scene's views (synthetic.LegoProxy.ground_truth_labels: parts 0-3, 4 = sky,
    256 = ignore) -> (n, h, w) int64; export_tnt / export_colmap take them as `labels`"""
    w, h = scene.img_wh
    pix = torch.arange(w * h, device=scene.device)
    out = []
    for i in idxs:
        o, d = scene.rays(torch.full((w * h,), int(i), dtype=torch.long, device=scene.device), pix)
        out.append(scene.ground_truth_labels(o, d, n_quad=n_quad).reshape(h, w).cpu().numpy())
    return np.stack(out)


@torch.no_grad()
def render_scene_normals(scene, idxs, n_quad=256):
    """per-pixel world-space normals of an analytic scene's views (synthetic.LegoProxy.ground_truth_normals: unit
    vectors, (0, 0, 0) where the pixel has none) -> (n, h, w, 3) float32; export_tnt takes them as `normals`"""
    w, h = scene.img_wh
    pix = torch.arange(w * h, device=scene.device)
    out = []
    for i in idxs:
        o, d = scene.rays(torch.full((w * h,), int(i), dtype=torch.long, device=scene.device), pix)
        out.append(scene.ground_truth_normals(o, d, n_quad=n_quad).reshape(h, w, 3).cpu().numpy())
    return np.stack(out)


@torch.no_grad()
def render_scene_depths(scene, idxs, n_quad=256):
    """per-pixel expected distance of an analytic scene's views (synthetic.LegoProxy.ground_truth_depths: 0 where the
    pixel has none) -> (n, h, w) float32; export_tnt takes them, or an affine function of them, as `depths`"""
    w, h = scene.img_wh
    pix = torch.arange(w * h, device=scene.device)
    out = []
    for i in idxs:
        o, d = scene.rays(torch.full((w * h,), int(i), dtype=torch.long, device=scene.device), pix)
        out.append(scene.ground_truth_depths(o, d, n_quad=n_quad).reshape(h, w).cpu().numpy())
    return np.stack(out)


def write_synthetic_dataset(root_dir, scene, n_train=20, n_test=4, rgba=True, n_quad=256):
    """Exports views of `scene` as a NeRF-Synthetic directory.  The image size must be
    int(800*downsample) for the downsample used at load time."""
    w, _ = scene.img_wh
    assert n_train + n_test <= scene.poses.shape[0]
    idxs = list(range(n_train + n_test))
    images = render_scene_views(scene, idxs, rgba=rgba, n_quad=n_quad)
    c2w = scene.poses[:n_train + n_test].cpu().numpy().astype(np.float64)
    held_out = list(range(n_train, n_train + n_test))
    return export_blender(root_dir, images, c2w, 2 * math.atan(0.5 * w / float(scene.K[0, 0])),
                          {"train": list(range(n_train)), "test": held_out, "val": held_out})
