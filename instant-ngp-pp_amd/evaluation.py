"""Image-shaped outputs of the test-time renderer: whole frames from one camera, their 8-bit images, and the metrics of
a held-out split (what the reference's render.py:50-218 and validation step train.py:347-392 do).

  render_image(model, directions, pose, chunk, **render_kwargs) -> the per-ray results of render(test_time=True);
                                                                   anti_aliasing_factor=s, K=, img_wh= renders the
                                                                   int(h*s) x int(w*s) lattice of the same camera
  render_rays(model, rays_o, rays_d, chunk, **render_kwargs)    -> the same for given rays (a camera path's)
  image_metrics(rgb, gt, img_wh)                                -> (psnr, ssim) of one image on the device
  frame_images(results, pose, scale, num_classes, want, img_wh) -> {name: uint8 image} through ngp_frame_pack (I2);
                                                                   out_wh= brings a supersampled frame back to the
                                                                   image size (ngp_resize_bicubic_u8, I3)
  evaluate_split(model, test_set, ...)                          -> {'psnr': [...], 'ssim': [...]} per held-out image,
                                                                   with labels also 'sem_acc', 'sem_miou', 'sem_valid'
  depth_absrel(depth, target)                                   -> mean |a D + b - z| / z over the pixels that have a depth,
                                                                   (a, b) the image's own least-squares fit
  depth_summary(res)                                            -> mean of 'depth_absrel' over the images that have depths
  normal_degrees(pred, target)                                  -> mean angle in degrees over the pixels that have a normal
  normal_summary(res)                                           -> mean of 'normal_deg' over the images that have normals
  semantic_summary(res)                                         -> (pixel-weighted accuracy, mean IoU) of the split
  semantic_metrics(pred, label, classes)                        -> (accuracy, mean IoU) of one label image on the device
"""
import torch
import torch.nn.functional as F

from ._lib import call, check_input
from .colormap import turbo_lut
from .datasets.ray_utils import get_ray_directions, get_rays
from .imaging import resize_u8
from .metrics import psnr, ssim
from .rendering import render_chunks

# image name -> (results key, channels of the packed image)
FRAME_OUTPUTS = {"rgb": ("rgb", 3), "opacity": ("opacity", 1), "depth": ("depth", 3), "normal": ("normal_pred", 3),
                 "normal_raw": ("normal_raw", 3), "semantic": ("semantic", 3)}
_LUTS = {}
_FINE_DIRECTIONS = {}


def colour_table(device):
    """the shipped Turbo table as a (256, 3) uint8 tensor on `device` (uploaded once per device)"""
    device = torch.device(device)
    if device not in _LUTS:
        _LUTS[device] = torch.from_numpy(turbo_lut()).to(device)
    return _LUTS[device]


@torch.no_grad()
def render_rays(model, rays_o, rays_d, chunk=131072, **render_kwargs):
    """render_chunks(test_time=True, T_threshold=1e-2) over the rays of one frame in chunks of `chunk` rays -> the
    results dictionary (per-ray tensors; `total_samples` a list, one per chunk)"""
    kwargs = {"test_time": True, "T_threshold": 1e-2}
    kwargs.update(render_kwargs)
    return render_chunks(model, rays_o.contiguous(), rays_d.contiguous(), chunk, **kwargs)


def supersampled_directions(h, w, s, K, device):
    """get_ray_directions of the int(h*s) x int(w*s) lattice of a camera with intrinsics K at (h, w), as the
    reference's loaders build them for --anti_aliasing_factor (ray_utils.py:24-27); K itself is left alone.  Cached
    per (h, w, s, K, device)."""
    K = torch.as_tensor(K, dtype=torch.float32).cpu()
    key = (int(h), int(w), float(s), tuple(K.reshape(-1).tolist()), torch.device(device))
    if key not in _FINE_DIRECTIONS:
        # a clone: get_ray_directions scales the matrix it is given in place
        _FINE_DIRECTIONS[key] = get_ray_directions(h, w, K.clone(), device=device, anti_aliasing_factor=float(s))
    return _FINE_DIRECTIONS[key]


@torch.no_grad()
def render_image(model, directions, pose, chunk=131072, anti_aliasing_factor=1.0, K=None, img_wh=None,
                 **render_kwargs):
    """One camera: render_rays of get_rays(directions, pose) (h*w rows).  With anti_aliasing_factor s > 1 the rays
    are those of the int(h*s) x int(w*s) lattice of the camera K at img_wh=(w, h) (`directions` is not used, so this
    works for every loader): int(h*s) * int(w*s) rows, to be packed and brought back with frame_images(out_wh=)."""
    if anti_aliasing_factor > 1.0:
        if K is None or img_wh is None:
            raise ValueError("anti_aliasing_factor > 1 needs the camera: K=(3, 3) intrinsics and img_wh=(w, h)")
        w, h = img_wh
        directions = supersampled_directions(h, w, anti_aliasing_factor, K, pose.device)
    rays_o, rays_d = get_rays(directions, pose)
    return render_rays(model, rays_o, rays_d, chunk, **render_kwargs)


def pack_frame(n, rgb=None, opacity=None, depth=None, depth_scale=1.0, normal_pred=None, normal_raw=None,
               rotation=None, semantic=None, classes=0, lut=None):
    """ngp_frame_pack on per-ray tensors: each input that is given yields its packed uint8 tensor ((n,3), opacity (n))
    under the names of FRAME_OUTPUTS; one launch."""
    ins = {"rgb": rgb, "opacity": opacity, "depth": depth, "normal": normal_pred, "normal_raw": normal_raw,
           "semantic": semantic}
    if all(t is None for t in ins.values()):
        raise ValueError("no input to pack")
    dev = next(t.device for t in ins.values() if t is not None)
    for name, t in ins.items():
        if t is None:
            continue
        check_input(t, name)
        want_dtype = torch.int64 if name == "semantic" else torch.float32
        rows = (n,) if name in ("opacity", "depth", "semantic") else (n, 3)
        if t.dtype != want_dtype or tuple(t.shape) != rows:
            raise ValueError(f"{name} must be {rows} {want_dtype}, got {tuple(t.shape)} {t.dtype}")
    if (normal_pred is not None or normal_raw is not None):
        if rotation is None:
            raise ValueError("normals need the camera-to-world rotation")
        check_input(rotation, "rotation")
        if rotation.dtype != torch.float32 or tuple(rotation.shape) != (3, 3):
            raise ValueError(f"rotation must be (3, 3) float32, got {tuple(rotation.shape)} {rotation.dtype}")
    if depth is not None or semantic is not None:
        lut = colour_table(dev) if lut is None else lut
        check_input(lut, "lut")
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError(f"lut must be (256, 3) uint8, got {tuple(lut.shape)} {lut.dtype}")
    if semantic is not None and int(classes) < 2:
        raise ValueError(f"semantic images need classes >= 2, got {classes}")
    out = {name: torch.empty((n,) if name == "opacity" else (n, 3), dtype=torch.uint8, device=dev)
           for name, t in ins.items() if t is not None}
    call("frame_pack", n, rgb, opacity, depth, float(depth_scale), normal_pred, normal_raw, rotation, semantic,
         int(classes), lut, *[out.get(k) for k in ("rgb", "opacity", "depth", "normal", "normal_raw", "semantic")])
    return out


@torch.no_grad()
def frame_images(results, pose, scale, num_classes=7, want=("rgb", "depth", "normal", "normal_raw", "semantic"),
                 img_wh=None, out_wh=None):
    """The 8-bit images of one frame, as the reference's render.py writes them, packed on the device in one launch:
    rgb, opacity, depth (Turbo of depth / (2 * scale)), normal / normal_raw (world -> camera through `pose`, then
    (c + 1) / 2), semantic (Turbo of label / (num_classes - 1)) -> {name: uint8 tensor}, (h*w[, 3]) rows, or
    (H, W[, 3]) with img_wh=(W, H).  With out_wh=(w, h) other than img_wh (a supersampled frame) every image is
    resized to (h, w[, 3]) as PIL's Image.resize(out_wh, BICUBIC) would, on the device (imaging.resize_u8); a label
    image cannot be averaged, so `semantic` is refused then."""
    unknown = [w for w in want if w not in FRAME_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown frame outputs {unknown}; known: {sorted(FRAME_OUTPUTS)}")
    resize = out_wh is not None and (img_wh is None or tuple(out_wh) != tuple(img_wh))
    if resize and img_wh is None:
        raise ValueError("out_wh needs img_wh, the size the frame was rendered at")
    if resize and "semantic" in want:
        raise ValueError("a semantic image cannot be resampled: labels do not average")
    n = results["rgb"].shape[0]
    ins = {}
    for name in want:
        t = results[FRAME_OUTPUTS[name][0]]
        ins[name] = (t.reshape(n) if name == "semantic" else t).contiguous()
    rot = None
    if "normal" in ins or "normal_raw" in ins:
        rot = torch.as_tensor(pose, dtype=torch.float32, device=results["rgb"].device)[:3, :3].contiguous()
    out = pack_frame(n, rgb=ins.get("rgb"), opacity=ins.get("opacity"), depth=ins.get("depth"),
                     depth_scale=2 * float(scale), normal_pred=ins.get("normal"), normal_raw=ins.get("normal_raw"),
                     rotation=rot, semantic=ins.get("semantic"), classes=num_classes)
    if img_wh is not None:
        w, h = img_wh
        out = {k: v.reshape((h, w) + tuple(v.shape[1:])) for k, v in out.items()}
    if resize:
        out = {k: resize_u8(v, out_wh) for k, v in out.items()}
    return out


@torch.no_grad()
def image_metrics(rgb, gt, img_wh):
    """(psnr, ssim) of one rendered image against its ground truth, both (h*w, 3): rgb is clamped to [0, 1] first, as
    the reference's validation step does -> two 0-dim tensors on the device (no read-back) and the clamped image"""
    rgb = rgb.clamp(0, 1)
    gt = gt.to(rgb.device).contiguous()
    return psnr(rgb, gt), ssim(rgb, gt, img_wh=img_wh), rgb


@torch.no_grad()
def semantic_metrics(pred, label, classes):
    """(accuracy, mean IoU) of predicted classes against a label image, both (h*w) integers, as two 0-dim tensors on the
    device.  A pixel is valid iff 0 <= label < classes (256, 255, ... are ignored, as in the loss).  accuracy: share of the
    valid pixels whose prediction equals the label; mean IoU: over the classes that occur in the label or the prediction
    among the valid pixels.  Both from ONE bincount of label * classes + pred; NaN when no pixel is valid."""
    C = int(classes)
    pred = pred.reshape(-1).to(torch.int64)
    label = label.reshape(-1).to(pred.device, torch.int64)
    valid = (label >= 0) & (label < C)
    # invalid pixels land in one extra bin behind the C * C cells
    cell = torch.where(valid, label.clamp(0, C - 1) * C + pred.clamp(0, C - 1), C * C)
    conf = torch.bincount(cell, minlength=C * C + 1)[:C * C].reshape(C, C).to(torch.float64)   # [label, prediction]
    hit = conf.diagonal()
    union = conf.sum(0) + conf.sum(1) - hit
    seen = union > 0
    iou = torch.where(seen, hit / union.clamp(min=1), torch.zeros_like(hit))
    return hit.sum() / conf.sum(), iou.sum() / seen.sum()


def semantic_summary(res):
    """(accuracy over all valid pixels of the split, mean IoU over the images that have valid pixels) from evaluate_split's
    dictionary; images without a valid label (sem_acc NaN) take no part; (None, None) when no image has one"""
    rows = [(a, m, n) for a, m, n in zip(res["sem_acc"], res["sem_miou"], res["sem_valid"]) if n > 0]
    if not rows:
        return None, None
    total = sum(n for _, _, n in rows)
    return sum(a * n for a, _, n in rows) / total, sum(m for _, m, _ in rows) / len(rows)


def normal_summary(res):
    """mean of evaluate_split's 'normal_deg' over the images that have pixels with a normal (NaN entries take no part);
    None when no image has one"""
    rows = [d for d in res["normal_deg"] if d == d]
    return sum(rows) / len(rows) if rows else None


def depth_summary(res):
    """mean of evaluate_split's 'depth_absrel' over the images that have pixels with a depth (NaN entries take no part);
    None when no image has one"""
    rows = [d for d in res["depth_absrel"] if d == d]
    return sum(rows) / len(rows) if rows else None


@torch.no_grad()
def depth_absrel(depth, target):
    """absolute relative error of a rendered depth image against a monocular depth map, both (h*w): with z = target / 25
    (NeRFLoss._depth_mono's unit) and the pixels with z > 0 valid, (a, b) is the least-squares scale and shift of
    a depth + b ~ z over the valid pixels (Cramer's rule in float64, a singular system gives (0, 0)), and the result the mean
    of |a depth + b - z| / z over them -> 0-dim tensor on depth's device; NaN when no pixel is valid.  No host read."""
    D = depth.reshape(-1).to(torch.float64)
    z = target.reshape(-1).to(D.device, torch.float64) / 25
    valid = z > 0
    zero = torch.zeros_like(D)
    d, t = torch.where(valid, D, zero), torch.where(valid, z, zero)
    n = valid.sum().to(torch.float64)
    s_dd, s_d, s_dz, s_z = (d * d).sum(), d.sum(), (d * t).sum(), t.sum()
    det = s_dd * n - s_d * s_d
    safe = torch.where(det == 0, torch.ones_like(det), det)
    a = torch.where(det == 0, torch.zeros_like(det), (n * s_dz - s_d * s_z) / safe)
    b = torch.where(det == 0, torch.zeros_like(det), (s_dd * s_z - s_d * s_dz) / safe)
    rel = torch.where(valid, (a * D + b - z).abs() / torch.where(valid, z, torch.ones_like(z)), zero)
    return (rel.sum() / n).to(torch.float32)       # (0 / 0 = NaN: no such pixel)


@torch.no_grad()
def normal_degrees(pred, target):
    """mean angle in degrees between predicted and target normals, both (h*w, 3) and normalised here, over the pixels
    whose target is non-zero ((0, 0, 0): the pixel has no normal) -> 0-dim tensor on pred's device; NaN when there is none"""
    target = target.reshape(-1, 3).to(pred.device, torch.float32)
    pred = pred.reshape(-1, 3).to(torch.float32)
    have = (target != 0).any(-1)
    cos = (F.normalize(pred, dim=-1) * F.normalize(target, dim=-1)).sum(-1).clamp(-1.0, 1.0)
    ang = torch.rad2deg(torch.acos(cos))
    return torch.where(have, ang, torch.zeros_like(ang)).sum() / have.sum()       # (0 / 0 = NaN: no such pixel)


@torch.no_grad()
def evaluate_split(model, test_set, chunk=131072, on_image=None, **render_kwargs):
    """Per-image PSNR and SSIM of a held-out split through render(test_time=True) (train.py:347-392): rgb is clamped
    to [0, 1] and compared with the split's ground truth -> {'psnr': [floats], 'ssim': [floats]}.  `on_image(i, rgb,
    results)` is called with each clamped (h*w, 3) image and its results dictionary (to save frames).  The metrics stay
    on the device until every image is rendered: one read-back at the end.  When a test item carries 'label' the
    dictionary also holds 'sem_acc' and 'sem_miou' (semantic_metrics of results['semantic'] with render_kwargs'
    num_classes, default 7), one per image, NaN for an image without a valid label, and 'sem_valid', the number of valid
    pixels of each image (the weights of an accuracy over the split; semantic_summary forms it).  When the split has
    `normals` (test items carry no 'normal', the reference's rule in datasets/base.py: test_set.normals[i] is read) the
    dictionary also holds 'normal_deg', normal_degrees of results['normal_pred'] per image (NaN: no pixel has a normal).
    When the split has `depths_2d` (read as test_set.depths_2d[i], like the normals) it also holds 'depth_absrel',
    depth_absrel of results['depth'] per image (NaN: no pixel has a depth).  When a test item carries 'exposure' (HDR-NeRF
    data) and the model is tone-mapped (rgb_act='None'), that image is rendered at its exposure time, unless render_kwargs
    names an exposure itself."""
    psnrs, ssims, accs, mious, valids, degs, rels = [], [], [], [], [], [], []
    classes = render_kwargs.get("num_classes", 7)
    for i in range(len(test_set)):
        s = test_set[i]
        if "rgb" not in s:
            raise ValueError("the split has no ground-truth images to evaluate against")
        kw = render_kwargs
        if "exposure" in s and getattr(model, "rgb_act", "Sigmoid") == "None" and "exposure" not in render_kwargs:
            # HDR-NeRF data: one exposure time per test image, every sample's (a (1, 1) tensor is not expanded per ray)
            kw = dict(render_kwargs, exposure=torch.as_tensor(s["exposure"], dtype=torch.float32)
                      .to(s["pose"].device).reshape(1, 1))
        results = render_image(model, test_set.directions, s["pose"], chunk, **kw)
        p, q, rgb = image_metrics(results["rgb"], s["rgb"], test_set.img_wh)
        psnrs.append(p)
        ssims.append(q)
        if "label" in s:
            a, m = semantic_metrics(results["semantic"], s["label"], classes)
            accs.append(a)
            mious.append(m)
            lab = s["label"].reshape(-1)
            valids.append(((lab >= 0) & (lab < classes)).sum().to(a.device))
        if hasattr(test_set, "normals"):
            degs.append(normal_degrees(results["normal_pred"], test_set.normals[i]))
        if hasattr(test_set, "depths_2d"):
            rels.append(depth_absrel(results["depth"], test_set.depths_2d[i]))
        if on_image is not None:
            on_image(i, rgb, results)
    if not psnrs:
        return {"psnr": [], "ssim": []}
    out = {"psnr": torch.stack(psnrs).tolist(), "ssim": torch.stack(ssims).tolist()}
    if accs:
        out.update(sem_acc=torch.stack(accs).tolist(), sem_miou=torch.stack(mious).tolist(),
                   sem_valid=torch.stack(valids).tolist())
    if degs:
        out["normal_deg"] = torch.stack(degs).tolist()
    if rels:
        out["depth_absrel"] = torch.stack(rels).tolist()
    return out
