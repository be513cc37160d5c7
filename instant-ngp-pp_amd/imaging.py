"""Image-space helpers of the test-time renderer beyond one ray per pixel: supersampled (anti-aliased) frames and
panorama rays.

  bicubic_taps(n_in, n_out)         -> Pillow's 22-bit fixed-point bicubic taps and bounds of one axis (numpy, cached)
  resize_u8(img, out_wh)            -> PIL.Image.resize(out_wh, BICUBIC) of uint8 CUDA images, byte for byte, through
                                       ngp_resize_bicubic_u8 (include/ngp_hip.h I3)
  supersampled_size(h, w, s)        -> the lattice --anti_aliasing_factor s renders on (datasets/ray_utils.py:24-27)
  panorama_rays(H, W, forward, ...) -> rays of an equirectangular frame around a point (render_panorama.py:87-107)
"""
import functools
import math

import numpy as np
import torch

from ._lib import call

MAX_RATIO = 8           # n_in <= MAX_RATIO * n_out on each axis (the kernel's LDS tile is sized for it)
PRECISION_BITS = 22     # Pillow's fixed point for 8-bit images: 32 - 8 - 2
_DEVICE_TAPS = {}


@functools.lru_cache(maxsize=None)
def bicubic_taps(n_in, n_out):
    """One axis of Pillow's antialiased bicubic resize from n_in to n_out samples (Resample.c: precompute_coeffs,
    normalize_coeffs_8bpc), in float64 as Pillow computes it -> (kk (n_out, ksize) int32, bounds (n_out, 2) int32 =
    (first input sample, taps used), ksize).  The arrays are cached and read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) / fs)
    a = -0.5
    k = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1,
                 np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
    k = np.where(x < xmax[:, None], k, 0.0)
    total = np.zeros(n_out, dtype=np.float64)
    for j in range(ksize):          # in order, as the C loop adds them (np.sum adds pairwise)
        total = total + k[:, j]
    nonzero = total != 0.0
    k[nonzero] = k[nonzero] / total[nonzero, None]
    one = float(1 << PRECISION_BITS)
    kk = np.where(k < 0, np.trunc(-0.5 + k * one), np.trunc(0.5 + k * one)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    kk.setflags(write=False)
    bounds.setflags(write=False)
    return kk, bounds, ksize


def _device_taps(n_in, n_out, device):
    """the taps of one axis on `device` (uploaded once per sizes and device); (None, None, 0) for an unchanged axis"""
    if n_in == n_out:
        return None, None, 0
    key = (n_in, n_out, device)
    if key not in _DEVICE_TAPS:
        kk, bounds, ksize = bicubic_taps(n_in, n_out)
        _DEVICE_TAPS[key] = (torch.from_numpy(kk.copy()).to(device), torch.from_numpy(bounds.copy()).to(device), ksize)
    return _DEVICE_TAPS[key]


@torch.no_grad()
def resize_u8(img, out_wh):
    """PIL.Image.resize(out_wh, Image.Resampling.BICUBIC) of 8-bit images on the device, byte for byte: img a
    contiguous uint8 CUDA tensor (H, W), (H, W, C) or (B, H, W, C) with C 1 or 3 -> the same rank at (out_h, out_w).
    ValueError for another dtype, layout or channel count, or for more than 8 input samples per output sample."""
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        raise ValueError(f"img must be a uint8 tensor, got {getattr(img, 'dtype', type(img))}")
    if img.dim() not in (2, 3, 4):
        raise ValueError(f"img must be (H, W), (H, W, C) or (B, H, W, C), got {tuple(img.shape)}")
    if not img.is_contiguous():
        raise ValueError("img must be contiguous")
    if not img.is_cuda:
        raise RuntimeError("img must be a CUDA tensor")
    out_w, out_h = int(out_wh[0]), int(out_wh[1])
    count = img.shape[0] if img.dim() == 4 else 1
    channels = 1 if img.dim() == 2 else img.shape[-1]
    in_h, in_w = (img.shape[0], img.shape[1]) if img.dim() < 4 else (img.shape[1], img.shape[2])
    if channels not in (1, 3):
        raise ValueError(f"img must have 1 or 3 channels, got {channels}")
    if min(in_h, in_w, out_h, out_w) < 1:
        raise ValueError(f"sizes must be positive, got {in_h}x{in_w} -> {out_h}x{out_w}")
    if in_h > MAX_RATIO * out_h or in_w > MAX_RATIO * out_w:
        raise ValueError(f"at most {MAX_RATIO} input samples per output sample: {in_h}x{in_w} -> {out_h}x{out_w}")
    shape = {2: (out_h, out_w), 3: (out_h, out_w, channels), 4: (count, out_h, out_w, channels)}[img.dim()]
    out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    kx, bx, ksize_x = _device_taps(in_w, out_w, img.device)
    ky, by, ksize_y = _device_taps(in_h, out_h, img.device)
    call("resize_bicubic_u8", img, count, in_h, in_w, channels, out, out_h, out_w, kx, bx, ksize_x, ky, by, ksize_y)
    return out


def supersampled_size(h, w, s):
    """(int(h * s), int(w * s)): the lattice get_ray_directions(anti_aliasing_factor=s) lays out"""
    return int(h * s), int(w * s)


def panorama_rays(H, W, forward, down, right, origin=(0.0, 0.0, 0.0), radius=0.0, device="cpu"):
    """Rays of an equirectangular H x W frame around `origin` (render_panorama.py:87-107): longitude theta =
    (u - W/2 + 0.5) 2 pi / W from `forward` toward `right`, latitude phi = (v - H/2 + 0.5) pi / H toward `down`,
    d = sin(phi) down + cos(phi) sin(theta) right + cos(phi) cos(theta) forward, normalised; the origins are moved
    `radius` along the rays -> rays_o, rays_d (H*W, 3) float32, row-major over (v, u)."""
    f32 = dict(dtype=torch.float32, device=device)
    forward, down, right, origin = (torch.as_tensor(v, **f32).reshape(1, 3) for v in (forward, down, right, origin))
    v, u = torch.meshgrid(torch.arange(H, **f32), torch.arange(W, **f32), indexing="ij")
    thetas = ((u - W / 2 + 0.5) * 2 * torch.pi / W).reshape(-1, 1)
    phis = ((v - H / 2 + 0.5) * torch.pi / H).reshape(-1, 1)
    d = torch.sin(phis) * down + torch.cos(phis) * torch.sin(thetas) * right \
        + torch.cos(phis) * torch.cos(thetas) * forward
    rays_d = torch.nn.functional.normalize(d, p=2, dim=-1, eps=1e-9).contiguous()
    rays_o = (origin + rays_d * float(radius)).contiguous()
    return rays_o, rays_d
