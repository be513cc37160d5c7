"""Numpy restatement of Pillow's 8-bit antialiased bicubic resize (libImaging/Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc), the yardstick of ngp_resize_bicubic_u8.
Independent of the package: taps in plain Python floats (IEEE double, the operations in Pillow's order), the two
passes in int32 numpy.  tests/test_resample_host.py holds it against Pillow itself and against recorded Pillow output
(tests/golden/g16_pillow_bicubic.npz)."""
import math

import numpy as np

PRECISION_BITS = 22


def keys_cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def taps(n_in, n_out):
    """-> kk (n_out, ksize) int32, bounds (n_out, 2) int32 = (xmin, xmax), ksize"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((n_out, ksize), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                 # int(): truncation, as the C cast
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [keys_cubic((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        total = 0.0
        for w in k:
            total += w
        if total != 0.0:
            k = [w / total for w in k]
        for x, w in enumerate(k):
            kk[xx, x] = int(w * (1 << PRECISION_BITS) + (0.5 if w >= 0 else -0.5))
        bounds[xx] = (xmin, xmax)
    return kk, bounds, ksize


def _pass(img, n_out, axis):
    """one pass along `axis` (0 or 1) of an (H, W, C) uint8 image"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    kk, bounds, _ = taps(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, xmax = bounds[xx]
        w = kk[xx, :xmax].reshape((-1,) + (1,) * (src.ndim - 1))
        acc = np.int32(1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + xmax] * w).sum(0, dtype=np.int32)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_bicubic_u8(img, out_wh):
    """(H, W) or (H, W, C) uint8 -> (out_h, out_w[, C]): columns are resampled first (the horizontal pass) into an
    8-bit intermediate, then rows"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    out_w, out_h = out_wh
    x = img if img.ndim == 3 else img[..., None]
    x = _pass(_pass(x, out_w, 1), out_h, 0)
    return x if img.ndim == 3 else x[..., 0]


# the shapes the tests share: (in_h, in_w, out_h, out_w)
SHAPES = [(16, 16, 8, 8), (12, 18, 8, 12), (33, 47, 22, 31), (64, 40, 16, 10), (65, 65, 9, 9), (7, 5, 1, 1),
          (30, 20, 30, 10), (20, 30, 10, 30), (8, 8, 12, 12), (1, 9, 1, 3)]


def make_input(seed, h, w, c, kind):
    """a seeded test image: "random" bytes, "binary" 0/255 noise (both clip ends, the largest accumulators) or
    constant 255; (h, w) for one channel, else (h, w, c)"""
    g = np.random.default_rng(seed)
    if kind == "random":
        img = g.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif kind == "binary":
        img = (g.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)
    else:
        img = np.full((h, w, c), 255, np.uint8)
    return img[..., 0] if c == 1 else img
