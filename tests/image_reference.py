"""Yardsticks of the image kernels (include/ngp_hip.h I1, I2), in numpy.

ssim(pred, gt): float64 restatement of the SSIM definition the kernel implements (Wang et al. 2004; 11x11 separable
Gaussian, sigma 1.5, valid windows only, C1 = 0.01^2, C2 = 0.03^2, mean over window positions and channels), written
as two explicit 1-D passes.  ssim_correlate is the same definition through scipy.ndimage.correlate1d, cut to the valid
region: an independent formulation the host test holds the first one against.

pack_*: float32 restatements of ngp_frame_pack's rules in the op order the header gives (truncating uint8 conversion).
"""
import numpy as np

WINDOW = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2


def gaussian_taps():
    x = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-x * x / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def _filter_valid(img, taps):
    """img (H, W, C) float64 -> (H-10, W-10, C): rows (along W) then columns (along H), valid positions only"""
    h, w, _ = img.shape
    k = taps.size
    rows = np.zeros((h, w - k + 1, img.shape[2]))
    for t in range(k):
        rows += taps[t] * img[:, t:t + w - k + 1]
    out = np.zeros((h - k + 1, w - k + 1, img.shape[2]))
    for t in range(k):
        out += taps[t] * rows[t:t + h - k + 1]
    return out


def _ssim_from(filt, pred, gt):
    x, y = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    if x.shape != y.shape or x.ndim != 3 or x.shape[0] < WINDOW or x.shape[1] < WINDOW:
        raise ValueError(f"expected two (H, W, C) images with H, W >= {WINDOW}, got {x.shape} and {y.shape}")
    mx, my = filt(x), filt(y)
    vx = filt(x * x) - mx * mx
    vy = filt(y * y) - my * my
    cxy = filt(x * y) - mx * my
    s = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return float(s.mean())


def ssim(pred, gt):
    """mean SSIM of two (H, W, C) images in float64"""
    taps = gaussian_taps()
    return _ssim_from(lambda a: _filter_valid(a, taps), pred, gt)


def ssim_correlate(pred, gt):
    """the same through scipy.ndimage.correlate1d on the whole image, cut to the windows fully inside it"""
    from scipy.ndimage import correlate1d
    taps = gaussian_taps()
    r = WINDOW // 2

    def filt(a):
        f = correlate1d(correlate1d(a, taps, axis=1, mode="constant"), taps, axis=0, mode="constant")
        return f[r:a.shape[0] - r, r:a.shape[1] - r]
    return _ssim_from(filt, pred, gt)


# ------------------------------------------------------------------------------------------------------ frame packing
_F = np.float32


def u8(v):
    """(uint8)(clip(v, 0, 1) * 255) in float32, truncating"""
    v = np.asarray(v, _F)
    return (np.clip(v, _F(0), _F(1)) * _F(255)).astype(np.uint8)


def pack_rgb(rgb):
    return u8(rgb)


def pack_opacity(opacity):
    return u8(opacity)


def pack_depth(depth, depth_scale, lut):
    return lut[u8(np.asarray(depth, _F) / _F(depth_scale))]


def pack_normal(normal, rot):
    """normal (n,3), rot (3,3) camera-to-world rotation: n' = n + 1e-6, c_j = (n'_0 R_0j + n'_1 R_1j) + n'_2 R_2j"""
    n = np.asarray(normal, _F) + _F(1e-6)
    rot = np.asarray(rot, _F)
    c = np.stack([(n[:, 0] * rot[0, j] + n[:, 1] * rot[1, j]) + n[:, 2] * rot[2, j] for j in range(3)], 1)
    assert c.dtype == _F
    return u8((c + _F(1)) / _F(2))


def pack_semantic(label, classes, lut):
    level = _F(1.0) / _F(classes - 1)
    return lut[u8(level * np.asarray(label).astype(_F))]
