"""Image metrics with the reference's names and arguments (metrics.py:4-15)."""
import torch

from ._lib import call, call_host, check_input


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """squared error, optionally restricted to `valid_mask`; reduction "mean" -> scalar, else per element"""
    err = torch.square(image_pred - image_gt)
    err = err if valid_mask is None else err[valid_mask]
    return err.mean() if reduction == "mean" else err


@torch.no_grad()
def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """-10 log10(MSE) for images in [0, 1]"""
    return torch.log10(mse(image_pred, image_gt, valid_mask, reduction)).mul(-10.0)


SSIM_WINDOW = 11


def _ssim_shape(image_pred, image_gt, img_wh):
    """-> (count, H, W, batched) of the accepted layouts; ValueError for anything else"""
    shape = tuple(image_pred.shape)
    if tuple(image_gt.shape) != shape:
        raise ValueError(f"image_pred {shape} and image_gt {tuple(image_gt.shape)} differ in shape")
    if not shape or shape[-1] != 3:
        raise ValueError(f"images must be channel-last with 3 channels, got {shape}")
    if img_wh is None:
        if len(shape) not in (3, 4):
            raise ValueError(f"expected (H, W, 3) or (B, H, W, 3), got {shape}; pass img_wh=(W, H) for (H*W, 3) rows")
        h, w = shape[-3], shape[-2]
        batched = len(shape) == 4
    else:
        w, h = int(img_wh[0]), int(img_wh[1])
        if len(shape) not in (2, 3) or shape[-2] != h * w:
            raise ValueError(f"expected (H*W, 3) or (B, H*W, 3) with H*W = {h * w}, got {shape}")
        batched = len(shape) == 3
    if h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError(f"SSIM needs H and W >= {SSIM_WINDOW} (valid windows only), got H={h} W={w}")
    if image_pred.dtype != torch.float32 or image_gt.dtype != torch.float32:
        raise ValueError(f"images must be float32, got {image_pred.dtype} and {image_gt.dtype}")
    return (shape[0] if batched else 1), h, w, batched


@torch.no_grad()
def ssim(image_pred, image_gt, img_wh=None):
    """Mean SSIM per image for images in [0, 1] (what the reference logs through torchmetrics'
    StructuralSimilarityIndexMeasure(data_range=1), train.py:93,381-386): 11x11 Gaussian window, sigma 1.5, valid
    windows only, C1 = 0.01^2, C2 = 0.03^2, mean over window positions and channels (include/ngp_hip.h I1).

    image_pred, image_gt: (H, W, 3) or (B, H, W, 3), or (H*W, 3) / (B, H*W, 3) with img_wh=(W, H) (the loaders'
    order) — channel-last float32 CUDA tensors, the layout render() returns.  -> 0-dim or (B,) float32 tensor on the
    device; nothing is read back.  ValueError for bad shapes (checked first), RuntimeError for CPU tensors."""
    count, h, w, batched = _ssim_shape(image_pred, image_gt, img_wh)
    check_input(image_pred, "image_pred")
    check_input(image_gt, "image_gt")
    out = torch.empty(count, dtype=torch.float32, device=image_pred.device)
    if count:
        n_ws = call_host("ssim_workspace", count, h, w)
        if n_ws < 0:
            raise ValueError(f"unsupported SSIM batch: {count} images of {h}x{w}")
        partial = torch.empty(n_ws, dtype=torch.float64, device=image_pred.device)
        call("ssim", image_pred, image_gt, count, h, w, partial, out)
    return out if batched else out[0]
