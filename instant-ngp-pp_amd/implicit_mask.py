"""Transient mask field of the reference (models/implicit_mask.py:6-39, the `embed_msk` recipe): an 8-level F = 2
hash grid over uvi = (pixel row, pixel column, image index), each scaled into [-0.5, 0.5), followed by
Linear(16, 64) + ReLU + Linear(64, 1) + Sigmoid.  One mask value per RAY; NeRFLoss(embed_msk=True) weighs the colour
error of a ray with 1 - mask and keeps the mask small (losses.py:85-93, 142-151).

State-dict names and shapes are the reference's (mask_encoder.params, mask_net.0.*, mask_net.2.*); the sub-modules
only HOLD the parameters: forward and backward are one launch each (ngp_mask_field_fwd / ngp_mask_field_bwd), for every
batch size.  The backward gathers the 3.4 MB table again instead of saving the encoded features and the hidden layer.
"""
import math

import torch
from torch import nn
from torch.autograd import Function

from . import tinycudann as tcnn
from ._lib import call
from .link import FieldLink

_f32 = torch.float32


class _MaskFieldFn(Function):
    """mask (n) = field(uvi).  Gradients: into the owner's `link.grad_sinks` (a trainer's flat gradient views: the kernel
    accumulates straight into them and autograd gets None, as networks._FieldFn does) or, without sinks, handed to
    autograd."""

    @staticmethod
    def forward(ctx, uvi, table, W1, b1, W2, b2, owner):
        n = uvi.shape[0]
        mask = torch.empty(n, dtype=_f32, device=uvi.device)
        call("mask_field_fwd", owner.mask_encoder.desc, table, W1, b1, W2, b2, uvi, n, mask)
        ctx.save_for_backward(uvi, mask, table, W1, b1, W2)
        ctx.owner = owner
        return mask

    @staticmethod
    def backward(ctx, g):
        uvi, mask, table, W1, b1, W2 = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:6]):
            return (None,) * 7
        owner = ctx.owner
        sinks = owner.link.grad_sinks
        if sinks:
            out = [sinks[k] for k in ("table", "W1", "b1", "W2", "b2")]
        else:
            out = [torch.zeros_like(t) for t in (table, W1, b1, W2)] + [torch.zeros(1, dtype=_f32, device=g.device)]
        call("mask_field_bwd", owner.mask_encoder.desc, table, W1, b1, W2, uvi, mask, g.contiguous(), uvi.shape[0], *out)
        if sinks:
            return (None,) * 7
        return (None,) + tuple(t if need else None for t, need in zip(out, ctx.needs_input_grad[1:6])) + (None,)


class implicit_mask(nn.Module):
    def __init__(self, latent=32, W=128):
        """both arguments are unused, as in the reference (they belong to its retired frequency-encoded variant)"""
        super().__init__()
        self.link = FieldLink()   # a trainer's gradient sinks (link.py); empty: gradients go through autograd
        L, F, log2_T, N_min = 8, 2, 16, 16
        b = math.exp(math.log(2048 / N_min) / (L - 1))
        self.mask_encoder = tcnn.Encoding(
            n_input_dims=3,
            encoding_config={"otype": "Grid", "type": "Hash", "n_levels": L, "n_features_per_level": F,
                             "log2_hashmap_size": log2_T, "base_resolution": N_min, "per_level_scale": b,
                             "interpolation": "Linear"})
        self.mask_net = nn.Sequential(nn.Linear(self.mask_encoder.n_output_dims, 64), nn.ReLU(), nn.Linear(64, 1),
                                      nn.Sigmoid())

    def forward(self, uvi):
        """uvi (n, 3) float32 on the GPU -> mask (n, 1) in (0, 1)"""
        if not uvi.is_cuda:
            raise RuntimeError("uvi must be a CUDA tensor")
        if uvi.dim() != 2 or uvi.shape[1] != 3:
            raise ValueError("uvi must be (n, 3)")
        l1, l2 = self.mask_net[0], self.mask_net[2]
        mask = _MaskFieldFn.apply(uvi.float().contiguous(), self.mask_encoder.params, l1.weight, l1.bias, l2.weight,
                                  l2.bias, self)
        return mask.view(-1, 1)

    @staticmethod
    def uvi(uv, img_idxs, img_wh, n_imgs):
        """the field's input for a ray batch (train.py:281-287): uv (n, 2) = (pixel row, pixel column) as the datasets
        emit it, img_idxs (n), img_wh = (w, h), n_imgs = number of training images -> (n, 3) float32 in [-0.5, 0.5)"""
        w, h = img_wh
        uv, img_idxs = torch.as_tensor(uv), torch.as_tensor(img_idxs, device=torch.as_tensor(uv).device)
        out = torch.zeros((uv.shape[0], 3), dtype=_f32, device=uv.device)
        out[:, 0] = (uv[:, 0] - h / 2) / h
        out[:, 1] = (uv[:, 1] - w / 2) / w
        out[:, 2] = (img_idxs - n_imgs / 2) / n_imgs
        return out
