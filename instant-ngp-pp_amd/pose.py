"""Camera pose refinement, the reference's --optimize_ext (train.py:143-149, 225-230): a per-image axis-angle rotation dR
and translation dT trained beside the field,
    R' = axisangle_to_R(dR[img]) @ poses[img][:, :3],  t' = poses[img][:, 3] + dT[img],  rays = get_rays(directions[pix], [R' | t']).
The rays of a batch come from ngp_pose_rays_fwd (one launch) and their adjoint, reduced per image, from ngp_pose_rays_bwd
(one launch).

What the gradient is.  The reference runs its marcher under torch.no_grad() (models/rendering.py:207-212), so the backward
of RayMarcher (custom_functions.py:104-114) is never reached there and dR, dT stay where they start.  PoseRefiner builds the
gradient that backward was written for: the sample depths `ts`, the step lengths, the segments `rays_a` and the near clamp
are constants, the sample positions are x_s = o + t_s d and the sample directions dir_s = d.
"""
import torch
from torch import nn
from torch.autograd import Function

from ._lib import call
from .datasets.ray_utils import axisangle_to_R

_f32 = torch.float32


def _pose_bwd(ref, g_x, g_dir, ts, rays_a, img_idxs, pix_idxs):
    """-> (g_dR, g_dT) for autograd, or (None, None) when a trainer registered `grad_sink` (the kernel then adds straight
    into the trainer's gradient buffer)"""
    sink = ref.grad_sink
    if sink is None:
        g_dR, g_dT = torch.zeros_like(ref.dR), torch.zeros_like(ref.dT)
        out = (g_dR, g_dT)
    else:
        (g_dR, g_dT), out = sink, (None, None)
    call("pose_rays_bwd", g_x, g_dir, ts, rays_a, ref.poses, ref.dR.detach(), ref.directions, img_idxs, pix_idxs,
         ref.poses.shape[0], ref.directions.shape[0], rays_a.shape[0], g_x.shape[0], g_dR, g_dT)
    return out


class _PoseRaysFn(Function):
    """(dR, dT) -> rays_o, rays_d (n_rays, 3) of the (image, pixel) pairs.  The backward is ngp_pose_rays_bwd on one-sample
    segments: g_x = dL/drays_o, t = 0, g_dir = dL/drays_d."""

    @staticmethod
    def forward(ctx, dR, dT, ref, img_idxs, pix_idxs):
        n = img_idxs.shape[0]
        rays_o = torch.empty(n, 3, dtype=_f32, device=dR.device)
        rays_d = torch.empty(n, 3, dtype=_f32, device=dR.device)
        call("pose_rays_fwd", ref.poses, dR, dT, ref.directions, img_idxs, pix_idxs, ref.poses.shape[0],
             ref.directions.shape[0], n, rays_o, rays_d)
        ctx.ref = ref
        ctx.save_for_backward(img_idxs, pix_idxs)
        ctx.set_materialize_grads(False)
        return rays_o, rays_d

    @staticmethod
    def backward(ctx, g_o, g_d):
        img_idxs, pix_idxs = ctx.saved_tensors
        n = img_idxs.shape[0]
        dev = img_idxs.device
        if g_o is None and g_d is None:
            return None, None, None, None, None
        g_o = torch.zeros(n, 3, dtype=_f32, device=dev) if g_o is None else g_o.contiguous()
        r = torch.arange(n, dtype=torch.int64, device=dev)
        rays_a = torch.stack([r, r, torch.ones_like(r)], 1).contiguous()
        ts = torch.zeros(n, dtype=_f32, device=dev)
        g_dR, g_dT = _pose_bwd(ctx.ref, g_o, None if g_d is None else g_d.contiguous(), ts, rays_a, img_idxs, pix_idxs)
        return g_dR, g_dT, None, None, None


class _PoseSamplesFn(Function):
    """Ties the marcher's samples (computed without a graph from the rays' values) to (dR, dT): the outputs are xyzs and
    dirs themselves, and their gradients go through ngp_pose_rays_bwd — the per-ray sums of RayMarcher.backward and the
    chain to dR, dT in one launch."""

    @staticmethod
    def forward(ctx, dR, dT, ref, xyzs, dirs, ts, rays_a, img_idxs, pix_idxs):
        ctx.ref = ref
        ctx.save_for_backward(ts, rays_a, img_idxs, pix_idxs)
        ctx.set_materialize_grads(False)
        return xyzs.view_as(xyzs), dirs.view_as(dirs)

    @staticmethod
    def backward(ctx, g_x, g_dir):
        ts, rays_a, img_idxs, pix_idxs = ctx.saved_tensors
        if g_x is None and g_dir is None:
            return (None,) * 9
        g_x = torch.zeros(ts.shape[0], 3, dtype=_f32, device=ts.device) if g_x is None else g_x.contiguous()
        g_dR, g_dT = _pose_bwd(ctx.ref, g_x, None if g_dir is None else g_dir.contiguous(), ts, rays_a, img_idxs, pix_idxs)
        return (g_dR, g_dT) + (None,) * 7


class PoseRefiner(nn.Module):
    """poses (n_imgs, 3, 4) camera-to-world and directions (n_pix, 3) camera-space of the training set; parameters dR, dT
    (n_imgs, 3), zeros.  Their state_dict keys 'dR', 'dT', 'poses' are the ones Lightning gives the reference's system."""

    def __init__(self, poses, directions):
        super().__init__()
        poses = torch.as_tensor(poses, dtype=_f32)
        directions = torch.as_tensor(directions, dtype=_f32)
        if poses.ndim != 3 or tuple(poses.shape[1:]) != (3, 4) or directions.ndim != 2 or directions.shape[1] != 3:
            raise ValueError(f"poses must be (n_imgs, 3, 4) and directions (n_pix, 3), got {tuple(poses.shape)} and "
                             f"{tuple(directions.shape)}")
        self.register_buffer("poses", poses.detach().clone().contiguous())
        self.register_buffer("directions", directions.detach().clone().contiguous(), persistent=False)
        n = poses.shape[0]
        self.dR = nn.Parameter(torch.zeros(n, 3, dtype=_f32, device=poses.device))
        self.dT = nn.Parameter(torch.zeros(n, 3, dtype=_f32, device=poses.device))
        self.grad_sink = None    # (g_dR, g_dT) views of a trainer's pose gradient buffer, or None: gradients go to autograd

    @staticmethod
    def _idx(t, dev):
        return torch.as_tensor(t, device=dev).to(torch.int64).reshape(-1).contiguous()

    def rays(self, img_idxs, pix_idxs):
        """-> rays_o, rays_d (n_rays, 3) of the refined cameras, differentiable w.r.t. dR and dT"""
        if not self.dR.is_cuda:
            raise RuntimeError("PoseRefiner.rays needs CUDA tensors")
        img_idxs, pix_idxs = self._idx(img_idxs, self.dR.device), self._idx(pix_idxs, self.dR.device)
        if img_idxs.shape != pix_idxs.shape:
            raise ValueError(f"{img_idxs.shape[0]} image indices for {pix_idxs.shape[0]} pixel indices")
        return _PoseRaysFn.apply(self.dR, self.dT, self, img_idxs, pix_idxs)

    def attach_samples(self, xyzs, dirs, ts, rays_a, img_idxs, pix_idxs):
        """xyzs, dirs (N, 3) of a march of rays(img_idxs, pix_idxs)'s values -> the same values, requiring a gradient that
        reaches dR and dT through ngp_pose_rays_bwd"""
        img_idxs, pix_idxs = self._idx(img_idxs, self.dR.device), self._idx(pix_idxs, self.dR.device)
        return _PoseSamplesFn.apply(self.dR, self.dT, self, xyzs.contiguous(), dirs.contiguous(), ts.contiguous(),
                                    rays_a.contiguous(), img_idxs, pix_idxs)

    def refined_poses(self):
        """(n_imgs, 3, 4): [axisangle_to_R(dR) @ R | t + dT], the reference's own formulas in torch (train.py:143-149)"""
        R = axisangle_to_R(self.dR) @ self.poses[..., :3]
        return torch.cat([R, (self.poses[..., 3] + self.dT)[..., None]], -1)


def pose_errors(poses, truth):
    """mean translation error (scene units) and mean rotation error (degrees) of poses (n, 3, 4) against truth (n, 3, 4)"""
    poses, truth = torch.as_tensor(poses, dtype=torch.float64), torch.as_tensor(truth, dtype=torch.float64)
    t_err = (poses[..., 3] - truth[..., 3]).norm(dim=-1)
    rel = poses[..., :3] @ truth[..., :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2).clamp(-1, 1)
    return float(t_err.mean()), float(torch.rad2deg(torch.acos(cos)).mean())


def perturb_poses(poses, sigma_t, deg, seed=0):
    """seeded perturbation of camera-to-world poses (n, 3, 4): a translation drawn from N(0, sigma_t^2) per axis and a
    rotation of `deg` degrees about a random axis, applied from the left as the refinement itself is"""
    g = torch.Generator().manual_seed(int(seed))
    p = torch.as_tensor(poses, dtype=_f32).detach().cpu().clone()
    n = p.shape[0]
    axis = torch.randn(n, 3, generator=g)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    R = axisangle_to_R(axis * float(torch.deg2rad(torch.tensor(float(deg)))))
    p[..., :3] = R @ p[..., :3]
    p[..., 3] += torch.randn(n, 3, generator=g) * float(sigma_t)
    return p.to(torch.as_tensor(poses).device)
