"""Synthetic stand-in for NeRF-Synthetic lego (no dataset is available offline): the
"S-lego-proxy" scene of SURVEY.md §8(d).

An analytic field in [-0.5,0.5]^3 — union of three boxes and a sphere shell, sigma = 60 inside,
rgb = 0.5+0.5*sin(8*pi*x) — seen by pinhole cameras with lego's intrinsics (800x800,
camera_angle_x = 0.6911, datasets/nerf.py:33-41) on the upper hemisphere at radius 1.5
(datasets/nerf.py:48-60 normalises poses to that radius), looking at the origin.  Rays follow
datasets/ray_utils.py:8-74: camera-space directions ((u-cx+.5)/fx, (v-cy+.5)/fy, 1), rotated by
c2w, not normalised.  Ground-truth colours come from dense quadrature of the analytic field.
"""
import math

import torch

SIGMA_IN = 60.0


SKY_LABEL, IGNORE_LABEL = 4, 256   # the class losses.py:122 compares with, nn.CrossEntropyLoss's ignore_index there


def _solids(x):
    ax = x.abs()
    box1 = (ax[..., 0] < 0.35) & (ax[..., 1] < 0.10) & (ax[..., 2] < 0.10)
    box2 = (ax[..., 0] < 0.10) & (ax[..., 1] < 0.30) & ((x[..., 2] + 0.15).abs() < 0.08)
    box3 = ((x[..., 0] - 0.15).abs() < 0.08) & ((x[..., 1] + 0.1).abs() < 0.08) & (ax[..., 2] < 0.33)
    r = torch.linalg.norm(x - torch.tensor([-0.15, 0.12, 0.12], device=x.device), dim=-1)
    shell = (r < 0.2) & (r > 0.15)
    return box1, box2, box3, shell


def analytic_sigma(x):
    """x (...,3) world coordinates -> sigma (...)"""
    box1, box2, box3, shell = _solids(x)
    return torch.where(box1 | box2 | box3 | shell, SIGMA_IN, 0.0)


def analytic_part(x):
    """x (...,3) -> int64 (...): the solid a point belongs to, 0-3 for box1, box2, box3, shell (the first that contains
    it), -1 in empty space"""
    part = torch.full(x.shape[:-1], -1, dtype=torch.int64, device=x.device)
    for k, inside in reversed(list(enumerate(_solids(x)))):
        part = torch.where(inside, k, part)
    return part


# centres and half-widths of box1-3 and the shell's centre and radii, as _solids tests them
BOX_CENTRES = ((0.0, 0.0, 0.0), (0.0, 0.0, -0.15), (0.15, -0.1, 0.0))
BOX_HALVES = ((0.35, 0.10, 0.10), (0.10, 0.30, 0.08), (0.08, 0.08, 0.33))
SHELL_CENTRE, SHELL_RADII = (-0.15, 0.12, 0.12), (0.15, 0.2)


def analytic_normal(x, part):
    """outward unit normal of solid `part` (analytic_part's numbering, -1: none -> zero vector) at the surface point
    nearest to x (...,3), for x on or just inside the surface: a box's face nearest to x; the shell's outer sphere
    (+radial) or inner sphere (-radial), whichever is nearer"""
    out = torch.zeros_like(x)
    for k, (c, h) in enumerate(zip(BOX_CENTRES, BOX_HALVES)):
        rel = x - torch.tensor(c, device=x.device, dtype=x.dtype)
        axis = (rel.abs() - torch.tensor(h, device=x.device, dtype=x.dtype)).argmax(-1, keepdim=True)
        face = torch.zeros_like(x).scatter_(-1, axis, torch.sign(rel.gather(-1, axis)))
        out = torch.where((part == k)[..., None], face, out)
    rel = x - torch.tensor(SHELL_CENTRE, device=x.device, dtype=x.dtype)
    r = rel.norm(dim=-1, keepdim=True)
    radial = rel / r.clamp(min=1e-12) * torch.where(r > 0.5 * sum(SHELL_RADII), 1.0, -1.0)
    return torch.where((part == 3)[..., None], radial, out)


def analytic_rgb(x):
    return 0.5 + 0.5 * torch.sin(8 * math.pi * x)


SKY_HORIZON, SKY_ZENITH, SKY_LOBE = (0.55, 0.50, 0.40), (0.10, 0.30, 0.70), (0.40, 0.25, 0.05)
SKY_LOBE_DIR = (0.6, -0.48, 0.64)


def analytic_sky(d):
    """the colour of the background in direction d (N,3) (any length): a horizon-to-zenith gradient in the height of the
    normalised direction plus a broad warm lobe around SKY_LOBE_DIR; inside [0.1, 0.95], the clamp never acts.  Smooth and of
    low order in the direction (quadratic), so the skybox network (SH degree 3 -> 32 -> 3) can fit it."""
    u = d / d.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    c = lambda v: torch.tensor(v, device=d.device, dtype=d.dtype)
    up = 0.5 + 0.5 * u[..., 2:3]
    lobe = (0.5 + 0.5 * (u * c(SKY_LOBE_DIR)).sum(-1, keepdim=True)) ** 2
    return (c(SKY_HORIZON) + (c(SKY_ZENITH) - c(SKY_HORIZON)) * up + c(SKY_LOBE) * lobe).clamp(0.0, 1.0)


class LegoProxy:
    def __init__(self, n_images=100, img_wh=(800, 800), device="cuda", seed=20220806, radius=1.5):
        self.device = torch.device(device)
        self.img_wh = img_wh
        w, h = img_wh
        fx = fy = 0.5 * w / math.tan(0.5 * 0.6911112070083618)
        self.K = torch.tensor([[fx, 0, w / 2], [0, fy, h / 2], [0, 0, 1]], dtype=torch.float32, device=self.device)
        g = torch.Generator().manual_seed(seed)
        # upper-hemisphere camera centres, look-at origin, OpenCV axes (x right, y down, z forward)
        phi = torch.rand(n_images, generator=g) * 2 * math.pi
        cos_t = torch.rand(n_images, generator=g) * 0.9 + 0.05
        sin_t = torch.sqrt(1 - cos_t ** 2)
        pos = torch.stack([sin_t * torch.cos(phi), sin_t * torch.sin(phi), cos_t], -1) * radius
        fwd = -pos / pos.norm(dim=-1, keepdim=True)
        up = torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)
        right = torch.cross(fwd, up, dim=-1)
        right = right / right.norm(dim=-1, keepdim=True)
        down = torch.cross(fwd, right, dim=-1)
        self.poses = torch.stack([right, down, fwd, pos], -1).to(self.device)  # (n,3,4) c2w
        v, u = torch.meshgrid(torch.arange(h, device=self.device, dtype=torch.float32),
                              torch.arange(w, device=self.device, dtype=torch.float32), indexing="ij")
        self.directions = torch.stack([(u - w / 2 + 0.5) / fx, (v - h / 2 + 0.5) / fy, torch.ones_like(u)],
                                      -1).reshape(-1, 3)

    def rays(self, img_idxs, pix_idxs):
        """get_rays (ray_utils.py:50-74) for (image, pixel) pairs"""
        c2w = self.poses[img_idxs]
        d = self.directions[pix_idxs]
        rays_d = (d[:, None, :] @ c2w[:, :, :3].transpose(1, 2))[:, 0]
        rays_o = c2w[:, :, 3]
        return rays_o.contiguous(), rays_d.contiguous()

    def sample_batch(self, batch_size, generator=None):
        """random images + random pixels, as BaseDataset.__getitem__ (datasets/base.py:22-31)"""
        n_img = self.poses.shape[0]
        w, h = self.img_wh
        img = torch.randint(n_img, (batch_size,), device=self.device, generator=generator)
        pix = torch.randint(w * h, (batch_size,), device=self.device, generator=generator)
        return img, pix

    @torch.no_grad()
    def ground_truth(self, rays_o, rays_d, n_quad=1024, white_bg=False, sky=False):
        """dense quadrature of the analytic field inside the unit box -> rgb (N,3), opacity (N); sky: composited over
        analytic_sky(rays_d), a background that depends on the view direction (it takes precedence over white_bg)"""
        inv = 1.0 / rays_d
        a, b = (-0.5 - rays_o) * inv, (0.5 - rays_o) * inv
        t1 = torch.minimum(a, b).amax(-1).clamp(min=0)
        t2 = torch.maximum(a, b).amin(-1)
        hit = t2 > t1
        t2 = torch.where(hit, t2, t1)
        out_rgb = torch.zeros(len(rays_o), 3, device=rays_o.device)
        out_op = torch.zeros(len(rays_o), device=rays_o.device)
        step = (t2 - t1) / n_quad
        chunk = 16384
        for s in range(0, len(rays_o), chunk):
            sl = slice(s, s + chunk)
            k = torch.arange(n_quad, device=rays_o.device, dtype=torch.float32) + 0.5
            t = t1[sl, None] + step[sl, None] * k[None, :]
            x = rays_o[sl, None, :] + rays_d[sl, None, :] * t[..., None]
            sig = analytic_sigma(x)
            dl = step[sl, None] * rays_d[sl].norm(dim=-1, keepdim=True)
            alpha = 1 - torch.exp(-sig * dl)
            T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha], 1), 1)[:, :-1]
            w = alpha * T
            out_rgb[sl] = (w[..., None] * analytic_rgb(x)).sum(1)
            out_op[sl] = w.sum(1)
        if sky:
            out_rgb = out_rgb + analytic_sky(rays_d) * (1 - out_op)[:, None]
        elif white_bg:
            out_rgb = out_rgb + (1 - out_op)[:, None]
        return out_rgb, out_op

    @torch.no_grad()
    def ground_truth_labels(self, rays_o, rays_d, n_quad=1024):
        """per-ray class of the analytic scene by the quadrature of ground_truth -> int64 (N): the part (analytic_part,
        0-3) with the largest composited weight; SKY_LABEL (4) where the opacity is below 0.1; IGNORE_LABEL (256) where
        the ray grazes (0.1 <= opacity < 0.9) or where the best part holds less than 0.6 of the opacity"""
        inv = 1.0 / rays_d
        a, b = (-0.5 - rays_o) * inv, (0.5 - rays_o) * inv
        t1 = torch.minimum(a, b).amax(-1).clamp(min=0)
        t2 = torch.maximum(a, b).amin(-1)
        t2 = torch.where(t2 > t1, t2, t1)
        out = torch.empty(len(rays_o), dtype=torch.int64, device=rays_o.device)
        step = (t2 - t1) / n_quad
        chunk = 16384
        for s in range(0, len(rays_o), chunk):
            sl = slice(s, s + chunk)
            k = torch.arange(n_quad, device=rays_o.device, dtype=torch.float32) + 0.5
            t = t1[sl, None] + step[sl, None] * k[None, :]
            x = rays_o[sl, None, :] + rays_d[sl, None, :] * t[..., None]
            part = analytic_part(x)
            dl = step[sl, None] * rays_d[sl].norm(dim=-1, keepdim=True)
            alpha = torch.where(part >= 0, 1 - torch.exp(-SIGMA_IN * dl), torch.zeros_like(dl))
            T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha], 1), 1)[:, :-1]
            w = alpha * T
            share = torch.stack([(w * (part == c)).sum(1) for c in range(4)], -1)
            op = share.sum(-1)
            best, lab = share.max(-1)
            lab = torch.where((op < 0.9) | (best < 0.6 * op), IGNORE_LABEL, lab)
            out[sl] = torch.where(op < 0.1, SKY_LABEL, lab)
        return out

    @torch.no_grad()
    def ground_truth_normals(self, rays_o, rays_d, n_quad=1024):
        """per-ray surface normal of the analytic scene by the quadrature of ground_truth -> float32 (N, 3), world space:
        the outward unit normal (analytic_normal) of the solid the ray enters first, taken at the first quadrature point
        inside it; the zero vector (no normal: the fused normal tail and evaluate_split leave such pixels out) where the
        ray's opacity is below 0.5"""
        inv = 1.0 / rays_d
        a, b = (-0.5 - rays_o) * inv, (0.5 - rays_o) * inv
        t1 = torch.minimum(a, b).amax(-1).clamp(min=0)
        t2 = torch.maximum(a, b).amin(-1)
        t2 = torch.where(t2 > t1, t2, t1)
        out = torch.zeros(len(rays_o), 3, device=rays_o.device)
        step = (t2 - t1) / n_quad
        chunk = 16384
        for s in range(0, len(rays_o), chunk):
            sl = slice(s, s + chunk)
            k = torch.arange(n_quad, device=rays_o.device, dtype=torch.float32) + 0.5
            t = t1[sl, None] + step[sl, None] * k[None, :]
            x = rays_o[sl, None, :] + rays_d[sl, None, :] * t[..., None]
            part = analytic_part(x)
            dl = step[sl, None] * rays_d[sl].norm(dim=-1, keepdim=True)
            alpha = torch.where(part >= 0, 1 - torch.exp(-SIGMA_IN * dl), torch.zeros_like(dl))
            T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha], 1), 1)[:, :-1]
            op = (alpha * T).sum(1)
            first = (part >= 0).to(torch.int8).argmax(1)          # (the first point inside a solid; 0 if there is none)
            rows = torch.arange(len(first), device=rays_o.device)
            n = analytic_normal(x[rows, first], part[rows, first])
            out[sl] = torch.where((op >= 0.5)[:, None], n, torch.zeros_like(n))
        return out

    @torch.no_grad()
    def ground_truth_depths(self, rays_o, rays_d, n_quad=1024):
        """per-ray expected distance sum_s w_s t_s of the analytic scene by the quadrature of ground_truth -> float32 (N):
        t in units of |rays_d| as the marcher's ts are; 0 (no depth: the fused depth tail and evaluate_split leave such
        pixels out) where the ray's opacity is below 0.5"""
        inv = 1.0 / rays_d
        a, b = (-0.5 - rays_o) * inv, (0.5 - rays_o) * inv
        t1 = torch.minimum(a, b).amax(-1).clamp(min=0)
        t2 = torch.maximum(a, b).amin(-1)
        t2 = torch.where(t2 > t1, t2, t1)
        out = torch.zeros(len(rays_o), device=rays_o.device)
        step = (t2 - t1) / n_quad
        chunk = 16384
        for s in range(0, len(rays_o), chunk):
            sl = slice(s, s + chunk)
            k = torch.arange(n_quad, device=rays_o.device, dtype=torch.float32) + 0.5
            t = t1[sl, None] + step[sl, None] * k[None, :]
            x = rays_o[sl, None, :] + rays_d[sl, None, :] * t[..., None]
            part = analytic_part(x)
            dl = step[sl, None] * rays_d[sl].norm(dim=-1, keepdim=True)
            alpha = torch.where(part >= 0, 1 - torch.exp(-SIGMA_IN * dl), torch.zeros_like(dl))
            T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha], 1), 1)[:, :-1]
            w = alpha * T
            op = w.sum(1)
            out[sl] = torch.where(op >= 0.5, (w * t).sum(1), torch.zeros_like(op))
        return out

    @torch.no_grad()
    def occupancy_from_analytic(self, model, supersample=2):
        """density_grid (K, G^3, morton order) from the analytic sigma: the steady-state occupancy
        the schedule converges to, used to put the micro-benchmark straight into that regime."""
        from . import vren
        G = model.grid_size
        coords = model.grid_coords
        idx = vren.morton3D(coords).long()
        grid = torch.zeros(model.cascades, G ** 3, device=coords.device)
        for c in range(model.cascades):
            s = min(2 ** (c - 1), model.scale)
            best = torch.zeros(G ** 3, device=coords.device)
            for ox in range(supersample):
                for oy in range(supersample):
                    for oz in range(supersample):
                        off = (torch.tensor([ox, oy, oz], device=coords.device, dtype=torch.float32) + 0.5) / supersample
                        x = ((coords.float() + off) / G * 2 - 1) * s
                        best = torch.maximum(best, analytic_sigma(x))
            grid[c, idx] = best
        return grid
