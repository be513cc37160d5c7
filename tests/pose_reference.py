"""Restatements for the pose-refinement kernels, in torch, at the dtype of their inputs (float64: the truth; float32: the
yardstick of what float32 arithmetic costs).  Gradients come from autograd.

  rodrigues / pose_rays     the reference's formulas: axisangle_to_R (datasets/ray_utils.py:78-104), R' = Rd Rp,
                            t' = t + dT (train.py:143-149), get_rays (ray_utils.py:50-74) with the fixed-order dot product
  pose_grads                dL/ddR, dL/ddT of  sum_s g_x[s] . (o + t_s d) + g_dir[s] . d  over the samples of rays_a
                            (x_s = o + t_s d, dir_s = d; ts and rays_a constants)
  dir_encoding / sh_grads   normalize(eps=1e-6) -> (.+1)/2 -> SH degree 4 (networks.py:198,222), and dL/dd of it
"""
import numpy as np
import torch


def rodrigues(v):
    """(n, 3) -> (n, 3, 3), the literal formula of axisangle_to_R"""
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(-1, 3, 3)
    th = (v.norm(dim=1) + 1e-7)[:, None, None]
    eye = torch.eye(3, dtype=v.dtype)
    return eye + torch.sin(th) / th * K + (1 - torch.cos(th)) / th ** 2 * (K @ K)


def pose_rays(poses, dR, dT, directions, img, pix):
    """-> rays_o, rays_d (n_rays, 3); a ray whose image or pixel index is out of range is zero"""
    n_imgs, n_pix = poses.shape[0], directions.shape[0]
    ok = (img >= 0) & (img < n_imgs) & (pix >= 0) & (pix < n_pix)
    i, p = img.clamp(0, n_imgs - 1), pix.clamp(0, n_pix - 1)
    R = rodrigues(dR[i]) @ poses[i][:, :, :3]
    d = directions[p]
    rays_d = (R[:, :, 0] * d[:, 0:1] + R[:, :, 1] * d[:, 1:2]) + R[:, :, 2] * d[:, 2:3]
    rays_o = poses[i][:, :, 3] + dT[i]
    return rays_o * ok[:, None], rays_d * ok[:, None]


def pose_grads(poses, dR, dT, directions, img, pix, rays_a, ts, g_x, g_dir, dtype):
    """every array a numpy array; -> (g_dR, g_dT) as float64 numpy arrays, computed at `dtype`.  rays_a rows whose ray index
    is out of range, whose count is <= 0, or whose samples fall outside [0, N) contribute nothing (for those samples)."""
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    poses, directions, ts, g_x = T(poses), T(directions), T(ts), T(g_x)
    g_dir = None if g_dir is None else T(g_dir)
    dR, dT = T(dR).requires_grad_(True), T(dT).requires_grad_(True)
    img, pix = torch.from_numpy(img), torch.from_numpy(pix)
    o, d = pose_rays(poses, dR, dT, directions, img, pix)
    n_rays, N = img.shape[0], ts.shape[0]
    ray_of = torch.full((N,), -1, dtype=torch.int64)
    for ray, s, c in np.asarray(rays_a):
        if c > 0 and 0 <= ray < n_rays:
            ray_of[max(s, 0):min(s + c, N)] = int(ray)
    live = ray_of >= 0
    r = ray_of[live]
    x = o[r] + ts[live][:, None] * d[r]
    loss = (g_x[live] * x).sum()
    if g_dir is not None:
        loss = loss + (g_dir[live] * d[r]).sum()
    if not live.any():
        return np.zeros(dR.shape), np.zeros(dT.shape)
    loss.backward()
    return dR.grad.double().numpy(), dT.grad.double().numpy()


def sh4(u):
    """SH degree 4 of unit-range coordinates u in [-1, 1] (n, 3) -> (n, 16): tcnn's basis"""
    x, y, z = u.unbind(-1)
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999,
        -1.0925484305920792 * xz, 0.54627421529603959 * x2 - 0.54627421529603959 * y2,
        0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z2), 1.4453057213202769 * z * (x2 - y2),
        0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def dir_encoding(d):
    """(n, 3) raw directions -> (n, 16): F.normalize(eps=1e-6), remap to [0, 1], SH (which maps back to [-1, 1])"""
    dn = torch.nn.functional.normalize(d, p=2, dim=-1, eps=1e-6)
    return sh4((dn + 1) / 2 * 2 - 1)


def sh_grads(d, dL_dy, dtype):
    """numpy in, float64 numpy out: dL/dd of sum(dL_dy * dir_encoding(d)) computed at `dtype`"""
    d = torch.from_numpy(np.asarray(d)).to(dtype).requires_grad_(True)
    (torch.from_numpy(np.asarray(dL_dy)).to(dtype) * dir_encoding(d)).sum().backward()
    return d.grad.double().numpy()


# ---------------------------------------------------------------------------- shared cases
ANGLES = (0.0, 1e-7, 1e-4, 1e-2, 1.0, float(np.pi - 0.1))
COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 1024)
H = W = 12


def make_cameras(n_imgs, seed, angles=ANGLES, zero=False):
    """poses (n_imgs, 3, 4) on a sphere of radius 1.5 looking inward, dR of the lengths `angles` (cycled over the images,
    random axes), dT ~ 0.05 N(0, 1), directions of a 12 x 12 pinhole image -> float32 numpy arrays"""
    g = np.random.default_rng(seed)
    pos = g.standard_normal((n_imgs, 3))
    pos = 1.5 * pos / np.linalg.norm(pos, axis=1, keepdims=True)
    fwd = -pos / np.linalg.norm(pos, axis=1, keepdims=True)
    up = g.standard_normal((n_imgs, 3))
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    down = np.cross(fwd, right)
    poses = np.stack([right, down, fwd, pos], -1).astype(np.float32)
    axis = g.standard_normal((n_imgs, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    dR = (axis * np.array([angles[i % len(angles)] for i in range(n_imgs)])[:, None]).astype(np.float32)
    dT = (0.05 * g.standard_normal((n_imgs, 3))).astype(np.float32)
    if zero:
        dR[:], dT[:] = 0, 0
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    f = 0.5 * W / np.tan(0.5 * 0.69)
    directions = np.stack([(u - W / 2 + 0.5) / f, (v - H / 2 + 0.5) / f, np.ones_like(u)], -1).reshape(-1, 3).astype(np.float32)
    return poses, dR, dT, directions


def make_segments(n_rays, seed):
    """rays_a (n_rays, 3) int64 and N: counts from COUNTS (0 and 1024 among them from 7 rays on), segments in row order with
    ONE gap of 5 sample rows that no ray owns (from 7 rays on), ray indices a permutation"""
    g = np.random.default_rng(seed)
    p = np.array([2, 2, 2, 2, 2, 2, 2, 2, 0.15])
    counts = g.choice(COUNTS, size=n_rays, p=p / p.sum())
    if n_rays == 1:
        counts[:] = 33
    if n_rays >= 7:
        counts[[0, n_rays // 2, n_rays - 1]] = 0
        counts[[1, n_rays - 2]] = (1024, 1)
    starts = np.cumsum(counts) - counts
    if n_rays >= 7:
        starts[n_rays // 2:] += 5
    perm = g.permutation(n_rays)
    return np.stack([perm, starts, counts], 1).astype(np.int64), int((starts + counts).max())


def index_patterns(n_rays, n_imgs, seed):
    """{name: img (n_rays) int64}: one image, random, sorted runs, some out of range"""
    g = np.random.default_rng(seed)
    rnd = g.integers(0, n_imgs, n_rays).astype(np.int64)
    bad = rnd.copy()
    bad[::3] = np.where(np.arange(len(bad[::3])) % 2 == 0, n_imgs, -1)
    return {"one_image": np.full(n_rays, n_imgs // 2, np.int64), "random": rnd, "sorted": np.sort(rnd), "out_of_range": bad}


def rel_err(got, want):
    """largest |got - want| relative to the largest |want| (0 when want is all zero and got equals it)"""
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    return (err / scale if scale > 0 else err), scale

