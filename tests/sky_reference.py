"""Float64 restatement of the skybox (csrc/sky_kernels.hip: ngp_skybox_fwd / ngp_skybox_bwd), and the per-ray
background of the fused tail (ngp_render_loss_fused_sky) on tests/fused_tail_reference.py.

The skybox, per ray, with params the network's 1024 floats, W1 (32,16) row-major then W2 (16,32):
    u = d / |d|,  x = (u + 1) / 2,  y_0..8 = the degree-3 real SH basis of 2 x - 1 (ngp_sh_fwd's polynomial forms),
    z_j = sum_{k<9} W1[j][k] y_k + sum_{k=9..15} W1[j][k],  rgb_c = sigmoid(sum_j W2[c][j] relu(z_j)), c < 3.
The backward is stated by hand (dt_c = g_c rgb_c (1 - rgb_c), dz_j = [z_j > 0] sum_c dt_c W2[c][j], dW2[c][j] = sum dt_c
relu(z_j), dW1[j][k<9] = sum dz_j y_k, dW1[j][9..15] = sum dz_j, rows 3..15 of dW2 zero) and checked against torch autograd
of the same forward in tests/test_sky_host.py.

The tail needs no new arithmetic: fused_tail_reference.finish broadcasts x['bg'], so a copy of the batch whose bg holds
the background of every ROW gives every default output, and d_bg = g_rgb (1 - opacity) follows from the seeds it returns."""
import numpy as np
import torch

import fused_tail_reference as R

N_PARAMS = 1024
W2_AT = 512


def basis(d, dtype=torch.float64):
    """(n,3) raw directions -> (n,9)"""
    d = torch.as_tensor(np.asarray(d)).to(dtype)
    u = d / torch.linalg.norm(d, dim=1, keepdim=True)
    v = (u + 1) / 2 * 2 - 1
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return torch.stack([torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
                        -0.48860251190291987 * x, 1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
                        0.94617469575755997 * z * z - 0.31539156525251999, -1.0925484305920792 * x * z,
                        0.54627421529603959 * x * x - 0.54627421529603959 * y * y], 1)


def forward_t(params, d, dtype=torch.float64):
    """torch forward (differentiable w.r.t. params, a (1024) tensor of `dtype`) -> (rgb (n,3), z (n,32))"""
    W1, W2 = params[:W2_AT].reshape(32, 16), params[W2_AT:].reshape(16, 32)
    y = basis(d, dtype)
    z = y @ W1[:, :9].T + W1[:, 9:].sum(1)
    return torch.sigmoid(torch.relu(z) @ W2[:3].T), z


def forward(params, d):
    """-> rgb (n,3) float64"""
    return forward_t(torch.from_numpy(np.asarray(params, np.float64)), d)[0].numpy()


def backward(params, d, g):
    """the hand-stated backward -> dparams (1024) float64"""
    p = np.asarray(params, np.float64)
    W2 = p[W2_AT:].reshape(16, 32)
    rgb, z = (t.numpy() for t in forward_t(torch.from_numpy(p), d))
    y = basis(d).numpy()
    dt = np.asarray(g, np.float64) * rgb * (1 - rgb)
    h = np.maximum(z, 0)
    dz = (z > 0) * (dt @ W2[:3])
    dW1 = np.zeros((32, 16))
    dW1[:, :9] = dz.T @ y
    dW1[:, 9:] = dz.sum(0)[:, None]
    dW2 = np.zeros((16, 32))
    dW2[:3] = dt.T @ h
    return np.concatenate([dW1.ravel(), dW2.ravel()])


def min_preact_margin(params, d):
    """min |z_j| over rays and hidden units: how far the inputs stay from the ReLU's kink"""
    z = forward_t(torch.from_numpy(np.asarray(params, np.float64)), d)[1].numpy()
    return float(np.abs(z[np.isfinite(z)]).min()) if z.size else np.inf


def directions(n, seed=0):
    """n seeded directions: the axes and the negated axes first, then normal draws at lengths 1e-3 to 1e3 (non-unit)"""
    g = np.random.default_rng(8100 + seed)
    d = g.standard_normal((n, 3)) * 10.0 ** g.uniform(-3, 3, (n, 1))
    axes = np.concatenate([np.eye(3), -np.eye(3)]) * np.array([[1.0], [2.5], [0.01], [1.0], [40.0], [0.3]])
    d[:min(n, 6)] = axes[:n]
    return d.astype(np.float32)


def dead_unit_params(seed=0, n_dead=5):
    """a seeded parameter set with `n_dead` hidden units that no direction switches on: their nine weights are small and
    their padding columns sum to -7, below any |y| <= 1.1 can lift; the other units' padding columns are positive, so each
    of them is on for some directions.  -> (params float32 (1024), the dead units)"""
    g = np.random.default_rng(8200 + seed)
    p = (g.uniform(-1, 1, N_PARAMS) * 0.6).astype(np.float32)
    W1 = p[:W2_AT].reshape(32, 16)
    dead = np.sort(g.choice(32, n_dead, replace=False))
    W1[:, 9:] = np.abs(W1[:, 9:])          # every other unit is on for some directions (and off for others)
    W1[dead, :9] *= 0.1
    W1[dead, 9:] = -1.0
    return p, dead


# ------------------------------------------------------------------------------------------------ the tail
def sky_batch(x, seed=0):
    """a seeded background colour for every ray of a fused_tail_reference batch -> (n_rays, 3) float32"""
    return np.random.default_rng(8300 + seed).random((x["n_rays"], 3)).astype(np.float32)


def by_row(x, rgb_bg, n_rays=None):
    """a copy of the batch whose bg holds the background of every row of rays_a (what finish() broadcasts)"""
    y = dict(x)
    y["bg"] = np.asarray(rgb_bg)[x["rays_a"][:n_rays, 0]]
    return y


def with_d_bg(ref, x, n_rays=None):
    """adds d_bg (n_rays_total, 3), indexed by ray, NaN where no processed row names the ray: g_rgb (1 - opacity)"""
    rows = x["rays_a"][:n_rays]
    d = np.full((x["n_rays"], 3), np.nan)
    d[rows[:, 0]] = ref["g_rgb"] * (1 - ref["opacity"][rows[:, 0]])[:, None]
    out = dict(ref)
    out["d_bg"] = d
    return out


def evaluate(x, rgb_bg, dtype=torch.float64, stops=None, **cfg):
    """fused_tail_reference.evaluate over the per-ray background, with d_bg"""
    n_rays = cfg.get("n_rays")
    return with_d_bg(R.evaluate(by_row(x, rgb_bg, n_rays), dtype=dtype, stops=stops, **cfg), x, n_rays)


def noise_of(low, ref):
    out = R.noise_of(low, ref)
    out["d_bg"] = float(np.nanmax(np.abs(low["d_bg"] - ref["d_bg"]), initial=0.0))
    return out
