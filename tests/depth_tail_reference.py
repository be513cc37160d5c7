"""Float64 restatement of the depth_mono form of the fused render + loss tail (ngp_render_loss_fused_dep) for the tests,
and the seeded monocular depths of tests/test_depth_tail_gpu.py.

Everything the default recipe shares comes from fused_tail_reference (render / finish: the per-ray sums, the default
terms and their gradients).  On top of it, as losses.NeRFLoss._depth_mono and losses.compute_scale_and_shift state it:

  z_r    = depth_gt_r / 25,  valid iff z_r > 0          (zero, negative, NaN: the ray takes no part anywhere)
  (a, b) = least-squares scale and shift of a D + b ~ z over the valid rays, D DETACHED, by Cramer's rule on the sums of
           D^2, D, 1, D z, z; det == 0 gives (0, 0)
  term   = lambda_dm / R sum_valid exp(-D / scale) (a D + b - z)^2,   the falloff DETACHED

with the gradient w.r.t. sigma by torch.autograd, added to the default recipe's d_sig."""
import numpy as np
import torch

import fused_tail_reference as R
from fused_tail_reference import MAX_BORDERLINE, comparable, make_crafted, make_random, owned  # noqa: F401

LAMBDA_DM = 1.0                          # NeRFLoss.WEIGHTS['lambda_depth_mono']
ALPHA, BETA, NOISE = 0.04, 0.01, 0.004   # depth_gt = 25 (ALPHA D + BETA + uniform(-NOISE, NOISE)): always positive
INVALID_SHARE = 0.2
MIN_SPREAD = 0.1                         # var(D) / mean(D^2) over the valid rays of every batch and prefix compared tightly
PREFIXES = (7, 8, 9)


def spread(D, valid):
    """var(D) / mean(D^2) over the valid rays: 1 - cos^2 of the angle between D and the constant, what the determinant of
    the normal equations is relative to its two products (0 for fewer than two valid rays)"""
    d = np.asarray(D, np.float64)[np.asarray(valid, bool)]
    if len(d) < 2 or not (d * d).mean() > 0:
        return 0.0
    return float(d.var() / (d * d).mean())


def make_depths(x, seed=0, kind="mixed", D_ref=None):
    """float32 (n_rays,) raw monocular depths indexed by ray: 25 (0.04 D_ref + 0.01 + noise) with D_ref the float64
    composited depth, and about a fifth of the rows invalid, mixing 0, negative numbers and NaN (rows 2, 3 and 5 one of
    each, rows 0 and 1 never, so the prefixes 7 / 8 / 9 hold both kinds).  The invalid mask is drawn again while
    var(D) / mean(D^2) over the valid rows of the batch or of one of PREFIXES lies under MIN_SPREAD.
    kind='none': every row invalid (the three kinds in turn); 'one': row 0 alone valid."""
    g = np.random.default_rng(7700 + seed)
    rows = len(x["rays_a"])
    if D_ref is None:
        D_ref = R.render(x)["depth"].detach().numpy()
    z = ALPHA * D_ref + BETA + g.uniform(-NOISE, NOISE, rows)
    bad_values = np.array([0.0, -1.0, np.nan, -0.0, -37.5])
    while True:
        bad = g.random(rows) < INVALID_SHARE
        bad[[r for r in (2, 3, 5) if r < rows]] = True
        bad[:2] = False
        if kind == "none":
            bad[:] = True
        elif kind == "one":
            bad[1:] = True
        if kind != "mixed" or all(spread(D_ref[:p], ~bad[:p]) >= MIN_SPREAD for p in (rows,) + PREFIXES if p <= rows):
            break
    val = (25.0 * z).astype(np.float32)
    which = g.integers(len(bad_values), size=rows)
    which[[r for r in (2, 3, 5) if r < rows]] = [0, 1, 2][:len([r for r in (2, 3, 5) if r < rows])]
    val[bad] = bad_values[which[bad]].astype(np.float32)
    out = np.zeros(x["n_rays"], np.float32)
    out[x["rays_a"][:, 0]] = val
    return out


def scale_and_shift(D, z, valid):
    """Cramer's rule on the five sums over the valid entries; det == 0 -> (0, 0).  D, z tensors (z finite), valid bool"""
    zero = torch.zeros((), dtype=D.dtype)
    d, t = torch.where(valid, D, zero), torch.where(valid, z, zero)
    s_dd, s_d, n, s_dz, s_z = (d * d).sum(), d.sum(), valid.to(D.dtype).sum(), (d * t).sum(), t.sum()
    det = s_dd * n - s_d * s_d
    if float(det) == 0.0:
        return zero, zero
    return (n * s_dz - s_d * s_z) / det, (s_dd * s_z - s_d * s_dz) / det


def depth_term(D, z, valid, lam_dm=LAMBDA_DM, scene_scale=1.0):
    """-> (lambda_dm / R sum_valid exp(-D / scale) (a D + b - z)^2 with (a, b) and the falloff detached, a, b)"""
    a, b = scale_and_shift(D.detach(), z, valid)
    if not len(D):
        return D.sum(), a, b
    per_ray = torch.exp(-D.detach() / scene_scale) * (a * D + b - z) ** 2
    return lam_dm * torch.where(valid, per_ray, torch.zeros_like(per_ray)).sum() / len(D), a, b


def finish(st, x, depths, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, lam_dm=LAMBDA_DM, scene_scale=1.0, use_bg=True):
    """fused_tail_reference.finish plus the depth_mono term on a render() state -> its dict with terms (5) = [loss, rgb,
    opacity, distortion, depth_mono], d_sig with the term's share added, fit = [a, b], n_valid, and by row valid and
    g_D = d term / d depth"""
    out = R.finish(st, x, lam_o=lam_o, lam_d=lam_d, use_bg=use_bg)
    lam_dm, scene_scale = float(np.float32(lam_dm)), float(np.float32(scene_scale))   # (the entry takes both as float32)
    dtype, rays_a = st["dtype"], st["rays_a"]
    rows = len(rays_a)
    z = torch.from_numpy(np.asarray(depths, np.float32)[rays_a[:, 0]]).to(dtype) / 25
    valid = z > 0
    z = torch.where(valid, z, torch.zeros_like(z))
    D = st["depth"]
    term, a, b = depth_term(D, z, valid, lam_dm, scene_scale)
    num = lambda v: v.detach().to(torch.float64).numpy()
    if rows and term.requires_grad:
        g_sig, g_D = torch.autograd.grad(term, [st["sig"], D], allow_unused=True, retain_graph=True)
    else:
        g_sig = g_D = None
    if g_sig is not None:
        out["d_sig"] = out["d_sig"] + num(g_sig)          # (NaN where no processed row owns the sample stays NaN)
    out["g_D"] = np.zeros(rows) if g_D is None else num(g_D)
    out["valid"] = valid.numpy()
    out["n_valid"] = int(valid.sum())
    out["fit"] = np.array([float(a), float(b)])
    t = out["terms"]
    v = float(term.detach())
    out["terms"] = np.array([t[0] + v, t[1], t[2], t[3], v])
    return out


def evaluate(x, depths, dtype=torch.float64, stops=None, **cfg):
    st = R.render(x, dtype=dtype, stops=stops, **{k: v for k, v in cfg.items() if k in R.RENDER_KEYS})
    return finish(st, x, depths, **{k: v for k, v in cfg.items() if k not in R.RENDER_KEYS})


def noise_of(low, ref):
    out = R.noise_of(low, ref)
    out["fit"] = np.abs(low["fit"] - ref["fit"])
    return out


def fp32_error(x, depths, ref=None, **cfg):
    """the same restatement with every tensor in float32 (the stop samples of the float64 run) against the float64 one"""
    ref = evaluate(x, depths, **cfg) if ref is None else ref
    return noise_of(evaluate(x, depths, dtype=torch.float32, stops=ref["stops"], **cfg), ref)
