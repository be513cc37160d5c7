"""Float64 restatement of the normal_mono form of the fused render + loss tail (ngp_render_loss_fused_nrm) for the tests,
and the seeded target normals of tests/test_normal_tail_gpu.py.

Everything the default recipe shares comes from fused_tail_reference (render / finish: the per-ray sums, the default
terms and their gradients).  On top of it, as losses.NeRFLoss._normal_mono and rendering.py state it:

  n_s    = -F.normalize(h_s, eps=1e-6)           the head's raw output h is a leaf
  N_r    = sum_s w_s n_s                         the weights are DETACHED here (the reference's composite_train_bw drops
                                                 dL_dnormal_pred from dL_dsigma)
  term   = lambda_nm * mean over (R, 3) of |N^ - g^| - 0.1 N^ g^,   N^ = F.normalize(N), g^ = F.normalize(g)

with gradients by torch.autograd.  A ray whose target g is exactly (0, 0, 0) has no normal: its row is taken out of the
sum (and so of every gradient) while the divisor stays 3 R, the entry's documented superset of the module."""
import numpy as np
import torch
import torch.nn.functional as F

import fused_tail_reference as R
from fused_tail_reference import MAX_BORDERLINE, comparable, make_crafted, make_random, owned  # noqa: F401

LAMBDA_NM = 1e-3                         # NeRFLoss.WEIGHTS['lambda_normal_mono']
LENGTHS = (0.3, 1.0, 5.0)                # lengths of the non-zero targets
SIGN_MARGIN = 1e-3                       # no component of N^ - g^ is nearer to 0 than this (float64), by construction
ZERO_SHARE = 0.2


def composited_normals(x, **render_cfg):
    """N^ (rows, 3) of the batch in float64: what the sign of the term's derivative depends on"""
    st = R.render(x, **render_cfg)
    return F.normalize(st["normal"].detach(), dim=-1).numpy()


def make_normals(x, seed=0, zeros=True, N_hat=None):
    """float32 (n_rays, 3) targets indexed by ray: random directions of lengths 0.3, 1 and 5, about a fifth of the rows
    exactly (0, 0, 0) (rows 2 and 5 among them, rows 0 and 1 never, so the prefixes 7 / 8 / 9 hold both kinds).  A row
    where some |N^_c - g^_c| < SIGN_MARGIN in float64 is drawn again until none is: no ray sits on the jump of the sign,
    so none has to be left out of a comparison for it.  zeros=False: every target non-zero."""
    g = np.random.default_rng(7500 + seed)
    rows = len(x["rays_a"])
    N_hat = composited_normals(x) if N_hat is None else N_hat
    out = np.zeros((x["n_rays"], 3), np.float32)
    for row in range(rows):
        zero = zeros and row >= 2 and (row in (2, 5) or g.random() < ZERO_SHARE)
        while True:
            v = g.standard_normal(3)
            v = (v / np.linalg.norm(v) * LENGTHS[g.integers(3)]).astype(np.float32)
            vh = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64))
            if np.abs(N_hat[row] - vh).min() >= SIGN_MARGIN:
                break
        out[x["rays_a"][row, 0]] = 0.0 if zero else v
    return out


def sign_margin(x, normals, **render_cfg):
    """smallest |N^_c - g^_c| over the rows that have a target (float64)"""
    N_hat = composited_normals(x, **render_cfg)
    g = np.asarray(normals, np.float64)[x["rays_a"][:len(N_hat), 0]]
    have = (g != 0).any(1)
    gh = g[have] / np.linalg.norm(g[have], axis=1, keepdims=True)
    return float(np.abs(N_hat[have] - gh).min()) if have.any() else np.inf


def normal_term(N, g, lam_nm=LAMBDA_NM):
    """lambda_nm / (3 R) sum over the rows with a target of sum_c |N^_c - g^_c| - 0.1 N^_c g^_c; N, g (R, 3) tensors"""
    have = (g != 0).any(-1)
    N_hat, g_hat = F.normalize(N, dim=-1), F.normalize(g, dim=-1)
    per_ray = ((N_hat - g_hat).abs() - 0.1 * N_hat * g_hat).sum(-1)
    if not len(N):
        return per_ray.sum(), N_hat
    return lam_nm * torch.where(have, per_ray, torch.zeros_like(per_ray)).sum() / (3 * len(N)), N_hat


def finish(st, x, normals, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, lam_nm=LAMBDA_NM, use_bg=True):
    """fused_tail_reference.finish plus the normal_mono term on a render() state -> its dict with terms (5) = [loss, rgb,
    opacity, distortion, normal_mono], d_np (n, 3) (NaN where no processed row owns the sample, 0 behind a stop), and by
    row q = d term / d N^, g_N = d term / d N and has (the row has a target)"""
    out = R.finish(st, x, lam_o=lam_o, lam_d=lam_d, use_bg=use_bg)
    lam_nm = float(np.float32(lam_nm))   # (the entry takes its weight as float32)
    dtype, rays_a = st["dtype"], st["rays_a"]
    rows = len(rays_a)
    g = torch.from_numpy(np.asarray(normals, np.float32)[rays_a[:, 0]]).to(dtype)
    head = torch.from_numpy(np.array(x["nrm"][:, :3])).to(dtype).requires_grad_(True)
    n_s = -F.normalize(head, dim=-1, eps=1e-6)
    w = torch.from_numpy(np.nan_to_num(st["ws"])).to(dtype)           # detached weights, 0 behind the stop
    row_of = owned(x, st["n_rays"])[0]
    seg, own = torch.from_numpy(np.maximum(row_of, 0)), torch.from_numpy(row_of >= 0)
    N = torch.zeros(rows, 3, dtype=dtype).index_add(0, seg, torch.where(own[:, None], w[:, None] * n_s, 0.0))
    term, N_hat = normal_term(N, g, lam_nm)
    num = lambda v: v.detach().to(torch.float64).numpy()
    zero3 = lambda: np.zeros((rows, 3))
    if rows and term.requires_grad:
        g_head, g_Nh, g_N = torch.autograd.grad(term, [head, N_hat, N], allow_unused=True)
    else:
        g_head = g_Nh = g_N = None
    own = own.numpy()
    out["d_np"] = np.where(own[:, None], 0.0 if g_head is None else num(g_head), np.nan)
    out["q"] = zero3() if g_Nh is None else num(g_Nh)
    out["g_N"] = zero3() if g_N is None else num(g_N)
    out["has"] = (num(g) != 0).any(1)
    t = out["terms"]
    v = float(term.detach())
    out["terms"] = np.array([t[0] + v, t[1], t[2], t[3], v])
    return out


def evaluate(x, normals, dtype=torch.float64, stops=None, **cfg):
    st = R.render(x, dtype=dtype, stops=stops, **{k: v for k, v in cfg.items() if k in R.RENDER_KEYS})
    return finish(st, x, normals, **{k: v for k, v in cfg.items() if k not in R.RENDER_KEYS})


def noise_of(low, ref):
    out = R.noise_of(low, ref)
    out["d_np"] = float(np.nanmax(np.abs(low["d_np"] - ref["d_np"]), initial=0.0))
    return out


def fp32_error(x, normals, ref=None, **cfg):
    """the same restatement with every tensor in float32 (the stop samples of the float64 run) against the float64 one"""
    ref = evaluate(x, normals, **cfg) if ref is None else ref
    return noise_of(evaluate(x, normals, dtype=torch.float32, stops=ref["stops"], **cfg), ref)
