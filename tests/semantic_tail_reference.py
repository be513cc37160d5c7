"""Float64 restatement of the semantic form of the fused render + loss tail (ngp_render_loss_fused_sem) for the tests,
and the seeded labels and wide class logits of tests/test_semantic_tail_gpu.py.

Everything the default recipe shares comes from fused_tail_reference (render / finish: the per-ray sums, the default
terms and their gradients).  On top of it, as losses.NeRFLoss(semantic=True) and rendering.py state it:

  S_r    = sum_s w_s softmax(logits_s)          the class logits are a leaf; the weights are DETACHED here (the
                                                 reference's composite_train_bw drops dL_dsem from dL_dsigma)
  CELoss = lambda_sem * nn.CrossEntropyLoss(ignore_index=256)(S, y)      mean over the valid labels
  sky    = lambda_sky * mean_r [y_r == 4] exp(-depth_r)                   the weights are LIVE in the depth

with gradients by torch.autograd.  A label outside [0, classes) is mapped to 256 before torch sees it; a batch without
a valid label has CELoss = 0 and no gradient (torch: NaN), the entry's documented deviation."""
import numpy as np
import torch
import torch.nn.functional as F

import fused_tail_reference as R
from fused_tail_reference import MAX_BORDERLINE, comparable, make_crafted, make_random, owned  # noqa: F401

LAMBDA_SEM, LAMBDA_SKY = 4e-2, 1e-1      # NeRFLoss.WEIGHTS
IGNORE, SKY = 256, 4
CMAX = 16
SPECIAL = (IGNORE, 255, -1, SKY)         # every batch holds these beside valid labels


def widen(x, seed=0):
    """a copy of a fused_tail_reference batch whose class logits have CMAX columns: the first 8 are the batch's own, so
    that everything the existing suite established about the batch (stops, borderline rays) still holds"""
    g = np.random.default_rng(7300 + seed)
    y = dict(x)
    y["sem"] = np.concatenate([x["sem"], g.standard_normal((x["n"], CMAX - x["sem"].shape[1])).astype(np.float32)], 1)
    return y


def make_labels(n_rays, classes, seed=0, valid=True):
    """int64 (n_rays): about 60 % valid labels in [0, classes), the rest 256, 255, -1, 4 and classes (just out of range)
    in equal shares; the first entries are one of each, so every prefix of 9 rays holds a valid one.  valid=False: the
    valid labels are replaced by 256 (and a 4 stays a 4: valid only if classes > 4)"""
    g = np.random.default_rng(7400 + 31 * classes + seed)
    odd = np.array(SPECIAL + (classes,), np.int64)
    lab = np.where(g.random(n_rays) < 0.6, g.integers(0, classes, n_rays), odd[g.integers(0, len(odd), n_rays)])
    head = np.concatenate([[0, classes - 1], odd])[:n_rays]
    lab[:len(head)] = head
    if not valid:
        lab[(lab >= 0) & (lab < classes)] = IGNORE
        if classes > SKY:
            lab[lab == SKY] = 255
    return lab.astype(np.int64)


def labels_for(x, classes, seed=0, valid=True):
    """make_labels laid out by ROW of x['rays_a'] (so that the first rows of a batch hold one label of each kind whatever
    permutation maps rows to rays) -> int64 (n_rays), indexed by ray as the entry reads them"""
    lab = np.full(x["n_rays"], IGNORE, np.int64)
    lab[x["rays_a"][:, 0]] = make_labels(len(x["rays_a"]), classes, seed, valid)
    return lab


def mapped(labels, classes):
    """what torch's cross-entropy may see: valid labels and 256"""
    labels = np.asarray(labels, np.int64)
    return np.where((labels >= 0) & (labels < classes), labels, IGNORE)


def ce_term(S, labels, classes, lam_sem=LAMBDA_SEM):
    """lambda_sem * CrossEntropyLoss(ignore_index=256) on the composited probabilities S (R, classes), labels (R) any
    int64; 0 (attached to S) when no label is valid"""
    lab = torch.from_numpy(mapped(labels, classes))
    if not (lab != IGNORE).any():
        return (S * 0).sum()
    return lam_sem * F.cross_entropy(S, lab, ignore_index=IGNORE)


def finish(st, x, labels, classes, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, lam_sem=LAMBDA_SEM, lam_sky=LAMBDA_SKY, use_bg=True):
    """fused_tail_reference.finish plus the two semantic terms on a render() state -> its dict with terms (6) = [loss,
    rgb, opacity, distortion, CELoss, sky_depth], d_sig including the sky term, d_sem (n, classes) (NaN where no processed
    row owns the sample, 0 behind a stop), g_S (rows, classes) = dCE/dS and n_valid"""
    out = R.finish(st, x, lam_o=lam_o, lam_d=lam_d, use_bg=use_bg)
    # (the entry takes its weights as float32, like T_threshold in render(): the restatement weighs with those values)
    lam_sem, lam_sky = float(np.float32(lam_sem)), float(np.float32(lam_sky))
    dtype, rays_a = st["dtype"], st["rays_a"]
    rows = len(rays_a)
    lab_rows = np.asarray(labels, np.int64)[rays_a[:, 0]]
    logits = torch.from_numpy(np.array(x["sem"][:, :classes])).to(dtype).requires_grad_(True)
    prob = torch.softmax(logits, dim=-1)
    w = torch.from_numpy(np.nan_to_num(st["ws"])).to(dtype)           # detached weights, 0 behind the stop
    seg = torch.from_numpy(np.maximum(owned(x, st["n_rays"])[0], 0))
    own = torch.from_numpy(owned(x, st["n_rays"])[0] >= 0)
    S = torch.zeros(rows, classes, dtype=dtype).index_add(0, seg, torch.where(own[:, None], w[:, None] * prob, 0.0))
    S.retain_grad()
    ce = ce_term(S, lab_rows, classes, lam_sem)
    is_sky = torch.from_numpy(lab_rows == SKY).to(dtype)
    sky = lam_sky * (is_sky * torch.exp(-st["depth"])).mean() if rows else st["depth"].sum()
    g_logits, g_sig = torch.autograd.grad(ce + sky, [logits, st["sig"]], allow_unused=True, retain_graph=True)
    num = lambda v: v.detach().to(torch.float64).numpy()
    own = own.numpy()
    out["d_sem"] = np.where(own[:, None], 0.0 if g_logits is None else num(g_logits), np.nan)
    if g_sig is not None:
        out["d_sig"] = out["d_sig"] + np.where(own, num(g_sig), np.nan)
    (g_S,) = torch.autograd.grad(ce, [S], allow_unused=True, retain_graph=True)
    out["g_S"] = np.zeros((rows, classes)) if g_S is None else num(g_S)
    t = out["terms"]
    ce_v, sky_v = float(ce.detach()), float(sky.detach())
    out["terms"] = np.array([t[0] + ce_v + sky_v, t[1], t[2], t[3], ce_v, sky_v])
    out["n_valid"] = int(((lab_rows >= 0) & (lab_rows < classes)).sum())
    return out


def evaluate(x, labels, dtype=torch.float64, stops=None, **cfg):
    st = R.render(x, dtype=dtype, stops=stops, **{k: v for k, v in cfg.items() if k in R.RENDER_KEYS})
    return finish(st, x, labels, cfg.get("classes", 7), **{k: v for k, v in cfg.items() if k not in R.RENDER_KEYS})


def noise_of(low, ref):
    out = R.noise_of(low, ref)
    out["d_sem"] = float(np.nanmax(np.abs(low["d_sem"] - ref["d_sem"]), initial=0.0))
    return out


def fp32_error(x, labels, ref=None, **cfg):
    """the same restatement with every tensor in float32 (the stop samples of the float64 run) against the float64 one"""
    ref = evaluate(x, labels, **cfg) if ref is None else ref
    return noise_of(evaluate(x, labels, dtype=torch.float32, stops=ref["stops"], **cfg), ref)
