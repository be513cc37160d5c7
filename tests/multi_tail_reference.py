"""Float64 restatement of the fused render + loss tail with several optional terms at once
(ngp_render_loss_fused_multi) for the tests, built from the three single restatements and not a fourth copy.

On ONE fused_tail_reference.render state the default recipe's finish and the finish functions of
semantic_tail_reference, normal_tail_reference and depth_tail_reference are taken.  Each single finish returns the
default recipe's d_sig plus its own term's share, so its increment over the default is that share alone, and the terms
are independent functions of the state (the fit and the falloff of depth_mono are constants of that term, the weights
constants of the CE and normal terms):

  d_sig  = default + sum over the named terms of (single d_sig - default d_sig)
  d_sem, d_np as the semantic / normal finish give them
  terms (8) = [loss, rgb, opacity, distortion, CELoss, sky_depth, normal_mono, depth_mono], a term that is not named 0 and
              its increment left out

tests/test_multi_tail_host.py holds this against one autograd pass over the whole sum of terms."""
import numpy as np
import torch

import depth_tail_reference as DR
import fused_tail_reference as R
import normal_tail_reference as NR
import semantic_tail_reference as SR
from fused_tail_reference import MAX_BORDERLINE, comparable, make_crafted, make_random, owned  # noqa: F401

TERMS = ("semantic", "normal_mono", "depth_mono")          # bit i of the entry's term_mask
MASKS = {1: ("semantic",), 2: ("normal_mono",), 4: ("depth_mono",), 3: ("semantic", "normal_mono"),
         5: ("semantic", "depth_mono"), 6: ("normal_mono", "depth_mono"), 7: TERMS}
MULTI_MASKS = (3, 5, 6, 7)
LABEL_SEED, NORMAL_SEED, DEPTH_SEED = 11, 12, 13           # the targets' own seeds on the combined batch


def make_batch(name):
    """a batch of tests/test_fused_tail_gpu.py ('crafted', '300', '1500') with 16 logit columns (the first 8 its own)"""
    return SR.widen(make_crafted(0) if name == "crafted" else make_random(int(name)))


def make_labels(x, classes, valid=True):
    """semantic_tail_reference.labels_for on the combined batch.  With LABEL_SEED every batch and class count of the tests
    has a ray labelled 4 whose depth in make_depths(x) is valid (sky_rows_with_depth; the head's own 4 sits on row 5,
    which make_depths always makes invalid): tests/test_multi_tail_host.py checks it"""
    return SR.labels_for(x, classes, seed=LABEL_SEED, valid=valid)


def make_normals(x, kind="mixed", T_thr=1e-4):
    """normal_tail_reference.make_normals against the normals composited at T_thr (the stop samples, and with them N^,
    depend on it: the targets keep SIGN_MARGIN at the threshold they are used at); kind='none': every row (0, 0, 0)"""
    if kind == "none":
        return np.zeros((x["n_rays"], 3), np.float32)
    return NR.make_normals(x, seed=NORMAL_SEED, N_hat=NR.composited_normals(x, T_thr=T_thr))


def make_depths(x, kind="mixed"):
    return DR.make_depths(x, seed=DEPTH_SEED, kind=kind)


def sky_rows_with_depth(x, labels, depths, n_rays=None):
    """rows labelled 4 whose monocular depth is valid: where the sky seed and the depth_mono seed add into one g_D"""
    rays = x["rays_a"][:n_rays, 0]
    return np.nonzero((np.asarray(labels)[rays] == SR.SKY) & (np.asarray(depths)[rays] > 0))[0]


def finish(st, x, named, targets, classes, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, lam_sem=SR.LAMBDA_SEM, lam_sky=SR.LAMBDA_SKY,
           lam_nm=NR.LAMBDA_NM, lam_dm=DR.LAMBDA_DM, scene_scale=1.0, use_bg=True):
    """the combination described in the module docstring on a render() state.  named: a subset of TERMS; targets: dict with
    'labels', 'normals', 'depths' (those of the named terms are read).  -> fused_tail_reference.finish's dict with terms (8),
    the combined d_sig, and what the named terms' own finish adds: d_sem, n_valid_labels; d_np; fit, n_valid_depths, g_D"""
    base = R.finish(st, x, lam_o=lam_o, lam_d=lam_d, use_bg=use_bg)
    out = dict(base)
    d_sig = base["d_sig"].copy()
    terms = np.zeros(8)
    terms[:4] = base["terms"]
    kw = dict(lam_o=lam_o, lam_d=lam_d, use_bg=use_bg)
    if "semantic" in named:
        s = SR.finish(st, x, targets["labels"], classes, lam_sem=lam_sem, lam_sky=lam_sky, **kw)
        d_sig += s["d_sig"] - base["d_sig"]
        out["d_sem"], out["n_valid_labels"] = s["d_sem"], s["n_valid"]
        terms[4:6] = s["terms"][4:6]
    if "normal_mono" in named:
        s = NR.finish(st, x, targets["normals"], lam_nm=lam_nm, **kw)
        d_sig += s["d_sig"] - base["d_sig"]          # (zero: the weights are constants of this term)
        out["d_np"] = s["d_np"]
        terms[6] = s["terms"][4]
    if "depth_mono" in named:
        s = DR.finish(st, x, targets["depths"], lam_dm=lam_dm, scene_scale=scene_scale, **kw)
        d_sig += s["d_sig"] - base["d_sig"]
        out["fit"], out["n_valid_depths"], out["g_D"] = s["fit"], s["n_valid"], s["g_D"]
        terms[7] = s["terms"][4]
    terms[0] = base["terms"][0] + terms[4:].sum()
    out["d_sig"], out["terms"] = d_sig, terms
    return out


def evaluate(x, named, targets, dtype=torch.float64, stops=None, **cfg):
    st = R.render(x, dtype=dtype, stops=stops, **{k: v for k, v in cfg.items() if k in R.RENDER_KEYS})
    return finish(st, x, named, targets, cfg.get("classes", 7), **{k: v for k, v in cfg.items() if k not in R.RENDER_KEYS})


def noise_of(low, ref):
    out = R.noise_of(low, ref)
    for key in ("d_sem", "d_np"):
        if key in ref:
            out[key] = float(np.nanmax(np.abs(low[key] - ref[key]), initial=0.0))
    if "fit" in ref:
        out["fit"] = np.abs(low["fit"] - ref["fit"])
    return out


def fp32_error(x, named, targets, ref=None, **cfg):
    """the same restatement with every tensor in float32 (the stop samples of the float64 run) against the float64 one"""
    ref = evaluate(x, named, targets, **cfg) if ref is None else ref
    return noise_of(evaluate(x, named, targets, dtype=torch.float32, stops=ref["stops"], **cfg), ref)
