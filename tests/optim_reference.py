"""Plain-numpy restatement of the optimizer step in csrc/optim_kernels.hip: Adam as ngp_adam_step_width computes it
(torch.optim.Adam's semantics: coupled weight decay, denom = sqrt(v') / sqrt(bc2) + eps) in float64, the same formula
op by op in float32 (the "reference alone" noise, with and without the contractions a compiler may make), the clipping
coefficient of clip_coef_kernel, the `safe` decision of clip_decide_kernel, and the per-element bars the kernels are held
to.  No GPU, no torch.

The bars are derived from rounding counts, with e = 2^-24 (half an ulp, relative):

  m' = m + (g^ - m) (1 - beta1)       the difference rounds to e (|g^| + |m|) <= 2e max, its tenth is added to m and the
                                      sum rounds to e |m'|: about 1.4e max(|g^|, |m|).                      bar 4e max
  v' = v beta2 + (1 - beta2) g^ g^    the product v beta2 and the sum round to e v each, the second term is a thousandth of
                                      g^2: about 2e max(g^2, v).                                            bar 4e max
  p' = p - step_size (m' / denom)     the final difference rounds to e (|p| + |u|), the quotient and the product with
                                      step_size to e |u| each; the errors of m' and of denom = sqrt(v') / bc2_sqrt + eps
                                      (half the relative error of v', then three roundings) reach p' through
                                      u = step_size m' / denom.

Below 2^-126 float32 is spaced by TINY = 2^-149 and a rounding is off by up to TINY / 2 however small the value: the second
moment of a table entry that saw one gradient of 1e-20 lives there, and so do products on their way to it (g^ g^ of a
normal g^).  m' and v' take at most three such roundings (1.5 TINY), so their bars carry 4 TINY on top, which keeps the
factor of 2 to 3.5 the relative part has; p' inherits it through the bars of m' and denom.  Where g^ = m = v = 0 nothing
rounds and the bars of m' and v' stay 0.

With weight decay g^ = g gs + wd p is a sum of two terms that can cancel, so its own rounding is measured by
|g gs| + |wd p|, not by |g^|.  tests/test_optim_host.py holds the float32 restatements to HALF of every bar on every input
set of tests/test_optim_gpu.py and shows that a list of wrong Adams misses them; profiles/optim_reference.txt has the
measured ratios."""
from types import SimpleNamespace

import numpy as np

E = 2.0 ** -24
TINY = 2.0 ** -149          # the spacing of float32 below 2^-126: there a rounding is off by up to TINY / 2, whatever e says
F32, F64 = np.float32, np.float64


def _f(x):
    """a Python number as the float32 value the C ABI passes, in float64"""
    return F64(F32(x))


def host_constants(lr, beta1, beta2, step):
    """step_size and bc2_sqrt exactly as ngp_adam_step_width rounds them: float arguments, double arithmetic, one
    rounding to float each"""
    bc1 = 1.0 - _f(beta1) ** F64(step)
    bc2 = 1.0 - _f(beta2) ** F64(step)
    with np.errstate(divide="ignore"):
        return _f(_f(lr) / F64(bc1)), _f(np.sqrt(bc2))


def adam_step64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """one Adam step in float64 (the inputs as they are: float32 from the tests) -> namespace(p, m, v, ghat, u, denom, gscale,
    step_size, bc2_sqrt).  gscale is the rounding scale of ghat: |g gs| + |wd p|.  grad_scale None = 1."""
    p, g, m, v = (np.asarray(a, dtype=F64) for a in (p, g, m, v))
    step_size, bc2_sqrt = host_constants(lr, beta1, beta2, step)
    b1, b2, eps, wd = _f(beta1), _f(beta2), _f(eps), _f(weight_decay)
    gs = F64(1.0) if grad_scale is None else _f(grad_scale)
    omb1, omb2 = F64(F32(1.0) - F32(beta1)), F64(F32(1.0) - F32(beta2))
    with np.errstate(all="ignore"):
        ghat = g * gs + wd * p if wd != 0 else g * gs
        gscale = np.abs(g * gs) + np.abs(wd * p)
        mn = m + (ghat - m) * omb1
        vn = v * b2 + omb2 * ghat * ghat
        denom = np.sqrt(vn) / bc2_sqrt + eps
        u = step_size * (mn / denom)
        pn = p - u
    return SimpleNamespace(p=pn, m=mn, v=vn, ghat=ghat, u=u, denom=denom, gscale=gscale, step_size=step_size,
                           bc2_sqrt=bc2_sqrt)


def _fma(a, b, c, contract):
    """a * b + c in float32: two roundings, or one (computed in float64, rounded once) where the compiler contracts"""
    if contract:
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
    return np.asarray(a * b, F32) + c


def adam_step32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, contract=False, **mutant):
    """the kernel's formula op by op in np.float32 -> (p', m', v').  contract=True evaluates every a * b + c of it with one
    rounding (computed in float64, rounded once): the weight-decay term, m', v' with the product v beta2 inside and p',
    which is what adam_update fuses by name.  The keyword switches state wrong Adams (tests/test_optim_host.py: MUTANTS)."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    mu = SimpleNamespace(eps_in_sqrt=False, bc2_no_sqrt=False, bc2_left_out=False, step_shift=0, swap_betas=False,
                         scale_m_only=False, decoupled=False, v_from_g=False, folded_denom=False, zero_first=False)
    mu.__dict__.update(mutant)
    b1, b2 = (beta2, beta1) if mu.swap_betas else (beta1, beta2)
    step_size, bc2_sqrt = host_constants(lr, beta1, beta2, step + mu.step_shift)
    step_size, bc2_sqrt = F32(step_size), F32(bc2_sqrt)
    if mu.bc2_no_sqrt:
        bc2_sqrt = F32(F64(bc2_sqrt) ** 2)
    if mu.bc2_left_out:
        bc2_sqrt = F32(1.0)
    if mu.folded_denom:       # the factor moved from the denominator into the step size: eps is no longer divided by it
        step_size, bc2_sqrt = F32(step_size * bc2_sqrt), F32(1.0)
    b1, b2, eps, wd = F32(b1), F32(b2), F32(eps), F32(weight_decay)
    gs = F32(1.0) if grad_scale is None else F32(grad_scale)
    omb1, omb2 = F32(1.0) - b1, F32(1.0) - b2
    with np.errstate(all="ignore"):
        g_read = np.zeros_like(g) if mu.zero_first else g
        gr = g_read * gs
        gv = g_read if mu.scale_m_only else gr
        if wd != 0 and not mu.decoupled:
            gr = _fma(p, wd, gr, contract)
            if not mu.v_from_g:
                gv = _fma(p, wd, gv, contract) if mu.scale_m_only else gr
        mn = _fma(gr - m, omb1, m, contract)
        vn = _fma(v, b2, (omb2 * gv) * gv, contract)
        if mu.eps_in_sqrt:
            denom = np.sqrt(vn + eps) / bc2_sqrt
        else:
            denom = np.sqrt(vn) / bc2_sqrt + eps
        pn = _fma(mn / denom, -step_size, p, contract)
        if wd != 0 and mu.decoupled:
            pn = pn - F32(lr) * wd * p
    return pn.astype(F32), mn.astype(F32), vn.astype(F32)


def bars(p, m, v, ref, weight_decay):
    """per-element bounds on |kernel - adam_step64| for (p', m', v'), from the inputs and the float64 step `ref`"""
    p, m, v = (np.asarray(a, F32).astype(F64) for a in (p, m, v))
    with np.errstate(all="ignore"):
        gsc = ref.gscale if weight_decay != 0 else np.abs(ref.ghat)
        under = np.where((gsc == 0) & (m == 0) & (v == 0), 0.0, 4 * TINY)   # (nothing rounds where everything is zero)
        bar_m = 4 * E * np.maximum(gsc, np.abs(m)) + under
        bar_v = 4 * E * np.maximum(gsc * gsc, v) + under
        bar_denom = np.where(ref.v > 0, bar_v / (2 * np.sqrt(ref.v)) / ref.bc2_sqrt, np.sqrt(bar_v) / ref.bc2_sqrt) \
            + 4 * E * ref.denom
        bar_p = 2 * E * (np.abs(p) + np.abs(ref.u)) + 4 * E * np.abs(ref.u) \
            + ref.step_size * (bar_m / ref.denom + np.abs(ref.m) * bar_denom / ref.denom ** 2)
    return SimpleNamespace(p=bar_p, m=bar_m, v=bar_v)


def ratios(got, ref, bar):
    """-> {"p": r, "m": r, "v": r}: the largest |got - ref| / bar over the elements whose reference is finite (0 / 0 counts
    as 0, a difference over a zero bar and a non-finite value against a finite reference as inf), and "nonfinite": whether
    got is non-finite exactly where the reference's p' is"""
    out = {}
    bad = ~np.isfinite(ref.p)
    for k, a in zip("pmv", got):
        a, r, b = np.asarray(a).astype(F64), getattr(ref, k), getattr(bar, k)
        ok = np.isfinite(r) & ~bad
        with np.errstate(all="ignore"):
            d = np.abs(a - r)
            q = np.where(d == 0, 0.0, np.where(np.isfinite(d), d / b, np.inf))
        out[k] = float(q[ok].max()) if ok.any() else 0.0
    out["nonfinite"] = bool(np.array_equal(~np.isfinite(np.asarray(got[0]).astype(F64)), bad))
    return out


def within(r, factor=1.0):
    return r["p"] <= factor and r["m"] <= factor and r["v"] <= factor and r["nonfinite"]


# ---------------------------------------------------------------------------------------------------- clipping
def clip_coef64(sumsq, max_norm, extra_scale=1.0):
    """clip_coef_kernel in float64 -> (coef, c): coef = extra_scale * min(1, c), c = max_norm / (sqrt(sumsq) extra_scale +
    1e-6).  c > 1 means no clipping (coef is then exactly extra_scale); NaN stays NaN, an infinite norm gives 0."""
    with np.errstate(all="ignore"):
        norm = np.sqrt(_f(sumsq)) * _f(extra_scale)
        c = _f(max_norm) / (norm + _f(1e-6))
    return (float(c) if not c > 1.0 else 1.0) * float(_f(extra_scale)), float(c)


def clip_bound64(row_norm_sums, w1a, w2a, w1b, w2b, rest_sq, max_norm, extra_scale=1.0):
    """clip_decide_kernel's bound and decision in float64 -> (bound, safe).  bound = sqrt(sum_t (||W1_t||_F ||W2_t||_F S_t)^2
    + rest_sq) * extra_scale; safe = bound * 1.001 + 1e-6 < max_norm, which is False for a NaN or infinite bound."""
    def fro(w):
        return np.sqrt((np.asarray(w, F32).astype(F64) ** 2).sum())
    with np.errstate(all="ignore"):
        ba = fro(w1a) * fro(w2a) * _f(row_norm_sums[0])
        bb = fro(w1b) * fro(w2b) * _f(row_norm_sums[1])
        bound = np.sqrt(ba * ba + bb * bb + F64(rest_sq)) * _f(extra_scale)
        safe = bool(bound * 1.001 + 1e-6 < max_norm)
    return float(bound), safe
