"""Guards of tests/optim_reference.py and of the comparer behind tests/test_optim_gpu.py, without a GPU:
adam_step64 is torch.optim.Adam in float64; on every input set of the GPU module the float32 restatements (plain and with
every contraction) stay within HALF of each bar; each wrong Adam of MUTANTS misses the bars on every argument set that
tells it from the right one; the clip restatements are torch.nn.utils.clip_grad_norm_."""
import math

import numpy as np
import pytest
import torch

import optim_reference as R
import test_optim_gpu as G

B1, B2, EPS = G.BETA1, G.BETA2, G.EPS


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------- against torch
def torch_adam(opt, P, g, lr, step, grad_scale):
    """one step of torch's float64 Adam with the float32-rounded step_size and bc2_sqrt of the host: lr and eps are set
    such that torch's own double constants reproduce them (p - lr / bc1 * m / (sqrt(v) / s + eps), s = sqrt(bc2))"""
    step_size, bc2_sqrt = R.host_constants(lr, B1, B2, step)
    bc1, s = 1.0 - f32(B1) ** step, math.sqrt(1.0 - f32(B2) ** step)
    opt.param_groups[0]["lr"] = float(step_size) * bc1 * float(bc2_sqrt) / s
    opt.param_groups[0]["eps"] = f32(EPS) * float(bc2_sqrt) / s
    P.grad = torch.from_numpy(np.asarray(g, np.float64) * (1.0 if grad_scale is None else f32(grad_scale)))
    opt.step()


def agree(got, want, scale):
    assert (np.abs(got - want) <= 1e-12 * scale).all(), float((np.abs(got - want) / scale).max())


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step64_is_torch_adam(wd):
    x = G.adam_inputs(G.SWEEP_N)
    # single steps from arbitrary state, loaded through optimizer.state
    for step in G.STEPS:
        for lr in G.LRS:
            for gs in (None, 0.37):
                P = torch.from_numpy(x["p"].astype(np.float64)).requires_grad_(True)
                opt = torch.optim.Adam([P], lr=1.0, betas=(f32(B1), f32(B2)), eps=1.0, weight_decay=f32(wd), foreach=False)
                opt.state[P] = dict(step=torch.tensor(float(step - 1), dtype=torch.float64),
                                    exp_avg=torch.from_numpy(x["m"].astype(np.float64)),
                                    exp_avg_sq=torch.from_numpy(x["v"].astype(np.float64)))
                torch_adam(opt, P, x["g"], lr, step, gs)
                ref = R.adam_step64(x["p"], x["g"], x["m"], x["v"], lr, B1, B2, EPS, wd, step, gs)
                st = opt.state[P]
                assert float(st["step"]) == step
                agree(P.detach().numpy(), ref.p, np.abs(x["p"]) + np.abs(ref.u))
                agree(st["exp_avg"].numpy(), ref.m, np.maximum(ref.gscale, np.abs(x["m"])) + 1e-300)
                agree(st["exp_avg_sq"].numpy(), ref.v, np.maximum(ref.gscale ** 2, x["v"]) + 1e-300)
    # a few steps from zero state, every step with a new gradient
    g = np.random.default_rng(1)
    n = 1000
    p = g.normal(size=n)
    m, v = np.zeros(n), np.zeros(n)
    P = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([P], lr=1.0, betas=(f32(B1), f32(B2)), eps=1.0, weight_decay=f32(wd), foreach=False)
    for step in range(1, 6):
        grad = g.normal(size=n) * 10.0 ** g.uniform(-6, 0, n)
        torch_adam(opt, P, grad, 1e-2, step, None)
        ref = R.adam_step64(p, grad, m, v, 1e-2, B1, B2, EPS, wd, step, None)
        agree(P.detach().numpy(), ref.p, np.abs(p) + np.abs(ref.u))
        agree(opt.state[P]["exp_avg"].numpy(), ref.m, np.maximum(ref.gscale, np.abs(m)))
        agree(opt.state[P]["exp_avg_sq"].numpy(), ref.v, np.maximum(ref.gscale ** 2, v))
        p, m, v = ref.p, ref.m, ref.v


# ---------------------------------------------------------------------------------------------------- headroom
def family(name):
    return name.split("/")[0] if not name.startswith("n=") else ("sizes" if int(name[2:].split("/")[0]) < G.BIG else "big")


def restated(x, a, **kw):
    return R.adam_step32(x["p"], x["g"], x["m"], x["v"], a["lr"], B1, B2, EPS, a["weight_decay"], a["step"],
                         a["grad_scale"], **kw)


def test_float32_restatements_stay_within_half_of_every_bar():
    """a condition on the bars and the inputs, not a measurement: the reference alone, in float32 op by op and with every
    a * b + c rounded once, uses at most half of what the kernel is allowed"""
    worst = {}
    for name, x, a in G.all_cases():
        ref, bar = G.reference(x, a)
        for contract in (False, True):
            r = R.ratios(restated(x, a, contract=contract), ref, bar)
            key = (family(name), "wd" if a["weight_decay"] else "no wd", "contracted" if contract else "plain")
            w = worst.setdefault(key, dict(p=0.0, m=0.0, v=0.0))
            for k in "pmv":
                w[k] = max(w[k], r[k])
            assert R.within(r, 0.5), (name, contract, r)
    for key, w in sorted(worst.items()):
        print(" ".join(key), " ".join(f"{k} {w[k]:.3f}" for k in "pmv"))


def test_weight_decay_scale_of_the_gradient():
    """with weight decay the rounding of g^ = g gs + wd p is measured by |g gs| + |wd p|: where the two terms cancel, the
    float32 g^ is further from the float64 one than a few ulp of |g^|, and the bars must not be built on |g^|"""
    n = 4096
    p = np.linspace(1.0, 2.0, n).astype(np.float32)
    g = (-np.float32(0.01) * p * (1 + np.float32(1e-5))).astype(np.float32)          # g + wd p is 1e-5 of either term
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    a = G.args_of(None, 0.01, 10, 1e-2, 1)
    x = dict(p=p, g=g, m=m, v=v)
    ref, bar = G.reference(x, a)
    for contract in (False, True):
        r = R.ratios(restated(x, a, contract=contract), ref, bar)
        assert R.within(r, 0.5), r
    got_m = restated(x, a)[1].astype(np.float64)
    on_ghat = np.abs(got_m - ref.m) / (4 * R.E * np.maximum(np.abs(ref.ghat), np.abs(m)))
    print(f"float32 m' against float64 in units of a bar built on |g^|: {on_ghat.max():.1f}; on |g gs| + |wd p|: "
          f"{(np.abs(got_m - ref.m) / bar.m).max():.3f}")
    assert on_ghat.max() > 1.0


# ---------------------------------------------------------------------------------------------------- mutants
def _twice(x, a, out):
    b = x["border"]
    s = slice(b, b + 4)
    g2 = np.zeros(4, np.float32) if a["zero_grad"] else x["g"][s]
    again = R.adam_step32(out[0][s], g2, out[1][s], out[2][s], a["lr"], B1, B2, EPS, a["weight_decay"], a["step"],
                          a["grad_scale"])
    for o, q in zip(out, again):
        o[s] = q


def _keep(lo, hi):
    def f(x, a, out):
        for o, k in zip(out, "pmv"):
            o[lo(x):hi(x)] = x[k][lo(x):hi(x)]
    return f


def small_step(a):          # the bias corrections differ from 1 (and from step to step) in float32
    return a["step"] <= 1000


# name: (adam_step32 switches, a change of its result, the argument sets on which the mutant is a different function)
MUTANTS = {
    "eps inside the square root": (dict(eps_in_sqrt=True), None, lambda a: True),
    "bc2 without its square root": (dict(bc2_no_sqrt=True), None, small_step),
    "bc2 left out": (dict(bc2_left_out=True), None, small_step),
    "bias correction from step - 1": (dict(step_shift=-1), None, small_step),
    "bias correction from step + 1": (dict(step_shift=1), None, small_step),
    "beta1 and beta2 swapped": (dict(swap_betas=True), None, lambda a: True),
    "grad_scale on m but not on v": (dict(scale_m_only=True), None, lambda a: a["grad_scale"] in (0.37, 0.0)),
    "decoupled (AdamW) decay": (dict(decoupled=True), None, lambda a: a["weight_decay"] != 0),
    "v from g instead of g^": (dict(v_from_g=True), None, lambda a: a["weight_decay"] != 0),
    "1 / bc2_sqrt moved from denom into the step size": (dict(folded_denom=True), None, small_step),
    "the last n mod 4 elements untouched": ({}, _keep(lambda x: x["p"].size // 4 * 4, lambda x: x["p"].size), lambda a: True),
    "one quad at a piece border updated twice": ({}, _twice, lambda a: True),
    "one quad at a piece border skipped": ({}, _keep(lambda x: x["border"], lambda x: x["border"] + 4), lambda a: True),
    "the gradient zeroed before it is read": (dict(zero_first=True), None, lambda a: a["grad_scale"] != 0.0),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_wrong_adams_miss_the_bars(name):
    switches, change, differs = MUTANTS[name]
    x = G.adam_inputs(G.SWEEP_N)
    assert x["p"].size % 4 == 3 and 0 < x["border"] < x["p"].size - 8
    tried = 0
    for a in G.sweep_args():
        if not differs(a):
            continue
        tried += 1
        ref, bar = G.reference(x, a)
        with np.errstate(all="ignore"):
            out = [np.array(o) for o in restated(x, a, **switches)]
            if change:
                change(x, a, out)
        r = R.ratios(out, ref, bar)
        assert not R.within(r), (name, a, r)
    assert tried >= 48


def test_comparer_counts_what_it_must():
    x, a = G.adam_inputs(1025), G.SIZE_ARGS[0]
    ref, bar = G.reference(x, a)
    good = [np.array(o) for o in restated(x, a)]
    assert R.within(R.ratios(good, ref, bar))
    for k in range(3):
        for bad in (np.nan, np.inf):
            out = [o.copy() for o in good]
            out[k][517] = bad
            assert not R.within(R.ratios(out, ref, bar))
    s = np.flatnonzero(x["still"])[0]             # a zero bar: nothing but the exact value passes
    assert bar.m[s] == 0 and bar.v[s] == 0
    out = [o.copy() for o in good]
    out[1][s] = 1e-45
    assert R.ratios(out, ref, bar)["m"] == np.inf


# ---------------------------------------------------------------------------------------------------- clipping
def test_clip_restatements_are_clip_grad_norm():
    g = np.random.default_rng(7)
    parts = [g.normal(size=k) for k in (1000, 48, 777)]
    sumsq = float(sum((a ** 2).sum() for a in parts))
    for extra in (1.0, 0.5):
        for max_norm in (50.0, 0.5 * math.sqrt(sumsq) * extra, math.sqrt(sumsq) * extra, 1e-4):
            ps = [torch.zeros(a.size, dtype=torch.float64, requires_grad=True) for a in parts]
            for P, a in zip(ps, parts):
                P.grad = torch.from_numpy(a * extra)
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
            coef, c = R.clip_coef64(sumsq, max_norm, extra)
            for P, a in zip(ps, parts):
                assert np.abs(P.grad.numpy() - coef * a).max() <= 1e-7 * np.abs(coef * a).max()   # (sumsq and 1e-6 pass as float32)
            if c > 1.0 + 1e-6:            # (at max_norm = norm itself the float32 sumsq decides: not this line's business)
                assert coef == extra and all(np.array_equal(P.grad.numpy(), a * extra) for P, a in zip(ps, parts))
    assert R.clip_coef64(0.0, 50.0, 0.5)[0] == 0.5
    assert R.clip_coef64(float("inf"), 50.0, 1.0)[0] == 0.0 and math.isnan(R.clip_coef64(float("nan"), 50.0, 1.0)[0])
    # the bound: with S_t = ||table gradient t|| / (||W1_t|| ||W2_t||) it IS the norm, and "safe" then means torch does not clip
    w = [g.normal(size=k).astype(np.float32) for k in (1000, 48, 777, 128)]
    f = [np.linalg.norm(a.astype(np.float64)) for a in w]
    ta, tb, rest = parts
    sums = np.array([np.linalg.norm(ta) / (f[0] * f[1]), np.linalg.norm(tb) / (f[2] * f[3])], np.float32)
    norm = math.sqrt(sumsq)
    for max_norm in (0.5 * norm, norm * 1.0005, norm * 1.002 + 2e-6, 2 * norm, 50.0):
        bound, safe = R.clip_bound64(sums, *w, float((rest ** 2).sum()), max_norm, 1.0)
        assert abs(bound - norm) <= 1e-6 * norm
        assert safe == (norm * 1.001 + 1e-6 < max_norm)
        ps = [torch.zeros(a.size, dtype=torch.float64, requires_grad=True) for a in parts]
        for P, a in zip(ps, parts):
            P.grad = torch.from_numpy(a.copy())
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        if safe:
            assert all(np.array_equal(P.grad.numpy(), a) for P, a in zip(ps, parts))
    for bad in (float("nan"), float("inf")):
        assert R.clip_bound64(np.array([bad, 1.0], np.float32), *w, 0.0, 50.0, 1.0)[1] is False
        assert R.clip_bound64(sums, *w, bad, 50.0, 1.0)[1] is False
