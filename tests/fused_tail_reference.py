"""Float64 restatement of the fused render + loss tail (ngp_render_loss_fused / ngp_render_loss_fused_masked) for the
tests, and the seeded inputs of tests/test_fused_tail_gpu.py, so that the host suite can check both without a GPU.

The operation is written from what rendering.py (_render_rays_train) and losses.py (NeRFLoss, sum of term means) compute,
one ray at a time with serial cumprod / cumsum in torch on the CPU: no lanes, no chunks, no closed-form gradients.  The
gradients come from torch.autograd on that graph.  The stop sample of a ray (first k with T[k] <= T_threshold) is decided
once, in float64, and then held fixed: samples behind it take no part in any sum."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import borderline_rays

LAMBDA_O, LAMBDA_D = 2e-4, 3e-4          # NeRFLoss.WEIGHTS
MAX_BORDERLINE = 0.02                    # at most this share of a random batch may be left out of a comparison
NO_STOP = (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 200)
STOPPED = ((1, 0), (2, 0), (32, 31), (33, 31), (33, 32), (40, 39), (64, 31), (64, 32), (64, 63), (65, 63), (65, 64),
           (97, 0), (97, 95), (97, 96), (200, 100))
CASES = tuple((n, None) for n in NO_STOP) + STOPPED      # (segment length, designed stop sample or None), one ray each
GAP_BEFORE, GAP = 14, 6                  # GAP samples that no ray owns lie in front of the segment of CASES[GAP_BEFORE]
RAY_KEYS = ("opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "dist")
SAMPLE_KEYS = ("ws", "d_sig", "d_rgb")


# ---------------------------------------------------------------------------------------------- inputs
def _field_outputs(g, n, n_rays):
    f = lambda *s: g.random(s).astype(np.float32)
    nrm = lambda *s: g.standard_normal(s).astype(np.float32)
    return dict(rgbs=f(n, 3), dsig=nrm(n, 3), nrm=nrm(n, 3), sem=nrm(n, 8), dirs=nrm(n, 3), gt=f(n_rays, 3), bg=f(3),
                scale3=(0.5 + 1.5 * f(3)), mask=(0.02 + 0.96 * f(n_rays)))


def make_crafted(seed=0, T_thr=1e-4):
    """one ray per CASES entry.  Optical depth is designed per sample: about 30 % exact zeros, at most 1.2 per ray in
    total (T >= 0.25 wherever no stop is designed), 20 on the designed stop sample (T drops below 1e-8 there), so the
    stop lands on the designed sample for every T_threshold in [1e-7, 0.2] and no ray is borderline.  Segments lie in
    CASES order with one gap; the rows of rays_a and the ray indices are two different permutations.  A few live
    samples have dsigma_dx = 0, normal_head = 0 or dirs = 0 (the three 1e-6 clamps); mask holds exact 0 and 1."""
    g = np.random.default_rng(7100 + seed)
    n_rays = len(CASES)
    starts, pos = [], 0
    for i, (n, _) in enumerate(CASES):
        if i == GAP_BEFORE:
            pos += GAP
        starts.append(pos)
        pos += n
    N = pos
    sig = (g.random(N) * 50).astype(np.float32)          # (the gap holds plausible values too)
    deltas = g.uniform(0.004, 0.008, N).astype(np.float32)
    ts = np.sort(g.random(N)).astype(np.float32)
    for (n, stop), s in zip(CASES, starts):
        if n == 0:
            continue
        u = g.random(n)
        u[g.random(n) < 0.3] = 0.0
        tau = u / max(u.sum(), 1e-30) * g.uniform(0.3, 1.2)
        if stop is not None:
            tau[stop] = 20.0
        sig[s:s + n] = (tau / deltas[s:s + n]).astype(np.float32)
        ts[s:s + n] = 0.5 + np.cumsum(deltas[s:s + n])
    row_case = g.permutation(n_rays)
    ray_of_row = g.permutation(n_rays)
    rays_a = np.array([[ray_of_row[r], starts[c], CASES[c][0]] for r, c in enumerate(row_case)], np.int64)
    x = dict(n=N, n_rays=n_rays, sig=sig, deltas=deltas, ts=ts, rays_a=rays_a, T_thr=T_thr,
             cases=[CASES[c] for c in row_case], **_field_outputs(g, N, n_rays))
    live = {c: s for c, s in zip(CASES, starts)}
    a, b = live[(200, None)], live[(64, 32)]
    x["dsig"][[a + 3, a + 150, b + 10, b + 31]] = 0.0
    x["nrm"][[a + 40, a + 150, b + 11, b + 32]] = 0.0
    x["dirs"][[a + 77, a + 150, b + 12]] = 0.0
    x["mask"][ray_of_row[[0, 3, 11]]] = 0.0
    x["mask"][ray_of_row[[1, 5, 20]]] = 1.0
    return x


def make_random(n_rays, seed=0):
    """the batch of tests/test_mask_gpu.py:_tail_inputs: 0 to 89 samples per ray, every 11th ray empty, sigma up to 40 (many
    rays stop early, wherever the draw puts it), rows in ray order, segments back to back"""
    g = np.random.default_rng(7200 + 13 * n_rays + seed)
    counts = g.integers(0, 90, n_rays)
    counts[::11] = 0
    starts = np.cumsum(counts) - counts
    n = int(counts.sum())
    rays_a = np.stack([np.arange(n_rays), starts, counts], 1).astype(np.int64)
    f = lambda *s: g.random(s).astype(np.float32)
    x = dict(n=n, n_rays=n_rays, sig=f(n) * 40, deltas=f(n) * 0.02 + 1e-3, ts=np.sort(f(n) * 3), rays_a=rays_a, T_thr=1e-4,
             cases=[(int(c), None) for c in counts], **_field_outputs(g, n, n_rays))
    x["mask"][:: 97] = 0.0
    x["mask"][5:: 97] = 1.0
    return x


def owned(x, n_rays=None):
    """(sample -> row of rays_a or -1, position of the sample in its segment)"""
    row = np.full(x["n"], -1, np.int64)
    k = np.zeros(x["n"], np.int64)
    for i, (_, s, n) in enumerate(x["rays_a"][:n_rays]):
        row[s:s + n] = i
        k[s:s + n] = np.arange(n)
    return row, k


def comparable(x, T_thr, rel, n_rays=None):
    """rows of rays_a whose float64 transmittance stays clear of T_threshold by `rel` (helpers.borderline_rays): only
    there is the stop sample the same in every faithful evaluation.  -> (row mask, ray mask, sample mask)"""
    rays_a = x["rays_a"][:n_rays]
    ok = ~borderline_rays(x["sig"], x["deltas"], rays_a, T_thr, rel=rel)
    ray_ok = np.zeros(x["n_rays"], bool)
    ray_ok[rays_a[ok, 0]] = True
    row, _ = owned(x, n_rays)
    return ok, ray_ok, (row >= 0) & ok[np.maximum(row, 0)]


# ---------------------------------------------------------------------------------------------- the operation
def render(x, T_thr=1e-4, classes=7, use_scale=False, n_rays=None, dtype=torch.float64, stops=None):
    """everything up to the loss on the first n_rays rows of x['rays_a'] (default: all): the per-ray sums as torch
    tensors that still carry their graph, so that finish() can be called for several losses.  `stops` fixes the stop
    samples (by row, -1: none) instead of deciding them in `dtype`."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)          # (a copy: the inputs may be read-only)
    rays_a = x["rays_a"][:n_rays]
    thr = float(np.float32(T_thr))
    sig, rgbs = t(x["sig"]).requires_grad_(True), t(x["rgbs"]).requires_grad_(True)
    deltas, ts = t(x["deltas"]), t(x["ts"])

    # per sample: the two normals, the Ref-NeRF integrands, the class probabilities
    grad = t(x["dsig"]) * t(x["scale3"]) if use_scale else t(x["dsig"])
    n_raw = -F.normalize(grad, dim=-1, eps=1e-6)
    n_pred = -F.normalize(t(x["nrm"])[:, :3], dim=-1, eps=1e-6)
    ndiff = (n_raw - n_pred) ** 2
    nori = torch.clamp((n_raw * F.normalize(t(x["dirs"]), dim=-1, eps=1e-6)).sum(-1), min=0) ** 2
    prob = torch.softmax(t(x["sem"])[:, :classes], dim=-1)

    one, zero = torch.ones(1, dtype=dtype), torch.zeros(1, dtype=dtype)
    O, D, C, Nn, S, Ro, Rp, dist, found = [], [], [], [], [], [], [], [], []
    ws = np.full(x["n"], np.nan)
    for row, (_, s, n) in enumerate(rays_a):
        sl = slice(s, s + n)
        alpha = 1 - torch.exp(-sig[sl] * deltas[sl])
        T = torch.cumprod(1 - alpha, 0)
        if stops is None:
            hit = torch.nonzero(T.detach() <= thr)
            stop = int(hit[0]) if len(hit) else -1
        else:
            stop = int(stops[row])
        found.append(stop)
        m = stop + 1 if stop >= 0 else int(n)
        sl = slice(s, s + m)
        w = alpha[:m] * torch.cat([one, T[:m - 1]]) if m else alpha[:0]
        ws[s:s + n] = 0.0
        ws[sl] = w.detach().numpy()
        tt, dl = ts[sl], deltas[sl]
        O.append(w.sum())
        D.append((w * tt).sum())
        C.append((w[:, None] * rgbs[sl]).sum(0))
        Nn.append((w[:, None] * n_pred[sl]).sum(0))
        S.append((w[:, None] * prob[sl]).sum(0))
        Ro.append((w * nori[sl]).sum())
        Rp.append((w[:, None] * ndiff[sl]).sum(0))
        wi, wti = torch.cumsum(w, 0), torch.cumsum(w * tt, 0)
        we, wte = torch.cat([zero, wi[:-1]])[:m], torch.cat([zero, wti[:-1]])[:m]
        dist.append((2 * (wti * we - wi * wte) + w * w * dl / 3).sum())
    st = dict(zip(("opacity", "depth", "rgb_fg", "normal", "sem", "Ro", "Rp", "dist"),
                  (torch.stack(v) for v in (O, D, C, Nn, S, Ro, Rp, dist))))
    st.update(sig=sig, rgbs=rgbs, ws=ws, stops=np.array(found, np.int64), rays_a=rays_a, n_rays=n_rays, dtype=dtype,
              per_sample=dict(n_pred=n_pred, prob=prob, ndiff=ndiff, nori=nori))
    return st


def finish(st, x, lam_o=LAMBDA_O, lam_d=LAMBDA_D, use_bg=True, masked=False, size_delta=0.0):
    """the loss of NeRFLoss's default recipe (with the mask terms if `masked`) on a render() state, and its gradients by
    autograd.  Per-ray outputs are indexed by ray and per-sample outputs by sample, NaN where no processed row owns the
    entry.  -> dict of float64 / int64 numpy arrays: total, vr, opacity, depth, rgb (over the background), rgb_fg, normal,
    sem, ws, Ro, Rp, dist, terms, d_sig, d_rgb, d_mask, the seeds g_rgb (R,3) = dL/d rgb_fg, g_op = dL/d opacity and
    g_dist = dL/d dist (by row), stops (by row) and the per-sample n_pred, prob, ndiff, nori"""
    dtype, rays_a = st["dtype"], st["rays_a"]
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)          # (a copy: the inputs may be read-only)
    NR = x["n_rays"]
    rays = torch.from_numpy(rays_a[:, 0].copy())
    O, C, dist = st["opacity"], st["rgb_fg"], st["dist"]
    mask_all = t(x["mask"]).requires_grad_(True) if masked else None

    rgb = C + t(x["bg"]) * (1 - O)[:, None] if use_bg else C
    err = (rgb - t(x["gt"])[rays]) ** 2
    o = O + 1e-10
    terms = [(err if not masked else (1 - mask_all[rays])[:, None] * err).mean(), lam_o * (-o * torch.log(o)).mean(),
             lam_d * dist.mean()]
    if masked:
        terms.append(size_delta * (mask_all[rays] ** 2).mean())
    loss = sum(terms)
    wrt = [st["sig"], st["rgbs"], C, O, dist] + ([mask_all] if masked else [])
    grads = torch.autograd.grad(loss, wrt, allow_unused=True, retain_graph=True)
    grads = [torch.zeros_like(v) if gr is None else gr for v, gr in zip(wrt, grads)]

    num = lambda v: v.detach().to(torch.float64).numpy()
    out = dict(total=np.zeros(NR, np.int64), stops=st["stops"], terms=num(torch.stack([loss] + terms)))
    total_rows = np.where(out["stops"] >= 0, out["stops"], rays_a[:, 2])
    out["total"][rays_a[:, 0]] = total_rows
    out["vr"] = np.array([total_rows.sum()], np.int64)
    for key in ("opacity", "depth", "rgb", "rgb_fg", "normal", "sem", "Ro", "Rp", "dist"):
        v = rgb if key == "rgb" else st[key]
        a = np.full((NR,) + tuple(v.shape[1:]), np.nan)
        a[rays_a[:, 0]] = num(v)
        out[key] = a
    own = owned(x, st["n_rays"])[0] >= 0
    out["ws"] = st["ws"]
    out["d_sig"] = np.where(own, num(grads[0]), np.nan)
    out["d_rgb"] = np.where(own[:, None], num(grads[1]), np.nan)
    out["g_rgb"], out["g_op"], out["g_dist"] = num(grads[2]), num(grads[3]), num(grads[4])
    if masked:
        out["d_mask"] = np.full(NR, np.nan)
        out["d_mask"][rays_a[:, 0]] = num(grads[5])[rays_a[:, 0]]
    out.update({k: num(v) for k, v in st["per_sample"].items()})
    return out


RENDER_KEYS = ("T_thr", "classes", "use_scale", "n_rays")


def evaluate(x, dtype=torch.float64, stops=None, **cfg):
    """render() then finish(): cfg holds the keywords of both"""
    st = render(x, dtype=dtype, stops=stops, **{k: v for k, v in cfg.items() if k in RENDER_KEYS})
    return finish(st, x, **{k: v for k, v in cfg.items() if k not in RENDER_KEYS})


def noise_of(low, ref):
    """{output: max |low - ref|} (terms: one figure per term)"""
    keys = RAY_KEYS + SAMPLE_KEYS + (("d_mask",) if "d_mask" in ref else ())
    out = {k: float(np.nanmax(np.abs(low[k] - ref[k]), initial=0.0)) for k in keys}
    out["terms"] = np.abs(low["terms"] - ref["terms"])
    return out


def fp32_error(x, ref=None, **cfg):
    """the same restatement with every tensor in float32 (serial sums, libm exp, the stop samples of the float64 run)
    against the float64 one: the noise of a faithful float32 evaluation of these inputs"""
    ref = evaluate(x, **cfg) if ref is None else ref
    return noise_of(evaluate(x, dtype=torch.float32, stops=ref["stops"], **cfg), ref)
