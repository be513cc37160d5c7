"""Plain references of the two kernels behind NGPTrainer(normal_ref=True), numpy and torch on the CPU only.

(1) ngp_density_head_bwd2, the element-wise pass of the density head's second-order backward.  `head_definition` is the
    plain definition: z1 -> a1 = softplus(z1) -> z2 = a1 . w2 + b2 -> sigma = softplus(z2), m = d(sigma)/dz1 from
    torch.autograd (create_graph=True), L = <m, r> + <sigma, g>, and e1 = dL/dz1, dW2 = dL/dw2, db2 = dL/db2 from a second
    autograd.grad: nothing derived by hand.  `head_closed` restates the closed forms of include/ngp_hip.h (D2) on
    (a1, sigma) as the kernel takes them; tests/test_normal_ref_host.py holds the two together to 1e-12 in float64.
(2) ngp_normal_ref_tail.  `tail_definition`: L = lambda_rp mean(Rp) + lambda_ro mean(Ro) with Rp[r] = sum_s ws (n_raw -
    n_pred)^2, Ro[r] = sum_s ws max(<n_raw, normalize(dir)>, 0)^2 over the samples of the rays rays_a names, the means
    over 3 R and R values (R = rows of rays_a), n_raw = -F.normalize(dsigma_dx * scale3, eps=1e-6), n_pred =
    -F.normalize(head, eps=1e-6); every gradient from torch.autograd.  `tail_closed` restates the header's per-sample forms.

Each function evaluates in float64 (the reference) or in float32 (the same expressions, used only to measure what one
float32 evaluation costs against exact: the floor of second_order_reference.compare)."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(a, dtype):
    """float32 inputs as the kernels get them; a float64 array keeps its digits (the host test feeds a definition's float64
    outputs to a closed form)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.float64 else a.astype(np.float32)).to(dtype)


def _np(d):
    return {k: (v.detach().double().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------- (1) the density head
HEAD_KEYS = ("m", "e1", "dW2", "db2")


def head_definition(z1, w2, b2, r, g, dtype=torch.float64):
    """z1 (n,H), w2 (H,), b2 (1,), r (n,H), g (n,) or None -> dict of HEAD_KEYS, a1, sig (numpy float64)"""
    z1 = _t(z1, dtype).requires_grad_(True)
    w2, b2 = _t(w2, dtype).requires_grad_(True), _t(b2, dtype).requires_grad_(True)
    a1 = F.softplus(z1)
    sig = F.softplus(a1 @ w2 + b2)
    (m,) = torch.autograd.grad(sig.sum(), z1, create_graph=True)
    L = (m * _t(r, dtype)).sum()
    if g is not None:
        L = L + (sig * _t(g, dtype)).sum()
    e1, dW2, db2 = torch.autograd.grad(L, [z1, w2, b2])
    return _np(dict(m=m, e1=e1, dW2=dW2, db2=db2, a1=a1, sig=sig))


def head_closed(a1, sig, r, w2, g, dtype=torch.float64):
    """the closed forms on (a1, sig) as independent inputs, what the kernel computes"""
    a1, sig, r, w2 = _t(a1, dtype), _t(sig, dtype), _t(r, dtype), _t(w2, dtype)
    s1, o1 = -torch.expm1(-a1), torch.exp(-a1)                    # sigmoid(z1), 1 - sigmoid(z1)
    s2, o2 = -torch.expm1(-sig)[:, None], torch.exp(-sig)[:, None]
    ws1 = w2[None, :] * s1
    q = (r * ws1).sum(1, keepdim=True)
    e2 = q * s2 * o2
    if g is not None:
        e2 = e2 + _t(g, dtype)[:, None] * s2
    m = s2 * ws1
    e1 = ws1 * (e2 + r * s2 * o1)
    dW2 = (e2 * a1 + s2 * r * s1).sum(0)
    db2 = e2.sum().reshape(1)
    return _np(dict(m=m, e1=e1, dW2=dW2, db2=db2))


def head_case(kind, n, seed, with_g=True, H=128):
    """seeded float32 inputs (a1, sig, r, w2, g).  kind: 'mixed' (both signs, a1 in [0.05, 3], sig in [0.01, 5]); 'positive'
    (r, a1, w2, g > 0: every sum is one-signed, a lost tile shows in dW2 / db2); 'tiny' / 'large' (every a1 and sig within
    a factor 2 of 1e-6 / within 1 of 30: every output of such a case is small by the same factor, so a max-normalised
    comparison sees the digits that 1 - exp(-y) and s (1 - s) lose there)"""
    rng = np.random.default_rng(61000 + seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    r, w2 = rng.standard_normal((n, H)), rng.standard_normal(H) * 0.3
    g = rng.standard_normal(n)
    if kind in ("mixed", "positive"):
        a1, sig = rng.uniform(0.05, 3.0, (n, H)), rng.uniform(0.01, 5.0, n)
        if kind == "positive":
            r, w2, g = np.abs(r) + 0.1, np.abs(w2) + 0.05, np.abs(g) + 0.1
    elif kind == "tiny":
        a1, sig = 1e-6 * rng.uniform(1.0, 2.0, (n, H)), 1e-6 * rng.uniform(1.0, 2.0, n)
    elif kind == "large":
        a1, sig = 30.0 + rng.uniform(-1.0, 1.0, (n, H)), 30.0 + rng.uniform(-1.0, 1.0, n)
    else:
        raise KeyError(kind)
    return f(a1), f(sig), f(r), f(w2), (f(g) if with_g else None)


# ---------------------------------------------------------------------------------------------- (2) the tail
TAIL_KEYS = ("d_grads", "d_head", "terms")
TAIL_LENGTHS = (0, 1, 32, 33, 70, 0, 1, 40, 9, 5)     # samples per ray; ray 8 of them is marched but NOT named
TAIL_OMITTED = 8
TAIL_STOPPED = (7, 10)                                # ray 7: ws = 0 from its 10th sample on (an early stop)


def tail_case(scale, seed=0):
    """One batch with empty rays, 1-sample rays, rays of 32, 33 and 70 samples, an early-stopped ray and a ray that rays_a
    omits (its samples lie in the arrays, its slot in loss_o / loss_p exists).  Rows with exactly zero dsigma_dx, rows with
    an exactly zero head output, rows with <n_raw, d> < 0; every other row's norms are >= 1e-3 (scaled: dsigma_dx *
    scale3), so no row is borderline at eps.  -> dict of float32 / int64 numpy arrays; scale3 = 1 / (2 scale)."""
    rng = np.random.default_rng(62000 + seed)
    lens = np.asarray(TAIL_LENGTHS)
    starts = np.cumsum(lens) - lens
    N = int(lens.sum())
    named = [i for i in range(len(lens)) if i != TAIL_OMITTED]
    rays_a = np.stack([np.asarray(named), starts[named], lens[named]], 1).astype(np.int64)
    scale3 = np.full(3, 1.0 / (2.0 * scale), np.float32)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    dirs = unit(rng.standard_normal((N, 3))) * rng.uniform(0.8, 1.3, (N, 1))
    # d sigma/dx: directions with both signs of <n_raw, d>, lengths over five decades, never below 1e-3 once scaled
    dsig = unit(rng.standard_normal((N, 3))) * (10.0 ** rng.uniform(-3, 2, (N, 1))) / scale3[0] * 1.001
    head = unit(rng.standard_normal((N, 3))) * (10.0 ** rng.uniform(-3, 1, (N, 1))) * 1.001
    ws = rng.uniform(0.0, 0.2, N)
    s7 = starts[TAIL_STOPPED[0]]
    ws[s7 + TAIL_STOPPED[1]:s7 + lens[TAIL_STOPPED[0]]] = 0.0
    zero_g = np.asarray([starts[2] + 3, starts[3] + 32, starts[9] + 1])
    zero_h = np.asarray([starts[2] + 7, starts[3] + 0, starts[9] + 1])      # (one row has both)
    dsig[zero_g] = 0.0
    head[zero_h] = 0.0
    f = lambda a: np.ascontiguousarray(a, np.float32)
    c = dict(dsig=f(dsig), head=f(head), dirs=f(dirs), ws=f(ws), rays_a=rays_a, scale3=scale3, n_slots=len(lens), N=N,
             zero_g=zero_g, zero_h=zero_h, named_rows=np.concatenate([np.arange(s, s + n) for _, s, n in rays_a]).astype(np.int64),
             omitted_rows=np.arange(starts[TAIL_OMITTED], starts[TAIL_OMITTED] + lens[TAIL_OMITTED]))
    return c


def _tail_normals(dsig, head, dirs, scale3):
    n_raw = -F.normalize(dsig * scale3[None, :], p=2, dim=-1, eps=1e-6)
    n_pred = -F.normalize(head, p=2, dim=-1, eps=1e-6)
    return n_raw, n_pred, F.normalize(dirs, p=2, dim=-1, eps=1e-6)


def tail_definition(c, lam_rp, lam_ro, dtype=torch.float64):
    """-> dict: d_grads (N,3), d_head (N,3) (zero on rows rays_a does not name), terms (2), Ro (n_slots), Rp (n_slots,3)"""
    dsig, head = _t(c["dsig"], dtype).requires_grad_(True), _t(c["head"], dtype).requires_grad_(True)
    n_raw, n_pred, dn = _tail_normals(dsig, head, _t(c["dirs"], dtype), _t(c["scale3"], dtype))
    ws = _t(c["ws"], dtype)
    diff = (n_raw - n_pred) ** 2 * ws[:, None]
    ori = torch.clamp((n_raw * dn).sum(-1), min=0.0) ** 2 * ws
    Ro, Rp = torch.zeros(c["n_slots"], dtype=dtype), torch.zeros(c["n_slots"], 3, dtype=dtype)
    rows_o, rows_p = [], []
    for ray, s, n in c["rays_a"]:
        rows_o.append(ori[s:s + n].sum())
        rows_p.append(diff[s:s + n].sum(0))
    Ro_named, Rp_named = torch.stack(rows_o), torch.stack(rows_p)
    terms = torch.stack([lam_rp * Rp_named.mean(), lam_ro * Ro_named.mean()])
    d_grads, d_head = torch.autograd.grad(terms.sum(), [dsig, head])
    with torch.no_grad():
        Ro[torch.from_numpy(c["rays_a"][:, 0])] = Ro_named
        Rp[torch.from_numpy(c["rays_a"][:, 0])] = Rp_named
    return _np(dict(d_grads=d_grads, d_head=d_head, terms=terms, Ro=Ro, Rp=Rp))


def _neg_normalize_bwd(x, g):
    """ngp_neg_normalize_bwd's two branches"""
    nrm = x.norm(dim=-1, keepdim=True)
    u = x / torch.where(nrm > 1e-6, nrm, torch.ones_like(nrm))
    inside = -(g - u * (u * g).sum(-1, keepdim=True)) / torch.where(nrm > 1e-6, nrm, torch.ones_like(nrm))
    return torch.where(nrm > 1e-6, inside, -g * 1e6)


def tail_closed(c, lam_rp, lam_ro, dtype=torch.float64):
    """the header's per-sample forms (G_p, G_o, d_nraw, d_npred through the backward of -normalize)"""
    dsig, head, scale3 = _t(c["dsig"], dtype), _t(c["head"], dtype), _t(c["scale3"], dtype)
    n_raw, n_pred, dn = _tail_normals(dsig, head, _t(c["dirs"], dtype), scale3)
    R = len(c["rays_a"])
    named = torch.zeros(c["N"], dtype=dtype)
    named[torch.from_numpy(c["named_rows"])] = 1.0
    ws = _t(c["ws"], dtype) * named
    Gp, Go = (lam_rp * ws / (3 * R))[:, None], (lam_ro * ws / R)[:, None]
    e = n_raw - n_pred
    dot = torch.clamp((n_raw * dn).sum(-1, keepdim=True), min=0.0)
    d_nraw = 2 * e * Gp + 2 * dot * dn * Go
    d_npred = -2 * e * Gp
    d_grads = _neg_normalize_bwd(dsig * scale3[None, :], d_nraw) * scale3[None, :]
    d_head = _neg_normalize_bwd(head, d_npred)
    terms = torch.stack([lam_rp * (e * e * ws[:, None]).sum() / (3 * R), lam_ro * (dot[:, 0] ** 2 * ws).sum() / R])
    return _np(dict(d_grads=d_grads, d_head=d_head, terms=terms))
