"""The fused render + loss tail on the GPU (render_loss_fused_kernel<8, 32, MASKED> behind ngp_render_loss_fused and
ngp_render_loss_fused_masked) against the float64 restatement of tests/fused_tail_reference.py, per ray and per sample,
on rays whose lengths and stop samples sit on the edges of the kernel's 32-sample chunks, and on random batches.

Bars.  opacity, depth, rgb, normal_pred, semantic, ws: rtol 2e-5, atol 2e-6, and d_sigmas, d_rgbs: rtol 2e-4, atol
2e-5 / n_rays (tests/test_gpu_parity.py's bars of the per-operation kernels; their upstream gradients are of order 1,
the loss's seeds here of order 1 / n_rays).  Ro, Rp, the loss terms and d_mask have no earlier bar against a reference:
they are held to 8 times the error of the restatement run in float32 on the same inputs (fused_tail_reference.fp32_error;
8 for tree sums, __expf and float atomics in arbitrary order instead of serial sums), but not below the atol above — for
a loss term the atol times the term's weight (1, lambda_o, lambda_d, size_delta; the sum: 1), for d_mask 2e-5 / n_rays.
The measured figures are in profiles/fused_tail_reference.txt.  A failure names the ray's (length, stop) case and the
sample."""
import numpy as np
import pytest
import torch

import fused_tail_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FW_RTOL, FW_ATOL, BW_RTOL, BW_ATOL, NOISE_FACTOR = 2e-5, 2e-6, 2e-4, 2e-5, 8.0
REORDER = 2.0 ** -24          # relative change of a sum of n non-negative float32 terms under reordering: at most n * this

ARGS = {"bg": dict(use_bg=True, use_scale=False, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D),
        "nobg-scale": dict(use_bg=False, use_scale=True, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D),
        "bg-scale-nolambda": dict(use_bg=True, use_scale=True, lam_o=0.0, lam_d=0.0),
        # at NeRFLoss's weights the distortion term's share of n_rays * d_sigmas is about 2e-6, a tenth of the bar: with
        # weights of order 1 the entropy and distortion gradients (passes B and C) are as large as the colour term's
        "bg-heavy-lambda": dict(use_bg=True, use_scale=False, lam_o=0.5, lam_d=1.0)}
PER_RAY = ("opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp")
PER_SAMPLE = ("ws", "d_sig", "d_rgb")


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


_BATCH, _STATE, _REF = {}, {}, {}


def batch(name):
    if name not in _BATCH:
        _BATCH[name] = R.make_crafted(0) if name == "crafted" else R.make_random(int(name))
        for v in _BATCH[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _BATCH[name]


def reference(name, **cfg):
    """(float64 restatement, its float32 noise) of a batch and a set of arguments: computed once, shared, read-only.
    The per-ray part (render) is shared between the losses that differ only in finish()'s arguments."""
    key = (name,) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x = batch(name)
        rkw = {k: v for k, v in cfg.items() if k in R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = R.render(x, **rkw)
            _STATE[rkey] = (hi, R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        ref = R.finish(hi, x, **fkw)
        _REF[key] = (ref, R.noise_of(R.finish(lo, x, **fkw), ref))
    return _REF[key]


def run_tail(ngp, x, T_thr=1e-4, classes=7, lam_o=R.LAMBDA_O, lam_d=R.LAMBDA_D, use_bg=True, use_scale=False, masked=False,
             size_delta=0.0, n_rays=None, ld=None, adjacent=True):
    """one direct call of the C entry on the first n_rays rows (default: all).  Every output is pre-filled with NaN
    (total_samples and vr_samples with a negative number); per-ray buffers have one entry per ray of the batch."""
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3", "mask")}
    nrm, sem = t["nrm"], t["sem"]
    if ld is not None:          # the two heads as the leading columns of wider matrices
        wide = torch.full((2, n, ld), float("nan"), device=DEV)
        wide[0, :, :3], wide[1, :, :sem.shape[1]] = nrm, sem
        nrm, sem = wide[0], wide[1]
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR,), -7, dtype=torch.int64, device=DEV)
    n_terms = 5 if masked else 4
    if adjacent:                # rendering._RenderLossFn's layout: one buffer, one memset
        acc = E(8)
        terms, vr = acc[:n_terms], acc[6 if masked else 4:][:2].view(torch.int64)
    else:
        terms, vr = E(n_terms), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 4 * (6 if masked else 4)
    o = dict(opacity=E(NR), depth=E(NR), rgb=E(NR, 3), normal=E(NR, 3), sem=E(NR, classes), ws=E(n), Ro=E(NR), Rp=E(NR, 3),
             terms=terms, d_sig=E(n), d_rgb=E(n, 3))
    head = (t["sig"], t["rgbs"], t["dsig"], t["scale3"] if use_scale else None, nrm, nrm.stride(0), sem, sem.stride(0),
            t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"], t["bg"] if use_bg else None)
    tail = (float(T_thr), int(classes), rows, float(lam_o), float(lam_d), total, vr, o["opacity"], o["depth"], o["rgb"],
            o["normal"], o["sem"], o["ws"], o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"])
    if masked:
        o["d_mask"] = E(NR)
        ngp._lib.call("render_loss_fused_masked", *head, t["mask"], float(size_delta), *tail, o["d_mask"])
    else:
        ngp._lib.call("render_loss_fused", *head, *tail)
    torch.cuda.synchronize()
    o["total"], o["vr"] = total, vr
    return {k: N(v) for k, v in o.items()}


def where(x, key, item, n_rays=None):
    """'ray 5 (row 2, case (65, 63))[, sample 64 of the segment]' of an entry of a per-ray or per-sample output"""
    rows = x["rays_a"][:n_rays]
    if key in PER_SAMPLE:
        row, k = R.owned(x, n_rays)
        if row[item] < 0:
            return f"sample {item}, owned by no ray"
        return f"ray {rows[row[item], 0]} (row {row[item]}, case {x['cases'][row[item]]}), sample {k[item]} of the segment"
    hit = np.nonzero(rows[:, 0] == item)[0]
    return f"ray {item} (row {hit[0]}, case {x['cases'][hit[0]]})" if len(hit) else f"ray {item}, in no row"


def against_reference(tag, got, ref, noise, x, cfg, ray_ok=None, smp_ok=None, nan_elsewhere=True):
    """every output of one launch against the restatement.  ray_ok / smp_ok: the rays / samples that are compared
    (default: all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    n_rays = cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    smp_own = R.owned(x, n_rays)[0] >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    weights = [1.0, 1.0, cfg.get("lam_o", R.LAMBDA_O), cfg.get("lam_d", R.LAMBDA_D), cfg.get("size_delta", 0.0)]
    misses = []

    def held(key, g, w, bar, sel, scale=1.0):
        g = g.astype(np.float64)
        if g.size == 0:
            return
        width = g.size // len(g)
        sel = np.broadcast_to(sel.reshape(sel.shape + (1,) * (g.ndim - 1)), g.shape)
        w, bar = np.broadcast_to(w, g.shape), np.broadcast_to(bar, g.shape)
        err = np.where(sel, np.nan_to_num(np.abs(g - w), nan=np.inf), 0.0)          # (a NaN misses)
        ratio = np.where(sel, err / np.maximum(np.nan_to_num(bar), 1e-300), 0.0)
        worst = int(np.argmax(ratio))
        print(f"FIG {tag} {key}: max|err| {scale * err.max():.3g}" + (f" (times n_rays = {scale})" if scale != 1 else "") +
              f", worst err/bar {ratio.ravel()[worst]:.3g}")
        bad = sel & ~(err <= bar)
        if bad.any():
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at {where(x, key, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {bar.ravel()[worst]:.3g}")

    # exact: the sample counts
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    if nan_elsewhere:       # what no processed row owns is left alone
        for key in PER_RAY + PER_SAMPLE + (("d_mask",) if "d_mask" in got else ()):
            own = smp_own if key in PER_SAMPLE else ray_own
            if not np.isnan(got[key][~own]).all():
                misses.append(f"{key}: entries that no processed row owns were written")
        if not (got["total"][~ray_own] == -7).all():
            misses.append("total_samples: entries that no processed row owns were written")
    for key in ("opacity", "depth", "rgb", "normal", "sem"):
        held(key, got[key], ref[key], FW_ATOL + FW_RTOL * np.abs(ref[key]), ray_ok)
    held("ws", got["ws"], ref["ws"], FW_ATOL + FW_RTOL * np.abs(ref["ws"]), smp_ok)
    for key in ("Ro", "Rp"):
        held(key, got[key], ref[key], max(NOISE_FACTOR * noise[key], FW_ATOL), ray_ok)
    for key in ("d_sig", "d_rgb"):
        held(key, got[key], ref[key], BW_ATOL / n_rows + BW_RTOL * np.abs(ref[key]), smp_ok, scale=n_rows)
    if "d_mask" in ref:
        held("d_mask", got["d_mask"], ref["d_mask"], max(NOISE_FACTOR * noise["d_mask"], BW_ATOL / n_rows), ray_ok, scale=n_rows)
    n_terms = len(ref["terms"])
    assert got["terms"].shape == (n_terms,)
    bars = np.maximum(NOISE_FACTOR * noise["terms"], FW_ATOL * np.array(weights[:n_terms]))
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bars}")
    for i in range(n_terms):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bars[i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bars[i]:.3g}")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("args", list(ARGS))
@pytest.mark.parametrize("classes", [0, 1, 7, 8])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
def test_crafted_edges(ngp, T_thr, classes, args):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges; nothing is left out of the comparison"""
    x = batch("crafted")
    cfg = dict(T_thr=T_thr, classes=classes, **ARGS[args])
    ref, noise = reference("crafted", **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    ok, _, _ = R.comparable(x, T_thr, 1e-2)
    assert ok.all()
    got = run_tail(ngp, x, **cfg)
    against_reference(f"crafted T_thr={T_thr} classes={classes} {args}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. leading dimensions
def _same_launch(a, b, n_blocks, keys=None):
    """two launches that must agree bit for bit (NaN where nothing was written included), except for the loss terms when
    more than one workgroup adds to them: float atomics in arrival order, at most n_blocks * 2^-24 relative apart"""
    for k in keys or [k for k in a if k != "terms"]:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    if n_blocks == 1:
        assert np.array_equal(a["terms"], b["terms"])
    else:
        np.testing.assert_allclose(a["terms"], b["terms"], rtol=n_blocks * REORDER, atol=0)


@pytest.mark.parametrize("masked", [False, True])
def test_leading_dimensions(ngp, masked):
    """normal_head and sem_logits as the leading columns of 16-wide matrices whose other columns hold NaN"""
    x = batch("crafted")
    cfg = dict(classes=7, use_scale=True, masked=masked, size_delta=6e-2)
    a = run_tail(ngp, x, **cfg)
    b = run_tail(ngp, x, ld=16, **cfg)
    assert np.isfinite(a["terms"]).all() and np.isfinite(a["opacity"]).all()
    _same_launch(a, b, 4)


# ------------------------------------------------------------------------------------------- c. ownership
@pytest.mark.parametrize("classes", [0, 1, 7])
def test_ownership(ngp, classes):
    """the gap between two segments is not touched, everything behind a stop is exactly zero, empty rays give the
    background, and sem is written in all of its columns"""
    x = batch("crafted")
    got = run_tail(ngp, x, classes=classes)
    row, k = R.owned(x)
    assert (row < 0).sum() == R.GAP
    stop_of_row = np.array([10 ** 6 if s is None else s for _, s in x["cases"]])
    behind = (row >= 0) & (k > stop_of_row[np.maximum(row, 0)])
    live = (row >= 0) & ~behind
    assert behind.sum() > 200
    for key in PER_SAMPLE:
        assert np.isnan(got[key][row < 0]).all(), key
        assert not got[key][behind].any() and not np.isnan(got[key][behind]).any(), key
        assert np.isfinite(got[key][live]).all(), key
    assert got["ws"][live].max() > 0.5 and np.count_nonzero(got["d_sig"][live]) > 0.6 * live.sum()
    empty = x["rays_a"][x["rays_a"][:, 2] == 0, 0]
    assert len(empty) == 1
    assert (got["opacity"][empty] == 0).all() and (got["total"][empty] == 0).all() and (got["depth"][empty] == 0).all()
    assert np.array_equal(got["rgb"][empty], np.broadcast_to(x["bg"], (1, 3)))
    assert got["sem"].shape == (27, classes) and not np.isnan(got["sem"]).any()
    if classes == 1:
        np.testing.assert_allclose(got["sem"][:, 0], got["opacity"], rtol=FW_RTOL, atol=FW_ATOL)
    for key in PER_RAY:
        assert np.isfinite(got[key]).all(), key


# ------------------------------------------------------------------------------------------- d. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9).  What does not depend on the ray count equals the full launch bit for bit; the
    gradients and the terms (seeds scale with 1 / rows) are held to the restatement of the same rows; everything that
    belongs to the other rows is left alone."""
    x = batch("crafted")
    cfg = dict(classes=7, use_scale=True, n_rays=rows)
    full = run_tail(ngp, x, classes=7, use_scale=True)
    got = run_tail(ngp, x, **cfg)
    rays = x["rays_a"][:rows, 0]
    smp = R.owned(x, rows)[0] >= 0
    for key in ("opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "total"):
        assert np.array_equal(got[key][rays], full[key][rays]), key
    assert np.array_equal(got["ws"][smp], full["ws"][smp])
    ref, noise = reference("crafted", **cfg)
    against_reference(f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- e. memset branches
@pytest.mark.parametrize("masked", [False, True])
def test_memset_branches(ngp, masked):
    """terms and vr_samples adjacent as rendering._RenderLossFn lays them out (one fill) and in separate allocations
    (two fills), both pre-filled with NaN / a large negative count"""
    x = batch("crafted")
    cfg = dict(classes=7, masked=masked, size_delta=6e-2)
    a = run_tail(ngp, x, adjacent=True, **cfg)
    b = run_tail(ngp, x, adjacent=False, **cfg)
    _same_launch(a, b, 4)
    ref, noise = reference("crafted", **cfg)
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference(f"crafted masked={masked} {tag}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f, g. mask, random batches
def _random_batch(ngp, name, cfg):
    """rays whose float64 transmittance comes within 1e-3 (relative) of T_threshold, and their samples, are left out of
    the per-ray and per-sample comparisons.  The loss terms are compared all the same: should such a ray stop one sample
    apart from the restatement, a weight below 1.001 * T_threshold = 1e-4 moves, and with it the ray's share of a mean by
    less than 2e-4 / n_rays of the term's weight.  For the 0.5 % of the rays that are flagged in these batches that is
    under 1e-6 of the weight, half the floor of the bars, even if every one of them did."""
    x = batch(name)
    ok, ray_ok, smp_ok = R.comparable(x, cfg.get("T_thr", 1e-4), 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= R.MAX_BORDERLINE
    ref, noise = reference(name, **cfg)
    assert 0.2 < (ref["stops"] >= 0).mean() < 0.9
    got = run_tail(ngp, x, **cfg)
    against_reference(f"random-{name} " + " ".join(f"{k}={v}" for k, v in cfg.items()), got, ref, noise, x, cfg, ray_ok, smp_ok)


@pytest.mark.parametrize("size_delta", [1.0, 6e-2])
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_masked_entry_with_a_real_mask(ngp, name, size_delta):
    """mask in (0, 1) with exact 0 and exact 1 on a few rays: d_mask, terms[4] and everything else"""
    cfg = dict(classes=7, masked=True, size_delta=size_delta)
    x = batch(name)
    assert (x["mask"] == 0).any() and (x["mask"] == 1).any() and 0.3 < x["mask"].mean() < 0.7
    if name == "crafted":
        ref, noise = reference(name, **cfg)
        assert ref["terms"][4] > 0 and np.abs(ref["d_mask"]).max() > 0
        against_reference(f"crafted masked size_delta={size_delta}", run_tail(ngp, x, **cfg), ref, noise, x, cfg)
    else:
        _random_batch(ngp, name, cfg)


@pytest.mark.parametrize("name", ["300", "1500"])
def test_random_batch(ngp, name):
    _random_batch(ngp, name, dict(classes=7))


# ------------------------------------------------------------------------------------------- h. the autograd wrappers
@pytest.mark.parametrize("masked", [False, True])
def test_wrapper_hands_back_the_direct_call(ngp, masked):
    """rendering._RenderLossFn (with and without a mask in its FusedTail) on the crafted batch: the outputs are those of the
    direct call, and back-propagating terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs (and d_mask) bit
    for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x = batch("crafted")
    cfg = dict(classes=7, use_scale=True, masked=masked, size_delta=6e-2)
    direct = run_tail(ngp, x, **cfg)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3", "mask")}
    sig, rgbs, mask = t["sig"].requires_grad_(True), t["rgbs"].requires_grad_(True), t["mask"][:, None].requires_grad_(True)
    tail = FusedTail(t["gt"], R.LAMBDA_O, R.LAMBDA_D, mask=mask, size_delta=6e-2) if masked else FusedTail(t["gt"], R.LAMBDA_O, R.LAMBDA_D)
    outs = _RenderLossFn.apply(sig, rgbs, t["sem"], t["nrm"], tail.mask, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"],
                               tail, t["scale3"], 1e-4, 7, t["bg"])
    terms = outs[0]
    assert outs[11] is None          # neither entry has a workspace
    assert terms.shape == (5 if masked else 4,) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
    seed = torch.zeros_like(terms)
    seed[0] = 1.0
    torch.autograd.backward([terms], [seed])
    own = R.owned(x)[0] >= 0
    got = dict(zip(("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp"), (N(o) for o in outs)))
    assert got["vr"].shape == (1,) and got["vr"].dtype == np.int64
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
        assert np.array_equal(got[k], direct[k]), k
    assert np.array_equal(got["ws"][own], direct["ws"][own])
    np.testing.assert_allclose(got["terms"], direct["terms"], rtol=4 * REORDER, atol=0)
    assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
    assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
    if masked:
        assert mask.grad.shape == (27, 1) and np.array_equal(N(mask.grad)[:, 0], direct["d_mask"])
