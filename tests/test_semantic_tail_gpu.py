"""The semantic form of the fused render + loss tail on the GPU (render_loss_fused_kernel<8 | 16, 32, false, true> behind
ngp_render_loss_fused_sem) against the float64 restatement of tests/semantic_tail_reference.py, and the routes built on
it: rendering._RenderLossFn, NGPTrainer(semantic=True), tools/train_dataset.py --render_semantic.

Bars.  The outputs this entry shares with ngp_render_loss_fused keep tests/test_fused_tail_gpu.py's bars: opacity, depth,
rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_rgbs rtol 2e-4, atol 2e-5 / n_rays; Ro, Rp and terms[0:4] 8 times
the float32 restatement's own error on the same inputs, not below 2e-6 (times the term's weight).  d_sigmas (which now
carries the sky term), d_sem_logits and terms[4:6] are held to 8 times the float32 restatement's error as well, with the
floor 2e-5 / n_rays times the term's weight (1 for d_sigmas, lambda_sem for d_sem_logits and CELoss, lambda_sky for
sky_depth).  Each case runs at NeRFLoss's weights (4e-2, 1e-1) and at lambda_sem = lambda_sky = 1, where both new
gradients are as large as the colour term's.  Every figure is printed (FIG lines) before it is asserted; the measured
maxima are in profiles/semantic_tail.txt.

No label outside [0, classes) or 256 ever reaches torch's cross-entropy on the GPU (a device-side assert): the float64
restatement runs on the CPU with such labels mapped, and the routes that go through torch's loss get valid labels or 256."""
import os
import sys

import numpy as np
import pytest
import torch

import semantic_tail_reference as S
import test_fused_tail_gpu as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N = TF.T, TF.N
CLASSES = [1, 2, 7, 8, 9, 10, 16]           # both CMAX forms and their boundary; 4 is sky but not valid for the first two
WEIGHTS = {"nerfloss": (S.LAMBDA_SEM, S.LAMBDA_SKY), "unit": (1.0, 1.0)}
PER_RAY = TF.PER_RAY
PER_SAMPLE = TF.PER_SAMPLE + ("d_sem",)

_WIDE, _STATE, _REF = {}, {}, {}


def batch(name):
    """the batches of tests/test_fused_tail_gpu.py (crafted, random 300 / 1500) with 16 logit columns"""
    if name not in _WIDE:
        _WIDE[name] = S.widen(TF.batch(name))
        _WIDE[name]["sem"].setflags(write=False)
    return _WIDE[name]


def reference(name, labels, **cfg):
    """(float64 restatement, its float32 noise): computed once per (batch, labels, arguments), shared, read-only.  The
    per-ray part (render, in float64 and in float32 at the float64 stops) is shared between the cases that differ only
    in the loss's arguments."""
    key = (name, labels.tobytes()) + tuple(sorted(cfg.items()))
    if key not in _REF:
        x = batch(name)
        rkw = {k: v for k, v in cfg.items() if k in S.R.RENDER_KEYS}
        fkw = {k: v for k, v in cfg.items() if k not in S.R.RENDER_KEYS}
        rkey = (name,) + tuple(sorted(rkw.items()))
        if rkey not in _STATE:
            hi = S.R.render(x, **rkw)
            _STATE[rkey] = (hi, S.R.render(x, dtype=torch.float32, stops=hi["stops"], **rkw))
        hi, lo = _STATE[rkey]
        classes = cfg.get("classes", 7)
        ref = S.finish(hi, x, labels, classes, **fkw)
        _REF[key] = (ref, S.noise_of(S.finish(lo, x, labels, classes, **fkw), ref))
    return _REF[key]


def run_sem(ngp, x, labels, T_thr=1e-4, classes=7, lam_o=S.R.LAMBDA_O, lam_d=S.R.LAMBDA_D, lam_sem=S.LAMBDA_SEM,
            lam_sky=S.LAMBDA_SKY, use_bg=True, use_scale=False, n_rays=None, ld=None, adjacent=True):
    """one direct call of ngp_render_loss_fused_sem on the first n_rays rows (default: all), every output pre-filled with
    NaN (the counts with negative numbers); per-ray buffers have one entry per ray of the batch"""
    rows = len(x["rays_a"]) if n_rays is None else n_rays
    NR, n = x["n_rays"], x["n"]
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    nrm, sem = t["nrm"], t["sem"][:, :classes].contiguous()
    if ld is not None:          # the two heads as the leading columns of wider matrices whose other columns hold NaN
        wide = torch.full((2, n, ld), float("nan"), device=DEV)
        wide[0, :, :3], wide[1, :, :classes] = nrm, sem
        nrm, sem = wide[0], wide[1]
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.full((NR,), -7, dtype=torch.int64, device=DEV)
    if adjacent:                # rendering.TAIL_LAYOUT['sem']: one buffer, one memset
        acc = E(8)
        terms, vr = acc[:6], acc[6:8].view(torch.int64)
    else:
        terms, vr = E(6), torch.full((1,), -(2 ** 40) - 3, dtype=torch.int64, device=DEV)
        assert vr.data_ptr() != terms.data_ptr() + 24
    n_valid = torch.full((8,), -5, dtype=torch.int32, device=DEV)          # NGP_SEM_WS_INTS, [0] = n_valid afterwards
    o = dict(opacity=E(NR), depth=E(NR), rgb=E(NR, 3), normal=E(NR, 3), sem=E(NR, classes), ws=E(n), Ro=E(NR), Rp=E(NR, 3),
             terms=terms, d_sig=E(n), d_rgb=E(n, 3), d_sem=E(n, classes))
    ngp._lib.call("render_loss_fused_sem", t["sig"], t["rgbs"], t["dsig"], t["scale3"] if use_scale else None, nrm,
                  nrm.stride(0), sem, sem.stride(0), t["dirs"], t["deltas"], t["ts"], t["rays_a"], t["gt"],
                  t["bg"] if use_bg else None, T(labels), float(lam_sem), float(lam_sky), float(T_thr), int(classes), rows,
                  float(lam_o), float(lam_d), total, vr, o["opacity"], o["depth"], o["rgb"], o["normal"], o["sem"], o["ws"],
                  o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"], n_valid, o["d_sem"])
    torch.cuda.synchronize()
    o["total"], o["vr"], o["n_valid"] = total, vr, n_valid
    return {k: N(v) for k, v in o.items()}


def against_reference(tag, got, ref, noise, x, cfg, ray_ok=None, smp_ok=None):
    """every output of one launch against the restatement (module docstring's bars).  ray_ok / smp_ok: what is compared
    (default: all that a processed row owns).  Prints each figure, then fails with the list of outputs that miss."""
    n_rays = cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    n_rows = len(rows)
    ray_own = np.zeros(x["n_rays"], bool)
    ray_own[rows[:, 0]] = True
    smp_own = S.owned(x, n_rays)[0] >= 0
    ray_ok = ray_own if ray_ok is None else ray_ok & ray_own
    smp_ok = smp_own if smp_ok is None else smp_ok & smp_own
    everything = ray_ok.sum() == n_rows
    lam_sem, lam_sky = cfg.get("lam_sem", S.LAMBDA_SEM), cfg.get("lam_sky", S.LAMBDA_SKY)
    weights = [1.0, 1.0, cfg.get("lam_o", S.R.LAMBDA_O), cfg.get("lam_d", S.R.LAMBDA_D), lam_sem, lam_sky]
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
            what = "d_sig" if key == "d_sem" else key
            misses.append(f"{key}: {bad.sum()} of {sel.sum()} miss; worst at {TF.where(x, what, worst // width, n_rays)}: got "
                          f"{g.ravel()[worst]!r}, reference {w.ravel()[worst]!r}, bar {bar.ravel()[worst]:.3g}")

    if got["n_valid"][0] != ref["n_valid"]:
        misses.append(f"n_valid workspace: got {got['n_valid'][0]}, reference {ref['n_valid']}")
    if not np.array_equal(got["total"][ray_ok], ref["total"][ray_ok]):
        i = int(np.nonzero(ray_ok & (got["total"] != ref["total"]))[0][0])
        misses.append(f"total_samples: {TF.where(x, 'total', i, n_rays)}: got {got['total'][i]}, reference {ref['total'][i]}")
    if got["vr"][0] != got["total"][ray_own].sum() or (everything and got["vr"][0] != ref["vr"][0]):
        misses.append(f"vr_samples: got {got['vr'][0]}, sum of total_samples {got['total'][ray_own].sum()}, reference {ref['vr'][0]}")
    for key in PER_RAY + PER_SAMPLE:        # what no processed row owns is left alone
        own = smp_own if key in PER_SAMPLE else ray_own
        if not np.isnan(got[key][~own]).all():
            misses.append(f"{key}: entries that no processed row owns were written")
    if not (got["total"][~ray_own] == -7).all():
        misses.append("total_samples: entries that no processed row owns were written")
    # shared with ngp_render_loss_fused: its bars
    for key in ("opacity", "depth", "rgb", "normal", "sem"):
        held(key, got[key], ref[key], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref[key]), ray_ok)
    held("ws", got["ws"], ref["ws"], TF.FW_ATOL + TF.FW_RTOL * np.abs(ref["ws"]), smp_ok)
    for key in ("Ro", "Rp"):
        held(key, got[key], ref[key], max(TF.NOISE_FACTOR * noise[key], TF.FW_ATOL), ray_ok)
    held("d_rgb", got["d_rgb"], ref["d_rgb"], TF.BW_ATOL / n_rows + TF.BW_RTOL * np.abs(ref["d_rgb"]), smp_ok, scale=n_rows)
    # new or changed by the semantic terms: 8 x the float32 restatement's error, floor 2e-5 / n_rays x the term's weight
    held("d_sig", got["d_sig"], ref["d_sig"], max(TF.NOISE_FACTOR * noise["d_sig"], TF.BW_ATOL / n_rows), smp_ok, scale=n_rows)
    held("d_sem", got["d_sem"], ref["d_sem"], max(TF.NOISE_FACTOR * noise["d_sem"], TF.BW_ATOL / n_rows * lam_sem), smp_ok,
         scale=n_rows)
    assert got["terms"].shape == (6,)
    bars = np.maximum(TF.NOISE_FACTOR * noise["terms"], TF.FW_ATOL * np.array(weights))
    bars[4:] = np.maximum(TF.NOISE_FACTOR * noise["terms"][4:], TF.BW_ATOL / n_rows * np.array(weights[4:]))
    print(f"FIG {tag} terms: got {got['terms']}, |err| {np.abs(got['terms'] - ref['terms'])}, bars {bars}")
    for i in range(6):
        if not abs(float(got["terms"][i]) - ref["terms"][i]) <= bars[i]:
            misses.append(f"terms[{i}]: got {got['terms'][i]!r}, reference {ref['terms'][i]!r}, bar {bars[i]:.3g}")
    print(f"FIG {tag} float32 noise of the restatement: " + ", ".join(f"{k} {np.max(v):.3g}" for k, v in noise.items()))
    assert not misses, f"{tag}:\n  " + "\n  ".join(misses)


def _labels_present(labels, classes):
    have = set(labels.tolist())
    assert {256, 255, -1, 4} <= have and any(0 <= v < classes for v in have), sorted(have)


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("classes", CLASSES)
def test_crafted_edges(ngp, classes, weights):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges, with the gap and the permuted rows; nothing is left out of the comparison"""
    x = batch("crafted")
    labels = S.labels_for(x, classes)
    _labels_present(labels, classes)
    lam_sem, lam_sky = WEIGHTS[weights]
    cfg = dict(classes=classes, lam_sem=lam_sem, lam_sky=lam_sky, use_scale=classes % 2 == 0)
    ref, noise = reference("crafted", labels, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert ref["terms"][5] > 0 and ref["n_valid"] >= 5
    if classes > 1:             # (one class: logsumexp(S) = S_y, the CE term and its gradient vanish)
        assert ref["terms"][4] > 0 and np.nanmax(np.abs(ref["d_sem"])) > 0
    got = run_sem(ngp, x, labels, **cfg)
    against_reference(f"crafted classes={classes} {weights}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("name,classes", [("300", 7), ("300", 10), ("1500", 3), ("1500", 16)])
def test_random_batch(ngp, name, classes, weights):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of
    T_threshold in float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the
    loss terms are compared all the same).  Labels do not affect stops."""
    x = batch(name)
    labels = S.labels_for(x, classes)
    _labels_present(labels, classes)
    lam_sem, lam_sky = WEIGHTS[weights]
    cfg = dict(classes=classes, lam_sem=lam_sem, lam_sky=lam_sky)
    ok, ray_ok, smp_ok = S.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= S.MAX_BORDERLINE
    ref, noise = reference(name, labels, **cfg)
    got = run_sem(ngp, x, labels, **cfg)
    against_reference(f"random-{name} classes={classes} {weights}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("classes", [7, 10])
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows, classes):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9); n_valid counts these rows only, and the seeds scale with 1 / rows and
    1 / n_valid.  Everything that belongs to the other rows is left alone."""
    x = batch("crafted")
    labels = S.labels_for(x, classes)
    cfg = dict(classes=classes, n_rays=rows, lam_sem=1.0, lam_sky=1.0)
    ref, noise = reference("crafted", labels, **cfg)
    assert 1 <= ref["n_valid"] <= rows
    got = run_sem(ngp, x, labels, **cfg)
    against_reference(f"crafted rows={rows} classes={classes}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts
@pytest.mark.parametrize("classes", [7, 10])
def test_wide_logit_rows(ngp, classes):
    """sem_logits (and normal_head) as the leading columns of 20-wide matrices whose other columns hold NaN: d_sem_logits
    stays dense (n, classes) and every output is that of the dense call, bit for bit"""
    x = batch("crafted")
    labels = S.labels_for(x, classes)
    cfg = dict(classes=classes, use_scale=True, lam_sem=1.0, lam_sky=1.0)
    a = run_sem(ngp, x, labels, **cfg)
    b = run_sem(ngp, x, labels, ld=20, **cfg)
    assert np.isfinite(a["terms"]).all() and b["d_sem"].shape == (x["n"], classes)
    TF._same_launch(a, b, 4)


def test_memset_branches(ngp):
    """terms and vr_samples adjacent as rendering._RenderLossFn lays them out (one fill) and in separate allocations
    (two fills), both pre-filled with NaN / a large negative count"""
    x = batch("crafted")
    labels = S.labels_for(x, 10)
    cfg = dict(classes=10)
    a = run_sem(ngp, x, labels, adjacent=True, **cfg)
    b = run_sem(ngp, x, labels, adjacent=False, **cfg)
    TF._same_launch(a, b, 4)
    ref, noise = reference("crafted", labels, **cfg)
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference(f"crafted memset {tag}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- e. no valid label
@pytest.mark.parametrize("classes", [3, 7, 16])
def test_batch_without_a_valid_label(ngp, classes):
    """256, 255, -1, `classes` (and 4 where it is not a class): everything finite, CELoss exactly 0, d_sem_logits exactly
    0 where a row owns the sample — torch's 0 / 0 is the documented difference — and the rest as the restatement"""
    x = batch("crafted")
    labels = S.labels_for(x, classes, valid=False)
    assert not ((labels >= 0) & (labels < classes)).any() and (4 in labels.tolist()) == (classes <= 4)
    cfg = dict(classes=classes, lam_sem=1.0, lam_sky=1.0)
    got = run_sem(ngp, x, labels, **cfg)
    own = S.owned(x)[0] >= 0
    assert got["n_valid"][0] == 0 and got["terms"][4] == 0.0 and np.isfinite(got["terms"]).all()
    assert not got["d_sem"][own].any() and not np.isnan(got["d_sem"][own]).any()
    assert np.isfinite(got["d_sig"][own]).all() and np.isfinite(got["d_rgb"][own]).all()
    assert (got["terms"][5] > 0) == (classes <= 4)
    ref, noise = reference("crafted", labels, **cfg)
    against_reference(f"crafted no valid label classes={classes}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_zero_weights_give_the_existing_tail(ngp, name):
    """lambda_sem = lambda_sky = 0: every output this entry shares with ngp_render_loss_fused agrees with that entry on the
    same inputs within the shared bars (a comparison of two float32 launches: rtol / atol of the module docstring); whether
    they agree bit for bit is reported"""
    x = batch(name)
    labels = S.labels_for(x, 7)
    a = run_sem(ngp, x, labels, classes=7, lam_sem=0.0, lam_sky=0.0)
    xb = dict(x, sem=np.ascontiguousarray(x["sem"][:, :8]))
    b = TF.run_tail(ngp, xb, classes=7)
    own, n_rows = S.owned(x)[0] >= 0, len(x["rays_a"])
    exact = []
    for key in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb"):
        same = np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f")
        exact.append(same)
        if key in ("total", "vr"):
            assert same, key
            continue
        sel = own if key in ("ws", "d_sig", "d_rgb") else np.ones(len(a[key]), bool)
        rtol, atol = (TF.BW_RTOL, TF.BW_ATOL / n_rows) if key.startswith("d_") else (TF.FW_RTOL, TF.FW_ATOL)
        np.testing.assert_allclose(a[key][sel], b[key][sel], rtol=rtol, atol=atol, err_msg=key)
    print(f"FIG zero-weights {name}: shared outputs bit for bit: {all(exact)} ({sum(exact)} of {len(exact)})")
    np.testing.assert_allclose(a["terms"][:4], b["terms"], rtol=(n_rows // 8 + 1) * TF.REORDER, atol=0)
    assert a["terms"][4] == 0.0 and a["terms"][5] == 0.0 and not a["d_sem"][own].any()


# ------------------------------------------------------------------------------------------- g. autograd
def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def _grid_buffers(model):
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    return model


def _scene_labels(scene, o, d, classes, gen):
    """the scene's labels (0-4, 256), with a fifth of the rays spread over all `classes`: valid labels or 256 only"""
    lab = scene.ground_truth_labels(o, d, n_quad=64)
    rnd = torch.randint(classes, lab.shape, device=DEV, generator=gen)
    lab = torch.where(torch.rand(lab.shape, device=DEV, generator=gen) < 0.2, rnd, lab)
    assert bool(((lab >= 0) & (lab < classes) | (lab == 256)).all())
    return lab


@pytest.mark.parametrize("classes", [7, 10])
def test_fused_semantic_tail_matches_the_launch_per_operation_route(ngp, classes):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes.  A: render + NeRFLoss(semantic=True) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, terms={'semantic': ...}, packed=True) through rendering._RenderLossFn.
    tests/test_mask_gpu.py's tolerances for its masked-tail-against-layered comparison."""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(33)
    model = _grid_buffers(ngp.networks.NGP(scale=8.0, classes=classes).to(DEV))
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    labels = _scene_labels(scene, o, d, classes, gen)
    assert int((labels == 4).sum()) > 100 and int((labels == 256).sum()) > 0
    loss_fn = NeRFLoss()
    lam = (loss_fn.lambda_opa, loss_fn.lambda_distortion, loss_fn.lambda_semantic, loss_fn.lambda_sky)
    named = [(n, p) for n, p in model.named_parameters() if p.numel() > 0]
    out = {}
    for fused in (False, True):
        for _, p in named:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, num_classes=classes, random_bg=True)
        if fused:
            tail = FusedTail(gt, lam[0], lam[1], terms={"semantic": (labels, lam[2], lam[3])}, packed=True)
            res = render(model, o, d, _fused_loss=tail, **kw)
            assert "_loss_terms" in res
            terms = res.pop("_loss_terms")
            assert terms.shape == (6,) and terms.requires_grad
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0, 0, 0], device=DEV)])
            terms = N(terms)
        else:
            res = render(model, o, d, **kw)
            ld = loss_fn(res, {"rgb": gt, "label": labels}, semantic=True)
            loss = sum(t.mean() for t in ld.values())
            loss.backward()
            terms = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in
                                                        ("rgb", "opacity", "distortion", "CELoss", "sky_depth")], np.float32)
        out[fused] = (res, terms, {n: None if p.grad is None else N(p.grad).copy() for n, p in named})
    ra, ta, ga = out[False]
    rb, tb, gb = out[True]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for key in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp"):
        _close(N(rb[key]), N(ra[key]), 2e-5, 2e-6)
    print("FIG autograd terms A", ta, "terms B", tb)
    _close(tb, ta, 1e-4, 1e-9)
    assert tb[4] > 0 and tb[5] > 0
    for name in ga:
        a, b = ga[name], gb[name]
        if a is None:
            assert b is None or not b.any(), name
            continue
        scale = np.abs(a).max()
        print(f"FIG autograd grad {name}: max|a - b| / max|a| = {np.abs(a - b).max() / max(scale, 1e-300):.3g}")
        assert np.abs(a - b).max() <= 3e-4 * scale + 1e-12, (name, np.abs(a - b).max(), scale)
    for name in ("semantic_header.params", "rgb_encoder.params", "xyz_encoder.params"):
        assert np.abs(gb[name]).sum() > 0, name


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed semantic term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs and d_sem_logits bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x = batch("crafted")
    classes = 10
    labels = S.labels_for(x, classes)
    direct = run_sem(ngp, x, labels, classes=classes, use_scale=True)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt", "bg", "scale3")}
    sig, rgbs = t["sig"].requires_grad_(True), t["rgbs"].requires_grad_(True)
    logits = t["sem"][:, :classes].contiguous().requires_grad_(True)
    args = (sig, rgbs, logits, t["nrm"], None, t["dsig"], t["dirs"], t["deltas"], t["ts"], t["rays_a"])
    tail = FusedTail(t["gt"], S.R.LAMBDA_O, S.R.LAMBDA_D, terms={"semantic": (T(labels), S.LAMBDA_SEM, S.LAMBDA_SKY)}, packed=True)
    outs = _RenderLossFn.apply(*args, tail, t["scale3"], 1e-4, classes, t["bg"])
    terms = outs[0]
    assert terms.shape == (6,) and terms.requires_grad and not any(o.requires_grad for o in outs[1:] if o is not None)
    seed = torch.zeros_like(terms)
    seed[0] = 1.0
    torch.autograd.backward([terms], [seed])
    own = S.owned(x)[0] >= 0
    got = dict(zip(("terms", "total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp"), (N(o) for o in outs)))
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp"):
        assert np.array_equal(got[k], direct[k]), k
    np.testing.assert_allclose(got["terms"], direct["terms"], rtol=4 * TF.REORDER, atol=0)
    assert np.array_equal(N(sig.grad)[own], direct["d_sig"][own])
    assert np.array_equal(N(rgbs.grad)[own], direct["d_rgb"][own])
    assert logits.grad.shape == (x["n"], classes) and np.array_equal(N(logits.grad)[own], direct["d_sem"][own])
    with pytest.raises(ValueError):
        _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"semantic": (T(labels)[:5], 0.0, 0.0)}, packed=True),
                            t["scale3"], 1e-4, classes, None)


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_semantic_route_matches_module_route(ngp):
    """NGPTrainer(semantic=True) with step(labels=) follows the trajectory of NGPTrainer(loss_kwargs={'semantic': True})
    with step(target={'label': ...}) for six steps of 1024 rays (labels in range or 256): the construction and bars of
    test_trainer_fused_loss_path_matches_module_path, plus semantic_header.params within the same bar, which also moved"""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(51)
    batches = []
    for i in range(6):
        img, pix = scene.sample_batch(1024, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        batches.append((o, d, gt, _scene_labels(scene, o, d, 7, gen)))
    out = []
    for fused in (True, False):
        torch.manual_seed(52)
        model = _grid_buffers(ngp.networks.NGP(scale=0.5).to(DEV))
        start = N(model.semantic_header.params).copy()
        tr = NGPTrainer(model, lr=1e-2, semantic=True) if fused else NGPTrainer(model, lr=1e-2, loss_kwargs={"semantic": True})
        assert tr.fused_loss == fused and tr.semantic == fused
        torch.manual_seed(53)
        if fused:
            losses = [float(tr.step(o, d, gt, labels=lab)[0]) for o, d, gt, lab in batches]
        else:
            losses = [float(tr.step(o, d, gt, target={"label": lab})[0]) for o, d, gt, lab in batches]
        tr.wait()
        out.append((losses, N(model.xyz_net[0].weight).copy(), N(model.rgb_net.params).copy(),
                    N(model.semantic_header.params).copy()))
        assert np.abs(out[-1][3] - start).max() > 1e-3          # the head was trained
    print("FIG trainer losses fused", out[0][0], "module", out[1][0])
    _close(np.array(out[0][0]), np.array(out[1][0]), 1e-3, 1e-7)
    for k in (1, 2, 3):
        print(f"FIG trainer params[{k}]: max|diff| {np.abs(out[0][k] - out[1][k]).max():.3g}")
        _close(out[0][k], out[1][k], 5e-3, 5e-5)


def test_trainer_semantic_argument_checks(ngp):
    """a missing labels= and every combination the semantic tail does not cover raise ValueError"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()              # (a refused construction leaves the model as it was: one model serves them all)
    refused = [dict(msk_model=implicit_mask().to(DEV)),
               dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True}),
               dict(num_classes=17), dict(num_classes=5)]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, semantic=True, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), semantic=True)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    some = torch.zeros(64, dtype=torch.int64, device=DEV)
    plain = NGPTrainer(model)
    with pytest.raises(ValueError):
        plain.step(o, d, gt, labels=some)
    # combines with appearance codes and a random background; labels of every kind, no valid one included
    model = make(embed_a=True, embed_a_len=4, classes=10)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, semantic=True, num_classes=10, embedding_a=emb, exp_step_factor=1 / 256,
                    render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, labels=some, target={"label": None})
    before = N(model.semantic_header.params).copy()
    odd = torch.tensor([256, 255, -1, 10, 300], device=DEV).repeat(13)[:64]
    loss, _ = tr.step(o, d, gt, labels=odd, img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all()
    assert np.array_equal(N(model.semantic_header.params), before)          # zero gradient, fresh Adam state: no move
    loss, res = tr.step(o, d, gt, labels=torch.randint(10, (64,), device=DEV), img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and not np.array_equal(N(model.semantic_header.params), before)
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without labels
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, labels=some, img_idxs=img)
    model.differentiable_normals = False


# ------------------------------------------------------------------------------------------- i. end to end
@pytest.mark.parametrize("fmt", ["tnt", "colmap"])
def test_train_dataset_with_labels_end_to_end(ngp, tmp_path, fmt):
    """the proxy scene with labels in the tnt layout (and in the colmap layout, whose loader reads the labels of all
    frames: train_dataset.labels_of_split pairs them with the split's images) (34 views of 80 x 80, every 8th held out), train_dataset.train(...,
    semantic=True) for 600 steps of 2048 rays.  Held-out PSNR keeps test_train_from_other_dataset_formats' bar (mean > 20
    dB); the held-out label accuracy must beat the share of the majority class among the valid held-out pixels by three
    standard errors of that proportion; tools/render.py --render_semantic renders the checkpoint.

    The model is built at scale 2, not the 0.5 of the unlabelled test: the sky term rewards depth on the 70 % of the rays
    labelled 4, i.e. black density at the far end of the volume, and the loader puts the cameras at radius 0.83.  A
    volume of half-width 0.5 ends inside the camera ring, so that density lands between the object and the cameras on
    the other side (measured at scale 0.5: held-out PSNR 29.6 / 16.5 / 10.1 / 17.3 / 11.5 dB, against 28.5 / 24.3 / 21.7 /
    23.9 / 18.2 with lambda_sky = 0 and 28.5 / 24.5 / 21.9 / 24.2 / 19.0 without labels); the reference uses the term on
    scenes whose cameras are inside the volume, and at scale 2 so are these (31.1 / 26.4 / 22.4 / 21.8 / 23.7 dB)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render as render_tool
    import train_dataset as td
    from ngp_amd import ckpt
    from ngp_amd.datasets import dataset_dict
    from ngp_amd.evaluation import evaluate_split, semantic_summary
    from ngp_amd.synthetic import LegoProxy
    C = 5
    scene = LegoProxy(n_images=34, img_wh=(80, 80), device=DEV)
    root = td.make_labelled_proxy(str(tmp_path / "scene"), fmt, scene, n_quad=128)
    train_set = dataset_dict[fmt](root, "train", 1.0, device=DEV, use_sem=True, num_classes=C)
    test_set = td.labels_of_split(dataset_dict[fmt](root, "test", 1.0, device=DEV, use_sem=True, num_classes=C))
    assert td.cameras_outside(train_set, 0.5) is not None and td.cameras_outside(train_set, 2.0) is None
    assert len(test_set) == 5 and test_set.labels.shape == (5, 80 * 80) and int(train_set.labels.max()) == 255
    torch.manual_seed(43)
    model = td.build_model(2.0, DEV, num_classes=C)
    tr = td.train(model, train_set, num_epochs=3, steps_per_epoch=200, batch_size=2048, lr=1e-2, semantic=True, num_classes=C)
    assert tr.global_step == 600 and tr.semantic and train_set.labels.shape == (29, 80 * 80)
    res = evaluate_split(model, test_set, num_classes=C)
    psnrs = res["psnr"]
    assert len(psnrs) == 5 and sum(psnrs) / 5 > 20.0, psnrs
    lab = test_set.labels.cpu().numpy()
    valid = (lab >= 0) & (lab < C)
    n_valid = valid.sum(1)
    counts = np.bincount(lab[valid], minlength=C)
    p = counts.max() / counts.sum()
    acc = float((np.array(res["sem_acc"]) * n_valid).sum() / n_valid.sum())
    assert res["sem_valid"] == n_valid.tolist() and semantic_summary(res)[0] == pytest.approx(acc, abs=1e-12)
    bar = p + 3 * np.sqrt(p * (1 - p) / n_valid.sum())
    print(f"FIG end-to-end {fmt}: psnr {sum(psnrs) / 5:.2f} dB, sem_acc {acc:.4f} (per image {res['sem_acc']}), sem_miou "
          f"{sum(res['sem_miou']) / 5:.4f} (per image {res['sem_miou']}), majority share {p:.4f}, bar {bar:.4f}, "
          f"valid pixels {int(n_valid.sum())}")
    assert acc > bar
    path = str(tmp_path / "sem.ckpt")
    ckpt.save_ckpt(model, path)
    out_dir = str(tmp_path / "frames")
    render_tool.main(["--ckpt", path, "--root_dir", root, "--dataset_name", fmt, "--out_dir", out_dir, "--render_semantic",
                      "--render_rgb", "--num_classes", str(C), "--scale", "2"])
    from PIL import Image
    frames = sorted(f for f in os.listdir(out_dir) if f.endswith("-semantic.png"))
    assert len(frames) == 5
    with Image.open(os.path.join(out_dir, frames[0])) as im:
        assert im.size == (80, 80) and len(im.getcolors(80 * 80)) >= 3          # several classes were drawn
