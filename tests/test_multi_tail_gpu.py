"""The fused render + loss tail with several optional terms at once on the GPU (ngp_render_loss_fused_multi: the label
count, the depth fit and render_loss_fused_kernel<CMAX, 32, false, SEM, NRM, DEP>) against the parent's single entries bit
for bit, against ngp_render_loss_fused bit for bit, against the float64 restatement of tests/multi_tail_reference.py, and
the routes built on it: rendering._RenderLossFn, NGPTrainer(multi_terms=...), tools/train_dataset.py --multi_terms.

Bars.  The outputs shared with ngp_render_loss_fused are that entry's bit for bit; against the restatement they keep
tests/test_fused_tail_gpu.py's bars (opacity, depth, rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_rgbs rtol 2e-4,
atol 2e-5 / n_rays; Ro, Rp and terms[0:4] 8 times the float32 restatement's own error, not below 2e-6 times the term's
weight).  d_sigmas, d_sem, d_np, terms[4:8] and the fit's (a, b) are held to 8 times the float32 restatement's error
against float64 on that batch, with no floor: the rule and the constants (tail_harness.NOISE_FACTOR) of the three sibling
suites.
The inputs' promises (borderline rays, the sign margin of the normals, the spread of the depths, a sky ray with a valid
depth) are checked in tests/test_multi_tail_host.py.  Every figure is printed (FIG lines) before it is asserted; the
measured maxima are in profiles/multi_tail.txt, the end-to-end figures in profiles/multi_terms.txt."""
import json
import os

import numpy as np
import pytest
import torch

import multi_tail_reference as M
from multi_tail_reference import DR, NR, R, SR
from tail_harness import (DEP, DEV, NRM, REORDER, SEM, TRAJ_LR, ULP, N, _grid_buffers, _tool, against_reference, batch,
                          fused_against_layered, multi_targets as targets, reference, run_entry, trainer_against_module,
                          wrapper_against_direct)

pytestmark = pytest.mark.gpu
WS_INTS = 30
ALL = M.TERMS
ARGS = {"bg": dict(use_bg=True, use_scale=False), "nobg-scale": dict(use_bg=False, use_scale=True)}


# ------------------------------------------------------------------------------------------- a. the parent's entries
@pytest.mark.parametrize("n_rays", [None, 8])
@pytest.mark.parametrize("name,classes", [("crafted", 7), ("crafted", 10), ("1500", 8)])
def test_single_bit_masks_are_the_single_entries(ngp, name, classes, n_rays):
    """a mask with one bit launches that term's own kernel: every per-ray and per-sample output, d_sem and d_np, the labels'
    n_valid and the fit's n_valid equal ngp_render_loss_fused_sem / _nrm / _dep's on the same inputs bit for bit.  The terms
    and (a, b) bit for bit where one workgroup forms them (8 rays); elsewhere within the reordering of one float atomic per
    workgroup (terms[0:4]) and one ulp of the once-rounded double sums (the optional terms, a, b), the siblings' bars for two
    launches on the same inputs."""
    x = batch(name, wide=True)
    tg = targets(name, classes)
    blocks = ((len(x["rays_a"]) if n_rays is None else n_rays) + 7) // 8
    cfg = dict(classes=classes, n_rays=n_rays, use_scale=True, T_thr=1e-4)
    singles = [(SEM, run_entry(ngp, "sem", x, tg, **cfg), [4, 5])]
    if classes <= 8:
        singles += [(NRM, run_entry(ngp, "nrm", x, tg, **cfg), [6]), (DEP, run_entry(ngp, "dep", x, tg, scene_scale=0.5, **cfg), [7])]
    for mask, b, slots in singles:
        a = run_entry(ngp, "multi", x, tg, mask=mask, scene_scale=0.5, **cfg)
        keys = ["total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_sig", "d_rgb"]
        keys += {SEM: ["d_sem"], NRM: ["d_np"], DEP: []}[mask]
        exact_fit = mask != DEP or blocks <= 2          # (two double addends commute; more arrive in any order)
        for key in keys:
            if key == "d_sig" and not exact_fit and not np.array_equal(a["fit"], b["fit"]):
                np.testing.assert_allclose(a[key], b[key], rtol=1e-6, atol=1e-12)
                continue
            assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (mask, key)
        if mask == SEM:
            assert a["n_valid_labels"] == int(b["n_valid"][0]) > 0
        if mask == DEP:
            assert a["n_valid_depths"] == b["n_valid"] > 1
            if exact_fit:
                assert np.array_equal(a["fit"], b["fit"]), (a["fit"], b["fit"])
            else:
                np.testing.assert_allclose(a["fit"], b["fit"], rtol=ULP, atol=0)
        opt = np.zeros(4)
        opt[np.array(slots) - 4] = b["terms"][4:]
        print(f"FIG single mask={mask} {name} classes={classes} rows={n_rays}: terms multi {a['terms']}, single {b['terms']}")
        if blocks == 1:
            assert np.array_equal(a["terms"][1:4], b["terms"][1:4]) and np.array_equal(a["terms"][4:], opt)
            assert a["terms"][0] == b["terms"][0]
        else:
            np.testing.assert_allclose(a["terms"][:4], b["terms"][:4], rtol=blocks * REORDER, atol=0)
            np.testing.assert_allclose(a["terms"][4:], opt, rtol=ULP, atol=0)
        assert all(a["terms"][s] != 0 for s in slots)


# ------------------------------------------------------------------------------------------- b. the default entry
@pytest.mark.parametrize("name,classes,mask", [(n, c, m) for n, c in (("crafted", 7), ("crafted", 16), ("1500", 8))
                                               for m in sorted(M.MASKS) if c <= 8 or m & SEM])
def test_shared_outputs_are_the_default_entrys(ngp, name, classes, mask):
    """depth, opacity, rgb, normal_pred, sem, ws, Ro, Rp, d_rgbs and the sample counts are ngp_render_loss_fused's bit for bit
    at any weight (the 16-class forms too, but for `sem`, which the default entry does not have at that width); with every
    optional weight 0 so is d_sigmas.  (a, b) of a mask with the depth term beside others is ngp_render_loss_fused_dep's bit
    for bit on up to 16 rays (one or two workgroups: the double sums do not depend on the arrival order), which together with
    the bit-equal `depth` pins the rounded product and add of the composited depth in the new kernels."""
    x = batch(name, wide=True)
    tg = targets(name, classes)
    plain = run_entry(ngp, "default", x, classes=min(classes, 8), use_scale=True)
    shared = ("total", "vr", "opacity", "depth", "rgb", "normal", "Ro", "Rp", "ws", "d_rgb")
    for zero in (False, True):
        lam = dict(lam_sem=0.0, lam_sky=0.0, lam_nm=0.0, lam_dm=0.0) if zero else {}
        got = run_entry(ngp, "multi", x, tg, mask=mask, classes=classes, use_scale=True, scene_scale=0.5, **lam)
        for key in shared + (("d_sig",) if zero else ()):
            assert np.array_equal(got[key], plain[key], equal_nan=got[key].dtype.kind == "f"), (key, zero)
        if classes <= 8:
            assert np.array_equal(got["sem"], plain["sem"], equal_nan=True), zero
        if zero:
            assert not got["terms"][4:].any()
            blocks = len(x["rays_a"]) // 8 + 1
            np.testing.assert_allclose(got["terms"][:4], plain["terms"], rtol=blocks * REORDER, atol=0)
    if mask & DEP and mask != DEP and classes <= 8:
        for rows in (7, 8, 9, 16):
            a = run_entry(ngp, "multi", x, tg, mask=mask, classes=classes, n_rays=rows, scene_scale=0.5)
            b = run_entry(ngp, "dep", x, tg, classes=classes, n_rays=rows, scene_scale=0.5)
            print(f"FIG fit mask={mask} {name} rows={rows}: multi {a['fit']}, dep {b['fit']}")
            assert np.array_equal(a["fit"], b["fit"]) and a["n_valid_depths"] == b["n_valid"] > 1
            assert np.array_equal(a["depth"], b["depth"], equal_nan=True)


# ------------------------------------------------------------------------------------------- c. the restatement
def _cases():
    out = []
    for mask in M.MULTI_MASKS:
        for classes in ((1, 5, 7, 8, 9, 10, 16) if mask & SEM else (0, 7, 8)):
            out.append((mask, classes))
    return out


@pytest.mark.parametrize("args", ["bg", "nobg-scale"])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
@pytest.mark.parametrize("mask,classes", _cases())
def test_crafted_edges(ngp, mask, classes, T_thr, args):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison.
    Among the labels a sky ray with a valid depth, so the summed depth seed is exercised."""
    x = batch("crafted", wide=True)
    tg = targets("crafted", classes, T_thr)
    scale = 0.5 if args == "bg" else 8.0
    cfg = dict(mask=mask, T_thr=T_thr, classes=classes, scene_scale=scale, **ARGS[args])
    ref, noise = reference("multi", "crafted", tg, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    if mask & SEM and mask & DEP:
        sky = M.sky_rows_with_depth(x, tg["labels"], tg["depths"])
        assert len(sky) and np.abs(ref["g_D"][sky]).max() > 0
    if mask & NRM:
        assert NR.sign_margin(x, tg["normals"], T_thr=T_thr) >= NR.SIGN_MARGIN
    got = run_entry(ngp, "multi", x, tg, **cfg)
    against_reference("multi", f"crafted mask={mask} classes={classes} T_thr={T_thr} {args}", got, ref, noise, x, cfg)


@pytest.mark.parametrize("name,mask,classes,scene_scale", [("300", 3, 9, 1.0), ("300", 5, 7, 0.5), ("300", 6, 7, 8.0),
                                                           ("300", 7, 16, 0.5), ("1500", 6, 8, 0.5), ("1500", 7, 10, 8.0)])
def test_random_batch(ngp, name, mask, classes, scene_scale):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of T_threshold in
    float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the loss terms are
    compared all the same, (a, b) when no ray is borderline)"""
    x = batch(name, wide=True)
    tg = targets(name, classes)
    cfg = dict(mask=mask, classes=classes, scene_scale=scene_scale)
    ok, ray_ok, smp_ok = M.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= M.MAX_BORDERLINE
    if mask & SEM and mask & DEP:
        assert len(M.sky_rows_with_depth(x, tg["labels"], tg["depths"]))
    ref, noise = reference("multi", name, tg, **cfg)
    got = run_entry(ngp, "multi", x, tg, **cfg)
    against_reference("multi", f"random-{name} mask={mask} classes={classes}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- d. launch shapes
@pytest.mark.parametrize("mask", [6, 7])
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows, mask):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8), a
    second workgroup with one ray (9); the seeds scale with 1 / rows.  One row is the singular system: (a, b) = (0, 0)
    exactly.  Everything that belongs to the other rows is left alone."""
    x = batch("crafted", wide=True)
    tg = targets("crafted", 7)
    cfg = dict(mask=mask, n_rays=rows, classes=7)
    ref, noise = reference("multi", "crafted", tg, **cfg)
    got = run_entry(ngp, "multi", x, tg, **cfg)
    if rows == 1:
        assert got["fit"].tolist() == [0.0, 0.0] and ref["terms"][7] > 0
    against_reference("multi", f"crafted mask={mask} rows={rows}", got, ref, noise, x, cfg)


def test_memset_branches_garbage_and_a_second_call(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), the workspace starting as -5, as all bits set and as a large positive pattern: the entry
    clears it, so the launches agree with one another and with the restatement, and a second call on the same buffers
    leaves the same per-ray and per-sample outputs bit for bit"""
    x = batch("crafted", wide=True)
    tg = targets("crafted", 7)
    cfg = dict(mask=7, classes=7, scene_scale=0.5)
    runs = [("adjacent", run_entry(ngp, "multi", x, tg, adjacent=True, twice=True, **cfg)),
            ("separate", run_entry(ngp, "multi", x, tg, adjacent=False, twice=True, **cfg)),
            ("adjacent all-ones", run_entry(ngp, "multi", x, tg, adjacent=True, garbage=-1, **cfg)),
            ("separate 0x7f7f7f7f", run_entry(ngp, "multi", x, tg, adjacent=False, garbage=0x7F7F7F7F, **cfg))]
    ref, noise = reference("multi", "crafted", tg, **cfg)
    a = runs[0][1]
    for tag, got in runs:
        for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "Ro", "Rp", "ws", "d_rgb", "d_sem", "d_np", "counts"):
            assert np.array_equal(a[k], got[k], equal_nan=a[k].dtype.kind == "f"), (tag, k)
        assert got["n_valid_labels"] == a["n_valid_labels"] and got["n_valid_depths"] == a["n_valid_depths"]
        # (the fit's five sums are doubles added in arrival order: (a, b) within an ulp, the optional terms rounded once)
        np.testing.assert_allclose(got["fit"], a["fit"], rtol=ULP, atol=0)
        np.testing.assert_allclose(got["terms"][4:], a["terms"][4:], rtol=ULP, atol=0)
        np.testing.assert_allclose(got["terms"][:4], a["terms"][:4], rtol=4 * REORDER, atol=0)
        against_reference("multi", f"crafted memset {tag}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- e. degenerate batches
@pytest.mark.parametrize("what", ["labels", "normals", "depths-none", "depths-one"])
def test_degenerate_targets(ngp, what):
    """no valid label / every normal zero / no valid depth / one valid depth: that term is exactly 0 with exactly zero
    gradients ((a, b) = (0, 0) for the fit) while the other terms and every output keep to the restatement"""
    x = batch("crafted", wide=True)
    kinds = {"labels": dict(labels="none"), "normals": dict(normals="none"), "depths-none": dict(depths="none"),
             "depths-one": dict(depths="one")}[what]
    tg = targets("crafted", 7, **kinds)
    cfg = dict(mask=7, classes=7, scene_scale=0.5)
    got = run_entry(ngp, "multi", x, tg, **cfg)
    own = M.owned(x)[0] >= 0
    if what == "labels":
        assert got["n_valid_labels"] == 0 and got["terms"][4] == 0.0 and not got["d_sem"][own].any()
        assert got["terms"][6] != 0 and got["terms"][7] != 0 and got["d_np"][own].any()
    elif what == "normals":
        assert got["terms"][6] == 0.0 and not got["d_np"][own].any()
        assert got["terms"][4] != 0 and got["terms"][7] != 0 and got["d_sem"][own].any()
    else:
        assert got["fit"].tolist() == [0.0, 0.0] and got["n_valid_depths"] == (0 if what == "depths-none" else 1)
        if what == "depths-none":
            assert got["terms"][7] == 0.0
        # without a fit the depth term has no gradient: d_sigmas is that of the semantic + normal form, to the restatement
        assert got["terms"][4] != 0 and got["terms"][6] != 0
    assert np.isfinite(got["terms"]).all() and np.isfinite(got["d_sig"][own]).all()
    ref, noise = reference("multi", "crafted", tg, **cfg)
    against_reference("multi", f"crafted degenerate {what}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f. autograd
def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with several terms on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs, d_sem and d_np bit for bit (padded with zeros to the
    inputs' widths); a term that is not named gives its input no gradient"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x = batch("crafted", wide=True)
    tg = targets("crafted", 10)
    for mask in (7, 6, 5):
        classes = 10 if mask & SEM else 7

        def tail(t, _):
            named = {}
            if mask & SEM:
                named["semantic"] = (t["labels"], SR.LAMBDA_SEM, SR.LAMBDA_SKY)
            if mask & NRM:
                named["normal_mono"] = (t["normals"], NR.LAMBDA_NM)
            if mask & DEP:
                named["depth_mono"] = (t["depths"], DR.LAMBDA_DM, 0.5)
            return FusedTail(t["gt"], R.LAMBDA_O, R.LAMBDA_D, terms=named)
        _, outs, t, args = wrapper_against_direct(ngp, "multi", x, tg, tail, opt_rtol=ULP, mask=mask, classes=classes,
                                                  use_scale=True, scene_scale=0.5)
        w = N(outs[11])
        assert w.shape == (WS_INTS,) and w.dtype == np.int32
    for bad in (dict(), dict(sky=(1,)), dict(semantic=(t["labels"][:5], 1.0, 1.0)), dict(normal_mono=(t["normals"].double(), 1.0)),
                dict(depth_mono=(t["depths"].reshape(-1, 1), 1.0, 1.0)), dict(depth_mono=(t["depths"], 1.0, 0.0))):
        with pytest.raises((ValueError, RuntimeError)):
            _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms=bad), t["scale3"], 1e-4, 7, None)


@pytest.mark.parametrize("classes", [7, 10])
def test_fused_multi_tail_matches_the_launch_per_operation_route(ngp, classes):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes, labels valid or 256, every normal non-zero, depths without NaN (where the module states the same
    loss).  A: render + NeRFLoss(semantic, normal_mono, depth_mono, scale=8) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, terms={...}) through rendering._RenderLossFn.  The bars of the three sibling
    comparisons: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
    tb, gb, tg = fused_against_layered(ngp, ALL, classes, packed=False)
    labels, depths = tg["semantic"], tg["depth_mono"]
    assert int(((labels == 4) & (depths > 0)).sum()) > 0 or int((labels == 4).sum()) > 100
    assert (tb[4:] > 0).all()
    for name in ("semantic_header.params", "norm_pred_header.params"):
        if name in gb:
            assert np.abs(gb[name]).sum() > 0, name


# ------------------------------------------------------------------------------------------- g. the trainer
def _was_bound_step(model):
    """whether the step just taken ran on the norm-bound clip: only then do the two MLP backwards note their sums with the
    field's link (link.FieldLink.bound_note), and nothing may have spoiled the bound"""
    return model.link.hits == 2 and model.link.ok


def test_trainer_multi_route_matches_module_route(ngp):
    """NGPTrainer(multi_terms=all three) with step(labels=, normals=, depths=) follows the trajectory of
    NGPTrainer(loss_kwargs={'semantic', 'normal_mono', 'depth_mono', 'scale': 0.5}) with step(target={...}) for six steps of
    1024 rays at lr = TRAJ_LR (tests/tail_harness.py says why not 1e-2), within the siblings' bars: losses rtol 1e-3,
    parameters rtol 5e-3 / atol 5e-5.  The fused route takes the exact gradient norm (the heads add to the colour table)."""
    def exact_norm(model):
        assert not _was_bound_step(model)
    runs = trainer_against_module(ngp, ALL, dict(multi_terms=ALL), TRAJ_LR, ("xyz_encoder.params", "semantic_header.params"),
                                  after_step=exact_norm)
    for fused, run in runs.items():
        tr = run["tr"]
        assert tr.recipe.multi_terms == (ALL if fused else ()) and not (tr.recipe.semantic or tr.recipe.normal_mono or tr.recipe.depth_mono)
    steps = runs[True]["steps"]
    assert all(s[1]["loss_terms"].shape == (8,) for s in steps)
    opt = np.stack([N(s[1]["loss_terms"])[4:] for s in steps])
    print("FIG trainer optional terms per step", opt.tolist())
    assert (opt > 0).all()


def test_trainer_multi_argument_checks(ngp):
    """every combination the multi tail does not cover raises ValueError; the route combines with appearance codes and a
    random background; any non-empty subset trains; degenerate targets train on; ('depth_mono',) alone keeps the norm-bound
    clip; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()
    refused = [dict(msk_model=implicit_mask().to(DEV)), dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(normal_mono=True), dict(depth_mono=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True}), dict(num_classes=5)]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, multi_terms=ALL, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), multi_terms=ALL)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    lab = torch.randint(0, 7, (64,), device=DEV)
    lab[::9] = 256
    nrm = torch.randn(64, 3, device=DEV)
    nrm[::4] = 0
    dep = 25 * (0.2 + torch.rand(64, device=DEV))
    dep[::5] = float("nan")
    full = dict(labels=lab, normals=nrm, depths=dep)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, multi_terms=ALL, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, labels=lab, normals=nrm)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, target={"depth": None}, **full)
    loss, res = tr.step(o, d, gt, img_idxs=img, **full)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and res["loss_terms"].shape == (8,)
    loss, res = tr.step(o, d, gt, img_idxs=img, labels=torch.full_like(lab, 256), normals=torch.zeros_like(nrm),
                        depths=torch.zeros_like(dep))
    tr.wait()
    t = N(res["loss_terms"])
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and not t[[4, 6, 7]].any()
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without targets
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, img_idxs=img, **full)
    model.differentiable_normals = False
    for terms in (("depth_mono",), ("normal_mono", "depth_mono"), ("semantic",)):
        tr = NGPTrainer(make(), multi_terms=terms)
        kw = {k: v for k, v in full.items() if {"labels": "semantic", "normals": "normal_mono", "depths": "depth_mono"}[k] in terms}
        loss, res = tr.step(o, d, gt, **kw)
        tr.wait()
        t = N(res["loss_terms"])
        assert t.shape == (8,) and np.isfinite(t).all()
        assert _was_bound_step(tr.model) == (terms == ("depth_mono",) and bool(tr.norm_bound))
        with pytest.raises(ValueError):
            tr.step(o, d, gt, **full) if len(kw) < 3 else tr.step(o, d, gt)


# ------------------------------------------------------------------------------------------- h. end to end
def test_train_dataset_with_all_three_terms_end_to_end(ngp, tmp_path):
    """the tool in a fresh child process under a time limit: the proxy scene with labels, normal and depth maps in the tnt
    layout (34 views of 80 x 80, every 8th held out), 600 steps of 2048 rays with --multi_terms semantic normal_mono
    depth_mono.  Barred: the JSON line has the four metrics and loss_terms == 8, every term is finite, held-out PSNR > 20 dB
    (the project's bar for 600 steps on a tnt export).  The metric values and the terms' first / last means are recorded
    (FIG lines, profiles/multi_terms.txt), not barred."""
    root = str(tmp_path / "scene")
    out = _tool(["--make_proxy", root, "--downsample", "0.1", "--proxy_views", "34", "--dataset_name", "tnt", "--num_epochs",
                    "3", "--steps_per_epoch", "200", "--batch_size", "2048", "--num_classes", "5", "--multi_terms", "semantic",
                    "normal_mono", "depth_mono"], 300)
    for sub in ("semantic", "normal", "depth"):
        assert len(os.listdir(os.path.join(root, sub))) == 34, sub
    keys = ["test_psnr_mean", "test_ssim_mean", "test_sem_acc_mean", "test_sem_miou_mean", "test_normal_deg_mean",
            "test_depth_absrel_mean"]
    keys += [f"{t}_term_{w}" for t in ("CELoss", "sky_depth", "normal_mono", "depth_mono") for w in ("first", "last")]
    for key in keys:
        assert key in out and np.isfinite(out[key]), (key, out.get(key))
    assert out["steps"] == 600 and out["img_wh"] == [80, 80] and out["loss_terms"] == 8 and out["num_classes"] == 5
    assert out["multi_terms"] == list(ALL)
    print("FIG end-to-end multi_terms: " + json.dumps({k: out[k] for k in keys}))
    assert out["test_psnr_mean"] > 20.0
