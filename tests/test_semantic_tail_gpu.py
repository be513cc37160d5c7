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
from tail_harness import (BW_ATOL, BW_RTOL, DEV, FW_ATOL, FW_RTOL, REORDER, SHARED, N, _grid_buffers, _same_launch,
                          against_reference, batch, fused_against_layered, labels_for, reference, run_entry,
                          trainer_against_module, wrapper_against_direct)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [1, 2, 7, 8, 9, 10, 16]           # both CMAX forms and their boundary; 4 is sky but not valid for the first two
WEIGHTS = {"nerfloss": (S.LAMBDA_SEM, S.LAMBDA_SKY), "unit": (1.0, 1.0)}


def _labels_present(labels, classes):
    have = set(labels.tolist())
    assert {256, 255, -1, 4} <= have and any(0 <= v < classes for v in have), sorted(have)


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("classes", CLASSES)
def test_crafted_edges(ngp, classes, weights):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges, with the gap and the permuted rows; nothing is left out of the comparison"""
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", classes)}
    _labels_present(tg["labels"], classes)
    lam_sem, lam_sky = WEIGHTS[weights]
    cfg = dict(classes=classes, lam_sem=lam_sem, lam_sky=lam_sky, use_scale=classes % 2 == 0)
    ref, noise = reference("sem", "crafted", tg, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert ref["terms"][5] > 0 and ref["n_valid"] >= 5
    if classes > 1:             # (one class: logsumexp(S) = S_y, the CE term and its gradient vanish)
        assert ref["terms"][4] > 0 and np.nanmax(np.abs(ref["d_sem"])) > 0
    got = run_entry(ngp, "sem", x, tg, **cfg)
    against_reference("sem", f"crafted classes={classes} {weights}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("name,classes", [("300", 7), ("300", 10), ("1500", 3), ("1500", 16)])
def test_random_batch(ngp, name, classes, weights):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of
    T_threshold in float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the
    loss terms are compared all the same).  Labels do not affect stops."""
    x, tg = batch(name, wide=True), {"labels": labels_for(name, classes)}
    _labels_present(tg["labels"], classes)
    lam_sem, lam_sky = WEIGHTS[weights]
    cfg = dict(classes=classes, lam_sem=lam_sem, lam_sky=lam_sky)
    ok, ray_ok, smp_ok = S.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= S.MAX_BORDERLINE
    ref, noise = reference("sem", name, tg, **cfg)
    got = run_entry(ngp, "sem", x, tg, **cfg)
    against_reference("sem", f"random-{name} classes={classes} {weights}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("classes", [7, 10])
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows, classes):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9); n_valid counts these rows only, and the seeds scale with 1 / rows and
    1 / n_valid.  Everything that belongs to the other rows is left alone."""
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", classes)}
    cfg = dict(classes=classes, n_rays=rows, lam_sem=1.0, lam_sky=1.0)
    ref, noise = reference("sem", "crafted", tg, **cfg)
    assert 1 <= ref["n_valid"] <= rows
    got = run_entry(ngp, "sem", x, tg, **cfg)
    against_reference("sem", f"crafted rows={rows} classes={classes}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts
@pytest.mark.parametrize("classes", [7, 10])
def test_wide_logit_rows(ngp, classes):
    """sem_logits (and normal_head) as the leading columns of 20-wide matrices whose other columns hold NaN: d_sem_logits
    stays dense (n, classes) and every output is that of the dense call, bit for bit"""
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", classes)}
    cfg = dict(classes=classes, use_scale=True, lam_sem=1.0, lam_sky=1.0)
    a = run_entry(ngp, "sem", x, tg, **cfg)
    b = run_entry(ngp, "sem", x, tg, ld=20, **cfg)
    assert np.isfinite(a["terms"]).all() and b["d_sem"].shape == (x["n"], classes)
    _same_launch(a, b, 4)


def test_memset_branches(ngp):
    """terms and vr_samples adjacent as rendering._RenderLossFn lays them out (one fill) and in separate allocations
    (two fills), both pre-filled with NaN / a large negative count"""
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", 10)}
    cfg = dict(classes=10)
    a = run_entry(ngp, "sem", x, tg, adjacent=True, **cfg)
    b = run_entry(ngp, "sem", x, tg, adjacent=False, **cfg)
    _same_launch(a, b, 4)
    ref, noise = reference("sem", "crafted", tg, **cfg)
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference("sem", f"crafted memset {tag}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- e. no valid label
@pytest.mark.parametrize("classes", [3, 7, 16])
def test_batch_without_a_valid_label(ngp, classes):
    """256, 255, -1, `classes` (and 4 where it is not a class): everything finite, CELoss exactly 0, d_sem_logits exactly
    0 where a row owns the sample — torch's 0 / 0 is the documented difference — and the rest as the restatement"""
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", classes, valid=False)}
    labels = tg["labels"]
    assert not ((labels >= 0) & (labels < classes)).any() and (4 in labels.tolist()) == (classes <= 4)
    cfg = dict(classes=classes, lam_sem=1.0, lam_sky=1.0)
    got = run_entry(ngp, "sem", x, tg, **cfg)
    own = S.owned(x)[0] >= 0
    assert got["n_valid"][0] == 0 and got["terms"][4] == 0.0 and np.isfinite(got["terms"]).all()
    assert not got["d_sem"][own].any() and not np.isnan(got["d_sem"][own]).any()
    assert np.isfinite(got["d_sig"][own]).all() and np.isfinite(got["d_rgb"][own]).all()
    assert (got["terms"][5] > 0) == (classes <= 4)
    ref, noise = reference("sem", "crafted", tg, **cfg)
    against_reference("sem", f"crafted no valid label classes={classes}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_zero_weights_give_the_existing_tail(ngp, name):
    """lambda_sem = lambda_sky = 0: every output this entry shares with ngp_render_loss_fused agrees with that entry on the
    same inputs within the shared bars (a comparison of two float32 launches: rtol / atol of the module docstring); whether
    they agree bit for bit is reported"""
    x = batch(name, wide=True)
    a = run_entry(ngp, "sem", x, {"labels": labels_for(name, 7)}, classes=7, lam_sem=0.0, lam_sky=0.0)
    b = run_entry(ngp, "default", batch(name), classes=7)
    own, n_rows = S.owned(x)[0] >= 0, len(x["rays_a"])
    exact = []
    for key in SHARED:
        same = np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f")
        exact.append(same)
        if key in ("total", "vr"):
            assert same, key
            continue
        sel = own if key in ("ws", "d_sig", "d_rgb") else np.ones(len(a[key]), bool)
        rtol, atol = (BW_RTOL, BW_ATOL / n_rows) if key.startswith("d_") else (FW_RTOL, FW_ATOL)
        np.testing.assert_allclose(a[key][sel], b[key][sel], rtol=rtol, atol=atol, err_msg=key)
    print(f"FIG zero-weights {name}: shared outputs bit for bit: {all(exact)} ({sum(exact)} of {len(exact)})")
    np.testing.assert_allclose(a["terms"][:4], b["terms"], rtol=(n_rows // 8 + 1) * REORDER, atol=0)
    assert a["terms"][4] == 0.0 and a["terms"][5] == 0.0 and not a["d_sem"][own].any()


# ------------------------------------------------------------------------------------------- g. autograd
@pytest.mark.parametrize("classes", [7, 10])
def test_fused_semantic_tail_matches_the_launch_per_operation_route(ngp, classes):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes.  A: render + NeRFLoss(semantic=True) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, terms={'semantic': ...}, packed=True) through rendering._RenderLossFn.
    tests/test_mask_gpu.py's tolerances for its masked-tail-against-layered comparison."""
    tb, gb, tg = fused_against_layered(ngp, ("semantic",), classes)
    labels = tg["semantic"]
    assert int((labels == 4).sum()) > 100 and int((labels == 256).sum()) > 0
    assert tb[4] > 0 and tb[5] > 0
    assert np.abs(gb["semantic_header.params"]).sum() > 0


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed semantic term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs and d_sem_logits bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x, tg = batch("crafted", wide=True), {"labels": labels_for("crafted", 10)}
    tail = lambda t, _: FusedTail(t["gt"], S.R.LAMBDA_O, S.R.LAMBDA_D, terms={"semantic": (t["labels"], S.LAMBDA_SEM, S.LAMBDA_SKY)},
                                  packed=True)
    _, _, t, args = wrapper_against_direct(ngp, "sem", x, tg, tail, classes=10, use_scale=True)
    assert args[2].grad.shape == (x["n"], 10)
    with pytest.raises(ValueError):
        _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"semantic": (t["labels"][:5], 0.0, 0.0)}, packed=True),
                            t["scale3"], 1e-4, 10, None)


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_semantic_route_matches_module_route(ngp):
    """NGPTrainer(semantic=True) with step(labels=) follows the trajectory of NGPTrainer(loss_kwargs={'semantic': True})
    with step(target={'label': ...}) for six steps of 1024 rays (labels in range or 256): the construction and bars of
    test_trainer_fused_loss_path_matches_module_path, plus semantic_header.params within the same bar, which also moved"""
    head = "semantic_header.params"
    runs = trainer_against_module(ngp, ("semantic",), dict(semantic=True), 1e-2, (head,))
    for fused, run in runs.items():
        assert run["tr"].recipe.semantic == fused
        assert np.abs(run["end"][head] - run["start"][head]).max() > 1e-3          # the head was trained


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
    assert tr.global_step == 600 and tr.recipe.semantic and train_set.labels.shape == (29, 80 * 80)
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
