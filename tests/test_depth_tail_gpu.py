"""The depth_mono form of the fused render + loss tail on the GPU (depth_fit_kernel, then
render_loss_fused_kernel<8, 32, false, false, false, true>, behind ngp_render_loss_fused_dep) against the float64
restatement of tests/depth_tail_reference.py, and the routes built on it: rendering._RenderLossFn,
NGPTrainer(depth_mono=True), tools/train_dataset.py --depth_mono.

Bars.  The outputs this entry shares with ngp_render_loss_fused keep tests/test_fused_tail_gpu.py's bars: opacity, depth,
rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_rgbs rtol 2e-4, atol 2e-5 / n_rays; Ro, Rp and terms[0:4] 8 times
the float32 restatement's own error on the same inputs, not below 2e-6 (times the term's weight).  d_sigmas, terms[4] and
the workspace's (a, b) are held to 8 times the float32 restatement's error against float64 on that batch, with no floor
(the rule of the semantic and normal tails; d_sigmas: the largest error over the batch's samples).  The seeded depths keep
var(D) / mean(D^2) >= 0.1 over the valid rays of every batch and prefix compared here (tests/test_depth_tail_host.py).
Every figure is printed (FIG lines) before it is asserted; the measured maxima are in profiles/depth_tail.txt.

End to end (test_train_dataset_with_depths_end_to_end) held-out PSNR and depth_absrel with lambda_depth_mono = 1 and = 0
are recorded, not barred: profiles/depth_mono.txt."""
import os

import numpy as np
import pytest
import torch

import depth_tail_reference as DR
from tail_harness import (DEV, TRAJ_LR, ULP, N, T, _grid_buffers, _same_launch, _tool, against_reference, batch,
                          fused_against_layered, make_depths, reference, run_entry, same_as_default, trainer_against_module,
                          wrapper_against_direct)

pytestmark = pytest.mark.gpu
WS_INTS = 18
ARGS = {"bg": dict(use_bg=True, use_scale=False), "nobg-scale": dict(use_bg=False, use_scale=True)}


def _kinds_present(x, depths, n_rays=None):
    z = depths[x["rays_a"][:n_rays, 0]]
    assert (z > 0).sum() >= 2 and (z == 0).any() and (z < 0).any() and np.isnan(z).any()


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("scene_scale", [0.5, 8.0])
@pytest.mark.parametrize("args", ["bg", "nobg-scale"])
@pytest.mark.parametrize("T_thr", [1e-4, 1e-2])
def test_crafted_edges(ngp, T_thr, args, scene_scale):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison"""
    x, tg = batch("crafted"), {"depths": make_depths("crafted")}
    _kinds_present(x, tg["depths"])
    cfg = dict(T_thr=T_thr, scene_scale=scene_scale, **ARGS[args])
    ref, noise = reference("dep", "crafted", tg, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert DR.R.comparable(x, T_thr, 1e-2)[0].all()
    assert ref["terms"][4] > 0 and np.abs(ref["g_D"]).max() > 0
    got = run_entry(ngp, "dep", x, tg, **cfg)
    against_reference("dep", f"crafted T_thr={T_thr} {args} scale={scene_scale}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("name,scene_scale", [("300", 0.5), ("1500", 8.0)])
def test_random_batch(ngp, name, scene_scale):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of T_threshold in
    float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the loss terms are
    compared all the same, (a, b) when no ray is borderline)"""
    x, tg = batch(name), {"depths": make_depths(name)}
    _kinds_present(x, tg["depths"])
    cfg = dict(scene_scale=scene_scale)
    ok, ray_ok, smp_ok = DR.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}")
    assert left_out <= DR.MAX_BORDERLINE
    ref, noise = reference("dep", name, tg, **cfg)
    got = run_entry(ngp, "dep", x, tg, **cfg)
    print(f"FIG random-{name} fit: got {got['fit']}, reference {ref['fit']}, float32 restatement's error {noise['fit']}")
    against_reference("dep", f"random-{name} scale={scene_scale}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8), a
    second workgroup with one ray (9); the seeds scale with 1 / rows.  One row is the singular system: (a, b) = (0, 0)
    exactly.  Everything that belongs to the other rows is left alone."""
    x, tg = batch("crafted"), {"depths": make_depths("crafted")}
    if rows > 6:
        _kinds_present(x, tg["depths"], rows)
    cfg = dict(n_rays=rows)
    ref, noise = reference("dep", "crafted", tg, **cfg)
    got = run_entry(ngp, "dep", x, tg, **cfg)
    if rows == 1:
        assert ref["n_valid"] == 1 and got["fit"].tolist() == [0.0, 0.0] and ref["terms"][4] > 0
    against_reference("dep", f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts, the workspace
def test_memset_branches_and_garbage_in_the_workspace(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), the workspace starting as -5, as all bits set and as a large positive pattern: the entry
    clears it, so the four launches agree bit for bit and with the restatement"""
    x, tg = batch("crafted"), {"depths": make_depths("crafted")}
    runs = [("adjacent", run_entry(ngp, "dep", x, tg, adjacent=True)),
            ("separate", run_entry(ngp, "dep", x, tg, adjacent=False)),
            ("adjacent all-ones", run_entry(ngp, "dep", x, tg, adjacent=True, garbage=-1)),
            ("separate 0x7f7f7f7f", run_entry(ngp, "dep", x, tg, adjacent=False, garbage=0x7F7F7F7F))]
    ref, noise = reference("dep", "crafted", tg)
    a = runs[0][1]
    for tag, got in runs:
        _same_launch(a, got, 4, keys=[k for k in a if k not in ("terms", "sums", "fit", "n_valid")])
        assert got["n_valid"] == a["n_valid"]
        # (the five sums are doubles added in arrival order: (a, b) within an ulp, the term rounded once)
        np.testing.assert_allclose(got["fit"], a["fit"], rtol=ULP, atol=0)
        np.testing.assert_allclose(got["terms"][4], a["terms"][4], rtol=ULP, atol=0)
        assert got["vr"][0] == ref["vr"][0]
        against_reference("dep", f"crafted memset {tag}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- e. no depth at all
@pytest.mark.parametrize("kind", ["none", "one"])
def test_batch_without_a_fit(ngp, kind):
    """no ray with a valid depth (0, negative, NaN in turn), and one alone: (a, b) = (0, 0) exactly, d_sigmas is the default
    entry's bit for bit, the term exactly 0 without a valid ray, and everything finite"""
    x, tg = batch("crafted"), {"depths": make_depths("crafted", kind)}
    got = run_entry(ngp, "dep", x, tg)
    plain = run_entry(ngp, "default", x)
    own = DR.owned(x)[0] >= 0
    assert got["fit"].tolist() == [0.0, 0.0] and got["n_valid"] == (0 if kind == "none" else 1)
    assert np.isfinite(got["terms"]).all() and np.isfinite(got["d_sig"][own]).all()
    assert np.array_equal(got["d_sig"], plain["d_sig"], equal_nan=True)
    if kind == "none":
        assert got["terms"][4] == 0.0
    ref, noise = reference("dep", "crafted", tg)
    against_reference("dep", f"crafted depths: {kind}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_depth_and_zero_weight_give_the_existing_tail(ngp, name):
    """`depth` is ngp_render_loss_fused's bit for bit at any weight.  lambda_dm = 0: every output this entry shares with
    ngp_render_loss_fused equals that entry's on the same inputs bit for bit; the loss terms bit for bit when one workgroup
    forms them (the first 8 rows), else within the reordering of one float atomic per workgroup"""
    x, tg = batch(name), {"depths": make_depths(name)}
    full = run_entry(ngp, "dep", x, tg, scene_scale=0.5)
    assert np.array_equal(full["depth"], run_entry(ngp, "default", x)["depth"], equal_nan=True)
    for n_rays in (None, 8):
        a = same_as_default(ngp, "dep", x, tg, dict(lam_dm=0.0), n_rays)
        assert a["terms"][4] == 0.0
        assert a["n_valid"] > 0 and a["fit"][0] != 0          # the fit ran all the same


def test_argument_checks(ngp):
    """the wrapper raises on what the entry refuses: more than 8 classes, a scene scale of 0, a misaligned workspace, a
    missing target"""
    x, depths = batch("crafted"), make_depths("crafted")
    for bad in (dict(classes=9), dict(scene_scale=0.0), dict(scene_scale=-1.0)):
        with pytest.raises(RuntimeError):
            run_entry(ngp, "dep", x, {"depths": depths}, **bad)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt")}
    n, R_ = x["n"], x["n_rays"]
    E = lambda *s: torch.empty(*s, device=DEV)
    acc = E(9 + WS_INTS)
    total = torch.empty(R_, dtype=torch.int64, device=DEV)

    def call(depth_t, ws_):
        ngp._lib.call("render_loss_fused_dep", t["sig"], t["rgbs"], t["dsig"], None, t["nrm"], 3, t["sem"], 8, t["dirs"],
                      t["deltas"], t["ts"], t["rays_a"], t["gt"], None, depth_t, 1.0, 1.0, 1e-4, 7, R_, 2e-4, 3e-4, total,
                      acc[6:8].view(torch.int64), E(R_), E(R_), E(R_, 3), E(R_, 3), E(R_, 7), E(n), E(R_), E(R_, 3), acc[:5],
                      E(n), E(n, 3), ws_)
    good = acc[8:8 + WS_INTS].view(torch.int32)
    call(T(depths), good)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        call(None, good)
    with pytest.raises(RuntimeError):
        call(T(depths), None)
    with pytest.raises(RuntimeError):
        call(T(depths), acc[9:9 + WS_INTS].view(torch.int32))          # 4 bytes off an 8-byte boundary


# ------------------------------------------------------------------------------------------- g. autograd
def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed depth_mono term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas and d_rgbs bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x, tg = batch("crafted"), {"depths": make_depths("crafted")}
    tail = lambda t, _: FusedTail(t["gt"], DR.R.LAMBDA_O, DR.R.LAMBDA_D, terms={"depth_mono": (t["depths"], DR.LAMBDA_DM, 0.5)},
                                  packed=True)
    _, _, t, args = wrapper_against_direct(ngp, "dep", x, tg, tail, use_scale=True, scene_scale=0.5)
    for bad in (t["depths"][:5], t["depths"].double(), t["depths"].reshape(-1, 1)):
        with pytest.raises(ValueError):
            _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"depth_mono": (bad, 0.0, 1.0)}, packed=True),
                                t["scale3"], 1e-4, 7, None)


def test_fused_depth_tail_matches_the_launch_per_operation_route(ngp):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes.  A: render + NeRFLoss(depth_mono=True, scale=8) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(..., terms={'depth_mono': ...}, packed=True) through rendering._RenderLossFn.  The bars of the
    semantic and normal counterparts: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
    tb, _, _ = fused_against_layered(ngp, ("depth_mono",))
    assert tb[4] > 0


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_depth_route_matches_module_route(ngp):
    """NGPTrainer(depth_mono=True) with step(depths=) follows the trajectory of NGPTrainer(loss_kwargs={'depth_mono': True,
    'scale': 0.5}) with step(target={'depth': ...}) for six steps of 1024 rays at lr = TRAJ_LR (tests/tail_harness.py says
    why not 1e-2), within the bars of the semantic and normal counterparts: losses rtol 1e-3, parameters rtol 5e-3 / atol
    5e-5.  The fused route keeps the norm-bound clip (the term reaches the parameters through d_sigmas alone)."""
    runs = trainer_against_module(ngp, ("depth_mono",), dict(depth_mono=True), TRAJ_LR, ("xyz_encoder.params",))
    assert runs[True]["tr"].recipe.depth_mono and not runs[False]["tr"].recipe.depth_mono
    steps = runs[True]["steps"]
    assert all(s[1]["loss_terms"].shape == (5,) for s in steps)
    dm = [float(s[1]["loss_terms"][4]) for s in steps]
    print("FIG trainer depth_mono term per step", dm)
    assert all(v > 0 for v in dm)


def test_trainer_depth_argument_checks(ngp):
    """every combination the depth tail does not cover raises ValueError; the route combines with appearance codes and a
    random background; a batch without a valid depth trains on; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()              # (a refused construction leaves the model as it was: one model serves them all)
    refused = [dict(msk_model=implicit_mask().to(DEV)),
               dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(normal_mono=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True})]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, depth_mono=True, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), depth_mono=True)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    some = 25 * (0.2 + torch.rand(64, device=DEV))
    some[::5] = float("nan")
    plain = NGPTrainer(model)
    with pytest.raises(ValueError):
        plain.step(o, d, gt, depths=some)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, depth_mono=True, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img)
    for bad in (some[:5], some.reshape(-1, 1), some.to(torch.int64)):
        with pytest.raises(ValueError):
            tr.step(o, d, gt, img_idxs=img, depths=bad)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, depths=some, target={"depth": None})
    loss, res = tr.step(o, d, gt, depths=torch.zeros(64, device=DEV), img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and float(res["loss_terms"][4]) == 0.0
    loss, res = tr.step(o, d, gt, depths=some, img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all() and res["loss_terms"].shape == (5,)
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without depths
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, depths=some, img_idxs=img)
    model.differentiable_normals = False


# ------------------------------------------------------------------------------------------- i. end to end
def test_train_dataset_with_depths_end_to_end(ngp, tmp_path):
    """the tool in a child process: the proxy scene with monocular depth maps in the tnt layout (34 views of 80 x 80, every
    8th held out, the files 25 (0.37 D + 0.11)), 600 steps of 2048 rays with --depth_mono.  The JSON keys exist and are
    finite, the loss had five terms and the depth_mono term (mean of the last ten steps) ends below where it began (mean of
    the first ten).  Held-out PSNR and depth_absrel of that run and of a second one with --lambda_depth_mono 0 on the same
    files are recorded (FIG lines, profiles/depth_mono.txt), not barred."""
    root = str(tmp_path / "scene")
    common = ["--dataset_name", "tnt", "--num_epochs", "3", "--steps_per_epoch", "200", "--batch_size", "2048", "--depth_mono"]
    out = _tool(["--make_proxy", root, "--downsample", "0.1", "--proxy_views", "34"] + common, 300)
    assert len(os.listdir(os.path.join(root, "depth"))) == 34
    for key in ("test_psnr_mean", "test_ssim_mean", "test_depth_absrel_mean", "depth_mono_term_first", "depth_mono_term_last"):
        assert key in out and np.isfinite(out[key]), (key, out.get(key))
    assert out["steps"] == 600 and out["img_wh"] == [80, 80] and out["loss_terms"] == 5 and out["lambda_depth_mono"] == 1
    assert len(out["test_depth_absrel"]) == len(out["test_psnr"]) == 5 and np.isfinite(out["test_depth_absrel"]).all()
    print(f"FIG end-to-end lambda 1: psnr {out['test_psnr_mean']:.2f} dB (per image {out['test_psnr']}), depth_absrel mean "
          f"{out['test_depth_absrel_mean']:.4f} (per image {out['test_depth_absrel']}), depth_mono term "
          f"{out['depth_mono_term_first']:.3g} -> {out['depth_mono_term_last']:.3g}")
    assert 0 < out["depth_mono_term_last"] < out["depth_mono_term_first"]
    zero = _tool(["--root_dir", root, "--lambda_depth_mono", "0"] + common, 300)
    print(f"FIG end-to-end lambda 0: psnr {zero['test_psnr_mean']:.2f} dB (per image {zero['test_psnr']}), depth_absrel mean "
          f"{zero['test_depth_absrel_mean']:.4f} (per image {zero['test_depth_absrel']})")
    assert zero["loss_terms"] == 5 and zero["lambda_depth_mono"] == 0 and zero["depth_mono_term_last"] == 0.0
