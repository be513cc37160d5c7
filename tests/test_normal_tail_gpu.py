"""The normal_mono form of the fused render + loss tail on the GPU (render_loss_fused_kernel<8, 32, false, false, true>
behind ngp_render_loss_fused_nrm) against the float64 restatement of tests/normal_tail_reference.py, and the routes
built on it: rendering._RenderLossFn, NGPTrainer(normal_mono=True), tools/train_dataset.py --normal_mono.

Bars.  The outputs this entry shares with ngp_render_loss_fused keep tests/test_fused_tail_gpu.py's bars: opacity, depth,
rgb, normal_pred, semantic, ws rtol 2e-5, atol 2e-6; d_sigmas, d_rgbs rtol 2e-4, atol 2e-5 / n_rays; Ro, Rp and
terms[0:4] 8 times the float32 restatement's own error on the same inputs, not below 2e-6 (times the term's weight).
d_normal_head and terms[4] are held to 8 times the float32 restatement's error as well, with the floor 2e-5 / n_rays
times lambda_nm.  Each case runs at NeRFLoss's weight (1e-3) and at lambda_nm = 1.  No ray is left out of a comparison
for the jump of sign(N^ - g^): the targets keep every component 1e-3 away from it by construction
(normal_tail_reference.make_normals).  Every figure is printed (FIG lines) before it is asserted; the measured maxima
are in profiles/normal_tail.txt.

Measured on one MI355X, end to end (test_train_dataset_with_normals_end_to_end, profiles/normal_mono.txt): held-out PSNR
27.35 dB and 13.0 degrees with lambda_normal_mono = 1e-3, 23.61 dB and 101.6 degrees with 0 (max - min 53.2 degrees)."""
import os
import sys

import numpy as np
import pytest
import torch

import normal_tail_reference as NR
from tail_harness import (DEV, TRAJ_LR, N, T, _grid_buffers, _same_launch, against_reference, batch, fused_against_layered,
                          make_normals, reference, run_entry, same_as_default, trainer_against_module, wrapper_against_direct)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = {"nerfloss": NR.LAMBDA_NM, "unit": 1.0}


def _zeros_present(x, normals, n_rays=None):
    g = normals[x["rays_a"][:n_rays, 0]]
    zero = ~(g != 0).any(1)
    assert zero.any() and (~zero).any()


# ------------------------------------------------------------------------------------------- a. crafted edges
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_crafted_edges(ngp, weights, use_scale):
    """27 rays, one per (length, stop) case of fused_tail_reference.CASES: lengths and stop samples on both sides of the
    32-sample chunk edges (length 0 included), with the gap and the permuted rows; nothing is left out of the comparison"""
    x, tg = batch("crafted"), {"normals": make_normals("crafted")}
    _zeros_present(x, tg["normals"])
    cfg = dict(lam_nm=WEIGHTS[weights], use_scale=use_scale)
    ref, noise = reference("nrm", "crafted", tg, **cfg)
    assert ref["stops"].tolist() == [-1 if s is None else s for _, s in x["cases"]]
    assert NR.sign_margin(x, tg["normals"]) >= NR.SIGN_MARGIN
    assert ref["terms"][4] > 0 and np.nanmax(np.abs(ref["d_np"])) > 0
    got = run_entry(ngp, "nrm", x, tg, **cfg)
    against_reference("nrm", f"crafted {weights} scale3={use_scale}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- b. random batches
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("name", ["300", "1500"])
def test_random_batch(ngp, name, weights):
    """the random batches of tests/test_fused_tail_gpu.py, under its rule for borderline rays (within 1e-3 of
    T_threshold in float64: left out of the per-ray and per-sample comparisons, at most MAX_BORDERLINE of the batch; the
    loss terms are compared all the same).  No ray is left out for the sign's jump."""
    x, tg = batch(name), {"normals": make_normals(name)}
    _zeros_present(x, tg["normals"])
    cfg = dict(lam_nm=WEIGHTS[weights])
    ok, ray_ok, smp_ok = NR.comparable(x, 1e-4, 1e-3)
    left_out = 1.0 - ok.mean()
    margin = NR.sign_margin(x, tg["normals"])
    print(f"FIG random-{name}: {x['n_rays']} rays, {x['n']} samples, borderline share {left_out:.4f}, rays left out for the "
          f"sign's jump 0 (smallest |N^ - g^| component {margin:.3g})")
    assert left_out <= NR.MAX_BORDERLINE and margin >= NR.SIGN_MARGIN
    ref, noise = reference("nrm", name, tg, **cfg)
    got = run_entry(ngp, "nrm", x, tg, **cfg)
    against_reference("nrm", f"random-{name} {weights}", got, ref, noise, x, cfg, ray_ok, smp_ok)


# ------------------------------------------------------------------------------------------- c. block edges
@pytest.mark.parametrize("rows", [1, 7, 8, 9])
def test_block_edges(ngp, rows):
    """the first `rows` rows of the crafted batch: a workgroup with idle half-waves at its barrier (1, 7), a full one (8),
    a second workgroup with one ray (9); the seeds scale with 1 / rows.  Everything that belongs to the other rows is
    left alone."""
    x, tg = batch("crafted"), {"normals": make_normals("crafted")}
    if rows > 2:
        _zeros_present(x, tg["normals"], rows)
    cfg = dict(n_rays=rows, lam_nm=1.0)
    ref, noise = reference("nrm", "crafted", tg, **cfg)
    got = run_entry(ngp, "nrm", x, tg, **cfg)
    against_reference("nrm", f"crafted rows={rows}", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- d. layouts
def test_wide_normal_rows(ngp):
    """normal_head (and sem_logits) as the leading columns of 20-wide matrices whose other columns hold NaN: d_normal_head
    stays dense (n, 3) and every output is that of the dense call, bit for bit"""
    x, tg = batch("crafted"), {"normals": make_normals("crafted")}
    cfg = dict(use_scale=True, lam_nm=1.0)
    a = run_entry(ngp, "nrm", x, tg, **cfg)
    b = run_entry(ngp, "nrm", x, tg, ld=20, **cfg)
    assert np.isfinite(a["terms"]).all() and b["d_np"].shape == (x["n"], 3)
    _same_launch(a, b, 4)


def test_memset_branches(ngp):
    """terms, vr_samples and the workspace adjacent as rendering._RenderLossFn lays them out (one fill) and in separate
    allocations (three fills), all pre-filled with NaN / negative numbers"""
    x, tg = batch("crafted"), {"normals": make_normals("crafted")}
    a = run_entry(ngp, "nrm", x, tg, adjacent=True)
    b = run_entry(ngp, "nrm", x, tg, adjacent=False)
    _same_launch(a, b, 4)
    assert a["terms"][4] == b["terms"][4]          # rounded once: no dependence on the order of the workgroups
    ref, noise = reference("nrm", "crafted", tg)
    for tag, got in (("adjacent", a), ("separate", b)):
        assert got["vr"][0] == ref["vr"][0]
        against_reference("nrm", f"crafted memset {tag}", got, ref, noise, x, {})


# ------------------------------------------------------------------------------------------- e. no target at all
def test_batch_without_a_normal(ngp):
    """every target (0, 0, 0): the term is exactly 0, d_normal_head exactly 0 where a row owns the sample, everything
    finite, and the rest as the restatement"""
    x, tg = batch("crafted"), {"normals": make_normals("crafted", "none")}
    cfg = dict(lam_nm=1.0)
    got = run_entry(ngp, "nrm", x, tg, **cfg)
    own = NR.owned(x)[0] >= 0
    assert got["terms"][4] == 0.0 and np.isfinite(got["terms"]).all()
    assert not got["d_np"][own].any() and not np.isnan(got["d_np"][own]).any()
    assert np.isfinite(got["d_sig"][own]).all() and np.isfinite(got["d_rgb"][own]).all()
    ref, noise = reference("nrm", "crafted", tg, **cfg)
    against_reference("nrm", "crafted no target", got, ref, noise, x, cfg)


# ------------------------------------------------------------------------------------------- f. the existing tail
@pytest.mark.parametrize("name", ["crafted", "1500"])
def test_zero_weight_gives_the_existing_tail(ngp, name):
    """lambda_nm = 0: every output this entry shares with ngp_render_loss_fused equals that entry's on the same inputs bit
    for bit; the loss terms bit for bit when one workgroup forms them (the first 8 rows), else within the reordering of
    one float atomic per workgroup"""
    x, tg = batch(name), {"normals": make_normals(name)}
    for n_rays in (None, 8):
        a = same_as_default(ngp, "nrm", x, tg, dict(lam_nm=0.0), n_rays)
        assert a["terms"][4] == 0.0
        sel = NR.owned(x, n_rays)[0] >= 0
        assert sel.any() and not a["d_np"][sel].any() and not np.isnan(a["d_np"][sel]).any()


def test_argument_checks(ngp):
    """the wrapper raises on what the entry refuses: more than 8 classes, a narrow normal head, a misaligned workspace,
    a missing target"""
    x, normals = batch("crafted"), make_normals("crafted")
    with pytest.raises(RuntimeError):
        run_entry(ngp, "nrm", x, {"normals": normals}, classes=9)
    t = {k: T(x[k]) for k in ("sig", "rgbs", "dsig", "nrm", "sem", "dirs", "deltas", "ts", "rays_a", "gt")}
    n, R_ = x["n"], x["n_rays"]
    E = lambda *s: torch.empty(*s, device=DEV)
    acc = E(13)
    total = torch.empty(R_, dtype=torch.int64, device=DEV)

    def call(normals_t, ws_, ld_normal=3):
        ngp._lib.call("render_loss_fused_nrm", t["sig"], t["rgbs"], t["dsig"], None, t["nrm"], ld_normal, t["sem"], 8, t["dirs"],
                      t["deltas"], t["ts"], t["rays_a"], t["gt"], None, normals_t, 1e-3, 1e-4, 7, R_, 2e-4, 3e-4, total,
                      acc[6:8].view(torch.int64), E(R_), E(R_), E(R_, 3), E(R_, 3), E(R_, 7), E(n), E(R_), E(R_, 3), acc[:5],
                      E(n), E(n, 3), ws_, E(n, 3))
    good = acc[8:12].view(torch.int32)
    call(T(normals), good)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        call(None, good)
    with pytest.raises(RuntimeError):
        call(T(normals), acc[9:13].view(torch.int32))          # 4 bytes off an 8-byte boundary
    with pytest.raises(RuntimeError):
        call(T(normals), good, ld_normal=2)


# ------------------------------------------------------------------------------------------- g. autograd
def test_fused_normal_tail_matches_the_launch_per_operation_route(ngp):
    """scale 8, exponential stepping, random background, 1500 rays of the proxy scene, same marcher noise and background
    draw on both routes, every target non-zero.  A: render + NeRFLoss(normal_mono=True) + sum of means + autograd; B:
    render with _fused_loss=FusedTail(..., terms={'normal_mono': ...}, packed=True) through rendering._RenderLossFn.  The
    bars of the semantic counterpart: terms rtol 1e-4, parameter gradients within 3e-4 of the largest entry."""
    tb, gb, _ = fused_against_layered(ngp, ("normal_mono",))
    assert tb[4] > 0
    assert np.abs(gb["norm_pred_header.params"]).sum() > 0


def test_wrapper_hands_back_the_direct_call(ngp):
    """rendering._RenderLossFn with the packed normal_mono term on the crafted batch: the outputs are those of the direct call, and back-propagating
    terms[0] with a unit seed hands back the launch's d_sigmas, d_rgbs and d_normal_head bit for bit"""
    from ngp_amd.rendering import FusedTail, _RenderLossFn
    x, tg = batch("crafted"), {"normals": make_normals("crafted")}
    tail = lambda t, _: FusedTail(t["gt"], NR.R.LAMBDA_O, NR.R.LAMBDA_D, terms={"normal_mono": (t["normals"], NR.LAMBDA_NM)},
                                  packed=True)
    direct, outs, t, args = wrapper_against_direct(ngp, "nrm", x, tg, tail, use_scale=True)
    assert N(outs[0])[4] == direct["terms"][4]
    for bad in (t["normals"][:5], t["normals"].double(), t["normals"][:, :2]):
        with pytest.raises(ValueError):
            _RenderLossFn.apply(*args, FusedTail(t["gt"], 0.0, 0.0, terms={"normal_mono": (bad, 0.0)}, packed=True),
                                t["scale3"], 1e-4, 7, None)


# ------------------------------------------------------------------------------------------- h. the trainer
def test_trainer_normal_route_matches_module_route(ngp):
    """NGPTrainer(normal_mono=True) with step(normals=) follows the trajectory of NGPTrainer(loss_kwargs={'normal_mono':
    True}) with step(target={'normal': ...}) for six steps of 1024 rays (every target non-zero), within the bars of the
    semantic counterpart: losses rtol 1e-3, parameters rtol 5e-3 / atol 5e-5, norm_pred_header.params included, which moved.

    The learning rate is TRAJ_LR = 3e-4, not the 1e-2 of a training run: tests/tail_harness.py says why, beside TRAJ_LR.
    Figures: profiles/normal_tail.txt."""
    head = "norm_pred_header.params"
    runs = trainer_against_module(ngp, ("normal_mono",), dict(normal_mono=True), TRAJ_LR, (head,))
    for fused, run in runs.items():
        assert run["tr"].recipe.normal_mono == fused
        moved = np.abs(run["end"][head] - run["start"][head]).max()
        print(f"FIG trainer {'fused' if fused else 'module'}: norm_pred_header moved by at most {moved:.3g}")
        assert moved > 3 * TRAJ_LR          # the head was trained: Adam moves a parameter by about lr per step


def test_trainer_normal_argument_checks(ngp):
    """a missing or misshapen normals= and every combination the normal tail does not cover raise ValueError; the route
    combines with appearance codes and a random background; a model that leaves the fused tail makes step() raise"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    scene = LegoProxy(n_images=4, img_wh=(20, 20), device=DEV)
    make = lambda **kw: _grid_buffers(ngp.networks.NGP(scale=0.5, **kw).to(DEV))
    model = make()              # (a refused construction leaves the model as it was: one model serves them all)
    refused = [dict(msk_model=implicit_mask().to(DEV)),
               dict(pose_refiner=PoseRefiner(scene.poses, scene.directions).to(DEV)),
               dict(semantic=True), dict(render_kwargs={"use_skybox": True}),
               dict(loss_kwargs={"normal_mono": True}), dict(loss_kwargs={"semantic": True}),
               dict(loss_kwargs={"depth_mono": True}), dict(loss_kwargs={"normal_ref": True})]
    for kw in refused:
        with pytest.raises(ValueError):
            NGPTrainer(model, normal_mono=True, **kw)
    assert model.differentiable_normals is False
    for model_kw in (dict(rgb_act="None"), dict(use_skybox=True)):
        with pytest.raises(ValueError):
            NGPTrainer(make(**model_kw), normal_mono=True)
    img, pix = scene.sample_batch(64)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV)
    some = torch.nn.functional.normalize(torch.randn(64, 3, device=DEV), dim=-1)
    plain = NGPTrainer(model)
    with pytest.raises(ValueError):
        plain.step(o, d, gt, normals=some)
    model = make(embed_a=True, embed_a_len=4)
    emb = torch.nn.Embedding(4, 4).to(DEV)
    tr = NGPTrainer(model, normal_mono=True, embedding_a=emb, exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img)
    for bad in (some[:5], some[:, :2], some.to(torch.int64), some.reshape(-1)):
        with pytest.raises(ValueError):
            tr.step(o, d, gt, img_idxs=img, normals=bad)
    with pytest.raises(ValueError):
        tr.step(o, d, gt, img_idxs=img, normals=some, target={"normal": None})
    before = N(model.norm_pred_header.params).copy()
    loss, _ = tr.step(o, d, gt, normals=torch.zeros(64, 3, device=DEV), img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and np.isfinite(N(tr.flat_param)).all()
    assert np.array_equal(N(model.norm_pred_header.params), before)          # zero gradient, fresh Adam state: no move
    loss, res = tr.step(o, d, gt, normals=some, img_idxs=img)
    tr.wait()
    assert np.isfinite(float(loss)) and not np.array_equal(N(model.norm_pred_header.params), before)
    # a model that leaves the fused tail after construction is an error, not a step on the default loss without normals
    model.differentiable_normals = True
    with pytest.raises(RuntimeError):
        tr.step(o, d, gt, normals=some, img_idxs=img)
    model.differentiable_normals = False


# ------------------------------------------------------------------------------------------- i. end to end
def test_train_dataset_with_normals_end_to_end(ngp, tmp_path):
    """the proxy scene with its analytic normal maps in the tnt layout (34 views of 80 x 80, every 8th held out),
    train_dataset.train(..., normal_mono=True) for 600 steps of 2048 rays, twice from the same seed: with
    lambda_normal_mono at NeRFLoss's 1e-3 and at 0, where the head stays untrained.  Held-out PSNR of the supervised run
    keeps test_train_from_other_dataset_formats' bar (mean > 20 dB); its mean held-out angle between predicted and target
    normals must lie below the unsupervised run's by more than that run's own max - min over the held-out images.
    Measured figures: profiles/normal_mono.txt."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd.datasets import dataset_dict
    from ngp_amd.evaluation import evaluate_split, normal_summary
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=34, img_wh=(80, 80), device=DEV)
    root = td.make_proxy_with_normals(str(tmp_path / "scene"), scene, n_quad=128)
    assert len(os.listdir(os.path.join(root, "normal"))) == 34
    test_set = dataset_dict["tnt"](root, "test", 1.0, device=DEV, normal_mono=True)
    assert len(test_set) == 5 and tuple(test_set.normals.shape) == (5, 80 * 80, 3)
    share = float((test_set.normals != 0).any(-1).float().mean())
    assert 0.05 < share < 0.9
    runs = {}
    for tag, lam in (("supervised", None), ("lambda 0", 0.0)):
        train_set = dataset_dict["tnt"](root, "train", 1.0, device=DEV, normal_mono=True)
        assert tuple(train_set.normals.shape) == (29, 80 * 80, 3)
        torch.manual_seed(43)
        model = td.build_model(0.5, DEV)
        tr = td.train(model, train_set, num_epochs=3, steps_per_epoch=200, batch_size=2048, lr=1e-2, normal_mono=True,
                      lambda_normal_mono=lam)
        assert tr.global_step == 600 and tr.recipe.normal_mono and tr.loss_fn.lambda_normal_mono == (1e-3 if lam is None else 0.0)
        res = evaluate_split(model, test_set)
        assert len(res["normal_deg"]) == 5 and all(np.isfinite(res["normal_deg"]))
        runs[tag] = (sum(res["psnr"]) / 5, normal_summary(res), res["normal_deg"], res["psnr"])
        print(f"FIG end-to-end {tag}: psnr {runs[tag][0]:.2f} dB (per image {res['psnr']}), normal_deg mean {runs[tag][1]:.2f} "
              f"(per image {res['normal_deg']}), pixels with a normal {share:.3f}")
    sup, zero = runs["supervised"], runs["lambda 0"]
    spread = max(zero[2]) - min(zero[2])
    print(f"FIG end-to-end margin: {zero[1] - sup[1]:.2f} degrees, spread of the lambda 0 run {spread:.2f}")
    assert sup[0] > 20.0, sup[3]
    assert zero[1] - sup[1] > spread, (sup[1], zero[1], spread)
