"""Host-side checks of the normal_mono training route (no GPU): the float64 restatement of the normal tail
(tests/normal_tail_reference.py) against torch autograd of losses.NeRFLoss._normal_mono, the rule for rays without a
normal, the proxy scene's analytic normals, the normal maps of the tnt layout from exporter to loader, the normal metric,
the new flag of tools/train_dataset.py, the argument checks of ngp_render_loss_fused_nrm and the trainer's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normal_tail_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_X = {}


def crafted():
    if "x" not in _X:
        x = NR.make_crafted(0)
        _X["x"] = (x, NR.composited_normals(x))
    return _X["x"]


def _module_term(ngp, x, ref, g_rows, lam_nm, keep=None):
    """losses.NeRFLoss._normal_mono on normal_pred composited ray by ray from the restatement's weights, in float64 ->
    (mean over (R, 3) with the rows outside `keep` taken out of the sum, its gradient w.r.t. the head's raw output)"""
    loss_fn = ngp.losses.NeRFLoss()
    loss_fn.lambda_normal_mono = float(np.float32(lam_nm))        # the entry takes its weight as float32
    head = torch.from_numpy(np.array(x["nrm"], np.float64)).requires_grad_(True)
    n_pred = -F.normalize(head, dim=-1, eps=1e-6)
    w = torch.from_numpy(np.nan_to_num(ref["ws"]))
    N = torch.stack([(w[s:s + n, None] * n_pred[s:s + n]).sum(0) for _, s, n in x["rays_a"]])
    per = loss_fn._normal_mono({"normal_pred": N}, {"normal": torch.from_numpy(g_rows)})
    assert per.shape == (len(x["rays_a"]), 3)
    if keep is not None:
        per = per[torch.from_numpy(keep)]
    value = per.sum() / (3 * len(x["rays_a"]))
    (grad,) = torch.autograd.grad(value, [head])
    return float(value.detach()), grad.numpy()


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("lam_nm", [NR.LAMBDA_NM, 1.0])
def test_restatement_equals_nerfloss_normal_mono(ngp, lam_nm):
    """every target non-zero: the term and its gradient w.r.t. the per-sample head outputs are torch autograd's of
    NeRFLoss._normal_mono on the same composited normals"""
    x, N_hat = crafted()
    normals = NR.make_normals(x, zeros=False, N_hat=N_hat)
    assert (normals[x["rays_a"][:, 0]] != 0).any(1).all()
    lengths = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert all(np.isclose(lengths, v, rtol=1e-6).any() for v in NR.LENGTHS)
    ref = NR.evaluate(x, normals, lam_nm=lam_nm)
    value, grad = _module_term(ngp, x, ref, normals[x["rays_a"][:, 0]].astype(np.float64), lam_nm)
    own = NR.owned(x)[0] >= 0
    assert ref["terms"].shape == (5,) and ref["terms"][4] > 0
    np.testing.assert_allclose(ref["terms"][4], value, rtol=1e-12)
    np.testing.assert_allclose(ref["d_np"][own], grad[own], rtol=1e-9, atol=1e-18)
    assert np.isnan(ref["d_np"][~own]).all() and np.abs(ref["d_np"][own]).max() > 0
    base = NR.R.evaluate(x)
    np.testing.assert_allclose(ref["terms"][:4], [base["terms"][0] + value] + list(base["terms"][1:]), rtol=1e-12)
    for key in ("d_sig", "d_rgb"):          # the term does not enter the density's or the colours' gradient
        assert np.array_equal(ref[key], base[key], equal_nan=True)


def test_restatement_seeds_and_stops():
    """q = lambda / (3 R) (sign(N^ - g^) - 0.1 g^), g_N is orthogonal to N, d_np is orthogonal to the sample's head output,
    zero behind a stop and exactly w g_N / 1e-6 (sign included) where the head's output is the zero vector; the float32
    companion stays close"""
    x, N_hat = crafted()
    normals = NR.make_normals(x, N_hat=N_hat)
    assert NR.sign_margin(x, normals) >= NR.SIGN_MARGIN
    ref = NR.evaluate(x, normals, lam_nm=1.0)
    R_ = len(x["rays_a"])
    g = normals[x["rays_a"][:, 0]].astype(np.float64)
    has = ref["has"]
    assert has.sum() >= 15 and (~has).sum() >= 2
    gh = g[has] / np.linalg.norm(g[has], axis=1, keepdims=True)
    lam = float(np.float32(1.0))
    np.testing.assert_allclose(ref["q"][has], lam / (3 * R_) * (np.sign(N_hat[has] - gh) - 0.1 * gh), rtol=1e-12, atol=1e-18)
    assert not ref["q"][~has].any() and not ref["g_N"][~has].any()
    weight = np.linalg.norm(ref["normal"][x["rays_a"][:, 0]], axis=1) > 1e-9
    assert np.abs((ref["g_N"] * N_hat).sum(1))[weight].max() < 1e-12
    row, k = NR.owned(x)
    own = row >= 0
    stop = np.array([10 ** 6 if s is None else s for _, s in x["cases"]])
    behind = own & (k > stop[np.maximum(row, 0)])
    no_target = own & ~has[np.maximum(row, 0)]
    assert not ref["d_np"][behind].any() and not ref["d_np"][no_target].any()
    head = x["nrm"].astype(np.float64)
    live = own & ~behind & ~no_target & (np.linalg.norm(head, axis=1) > 0)
    assert np.abs(ref["d_np"][live]).max() > 1e-4
    assert np.abs((ref["d_np"][live] * head[live]).sum(1)).max() < 1e-12
    dead = own & ~behind & ~no_target & (np.linalg.norm(head, axis=1) == 0) & (np.nan_to_num(ref["ws"]) > 0)
    assert dead.any()
    want = -ref["ws"][dead, None] * ref["g_N"][row[dead]] / 1e-6
    np.testing.assert_allclose(ref["d_np"][dead], want, rtol=1e-12)
    noise = NR.fp32_error(x, normals, ref=ref, lam_nm=1.0)
    assert 0 < noise["d_np"] and noise["terms"][4] < 1e-6


def test_rays_without_a_normal_leave_the_batch(ngp):
    """zero-target rows: the term and the gradient are those of the same batch with these rays' contribution removed
    and the divisor left at 3 R; with every target zero the term is 0 and so is every gradient"""
    x, N_hat = crafted()
    normals = NR.make_normals(x, N_hat=N_hat)
    g_rows = normals[x["rays_a"][:, 0]].astype(np.float64)
    has = (g_rows != 0).any(1)
    assert not has[2] and not has[5] and has[0] and has[1]
    ref = NR.evaluate(x, normals, lam_nm=1.0)
    filled = np.where(has[:, None], g_rows, [1.0, 0.0, 0.0])          # any target: these rows are taken out below
    value, grad = _module_term(ngp, x, ref, filled, 1.0, keep=has)
    own = NR.owned(x)[0] >= 0
    np.testing.assert_allclose(ref["terms"][4], value, rtol=1e-12)
    np.testing.assert_allclose(ref["d_np"][own], grad[own], rtol=1e-9, atol=1e-18)
    everything, _ = _module_term(ngp, x, ref, filled, 1.0)
    assert abs(everything - value) > 1e-3          # (the rows taken out do matter)
    none = NR.evaluate(x, np.zeros_like(normals), lam_nm=1.0)
    assert none["terms"][4] == 0.0 and not none["d_np"][own].any() and np.isfinite(none["terms"]).all()


def test_target_maker():
    for name in ("crafted", "300"):
        x = NR.make_crafted(0) if name == "crafted" else NR.make_random(300)
        normals = NR.make_normals(x)
        assert normals.dtype == np.float32 and normals.shape == (x["n_rays"], 3)
        zero = ~(normals != 0).any(1)
        assert 0.05 < zero.mean() < 0.45
        assert NR.sign_margin(x, normals) >= NR.SIGN_MARGIN


# ------------------------------------------------------------------------------------------- the scene's normals
def test_proxy_scene_normals(ngp):
    from ngp_amd.synthetic import (BOX_CENTRES, BOX_HALVES, SHELL_CENTRE, SHELL_RADII, LegoProxy, analytic_normal,
                                   analytic_part)
    scene = LegoProxy(n_images=2, img_wh=(8, 8), device="cpu")
    c = np.array(SHELL_CENTRE)
    o = torch.tensor([[0.3, 0.0, 1.5],               # straight down onto box1's top
                      [c[0] + 0.05, c[1], 1.5],      # straight down onto the shell
                      [1.5, 1.5, 1.5],               # away from the scene
                      [0.45, 0.45, 1.5],             # through the unit box, past every solid
                      [1.5, 0.0, 0.0]], dtype=torch.float32)          # along -x onto box1's +x face
    d = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.1, 1.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]])
    n = scene.ground_truth_normals(o, d, n_quad=1024)
    assert n.shape == (5, 3) and n.dtype == torch.float32
    assert n[0].tolist() == [0.0, 0.0, 1.0] and n[4].tolist() == [1.0, 0.0, 0.0]
    assert n[2].tolist() == [0.0, 0.0, 0.0] and n[3].tolist() == [0.0, 0.0, 0.0]
    radial = np.array([0.05, 0.0, np.sqrt(SHELL_RADII[1] ** 2 - 0.05 ** 2)]) / SHELL_RADII[1]
    assert abs(float(n[1].norm()) - 1) < 1e-6 and np.abs(n[1].numpy() - radial).max() < 1e-2
    # the constants describe the solids that analytic_part tests
    x = torch.rand(20000, 3, generator=torch.Generator().manual_seed(2)) - 0.5
    part = analytic_part(x)
    inside = [((x - torch.tensor(ce)).abs() < torch.tensor(h)).all(-1) for ce, h in zip(BOX_CENTRES, BOX_HALVES)]
    r = (x - torch.tensor(SHELL_CENTRE)).norm(dim=-1)
    inside.append((r > SHELL_RADII[0]) & (r < SHELL_RADII[1]))
    want = torch.full_like(part, -1)
    for k in (3, 2, 1, 0):
        want = torch.where(inside[k], k, want)
    assert torch.equal(part, want)
    nn = analytic_normal(x, part)
    assert torch.equal(nn.norm(dim=-1) > 0.5, part >= 0) and ((nn.norm(dim=-1) - 1).abs()[part >= 0] < 1e-6).all()
    # from inside the hollow the shell's normal points at the centre
    inner = torch.tensor([[c[0], c[1], c[2] + SHELL_RADII[0] + 1e-3]], dtype=torch.float32)
    assert analytic_normal(inner, torch.tensor([3]))[0, 2] < -0.99


def test_normal_maps_from_exporter_to_loader(ngp, tmp_path):
    """export_tnt(normals=) writes normal/<p>_<name>.npy as (h, w, 3) float32; the loader reads them with
    normal_mono=True, per split, into (N_img, h*w, 3); train items carry 'normal', test items do not"""
    from ngp_amd.datasets import dataset_dict, export
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=9, img_wh=(16, 16), device="cpu")
    images = export.render_scene_views(scene, range(9), rgba=False, n_quad=32)
    normals = export.render_scene_normals(scene, range(9), n_quad=64)
    assert normals.shape == (9, 16, 16, 3) and normals.dtype == np.float32
    length = np.linalg.norm(normals, axis=-1)
    assert ((np.abs(length - 1) < 1e-5) | (length == 0)).all() and 0.02 < (length > 0).mean() < 0.9
    c2w, K = scene.poses.numpy().astype(np.float64), scene.K.numpy().astype(np.float64)
    root = export.export_tnt(str(tmp_path / "tnt"), images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(9)],
                             normals=normals.astype(np.float64))
    stored = np.load(os.path.join(root, "normal", "1_00000008.npy"))
    assert stored.shape == (16, 16, 3) and stored.dtype == np.float32 and np.array_equal(stored, normals[8])
    test_set = dataset_dict["tnt"](root, "test", 1.0, normal_mono=True)
    assert test_set.normals.dtype == torch.float32 and tuple(test_set.normals.shape) == (2, 256, 3)
    assert np.array_equal(test_set.normals.numpy(), normals[[0, 8]].reshape(2, 256, 3))
    assert "normal" not in test_set[0] and "rgb" in test_set[0]
    train_set = dataset_dict["tnt"](root, "train", 1.0, normal_mono=True)
    train_set.batch_size = 64
    s = train_set[0]
    frames = np.arange(1, 8)[s["img_idxs"].numpy()]
    assert np.array_equal(s["normal"].numpy(), normals.reshape(9, 256, 3)[frames, s["pix_idxs"].numpy()])
    assert not hasattr(dataset_dict["tnt"](root, "train", 1.0), "normals")


def test_normal_degrees(ngp):
    from ngp_amd.evaluation import normal_degrees, normal_summary
    target = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    pred = torch.tensor([[0.0, 0.0, 0.5], [1.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, -1.0, 0.0]])
    assert float(normal_degrees(pred, target)) == pytest.approx((0 + 90 + 180) / 3, abs=1e-3)
    assert torch.isnan(normal_degrees(pred, torch.zeros(4, 3)))
    assert normal_summary({"normal_deg": [10.0, float("nan"), 30.0]}) == 20.0
    assert normal_summary({"normal_deg": [float("nan")]}) is None


# ------------------------------------------------------------------------------------------- the tool's flag
def test_train_dataset_flag(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    assert td.parse_args(["--root_dir", "x"]).normal_mono is False
    a = td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--normal_mono", "--embed_a", "--random_bg"])
    assert a.normal_mono and a.scale == 0.5
    for bad in (["--make_proxy", "d", "--normal_mono"], ["--make_proxy", "d", "--normal_mono", "--dataset_name", "colmap"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--normal_mono", "--embed_msk"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--normal_mono", "--optimize_ext"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--normal_mono", "--render_semantic"]):
        with pytest.raises(SystemExit) as e:
            td.parse_args(bad)
        assert e.value.code == 2, bad

    class _Set:          # a dataset without normals is refused before anything else is looked at
        batch_size = 0
    with pytest.raises(ValueError, match="normal"):
        td.train(None, _Set(), 1, 1, 64, 1e-2, normal_mono=True)


# ------------------------------------------------------------------------------------------- the C entry
def test_c_entry_checks_its_arguments(ngp):
    """classes outside [0, 8] and a negative ray count are NGP_EINVAL, an empty batch is NGP_OK before any pointer is
    looked at (every pointer is NULL here: nothing may reach a launch)"""
    _lib = ngp._lib
    lib = _lib.load()
    _, args = _lib.PROTOS["ngp_render_loss_fused_nrm"]
    names = [a for _, a in args]
    assert names[-4:] == ["dL_drgbs", "nrm_ws", "dL_dnormal_head", "stream"]
    assert names[names.index("rgb_bg") + 1:names.index("rgb_bg") + 4] == ["normals_gt", "lambda_nm", "T_threshold"]
    _, plain = _lib.PROTOS["ngp_render_loss_fused"]
    assert [a for a in names if a not in ("normals_gt", "lambda_nm", "nrm_ws", "dL_dnormal_head")] == [a for _, a in plain]

    def run(classes, n_rays, ld_sem=8, ld_normal=3):
        vals = []
        for t, a in args:
            if t is C.c_void_p:
                vals.append(None)
            elif t is C.c_float:
                vals.append(1.0)
            else:
                vals.append({"classes": classes, "n_rays": n_rays, "ld_normal": ld_normal, "ld_sem": ld_sem}[a])
        return lib.ngp_render_loss_fused_nrm(*vals)
    for n_rays in (0, 5):
        assert run(9, n_rays) == -22 and run(-1, n_rays) == -22 and run(7, n_rays, ld_normal=2) == -22
    assert run(0, 0) == 0 and run(8, 0) == 0 and run(7, 0) == 0
    assert run(7, -1) == -22 and run(7, 0, ld_sem=6) == -22
    assert run(7, 5) == -22            # NULL pointers with rays to process


# ------------------------------------------------------------------------------------------- the trainer
def test_trainer_refuses_what_the_normal_tail_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer

    class _Head:
        n_output_dims = 7

    class _Model:          # what the checks look at
        rgb_act, use_skybox, differentiable_normals = "Sigmoid", False, False
        semantic_header = _Head()
    refused = [dict(msk_model=implicit_mask()), dict(pose_refiner=object()), dict(semantic=True),
               dict(render_kwargs={"use_skybox": True}), dict(loss_kwargs={"normal_mono": True}),
               dict(loss_kwargs={"semantic": True}), dict(loss_kwargs={"depth_mono": True}),
               dict(loss_kwargs={"normal_ref": True}), dict(num_classes=9)]
    for kw in refused:
        model = _Model()
        with pytest.raises(ValueError):
            NGPTrainer(model, normal_mono=True, **kw)
        assert model.differentiable_normals is False
    for attr, value in (("rgb_act", "None"), ("use_skybox", True), ("differentiable_normals", True)):
        model = _Model()
        setattr(model, attr, value)
        with pytest.raises(ValueError, match="normal_mono=True"):
            NGPTrainer(model, normal_mono=True)
