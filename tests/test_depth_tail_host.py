"""Host-side checks of the depth_mono training route (no GPU): the float64 restatement of the depth tail
(tests/depth_tail_reference.py) against torch autograd of losses.NeRFLoss._depth_mono, the fit against numpy's least
squares, the singular systems, the conditioning promise of the seeded depths, the proxy scene's depths, the depth metric,
the new flag of tools/train_dataset.py, the argument checks of ngp_render_loss_fused_dep and the trainer's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import depth_tail_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_X = {}


def crafted():
    if "x" not in _X:
        x = DR.make_crafted(0)
        _X["x"] = (x, DR.R.render(x)["depth"].detach().numpy())
    return _X["x"]


def _module_term(ngp, D, depth_rows, lam_dm, scale):
    """losses.NeRFLoss(depth_mono=True, scale=) on float64 tensors -> (mean of the 'depth_mono' entry, its autograd
    gradient w.r.t. results['depth'])"""
    loss_fn = ngp.losses.NeRFLoss()
    loss_fn.lambda_depth_mono = float(np.float32(lam_dm))          # the entry takes its weight as float32
    loss_fn.lambda_distortion = 0
    depth = torch.from_numpy(np.array(D, np.float64)).requires_grad_(True)
    R_ = len(D)
    results = {"rgb": torch.zeros(R_, 3, dtype=torch.float64), "opacity": torch.full((R_,), 0.5, dtype=torch.float64),
               "depth": depth}
    target = {"rgb": torch.zeros(R_, 3, dtype=torch.float64), "depth": torch.from_numpy(np.asarray(depth_rows, np.float64))}
    d = loss_fn(results, target, depth_mono=True, scale=float(np.float32(scale)))
    value = d["depth_mono"].mean()
    (grad,) = torch.autograd.grad(value, [depth], allow_unused=True)
    return float(value.detach()), np.zeros(R_) if grad is None else grad.numpy()


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("scale", [0.5, 1.0, 8.0])
def test_restatement_equals_nerfloss_depth_mono(ngp, scale):
    """the term and its gradient w.r.t. the composited depth are torch autograd's of NeRFLoss(depth_mono=True, scale=s) on
    the same depths in float64, with zero, negative and NaN targets among them; the default terms and d_rgb are untouched
    and d_sig is the default one plus the chain through the depth"""
    x, D = crafted()
    depths = DR.make_depths(x, D_ref=D)
    rows = depths[x["rays_a"][:, 0]]
    assert np.isnan(rows).any() and (rows == 0).any() and (rows < 0).any() and (rows > 0).sum() > 15
    ref = DR.evaluate(x, depths, scene_scale=scale)
    # (NaN targets: the module multiplies by valid = 0, which keeps NaN; they are zeroed for it, as 0 is invalid all the same)
    value, grad = _module_term(ngp, D, np.nan_to_num(rows.astype(np.float64)), 1.0, scale)
    assert ref["terms"].shape == (5,) and ref["terms"][4] > 0
    np.testing.assert_allclose(ref["terms"][4], value, rtol=1e-12)
    np.testing.assert_allclose(ref["g_D"], grad, rtol=1e-9, atol=1e-18)
    assert not ref["g_D"][~ref["valid"]].any() and np.abs(ref["g_D"][ref["valid"]]).max() > 0
    base = DR.R.evaluate(x)
    np.testing.assert_allclose(ref["terms"][:4], [base["terms"][0] + value] + list(base["terms"][1:]), rtol=1e-12)
    assert np.array_equal(ref["d_rgb"], base["d_rgb"], equal_nan=True)
    own = DR.owned(x)[0] >= 0
    assert np.isnan(ref["d_sig"][~own]).all() and np.abs(ref["d_sig"][own] - base["d_sig"][own]).max() > 1e-9
    # the chain through the depth: d D / d sigma by autograd of the restatement's own depth
    st = DR.R.render(x)
    (dD,) = torch.autograd.grad((st["depth"] * torch.from_numpy(ref["g_D"])).sum(), [st["sig"]])
    np.testing.assert_allclose(ref["d_sig"][own] - base["d_sig"][own], dD.numpy()[own], rtol=1e-9, atol=1e-15)
    noise = DR.fp32_error(x, depths, ref=ref, scene_scale=scale)
    assert 0 < noise["d_sig"] and noise["terms"][4] < 1e-6 and (noise["fit"] < 1e-6).all()


def test_fit_equals_lstsq():
    for name in ("crafted", "300", "1500"):
        x = DR.make_crafted(0) if name == "crafted" else DR.make_random(int(name))
        D = DR.R.render(x)["depth"].detach().numpy()
        depths = DR.make_depths(x, D_ref=D)
        ref = DR.finish(DR.R.render(x), x, depths)
        z = depths[x["rays_a"][:, 0]].astype(np.float64) / 25
        ok = z > 0
        assert ref["n_valid"] == ok.sum() and np.array_equal(ref["valid"], ok)
        A = np.stack([D[ok], np.ones(ok.sum())], 1)
        want = np.linalg.lstsq(A, z[ok], rcond=None)[0]
        np.testing.assert_allclose(ref["fit"], want, rtol=1e-9)
        assert abs(ref["fit"][0] - DR.ALPHA) < 0.01 and abs(ref["fit"][1] - DR.BETA) < 0.01


@pytest.mark.parametrize("kind", ["none", "one"])
def test_singular_systems(ngp, kind):
    """no valid ray, one valid ray: (a, b) = (0, 0), as compute_scale_and_shift gives, and the term's gradient is zero (with
    one valid ray the term itself is exp(-D / s) z^2 / R)"""
    x, D = crafted()
    depths = DR.make_depths(x, D_ref=D, kind=kind)
    ref = DR.evaluate(x, depths)
    base = DR.R.evaluate(x)
    assert ref["n_valid"] == (0 if kind == "none" else 1)
    assert ref["fit"].tolist() == [0.0, 0.0] and not ref["g_D"].any()
    assert np.array_equal(ref["d_sig"], base["d_sig"], equal_nan=True)
    rows = depths[x["rays_a"][:, 0]]
    value, grad = _module_term(ngp, D, np.nan_to_num(rows.astype(np.float64)), 1.0, 1.0)
    assert not grad.any()
    np.testing.assert_allclose(ref["terms"][4], value, rtol=1e-12, atol=0)
    if kind == "none":
        assert ref["terms"][4] == 0.0
    else:
        z = float(np.float32(rows[0])) / 25
        np.testing.assert_allclose(ref["terms"][4], np.exp(-D[0]) * z * z / len(rows), rtol=1e-12)
    a, b = ngp.losses.compute_scale_and_shift(torch.tensor([0.7], dtype=torch.float64), torch.tensor([0.3], dtype=torch.float64))
    assert float(a) == 0.0 and float(b) == 0.0


def test_conditioning_of_the_seeded_depths():
    """var(D) / mean(D^2) >= 0.1 over the valid rays of every batch and prefix the GPU file compares tightly; over all rays
    the three batches read 0.158, 0.339, 0.348; a fit from float32 depths moves a by under 1e-7 relative"""
    want = {"crafted": 0.158, "300": 0.339, "1500": 0.348}
    for name in want:
        x = DR.make_crafted(0) if name == "crafted" else DR.make_random(int(name))
        D = DR.R.render(x)["depth"].detach().numpy()
        everything = DR.spread(D, np.ones(len(D), bool))
        assert everything == pytest.approx(want[name], abs=2e-3), (name, everything)
        depths = DR.make_depths(x, D_ref=D)
        assert depths.dtype == np.float32 and depths.shape == (x["n_rays"],)
        rows = depths[x["rays_a"][:, 0]]
        ok = rows / np.float32(25) > 0
        assert 0.05 < 1 - ok.mean() < 0.45 and ok[0] and ok[1] and not ok[[2, 3, 5]].any()
        assert rows[2] == 0 and rows[3] < 0 and np.isnan(rows[5])
        for p in (len(D),) + DR.PREFIXES:
            s = DR.spread(D[:p], ok[:p])
            print(f"FIG spread {name} rows={p}: {s:.3f}")
            assert s >= DR.MIN_SPREAD, (name, p, s)
        z = torch.from_numpy((rows / np.float32(25)).astype(np.float64))
        zz = torch.where(torch.from_numpy(ok), z, torch.zeros_like(z))
        a64, _ = DR.scale_and_shift(torch.from_numpy(D), zz, torch.from_numpy(ok))
        a32, _ = DR.scale_and_shift(torch.from_numpy(D.astype(np.float32).astype(np.float64)), zz, torch.from_numpy(ok))
        assert abs(float(a32) - float(a64)) < 1e-7 * abs(float(a64)), (name, float(a32), float(a64))


# ------------------------------------------------------------------------------------------- the scene's depths
def test_proxy_scene_depths(ngp):
    from ngp_amd.synthetic import SIGMA_IN, LegoProxy, analytic_part
    scene = LegoProxy(n_images=2, img_wh=(8, 8), device="cpu")
    o = torch.tensor([[0.3, 0.0, 1.5],               # straight down onto box1's top (z = 0.1)
                      [1.5, 1.5, 1.5],               # away from the scene
                      [0.45, 0.45, 1.5],             # through the unit box, past every solid
                      [1.5, 0.0, 0.0],               # along -x onto box1's +x face (x = 0.35)
                      [0.3, 0.02, 3.0]], dtype=torch.float32)
    d = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.1, 1.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -2.0]])
    got = scene.ground_truth_depths(o, d, n_quad=4096)
    assert got.shape == (5,) and got.dtype == torch.float32
    assert got[1] == 0 and got[2] == 0
    # a direct quadrature of sum w t on the same rays, in float64, from the camera to far behind the scene
    t = (torch.arange(200000, dtype=torch.float64) + 0.5) * (4.0 / 200000)
    for i in (0, 3, 4):
        oo, dd = o[i].double(), d[i].double()
        inside = analytic_part((oo + dd * t[:, None]).float()) >= 0
        alpha = torch.where(inside, 1 - torch.exp(-SIGMA_IN * (4.0 / 200000) * dd.norm()), torch.zeros_like(t))
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1 - alpha]), 0)[:-1]
        want = float((alpha * T * t).sum())
        assert float(got[i]) == pytest.approx(want, rel=2e-3), (i, float(got[i]), want)
    assert 1.39 < float(got[0]) < 1.45 and 1.14 < float(got[3]) < 1.2
    assert float(got[4]) == pytest.approx(0.5 * float(scene.ground_truth_depths(o[4:], d[4:] / 2, n_quad=4096)[0]), rel=1e-4)


def test_depth_maps_from_exporter_to_loader(ngp, tmp_path):
    """the tool's proxy writes depth/<p>_<name>.npy as 25 (0.37 D + 0.11), 0 where the pixel has no depth; the loader
    reads them with depth_mono=True into depths_2d, train items carry 'depth'"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd.datasets import dataset_dict, export
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=9, img_wh=(16, 16), device="cpu")
    D = export.render_scene_depths(scene, range(9), n_quad=256)
    assert D.shape == (9, 16, 16) and D.dtype == np.float32 and 0.02 < (D > 0).mean() < 0.9 and (D >= 0).all()
    root = td.make_proxy_with_depths(str(tmp_path / "tnt"), scene, n_quad=256)
    assert (td.PROXY_DEPTH_SCALE, td.PROXY_DEPTH_SHIFT) != (1, 0)
    stored = np.load(os.path.join(root, "depth", "1_00000008.npy"))
    assert stored.shape == (16, 16) and stored.dtype == np.float32
    want = np.where(D[8] > 0, 25.0 * (td.PROXY_DEPTH_SCALE * D[8] + td.PROXY_DEPTH_SHIFT), 0.0).astype(np.float32)
    assert np.array_equal(stored, want) and (stored == 0).any() and (stored > 0).any()
    test_set = dataset_dict["tnt"](root, "test", 1.0, depth_mono=True)
    assert tuple(test_set.depths_2d.shape) == (2, 256)
    train_set = dataset_dict["tnt"](root, "train", 1.0, depth_mono=True)
    train_set.batch_size = 64
    s = train_set[0]
    assert tuple(s["depth"].shape) == (64,)
    assert not hasattr(dataset_dict["tnt"](root, "train", 1.0), "depths_2d")


def test_depth_absrel(ngp):
    from ngp_amd.evaluation import depth_absrel, depth_summary
    g = torch.Generator().manual_seed(3)
    D = torch.rand(50, generator=g) + 0.5
    target = 25 * (0.37 * D + 0.11)
    target[::7] = 0.0
    target[3] = float("nan")
    target[4] = -2.0
    assert float(depth_absrel(D, target)) < 1e-6            # an exact affine map: the fit absorbs it
    assert float(depth_absrel(D.reshape(5, 10), target.reshape(5, 10))) < 1e-6
    assert torch.isnan(depth_absrel(D, torch.zeros(50)))
    assert torch.isnan(depth_absrel(D, torch.full((50,), float("nan"))))
    # by hand: D = (0, 1, 2), z = (1, 2, 4) -> a = 1.5, b = 5/6, residuals (-1/6, 1/3, -1/6)
    got = float(depth_absrel(torch.tensor([0.0, 1.0, 2.0, 9.0]), 25 * torch.tensor([1.0, 2.0, 4.0, 0.0])))
    assert got == pytest.approx((1 / 6 / 1 + 1 / 3 / 2 + 1 / 6 / 4) / 3, rel=1e-6)
    assert depth_summary({"depth_absrel": [0.1, float("nan"), 0.3]}) == pytest.approx(0.2)
    assert depth_summary({"depth_absrel": [float("nan")]}) is None


# ------------------------------------------------------------------------------------------- the tool's flag
def test_train_dataset_flag(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    assert td.parse_args(["--root_dir", "x"]).depth_mono is False
    a = td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--depth_mono", "--embed_a", "--random_bg"])
    assert a.depth_mono and a.scale == 0.5 and a.lambda_depth_mono is None and a.proxy_views == 108
    for bad in (["--make_proxy", "d", "--depth_mono"], ["--make_proxy", "d", "--depth_mono", "--dataset_name", "colmap"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--depth_mono", "--embed_msk"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--depth_mono", "--optimize_ext"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--depth_mono", "--render_semantic"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--depth_mono", "--normal_mono"]):
        with pytest.raises(SystemExit) as e:
            td.parse_args(bad)
        assert e.value.code == 2, bad

    class _Set:          # a dataset without depth maps is refused before anything else is looked at
        batch_size = 0
    with pytest.raises(ValueError, match="depth"):
        td.train(None, _Set(), 1, 1, 64, 1e-2, depth_mono=True)
    n, first, last = td.terms_summary([torch.tensor([9.0, 1, 1, 1, 4.0 - 0.1 * i]) for i in range(30)])
    assert n == 5 and first == pytest.approx(3.55) and last == pytest.approx(1.55)


# ------------------------------------------------------------------------------------------- the C entry
def test_c_entry_checks_its_arguments(ngp):
    """classes outside [0, 8], a negative ray count and a scene scale that is not positive are NGP_EINVAL, an empty batch
    is NGP_OK before any pointer is looked at (every pointer is NULL here: nothing may reach a launch)"""
    _lib = ngp._lib
    lib = _lib.load()
    _, args = _lib.PROTOS["ngp_render_loss_fused_dep"]
    names = [a for _, a in args]
    assert names[-3:] == ["dL_drgbs", "dep_ws", "stream"]
    assert names[names.index("rgb_bg") + 1:names.index("rgb_bg") + 5] == ["depth_gt", "lambda_dm", "scene_scale", "T_threshold"]
    _, plain = _lib.PROTOS["ngp_render_loss_fused"]
    assert [a for a in names if a not in ("depth_gt", "lambda_dm", "scene_scale", "dep_ws")] == [a for _, a in plain]

    def run(classes, n_rays, ld_sem=8, ld_normal=3, scale=1.0):
        vals = []
        for t, a in args:
            if t is C.c_void_p:
                vals.append(None)
            elif t is C.c_float:
                vals.append(scale if a == "scene_scale" else 1.0)
            else:
                vals.append({"classes": classes, "n_rays": n_rays, "ld_normal": ld_normal, "ld_sem": ld_sem}[a])
        return lib.ngp_render_loss_fused_dep(*vals)
    for n_rays in (0, 5):
        assert run(9, n_rays) == -22 and run(-1, n_rays) == -22 and run(7, n_rays, ld_normal=2) == -22
        assert run(7, n_rays, scale=0.0) == -22 and run(7, n_rays, scale=-1.0) == -22
        assert run(7, n_rays, scale=float("nan")) == -22
    assert run(0, 0) == 0 and run(8, 0) == 0 and run(7, 0) == 0
    assert run(7, -1) == -22 and run(7, 0, ld_sem=6) == -22
    assert run(7, 5) == -22            # NULL pointers with rays to process
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert "#define NGP_DEP_WS_INTS 18" in header


# ------------------------------------------------------------------------------------------- the trainer
def test_trainer_refuses_what_the_depth_tail_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer

    class _Head:
        n_output_dims = 7

    class _Model:          # what the checks look at
        rgb_act, use_skybox, differentiable_normals = "Sigmoid", False, False
        semantic_header = _Head()
    refused = [dict(msk_model=implicit_mask()), dict(pose_refiner=object()), dict(semantic=True), dict(normal_mono=True),
               dict(render_kwargs={"use_skybox": True}), dict(loss_kwargs={"normal_mono": True}),
               dict(loss_kwargs={"semantic": True}), dict(loss_kwargs={"depth_mono": True}),
               dict(loss_kwargs={"normal_ref": True}), dict(num_classes=9)]
    for kw in refused:
        model = _Model()
        with pytest.raises(ValueError):
            NGPTrainer(model, depth_mono=True, **kw)
        assert model.differentiable_normals is False
    for attr, value in (("rgb_act", "None"), ("use_skybox", True), ("differentiable_normals", True)):
        model = _Model()
        setattr(model, attr, value)
        with pytest.raises(ValueError, match="depth_mono=True"):
            NGPTrainer(model, depth_mono=True)


def test_step_checks_the_depths_argument(ngp):
    """step()'s checks of depths= come before anything touches the device: a missing, misshapen or integer depths=, a
    target= beside it, CPU tensors, and depths= handed to a trainer without the flag"""
    from ngp_amd.recipe import Recipe
    from ngp_amd.trainer import NGPTrainer

    class _Trainer:          # what step() looks at before its first launch
        model, recipe = None, Recipe(depth_mono=True)
    o, d, gt = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, 3)
    good = torch.ones(6)
    with pytest.raises(ValueError, match="needs depths="):
        NGPTrainer.step(_Trainer(), o, d, gt)
    for bad in (good[:5], good.reshape(6, 1), good.reshape(2, 3), good.to(torch.int64)):
        with pytest.raises(ValueError, match="depths= must be"):
            NGPTrainer.step(_Trainer(), o, d, gt, depths=bad)
    with pytest.raises(ValueError, match="no target="):
        NGPTrainer.step(_Trainer(), o, d, gt, depths=good, target={"depth": good})
    with pytest.raises(ValueError, match="no target="):
        NGPTrainer.step(_Trainer(), o, d, gt, depths=good, scale=2.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        NGPTrainer.step(_Trainer(), o, d, gt, depths=good)
    plain = _Trainer()
    plain.recipe = Recipe()
    with pytest.raises(ValueError, match="depths= is for"):
        NGPTrainer.step(plain, o, d, gt, depths=good)
