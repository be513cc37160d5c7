"""The skybox recipe (use_skybox) without a GPU: the float64 restatement of the sky network (sky_reference.py) against the
reference's recorded outputs (G6) and, for its backward, against torch autograd; the per-ray background of the fused tail's
restatement against autograd; the proxy scene's sky; the trainer's and the tools' refusals and the warm-up gate on
stand-ins; and the C interface's declarations and host-side answers."""
import os
import sys

import numpy as np
import pytest
import torch

import fused_tail_reference as R
import sky_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_matches_reference_golden(golden):
    """G6 holds the reference's own forward_skybox of 100 directions of normal length (not unit): the bar of
    test_gpu_parity.test_skybox_matches_reference_ngp_golden"""
    g = golden("g6_ngp_field.npz")
    assert g["sky_params"].shape == (S.N_PARAMS,) and g["sky_d"].shape == (100, 3)
    assert np.abs(np.linalg.norm(g["sky_d"], axis=1) - 1).max() > 0.5
    close(S.forward(g["sky_params"], g["sky_d"]), g["sky_rgb"], 2e-4, 1e-5)
    # the direction is normalised: its length does not matter
    close(S.forward(g["sky_params"], 3.0 * g["sky_d"].astype(np.float64)), S.forward(g["sky_params"], g["sky_d"]), 1e-12, 1e-14)


@pytest.mark.parametrize("which", ["g6", "dead"])
def test_backward_matches_autograd(golden, which):
    """the hand-stated backward against torch autograd of the same float64 forward; the structure the kernel's header
    states: equal padding columns, rows 3..15 of dW2 zero, a dead unit has no gradient"""
    params = golden("g6_ngp_field.npz")["sky_params"] if which == "g6" else S.dead_unit_params()[0]
    d = S.directions(300, seed=3)
    g = np.random.default_rng(5).standard_normal((300, 3))
    assert S.min_preact_margin(params, d) > 1e-9          # no pre-activation on the kink: the derivative is defined
    p = torch.from_numpy(np.asarray(params, np.float64)).requires_grad_(True)
    rgb, _ = S.forward_t(p, d)
    (rgb * torch.from_numpy(g)).sum().backward()
    got = S.backward(params, d, g)
    close(got, p.grad.numpy(), 1e-11, 1e-13)
    dW1, dW2 = got[:S.W2_AT].reshape(32, 16), got[S.W2_AT:].reshape(16, 32)
    assert np.abs(dW1[:, :9]).max() > 0 and np.abs(dW2[:3]).max() > 0
    assert (dW1[:, 9:] == dW1[:, 9:10]).all() and not dW2[3:].any()
    if which == "dead":
        dead = S.dead_unit_params()[1]
        assert len(dead) == 5 and not dW1[dead].any() and not dW2[:, dead].any()
        live = np.setdiff1d(np.arange(32), dead)
        assert np.abs(dW1[live]).max(1).min() > 0


def test_directions_cover_what_they_promise():
    d = S.directions(300)
    assert (np.count_nonzero(d[:6], axis=1) == 1).all() and (d[:3] > 0).any(1).all() and (d[3:6] < 0).any(1).all()
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert ln.min() < 1e-2 and ln.max() > 1e2
    assert S.directions(1).shape == (1, 3) and S.directions(0).shape == (0, 3)


# ------------------------------------------------------------------------------------------- the tail's restatement
@pytest.mark.parametrize("name", ["crafted", "40"])
def test_tail_reference_against_autograd(name):
    """d_bg of the restatement (g_rgb (1 - opacity), from what fused_tail_reference.finish returns) against autograd of
    the same loss with respect to the per-ray background; a ray without samples gets the whole seed; with every row of
    the background equal to the batch's colour the restatement is fused_tail_reference's own"""
    x = R.make_crafted(0) if name == "crafted" else R.make_random(int(name))
    bg = S.sky_batch(x)
    ref = S.evaluate(x, bg)
    st = R.render(x)
    rays = torch.from_numpy(x["rays_a"][:, 0].copy())
    b = torch.from_numpy(bg.astype(np.float64)).requires_grad_(True)
    O, C = st["opacity"].detach(), st["rgb_fg"].detach()
    rgb = C + b[rays] * (1 - O)[:, None]
    # (the opacity and distortion terms do not depend on the background)
    ((rgb - torch.from_numpy(x["gt"].astype(np.float64))[rays]) ** 2).mean().backward()
    close(ref["d_bg"], b.grad.numpy(), 1e-12, 1e-18)
    close(ref["rgb"][rays.numpy()], rgb.detach().numpy(), 1e-13, 0)
    empty = x["rays_a"][x["rays_a"][:, 2] == 0, 0]
    assert len(empty) >= 1
    close(ref["rgb"][empty], bg[empty], 0, 0)
    close(ref["d_bg"][empty], 2 * (bg[empty].astype(np.float64) - x["gt"][empty]) / (3 * len(rays)), 1e-12, 1e-18)
    assert np.abs(ref["d_bg"]).max() > 0
    one = np.broadcast_to(x["bg"], bg.shape)
    plain, same = R.evaluate(x), S.evaluate(x, one)
    for k in ("rgb", "opacity", "d_sig", "d_rgb", "terms"):
        close(same[k], plain[k], 0, 0)
    # the column sums of d_bg are the constant background's gradient
    b1 = torch.from_numpy(x["bg"].astype(np.float64)).requires_grad_(True)
    ((C + b1 * (1 - O)[:, None] - torch.from_numpy(x["gt"].astype(np.float64))[rays]) ** 2).mean().backward()
    close(same["d_bg"].sum(0), b1.grad.numpy(), 1e-11, 1e-18)


def test_fused_tail_sky_selects_the_default_layout(ngp):
    from ngp_amd.rendering import TAIL_LAYOUT, FusedTail
    gt = torch.zeros(4, 3)
    t = FusedTail(gt, 1.0, 2.0, sky=True)
    assert t.entry == "default" and t.sky and t.symbol == "render_loss_fused_sky" and TAIL_LAYOUT[t.entry].n_terms == 4
    plain = FusedTail(gt, 1.0, 2.0)
    assert plain.entry == "default" and not plain.sky and plain.symbol == "render_loss_fused"
    assert FusedTail(gt, 0, 0, mask=gt, size_delta=0.5).symbol == "render_loss_fused_masked"
    assert FusedTail(gt, 0, 0, terms={"depth_mono": ()}, packed=True).symbol == "render_loss_fused_dep"
    assert FusedTail(gt, 0, 0, terms={"depth_mono": ()}).symbol == "render_loss_fused_multi"
    assert "sky" not in TAIL_LAYOUT
    for bad in (dict(mask=gt), dict(terms={"semantic": ()}), dict(terms={"depth_mono": ()}, packed=True)):
        with pytest.raises(ValueError, match="skybox"):
            FusedTail(gt, 0, 0, sky=True, **bad)


def test_fused_tail_ok_takes_a_skybox_only_from_a_sky_tail(ngp):
    from ngp_amd.rendering import FusedTail, _fused_tail_ok

    class _M:
        rgb_act, use_skybox, differentiable_normals = "Sigmoid", True, False

        def _field(self):
            pass
    gt = torch.zeros(4, 3)
    kw = {"use_skybox": True}
    assert not _fused_tail_ok(_M(), kw, 0.0, 7) and not _fused_tail_ok(_M(), kw, 0.0, 7, FusedTail(gt, 0, 0))
    assert _fused_tail_ok(_M(), kw, 0.0, 7, FusedTail(gt, 0, 0, sky=True))
    assert _fused_tail_ok(_M(), {}, 0.0, 7, FusedTail(gt, 0, 0))
    plain = _M()
    plain.use_skybox = False          # a model without the network: the kwarg cannot be served
    assert not _fused_tail_ok(plain, kw, 0.0, 7, FusedTail(gt, 0, 0, sky=True))
    tone = _M()
    tone.rgb_act = "None"
    assert not _fused_tail_ok(tone, kw, 0.0, 7, FusedTail(gt, 0, 0, sky=True))


# ------------------------------------------------------------------------------------------- the proxy scene
def test_analytic_sky(ngp):
    from ngp_amd.synthetic import LegoProxy, analytic_sky
    g = torch.Generator().manual_seed(3)
    d = torch.randn(4000, 3, generator=g)
    c = analytic_sky(d)
    assert c.shape == (4000, 3) and float(c.min()) >= 0.1 - 1e-6 and float(c.max()) <= 0.95 + 1e-6
    assert torch.allclose(analytic_sky(7.5 * d), c, atol=1e-6)          # a function of the direction alone
    # it does depend on the direction, in every channel, and smoothly: a 1e-3 turn moves it by O(1e-3)
    assert float(c.std(0).min()) > 0.03
    u = torch.nn.functional.normalize(d, dim=-1)
    near = analytic_sky(u + 1e-3 * torch.randn(4000, 3, generator=g))
    assert float((near - c).abs().max()) < 5e-3
    up, down = analytic_sky(torch.tensor([[0.0, 0.0, 1.0]])), analytic_sky(torch.tensor([[0.0, 0.0, -1.0]]))
    assert float(up[0, 2]) > float(down[0, 2]) + 0.2          # bluer at the zenith
    # ground_truth(sky=True) composites over it: a ray that misses the scene is the sky, opacity 0
    scene = LegoProxy(n_images=2, img_wh=(8, 8), device="cpu")
    o = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0]])
    dd = torch.tensor([[0.3, 0.2, 1.0], [0.01, 0.02, -1.0]])
    rgb, op = scene.ground_truth(o, dd, n_quad=64, sky=True)
    black, op0 = scene.ground_truth(o, dd, n_quad=64)
    assert float(op[0]) == 0.0 and torch.equal(op, op0) and torch.allclose(rgb[0], analytic_sky(dd[:1])[0])
    assert torch.allclose(rgb, black + analytic_sky(dd) * (1 - op)[:, None])


# ------------------------------------------------------------------------------------------- the trainer
class _Head:
    n_output_dims = 7


class _Model:          # what the construction checks look at
    rgb_act, use_skybox, differentiable_normals = "Sigmoid", True, False
    semantic_header = _Head()


def test_trainer_refuses_what_use_skybox_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    plain = _Model()
    plain.use_skybox = False
    with pytest.raises(ValueError, match="needs a model built with use_skybox=True"):
        NGPTrainer(plain, use_skybox=True)
    head = "use_skybox=True runs on the fused render \\+ loss tail, which does not take "
    tone, dn = _Model(), _Model()
    tone.rgb_act, dn.differentiable_normals = "None", True
    for model, kw, what in ((_Model(), dict(msk_model=implicit_mask()), "a msk_model"),
                            (_Model(), dict(pose_refiner=object()), "a pose_refiner"),
                            (tone, {}, "rgb_act != 'Sigmoid'"), (dn, {}, "differentiable normals"),
                            (_Model(), dict(loss_kwargs={"normal_mono": True}), "an optional term in loss_kwargs"),
                            (_Model(), dict(loss_kwargs={"normal_ref": True}), "an optional term in loss_kwargs"),
                            (_Model(), dict(render_kwargs={"use_skybox": True}), "render_kwargs\\['use_skybox'\\]")):
        with pytest.raises(ValueError, match=head + ".*" + what):
            NGPTrainer(model, use_skybox=True, **kw)
    # the options that were there before refuse a model with a skybox through their own messages, as they did
    for kw in (dict(semantic=True), dict(normal_mono=True), dict(depth_mono=True), dict(multi_terms=("depth_mono",))):
        with pytest.raises(ValueError, match="a skybox"):
            NGPTrainer(_Model(), use_skybox=True, **kw)
    with pytest.raises(ValueError, match="rgb_act='None'|a skybox"):
        NGPTrainer(_Model(), use_skybox=True, use_exposure=True)
    with pytest.raises(ValueError, match="use_exposure=True does not combine with a skybox"):
        NGPTrainer(tone, use_skybox=True, use_exposure=True)


def test_warmup_gate_and_step_checks(ngp):
    """the skybox joins at global_step >= warmup_steps (train.py:160); step()'s checks come before anything touches the
    device"""
    from ngp_amd.recipe import Recipe
    from ngp_amd.trainer import NGPTrainer

    class _Sky:          # what step() looks at before its first launch
        model = None
        warmup_steps, global_step = 256, 0

        def __init__(self):
            self.recipe = Recipe(use_skybox=True)

    class _Old:          # the default recipe
        recipe = Recipe()
        warmup_steps, global_step = 256, 1000
    tr = _Sky()
    for step, on in ((0, False), (255, False), (256, True), (257, True), (10 ** 6, True)):
        tr.global_step = step
        assert NGPTrainer.sky_active(tr) is on, step
    tr.recipe.use_skybox = False
    assert NGPTrainer.sky_active(tr) is False and NGPTrainer.sky_active(_Old()) is False
    o, d, gt = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, 3)
    for step in (0, 300):
        tr = _Sky()
        tr.global_step = step
        with pytest.raises(ValueError, match="use_skybox=True: the step stays on the fused render \\+ loss tail"):
            NGPTrainer.step(tr, o, d, gt, target={"normal": gt})
        with pytest.raises(ValueError, match="use_skybox=True: the step stays on the fused render \\+ loss tail"):
            NGPTrainer.step(tr, o, d, gt, normal_mono=True)
        with pytest.raises(RuntimeError, match="use_skybox=True needs CUDA tensors"):
            NGPTrainer.step(tr, o, d, gt)


def test_model_side(ngp):
    model = ngp.networks.NGP(scale=0.5, use_skybox=True)
    assert model._stock_skybox() and model.skybox_rgb_net.params.numel() == S.N_PARAMS
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model.skybox_rgb(torch.ones(4, 3))
    plain = ngp.networks.NGP(scale=0.5)
    assert not plain._stock_skybox() and plain.forward_skybox(torch.ones(2, 3)) is None
    with pytest.raises(RuntimeError, match="skybox_rgb needs the skybox"):
        plain.skybox_rgb(torch.ones(4, 3))
    assert not ngp.networks.NGP(scale=0.5, use_skybox=True, rgb_act="None")._stock_skybox()          # Sigmoid only


# ------------------------------------------------------------------------------------------- the tools' flags
def test_tool_flags(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render
    import render_panorama
    import train_dataset as td
    a = td.parse_args(["--make_proxy", "x", "--dataset_name", "tnt", "--use_skybox"])
    assert a.use_skybox and a.scale == 0.5
    assert not td.parse_args(["--root_dir", "x"]).use_skybox
    for bad in (["--embed_msk"], ["--optimize_ext"], ["--render_semantic"], ["--normal_mono"], ["--depth_mono"],
                ["--multi_terms", "depth_mono"], ["--use_exposure"]):
        with pytest.raises(SystemExit) as ex:
            td.parse_args(["--root_dir", "x", "--use_skybox"] + bad)
        assert ex.value.code == 2
    for name in ("nerf", "colmap"):
        with pytest.raises(SystemExit) as ex:
            td.parse_args(["--make_proxy", "x", "--dataset_name", name, "--use_skybox"])
        assert ex.value.code == 2
    td.parse_args(["--root_dir", "x", "--use_skybox", "--embed_a", "--random_bg"])
    base = ["--ckpt", "c", "--root_dir", "x", "--out_dir", "o", "--render_rgb"]
    assert render.parse_args(base + ["--use_skybox"]).use_skybox and not render.parse_args(base).use_skybox
    with pytest.raises(SystemExit) as ex:
        render.parse_args(base + ["--use_skybox", "--use_exposure"])
    assert ex.value.code == 2
    pano = ["--ckpt", "c", "--out_dir", "o", "--pano_hw", "4", "8", "--v_forward", "1", "0", "0", "--v_down", "0", "0", "-1",
            "--v_right", "0", "1", "0"]
    assert render_panorama.parse_args(pano + ["--use_skybox"]).use_skybox and not render_panorama.parse_args(pano).use_skybox
    assert "--use_skybox" in open(os.path.join(ROOT, "tools", "extract_mesh.py")).read()


def test_sky_psnr_pools_the_sky_pixels(ngp, tmp_path):
    """tools/train_dataset.py's test_sky_psnr: the opacity maps are found by image stem, and the error is pooled over the
    pixels below the opacity threshold alone"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td

    class _Set:
        img_wh = (2, 2)
        rays = torch.tensor([[[0.5, 0.5, 0.5]] * 4, [[0.2, 0.2, 0.2]] * 4])
        imgs = [str(tmp_path / "images" / "1_00000000.png"), str(tmp_path / "images" / "1_00000008.png")]
    assert td.opacity_maps(_Set(), str(tmp_path)) is None
    os.makedirs(tmp_path / "opacity")
    np.save(tmp_path / "opacity" / "1_00000000.npy", np.array([[0.0, 0.5], [1.0, 0.009]], np.float32))
    np.save(tmp_path / "opacity" / "1_00000008.npy", np.array([[1.0, 1.0], [0.02, 0.0]], np.float32))
    op = td.opacity_maps(_Set(), str(tmp_path))
    assert op.shape == (2, 4)
    seen = []
    acc = td.SkyPsnr(_Set(), op, then=lambda i, rgb, res: seen.append(i))
    assert acc.value() == (None, 0)
    acc(0, torch.tensor([[0.6, 0.5, 0.5], [9.0] * 3, [9.0] * 3, [0.5, 0.5, 0.3]]), None)
    acc(1, torch.tensor([[9.0] * 3, [9.0] * 3, [9.0] * 3, [0.2, 0.2, 0.2]]), None)
    value, n = acc.value()
    assert n == 3 and seen == [0, 1]
    assert abs(value + 10 * np.log10((0.01 + 0.04) / 9)) < 1e-4


# ------------------------------------------------------------------------------------------- the C interface
def test_entries_are_declared_and_built(ngp):
    from ngp_amd import _lib, build
    assert "sky_kernels.hip" in [s for s, _ in build.SOURCES]
    fwd, bwd, ws = (_lib.PROTOS[f"ngp_skybox_{k}"] for k in ("fwd", "bwd", "bwd_workspace"))
    assert [n for _, n in fwd[1]] == ["params", "rays_d", "n_rays", "rgb_bg", "stream"]
    assert [n for _, n in bwd[1]] == ["params", "rays_d", "dL_drgb_bg", "n_rays", "dparams", "workspace", "stream"]
    assert [n for _, n in ws[1]] == ["n"]
    # one row of 416 partial sums (doubles, counted in floats) per workgroup, a workgroup per tile of 256 rays up to
    # NGP_SKYBOX_BWD_MAX_BLOCKS
    assert [_lib.call_host("skybox_bwd_workspace", n) for n in (0, 1, 256, 257, 256 * 256, 10 ** 12, -1)] == \
        [0, 832, 832, 1664, 256 * 832, 256 * 832, -22]
    assert "#define NGP_SKYBOX_BWD_MAX_BLOCKS 256" in open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    src = open(os.path.join(ROOT, "instant-ngp-pp_amd", "csrc", "sky_kernels.hip")).read()
    assert "atomicAdd" not in src and "printf" not in src and "asm" not in src
    # the sky tail: ngp_render_loss_fused's arguments, and d_rgb_bg behind dL_drgbs
    plain, sky = ([n for _, n in _lib.PROTOS[k][1]] for k in ("ngp_render_loss_fused", "ngp_render_loss_fused_sky"))
    assert sky == plain[:-1] + ["dL_drgb_bg", "stream"] and plain[-2] == "dL_drgbs"


def test_empty_and_negative_batches(ngp):
    """n == 0 is NGP_OK before any pointer is looked at, n < 0 is NGP_EINVAL, a missing pointer is NGP_EINVAL: none of
    them reaches a launch"""
    lib = ngp._lib.load()
    assert lib.ngp_skybox_fwd(None, None, 0, None, None) == 0 and lib.ngp_skybox_fwd(None, None, -1, None, None) == -22
    assert lib.ngp_skybox_bwd(None, None, None, 0, None, None, None) == 0
    assert lib.ngp_skybox_bwd(None, None, None, -3, None, None, None) == -22
    assert lib.ngp_skybox_fwd(None, None, 5, None, None) == -22
    assert lib.ngp_skybox_bwd(None, None, None, 5, None, None, None) == -22
    n_args = len(ngp._lib.PROTOS["ngp_render_loss_fused_sky"][1])

    def tail(n_rays, classes=7):
        args = [None] * n_args
        names = [n for _, n in ngp._lib.PROTOS["ngp_render_loss_fused_sky"][1]]
        for k, v in (("ld_normal", 3), ("ld_sem", 8), ("T_threshold", 1e-4), ("classes", classes), ("n_rays", n_rays),
                     ("lambda_opacity", 1e-3), ("lambda_distortion", 1e-3)):
            args[names.index(k)] = v
        return lib.ngp_render_loss_fused_sky(*args)
    assert tail(0) == 0 and tail(-1) == -22 and tail(4) == -22 and tail(0, classes=9) == -22
