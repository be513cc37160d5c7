"""The HDR-NeRF recipe (use_exposure) on the GPU: ngp_tonemap_fwd / ngp_tonemap_bwd against the float64 restatement
(tonemap_reference.py) at the edges of their launch shapes, with the launch-per-operation route (the three tonemapper_net_i
modules composed as NGP.log_radiance_to_rgb composed them before) measured on the same inputs as the yardstick of the
tolerance; G13 through the public methods; one trainer step against the same step composed by hand; the recipe end to end
through tools/train_dataset.py against an exposure-blind run on the same images."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import tonemap_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE, MAX_BLOCKS = 256, 512                 # samples per tile, NGP_TONEMAP_BWD_MAX_BLOCKS
# 300 001 samples = 1172 tiles on 512 workgroups: every workgroup walks more than one tile, the last tile is ragged;
# 256, 257 and 513 samples are 1, 2 and 3 workgroups: the ordered sum's single row, its pair and its odd tail
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 300001)
TIMES = (0.125, 0.5, 2.0, 8.0, 32.0)        # the exposure table of the synthetic scenes
EPS = 2.0 ** -23


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def layered_tonemap(self, log_radiances, **kwargs):
    """NGP.log_radiance_to_rgb as it was composed before the fused kernels: module by module"""
    out = []
    for i in range(3):
        inp = log_radiances[:, i:i + 1]
        if 'exposure' in kwargs:
            inp = inp + torch.log(kwargs['exposure'])
        out.append(getattr(self, f'tonemapper_net_{i}')(inp))
    return torch.cat(out, 1)


@pytest.fixture(scope="module")
def g13(golden):
    g = golden("g13_tonemapper.npz")
    return [g[f"tonemapper_net_{i}.params"].copy() for i in range(3)]


@pytest.fixture(scope="module")
def hdr_model(ngp, g13):
    """NGP(rgb_act='None') with the G13 tone-mappers (the tables are not looked at)"""
    model = ngp.networks.NGP(scale=0.5, rgb_act='None').to(DEV)
    load_tonemappers(model, g13)
    return model


def load_tonemappers(model, params3):
    with torch.no_grad():
        for i in range(3):
            getattr(model, f"tonemapper_net_{i}").params.copy_(T(np.asarray(params3[i], np.float32)))


def inputs(n, mode, seed):
    g = np.random.default_rng(seed)
    lr = g.uniform(-6, 6, (n, 3)).astype(np.float32)
    dy = g.normal(size=(n, 3)).astype(np.float32)
    e = {"none": None, "broadcast": np.full((1, 1), 8.0, np.float32),
         "per_sample": g.choice(TIMES, (n, 1)).astype(np.float32)}[mode]
    return lr, e, dy


def run_route(model, fused, lr, e, dy):
    """-> rgb, d_log_radiance, dparams (3, 2048) of sum(rgb * dy) through one route of the tone-mapper"""
    tones = [getattr(model, f"tonemapper_net_{i}").params for i in range(3)]
    for p in tones:
        p.grad = None
    x = T(lr).requires_grad_(True)
    kw = {} if e is None else {"exposure": T(e)}
    rgb = model.log_radiance_to_rgb(x, **kw) if fused else layered_tonemap(model, x, **kw)
    rgb.backward(T(dy))
    return N(rgb), N(x.grad), np.stack([N(p.grad) for p in tones])


def errors(got, ref):
    """a route against the restatement -> (rgb: largest absolute error (colours lie in [0, 1]); d_log_radiance: largest error
    relative to the batch's largest entry; the absolute error of every parameter sum, (3, 2048))"""
    rgb, dlr, dp = got
    r_rgb, r_dlr, r_dp, scale = ref
    s_dlr = max(np.abs(r_dlr).max(), 1e-30)
    assert not dp[scale == 0].any()                 # a sum without a contribution is exactly 0
    return np.abs(rgb - r_rgb).max(), np.abs(dlr - r_dlr).max() / s_dlr, np.abs(dp - r_dp)


def check_against_layered(tag, model, params3, lr, e, dy):
    """both routes on the same inputs against float64; prints the figures and holds the fused kernels to the bar: rgb and
    d_log_radiance by their one figure, the parameter sums ONE BY ONE, err_fused[k] <= 4 err_layered[k] + 2^-23 scale[k] (a
    single worst ratio over the 6144 sums would be set by whichever sum the old route gets wrong most: a sum that only
    saturated samples feed is 100 % off there, and a bar of 4 x that holds nothing)"""
    got = run_route(model, True, lr, e, dy)
    ref = R.forward(params3, lr, e), *R.backward(params3, lr, e, dy)
    scale = ref[3]
    new, old = errors(got, ref), errors(run_route(model, False, lr, e, dy), ref)
    live = scale > 0
    ratio = lambda err: (err[live] / scale[live])
    worst = np.argmax(ratio(new[2]) - 4 * ratio(old[2]))
    print(f"tonemap {tag}: layered route rgb {old[0]:.3e} dlr {old[1]:.3e} dparams/scale median {np.median(ratio(old[2])):.3e} "
          f"max {ratio(old[2]).max():.3e} | fused kernels rgb {new[0]:.3e} dlr {new[1]:.3e} dparams/scale median "
          f"{np.median(ratio(new[2])):.3e} max {ratio(new[2]).max():.3e}; nearest the bar: fused {ratio(new[2])[worst]:.3e} "
          f"layered {ratio(old[2])[worst]:.3e}")
    for name, a, b in zip(("rgb", "d_log_radiance"), new[:2], old[:2]):
        assert a <= 4 * b + EPS, (name, a, b)
    over = new[2] > 4 * old[2] + EPS * scale
    assert not over.any(), (int(over.sum()), np.argwhere(over)[:5], new[2][over][:5], old[2][over][:5], scale[over][:5])
    return got, ref


@pytest.mark.parametrize("mode", ["none", "broadcast", "per_sample"])
@pytest.mark.parametrize("n", COUNTS)
def test_kernels_against_float64(ngp, hdr_model, g13, n, mode):
    """forward and backward of both routes on the same inputs against float64.  No tolerance is fixed: the fused kernels
    pass with an error of at most 4 e_ref + 2^-23 (in units of each figure's scale, see check_against_layered), e_ref the
    error of the launch-per-operation route; 4 allows for another summation order over 64 terms and __expf, the floor keeps
    a case where the old route happens to be exact from failing the new one."""
    lr, e, dy = inputs(max(n, 1), mode, 100 + n)
    lr, dy = lr[:n], dy[:n]
    if mode == "per_sample":
        e = e[:n]
    if n == 0:
        got = run_route(hdr_model, True, lr, e, dy)
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and not got[2].any()
        return
    got, _ = check_against_layered(f"n={n} exposure={mode}", hdr_model, g13, lr, e, dy)
    assert got[0].shape == (n, 3) and got[1].shape == (n, 3)


@pytest.mark.parametrize("n", [257, 300001])
def test_sums_that_do_not_cancel(ngp, hdr_model, g13, n):
    """dL_drgb of one sign: every contribution to a W2 sum has that sign, so the sum IS its absolute-contribution scale and a
    lost tile, a ragged tail counted twice or sums reset between a workgroup's tiles show at full size.  Same bar, sum by
    sum; and, whatever the old route does, every W2 sum within 1e-6 of the float64 one (the sums are carried in double and
    rounded once: 2^-24, with room for the float32 inputs' own conversion)"""
    lr, e, dy = inputs(n, "per_sample", 500 + n)
    got, ref = check_against_layered(f"n={n} exposure=per_sample dL_drgb=|N(0,1)|", hdr_model, g13, lr, e, np.abs(dy))
    w2 = slice(R.H * R.IN, R.H * R.IN + R.H)
    r_dp, scale = ref[2][:, w2], ref[3][:, w2]
    np.testing.assert_allclose(r_dp, scale, rtol=1e-12, atol=0)
    # (a unit that no sample of the batch switches on has scale 0 and must come out exactly 0)
    assert (scale > 0).sum() > 96 and (np.abs(got[2][:, w2] - r_dp) <= 1e-6 * scale).all()


def test_backward_is_the_same_on_every_run(ngp, hdr_model):
    """partials in a fixed order, no atomics: two launches give the same bits"""
    lr, e, dy = inputs(70001, "per_sample", 7)
    a, b = run_route(hdr_model, True, lr, e, dy), run_route(hdr_model, True, lr, e, dy)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _raw_bwd(params3, lr, e, stride, dy, sinks, want_dx=True):
    from ngp_amd._lib import call, call_host
    n = lr.shape[0]
    ws = torch.empty(max(int(call_host("tonemap_bwd_workspace", n)), 1), device=DEV)
    dx = torch.full((n, 3), 7.0, device=DEV) if want_dx else None
    call("tonemap_bwd", *params3, lr, e, stride, dy, n, dx, *sinks, ws)
    return dx


def test_dead_saturated_and_kink_batches(ngp, g13):
    from ngp_amd._lib import call
    # every hidden unit dead: positive W1[:, 0], padding columns that cannot lift u = -40 above 0
    dead = [np.abs(a).astype(np.float32) for a in g13]
    for a in dead:
        a[:R.H * R.IN].reshape(R.H, R.IN)[:, 1:] = -0.01
    n = 300
    params = [T(a) for a in dead]
    sinks = [torch.zeros(2048, device=DEV) for _ in range(3)]
    dx = _raw_bwd(params, torch.full((n, 3), -40.0, device=DEV), None, 0, torch.ones(n, 3, device=DEV), sinks)
    assert not dx.any() and not any(s.any() for s in sinks)
    # saturated: every weight positive, u = +40: y rounds to 1, the input gradient is 0 or subnormal, nothing is NaN
    sat = [T(np.abs(a).astype(np.float32)) for a in g13]
    lr = torch.full((n, 3), 40.0, device=DEV)
    rgb = torch.empty(n, 3, device=DEV)
    call("tonemap_fwd", *sat, lr, None, 0, n, rgb)
    assert (R.forward([np.abs(a) for a in g13], np.full((1, 3), 40.0)) == 1.0).all() and (rgb == 1.0).all()
    sinks = [torch.zeros(2048, device=DEV) for _ in range(3)]
    dx = _raw_bwd(sat, lr, None, 0, torch.ones(n, 3, device=DEV), sinks)
    tiny = float(np.finfo(np.float32).tiny)
    assert torch.isfinite(dx).all() and float(dx.abs().max()) < tiny
    assert all(torch.isfinite(s).all() and float(s.abs().max()) < tiny * n * 64 for s in sinks)
    # a pre-activation of exactly 0 (row 0 of channel 0's W1 is zero, whatever the input): its derivative is 0; the other
    # units of the sample are alive (their accuracy is test_kernels_against_float64's business)
    kink = [a.astype(np.float32).copy() for a in g13]
    kink[0][:R.IN] = 0.0
    lr_np, dy_np = np.full((1, 3), 0.75, np.float32), np.ones((1, 3), np.float32)
    sinks = [torch.zeros(2048, device=DEV) for _ in range(3)]
    dx = _raw_bwd([T(a) for a in kink], T(lr_np), None, 0, T(dy_np), sinks)
    _, r_dp, scale = R.backward(kink, lr_np, None, dy_np)
    assert not scale[0][:R.IN].any() and scale[0][R.H * R.IN] == 0.0 and scale[0][R.IN:R.H * R.IN].any()
    assert not sinks[0][:R.IN].any() and float(sinks[0][R.H * R.IN]) == 0.0
    got = np.stack([N(s) for s in sinks])
    assert np.isfinite(N(dx)).all() and not got[scale == 0].any() and got[scale > 0].all()


def test_backward_adds_into_its_sinks(ngp, g13):
    """dparams pre-filled with a pattern: the kernel adds its sums to it.  The sums are formed in a fixed order before they
    meet the sink, so the result is float32(pattern + the sums written into zeroed sinks), bit for bit; rows 1..15 of W2
    keep their bits; n = 0 touches nothing"""
    lr, e, dy = inputs(1000, "per_sample", 9)
    params = [T(a) for a in g13]
    pattern = (np.arange(2048) % 17 - 8).astype(np.float32) * 0.37
    zeroed = [torch.zeros(2048, device=DEV) for _ in range(3)]
    _raw_bwd(params, T(lr), T(e), 1, T(dy), zeroed)
    sinks = [T(pattern.copy()) for _ in range(3)]
    _raw_bwd(params, T(lr), T(e), 1, T(dy), sinks)
    for c in range(3):
        got, alone = N(sinks[c]), N(zeroed[c])
        assert np.array_equal(got[R.H * R.IN + R.H:].view(np.uint32), pattern[R.H * R.IN + R.H:].view(np.uint32))
        assert not alone[R.H * R.IN + R.H:].any() and alone[:R.H * R.IN + R.H].any()
        assert np.array_equal(got, pattern + alone)
    before = [s.clone() for s in sinks]
    _raw_bwd(params, T(lr[:0]), None, 0, T(dy[:0]), sinks)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, sinks))
    # the input gradient is optional
    again = [T(pattern.copy()) for _ in range(3)]
    assert _raw_bwd(params, T(lr), T(e), 1, T(dy), again, want_dx=False) is None
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, sinks))


def test_entries_refuse_bad_arguments(ngp, g13):
    from ngp_amd._lib import call, call_host
    params = [T(a) for a in g13]
    x, y, ws = torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV), torch.empty(1152, device=DEV)
    sinks = [torch.zeros(2048, device=DEV) for _ in range(3)]
    for n, stride in ((-1, 0), (4, 2), (4, -1)):
        with pytest.raises(RuntimeError, match="code -22"):
            call("tonemap_fwd", *params, x, None, stride, n, y)
        with pytest.raises(RuntimeError, match="code -22"):
            call("tonemap_bwd", *params, x, None, stride, y, n, None, *sinks, ws)
    assert not any(s.any() for s in sinks)
    assert [call_host("tonemap_bwd_workspace", n) for n in (0, 1, 256, 257, 512 * 256, 10 ** 12, -1)] == \
        [0, 1152, 1152, 2304, 512 * 1152, 512 * 1152, -22]      # (576 doubles a workgroup, counted in floats)


def test_model_checks_its_exposure(ngp, hdr_model):
    x = torch.zeros(5, 3, device=DEV)
    with pytest.raises(ValueError, match="takes no gradient"):
        hdr_model.log_radiance_to_rgb(x, exposure=torch.ones(5, 1, device=DEV, requires_grad=True))
    with pytest.raises(ValueError, match="one value or one per sample"):
        hdr_model.log_radiance_to_rgb(x, exposure=torch.ones(4, 1, device=DEV))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        hdr_model.log_radiance_to_rgb(x, exposure=torch.ones(5, 1))
    a = hdr_model.log_radiance_to_rgb(x, exposure=torch.tensor(2.0, device=DEV))
    assert torch.equal(a, hdr_model.log_radiance_to_rgb(x, exposure=torch.full((1, 1), 2.0, device=DEV)))
    assert torch.equal(a, hdr_model.log_radiance_to_rgb(x, exposure=torch.full((5, 1), 2.0, device=DEV)))


def test_g13_through_the_public_methods(ngp, golden):
    """forward and forward_test of NGP(rgb_act='None') with the golden parameters, with and without the recorded exposure, at
    the tolerances of test_gpu_parity.test_tonemapper_and_exposure_match_reference_golden: the rerouting changed nothing"""
    from helpers import table_rule
    g = golden("g13_tonemapper.npz")
    model = ngp.networks.NGP(scale=0.5, rgb_act='None').to(DEV)
    with torch.no_grad():
        named = dict(model.named_parameters())
        named["xyz_encoder.params"].copy_(T(table_rule(named["xyz_encoder.params"].numel())))
        named["rgb_encoder.params"].copy_(T(table_rule(named["rgb_encoder.params"].numel())))
        for k in g.files:
            if k in named:
                named[k].copy_(T(g[k]))
        x, d = T(g["x"]), T(g["d"])
        for tag, kw in (("ldr", {}), ("ldr_exposure", {"exposure": T(g["exposure"])})):
            close(N(model(x, d, **kw)[1]), g[f"fwd_{tag}_rgbs"], 5e-4, 1e-5)
            close(N(model.forward_test(x, d, **kw)[1]), g[f"test_{tag}_rgbs"], 5e-4, 1e-5)
        unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=DEV), exposure=torch.ones(1, 1, device=DEV))
        close(N(unit), g["unit_exposure_rgb"], 1e-5, 1e-6)


# ------------------------------------------------------------------------------------------- one trainer step
def _field_model(ngp, seed):
    torch.manual_seed(seed)
    model = ngp.networks.NGP(scale=0.5, rgb_act='None').to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.0)      # a random field dense enough to be seen
    return model


def test_trainer_step_against_the_step_composed_by_hand(ngp):
    """64 rays, two models with the same parameters.  One takes NGPTrainer(use_exposure=True).step(exposure=e) with the
    optimizer stubbed out; the other the same step from the pieces that were there before: render(exposure=e) with the
    tone-mapper module by module, NeRFLoss's default terms plus the unit-exposure term, loss.backward().  Loss and the five
    terms to 1e-6 relative, every gradient within 3e-4 of the hand-made step's largest entry of that tensor (the bars of
    test_embed_a_gpu.test_field_route_against_the_tensor_route)."""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import render
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    UNIT = 0.73
    a, b = _field_model(ngp, 71), _field_model(ngp, 71)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    scene = LegoProxy(n_images=4, img_wh=(32, 32), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(72)
    img, pix = scene.sample_batch(64, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(64, 3, device=DEV, generator=gen)
    e = torch.tensor(TIMES, device=DEV)[torch.randint(5, (64,), device=DEV, generator=gen)]
    thr = 0.01 * 1024 / 3 ** 0.5
    # --- the trainer's step
    tr = NGPTrainer(a, lr=1e-2, use_exposure=True, unit_exposure_rgb=UNIT)
    assert all(f"tone_{i}" in a.link.grad_sinks for i in range(3))
    tr.optimizer_step = lambda: None
    torch.manual_seed(73)
    loss_a, res_a = tr.step(o, d, gt, exposure=e)
    terms_a = N(res_a["loss_terms"])
    assert terms_a.shape == (5,) and float(loss_a) == terms_a[0] and int(res_a["total_samples"]) > 0
    # --- the same step by hand
    b.log_radiance_to_rgb = types.MethodType(layered_tonemap, b)
    torch.manual_seed(73)
    b.update_density_grid(thr, warmup=True)
    res_b = render(b, o, d, exp_step_factor=0.0, num_classes=7, exposure=e.reshape(-1, 1))
    loss_d = NeRFLoss()(res_b, {"rgb": gt})
    assert sorted(loss_d) == ["distortion", "opacity", "rgb"]
    unit = b.log_radiance_to_rgb(torch.zeros(1, 3, device=DEV), exposure=torch.ones(1, 1, device=DEV))
    loss_d["unit_exposure"] = 0.5 * (unit - UNIT) ** 2
    loss_b = sum(v.mean() for v in loss_d.values())
    loss_b.backward()
    terms_b = np.array([float(loss_b.detach())] + [float(loss_d[k].detach().mean())
                                                   for k in ("rgb", "opacity", "distortion", "unit_exposure")])
    assert int(res_a["total_samples"]) == int(res_b["total_samples"])
    print("loss terms, trainer", terms_a, "by hand", terms_b)
    np.testing.assert_allclose(terms_a, terms_b, rtol=1e-6, atol=0)
    named_b = dict(b.named_parameters())
    for name in tr.names:
        off, numel = tr.slices[name]
        gb = named_b[name].grad          # (None: no term of this loss reaches the parameter)
        ga, gb = N(tr.flat_grad[off:off + numel]), np.zeros(numel, np.float32) if gb is None else N(gb).reshape(-1)
        scale, err = np.abs(gb).max(), np.abs(ga - gb).max()
        print(f"gradient {name}: max difference {err:.3e}, largest entry {scale:.3e}")
        assert err <= 3e-4 * scale + 1e-12, (name, err, scale)
        if name.startswith("tonemapper_net") or name in ("rgb_net.params", "xyz_encoder.params"):
            assert scale > 0, name
    # the NeRFLoss module's route of the same trainer (fused_loss off, as test_trainer_fused_loss_path_matches_module_path
    # switches it) fills loss_terms with the same five terms
    c = _field_model(ngp, 71)
    tr_c = NGPTrainer(c, lr=1e-2, use_exposure=True, unit_exposure_rgb=UNIT)
    tr_c.recipe.fused_loss = False
    tr_c.optimizer_step = lambda: None
    torch.manual_seed(73)
    loss_c, res_c = tr_c.step(o, d, gt, exposure=e.reshape(-1, 1))
    terms_c = N(res_c["loss_terms"])
    print("loss terms, trainer on the module route", terms_c)
    assert terms_c.shape == (5,) and float(loss_c) == terms_c[0]
    np.testing.assert_allclose(terms_c, terms_b, rtol=1e-6, atol=0)
    # the trainer refuses what the recipe does not take, on the device as on the host
    with pytest.raises(ValueError, match="needs exposure="):
        tr.step(o, d, gt)


# ------------------------------------------------------------------------------------------- the recipe end to end
# Half the gap of the one measured run of both tools (profiles/use_exposure.txt: 22.76 dB against 16.15 dB): the
# exposure-blind baseline sees the same poses at three brightnesses and cannot tell which one a test image wants
PSNR_MARGIN_DB = 3.3


def _tool(args):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py")] + args, capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_recipe_end_to_end(ngp, tmp_path):
    """tools/train_dataset.py --make_proxy --dataset_name colmap --use_exposure at 80 x 80, 600 steps of 2048 rays (the
    size of test_gpu_parity.test_train_from_other_dataset_formats): the JSON line has the new keys, the tone-mappers'
    colour at unit exposure moved towards 0.73, and the held-out PSNR at the two exposures never seen in training beats the
    same tool without --use_exposure on the same directory by PSNR_MARGIN_DB"""
    size = ["--num_epochs", "3", "--steps_per_epoch", "200", "--batch_size", "2048"]
    hdr = _tool(["--make_proxy", str(tmp_path), "--dataset_name", "colmap", "--downsample", "0.1", "--use_exposure"] + size)
    root = os.path.join(str(tmp_path), "HDR-NeRF", "syndata", "chair")
    assert len(os.listdir(os.path.join(root, "train"))) == 54 and len(os.listdir(os.path.join(root, "test"))) == 34
    blind = _tool(["--root_dir", root, "--dataset_name", "colmap"] + size)
    assert hdr["use_exposure"] is True and hdr["steps"] == 600 and hdr["img_wh"] == [80, 80] and hdr["loss_terms"] == 5
    assert len(hdr["test_psnr"]) == 34 and len(hdr["test_ssim"]) == 34 and len(blind["test_psnr"]) == 34
    assert hdr["unit_exposure_rgb"] == 0.73
    pred, init = np.array(hdr["unit_exposure_rgb_pred"]), np.array(hdr["unit_exposure_rgb_init"])
    assert pred.shape == (3,) and init.shape == (3,)
    print(f"use_exposure: held-out PSNR {hdr['test_psnr_mean']:.2f} dB, SSIM {hdr['test_ssim_mean']:.4f}; exposure-blind "
          f"baseline {blind['test_psnr_mean']:.2f} dB, SSIM {blind['test_ssim_mean']:.4f}; unit-exposure colour {init} -> {pred}; "
          f"term {hdr['unit_exposure_term_first']:.3e} -> {hdr['unit_exposure_term_last']:.3e}")
    assert (np.abs(pred - 0.73) < np.abs(init - 0.73)).all(), (init, pred)
    assert hdr["unit_exposure_term_last"] < hdr["unit_exposure_term_first"]
    assert hdr["test_psnr_mean"] > blind["test_psnr_mean"] + PSNR_MARGIN_DB, (hdr["test_psnr_mean"], blind["test_psnr_mean"])
