"""Transient mask field on the GPU: ngp_mask_field_fwd / ngp_mask_field_bwd against tests/mask_reference.py, the masked
render + loss tail against the launch-per-operation route and against the unmasked entry, and the trainer with a
msk_model."""
import os

import numpy as np
import pytest
import torch

import mask_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared references are read-only)


def N(t):
    return t.detach().cpu().numpy()


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


_REF = {}


def reference(n):
    """(params, kept uvi, dL_dmask, float64 forward, float64 backward) of the seeded batch of n rows: computed once,
    shared by the tests, never written to"""
    if n not in _REF:
        p = R.make_params()
        uvi_all = R.make_uvi(n)
        fwd_all = R.forward(p, uvi_all)
        keep = R.select_rows(p, uvi_all)
        assert 1.0 - keep.mean() <= R.MAX_DROPPED
        uvi = np.ascontiguousarray(uvi_all[keep])
        g = np.random.default_rng(1900 + n).standard_normal(len(uvi)).astype(np.float32)
        fwd = R.forward(p, uvi)
        _REF[n] = dict(p=p, uvi_all=uvi_all, fwd_all=fwd_all, uvi=uvi, g=g, fwd=fwd, bwd=R.backward(p, uvi, g, fwd))
        for v in _REF[n].values():
            for a in (v.values() if isinstance(v, dict) else [v]):
                a.setflags(write=False)
    return _REF[n]


def make_module(ngp, p):
    from ngp_amd.implicit_mask import implicit_mask
    msk = implicit_mask().to(DEV)
    with torch.no_grad():
        for k, v in msk.state_dict().items():
            v.copy_(T(p[k]))
    return msk


def lib_args(msk):
    l1, l2 = msk.mask_net[0], msk.mask_net[2]
    return msk.mask_encoder.desc, msk.mask_encoder.params, l1.weight, l1.bias, l2.weight, l2.bias


@pytest.mark.parametrize("n", R.SIZES)
def test_mask_field_forward(ngp, n):
    """one launch uvi -> mask against the float64 restatement (rtol 1e-5, atol 1e-5: tests/test_oracle_kat.py's bar for a
    linear layer with activation); the batch holds -0.5 and 0 exactly, cell faces of levels 0-2 and 0.49999997"""
    ref = reference(n)
    want = ref["fwd_all"]
    assert 0.1 < (want["z1"] > 0).mean() < 0.9
    if n >= 63:
        assert want["mask"].min() < 0.2 and want["mask"].max() > 0.8
    msk = make_module(ngp, ref["p"])
    with torch.no_grad():
        got = msk(T(ref["uvi_all"]))
    assert got.shape == (n, 1) and got.dtype == torch.float32
    got = N(got)[:, 0]
    print(f"n={n}: max |mask - ref| = {np.abs(got - want['mask']).max():.3g}")
    assert got.min() > 0 and got.max() < 1
    close(got, want["mask"], 1e-5, 1e-5)


def _run_bwd(ngp, msk, uvi, mask, g, outs):
    desc, table, W1, b1, W2, b2 = lib_args(msk)
    ngp._lib.call("mask_field_bwd", desc, table, W1, b1, W2, uvi, mask, g, uvi.shape[0], *outs)


def _check_grads(got, ref, factor=1.0):
    """dtable: rtol 1e-4, atol 1e-4 * max(1, 0.01 * max|ref|) (tests/test_gpu_parity.py's bar for atomic scatters);
    weight gradients: |diff| <= 1e-4 * max|ref| of the tensor"""
    want = ref["mask_encoder.params"] * factor
    atol = 1e-4 * max(1.0, 0.01 * float(np.abs(want).max()))
    print(f"  dtable: max |diff| = {np.abs(got[0] - want).max():.3g} (max|ref| {np.abs(want).max():.3g})")
    close(got[0], want, 1e-4, atol)
    for a, k in zip(got[1:], R.KEYS[1:]):
        w = ref[k].reshape(a.shape) * factor
        print(f"  {k}: max |diff| = {np.abs(a - w).max():.3g} (max|ref| {np.abs(w).max():.3g})")
        assert np.abs(a - w).max() <= 1e-4 * np.abs(w).max(), k


@pytest.mark.parametrize("n", R.SIZES)
def test_mask_field_backward(ngp, n):
    """one launch from dL_dmask: the table gradient against the oracle's scatter of the reference's d feat, the weight
    gradients against float64; two runs from zeroed accumulators agree within the same bars (float atomics: not
    necessarily bit for bit); a second call into the same accumulators doubles them"""
    ref = reference(n)
    msk = make_module(ngp, ref["p"])
    uvi, g = T(ref["uvi"]), T(ref["g"])
    assert len(ref["uvi"]) >= 1
    with torch.no_grad():
        mask = msk(uvi)[:, 0].contiguous()
    close(N(mask), ref["fwd"]["mask"], 1e-5, 1e-5)

    def zeros():
        return [torch.zeros(R.SHAPES[k], device=DEV) for k in R.KEYS]

    a, b = zeros(), zeros()
    _run_bwd(ngp, msk, uvi, mask, g, a)
    _run_bwd(ngp, msk, uvi, mask, g, b)
    once = [N(t) for t in a]
    _check_grads(once, ref["bwd"])
    _check_grads([N(t) for t in b], ref["bwd"])
    _run_bwd(ngp, msk, uvi, mask, g, a)          # accumulates
    _check_grads([N(t) for t in a], ref["bwd"], factor=2.0)
    assert np.count_nonzero(once[0]) > 0

    # the module's autograd route (no trainer): gradients reach .grad of all five tensors
    out = msk(uvi)
    out.backward(g[:, None])
    got = [N(dict(msk.named_parameters())[k].grad) for k in R.KEYS]
    _check_grads(got, ref["bwd"])


def _scene_model(ngp, seed):
    torch.manual_seed(seed)
    model = ngp.networks.NGP(scale=8.0).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    return model


@pytest.mark.parametrize("k", [0, 5000])
def test_masked_fused_tail_matches_the_launch_per_operation_route(ngp, k):
    """scale 8, exponential stepping, random background, 1500 rays, same marcher noise and background draw on both
    routes.  A: render + NeRFLoss(embed_msk=True, mask=msk(uvi), step=k) + sum of means + autograd; B: render with
    _fused_loss=FusedTail(gt, lambda_o, lambda_d, mask=msk(uvi), size_delta=size_delta).
    test_fused_tail_with_random_background_and_codes' bars."""
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    model = _scene_model(ngp, 33)
    msk = make_module(ngp, R.make_params())
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    uvi = msk.uvi(torch.stack([pix // 100, pix % 100], -1), img, (100, 100), 6)
    loss_fn = NeRFLoss()
    lam_o, lam_d = loss_fn.lambda_opa, loss_fn.lambda_distortion
    size_delta = loss_fn.Annealing.getWeight(k)
    assert size_delta == (1.0 if k == 0 else 6e-2)
    params = [p for p in model.parameters() if p.numel() > 0] + list(msk.parameters())
    out = {}
    for fused in (False, True):
        for p in params:
            p.grad = None
        torch.manual_seed(35)
        kw = dict(exp_step_factor=1 / 256, num_classes=7, random_bg=True)
        if fused:
            res = render(model, o, d, _fused_loss=FusedTail(gt, lam_o, lam_d, mask=msk(uvi), size_delta=size_delta), **kw)
            assert "_loss_terms" in res
            terms = res.pop("_loss_terms")
            assert terms.shape == (5,)
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0, 0], device=DEV)])
            terms = N(terms)
        else:
            res = render(model, o, d, **kw)
            ld = loss_fn(res, {"rgb": gt}, embed_msk=True, mask=msk(uvi), step=k)
            loss = sum(t.mean() for t in ld.values())
            loss.backward()
            terms = np.array([float(loss.detach())] + [float(ld[n].detach().mean()) for n in ("rgb", "opacity", "distortion", "r_ms")], np.float32)
        out[fused] = (res, terms, [None if p.grad is None else N(p.grad).copy() for p in params])
    ra, ta, ga = out[False]
    rb, tb, gb = out[True]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for key in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp"):
        close(N(rb[key]), N(ra[key]), 2e-5, 2e-6)
    print("terms A", ta, "terms B", tb)
    close(tb, ta, 1e-4, 1e-9)
    assert tb[4] > 0
    for p, a, b in zip(params, ga, gb):
        if a is None:
            assert b is None or not b.any()
            continue
        scale = np.abs(a).max()
        assert np.abs(a - b).max() <= 3e-4 * scale + 1e-12, (tuple(p.shape), np.abs(a - b).max(), scale)
    table_grad = gb[len(params) - 5]
    assert table_grad.shape == R.SHAPES["mask_encoder.params"] and np.abs(table_grad).sum() > 0


def _tail_inputs(n_rays, seed):
    """field outputs for the two render + loss entries: random segments (some empty), densities that stop some rays early"""
    g = np.random.default_rng(seed)
    counts = g.integers(0, 90, n_rays)
    counts[::11] = 0
    starts = np.cumsum(counts) - counts
    n = int(counts.sum())
    rays_a = np.stack([np.arange(n_rays), starts, counts], 1).astype(np.int64)
    f = lambda *s: g.random(s).astype(np.float32)
    return dict(n=n, sig=f(n) * 40, rgbs=f(n, 3), dsig=g.standard_normal((n, 3)).astype(np.float32),
                nrm=g.standard_normal((n, 3)).astype(np.float32), sem=g.standard_normal((n, 7)).astype(np.float32),
                dirs=g.standard_normal((n, 3)).astype(np.float32), deltas=f(n) * 0.02 + 1e-3,
                ts=np.sort(f(n) * 3), rays_a=rays_a, gt=f(n_rays, 3), bg=f(3))


def _run_tail(ngp, x, n_rays, masked, mask=None, size_delta=0.0):
    n, classes = x["n"], 7
    t = {k: T(v) for k, v in x.items() if k != "n"}
    E = lambda *s: torch.full(s, float("nan"), device=DEV)
    total = torch.zeros(n_rays, dtype=torch.int64, device=DEV)
    vr = torch.zeros(1, dtype=torch.int64, device=DEV)
    o = dict(opacity=E(n_rays), depth=E(n_rays), rgb=E(n_rays, 3), normal=E(n_rays, 3), sem=E(n_rays, classes), ws=E(n),
             Ro=E(n_rays), Rp=E(n_rays, 3), terms=E(5 if masked else 4), d_sig=E(n), d_rgb=E(n, 3))
    head = (t["sig"], t["rgbs"], t["dsig"], None, t["nrm"], 3, t["sem"], 7, t["dirs"], t["deltas"], t["ts"], t["rays_a"],
            t["gt"], t["bg"])
    tail = (1e-4, classes, n_rays, 2e-4, 3e-4, total, vr, o["opacity"], o["depth"], o["rgb"], o["normal"], o["sem"],
            o["ws"], o["Ro"], o["Rp"], o["terms"], o["d_sig"], o["d_rgb"])
    if masked:
        o["d_mask"] = E(n_rays)
        ngp._lib.call("render_loss_fused_masked", *head, mask, float(size_delta), *tail, o["d_mask"])
    else:
        ngp._lib.call("render_loss_fused", *head, *tail)
    o["total"], o["vr"] = total, vr
    return {k: N(v) for k, v in o.items()}


@pytest.mark.parametrize("n_rays", [8, 1500])
def test_masked_entry_with_a_zero_mask_is_the_unmasked_entry(ngp, n_rays):
    """ngp_render_loss_fused_masked with mask = 0 and size_delta = 0 against ngp_render_loss_fused on the same inputs, bit
    for bit (products by 1.0 and sums with 0.0 are exact), and dL_dmask = -(sum e^2) / (3 R).  8 rays are one workgroup:
    every output, the loss terms included, bit for bit.  With 1500 rays the terms are sums of one float atomic per
    workgroup (188 of them) in whatever order the workgroups retire, in BOTH entries, so two launches of the unmasked
    entry itself need not agree in the last bit: there the terms are held to the worst case of reordering 188 additions
    of non-negative float32 values, 188 * 2^-24 = 1.2e-5 relative, and everything else bit for bit."""
    x = _tail_inputs(n_rays, 41 + n_rays)
    a = _run_tail(ngp, x, n_rays, False)
    b = _run_tail(ngp, x, n_rays, True, mask=torch.zeros(n_rays, device=DEV), size_delta=0.0)
    assert a["vr"][0] > 0 and (a["total"] < x["rays_a"][:, 2]).any()      # some rays stop early
    for k in ("total", "vr", "opacity", "depth", "rgb", "normal", "sem", "ws", "Ro", "Rp", "d_sig", "d_rgb"):
        assert not np.isnan(a[k].astype(np.float64)).any(), k
        assert np.array_equal(a[k], b[k]), k
    print("terms unmasked", a["terms"], "masked", b["terms"])
    if n_rays == 8:
        assert np.array_equal(a["terms"], b["terms"][:4])
    else:
        close(b["terms"][:4], a["terms"], 1.2e-5, 0)
    assert b["terms"][4] == 0
    e2 = ((a["rgb"].astype(np.float64) - x["gt"]) ** 2).sum(1)
    close(b["d_mask"], -e2 / (3.0 * n_rays), 1e-6, 0)


def _train_setup(ngp, seed, scale, n_images, wh):
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.synthetic import LegoProxy
    torch.manual_seed(seed)
    model = ngp.networks.NGP(scale=scale).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    msk = implicit_mask().to(DEV)
    scene = LegoProxy(n_images=n_images, img_wh=(wh, wh), device=DEV)
    return model, msk, scene


def test_trainer_with_a_mask_model(ngp, tmp_path):
    """NGPTrainer(model, msk_model=msk), 24 steps of 2048 rays as in test_trainer_unbounded_configs: the step stays on
    the fused tail and on the norm-bound clip, the mask parameters live in the flat store and move, a missing uvi
    raises, and a checkpoint restores the mask bit for bit"""
    from ngp_amd import ckpt
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    model, msk, scene = _train_setup(ngp, 31, 8.0, 20, 200)
    before = {k: v.detach().clone() for k, v in msk.state_dict().items()}
    tr = NGPTrainer(model, lr=1e-2, exp_step_factor=1 / 256, render_kwargs={"random_bg": True}, msk_model=msk)
    assert "msk_model.mask_encoder.params" in tr.slices and tr.names[:2] == ["rgb_encoder.params", "xyz_encoder.params"]
    assert all(tr.slices["msk_model." + k][0] >= tr._mlp_lo for k in R.KEYS)
    assert msk.mask_encoder.params.data_ptr() == tr.flat_param[tr.slices["msk_model.mask_encoder.params"][0]:].data_ptr()
    gen = torch.Generator(device=DEV).manual_seed(32)
    losses, bound_steps = [], 0
    for i in range(24):
        img, pix = scene.sample_batch(2048, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        uvi = implicit_mask.uvi(torch.stack([pix // 200, pix % 200], -1), img, (200, 200), 20)
        if i == 3:
            with pytest.raises(ValueError, match="uvi"):
                tr.step(o, d, gt)
        seen = {}
        orig = tr.optimizer_step

        def spy():
            seen["bound"], seen["fused"] = tr._bound_step, tr.recipe.fused_loss
            orig()
        tr.optimizer_step = spy
        loss, res = tr.step(o, d, gt, uvi=uvi)
        tr.optimizer_step = orig
        assert seen["fused"] is True and seen["bound"] is True, (i, seen)
        assert "_loss_terms" not in res and res["rgb"].shape == (2048, 3)
        losses.append(float(loss))
    tr.wait()
    assert tr.recipe.fused_loss is True
    assert np.isfinite(losses).all()
    assert np.mean(losses[-4:]) < np.mean(losses[:4])
    assert torch.isfinite(tr.flat_param).all()
    for k, v in msk.state_dict().items():
        assert torch.isfinite(v).all() and not torch.equal(v, before[k]), k
    path = os.path.join(tmp_path, "masked.ckpt")
    ckpt.save_ckpt(model, path, msk_model=msk)
    fresh = implicit_mask().to(DEV)
    ckpt.load_ckpt(fresh, path, model_name='msk_model', prefixes_to_ignore=['model', 'embedding_a'])
    with torch.no_grad():
        assert torch.equal(fresh(uvi), msk(uvi))
    other = ngp.networks.NGP(scale=8.0).to(DEV)      # the render tools' call on such a checkpoint
    ckpt.load_ckpt(other, path, prefixes_to_ignore=['embedding_a', 'msk_model', 'density_grid', 'grid_coords'])
    assert torch.equal(other.xyz_encoder.params, model.xyz_encoder.params)


MASKS_STEPS = 150


def test_the_mask_rises_where_the_images_disagree(ngp):
    """the proxy scene with a saturated rectangle pasted into the ground truth of half of the training images (here, not
    in the dataset code): the colour error stays large there, dL_dmask = 2 size_delta m / R - sum e^2 / (3 R) is negative,
    and after MASKS_STEPS steps the mean mask over the pasted pixels exceeds the mean over the clean pixels of the same
    images.  Only the ordering is required."""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    wh, n_img = 64, 8
    model, msk, scene = _train_setup(ngp, 51, 0.5, n_img, wh)
    tr = NGPTrainer(model, lr=1e-2, msk_model=msk)
    gen = torch.Generator(device=DEV).manual_seed(52)
    paint = torch.tensor([1.0, 0.0, 1.0], device=DEV)

    def pasted(img, pix):
        row, col = pix // wh, pix % wh
        return (img % 2 == 0) & (row >= 16) & (row < 40) & (col >= 20) & (col < 48)

    for i in range(MASKS_STEPS):
        img, pix = scene.sample_batch(2048, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        gt = torch.where(pasted(img, pix)[:, None], paint, gt)
        uvi = implicit_mask.uvi(torch.stack([pix // wh, pix % wh], -1), img, (wh, wh), n_img)
        tr.step(o, d, gt.contiguous(), uvi=uvi)
    tr.wait()
    pix = torch.arange(wh * wh, device=DEV)
    inside, outside = [], []
    with torch.no_grad():
        for i in range(0, n_img, 2):
            img = torch.full_like(pix, i)
            m = msk(implicit_mask.uvi(torch.stack([pix // wh, pix % wh], -1), img, (wh, wh), n_img))[:, 0]
            sel = pasted(img, pix)
            inside.append(m[sel])
            outside.append(m[~sel])
    m_in, m_out = float(torch.cat(inside).mean()), float(torch.cat(outside).mean())
    print(f"mean mask over pasted pixels {m_in:.4f}, over clean pixels {m_out:.4f}, ratio {m_in / m_out:.3f} "
          f"after {MASKS_STEPS} steps")
    assert m_in / m_out > 1
