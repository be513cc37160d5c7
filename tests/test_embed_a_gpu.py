"""Appearance codes (embed_a) on the GPU: ngp_embed_a_fwd against torch's gather + repeat_interleave bit for bit,
ngp_embed_a_bwd against float64 numpy, the RayCodes route of the field against the tensor route, the trainer's table in
the flat store, a scene whose images are tinted two ways, and the train -> checkpoint -> render round trip of the tools."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 1024)
N_RAYS = (1, 3, 65, 300)
# (E, n_cols): the issue's seven take the float4 route (column 144 of a matrix whose row stride is a multiple of 4); the
# last three take the one-float-per-lane route: a row stride that is no multiple of 4, and 12 columns (3 float4 a row do
# not divide a wave)
SHAPES = ((1, 16), (4, 16), (7, 16), (8, 16), (12, 16), (16, 16), (20, 32), (3, 5), (8, 12), (32, 33))
SENTINEL = -7.25
EXTRA_ROWS, EXTRA_COLS = 5, 8


def N(t):
    return t.detach().cpu().numpy()


def make_segments(n_rays, seed):
    """rays_a (n_rays, 3) int64: counts drawn from COUNTS (1024 rarely, but at least once from 65 rays on), a zero-count ray
    first, last and in the middle (3 rays: first and last; 1 ray: none, or nothing would be written), segments tiling
    [0, N) in row order, and a ray-index column that is a permutation other than the identity (1 ray: the identity)"""
    g = np.random.default_rng(seed)
    p = np.array([2, 2, 2, 2, 2, 2, 2, 2, 0.15])
    counts = g.choice(COUNTS, size=n_rays, p=p / p.sum())
    if n_rays == 1:
        counts[:] = 33
    elif n_rays == 3:
        counts[:] = (0, 65, 0)
    else:
        counts[[0, n_rays // 2, n_rays - 1]] = 0
        counts[[1, n_rays - 2]] = (1024, 1)
    starts = np.cumsum(counts) - counts
    perm = np.roll(np.arange(n_rays), 1) if n_rays < 4 else g.permutation(n_rays)
    if n_rays > 1:
        assert not np.array_equal(perm, np.arange(n_rays))
    return np.stack([perm, starts, counts], 1).astype(np.int64)


def index_patterns(n_rays, seed):
    """{name: (img_idxs (n_rays) int64, n_imgs)}: the four patterns of the backward test"""
    g = np.random.default_rng(seed + 1000)
    return {"one_image": (np.full(n_rays, 3, np.int64), 6),
            "sorted": (np.sort(g.integers(0, 6, n_rays)).astype(np.int64), 6),
            "random_5": (g.integers(0, 5, n_rays).astype(np.int64), 6),
            "random_400": (g.integers(0, 400, n_rays).astype(np.int64), 400)}


def expected_forward(weight, img_idxs, rays_a, E, n_cols):
    """the torch chain the kernel replaces, plus the ones block; an out-of-range image gives zero codes"""
    n_imgs = weight.shape[0]
    ok = (img_idxs >= 0) & (img_idxs < n_imgs)
    per_ray = weight[img_idxs.clamp(0, n_imgs - 1)] * ok[:, None]
    codes = torch.repeat_interleave(per_ray[rays_a[:, 0]], rays_a[:, 2], 0)
    return torch.cat([codes, torch.ones(codes.shape[0], n_cols - E, device=codes.device)], 1)


@pytest.mark.parametrize("E,n_cols", SHAPES)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_forward_is_the_gather_bit_for_bit(ngp, n_rays, E, n_cols):
    from ngp_amd._lib import call
    odd_stride = (E, n_cols) == (3, 5)
    ld = 144 + n_cols + EXTRA_COLS + (3 if odd_stride else 0)
    rays_a_np = make_segments(n_rays, 100 + n_rays)
    n = int(rays_a_np[:, 2].sum())
    rays_a = torch.from_numpy(rays_a_np).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7 * n_rays + E)
    n_imgs = 9
    weight = torch.randn(n_imgs, E, device=DEV, generator=g)
    for bad in (None, n_imgs, -1):
        img = torch.randint(n_imgs, (n_rays,), device=DEV, generator=g)
        if bad is not None:
            r = int(rays_a_np[np.argmax(rays_a_np[:, 2]), 0])       # the ray of the longest segment
            img[r] = bad
        buf = torch.full((n + EXTRA_ROWS, ld), SENTINEL, device=DEV)
        call("embed_a_fwd", weight, n_imgs, E, img, rays_a, n_rays, buf[:, 144:], ld, n_cols)
        want = expected_forward(weight, img, rays_a, E, n_cols)
        assert want.shape == (n, n_cols)
        assert torch.equal(buf[:n, 144:144 + n_cols], want), (n_rays, E, n_cols, bad)
        assert (buf[:, :144] == SENTINEL).all() and (buf[:, 144 + n_cols:] == SENTINEL).all()
        assert (buf[n:] == SENTINEL).all()
        if bad is not None:
            s, c = (int(v) for v in rays_a_np[np.argmax(rays_a_np[:, 2]), 1:])
            assert c > 0 and (buf[s:s + c, 144:144 + E] == 0).all() and (buf[s:s + c, 144 + E:144 + n_cols] == 1).all()


def test_forward_leaves_rows_between_segments_alone(ngp):
    """segments with gaps between them (not what the marcher emits): the rows of the gaps keep the sentinel"""
    from ngp_amd._lib import call
    rays_a = torch.tensor([[1, 4, 3], [0, 10, 0], [2, 12, 70]], dtype=torch.int64, device=DEV)
    weight = torch.arange(24, dtype=torch.float32, device=DEV).reshape(3, 8)
    img = torch.tensor([2, 0, 1], device=DEV)
    buf = torch.full((90, 160), SENTINEL, device=DEV)
    call("embed_a_fwd", weight, 3, 8, img, rays_a, 3, buf[:, 144:], 160, 16)
    covered = torch.zeros(90, dtype=torch.bool, device=DEV)
    covered[4:7] = covered[12:82] = True
    assert (buf[~covered] == SENTINEL).all() and (buf[:, :144] == SENTINEL).all()
    assert torch.equal(buf[4:7, 144:152], weight[0].expand(3, 8)) and torch.equal(buf[12:82, 144:152], weight[1].expand(70, 8))
    assert (buf[covered][:, 152:] == 1).all()


@pytest.mark.parametrize("E", sorted({e for e, _ in SHAPES}))
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_backward_against_float64(ngp, n_rays, E):
    """d_weight = pre-fill + float64 sums to 1e-4 of the case's largest |sum| (the bar for atomically
    accumulated gradients); rows no ray names keep their pre-fill exactly; an out-of-range ray adds nothing"""
    from ngp_amd._lib import call
    rays_a_np = make_segments(n_rays, 100 + n_rays)
    n = int(rays_a_np[:, 2].sum())
    rays_a = torch.from_numpy(rays_a_np).to(DEV)
    ld = 128 + E
    g = np.random.default_rng(5000 + 31 * n_rays + E)
    d_np = g.standard_normal((n + EXTRA_ROWS, ld)).astype(np.float32)
    d = torch.from_numpy(d_np).to(DEV)
    worst = 0.0
    for name, (img_np, n_imgs) in index_patterns(n_rays, n_rays + E).items():
        for bad in (None, n_imgs, -5):
            img_np = img_np.copy()
            if bad is not None:
                img_np[int(rays_a_np[np.argmax(rays_a_np[:, 2]), 0])] = bad
            want = np.zeros((n_imgs, E), np.float64)
            named = np.zeros(n_imgs, bool)
            for ray, s, c in rays_a_np:
                i = img_np[ray]
                if 0 <= i < n_imgs and c > 0:
                    want[i] += d_np[s:s + c, 128:].astype(np.float64).sum(0)
                    named[i] = True
            pre_np = g.standard_normal((n_imgs, E)).astype(np.float32)
            d_weight = torch.from_numpy(pre_np).to(DEV)
            call("embed_a_bwd", d[:, 128:], ld, E, torch.from_numpy(img_np).to(DEV), rays_a, n_rays, n_imgs, d_weight)
            got = N(d_weight)
            scale = np.abs(want).max()
            err = np.abs(got.astype(np.float64) - (pre_np.astype(np.float64) + want)).max()
            worst = max(worst, err / scale) if scale > 0 else worst
            print(f"embed_a_bwd n_rays={n_rays} E={E} {name} bad={bad}: max err {err:.3e}, largest |sum| {scale:.3e}")
            assert err <= 1e-4 * scale, (name, bad, err, scale)
            assert np.array_equal(got[~named], pre_np[~named]), (name, bad)
            if name == "random_400" and n_rays >= 65:
                assert (~named).sum() > 100
    print(f"embed_a_bwd n_rays={n_rays} E={E}: worst err / largest |sum| = {worst:.3e}")


def _playground_model(ngp, seed):
    torch.manual_seed(seed)
    model = ngp.networks.NGP(scale=8.0, embed_a=True, embed_a_len=8).to(DEV)
    _add_grid(model)
    return model


def _add_grid(model):
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())


@pytest.mark.parametrize("fused", [True, False])
def test_field_route_against_the_tensor_route(ngp, fused):
    """the setup of test_gpu_parity.test_fused_tail_with_random_background_and_codes (scale 8, E = 8, 6 images, 1500 rays,
    same seeds), rendered with embedding_a=codes[img] and with RayCodes(codes, img): rgb_net's input is the same matrix, so
    every per-ray result is bit-identical; the loss terms, which several workgroups add up atomically, to 1e-6 relative;
    every gradient within 3e-4 of the tensor route's largest entry (that test's own bar); codes.grad is not zero"""
    from ngp_amd.appearance import RayCodes
    from ngp_amd.losses import nerf_loss_and_grads, NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    from ngp_amd.synthetic import LegoProxy
    model = _playground_model(ngp, 33)
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.5)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    scene = LegoProxy(n_images=6, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(34)
    img, pix = scene.sample_batch(1500, generator=gen)
    o, d = scene.rays(img, pix)
    gt = torch.rand(1500, 3, device=DEV, generator=gen)
    codes = torch.nn.Parameter(torch.randn(6, 8, device=DEV) * 0.1)
    lam_o, lam_d = NeRFLoss().lambda_opa, NeRFLoss().lambda_distortion
    params = [p for p in model.parameters() if p.numel() > 0] + [codes]
    out = {}
    for route in ("tensor", "ray_codes"):
        for p in params:
            p.grad = None
        torch.manual_seed(35)                      # same marcher noise, same background colour
        emb = codes[img] if route == "tensor" else RayCodes(codes, img)
        kw = dict(exp_step_factor=1 / 256, num_classes=7, random_bg=True, embedding_a=emb)
        if fused:
            res = render(model, o, d, _fused_loss=FusedTail(gt, lam_o, lam_d), **kw)
            terms = res.pop("_loss_terms")
            torch.autograd.backward([terms], [torch.tensor([1.0, 0, 0, 0], device=DEV)])
        else:
            res = render(model, o, d, **kw)
            terms, (d_rgb, d_op, d_ws) = nerf_loss_and_grads(res["rgb"], res["opacity"], res["ws"], res["deltas"], res["ts"],
                                                            res["rays_a"], gt, lam_o, lam_d)
            torch.autograd.backward([res["rgb"], res["opacity"], res["ws"]], [d_rgb, d_op, d_ws])
        out[route] = (res, N(terms), [None if p.grad is None else N(p.grad).copy() for p in params])
    ra, ta, ga = out["tensor"]
    rb, tb, gb = out["ray_codes"]
    assert int(ra["total_samples"]) == int(rb["total_samples"]) > 0
    for k in ("opacity", "depth", "rgb", "normal_pred", "semantic", "ws", "Ro", "Rp", "sigma"):
        assert torch.equal(ra[k], rb[k]), k
    print("loss terms, tensor route", ta, "RayCodes route", tb)
    np.testing.assert_allclose(tb, ta, rtol=1e-6, atol=0)
    for p, a, b in zip(params, ga, gb):
        if a is None:
            assert b is None or not b.any()
            continue
        scale = np.abs(a).max()
        err = np.abs(a - b).max()
        print(f"gradient {tuple(p.shape)}: max difference {err:.3e}, largest entry {scale:.3e}")
        assert err <= 3e-4 * scale + 1e-12, (tuple(p.shape), err, scale)
    assert np.abs(gb[-1]).sum() > 0 and np.abs(ga[-1]).sum() > 0


def _trainer_run(ngp, with_mask):
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    model = _playground_model(ngp, 31)
    torch.manual_seed(41)
    emb = torch.nn.Embedding(20, 8).to(DEV)
    msk = implicit_mask().to(DEV) if with_mask else None
    before = emb.weight.detach().clone()
    msk_before = None if msk is None else msk.mask_encoder.params.detach().clone()
    scene = LegoProxy(n_images=20, img_wh=(200, 200), device=DEV)
    tr = NGPTrainer(model, lr=1e-2, exp_step_factor=1 / 256, render_kwargs={"random_bg": True}, embedding_a=emb,
                    msk_model=msk)
    gen = torch.Generator(device=DEV).manual_seed(32)
    losses = []
    for i in range(8):
        img, pix = scene.sample_batch(1024, generator=gen)
        img = img % 12                               # the batches only ever name images 0..11 of the 20
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        uvi = implicit_mask.uvi(torch.stack([pix // 200, pix % 200], -1), img, (200, 200), 20) if with_mask else None
        if i == 2:
            with pytest.raises(ValueError, match="img_idxs"):
                tr.step(o, d, gt, uvi=uvi)
        loss, res = tr.step(o, d, gt, uvi=uvi, img_idxs=img)
        assert "_loss_terms" not in res and res["rgb"].shape == (1024, 3)
        losses.append(float(loss))
    tr.wait()
    torch.cuda.synchronize()
    return tr, emb, before, msk, msk_before, losses


def test_trainer_owns_the_table(ngp):
    """20 images of which the batches name 12, 8 steps of 1024 rays: the table is a view of the flat store behind the MLPs,
    the step stays on the fused tail, the rows of the 12 seen images move and the other 8 keep their bits (g = m = v = 0
    there, and Adam then leaves p alone)"""
    tr, emb, before, _, _, losses = _trainer_run(ngp, False)
    assert "embedding_a.weight" in tr.names and tr.names[:2] == ["rgb_encoder.params", "xyz_encoder.params"]
    off, numel = tr.slices["embedding_a.weight"]
    assert numel == 160 and off >= tr._mlp_lo
    assert emb.weight.data_ptr() == tr.flat_param[off:].data_ptr()
    assert emb.weight.grad.data_ptr() == tr.flat_grad[off:].data_ptr()
    assert tr.model.link.grad_sinks["embedding_a"].data_ptr() == tr.flat_grad[off:].data_ptr()
    assert tr.recipe.fused_loss is True and tr.norm_bound is True
    assert np.isfinite(losses).all()
    assert torch.isfinite(tr.flat_param).all()
    w = emb.weight.detach()
    assert all(not torch.equal(w[i], before[i]) for i in range(12))
    assert torch.equal(w[12:], before[12:])


def test_trainer_with_table_and_mask_model(ngp):
    """the same run with msk_model= as well (the Playground recipe): finite, and both tables move"""
    tr, emb, before, msk, msk_before, losses = _trainer_run(ngp, True)
    assert "embedding_a.weight" in tr.names and "msk_model.mask_encoder.params" in tr.names
    assert np.isfinite(losses).all() and torch.isfinite(tr.flat_param).all()
    assert not torch.equal(emb.weight.detach()[:12], before[:12]) and torch.equal(emb.weight.detach()[12:], before[12:])
    assert not torch.equal(msk.mask_encoder.params.detach(), msk_before)


TINT_STEPS = 300
TINTS = ((1.0, 0.6, 0.6), (0.6, 0.6, 1.0))      # even images, odd images


def tinted_run(ngp, embed_a, steps=TINT_STEPS):
    """proxy scene, scale 0.5, 8 images of 64 x 64, 2048 rays a step; the ground truth of even images is multiplied by
    TINTS[0], that of odd images by TINTS[1] -> (model, table or None, scene, train PSNR of the last 20 steps)"""
    from ngp_amd.metrics import psnr
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    torch.manual_seed(61)
    model = (ngp.networks.NGP(scale=0.5, embed_a=True, embed_a_len=8) if embed_a else ngp.networks.NGP(scale=0.5)).to(DEV)
    _add_grid(model)
    emb = torch.nn.Embedding(8, 8).to(DEV) if embed_a else None
    scene = LegoProxy(n_images=8, img_wh=(64, 64), device=DEV)
    tr = NGPTrainer(model, lr=1e-2, embedding_a=emb)
    tints = torch.tensor(TINTS, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(62)
    tail = []
    for i in range(steps):
        img, pix = scene.sample_batch(2048, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        gt = (gt * tints[img % 2]).contiguous()
        _, res = tr.step(o, d, gt, **({"img_idxs": img} if embed_a else {}))
        if i >= steps - 20:
            tail.append(psnr(res["rgb"].detach(), gt))
    tr.wait()
    return model, emb, scene, float(torch.stack(tail).mean())


def tint_means(model, emb, scene):
    """training pose 0 rendered at test time with the code of image 0 and of image 1 -> mean(R - B) over the pixels with
    opacity > 0.5, for either code"""
    from ngp_amd.rendering import render
    pix = torch.arange(64 * 64, device=DEV)
    o, d = scene.rays(torch.zeros_like(pix), pix)
    means = []
    with torch.no_grad():
        for k in (0, 1):
            res = render(model, o, d, test_time=True, embedding_a=emb.weight[k:k + 1].detach().contiguous())
            solid = res["opacity"] > 0.5
            assert int(solid.sum()) > 100
            means.append(float((res["rgb"][solid, 0] - res["rgb"][solid, 2]).mean()))
    return means


def test_codes_learn_the_tint_of_their_images(ngp):
    """it learns what it is for: the same view comes out reddish with the code of an even image and bluish with the code of
    an odd one.  The sign criterion is fixed; the step count is TINT_STEPS."""
    model, emb, scene, train_psnr = tinted_run(ngp, True)
    m0, m1 = tint_means(model, emb, scene)
    print(f"after {TINT_STEPS} steps: mean(R - B) with code 0 {m0:+.4f}, with code 1 {m1:+.4f}; train PSNR {train_psnr:.2f} dB")
    assert m0 > 0 and m1 < 0, (m0, m1)


def test_tool_round_trip(ngp, tmp_path):
    """tools/train_dataset.py --embed_a on the proxy scene at 100 x 100 writes a checkpoint with the (100, 4) table, and
    tools/render.py --embed_a renders its frames from it (codes by the mean of the two nearest training cameras)"""
    ckpt_path = str(tmp_path / "codes.ckpt")
    scene_dir, frames = str(tmp_path / "scene"), str(tmp_path / "frames")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py"), "--make_proxy", scene_dir,
                          "--downsample", "0.125", "--num_epochs", "1", "--steps_per_epoch", "300", "--batch_size", "2048",
                          "--embed_a", "--embed_a_len", "4", "--ckpt_path", ckpt_path],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 300 and line["img_wh"] == [100, 100] and np.isfinite(line["test_psnr_mean"])
    sd = torch.load(ckpt_path, weights_only=True)["state_dict"]
    assert tuple(sd["embedding_a.weight"].shape) == (100, 4) and torch.isfinite(sd["embedding_a.weight"]).all()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py"), "--ckpt", ckpt_path, "--root_dir",
                          os.path.join(scene_dir), "--downsample", "0.125", "--out_dir", frames, "--render_rgb", "--embed_a",
                          "--embed_a_len", "4"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames"] == 8 and line["img_wh"] == [100, 100]
    for i in range(8):
        assert os.path.getsize(os.path.join(frames, f"{i:03d}-rgb.png")) > 0
    print("tool round trip: test PSNR", line.get("psnr_mean"))
