"""Pose refinement (optimize_ext) on the GPU: ngp_pose_rays_fwd, ngp_pose_rays_bwd and ngp_sh_bwd_dirs against the float64
restatements of tests/pose_reference.py, one trainer step against torch autograd through the same route, a registration run
on the proxy scene, and the default path left as it was.

Bars of the three kernel tests.  Per case (one launch: the same inputs) and per output, 4 x YARD, where YARD is the
largest error, relative to the case's largest |float64 value|, that the SAME restatement makes on that case when it is run
in float32 instead of float64 (computed once per module, on the CPU).  The factor 4 covers a different summation order and
the atomics.  No case's yardstick serves another case.  Every launch of the backward family carries ONE |v| (all images,
random axes), so the cases in which the literal float32 formula cancels (|v| = 1e-4, 1e-2) set no bar but their own.
Measured values: profiles/pose_refine.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = (1, 7, 64, 65, 300)
N_IMGS = (1, 3, 40)
SH_N = (1, 63, 64, 65, 4099)
SH_KINDS = ("unit", "axis", "tiny", "lengths")


def N(t):
    return t.detach().cpu().numpy()


def G(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---------------------------------------------------------------------------- forward
def fwd_case(n_rays, n_imgs, shift):
    """image i carries |v| = ANGLES[(i + shift) % 6]; the last third of the rays (from 7 on) have an index out of range"""
    angles = pr.ANGLES[shift:] + pr.ANGLES[:shift]
    poses, dR, dT, directions = pr.make_cameras(n_imgs, 10 * n_imgs + shift, angles)
    g = np.random.default_rng(1000 * n_rays + n_imgs + shift)
    img = g.integers(0, n_imgs, n_rays).astype(np.int64)
    pix = g.integers(0, len(directions), n_rays).astype(np.int64)
    if n_rays >= 7:
        img[-1], img[-2], pix[-3], pix[-4] = n_imgs, -1, len(directions), -7
    return poses, dR, dT, directions, img, pix


def fwd_restated(case, dtype):
    poses, dR, dT, directions, img, pix = case
    T = lambda a: torch.from_numpy(a).to(dtype)
    o, d = pr.pose_rays(T(poses), T(dR), T(dT), T(directions), torch.from_numpy(img), torch.from_numpy(pix))
    return o.double().numpy(), d.double().numpy()


@pytest.fixture(scope="module")
def fwd_family():
    """{(n_rays, n_imgs, shift): (inputs, float64 result, (yardstick of rays_o, of rays_d) of THIS case)}"""
    cases = {}
    for n_rays in N_RAYS:
        for n_imgs in N_IMGS:
            for shift in range(len(pr.ANGLES)):
                c = fwd_case(n_rays, n_imgs, shift)
                want, f32 = fwd_restated(c, torch.float64), fwd_restated(c, torch.float32)
                cases[(n_rays, n_imgs, shift)] = (c, want, tuple(pr.rel_err(f32[k], want[k])[0] for k in range(2)))
    # float32 costs a few units in the last place and no more: a restatement that had gone wrong would not be a yardstick
    assert all(y[0] < 1.2e-7 and y[1] < 1e-6 for _, _, y in cases.values())
    return cases


@pytest.mark.parametrize("n_imgs", N_IMGS)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_forward_against_float64(ngp, fwd_family, n_rays, n_imgs):
    from ngp_amd._lib import call
    failed = []
    for shift in range(len(pr.ANGLES)):
        (poses, dR, dT, directions, img, pix), want, yard = fwd_family[(n_rays, n_imgs, shift)]
        o = torch.full((n_rays + 3, 3), float("nan"), device=DEV)
        d = torch.full((n_rays + 3, 3), float("nan"), device=DEV)
        call("pose_rays_fwd", G(poses), G(dR), G(dT), G(directions), G(img), G(pix), n_imgs, len(directions), n_rays, o, d)
        assert torch.isnan(o[n_rays:]).all() and torch.isnan(d[n_rays:]).all()
        got = (N(o[:n_rays]), N(d[:n_rays]))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        bad = (img < 0) | (img >= n_imgs) | (pix < 0) | (pix >= len(directions))
        assert not got[0][bad].any() and not got[1][bad].any()
        assert n_rays < 7 or bad.sum() == 4
        err = [pr.rel_err(got[k], want[k])[0] for k in range(2)]
        print(f"pose_rays_fwd n_rays={n_rays} n_imgs={n_imgs} shift={shift}: rays_o kernel {err[0]:.3e} yardstick {yard[0]:.3e} "
              f"(bar {4 * yard[0]:.3e}); rays_d kernel {err[1]:.3e} yardstick {yard[1]:.3e} (bar {4 * yard[1]:.3e})")
        failed += [(name, shift, err[k], yard[k]) for k, name in enumerate(("rays_o", "rays_d")) if not err[k] <= 4 * yard[k]]
    assert not failed, failed


@pytest.mark.parametrize("n_imgs", N_IMGS)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_forward_at_zero_is_get_rays_bit_for_bit(ngp, n_rays, n_imgs):
    """dR = dT = 0: rays_o is poses[img][:, 3] and rays_d the float32 fixed-order product (R_i0 d_0 + R_i1 d_1) + R_i2 d_2"""
    from ngp_amd._lib import call
    poses, dR, dT, directions, img, pix = fwd_case(n_rays, n_imgs, 0)
    ok = (img >= 0) & (img < n_imgs) & (pix >= 0) & (pix < len(directions))
    zero = torch.zeros(n_imgs, 3, device=DEV)
    o = torch.full((n_rays, 3), float("nan"), device=DEV)
    d = torch.full((n_rays, 3), float("nan"), device=DEV)
    call("pose_rays_fwd", G(poses), zero, zero, G(directions), G(img), G(pix), n_imgs, len(directions), n_rays, o, d)
    P, D = torch.from_numpy(poses)[img[ok]], torch.from_numpy(directions)[pix[ok]]
    want_d = (P[:, :, 0] * D[:, 0:1] + P[:, :, 1] * D[:, 1:2]) + P[:, :, 2] * D[:, 2:3]
    assert torch.equal(o.cpu()[ok], P[:, :, 3])
    assert torch.equal(d.cpu()[ok], want_d)
    assert not o.cpu()[~ok].any() and not d.cpu()[~ok].any()


# ---------------------------------------------------------------------------- backward
BWD_PATTERNS = ("one_image", "random", "sorted", "out_of_range")
BWD_COMBOS = tuple((p, w) for p in BWD_PATTERNS for w in (True, False))
# the forward's six, and one on either side of the kernel's switch between the series and the closed form of a', b' (0.25)
BWD_ANGLES = pr.ANGLES + (0.2, 0.3)


def bwd_angle(n_rays, n_imgs, combo):
    """the eight (pattern, g_dir or not) launches of a size carry the eight |v|, one each; the pairing rotates with the size,
    so that over the 15 sizes every pattern meets every |v|"""
    return BWD_ANGLES[(combo + 3 * N_RAYS.index(n_rays) + N_IMGS.index(n_imgs)) % len(BWD_ANGLES)]


def bwd_case(n_rays, n_imgs, pattern, with_dir):
    """every image carries the SAME |v| (random axes): a launch is one |v| class"""
    angle = bwd_angle(n_rays, n_imgs, BWD_COMBOS.index((pattern, with_dir)))
    poses, dR, dT, directions = pr.make_cameras(n_imgs, 77 + n_imgs, (angle,))
    rays_a, n = pr.make_segments(n_rays, 300 + n_rays)
    g = np.random.default_rng(31 * n_rays + n_imgs + len(pattern))
    img = pr.index_patterns(n_rays, n_imgs, 5 * n_rays + n_imgs)[pattern]
    pix = g.integers(0, len(directions), n_rays).astype(np.int64)
    if pattern == "out_of_range" and n_rays >= 7:
        pix[1], pix[4] = len(directions), -3
    g_x = g.standard_normal((n, 3)).astype(np.float32)
    g_dir = g.standard_normal((n, 3)).astype(np.float32) if with_dir else None
    ts = g.uniform(0.05, 3.0, n).astype(np.float32)
    return poses, dR, dT, directions, img, pix, rays_a, ts, g_x, g_dir


@pytest.fixture(scope="module")
def bwd_family():
    """{(n_rays, n_imgs, pattern, with_dir): (inputs, float64 result, (yardstick of g_dR, of g_dT) of THIS case)}"""
    assert len(BWD_COMBOS) == len(BWD_ANGLES)
    cases, met = {}, set()
    for n_rays in N_RAYS:
        for n_imgs in N_IMGS:
            for k, (pattern, with_dir) in enumerate(BWD_COMBOS):
                c = bwd_case(n_rays, n_imgs, pattern, with_dir)
                want = pr.pose_grads(*c, torch.float64)
                f32 = pr.pose_grads(*c, torch.float32)
                cases[(n_rays, n_imgs, pattern, with_dir)] = (c, want, tuple(pr.rel_err(f32[j], want[j])[0] for j in range(2)))
                met.add((pattern, bwd_angle(n_rays, n_imgs, k)))
    assert len(met) == len(BWD_PATTERNS) * len(BWD_ANGLES)
    return cases


@pytest.mark.parametrize("n_imgs", N_IMGS)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_backward_against_float64(ngp, bwd_family, n_rays, n_imgs):
    from ngp_amd._lib import call
    failed = []
    for k, (pattern, with_dir) in enumerate(BWD_COMBOS):
        (poses, dR, dT, directions, img, pix, rays_a, ts, g_x, g_dir), want, yard = bwd_family[(n_rays, n_imgs, pattern, with_dir)]
        n = len(ts)
        if n_rays >= 7:
            assert rays_a[:, 2].max() == 1024 and (rays_a[:, 2] == 0).any() and rays_a[:, 2].sum() + 5 == n
        out = torch.zeros(2, n_imgs + 2, 3, device=DEV)          # accumulated into: zeros, and two rows behind the table
        call("pose_rays_bwd", G(g_x), None if g_dir is None else G(g_dir), G(ts), G(rays_a), G(poses), G(dR), G(directions),
             G(img), G(pix), n_imgs, len(directions), n_rays, n, out[0], out[1])
        got = N(out)
        assert np.isfinite(got).all() and not got[:, n_imgs:].any()
        named = np.zeros(n_imgs, bool)
        for ray, s, c in rays_a:
            if c > 0 and 0 <= img[ray] < n_imgs and 0 <= pix[ray] < len(directions):
                named[img[ray]] = True
        assert not got[0, :n_imgs][~named].any() and not got[1, :n_imgs][~named].any(), (pattern, with_dir)
        if n_imgs == 40 and n_rays <= 7:
            assert (~named).any()
        if not named.any():                                    # (one ray, and its image out of range)
            assert not got.any() and not want[0].any() and not want[1].any()
            continue
        err = [pr.rel_err(got[j, :n_imgs], want[j]) for j in range(2)]
        assert err[0][1] > 0 and err[1][1] > 0
        print(f"pose_rays_bwd n_rays={n_rays} n_imgs={n_imgs} {pattern} g_dir={with_dir} |v|={bwd_angle(n_rays, n_imgs, k):.3g}: "
              f"g_dR kernel {err[0][0]:.3e} yardstick {yard[0]:.3e} (bar {4 * yard[0]:.3e}); "
              f"g_dT kernel {err[1][0]:.3e} yardstick {yard[1]:.3e} (bar {4 * yard[1]:.3e})")
        failed += [(name, pattern, with_dir, err[j][0], yard[j]) for j, name in enumerate(("g_dR", "g_dT"))
                   if not err[j][0] <= 4 * yard[j]]
        # accumulation: a second call doubles the result (to the last bits of the atomics' order)
        if pattern == "random" and with_dir:
            call("pose_rays_bwd", G(g_x), G(g_dir), G(ts), G(rays_a), G(poses), G(dR), G(directions), G(img), G(pix),
                 n_imgs, len(directions), n_rays, n, out[0], out[1])
            np.testing.assert_allclose(N(out), 2 * got, rtol=1e-4, atol=1e-4 * np.abs(got).max())
    assert not failed, failed


def test_ray_function_backward_is_the_sample_kernel_on_one_sample_segments(ngp):
    """PoseRefiner.rays as an autograd function: gradients of a random linear functional of (rays_o, rays_d) against
    float64 autograd through the restatement, at the whole-step bar of the project (3e-4 of the largest entry)"""
    from ngp_amd.pose import PoseRefiner
    poses, dR, dT, directions = pr.make_cameras(5, 91)
    ref = PoseRefiner(torch.from_numpy(poses), torch.from_numpy(directions)).to(DEV)
    with torch.no_grad():
        ref.dR.copy_(G(dR))
        ref.dT.copy_(G(dT))
    g = np.random.default_rng(92)
    img, pix = g.integers(0, 5, 333).astype(np.int64), g.integers(0, len(directions), 333).astype(np.int64)
    c_o, c_d = g.standard_normal((333, 3)).astype(np.float32), g.standard_normal((333, 3)).astype(np.float32)
    o, d = ref.rays(G(img), G(pix))
    want_o, want_d = fwd_restated((poses, dR, dT, directions, img, pix), torch.float64)
    np.testing.assert_allclose(N(o), want_o, rtol=0, atol=2e-6)
    np.testing.assert_allclose(N(d), want_d, rtol=0, atol=2e-6)
    ((o * G(c_o)).sum() + (d * G(c_d)).sum()).backward()
    r = np.arange(333, dtype=np.int64)
    want = pr.pose_grads(poses, dR, dT, directions, img, pix, np.stack([r, r, np.ones_like(r)], 1), np.zeros(333, np.float32),
                         c_o, c_d, torch.float64)
    for got, w in zip((ref.dR.grad, ref.dT.grad), want):
        assert pr.rel_err(N(got), w)[0] <= 3e-4


# ---------------------------------------------------------------------------- adjoint of the direction encoding
def sh_case(n, kind):
    g = np.random.default_rng(17 * n + len(kind))
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if kind == "axis":
        d = np.eye(3)[g.integers(0, 3, n)] * g.choice([-1.0, 1.0], (n, 1))
    elif kind == "tiny":                  # under the 1e-6 clamp of F.normalize, the zero vector among them
        d = d * g.uniform(0, 9e-7, (n, 1))
        d[::2] = 0
    elif kind == "lengths":
        d = d * np.exp(g.uniform(np.log(1e-3), np.log(1e3), (n, 1)))
    return d.astype(np.float32), g.standard_normal((n, 16)).astype(np.float32)


@pytest.fixture(scope="module")
def sh_family():
    """{(n, kind): (d, dL/dy, float64 result, yardstick of THIS case)}"""
    cases = {}
    for n in SH_N:
        for kind in SH_KINDS:
            d, dy = sh_case(n, kind)
            want = pr.sh_grads(d, dy, torch.float64)
            cases[(n, kind)] = (d, dy, want, pr.rel_err(pr.sh_grads(d, dy, torch.float32), want)[0])
    assert all(c[3] < 1e-6 for c in cases.values())
    return cases


@pytest.mark.parametrize("n", SH_N)
def test_sh_bwd_dirs_against_float64(ngp, sh_family, n):
    """the four kinds of directions are separate launches with a bar each: the gradient scales with 1 / |d| (1e6 under the
    clamp), and one bar over all of them would only see the shortest vectors"""
    from ngp_amd._lib import call
    failed = []
    for kind in SH_KINDS:
        d, dy, want, yard = sh_family[(n, kind)]
        ld = 16 if kind != "lengths" else 21                      # a row stride of its own
        dy_dev = torch.full((n, ld), float("nan"), device=DEV)
        dy_dev[:, :16] = G(dy)
        out = torch.full((n + 2, 3), float("nan"), device=DEV)
        call("sh_bwd_dirs", G(d), dy_dev, ld, n, out)
        assert torch.isnan(out[n:]).all()
        got = N(out[:n])
        assert np.isfinite(got).all()
        err, scale = pr.rel_err(got, want)
        print(f"sh_bwd_dirs n={n} {kind}: kernel {err:.3e} yardstick {yard:.3e} (bar {4 * yard:.3e}), largest |gradient| {scale:.3e}")
        assert scale > 0
        if not err <= 4 * yard:
            failed.append((kind, err, yard))
        if kind == "lengths":
            # row by row as well, each row against its own largest component: the short vectors do not hide the long ones
            row = np.abs(got - want).max(1) / np.abs(want).max(1)
            assert row.max() <= 1e-4, row.max()
    assert not failed, failed


def test_field_direction_gradient_against_a_float64_restatement(ngp):
    """dL/dd out of _FieldFn.backward (rgb_net's data gradient for the 16 SH columns, then ngp_sh_bwd_dirs) for a random
    linear functional of the colours, against autograd through a float64 torch restatement of the colour branch
    (direction encoding | colour features | ones-padding -> 128 ReLU -> 3 sigmoid, weights in tcnn's layout); the
    project's whole-step gradient bar, 3e-4 of the largest entry, and the other gradients of the node are unchanged by it"""
    torch.manual_seed(51)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    with torch.no_grad():
        model.rgb_net.params.mul_(3.0)                           # (colours that are not all 0.5)
    g = np.random.default_rng(52)
    n = 777
    x = G(g.uniform(-0.45, 0.45, (n, 3)).astype(np.float32))
    d_np = (g.standard_normal((n, 3)) * np.exp(g.uniform(-1, 1, (n, 1)))).astype(np.float32)
    c = G(g.standard_normal((n, 3)).astype(np.float32))
    out = {}
    for with_d in (False, True):
        d = G(d_np).requires_grad_(with_d)
        for p_ in model.parameters():
            p_.grad = None
        _, rgbs, _, _, _ = model(x, d)
        (rgbs * c).sum().backward()
        out[with_d] = (None if d.grad is None else N(d.grad), N(model.rgb_net.params.grad), N(model.rgb_encoder.params.grad), N(rgbs))
    assert out[False][0] is None
    assert np.array_equal(out[False][3], out[True][3])
    for k in (1, 2):          # (summed by float atomics: the same to their order's last bits)
        np.testing.assert_allclose(out[True][k], out[False][k], rtol=0, atol=1e-5 * np.abs(out[False][k]).max())
    Kp = model.rgb_net.padded_in
    with torch.no_grad():
        feat = model.rgb_encoder(((x - model.xyz_min) / (model.xyz_max - model.xyz_min)).contiguous()).double().cpu()
    P = model.rgb_net.params.detach().double().cpu()
    W1, W2 = P[:128 * Kp].view(128, Kp), P[128 * Kp:].view(-1, 128)[:3]
    dd = torch.from_numpy(d_np).double().requires_grad_(True)
    rgb_in = torch.cat([pr.dir_encoding(dd), feat, torch.ones(n, Kp - 144, dtype=torch.float64)], 1)
    rgb64 = torch.sigmoid(torch.relu(rgb_in @ W1.T) @ W2.T)
    np.testing.assert_allclose(out[True][3], rgb64.detach().numpy(), rtol=0, atol=2e-5)
    (rgb64 * c.double().cpu()).sum().backward()
    err, scale = pr.rel_err(out[True][0], dd.grad.numpy())
    print(f"field dL/dd: largest entry {scale:.3e}, error {err:.3e} of it")
    assert scale > 0 and err <= 3e-4


# ---------------------------------------------------------------------------- one trainer step against torch autograd
def _add_grid(model):
    Gs = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, Gs ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(Gs, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())


def _capture_instead_of_stepping(tr):
    """the trainer's optimizer step replaced by a snapshot of the gradients it would have consumed"""
    got = {}

    def capture():
        torch.cuda.synchronize()
        got["model"] = tr.flat_grad.clone()
        got["pose"] = tr.pose_grad.clone() if tr.pose_refiner is not None else None
        got["bound_step"] = tr._bound_step
        tr.global_step += 1
    tr.optimizer_step = capture
    return got


@pytest.mark.parametrize("recipe", ["default", "codes_and_mask"])
def test_one_step_against_torch_autograd(ngp, recipe):
    """3 images of 24 x 24, 200 rays, scale 0.5, dR ~ 0.02 rad, dT ~ 0.01.  Route A: NGPTrainer.step with a refiner (fused
    tail, ngp_pose_rays_bwd, ngp_sh_bwd_dirs).  Route B: rays from axisangle_to_R / get_rays with a graph, the samples of
    route A's march (the marcher fed the kernel's ray values), x = o[ray] + t d[ray] by torch indexing, model(xyzs, dirs),
    VolumeRenderer, NeRFLoss.  dR.grad, dT.grad and the model's gradients agree to 3e-4 of the largest entry."""
    from ngp_amd.custom_functions import VolumeRenderer
    from ngp_amd.datasets.ray_utils import axisangle_to_R, get_rays
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    full = recipe == "codes_and_mask"
    torch.manual_seed(71)
    model = (ngp.networks.NGP(scale=0.5, embed_a=True, embed_a_len=4) if full else ngp.networks.NGP(scale=0.5)).to(DEV)
    _add_grid(model)
    with torch.no_grad():
        # A field that varies SMOOTHLY in space: the four coarsest levels (cells of 1/16 to 1/37) at +-0.5, the finer ones 0.
        # With the tables at their initial +-1e-4 on all 16 levels dL/dx of a sample is the slope of the finest cells, random
        # from cell to cell: its sum over a camera cancels (measured: dT.grad 4e-6, the two routes 4e-8 apart), and the two
        # routes' sample positions, 1e-7 apart, lie in different cells here and there (measured with all levels at +-0.2: dR.grad
        # 3e-3 apart).  Either is the test's conditioning, not the chain's.
        model.xyz_net[2].bias.fill_(1.5)
        for enc in (model.xyz_encoder, model.rgb_encoder):
            off = int(enc.desc.offsets[4]) * int(enc.desc.n_features)
            enc.params[:off].mul_(5000.0)
            enc.params[off:].zero_()
    scene = LegoProxy(n_images=3, img_wh=(24, 24), device=DEV)
    ref = PoseRefiner(scene.poses, scene.directions).to(DEV)
    emb = torch.nn.Embedding(3, 4).to(DEV) if full else None
    msk = implicit_mask().to(DEV) if full else None
    tr = NGPTrainer(model, pose_refiner=ref, embedding_a=emb, msk_model=msk)
    assert tr.recipe.fused_loss and ref.dR.data_ptr() == tr.pose_param.data_ptr() and ref.dR.data_ptr() % 16 == 0
    assert ref.dT.data_ptr() % 16 == 0 and "dR" not in tr.names and not any("pose" in n for n in tr.names)
    gen = torch.Generator(device=DEV).manual_seed(72)
    with torch.no_grad():
        ref.dR.copy_(torch.randn(3, 3, device=DEV, generator=gen) * 0.02)
        ref.dT.copy_(torch.randn(3, 3, device=DEV, generator=gen) * 0.01)
    img, pix = scene.sample_batch(200, generator=gen)
    gt = torch.rand(200, 3, device=DEV, generator=gen)
    uvi = implicit_mask.uvi(torch.stack([pix // 24, pix % 24], -1), img, (24, 24), 3) if full else None
    got = _capture_instead_of_stepping(tr)
    loss_a, res = tr.step(None, None, gt, img_idxs=img, pix_idxs=pix, uvi=uvi)
    assert got["bound_step"] is False and "_loss_terms" not in res and res["rgb"].shape == (200, 3)
    n = int(res["total_samples"])
    assert n > 2000 and res["xyzs"].requires_grad
    grads_a = N(got["model"])
    pose_a = N(got["pose"])
    n6 = ref.dR.numel()
    seg = (n6 + 3) // 4 * 4
    dR_a, dT_a = pose_a[:n6].reshape(3, 3), pose_a[seg:seg + n6].reshape(3, 3)

    # route B
    tr.flat_grad.zero_()
    tr.pose_grad.zero_()
    dR_t, dT_t = ref.dR.detach().clone().requires_grad_(True), ref.dT.detach().clone().requires_grad_(True)
    c2w = torch.cat([axisangle_to_R(dR_t[img]) @ scene.poses[img][..., :3], (scene.poses[img][..., 3] + dT_t[img])[..., None]], -1)
    o_t, d_t = get_rays(scene.directions[pix], c2w)
    with torch.no_grad():
        o_k, d_k = ref.rays(img, pix)
    np.testing.assert_allclose(N(o_k), N(o_t), rtol=0, atol=1e-6)
    np.testing.assert_allclose(N(d_k), N(d_t), rtol=0, atol=1e-6)
    rays_a, ts, deltas = res["rays_a"], res["ts"], res["deltas"]
    ray_of = torch.repeat_interleave(rays_a[:, 0], rays_a[:, 2])
    assert ray_of.shape[0] == n
    xyzs = o_t[ray_of] + ts[:, None] * d_t[ray_of]
    dirs = d_t[ray_of]
    np.testing.assert_allclose(N(xyzs), N(res["xyzs"]), rtol=0, atol=2e-6)
    kw = {}
    if full:
        kw["embedding_a"] = torch.repeat_interleave(emb.weight[img][rays_a[:, 0]], rays_a[:, 2], 0)
    sig, rgbs, _, nrm_pred, sems = model(xyzs, dirs, **kw)
    out = {"deltas": deltas, "ts": ts, "rays_a": rays_a}
    (_, out["opacity"], out["depth"], out["rgb"], _, _, out["ws"]) = VolumeRenderer.apply(
        sig.contiguous(), rgbs.contiguous(), nrm_pred.contiguous(), sems.contiguous(), deltas, ts, rays_a, 1e-4, 7)
    loss_fn = NeRFLoss()
    lkw = {}
    if full:
        lkw = dict(embed_msk=True, mask=msk(uvi), step=0)
    loss_b = sum(v.mean() for v in loss_fn(out, {"rgb": gt}, **lkw).values())
    loss_b.backward()
    torch.cuda.synchronize()
    print(f"[{recipe}] loss: trainer {float(loss_a):.6f}, torch route {float(loss_b.detach()):.6f}; {n} samples")
    np.testing.assert_allclose(float(loss_a), float(loss_b.detach()), rtol=1e-4)
    for name, a, b in (("dR", dR_a, N(dR_t.grad)), ("dT", dT_a, N(dT_t.grad)), ("model", grads_a, N(tr.flat_grad))):
        scale, err = np.abs(b).max(), np.abs(a - b).max()
        print(f"[{recipe}] {name}: largest entry {scale:.3e}, max difference {err:.3e} ({err / scale:.2e} of it)")
        assert scale > 0 and err <= 3e-4 * scale, (name, err, scale)
    for name, (off, numel) in tr.slices.items():      # every parameter tensor by itself as well
        a, b = grads_a[off:off + numel], N(tr.flat_grad[off:off + numel])
        scale = np.abs(b).max()
        if name.startswith(("semantic_header", "norm_pred_header")):
            assert scale == 0 and not a.any()
            continue
        assert scale > 0 and np.abs(a - b).max() <= 3e-4 * scale, (name, np.abs(a - b).max(), scale)


# ---------------------------------------------------------------------------- registration on the proxy scene
REG_STEPS_MAX, REG_POSE_STEPS, REG_POSE_LR = 1500, 300, 1e-3


def test_registration_on_the_proxy_scene(ngp):
    """8 cameras of 64 x 64 (2 more held out), scale 0.5.  Phase 1: true poses until the held-out PSNR exceeds 20 dB (checked
    every 100 steps, REG_STEPS_MAX at the most).  Phase 2: the model's lr = 0, cameras 0..3 translated by N(0, 0.02^2) per
    axis and rotated by 0.5 degrees, REG_POSE_STEPS steps at pose_lr = REG_POSE_LR (Adam moves an entry by at most about
    pose_lr a step: 0.3 in all, ten times the perturbation, with a jitter of the order of pose_lr, a twentieth of it).
    Required: the median translation error of the perturbed cameras ends below its starting value, and the unperturbed
    cameras' largest error stays below the perturbed cameras' starting median."""
    from ngp_amd.metrics import psnr
    from ngp_amd.pose import PoseRefiner, perturb_poses
    from ngp_amd.rendering import render
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    torch.manual_seed(81)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    _add_grid(model)
    scene = LegoProxy(n_images=10, img_wh=(64, 64), device=DEV)
    n_pix = 64 * 64
    all_img = torch.arange(10, device=DEV).repeat_interleave(n_pix)
    all_pix = torch.arange(n_pix, device=DEV).repeat(10)
    o_all, d_all = scene.rays(all_img, all_pix)
    gt_all = scene.ground_truth(o_all, d_all, n_quad=256)[0].reshape(10, n_pix, 3)
    held = slice(8 * n_pix, 10 * n_pix)
    gen = torch.Generator(device=DEV).manual_seed(82)

    def batch():
        img = torch.randint(8, (2048,), device=DEV, generator=gen)
        pix = torch.randint(n_pix, (2048,), device=DEV, generator=gen)
        return img, pix, gt_all[img, pix].contiguous()

    def held_out_psnr():
        with torch.no_grad():
            res = render(model, o_all[held].contiguous(), d_all[held].contiguous(), test_time=True)
        return float(psnr(res["rgb"], gt_all[8:].reshape(-1, 3)))

    tr = NGPTrainer(model, lr=1e-2)
    steps, quality = 0, 0.0
    while steps < REG_STEPS_MAX and quality <= 20.0:
        for _ in range(100):
            img, pix, gt = batch()
            tr.step(*scene.rays(img, pix), gt)
        steps += 100
        tr.wait()
        quality = held_out_psnr()
    print(f"registration: held-out PSNR {quality:.2f} dB after {steps} steps with the true poses")
    assert quality > 20.0
    tr.wait()
    torch.cuda.synchronize()

    truth = scene.poses[:8].clone()
    start = truth.clone()
    start[:4] = perturb_poses(truth[:4], 0.02, 0.5, seed=83)
    ref = PoseRefiner(start, scene.directions).to(DEV)
    tr2 = NGPTrainer(model, lr=0.0, pose_refiner=ref, pose_lr=REG_POSE_LR)
    before = tr2.flat_param.clone()

    def t_err():
        return (ref.refined_poses().detach()[..., 3] - truth[..., 3]).norm(dim=-1)

    e0 = t_err()
    for _ in range(REG_POSE_STEPS):
        img, pix, gt = batch()
        tr2.step(None, None, gt, img_idxs=img, pix_idxs=pix)
    tr2.wait()
    torch.cuda.synchronize()
    e1 = t_err()
    assert torch.equal(tr2.flat_param, before)                   # lr = 0: the field did not move
    assert torch.isfinite(ref.dR).all() and torch.isfinite(ref.dT).all() and ref.dR.abs().sum() > 0
    m0, m1, drift = float(e0[:4].median()), float(e1[:4].median()), float(e1[4:].max())
    print(f"registration: {REG_POSE_STEPS} steps at pose_lr {REG_POSE_LR}: median translation error of the perturbed cameras "
          f"{m0:.5f} -> {m1:.5f} (ratio {m1 / m0:.3f}); largest error of the unperturbed cameras {drift:.5f}; "
          f"per camera {[round(float(v), 5) for v in e0]} -> {[round(float(v), 5) for v in e1]}")
    assert m1 < m0
    assert drift < m0


# ---------------------------------------------------------------------------- the default path, and the argument checks
def test_default_path_is_untouched_and_the_argument_checks(ngp, tmp_path):
    from ngp_amd import ckpt
    from ngp_amd.networks import _FieldFn
    from ngp_amd.pose import PoseRefiner
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    _lib = ngp._lib
    torch.manual_seed(91)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    _add_grid(model)
    scene = LegoProxy(n_images=4, img_wh=(32, 32), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(92)
    img, pix = scene.sample_batch(512, generator=gen)
    gt = torch.rand(512, 3, device=DEV, generator=gen)
    o, d = scene.rays(img, pix)

    # without a refiner: the field returns None at the d (and x) position, no pose kernel is launched, the clip is bounded
    seen = []
    orig = _FieldFn.backward

    def spy(ctx, *grads):
        out = orig(ctx, *grads)
        seen.append((out[1], out[2]))
        return out
    _FieldFn.backward = staticmethod(spy)
    _lib.CAPTURE = {"sh_bwd_dirs": [], "pose_rays_bwd": [], "pose_rays_fwd": [], "clip_decide_rest": []}
    try:
        tr = NGPTrainer(model, lr=1e-2)
        got = _capture_instead_of_stepping(tr)
        tr.step(o, d, gt)
        assert got["bound_step"] is True and tr.norm_bound
        del tr.optimizer_step                                    # the real one again
        tr.step(o, d, gt)
        tr.wait()
        assert len(seen) == 2 and all(a is None and b is None for a, b in seen)
        assert len(_lib.CAPTURE["clip_decide_rest"]) == 1
        assert not _lib.CAPTURE["sh_bwd_dirs"] and not _lib.CAPTURE["pose_rays_bwd"] and not _lib.CAPTURE["pose_rays_fwd"]
        with pytest.raises(ValueError, match="pose_refiner"):
            tr.step(o, d, gt, pix_idxs=pix)

        # with one: the argument checks, one step, and the checkpoint round trip
        ref = PoseRefiner(scene.poses, scene.directions).to(DEV)
        with pytest.raises(ValueError, match="one rank"):
            NGPTrainer(model, pose_refiner=ref, force_sharded=True)
        tr2 = NGPTrainer(model, lr=1e-2, pose_refiner=ref, pose_lr=1e-4)
        with pytest.raises(ValueError, match="forms the rays itself"):
            tr2.step(o, d, gt, img_idxs=img, pix_idxs=pix)
        with pytest.raises(ValueError, match="forms the rays itself"):
            tr2.step(None, None, gt, img_idxs=img, pix_idxs=pix, next_rays=(o, d))
        with pytest.raises(ValueError, match="img_idxs= and pix_idxs="):
            tr2.step(None, None, gt, img_idxs=img)
        # only the field's dL/dx and dL/dd feed the pose gradient: recipes whose loss reaches the rays another way (the Ro
        # term through dirs, a skybox through rays_d, per-step terms off the fused tail) are refused, and leave the model alone
        with pytest.raises(ValueError, match="fused render \\+ loss tail"):
            NGPTrainer(model, pose_refiner=ref, loss_kwargs={"normal_ref": True})
        assert model.differentiable_normals is False
        with pytest.raises(ValueError, match="fused render \\+ loss tail"):
            NGPTrainer(model, pose_refiner=ref, render_kwargs={"use_skybox": True})
        with pytest.raises(ValueError, match="fused render \\+ loss tail"):
            tr2.step(None, None, gt, img_idxs=img, pix_idxs=pix, target={"depth": gt[:, 0]})
        with pytest.raises(ValueError, match="fused render \\+ loss tail"):
            tr2.step(None, None, gt, img_idxs=img, pix_idxs=pix, step=3)
        seen.clear()
        for _ in range(3):
            tr2.step(None, None, gt, img_idxs=img, pix_idxs=pix)
        tr2.wait()
        torch.cuda.synchronize()
        assert len(seen) == 3 and all(a is not None and b is not None for a, b in seen)
        assert len(_lib.CAPTURE["sh_bwd_dirs"]) == len(_lib.CAPTURE["pose_rays_bwd"]) == len(_lib.CAPTURE["pose_rays_fwd"]) == 3
        assert len(_lib.CAPTURE["clip_decide_rest"]) == 1        # pose steps take the exact norm
    finally:
        _FieldFn.backward = staticmethod(orig)
        _lib.CAPTURE = None
    assert tr2.pose_steps == 3 and not tr2.pose_grad.any()       # cleared by the Adam launch
    assert ref.dR.abs().max() > 0 and ref.dT.abs().max() > 0
    # Adam at a constant 1e-4: no entry has moved further than 3 steps of it
    assert float(torch.maximum(ref.dR.detach().abs().max(), ref.dT.detach().abs().max())) <= 3.01e-4
    path = str(tmp_path / "poses.ckpt")
    ckpt.save_ckpt(model, path, pose_refiner=ref)
    other = PoseRefiner(torch.zeros_like(scene.poses), scene.directions).to(DEV)
    ckpt.load_poses(other, path)
    for k in ("dR", "dT", "poses"):
        assert torch.equal(other.state_dict()[k], ref.state_dict()[k]), k
    assert torch.equal(other.poses, scene.poses)
    ckpt.load_ckpt(model, path)                                  # the model's loader ignores the pose keys


def test_tool_refines_perturbed_poses_on_the_proxy_scene(ngp, tmp_path):
    """tools/train_dataset.py --optimize_ext --perturb_poses on the proxy scene at 64 x 64, 40 steps: the batches without
    ray tensors, the pose errors of the JSON line and the checkpoint's pose keys"""
    ckpt_path, scene_dir = str(tmp_path / "poses.ckpt"), str(tmp_path / "scene")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py"), "--make_proxy", scene_dir,
                          "--downsample", "0.08", "--num_epochs", "1", "--steps_per_epoch", "40", "--batch_size", "1024",
                          "--optimize_ext", "--pose_lr", "1e-4", "--perturb_poses", "0.02", "0.5", "--ckpt_path", ckpt_path],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 40 and line["img_wh"] == [64, 64] and np.isfinite(line["test_psnr_mean"])
    assert line["pose_lr"] == 1e-4
    # N(0, 0.02^2) per axis: a mean length of 0.02 sqrt(8 / pi) = 0.032 over 100 cameras; 0.5 degrees each
    assert 0.025 < line["pose_t_err_before"] < 0.04 and abs(line["pose_rot_err_deg_before"] - 0.5) < 1e-2
    # Adam at a constant 1e-4 moves an entry by at most about 1e-4 a step: 40 steps change the mean errors by < 0.01 / 0.5 deg
    assert abs(line["pose_t_err_after"] - line["pose_t_err_before"]) < 0.01
    assert abs(line["pose_rot_err_deg_after"] - line["pose_rot_err_deg_before"]) < 0.5
    assert line["pose_t_err_after"] != line["pose_t_err_before"]
    sd = torch.load(ckpt_path, weights_only=True)["state_dict"]
    assert tuple(sd["dR"].shape) == tuple(sd["dT"].shape) == (100, 3) and tuple(sd["poses"].shape) == (100, 3, 4)
    assert torch.isfinite(sd["dR"]).all() and torch.isfinite(sd["dT"]).all()
    moved = sd["dT"].abs().amax(1) > 0
    assert moved.any() and torch.equal(moved, sd["dR"].abs().amax(1) > 0)   # a camera's rotation and translation move together
    assert float(torch.maximum(sd["dR"].abs().max(), sd["dT"].abs().max())) <= 40 * 1.01e-4
