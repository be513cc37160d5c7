"""ngp_density_field_fwd (the training forward's density path in one launch) against the four launches it replaces
(ngp_grid_fwd -> ngp_mlp2_fwd_dact -> ngp_mlp_bwd_input -> ngp_grid_bwd_input) on the same table, weights and points:
feat, a1, sigma and dfeat bit for bit, d sigma / dx within 128 ulps of each row's largest component.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from helpers import rng

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOFTPLUS = 3


def _layout(ngp, log2_T):
    desc = ngp._lib.GridDesc()
    b = float(np.exp(np.log(2048 * 0.5 / 16) / 15))
    size = ngp._lib.call_host("grid_layout", 16, 8, log2_T, 16, b, desc)
    assert size > 0
    return desc, int(size)


def _points(n, desc, seed):
    """uniform points, runs of ray-ordered samples (consecutive samples in one cell: the run-leader path), points on
    the cell faces and corners of random levels, and the faces of the unit cube"""
    g = rng(seed)
    x = g.random((n, 3)).astype(np.float32)
    if n >= 8:
        k = n // 4   # ray-ordered runs: 32 rays with small steps
        o = g.random((32, 3))
        d = g.normal(size=(32, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        t = np.arange((k + 31) // 32) * (np.sqrt(3) / 1024)
        run = (o[:, None, :] + t[None, :, None] * d[:, None, :]).reshape(-1, 3)[:k]
        x[:k] = np.clip(run, 0.0, 1.0).astype(np.float32)
    m = max(n // 4, 1)
    sel = g.choice(n, size=m, replace=False)
    lv = g.integers(0, 16, m)
    scale = np.array([desc.scale[i] for i in range(16)], np.float32)[lv]
    axis = g.integers(0, 3, m)
    cell = np.floor(x[sel, axis] * scale + 0.5)
    x[sel, axis] = ((cell - 0.5) / scale).astype(np.float32)      # on a face of level lv's cells
    corner = sel[: m // 4]
    for a in range(3):
        c = np.floor(x[corner, a] * scale[: m // 4] + 0.5)
        x[corner, a] = ((c - 0.5) / scale[: m // 4]).astype(np.float32)
    x[sel[-1]] = [0.0, 1.0, 0.5]
    return np.clip(x, 0.0, 1.0).astype(np.float32)


def _setup(ngp, n, log2_T=19, seed=0):
    desc, size = _layout(ngp, log2_T)
    g = torch.Generator(device=DEV).manual_seed(seed)
    table = (torch.rand(size, device=DEV, generator=g) * 2 - 1) * 0.3
    W1 = torch.randn(128, 128, device=DEV, generator=g) * 0.1
    b1 = torch.randn(128, device=DEV, generator=g) * 0.1
    W2 = torch.randn(1, 128, device=DEV, generator=g) * 0.1
    b2 = torch.randn(1, device=DEV, generator=g) * 0.1
    x = torch.from_numpy(_points(n, desc, seed + 1)).to(DEV)
    return desc, table, x, W1, b1, W2, b2


def _four_launches(call, desc, table, x, W1, b1, W2, b2):
    n = x.shape[0]
    feat, a1, dfeat = (torch.empty(n, 128, device=DEV) for _ in range(3))
    sig, dz2, grads = torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV), torch.empty(n, 3, device=DEV)
    call("grid_fwd", desc, table, x, n, feat, 128)
    call("mlp2_fwd_dact", feat, 128, W1, 128, b1, SOFTPLUS, W2, 128, b2, SOFTPLUS, n, 128, 128, 1, a1, 128, sig, 1, dz2)
    call("mlp_bwd_input", dz2, 1, W2, 128, a1, 128, SOFTPLUS, W1, 128, n, 128, 128, 1, dfeat, 128, 0)
    call("grid_bwd_input", desc, table, x, dfeat, 128, n, grads)
    return feat, a1, sig, dfeat, grads


def _fused(call, desc, table, x, W1, b1, W2, b2):
    n = x.shape[0]
    feat, a1, dfeat = (torch.full((n, 128), float("nan"), device=DEV) for _ in range(3))
    sig, grads = torch.full((n, 1), float("nan"), device=DEV), torch.full((n, 3), float("nan"), device=DEV)
    call("density_field_fwd", desc, table, x, n, W1, b1, W2, b2, feat, a1, sig, dfeat, grads)
    return feat, a1, sig, dfeat, grads


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 450_017])
@pytest.mark.parametrize("log2_T", [19, 14])
def test_density_field_fwd_bitwise_equal_to_four_launches(ngp, n, log2_T):
    from ngp_amd._lib import call
    args = _setup(ngp, n, log2_T, seed=n % 97)
    ref = _four_launches(call, *args)
    out = _fused(call, *args)
    torch.cuda.synchronize()
    for name, r, o in zip(("feat", "a1", "sig", "dfeat"), ref, out):
        assert torch.equal(r, o), f"{name} differs (n={n}, log2_T={log2_T}): max |d| {(r - o).abs().max().item()}"
    _grads_close(ref[4], out[4])


def _grads_close(r, o):
    """d sigma / dx: the same per-level expression, contracted into FMAs differently by the compiler in the two kernels.
    The 16 level terms (each up to the level's scale, ~1000) cancel in the sum, so a component near zero can differ by
    many of its own ulps; the bound is in ulps of the row's largest component: 128 (measured worst on 450 k samples:
    63, median of the differing components 1 ulp of their own)"""
    assert torch.isfinite(o).all()
    ulp = torch.ldexp(torch.ones_like(r[:, :1]), torch.frexp(r.abs().amax(dim=1, keepdim=True))[1] - 24)
    d_ulps = ((r - o).abs() / ulp).max().item()
    assert d_ulps <= 128, f"grads differ by {d_ulps} ulps of the row's largest component"


def test_density_field_fwd_without_biases(ngp):
    from ngp_amd._lib import call
    desc, table, x, W1, _, W2, _ = _setup(ngp, 777, seed=3)
    ref = _four_launches(call, desc, table, x, W1, None, W2, None)
    out = _fused(call, desc, table, x, W1, None, W2, None)
    for r, o in zip(ref[:4], out[:4]):
        assert torch.equal(r, o)
    _grads_close(ref[4], out[4])


def test_density_field_fwd_rejects_without_launch(ngp):
    """misaligned outputs and layouts other than 16 levels of F = 8 return NGP_EINVAL, and nothing is written"""
    from ngp_amd._lib import load
    lib = load()
    desc, table, x, W1, b1, W2, b2 = _setup(ngp, 64, seed=5)
    n = 63
    buf = torch.zeros(n * 128 + 1, device=DEV)
    good = [torch.zeros(n, 128, device=DEV) for _ in range(3)]
    sig, grads = torch.zeros(n, device=DEV), torch.zeros(n, 3, device=DEV)
    import ctypes as C

    def run(desc_, W1_, feat_):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return lib.ngp_density_field_fwd(C.addressof(desc_), p(table), p(x), n, p(W1_), p(b1), p(W2), p(b2), p(feat_),
                                         p(good[1]), p(sig), p(good[2]), p(grads), None)
    assert run(desc, W1, buf[1:]) == -22                       # feat not 16-byte aligned
    w1_buf = torch.zeros(128 * 128 + 1, device=DEV)
    assert run(desc, w1_buf[1:], good[0]) == -22               # W1 not 16-byte aligned
    other = ngp._lib.GridDesc()
    assert ngp._lib.call_host("grid_layout", 8, 8, 19, 16, 1.5, other) > 0
    assert run(other, W1, good[0]) == -22                      # 8 levels
    torch.cuda.synchronize()
    assert not buf.any() and not any(t.any() for t in good) and not sig.any() and not grads.any()


def _trainer_model(ngp):
    torch.manual_seed(7)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    with torch.no_grad():
        model.xyz_encoder.params.uniform_(-0.3, 0.3)
        model.rgb_encoder.params.uniform_(-0.3, 0.3)
        model.xyz_net[2].bias.fill_(1.0)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    c = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", c.reshape(-1, 3).contiguous())
    model.grid_rng = torch.Generator(device=DEV).manual_seed(11)
    return model


def test_trainer_step_matches_four_launch_route(ngp, monkeypatch):
    """one NGPTrainer.step through the fused density path against the same step on the four launches: same loss and
    parameters up to the run-to-run spread of the backward's float atomics"""
    from ngp_amd import networks
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer

    def one_step(fused):
        used = []
        real_call = networks.call

        def recording(name, *a):
            used.append(name)
            return real_call(name, *a)
        monkeypatch.setattr(networks, "call", recording)
        if not fused:
            monkeypatch.setattr(networks, "_density_fused_ok", lambda *a: False)
        model = _trainer_model(ngp)
        scene = LegoProxy(n_images=4, img_wh=(100, 100), device=DEV)
        tr = NGPTrainer(model, lr=1e-2)
        gen = torch.Generator(device=DEV).manual_seed(2)
        img, pix = scene.sample_batch(2048, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=64)
        loss, res = tr.step(o, d, gt)
        tr.wait()
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert ("density_field_fwd" in used) == fused
        return float(loss), int(res["total_samples"]), tr.flat_param.detach().clone()

    loss_f, n_f, p_f = one_step(True)
    loss_r, n_r, p_r = one_step(False)
    assert n_f == n_r and n_f > 1000
    assert abs(loss_f - loss_r) <= 7e-7 * max(1.0, abs(loss_r))
    assert (p_f - p_r).abs().max().item() <= 7e-7
