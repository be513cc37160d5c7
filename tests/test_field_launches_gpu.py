"""Every launch networks.py makes for one forward and backward of the field's autograd node (_FieldFn), written out:
entry point, stream role, every scalar argument, and of every tensor argument its storage offset and strides (which is
what tells the W1[:, 16:] column window and the second-layer slices of the flat tcnn parameters apart).  The lists below
pin launch identity, not values: the weight products combine with fp32 atomics and are not reproducible bit for bit.
The first six cases and EXPECTED_STEP were recorded from the node before its MLP plumbing was folded into one
description.  The other twelve (second_order, second_order_v_only, ray_codes, ray_codes_gaps, classes9,
density_four_launches, normal_only, semantic_only, normal_only_codes, sigma_only, collective_first, input_grads_codes) and
EXPECTED_STEP_NORMAL_REF were recorded on an MI355X from the node as it stood before its forward and backward were split
into named stages (3fd6ac8: one 125-line forward, one 200-line backward), each case in a process of its own: the routes
a restructuring disturbs most easily and no list reached.  Where a list cannot see the difference (a fill, zeros
against empty) the case also asserts values.
n = 257 samples: eight full 32-row tiles of one workgroup and one ragged row, the smallest size that reaches both the
full-tile and the tail code of the streaming kernels.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from helpers import rng
from test_gpu_parity import DEV, N, T, _grid_model, _lego_batch, _make_model, _record_step_launches

pytestmark = pytest.mark.gpu

N_SAMPLES = 257
_ROLES = ("colour", "scatter", "heads")
_TORCH_STREAM_POOL = 32   # (c10: kStreamsPerPool) streams per device and priority, handed out round-robin


def t(offset, *stride):
    """a tensor argument: storage offset and strides, in elements"""
    return ("t", offset, stride)


def _describe(a):
    if isinstance(a, torch.Tensor):
        return t(a.storage_offset(), *a.stride())
    if a is None or isinstance(a, (int, float)):
        return a
    return "desc"    # a grid layout (ngp_grid_desc)


def _model(ngp, classes=7, embed_a=False):
    if classes == 7:
        return _make_model(ngp, embed_a=embed_a)
    torch.manual_seed(5)
    model = ngp.networks.NGP(scale=0.5, classes=classes).to(DEV)
    with torch.no_grad():
        model.xyz_encoder.params.uniform_(-0.3, 0.3)
        model.rgb_encoder.params.uniform_(-0.3, 0.3)
    return model


def _ray_codes(ngp, g, gaps):
    """RayCodes over a 6-image table bound to 5 segments of unequal length: all 257 samples (and the flag that says so),
    or with samples 100..119 in no segment"""
    starts, counts = ((0, 40, 120, 170, 217), (40, 60, 50, 47, 40)) if gaps else ((0, 10, 100, 157, 194), (10, 90, 57, 37, 63))
    rays_a = torch.tensor([(r, s, c) for r, (s, c) in enumerate(zip(starts, counts))], dtype=torch.int64, device=DEV)
    assert int(rays_a[:, 2].sum()) == N_SAMPLES - (20 if gaps else 0) and int(rays_a[-1, 1:].sum()) == N_SAMPLES
    if not gaps:
        rays_a._ngp_full_cover = True
    weight = T(g.normal(size=(6, 8)).astype(np.float32)).requires_grad_(True)
    return ngp.appearance.RayCodes(weight, torch.tensor([4, 0, 5, 2, 2]), rays_a)


def record_field(ngp, classes=7, embed_a=False, seeded=("sigma", "rgb"), input_grads=False, prepare=None):
    """one _FieldFn forward and backward on a fresh model -> (launches, model, inputs, output weights, outputs)
    embed_a: True (a (n, 8) tensor of codes), "ray_codes" or "ray_codes_gaps" (_ray_codes); prepare(model) runs before
    the forward; seeded may name "dsigma_dx", the node's third output"""
    networks = ngp.networks
    model = _model(ngp, classes, bool(embed_a))
    if prepare is not None:
        prepare(model)
    g = rng(230)
    n = N_SAMPLES
    x = T(((g.random((n, 3)) - 0.5) * 0.98).astype(np.float32)).requires_grad_(input_grads)
    d = T(g.normal(size=(n, 3)).astype(np.float32)).requires_grad_(input_grads)
    kw = {}
    if embed_a is True:
        kw = {"embedding_a": T(g.normal(size=(n, 8)).astype(np.float32)).requires_grad_(True)}
    elif embed_a:
        kw = {"embedding_a": _ray_codes(ngp, g, gaps=embed_a == "ray_codes_gaps")}
    ws = dict(zip(("sigma", "rgb", "normal", "semantic", "dsigma_dx"),
                  (T(g.normal(size=s).astype(np.float32)) for s in ((n,), (n, 3), (n, 3), (n, classes), (n, 3)))))
    launches = []
    real_call = networks.call

    def recording_call(name, *args):
        launches.append((name, torch.cuda.current_stream().cuda_stream, tuple(_describe(a) for a in args)))
        return real_call(name, *args)
    caller = torch.cuda.current_stream().cuda_stream
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(networks, "call", recording_call)
        sig, rgb, dsig, nrm, sem = model._field(x, d, kw)
        outs = {"sigma": sig, "rgb": rgb, "normal": nrm, "semantic": sem, "dsigma_dx": dsig}
        sum((outs[k] * ws[k]).sum() for k in seeded).backward()
    torch.cuda.synchronize()
    roles = {networks._stream(role, DEV).cuda_stream: role for role in _ROLES}
    roles[caller] = "caller"
    assert len(roles) == 4 and {st for _, st, _ in launches} <= set(roles)
    return [(name, roles[st], args) for name, st, args in launches], model, (x, d, kw), ws, outs


def _assert_launches(got, want):
    assert [(name, role) for name, role, _ in got] == [(name, role) for name, role, _ in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} ({g[0]})"


def _assert_head_and_table_gradients(model, x, d, ws, classes, seeded=("rgb", "normal", "semantic"),
                                     names=("semantic_header", "rgb_encoder")):
    """the semantic head's and the colour table's gradient (`names`) against the fp64 restatement of the field that
    test_field_backward_matches_torch_fp64 uses (on the node's raw outputs, those of `seeded`), at that test's tolerance"""
    D = torch.float64
    F_ = torch.nn.functional
    params = [getattr(model, name).params for name in names]
    fused = [p.grad for p in params]
    xn = ((x - model.xyz_min) / (model.xyz_max - model.xyz_min)).contiguous()
    frgb = model.rgb_encoder(xn).to(D)
    rloss = 0.0
    if "rgb" in seeded:
        sh = model.dir_encoder((F_.normalize(d, dim=-1) + 1) / 2).to(D)
        inp = torch.cat([sh, frgb], 1)
        net = model.rgb_net
        rrgb = torch.sigmoid(torch.relu(inp @ net.layer_weight(0).to(D).T) @ net.layer_weight(1).to(D).T)[:, :3]
        rloss = rloss + (rrgb * ws["rgb"]).sum()
    for key, head, width in (("normal", model.norm_pred_header, 3), ("semantic", model.semantic_header, classes)):
        if key in seeded:
            h = torch.relu(frgb @ head.layer_weight(0).to(D).T) @ head.layer_weight(1).to(D).T
            rloss = rloss + (h[:, :width] * ws[key]).sum()
    ref = torch.autograd.grad(rloss, params)
    for name, a, b in zip(names, fused, ref):
        a, b = N(a).astype(np.float64), N(b).astype(np.float64)
        scale = np.abs(b).max() + 1e-12
        assert scale > 1e-6, name
        assert np.abs(a - b).max() <= 2e-4 * scale, (name, np.abs(a - b).max(), scale)


def _second_order(model):
    model.second_order_normals = True


def _four_launches(model):
    model.xyz_encoder._density_fused_layout = False


def _collective_first(model):
    model.rgb_encoder.grad_ready_is_collective = True
    model.rgb_encoder.on_grad_ready = lambda: None


ALL = ("sigma", "rgb", "normal", "semantic")
CASES = {
    "default_sigma_rgb": dict(),
    "default_all_outputs": dict(seeded=ALL),
    "classes4": dict(classes=4, seeded=ALL),
    "classes3": dict(classes=3, seeded=ALL),
    "codes_kp160": dict(embed_a=True),
    "input_grads": dict(input_grads=True),
    # the second-order route; its values are held by test_second_order_gpu.py and test_normal_ref_gpu.py, not here
    "second_order": dict(prepare=_second_order, seeded=("sigma", "rgb", "dsigma_dx")),
    "second_order_v_only": dict(prepare=_second_order, seeded=("dsigma_dx",)),   # (values: the same two modules)
    "ray_codes": dict(embed_a="ray_codes"),
    "ray_codes_gaps": dict(embed_a="ray_codes_gaps"),       # the two fills of rgb_in before embed_a_fwd
    "classes9": dict(classes=9, seeded=ALL),                # heads unforked, the semantic head as two linear_fwd
    "density_four_launches": dict(prepare=_four_launches),
    "normal_only": dict(seeded=("normal",)),                # a head creates dfeat_rgb; no fork, no density head
    "semantic_only": dict(seeded=("semantic",)),
    "normal_only_codes": dict(embed_a=True, seeded=("normal",)),   # the code columns of dfeat_rgb come from torch.zeros
    "sigma_only": dict(seeded=("sigma",)),
    "collective_first": dict(prepare=_collective_first),    # the colour scatter leads, the density scatter follows
    "input_grads_codes": dict(input_grads=True, embed_a=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_field_launches(ngp, case):
    cfg = CASES[case]
    got, model, (x, d, kw), ws, outs = record_field(ngp, **cfg)
    _assert_launches(got, EXPECTED[case])
    # launch lists cannot tell a fill from none, or zeros from empty: the routes no numeric test reaches assert values
    if case in ("classes4", "classes3", "classes9"):
        _assert_head_and_table_gradients(model, x.detach(), d.detach(), ws, cfg["classes"])
    if case == "normal_only_codes":
        g_codes = kw["embedding_a"].grad
        assert g_codes is not None and bool(torch.isfinite(g_codes).all()) and not bool(g_codes.any())
        _assert_head_and_table_gradients(model, x.detach(), d.detach(), ws, 7, seeded=("normal",), names=("rgb_encoder",))
    if case == "ray_codes_gaps":
        for k in ("rgb", "normal", "semantic"):
            assert outs[k].shape[0] == N_SAMPLES and bool(torch.isfinite(outs[k]).all()), k


def _trainer_step_launches(ngp, **trainer_kw):
    from ngp_amd import networks
    from ngp_amd.trainer import NGPTrainer
    model = _grid_model(ngp, seed=3)
    tr = NGPTrainer(model, lr=1e-2, **trainer_kw)
    # torch hands out streams round-robin from a pool of 32 per device, so in a long process a new stream IS an older one,
    # and which one depends on how many were drawn before.  test_trainer_streams_belong_to_its_model compares the handles
    # two trainers get with the field's own: this trainer drew 2 (optimizer, march-ahead), draw the other 30 so that
    # every later module finds the pool where it would be without this test
    assert tr._opt_stream is not None and tr._march_ahead.stream is not None
    for _ in range(_TORCH_STREAM_POOL - 2):
        torch.cuda.Stream(device=DEV)
    o, d, gt = _lego_batch()
    tr.step(o, d, gt)                                          # (the step with the all-cells occupancy update)
    rec = _record_step_launches(networks, pytest.MonkeyPatch(), tr, lambda: tr.step(o, d, gt))
    tr.wait()
    torch.cuda.synchronize()
    return [(name, role) for name, role, _ in rec]


def test_trainer_step_launches(ngp):
    """one steady-state NGPTrainer.step: the sinks and the act_bwd_rows route of a bound step"""
    assert _trainer_step_launches(ngp) == EXPECTED_STEP


def test_trainer_step_launches_normal_ref(ngp):
    """one steady-state NGPTrainer(normal_ref=True).step: the second-order route with the trainer's sinks"""
    assert _trainer_step_launches(ngp, normal_ref=True) == EXPECTED_STEP_NORMAL_REF


# (name, stream role, arguments) in launch order; t(offset, *strides) is a tensor argument
EXPECTED = {
    "default_sigma_rgb": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "default_all_outputs": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 1)),
        ("mlp_hidden_bwd", "caller", (t(0, 7, 1), 7, t(0, 7, 1), 7, 0, t(4096, 1), 32, t(0, 32, 1), 32, 1, 257, 32, 7, t(0, 16, 1), 16, t(0, 32, 1), 32, None, 0, None)),
        ("linear_bwd_input", "caller", (t(0, 32, 1), 32, t(0, 1), 128, 257, 128, 32, t(0, 128, 1), 128, 1)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 16, 1), 16, t(0, 32, 1), 32, 257, 32, 7, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 32, 1), 32, t(16, 144, 1), 144, 257, 128, 32, t(0, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "classes4": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 4, t(0, 32, 1), 32, t(0, 4, 1), 4)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 1)),
        ("mlp_hidden_bwd", "caller", (t(0, 4, 1), 4, t(0, 4, 1), 4, 0, t(4096, 1), 32, t(0, 32, 1), 32, 1, 257, 32, 4, None, 0, t(0, 32, 1), 32, t(4096, 1), 32, None)),
        ("linear_bwd_input", "caller", (t(0, 32, 1), 32, t(0, 1), 128, 257, 128, 32, t(0, 128, 1), 128, 1)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 32, 1), 32, t(16, 144, 1), 144, 257, 128, 32, t(0, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "classes3": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 1)),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 1)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "codes_kp160": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 160, 1), 160)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 160, 1), 160)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 160, 1), 160, t(0, 1), 160, None, 1, t(20480, 1), 128, None, 2, 257, 160, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 160, 257, 136, 128, 3, t(0, 136, 1), 136, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(0, 160, 1), 160, 257, 160, 128, 3, t(0, 1), 160, None, t(20480, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "input_grads": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 1), 144, 257, 16, 128, 3, t(0, 16, 1), 16, 0)),
        ("sh_bwd_dirs", "caller", (t(0, 3, 1), t(0, 16, 1), 16, 257, t(0, 3, 1))),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("grid_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 3, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_input", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, 0)),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("grid_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 3, 1))),
    ],
    "second_order": [
        ("sh_fwd", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("grid_bwd_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, t(0, 3, 1), 257, t(0, 1), t(0, 128, 1))),
        ("linear_fwd", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, None, 257, 128, 128, 0, t(0, 128, 1), 128, None)),
        ("density_head_bwd2", "caller", (t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1), 257, t(0, 128, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1), t(0, 1))),
        ("linear_bwd_weight", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, None)),
        ("linear_bwd_weight", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, t(0, 1))),
        ("linear_bwd_input", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
    ],
    "second_order_v_only": [
        ("sh_fwd", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, t(0, 3, 1), 257, t(0, 1), t(0, 128, 1))),
        ("linear_fwd", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, None, 257, 128, 128, 0, t(0, 128, 1), 128, None)),
        ("density_head_bwd2", "caller", (t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 128, 1), None, 257, t(0, 128, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1), t(0, 1))),
        ("linear_bwd_weight", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, None)),
        ("linear_bwd_weight", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, t(0, 1))),
        ("linear_bwd_input", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, 257, 128, 128, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
    ],
    "ray_codes": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 160, 1), 160)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 160, 1), 160)),
        ("embed_a_fwd", "colour", (t(0, 8, 1), 6, 8, t(0, 1), t(0, 3, 1), 5, t(144, 160, 1), 160, 16)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 160, 1), 160, t(0, 1), 160, None, 1, t(20480, 1), 128, None, 2, 257, 160, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 160, 257, 136, 128, 3, t(0, 136, 1), 136, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 1))),
        ("embed_a_bwd", "caller", (t(128, 136, 1), 136, 8, t(0, 1), t(0, 3, 1), 5, 6, t(0, 8, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(0, 160, 1), 160, 257, 160, 128, 3, t(0, 1), 160, None, t(20480, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "ray_codes_gaps": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 160, 1), 160)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 160, 1), 160)),
        ("embed_a_fwd", "colour", (t(0, 8, 1), 6, 8, t(0, 1), t(0, 3, 1), 5, t(144, 160, 1), 160, 16)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 160, 1), 160, t(0, 1), 160, None, 1, t(20480, 1), 128, None, 2, 257, 160, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 160, 257, 136, 128, 3, t(0, 136, 1), 136, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 1))),
        ("embed_a_bwd", "caller", (t(128, 136, 1), 136, 8, t(0, 1), t(0, 3, 1), 5, 6, t(0, 8, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(0, 160, 1), 160, 257, 160, 128, 3, t(0, 1), 160, None, t(20480, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "classes9": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("mlp2_fwd", "colour", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("linear_fwd", "colour", (t(16, 144, 1), 144, t(0, 1), 128, None, 257, 128, 32, 1, t(0, 32, 1), 32, None)),
        ("linear_fwd", "colour", (t(0, 32, 1), 32, t(4096, 1), 32, None, 257, 32, 9, 0, t(0, 9, 1), 9, None)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 1)),
        ("mlp_hidden_bwd", "caller", (t(0, 9, 1), 9, t(0, 9, 1), 9, 0, t(4096, 1), 32, t(0, 32, 1), 32, 1, 257, 32, 9, t(0, 16, 1), 16, t(0, 32, 1), 32, None, 0, None)),
        ("linear_bwd_input", "caller", (t(0, 32, 1), 32, t(0, 1), 128, 257, 128, 32, t(0, 128, 1), 128, 1)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 16, 1), 16, t(0, 32, 1), 32, 257, 32, 9, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 32, 1), 32, t(16, 144, 1), 144, 257, 128, 32, t(0, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "density_four_launches": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("grid_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), 128)),
        ("mlp2_fwd_dact", "caller", (t(0, 128, 1), 128, t(0, 128, 1), 128, t(0, 1), 3, t(0, 128, 1), 128, t(0, 1), 3, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1, 1), 1, t(0, 1, 1))),
        ("mlp_bwd_input", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, 0)),
        ("grid_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "normal_only": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 144, 1), 144, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
    ],
    "semantic_only": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("mlp_hidden_bwd", "caller", (t(0, 7, 1), 7, t(0, 7, 1), 7, 0, t(4096, 1), 32, t(0, 32, 1), 32, 1, 257, 32, 7, t(0, 16, 1), 16, t(0, 32, 1), 32, None, 0, None)),
        ("linear_bwd_input", "caller", (t(0, 32, 1), 32, t(0, 1), 128, 257, 128, 32, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("linear_bwd_weight", "caller", (t(0, 16, 1), 16, t(0, 32, 1), 32, 257, 32, 7, t(4096, 1), 32, None)),
        ("linear_bwd_weight", "caller", (t(0, 32, 1), 32, t(16, 144, 1), 144, 257, 128, 32, t(0, 1), 128, None)),
    ],
    "normal_only_codes": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 160, 1), 160)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 160, 1), 160)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 160, 1), 160, t(0, 1), 160, None, 1, t(20480, 1), 128, None, 2, 257, 160, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 0, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(0, 1), 128, 257, 128, 32, 3, t(0, 136, 1), 136, 0)),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(4096, 1), 32, t(0, 32, 1), 32, 1, t(16, 160, 1), 160, 257, 128, 32, 3, t(0, 1), 128, None, t(4096, 1), 32, None)),
    ],
    "sigma_only": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "collective_first": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 144, 1), 144)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 144, 1), 144)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 144, 1), 144, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 144, 1), 144, t(0, 1), 144, None, 1, t(18432, 1), 128, None, 2, 257, 144, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 144, 257, 128, 128, 3, t(0, 128, 1), 128, 0)),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("grid_bwd_param_scaled", "scatter", ("desc", t(0, 3, 1), t(0, 128, 1), 128, t(0, 1), 257, t(0, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(18432, 1), 128, t(0, 128, 1), 128, 1, t(0, 144, 1), 144, 257, 144, 128, 3, t(0, 1), 144, None, t(18432, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
    ],
    "input_grads_codes": [
        ("sh_fwd_dirs", "colour", (t(0, 3, 1), 257, 4, t(0, 160, 1), 160)),
        ("grid_fwd", "colour", ("desc", t(0, 1), t(0, 3, 1), 257, t(16, 160, 1), 160)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 3, t(0, 32, 1), 32, t(0, 3, 1), 3)),
        ("mlp2_fwd", "heads", (t(16, 160, 1), 160, t(0, 1), 128, None, 1, t(4096, 1), 32, None, 0, 257, 128, 32, 7, t(0, 32, 1), 32, t(0, 7, 1), 7)),
        ("mlp2_fwd", "colour", (t(0, 160, 1), 160, t(0, 1), 160, None, 1, t(20480, 1), 128, None, 2, 257, 160, 128, 3, t(0, 128, 1), 128, t(0, 3, 1), 3)),
        ("density_field_fwd", "caller", ("desc", t(0, 1), t(0, 3, 1), 257, t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 1), t(0, 128, 1), t(0, 128, 1), t(0, 1, 1), t(0, 128, 1), t(0, 3, 1))),
        ("act_bwd", "caller", (t(0, 3, 1), t(0, 3, 1), 771, 2, t(0, 3, 1))),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(16, 1), 160, 257, 136, 128, 3, t(0, 136, 1), 136, 0)),
        ("mlp_bwd_input", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(0, 1), 160, 257, 16, 128, 3, t(0, 16, 1), 16, 0)),
        ("sh_bwd_dirs", "caller", (t(0, 3, 1), t(0, 16, 1), 16, 257, t(0, 3, 1))),
        ("grid_bwd_param", "scatter", ("desc", t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 1))),
        ("grid_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 136, 1), 136, 257, t(0, 3, 1))),
        ("mlp_bwd_weight", "caller", (t(0, 3, 1), 3, t(20480, 1), 128, t(0, 128, 1), 128, 1, t(0, 160, 1), 160, 257, 160, 128, 3, t(0, 1), 160, None, t(20480, 1), 128, None)),
        ("act_bwd", "caller", (t(0, 1, 1), t(0, 1, 1), 257, 3, t(0, 1, 1))),
        ("mlp_bwd_input", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, 0)),
        ("mlp_bwd_weight", "caller", (t(0, 1, 1), 1, t(0, 128, 1), 128, t(0, 128, 1), 128, 3, t(0, 128, 1), 128, 257, 128, 128, 1, t(0, 128, 1), 128, t(0, 1), t(0, 128, 1), 128, t(0, 1))),
        ("grid_bwd_param", "caller", ("desc", t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 1))),
        ("grid_bwd_input", "caller", ("desc", t(0, 1), t(0, 3, 1), t(0, 128, 1), 128, 257, t(0, 3, 1))),
    ],
}
EXPECTED_STEP = [
    ("sh_fwd_dirs", "colour-forward"),
    ("grid_fwd", "colour-forward"),
    ("mlp2_fwd", "march-ahead"),
    ("mlp2_fwd", "march-ahead"),
    ("mlp2_fwd", "colour-forward"),
    ("density_field_fwd", "caller"),
    ("grid_bwd_param_scaled", "optimizer"),
    ("act_bwd_rows", "caller"),
    ("mlp_bwd_input", "caller"),
    ("grid_bwd_param", "optimizer"),
    ("mlp_bwd_weight", "caller"),
    ("act_bwd_rows", "caller"),
    ("mlp_bwd_weight", "caller"),
]
EXPECTED_STEP_NORMAL_REF = [
    ("sh_fwd", "colour-forward"),
    ("grid_fwd", "colour-forward"),
    ("mlp2_fwd", "march-ahead"),
    ("mlp2_fwd", "march-ahead"),
    ("mlp2_fwd", "colour-forward"),
    ("density_field_fwd", "caller"),
    ("act_bwd", "caller"),
    ("mlp_bwd_input", "caller"),
    ("act_bwd", "caller"),
    ("mlp_bwd_input", "caller"),
    ("grid_bwd_param", "optimizer"),
    ("mlp_bwd_weight", "caller"),
    ("mlp_bwd_weight", "caller"),
    ("grid_bwd_bwd_input", "caller"),
    ("linear_fwd", "caller"),
    ("density_head_bwd2", "caller"),
    ("linear_bwd_weight", "caller"),
    ("linear_bwd_weight", "caller"),
    ("linear_bwd_input", "caller"),
    ("grid_bwd_param", "caller"),
]
