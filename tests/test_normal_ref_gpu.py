"""NGPTrainer(normal_ref=True) on the GPU: the two new entries through the C ABI, the field's second order on the fused node,
the reference's own normal_ref step (G10), the trainer's step and the recipe end to end.

Bars.  (a), (b), (c) are held to the project's own second-order bar (tests/test_second_order_gpu.py): the error is
max-normalised against the float64 reference and must lie within second_order_reference.FACTOR (8) x floor, the floor being
the same expressions evaluated in float32 on the same case, clamped at 2^-23; every row is compared.
  (a) ngp_density_head_bwd2 against normal_ref_reference.head_closed (which test_normal_ref_host.py holds to autograd):
      n in {1, 31, 32, 33, 257}, one and two full tiles plus a ragged row, a second trip of the grid-stride loop with a ragged tile,
      and two full trips plus one row (all from NGP_DENSITY_BWD2_ROWS / _MAX_BLOCKS); d_sig NULL and present; prefilled
      sinks; a one-signed case; rows saturated at 1e-6 and at 30; e1 written over r; guard bands; bit-identical sums.
  (b) ngp_normal_ref_tail against torch float64 autograd of lambda_rp mean(Rp) + lambda_ro mean(Ro) on one batch with empty,
      1-sample, 32-, 33- and 70-sample rays, an early-stopped ray and an omitted one, exact-zero rows, a strided head; write
      and add mode; scale 0.5 and 8.  The rows of the eps branch (gradients of order 1e6 g) are ALSO compared on their own,
      and the others without them: a max over all rows alone would be blind to everything below 1e-6 of those.
  (c) the field: NGP(scale).second_order_normals on second_order_reference.field_points / density_field, scale 0.5 and 8,
      and the trainer-owned gradient buffer, empty and prefilled.
  (d) the fused route on tests/golden/g10_normal_ref_step.npz with the bars test_normal_ref_step_matches_reference_golden
      holds the module route to: terms 1e-3 relative, gradients G10_BAR = 5e-5 max-normalised, table L2 norms 5e-3.
  (e) the trainer: no new entry on a default step; one step each of three recipes; the ref terms alone.  The one route
      comparison (the fused step against loss_kwargs={'normal_ref': True} from the same seeds) carries
      tail_harness.fused_against_layered's bars: loss rtol 1e-4, gradients within 3e-4 of the tensor's largest entry.
  (f) the tool in a child process, with and without --normal_ref on the same files.
"""
import os
import re

import numpy as np
import pytest
import torch

import normal_ref_reference as R
import second_order_reference as S
import tail_harness as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 7.0
GUARD = 256            # floats around every output
G10_BAR = 5e-5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _launch_shape():
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    return (int(re.search(r"#define NGP_DENSITY_BWD2_ROWS (\d+)", hdr).group(1)),
            int(re.search(r"#define NGP_DENSITY_BWD2_MAX_BLOCKS (\d+)", hdr).group(1)))


class _Bands:
    """float32 device arrays cut from one allocation of SENTINEL, GUARD floats between and around them (16-byte aligned)"""

    def __init__(self, **shapes):
        sizes = {k: int(np.prod(s)) for k, s in shapes.items()}
        total = GUARD + sum((n + 3) // 4 * 4 + GUARD for n in sizes.values())
        self.buf = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
        self.at, off = {}, GUARD
        for k, n in sizes.items():
            self.at[k] = (off, n, shapes[k])
            off += (n + 3) // 4 * 4 + GUARD

    def __getitem__(self, k):
        off, n, shape = self.at[k]
        return self.buf[off:off + n].view(shape)

    def check(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        for off, n, _ in self.at.values():
            keep[off:off + n] = False
        assert bool((self.buf[keep] == SENTINEL).all()), "a guard band was written"


# ------------------------------------------------------------------------------------------- (a) ngp_density_head_bwd2
def _head_run(ngp, case, prefill=None, alias=False):
    a1, sig, r, w2, g = case
    n = len(sig)
    out = _Bands(m=(n, 128), e1=(n, 128), dW2=(128,), db2=(1,))
    if prefill is None:
        out["dW2"].zero_()
        out["db2"].zero_()
    else:
        out["dW2"].copy_(T(prefill[0]))
        out["db2"].copy_(T(prefill[1]))
    rt = T(r)
    if alias:
        out["e1"].copy_(rt)
        rt = out["e1"]
    ws = torch.empty(ngp._lib.call_host("density_head_bwd2_workspace", n), dtype=torch.float32, device=DEV)
    ngp._lib.call("density_head_bwd2", T(a1), T(sig), rt, T(w2), None if g is None else T(g), n, out["m"], out["e1"],
                  out["dW2"], out["db2"], ws)
    torch.cuda.synchronize()
    out.check()
    return {k: N(out[k]).astype(np.float64) for k in R.HEAD_KEYS}


def _head_compare(tag, got, case, prefill=None):
    r64, r32 = R.head_closed(*case), R.head_closed(*case, dtype=torch.float32)
    for k in R.HEAD_KEYS:
        want, low = r64[k], r32[k].astype(np.float32)
        if prefill is not None and k in ("dW2", "db2"):
            pre = prefill[0] if k == "dW2" else prefill[1]
            want, low = pre.astype(np.float64) + want, pre + low
        S.compare(got[k], want, S.floor_of(low, want), f"{tag} {k}")


def _head_counts():
    rows, blocks = _launch_shape()
    # (1, rows + 1 and 2 * rows + 1 rows are 1, 2 and 3 workgroups: the ordered sum's single row, its pair and its odd tail)
    counts = [1, 31, 32, 33, 257, rows + 1, 2 * rows + 1, rows * blocks + rows + 1, 2 * rows * blocks + 1]
    assert max(counts) <= 40000
    return counts


@pytest.mark.parametrize("with_g", [True, False], ids=["d_sig", "null"])
def test_head_bwd2_against_float64(ngp, with_g):
    for i, n in enumerate(_head_counts()):
        case = R.head_case("mixed", n, i, with_g)
        _head_compare(f"head n={n} {'g' if with_g else 'NULL'}", _head_run(ngp, case), case)


def test_head_bwd2_one_signed_sums_lose_no_tile(ngp):
    """r, a1, w2, d_sig > 0: every term of dW2 and db2 is positive, so a tile that is lost or counted twice moves the sums by
    its full share (8 rows of 8 201: 1e-3, a thousand bars)"""
    for n in _head_counts()[-3:]:
        case = R.head_case("positive", n, 20)
        got = _head_run(ngp, case)
        assert got["dW2"].min() > 0 and got["db2"][0] > 0
        _head_compare(f"head positive n={n}", got, case)


@pytest.mark.parametrize("kind", ["tiny", "large"])
@pytest.mark.parametrize("with_g", [True, False], ids=["d_sig", "null"])
def test_head_bwd2_saturated_rows(ngp, kind, with_g):
    case = R.head_case(kind, 257, 30, with_g)
    _head_compare(f"head {kind} {'g' if with_g else 'NULL'}", _head_run(ngp, case), case)


def test_head_bwd2_accumulates_bitwise_and_in_place(ngp):
    n = _head_counts()[-2]
    case = R.head_case("mixed", n, 40)
    rng = np.random.default_rng(41)
    pre = (rng.standard_normal(128).astype(np.float32) * 50, rng.standard_normal(1).astype(np.float32) * 50)
    first = _head_run(ngp, case, prefill=pre)
    _head_compare("head prefilled", first, case, prefill=pre)
    again = _head_run(ngp, case, prefill=pre)
    for k in R.HEAD_KEYS:
        assert np.array_equal(first[k], again[k]), k                        # no atomics: the same bits on every run
    over_r = _head_run(ngp, case, prefill=pre, alias=True)                   # e1 written over r
    for k in R.HEAD_KEYS:
        assert np.array_equal(first[k], over_r[k]), k


def test_head_bwd2_bad_arguments_launch_nothing(ngp):
    lib = ngp._lib.load()
    out = _Bands(m=(8, 128), e1=(8, 128), dW2=(128,), db2=(1,))
    a1, sig, r, w2 = (torch.ones(8, 128, device=DEV), torch.ones(8, device=DEV), torch.ones(8, 128, device=DEV),
                      torch.ones(128, device=DEV))
    ws = torch.empty(ngp._lib.call_host("density_head_bwd2_workspace", 8), dtype=torch.float32, device=DEV)
    p = lambda t, off=0: None if t is None else t.data_ptr() + off
    good = [p(a1), p(sig), p(r), p(w2), None, 8, p(out["m"]), p(out["e1"]), p(out["dW2"]), p(out["db2"]), p(ws)]
    stream = torch.cuda.current_stream().cuda_stream
    for at, value in ((0, None), (1, None), (2, None), (3, None), (6, None), (7, None), (8, None), (9, None), (10, None),
                      (5, -1), (0, p(a1, 4)), (2, p(r, 8)), (6, p(out["m"], 4)), (7, p(out["e1"], 12)), (10, p(ws, 4))):
        bad = list(good)
        bad[at] = value
        assert lib.ngp_density_head_bwd2(*bad, stream) == -22, at
    empty = list(good)
    empty[5] = 0
    assert lib.ngp_density_head_bwd2(*empty, stream) == 0
    torch.cuda.synchronize()
    assert bool((out.buf == SENTINEL).all())                                 # nothing ran


# ------------------------------------------------------------------------------------------- (b) ngp_normal_ref_tail
LAMBDAS = (1e-3, 2e-3)


def _tail_run(ngp, c, add, ld=5):
    n, slots = c["N"], c["n_slots"]
    ref = R.tail_definition(c, *LAMBDAS)
    out = _Bands(d_grads=(n, 3), d_head=(n, 3), terms=(2,))
    pre = None
    if add:
        pre = np.random.default_rng(5).standard_normal((n, 3)).astype(np.float32) * 1e-4
        out["d_head"].copy_(T(pre))
    head = torch.full((n, ld), float("nan"), device=DEV)                    # a strided head between NaN columns
    head[:, 1:4] = T(c["head"])
    Ro, Rp = ref["Ro"].astype(np.float32), ref["Rp"].astype(np.float32)
    Ro[R.TAIL_OMITTED], Rp[R.TAIL_OMITTED] = np.nan, np.nan                 # the omitted ray's slots are not read
    ngp._lib.call("normal_ref_tail", T(c["dsig"]), T(c["scale3"]), head[:, 1:4], ld, T(c["dirs"]), T(c["ws"]), T(c["rays_a"]),
                  len(c["rays_a"]), T(Ro), T(Rp), float(LAMBDAS[0]), float(LAMBDAS[1]), int(add), out["d_grads"], out["d_head"],
                  out["terms"])
    torch.cuda.synchronize()
    out.check()
    return {k: N(out[k]).astype(np.float64) for k in R.TAIL_KEYS}, pre, ref


@pytest.mark.parametrize("add", [False, True], ids=["write", "add"])
@pytest.mark.parametrize("scale", [0.5, 8.0])
def test_normal_ref_tail_against_float64(ngp, scale, add):
    c = R.tail_case(scale)
    got, pre, r64 = _tail_run(ngp, c, add)
    r32 = R.tail_definition(c, *LAMBDAS, dtype=torch.float32)
    om, named = c["omitted_rows"], c["named_rows"]
    # rows rays_a does not name are not touched: the sentinel, or what was there
    assert (got["d_grads"][om] == SENTINEL).all()
    assert np.array_equal(got["d_head"][om], pre[om].astype(np.float64)) if add else (got["d_head"][om] == SENTINEL).all()
    tag = f"tail s={scale:g} {'add' if add else 'write'} "
    S.compare(got["terms"], r64["terms"], S.floor_of(r32["terms"], r64["terms"]), tag + "terms")
    eps_g, eps_h = np.isin(named, c["zero_g"]), np.isin(named, c["zero_h"])
    for key, eps in (("d_grads", eps_g), ("d_head", eps_h)):
        want, low = r64[key][named], r32[key][named].astype(np.float32)
        if add and key == "d_head":
            want, low = pre[named].astype(np.float64) + want, pre[named] + low
        for part, rows in (("all rows", slice(None)), ("eps rows", eps), ("other rows", ~eps)):
            S.compare(got[key][named][rows], want[rows], S.floor_of(low[rows], want[rows]), tag + f"{key} {part}")
    # behind the early stop and on rows that face away: exact zeros
    stopped = np.flatnonzero(c["ws"] == 0)
    assert not got["d_grads"][stopped].any()
    if not add:
        assert not got["d_head"][stopped].any()


def test_normal_ref_tail_ro_gradient_is_zero_facing_away(ngp):
    """lambda_rp = 0 leaves Ro's gradient alone: exactly 0 on every row with <n_raw, d> < 0, and the head gets none"""
    c = R.tail_case(0.5)
    n = c["N"]
    out = _Bands(d_grads=(n, 3), d_head=(n, 3), terms=(2,))
    ref = R.tail_definition(c, 0.0, 2e-3)
    Ro, Rp = np.nan_to_num(ref["Ro"]).astype(np.float32), ref["Rp"].astype(np.float32)
    ngp._lib.call("normal_ref_tail", T(c["dsig"]), T(c["scale3"]), T(c["head"]), 3, T(c["dirs"]), T(c["ws"]), T(c["rays_a"]),
                  len(c["rays_a"]), T(Ro), T(Rp), 0.0, 2e-3, 0, out["d_grads"], out["d_head"], out["terms"])
    torch.cuda.synchronize()
    out.check()
    named = c["named_rows"]
    away = ((-(c["dsig"] * c["scale3"]).astype(np.float64)) * c["dirs"]).sum(1)[named] < 0
    got = N(out["d_grads"])[named]
    assert away.sum() > 20 and not got[away].any() and np.abs(got[~away]).max() > 0
    assert not N(out["d_head"])[named].any() and float(out["terms"][0]) == 0.0


# ------------------------------------------------------------------------------------------- (c) the field
_FIELDS = {}


def _field(ngp, scale):
    """tests/test_second_order_gpu.py's field case with the fused node's second order in place of the module route"""
    if scale in _FIELDS:
        return _FIELDS[scale]
    torch.manual_seed(5)
    model = ngp.networks.NGP(scale=scale).to(DEV)
    with torch.no_grad():            # tcnn's 1e-4 init makes every feature ~0: an O(1) table for a real test
        model.xyz_encoder.params.uniform_(-0.3, 0.3)
    model.second_order_normals = True
    pts = S.field_points(scale)
    lay = S.field_layout(scale)
    assert lay.n_params == model.xyz_encoder.params.numel()
    lo, hi = np.float32(-scale), np.float32(scale)
    xn = (pts["x"] - lo) / (hi - lo)
    assert np.array_equal(N((T(pts["x"]) - model.xyz_min) / (model.xyz_max - model.xyz_min)), xn)
    span = N(model.xyz_max - model.xyz_min).reshape(3)
    lin1, lin2 = model.xyz_net[0], model.xyz_net[2]
    p = dict(table=N(model.xyz_encoder.params), W1=N(lin1.weight), b1=N(lin1.bias), W2=N(lin2.weight), b2=N(lin2.bias))
    args = (p, xn, span, pts["g_sigma"], pts["g_normals"], lay)
    r64, r32 = S.density_field(*args), S.density_field(*args, dtype=torch.float32)
    floors = {k: S.floor_of(r32[k], r64[k]) for k in S.FIELD_KEYS}
    _FIELDS[scale] = (model, pts, r64, r32, floors)
    return _FIELDS[scale]


def _field_loss(model, pts):
    sig, _, n_raw, _, _ = model(T(pts["x"]), T(pts["d"]))
    return sig, n_raw, (sig * T(pts["g_sigma"])).sum() + (n_raw * T(pts["g_normals"])).sum()


def _field_params(model):
    return [model.xyz_encoder.params, model.xyz_net[0].weight, model.xyz_net[0].bias, model.xyz_net[2].weight,
            model.xyz_net[2].bias]


@pytest.mark.parametrize("scale", [0.5, 8.0])
def test_field_second_order_on_the_fused_node(ngp, scale):
    model, pts, r64, _, fl = _field(ngp, scale)
    calls = ngp._lib.CAPTURE = {"density_head_bwd2": [], "grid_bwd_bwd_input": [], "density_field_fwd": []}
    try:
        sig, n_raw, loss = _field_loss(model, pts)
        assert n_raw.requires_grad
        grads = torch.autograd.grad(loss, _field_params(model))
    finally:
        ngp._lib.CAPTURE = None
    assert [len(v) for v in calls.values()] == [1, 1, 1]                    # the fused node, not the module route
    tag = f"fused field s={scale:g} "
    S.compare(N(sig), r64["sigma"], fl["sigma"], tag + "sigma")
    S.compare(N(n_raw), r64["normals"], fl["normals"], tag + "normals")
    S.compare(N(grads[0]), r64["table"], fl["table"], tag + "table", rows=r64["rows"])
    for k, g in zip(("W1", "b1", "W2", "b2"), grads[1:]):
        S.compare(N(g), r64[k], fl[k], tag + k)
    if scale != 0.5:
        del _FIELDS[scale]           # the tables of a model are 1.3 GB


@pytest.mark.parametrize("prefilled", [False, True])
def test_trainer_owned_gradient_buffer_gets_both_orders_once(ngp, prefilled):
    """the encoder wired as the trainer wires it (enc.grad_buffer a view of a flat buffer): both table contributions of the
    second-order route go straight into it; the buffer ends as (what it held) + the reference gradient, each share once"""
    model, pts, r64, r32, fl = _field(ngp, 0.5)
    enc, rows = model.xyz_encoder, r64["rows"]
    Fd = enc.n_features
    flat = torch.zeros(enc.params.numel() + 256, device=DEV)
    view = flat[128:128 + enc.params.numel()]
    if prefilled:
        view.copy_(torch.randn(view.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(11)))
    before = view.clone()
    small = _field_params(model)[1:]
    try:
        enc.params.grad = view
        enc.grad_buffer = enc.params.grad
        _, _, loss = _field_loss(model, pts)
        loss.backward()
        torch.cuda.synchronize()
        assert enc.params.grad.data_ptr() == view.data_ptr()
        moved = torch.nonzero((view != before).view(-1, Fd).any(1)).reshape(-1).cpu().numpy()
        assert np.isin(moved, rows).all(), "rows that no sample touches changed"
        got = N(view.view(-1, Fd)[T(rows)])
        pre = N(before.view(-1, Fd)[T(rows)])
        want = pre.astype(np.float64) + r64["table"]
        floor = S.floor_of(pre + r32["table"].astype(np.float32), want) if prefilled else fl["table"]
        tag = "fused trainer buffer, prefilled: " if prefilled else "fused trainer buffer: "
        S.compare(got, want, floor, tag + "table")
        assert not flat[:128].any() and not flat[-128:].any()
        for k, p in zip(("W1", "b1", "W2", "b2"), small):
            S.compare(N(p.grad), r64[k], fl[k], tag + k)
    finally:
        enc.grad_buffer = None
        enc.params.grad = None
        for p in small:
            p.grad = None


def test_second_order_refuses_a_sample_gradient(ngp):
    model, pts, _, _, _ = _field(ngp, 0.5)
    x = T(pts["x"]).requires_grad_(True)
    with pytest.raises(RuntimeError, match="require a gradient"):
        model(x, T(pts["d"]))


# ------------------------------------------------------------------------------------------- (d) the reference's step
G10_SMALL = ("xyz_net.0.weight", "xyz_net.0.bias", "xyz_net.2.weight", "xyz_net.2.bias", "rgb_net.params",
             "norm_pred_header.params", "semantic_header.params")
G10_TABLES = ("xyz_encoder.params", "rgb_encoder.params")


@pytest.fixture(scope="module")
def g10_fused(ngp, golden):
    """The G10 fixture (the reference's render + NeRFLoss(normal_ref=True) + backward, 64 rays) on the FUSED route, once:
    model.second_order_normals and FusedTail(normal_ref=...), the backward seeded as NGPTrainer seeds it.  Cannot be built
    without the feature: FusedTail takes no normal_ref and the fused node's d(sigma)/dx carries no graph."""
    from helpers import table_rule
    from ngp_amd.losses import NeRFLoss
    from ngp_amd.rendering import FusedTail, render
    g = golden("g10_normal_ref_step.npz")
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    with torch.no_grad():
        model.xyz_encoder.params.copy_(T(table_rule(model.xyz_encoder.params.numel())))
        model.rgb_encoder.params.copy_(T(table_rule(model.rgb_encoder.params.numel())))
        named = dict(model.named_parameters())
        for k in G10_SMALL:
            named[k].copy_(T(g[k]))
        model.density_bitfield.copy_(T(g["density_bitfield"]))
    model.second_order_normals = True
    o, d, gt = T(g["rays_o"]), T(g["rays_d"]), T(g["rgb_gt"])
    noise = T(g["noise"])
    fn = NeRFLoss()
    tail = FusedTail(gt, fn.lambda_opa, fn.lambda_distortion, normal_ref=(fn.lambda_normal_ref_rp, fn.lambda_normal_ref_ro))
    calls = ngp._lib.CAPTURE = {"render_loss_fused": [], "normal_ref_tail": [], "density_head_bwd2": [], "sh_fwd": [],
                                "sh_fwd_dirs": []}
    real_rand_like = torch.rand_like
    try:
        torch.rand_like = lambda t, *a, **k: noise.clone()      # the marcher's jitter of the fixture
        res = render(model, o, d, exp_step_factor=0.0, num_classes=7, _fused_loss=tail)
        torch.rand_like = real_rand_like
        terms, ref_terms = res["_loss_terms"], res["_ref_terms"]
        torch.autograd.backward([terms, ref_terms], [T(np.asarray([1, 0, 0, 0], np.float32)), torch.ones(2, device=DEV)])
    finally:
        torch.rand_like = real_rand_like
        ngp._lib.CAPTURE = None
    torch.cuda.synchronize()
    lt = N(terms).astype(np.float64)
    rt = N(ref_terms).astype(np.float64)
    grads = {k: (N(p.grad).copy() if p.grad is not None else None) for k, p in named.items()}
    return dict(g=g, calls={k: len(v) for k, v in calls.items()}, grads=grads,
                terms=dict(rgb=lt[1], opacity=lt[2], distortion=lt[3], normal_ref_rp=rt[0], normal_ref_ro=rt[1]))


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_fused_normal_ref_step_terms_match_reference_golden(g10_fused):
    """the five loss terms within 1e-3 relative, from one call each of the tail, ngp_normal_ref_tail and
    ngp_density_head_bwd2, the directions encoded by ngp_sh_fwd as on the module route"""
    g = g10_fused["g"]
    assert g10_fused["calls"] == {"render_loss_fused": 1, "normal_ref_tail": 1, "density_head_bwd2": 1, "sh_fwd": 1,
                                  "sh_fwd_dirs": 0}
    for k, v in g10_fused["terms"].items():
        ref = float(g["loss_" + k])
        print(f"[G10 fused] term {k}: {v:.6e} (reference {ref:.6e})")
        assert abs(v - ref) <= 1e-3 * abs(ref) + 1e-9, (k, v, ref)


@pytest.mark.parametrize("name", G10_SMALL)
def test_fused_normal_ref_step_gradients_match_reference_golden(g10_fused, name):
    """Every gradient within G10_BAR = 5e-5 max-normalised, the bar test_normal_ref_step_matches_reference_golden holds the
    module route to.

    Measured on an MI355X (fused route / module route): xyz_net.0.weight 3.5e-6 / 3.4e-6, xyz_net.0.bias 3.3e-6 / 9.2e-7,
    xyz_net.2.weight 3.1e-6 / 1.4e-6, xyz_net.2.bias 3.2e-6 / 1.1e-6, norm_pred_header.params 5.8e-7 / 5.2e-7,
    semantic_header.params exactly zero on both, rgb_net.params 7.3e-7 / 5.9e-7.  The rgb_net case is what pins the route's
    direction encoding (networks._FieldFn, second_order): sample 4045 of the fixture's 6 724 has hidden unit 59's
    pre-activation at +1.23e-8 from the layered encoding's input row and at -1.26e-8 from ngp_sh_fwd_dirs's, and with that
    kernel on this route the case read 5.48e-5, all of it in that unit's row of dW1."""
    g, got = g10_fused["g"], g10_fused["grads"][name]
    ref = g["grad_" + name]
    got = got if got is not None else np.zeros_like(ref)
    if np.abs(ref).max() == 0:
        assert not got.any(), name
        return
    print(f"[G10 fused] grad {name}: max-normalised error {_rel(got, ref):.2e}")
    assert _rel(got, ref) < G10_BAR, (name, _rel(got, ref))


@pytest.mark.parametrize("name", G10_TABLES)
def test_fused_normal_ref_step_table_gradients_match_reference_golden(g10_fused, name):
    """the recorded entries within G10_BAR, the L2 norm within 5e-3.  Measured on an MI355X (fused / module):
    xyz_encoder.params 2.3e-6 / 2.1e-6, rgb_encoder.params 6.3e-7 / 6.3e-7 (3.8e-5 with ngp_sh_fwd_dirs on this route: the
    sample above)"""
    g, got = g10_fused["g"], g10_fused["grads"][name]
    err = _rel(got[g["grad_idx_" + name]], g["grad_val_" + name])
    print(f"[G10 fused] grad {name}: max-normalised error {err:.2e}")
    assert err < G10_BAR, name
    l2 = float(g["grad_l2_" + name])
    assert abs(np.sqrt((got.astype(np.float64) ** 2).sum()) - l2) < 5e-3 * l2, name


# ------------------------------------------------------------------------------------------- (e) the trainer
NEW = ("density_head_bwd2", "normal_ref_tail")


def _model(ngp, seed, scale=0.5, **kw):
    torch.manual_seed(seed)
    model = H._grid_buffers(ngp.networks.NGP(scale=scale, **kw).to(DEV))
    with torch.no_grad():
        model.xyz_net[2].bias.fill_(1.0)      # a random field dense enough to be seen
        model.xyz_encoder.params.uniform_(-0.3, 0.3)      # ... whose d(sigma)/dx is no rounding residue
    return model


def _batch(n_rays, seed, classes=7, terms=()):
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=10, img_wh=(100, 100), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    img, pix = scene.sample_batch(n_rays, generator=gen)
    o, d = scene.rays(img, pix)
    gt, _ = scene.ground_truth(o, d, n_quad=64)
    step_kw = {H.TERMS[k][1]: v for k, v in H._scene_targets(scene, o, d, classes, gen, terms).items()}
    return o, d, gt, img, step_kw


def _one_step(ngp, model, o, d, gt, trainer_kw, step_kw, seed):
    from ngp_amd.trainer import NGPTrainer
    tr = NGPTrainer(model, lr=1e-2, **trainer_kw)
    tr.optimizer_step = lambda: None
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    tr.global_step = tr.warmup_steps + 1
    calls = ngp._lib.CAPTURE = {k: [] for k in NEW}
    try:
        torch.manual_seed(seed)
        loss, res = tr.step(o, d, gt, **step_kw)
        torch.cuda.synchronize()
    finally:
        ngp._lib.CAPTURE = None
    grads = {n: N(tr.flat_grad[off:off + k]).copy() for n, (off, k) in tr.slices.items()}
    return tr, float(loss), res, grads, {k: len(v) for k, v in calls.items()}


def test_default_step_calls_neither_entry_and_the_fused_step_matches_the_module_route(ngp):
    o, d, gt, _, _ = _batch(1500, 91)
    runs = {}
    for name, kw in (("default", {}), ("fused", dict(normal_ref=True)), ("module", dict(loss_kwargs={"normal_ref": True}))):
        model = _model(ngp, 92)
        tr, loss, res, grads, n_calls = _one_step(ngp, model, o, d, gt, kw, {}, 93)
        runs[name] = (loss, res, grads)
        assert n_calls == ({k: 1 for k in NEW} if name == "fused" else {k: 0 for k in NEW}), (name, n_calls)
        assert model.second_order_normals is (name == "fused") and model.differentiable_normals is (name == "module")
    assert "loss_terms" not in runs["default"][1]
    (la, ra, ga), (lb, rb, gb) = runs["fused"], runs["module"]
    lt = N(ra["loss_terms"]).astype(np.float64)
    assert lt.shape == (6,) and lt[4] > 0 and lt[5] > 0
    np.testing.assert_allclose(lt[0], lt[1:].sum(), rtol=2e-6)
    assert la == lt[0]
    print("FIG normal_ref trainer step: loss fused", la, "module", lb, "default", runs["default"][0], "terms", lt)
    np.testing.assert_allclose(la, lb, rtol=1e-4, atol=1e-9)
    fn = tr.loss_fn
    np.testing.assert_allclose(lt[4], fn.lambda_normal_ref_rp * float(rb["Rp"].mean()), rtol=1e-4)
    np.testing.assert_allclose(lt[5], fn.lambda_normal_ref_ro * float(rb["Ro"].mean()), rtol=1e-4)
    for name in ga:
        scale, err = np.abs(gb[name]).max(), np.abs(ga[name] - gb[name]).max()
        print(f"FIG normal_ref trainer step grad {name}: max|a - b| {err:.3g}, largest entry {scale:.3g}")
        assert err <= 3e-4 * scale + 1e-12, (name, err, scale)
    # without the terms the normal head gets no gradient at all
    gd = runs["default"][2]
    assert not gd["norm_pred_header.params"].any() and np.abs(ga["norm_pred_header.params"]).max() > 0


@pytest.mark.parametrize("recipe", ["kitti", "depth"])
def test_one_step_with_multi_terms(ngp, recipe):
    """multi_terms=('semantic', 'normal_mono') + embedding_a + random_bg (the street-scene recipe) and ('depth_mono',): ten
    terms, the two ref terms behind the eight, loss with both; every gradient finite"""
    from ngp_amd.rendering import MULTI_TERMS
    if recipe == "kitti":
        terms, scale, more = ("semantic", "normal_mono"), 8.0, dict(exp_step_factor=1 / 256, render_kwargs={"random_bg": True})
    else:
        terms, scale, more = ("depth_mono",), 0.5, {}
    o, d, gt, img, step_kw = _batch(1024, 95, terms=terms)
    model = _model(ngp, 96, scale=scale, embed_a=recipe == "kitti", embed_a_len=4)
    if recipe == "kitti":
        torch.manual_seed(97)
        more["embedding_a"] = torch.nn.Embedding(10, 4).to(DEV)
        step_kw["img_idxs"] = img.to(torch.int64)
    tr, loss, res, grads, n_calls = _one_step(ngp, model, o, d, gt, dict(normal_ref=True, multi_terms=terms, **more), step_kw, 98)
    assert n_calls == {k: 1 for k in NEW}
    lt = N(res["loss_terms"]).astype(np.float64)
    assert lt.shape == (10,) and np.isfinite(lt).all() and lt[8] > 0 and lt[9] > 0
    np.testing.assert_allclose(lt[0], lt[1:].sum(), rtol=2e-6)
    assert loss == lt[0]
    for k, name in enumerate(MULTI_TERMS):
        slots = {"semantic": (4, 5), "normal_mono": (6,), "depth_mono": (7,)}[name]
        if name not in terms:
            assert all(lt[s] == 0 for s in slots), name
    assert lt[4 if recipe == "kitti" else 7] > 0
    for name, g in grads.items():
        assert np.isfinite(g).all(), name
    for name in ("xyz_encoder.params", "rgb_encoder.params", "xyz_net.0.weight", "norm_pred_header.params"):
        assert np.abs(grads[name]).max() > 0, name
    if recipe == "kitti":
        assert np.abs(grads["embedding_a.weight"]).max() > 0 and np.abs(grads["semantic_header.params"]).max() > 0


def test_the_ref_terms_alone_reach_the_density_field_and_the_normal_head(ngp):
    """seeding only ref_terms: the density table, xyz_net and norm_pred_header get a gradient, rgb_net exactly none"""
    from ngp_amd.rendering import FusedTail, render
    o, d, gt, _, _ = _batch(512, 101)
    model = _model(ngp, 102)
    model.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=True)
    model.second_order_normals = True
    res = render(model, o, d, exp_step_factor=0.0, num_classes=7, _fused_loss=FusedTail(gt, 1e-3, 1e-3, normal_ref=(1e-3, 1e-3)))
    assert int(res["total_samples"]) > 0
    torch.autograd.backward([res["_ref_terms"]], [torch.ones(2, device=DEV)])
    g = {n: p.grad for n, p in model.named_parameters()}
    for name in ("xyz_encoder.params", "xyz_net.0.weight", "xyz_net.2.weight", "norm_pred_header.params", "rgb_encoder.params"):
        assert g[name] is not None and float(g[name].abs().max()) > 0, name
    assert g["rgb_net.params"] is None or not bool(g["rgb_net.params"].any())
    assert g["semantic_header.params"] is None or not bool(g["semantic_header.params"].any())
    # and without the flag on the model the tail refuses instead of leaving Ro's route out
    model.second_order_normals = False
    with pytest.raises(RuntimeError, match="second_order_normals"):
        render(model, o, d, exp_step_factor=0.0, num_classes=7, _fused_loss=FusedTail(gt, 1e-3, 1e-3, normal_ref=(1e-3, 1e-3)))


# ------------------------------------------------------------------------------------------- (f) the recipe end to end
# Half the gap of the one measured run of both tools (profiles/normal_ref.txt: 17.05 deg against 93.38 deg over the held-out
# pixels with opacity above 0.5): without the term the predicted-normal head receives no gradient at all
AGREE_MARGIN_DEG = 38.1


def test_recipe_end_to_end(ngp, tmp_path):
    """tools/train_dataset.py --make_proxy --dataset_name tnt --downsample 0.1 --proxy_views 34 (34 views of 80 x 80, every
    8th held out), 600 steps of 2 048 rays, with --normal_ref and without it on the same files: held-out PSNR above 20 dB
    (the bar the other proxy recipes carry), six loss terms, and the predicted normals agree with the density normals
    better than those of the run without the term, by half the measured gap"""
    proxy = str(tmp_path / "proxy")
    size = ["--dataset_name", "tnt", "--num_epochs", "3", "--steps_per_epoch", "200", "--batch_size", "2048"]
    ref = H._tool(["--make_proxy", proxy, "--downsample", "0.1", "--proxy_views", "34", "--normal_ref"] + size, 600)
    plain = H._tool(["--root_dir", proxy] + size, 600)
    assert ref["normal_ref"] is True and "normal_ref" not in plain and ref["steps"] == 600 and ref["img_wh"] == [80, 80]
    assert ref["loss_terms"] == 6 and len(ref["test_psnr"]) == 5 == len(plain["test_psnr"])
    assert ref["test_normal_agree_pixels"] > 1000 and plain["test_normal_agree_pixels"] > 1000
    for key in ("normal_ref_rp_term_first", "normal_ref_rp_term_last", "normal_ref_ro_term_first", "normal_ref_ro_term_last"):
        assert np.isfinite(ref[key]) and ref[key] >= 0, key
    print(f"normal_ref: held-out PSNR {ref['test_psnr_mean']:.2f} dB, normals agree within {ref['test_normal_agree_deg_mean']:.2f} deg "
          f"({ref['test_normal_agree_pixels']} pixels), Rp {ref['normal_ref_rp_term_first']:.3g} -> {ref['normal_ref_rp_term_last']:.3g}, "
          f"Ro {ref['normal_ref_ro_term_first']:.3g} -> {ref['normal_ref_ro_term_last']:.3g}; without: "
          f"{plain['test_psnr_mean']:.2f} dB, {plain['test_normal_agree_deg_mean']:.2f} deg")
    assert ref["test_psnr_mean"] > 20.0
    assert ref["test_normal_agree_deg_mean"] < plain["test_normal_agree_deg_mean"] - AGREE_MARGIN_DEG
