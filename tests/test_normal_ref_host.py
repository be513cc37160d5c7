"""normal_ref on the fused field and tail without a GPU: the closed forms of ngp_density_head_bwd2 and ngp_normal_ref_tail
(normal_ref_reference.py) against torch.autograd on the plain definitions in float64, the cases the GPU tests are built
on, the trainer's and the tool's refusals on stand-ins, and the C interface's declarations and host-side answers."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import normal_ref_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------- the closed forms
@pytest.mark.parametrize("with_g", [True, False])
def test_head_closed_forms_match_autograd(with_g):
    """m, e1, dW2, db2 as the header states them against two autograd.grad calls on the head's plain definition"""
    rng = np.random.default_rng(7)
    n, H = 37, 128
    z1, w2, b2 = rng.standard_normal((n, H)) * 1.5, rng.standard_normal(H) * 0.3, rng.standard_normal(1)
    r, g = rng.standard_normal((n, H)), (rng.standard_normal(n) if with_g else None)
    want = R.head_definition(z1, w2, b2, r, g)
    got = R.head_closed(want["a1"], want["sig"], r, w2, g)
    for k in R.HEAD_KEYS:
        assert got[k].shape == want[k].shape and np.abs(want[k]).max() > 0
        assert rel(got[k], want[k]) <= 1e-12, (k, rel(got[k], want[k]))


def test_head_closed_forms_keep_their_digits_near_saturation():
    """the float32 evaluation of the closed forms (the GPU tests' floor) stays at float32's own precision on rows at 1e-6
    and at 30, where 1 - exp(-y) and s (1 - s) of a rounded s lose every digit"""
    for kind in ("tiny", "large"):
        for with_g in (False, True):
            a1, sig, r, w2, g = R.head_case(kind, 40, 3, with_g)
            r64, r32 = R.head_closed(a1, sig, r, w2, g), R.head_closed(a1, sig, r, w2, g, dtype=torch.float32)
            for k in R.HEAD_KEYS:   # (the two sums of a both-signed case cancel: their float32 order costs more)
                bar = 5e-6 if k in ("m", "e1") else 1e-3
                assert np.abs(r64[k]).max() > 0 and rel(r32[k], r64[k]) < bar, (kind, with_g, k, rel(r32[k], r64[k]))
    a1, sig, r, w2, _ = R.head_case("large", 40, 3, False)
    s2 = 1.0 - np.exp(-sig.astype(np.float32))
    assert not (s2 * (1.0 - s2)).any()          # what the naive form leaves of q's share of e2


def test_head_positive_case_is_one_signed():
    a1, sig, r, w2, g = R.head_case("positive", 64, 1)
    ref = R.head_closed(a1, sig, r, w2, g)
    assert min(a1.min(), r.min(), w2.min(), g.min()) > 0 and ref["dW2"].min() > 0 and ref["db2"][0] > 0 and ref["e1"].min() > 0


@pytest.mark.parametrize("scale", [0.5, 8.0])
def test_tail_closed_forms_match_autograd(scale):
    """the two gradients and the two terms as the header states them against autograd on lambda_rp mean(Rp) + lambda_ro
    mean(Ro); and the case holds what the GPU test promises"""
    c = R.tail_case(scale)
    lam = (1e-3, 2e-3)
    want, got = R.tail_definition(c, *lam), R.tail_closed(c, *lam)
    for k in R.TAIL_KEYS:
        assert rel(got[k], want[k]) <= 1e-12, (k, rel(got[k], want[k]))
    lens = [int(n) for n in c["rays_a"][:, 2]]
    assert {0, 1, 32, 33, 70} <= set(lens) and R.TAIL_OMITTED not in c["rays_a"][:, 0] and len(c["omitted_rows"]) > 0
    assert not want["d_grads"][c["omitted_rows"]].any() and not want["d_head"][c["omitted_rows"]].any()
    stopped = np.flatnonzero(c["ws"] == 0)
    assert len(stopped) >= 20 and not want["d_grads"][stopped].any() and not want["d_head"][stopped].any()
    # exact zeros in both inputs, and no other row near eps
    assert not c["dsig"][c["zero_g"]].any() and not c["head"][c["zero_h"]].any()
    live_g, live_h = np.ones(c["N"], bool), np.ones(c["N"], bool)
    live_g[c["zero_g"]], live_h[c["zero_h"]] = False, False
    assert np.linalg.norm(c["dsig"] * c["scale3"], axis=1)[live_g].min() >= 1e-3
    assert np.linalg.norm(c["head"], axis=1)[live_h].min() >= 1e-3
    # rows that face away from the ray: no Ro gradient at all (lambda_rp = 0 leaves only Ro's)
    only_o = R.tail_definition(c, 0.0, 2e-3)
    n_raw = -(c["dsig"] * c["scale3"]).astype(np.float64)
    away = (n_raw * c["dirs"]).sum(1) < 0
    named = np.zeros(c["N"], bool)
    named[c["named_rows"]] = True
    assert (away & named & (c["ws"] > 0)).sum() > 20 and not only_o["d_grads"][away].any()
    assert np.abs(only_o["d_grads"][~away & named]).max() > 0 and not only_o["d_head"].any()
    # the eps branch: a zero row's gradient is -g 1e6
    assert np.abs(want["d_head"][c["zero_h"]]).max() > 1e3 * np.abs(np.delete(want["d_head"], c["zero_h"], 0)).max()


# ------------------------------------------------------------------------------------------- the trainer
class _Head:
    n_output_dims = 7


class _Model:          # what the construction checks look at
    rgb_act, use_skybox, differentiable_normals = "Sigmoid", False, False
    semantic_header = _Head()


def test_trainer_refuses_what_normal_ref_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    head = "normal_ref=True runs on the fused field node and the fused render \\+ loss tail, which do not take "
    tone, dn, sky = _Model(), _Model(), _Model()
    tone.rgb_act, dn.differentiable_normals, sky.use_skybox = "None", True, True
    for model, kw, what in ((_Model(), dict(msk_model=implicit_mask()), "a msk_model"),
                            (_Model(), dict(pose_refiner=object()), "a pose_refiner"),
                            (sky, {}, "a skybox"), (_Model(), dict(render_kwargs={"use_skybox": True}), "a skybox"),
                            (tone, {}, "rgb_act != 'Sigmoid'"), (dn, {}, "differentiable normals"),
                            (_Model(), dict(semantic=True), "semantic=True"),
                            (_Model(), dict(normal_mono=True), "normal_mono=True"),
                            (_Model(), dict(depth_mono=True), "depth_mono=True"),
                            (_Model(), dict(loss_kwargs={"normal_ref": True}), "an optional term in loss_kwargs"),
                            (_Model(), dict(loss_kwargs={"normal_mono": True}), "an optional term in loss_kwargs"),
                            (_Model(), dict(force_sharded=True), "more than one rank")):
        with pytest.raises(ValueError, match=head + ".*" + what):
            NGPTrainer(model, normal_ref=True, **kw)
        assert not getattr(model, "second_order_normals", False)
    with pytest.raises(ValueError, match="use_exposure=True|rgb_act"):
        NGPTrainer(tone, normal_ref=True, use_exposure=True)
    # inside multi_terms the name stays refused
    with pytest.raises(ValueError, match="multi_terms is a subset"):
        NGPTrainer(_Model(), normal_ref=True, multi_terms=("semantic", "normal_ref"))


def test_step_checks_come_before_the_device(ngp):
    from ngp_amd.recipe import Recipe
    from ngp_amd.trainer import NGPTrainer

    class _Ref:          # what step() looks at before its first launch
        model, recipe = None, Recipe(normal_ref=True)
        warmup_steps, global_step = 256, 0
    o, d, gt = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, 3)
    with pytest.raises(ValueError, match="normal_ref=True: the step stays on the fused render \\+ loss tail"):
        NGPTrainer.step(_Ref(), o, d, gt, target={"normal": gt})
    with pytest.raises(ValueError, match="normal_ref=True: the step stays on the fused render \\+ loss tail"):
        NGPTrainer.step(_Ref(), o, d, gt, normal_mono=True)
    with pytest.raises(RuntimeError, match="normal_ref=True needs CUDA tensors"):
        NGPTrainer.step(_Ref(), o, d, gt)


def test_model_and_tail_side(ngp):
    from ngp_amd.rendering import FusedTail, _fused_tail_ok
    model = ngp.networks.NGP(scale=0.5)
    assert model.second_order_normals is False and model.differentiable_normals is False
    model.second_order_normals = True
    assert _fused_tail_ok(model, {}, 0.0, 7)                  # the fused tail stays the route
    with pytest.raises(RuntimeError, match="second_order_normals needs the density path"):
        model(torch.zeros(4, 3), torch.ones(4, 3))            # no GPU: refused with a message, never a silent other route
    gt = torch.zeros(4, 3)
    t = FusedTail(gt, 1e-3, 1e-3, normal_ref=(1e-3, 2e-3))
    assert t.normal_ref == (1e-3, 2e-3) and t.entry == "default" and t.symbol == "render_loss_fused"
    assert FusedTail(gt, 1e-3, 1e-3).normal_ref is None
    t = FusedTail(gt, 1e-3, 1e-3, terms={"depth_mono": (torch.zeros(4), 1.0, 0.5)}, normal_ref=(1.0, 1.0))
    assert t.entry == "multi" and t.normal_ref == (1.0, 1.0)
    for kw in (dict(sky=True), dict(mask=torch.zeros(4))):
        with pytest.raises(ValueError, match="normal_ref goes behind"):
            FusedTail(gt, 1e-3, 1e-3, normal_ref=(1.0, 1.0), **kw)


# ------------------------------------------------------------------------------------------- the tools' flags
def test_tool_flags(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    a = td.parse_args(["--make_proxy", "x", "--dataset_name", "tnt", "--normal_ref"])
    assert a.normal_ref and not td.parse_args(["--root_dir", "x"]).normal_ref
    a = td.parse_args(["--root_dir", "x", "--normal_ref", "--multi_terms", "semantic", "normal_mono", "--embed_a", "--random_bg"])
    assert a.normal_ref and a.multi_terms == ("semantic", "normal_mono")
    for bad in (["--embed_msk"], ["--optimize_ext"], ["--render_semantic"], ["--normal_mono"], ["--depth_mono"],
                ["--use_exposure"], ["--use_skybox"], ["--multi_terms", "normal_ref"]):
        with pytest.raises(SystemExit) as ex:
            td.parse_args(["--root_dir", "x", "--normal_ref"] + bad)
        assert ex.value.code == 2
    with pytest.raises(SystemExit) as ex:
        td.parse_args(["--root_dir", "x", "--multi_terms", "normal_ref"])
    assert ex.value.code == 2
    log = [torch.tensor([9.0, 1, 1, 1, float(i), 2.0 * i]) for i in range(40)]
    assert td.normal_ref_summary(log) == {"normal_ref_rp": (4.5, 34.5), "normal_ref_ro": (9.0, 69.0)}
    acc = td.NormalAgreement()
    assert acc.value() == (None, 0)
    up, side = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]
    acc(0, None, {"opacity": torch.tensor([1.0, 0.9, 0.1]), "normal_pred": torch.tensor([up, up, up]),
                  "normal_raw": torch.tensor([up, side, side])})
    deg, n = acc.value()
    assert n == 2 and abs(deg - 45.0) < 1e-4


# ------------------------------------------------------------------------------------------- the C interface
def test_entries_are_declared_and_built(ngp):
    from ngp_amd import _lib, build
    assert "density_bwd2_kernels.hip" in [s for s, _ in build.SOURCES]
    head, ws, tail = (_lib.PROTOS[k] for k in ("ngp_density_head_bwd2", "ngp_density_head_bwd2_workspace", "ngp_normal_ref_tail"))
    assert [n for _, n in head[1]] == ["a1", "sig", "r", "W2", "d_sig", "n", "m", "e1", "dW2", "db2", "workspace", "stream"]
    assert [n for _, n in ws[1]] == ["n"]
    assert [n for _, n in tail[1]] == ["dsigma_dx", "scale3", "normal_head", "ld_normal_head", "dirs", "ws", "rays_a", "n_rays",
                                       "loss_o", "loss_p", "lambda_rp", "lambda_ro", "add_to_normal_head", "dL_dgrads",
                                       "dL_dnormal_head", "ref_terms", "stream"]
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    rows = int(re.search(r"#define NGP_DENSITY_BWD2_ROWS (\d+)", hdr).group(1))
    blocks = int(re.search(r"#define NGP_DENSITY_BWD2_MAX_BLOCKS (\d+)", hdr).group(1))
    assert rows * blocks * 2 + 1 <= 40000          # the GPU test reaches a third trip of the grid-stride loop below 40 000 rows
    # one row of 129 partial sums (doubles, counted in floats) per workgroup, a workgroup per tile of `rows` rows
    per = 129 * 2
    assert [_lib.call_host("density_head_bwd2_workspace", n) for n in (0, 1, rows, rows + 1, rows * blocks, 10 ** 12, -1)] == \
        [0, per, per, 2 * per, blocks * per, blocks * per, -22]
    src = open(os.path.join(ROOT, "instant-ngp-pp_amd", "csrc", "density_bwd2_kernels.hip")).read()
    assert "atomicAdd" not in src and "printf" not in src and "asm" not in src


def test_empty_and_bad_arguments_never_launch(ngp):
    """n == 0 is NGP_OK before any pointer is looked at; n < 0, a NULL pointer or a misaligned one is NGP_EINVAL"""
    lib = ngp._lib.load()
    none = [None] * 5
    assert lib.ngp_density_head_bwd2(*none, 0, *none, None) == 0
    assert lib.ngp_density_head_bwd2(*none, -1, *none, None) == -22
    assert lib.ngp_density_head_bwd2(*none, 5, *none, None) == -22
    ok = dict(a1=1024, sig=2048, r=4096, W2=8192, d_sig=None, n=5, m=16384, e1=4096, dW2=32768, db2=65536, workspace=131072)
    names = [n for _, n in ngp._lib.PROTOS["ngp_density_head_bwd2"][1]][:-1]
    for k, v in (("a1", 1028), ("r", 4100), ("m", 16392), ("e1", 4100), ("workspace", 131076), ("sig", 2050), ("W2", None),
                 ("dW2", None), ("db2", None), ("sig", None), ("workspace", None)):
        bad = dict(ok)
        bad[k] = v
        assert lib.ngp_density_head_bwd2(*[bad[n] for n in names], None) == -22, k
    names = [n for _, n in ngp._lib.PROTOS["ngp_normal_ref_tail"][1]][:-1]
    base = {n: None for n in names}
    base.update(ld_normal_head=3, n_rays=0, lambda_rp=1.0, lambda_ro=1.0, add_to_normal_head=0)
    call = lambda **kw: lib.ngp_normal_ref_tail(*[dict(base, **kw)[n] for n in names], None)
    assert call() == 0 and call(n_rays=-1) == -22 and call(n_rays=4) == -22 and call(ld_normal_head=2) == -22
