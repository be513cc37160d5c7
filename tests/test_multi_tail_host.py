"""Host-side checks of the combined semantic + normal_mono + depth_mono training route (no GPU): the restatement by
increments (tests/multi_tail_reference.py) against ONE float64 autograd pass over the whole sum of terms, the promises of
the sibling suites' inputs on the widened, combined batch, the argument checks of ngp_render_loss_fused_multi, the
trainer's refusals, step()'s argument checks and the new flag of tools/train_dataset.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multi_tail_reference as M
from multi_tail_reference import DR, NR, R, SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
ROUNDING = 16           # bar of the increments-against-one-pass comparison, in eps64 of the tensor's largest entry: both sides
#                         form every entry from the same at most four shares (default, sky, normal, depth), each computed by
#                         the same operations; they differ in the order the shares are added (3 roundings each side) and in
#                         the subtraction that isolates an increment (2 per term)
CLASSES_SEM, CLASSES_PLAIN = (1, 5, 7, 8, 9, 10, 16), (0, 7, 8)
_X = {}


def inputs(name):
    """(batch, {labels by class count}, normals, depths) of a combined batch, computed once"""
    if name not in _X:
        x = M.make_batch(name)
        _X[name] = (x, {c: M.make_labels(x, c) for c in CLASSES_SEM}, M.make_normals(x), M.make_depths(x))
    return _X[name]


def whole_pass(x, named, targets, classes, scene_scale=1.0, use_bg=True, **render_cfg):
    """the whole loss (default recipe + every named term) as ONE float64 graph on one render() state, its gradients by one
    autograd call -> dict(terms (8), d_sig, d_rgb, d_sem, d_np), laid out as the restatement lays them out"""
    st = R.render(x, classes=classes, **render_cfg)
    dt = st["dtype"]
    t = lambda a: torch.from_numpy(np.array(a)).to(dt)
    rays_a = st["rays_a"]
    rays = torch.from_numpy(rays_a[:, 0].copy())
    rows = len(rays_a)
    O, Cc, dist, D = st["opacity"], st["rgb_fg"], st["dist"], st["depth"]
    rgb = Cc + t(x["bg"]) * (1 - O)[:, None] if use_bg else Cc
    o = O + 1e-10
    terms = [((rgb - t(x["gt"])[rays]) ** 2).mean(), R.LAMBDA_O * (-o * torch.log(o)).mean(), R.LAMBDA_D * dist.mean()]
    zero = D.sum() * 0
    row_of = M.owned(x)[0]
    seg, own = torch.from_numpy(np.maximum(row_of, 0)), torch.from_numpy(row_of >= 0)
    w = torch.from_numpy(np.nan_to_num(st["ws"])).to(dt)          # detached weights, 0 behind the stop
    logits = t(x["sem"][:, :classes]).requires_grad_(True)
    head = t(x["nrm"][:, :3]).requires_grad_(True)
    ce = sky = nm = dm = zero
    f32 = lambda v: float(np.float32(v))
    if "semantic" in named:
        lab = np.asarray(targets["labels"], np.int64)[rays_a[:, 0]]
        S = torch.zeros(rows, classes, dtype=dt).index_add(0, seg, torch.where(own[:, None], w[:, None] * torch.softmax(logits, -1), 0.0))
        ce = SR.ce_term(S, lab, classes, f32(SR.LAMBDA_SEM))
        sky = f32(SR.LAMBDA_SKY) * (torch.from_numpy(lab == SR.SKY).to(dt) * torch.exp(-D)).mean()
    if "normal_mono" in named:
        g = t(np.asarray(targets["normals"], np.float32)[rays_a[:, 0]])
        Nn = torch.zeros(rows, 3, dtype=dt).index_add(0, seg, torch.where(own[:, None], w[:, None] * -F.normalize(head, dim=-1, eps=1e-6), 0.0))
        nm = NR.normal_term(Nn, g, f32(NR.LAMBDA_NM))[0]
    if "depth_mono" in named:
        z = t(np.asarray(targets["depths"], np.float32)[rays_a[:, 0]]) / 25
        valid = z > 0
        dm = DR.depth_term(D, torch.where(valid, z, torch.zeros_like(z)), valid, f32(DR.LAMBDA_DM), f32(scene_scale))[0]
    loss = sum(terms) + ce + sky + nm + dm
    g_sig, g_rgb, g_log, g_head = torch.autograd.grad(loss, [st["sig"], st["rgbs"], logits, head], allow_unused=True)
    num = lambda v, like: np.zeros(tuple(like.shape)) if v is None else v.detach().numpy()
    own = own.numpy()
    return dict(terms=np.array([float(v.detach()) for v in [loss] + terms + [ce, sky, nm, dm]]),
                d_sig=np.where(own, num(g_sig, st["sig"]), np.nan), d_rgb=np.where(own[:, None], num(g_rgb, st["rgbs"]), np.nan),
                d_sem=np.where(own[:, None], num(g_log, logits), np.nan), d_np=np.where(own[:, None], num(g_head, head), np.nan))


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("mask", sorted(M.MASKS))
@pytest.mark.parametrize("name,classes,cfg", [("crafted", 7, {}), ("crafted", 16, dict(T_thr=1e-2, use_scale=True)),
                                              ("300", 9, {})])
def test_increments_equal_one_autograd_pass(name, classes, cfg, mask):
    """d_sig as the default recipe's plus the named terms' increments, d_sem, d_np and the 8 terms equal one float64 autograd
    pass over the whole sum, to ROUNDING * eps64 of each tensor's largest entry"""
    named = M.MASKS[mask]
    x, labels, normals, depths = inputs(name)
    targets = dict(labels=labels[classes], normals=normals, depths=depths)
    scale = 0.5 if name == "crafted" else 8.0
    ref = M.evaluate(x, named, targets, classes=classes, scene_scale=scale, **cfg)
    one = whole_pass(x, named, targets, classes, scene_scale=scale, **cfg)
    assert ref["terms"].shape == (8,)
    for i, term in ((4, "semantic"), (5, "semantic"), (6, "normal_mono"), (7, "depth_mono")):
        assert (ref["terms"][i] != 0) == (term in named), (i, ref["terms"])
    for key in ("terms", "d_sig", "d_rgb") + (("d_sem",) if "semantic" in named else ()) + (("d_np",) if "normal_mono" in named else ()):
        a, b = ref[key], one[key]
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        top = np.nanmax(np.abs(b))
        err = np.nanmax(np.abs(a - b))
        print(f"FIG increments {name} classes={classes} mask={mask} {key}: max|diff| {err:.3g}, bar {ROUNDING * EPS64 * top:.3g} "
              f"({ROUNDING} eps64 of {top:.3g})")
        assert err <= ROUNDING * EPS64 * top, (key, err, top)
    if "semantic" not in named:
        assert "d_sem" not in ref and not np.nan_to_num(one["d_sem"]).any()
    if "normal_mono" not in named:
        assert "d_np" not in ref and not np.nan_to_num(one["d_np"]).any()


def test_single_masks_are_the_single_restatements():
    x, labels, normals, depths = inputs("crafted")
    targets = dict(labels=labels[7], normals=normals, depths=depths)
    for mask, single in ((1, SR.evaluate(x, labels[7], classes=7)), (2, NR.evaluate(x, normals)), (4, DR.evaluate(x, depths))):
        ref = M.evaluate(x, M.MASKS[mask], targets)
        np.testing.assert_allclose(ref["d_sig"], single["d_sig"], rtol=0, atol=4 * EPS64 * np.nanmax(np.abs(single["d_sig"])))
        slot = {1: [4, 5], 2: [6], 4: [7]}[mask]
        assert np.array_equal(ref["terms"][slot], single["terms"][4:])
        assert not np.delete(ref["terms"][4:], np.array(slot) - 4).any()
        np.testing.assert_allclose(ref["terms"][0], single["terms"][0], rtol=4 * EPS64)
    noise = M.fp32_error(x, M.TERMS, targets, scene_scale=0.5)
    assert 0 < noise["d_sig"] and 0 < noise["d_sem"] and 0 < noise["d_np"] and (noise["fit"] < 1e-6).all()
    assert noise["terms"].shape == (8,)


# ------------------------------------------------------------------------------------------- the inputs' promises
@pytest.mark.parametrize("name", ["crafted", "300", "1500"])
def test_inputs_keep_the_siblings_promises(name):
    """on the widened, combined batch: nothing borderline in the crafted batch, at most MAX_BORDERLINE of the random ones
    left out; no component of N^ - g^ nearer to 0 than SIGN_MARGIN; var(D) / mean(D^2) >= MIN_SPREAD over the valid rays
    of the batch and of the 7 / 8 / 9-row prefixes; every kind of label, normal and depth present; a sky ray with a valid
    depth for every class count of the GPU sweep"""
    x, labels, normals, depths = inputs(name)
    assert x["sem"].shape == (x["n"], 16)
    assert np.array_equal(x["sem"][:, :8], (M.make_crafted(0) if name == "crafted" else M.make_random(int(name)))["sem"])
    if name == "crafted":
        for T_thr in (1e-4, 1e-2):
            assert M.comparable(x, T_thr, 1e-2)[0].all()
    else:
        left_out = 1.0 - M.comparable(x, 1e-4, 1e-3)[0].mean()
        print(f"FIG inputs {name}: borderline share {left_out:.4f}")
        assert left_out <= M.MAX_BORDERLINE
    rows = x["rays_a"][:, 0]
    margin = NR.sign_margin(x, normals)
    print(f"FIG inputs {name}: sign margin {margin:.3g}")
    assert margin >= NR.SIGN_MARGIN
    g = normals[rows]
    assert (g == 0).all(1).any() and (g != 0).any(1).sum() > len(rows) // 2 and not (g[:2] == 0).all(1).any()
    D = R.render(x)["depth"].detach().numpy()
    z = depths[rows]
    ok = z / np.float32(25) > 0
    assert (z == 0).any() and (z < 0).any() and np.isnan(z).any() and ok[0] and ok[1]
    for p in (len(D),) + DR.PREFIXES:
        s = DR.spread(D[:p], ok[:p])
        print(f"FIG inputs {name} rows={p}: spread {s:.3f}")
        assert s >= DR.MIN_SPREAD, (name, p, s)
    for classes, lab in labels.items():
        lr = lab[rows]
        valid = (lr >= 0) & (lr < classes)
        assert valid.any() and (~valid).any() and set(SR.SPECIAL) <= set(lr.tolist())
        sky = M.sky_rows_with_depth(x, lab, depths)
        assert len(sky) >= 1, (name, classes)


def test_crafted_normals_hold_the_margin_at_both_thresholds():
    """the crafted batch is compared at T_threshold 1e-4 and 1e-2, which moves the stop samples and with them N^: the
    targets are drawn per threshold (multi_tail_reference.make_normals), and scale3 does not enter N^"""
    x = inputs("crafted")[0]
    for T_thr in (1e-4, 1e-2):
        normals = M.make_normals(x, T_thr=T_thr)
        for use_scale in (False, True):
            assert NR.sign_margin(x, normals, T_thr=T_thr, use_scale=use_scale) >= NR.SIGN_MARGIN, (T_thr, use_scale)
        D = R.render(x, T_thr=T_thr)["depth"].detach().numpy()
        ok = inputs("crafted")[3][x["rays_a"][:, 0]] / np.float32(25) > 0
        for p in (len(D),) + DR.PREFIXES:
            assert DR.spread(D[:p], ok[:p]) >= DR.MIN_SPREAD, (T_thr, p)


# ------------------------------------------------------------------------------------------- the C entry
def test_c_entry_checks_its_arguments(ngp):
    """a zero mask with rays to process, unknown bits, classes out of range for the mask, a scene scale that is not positive with the depth term,
    leading dimensions, a negative ray count: NGP_EINVAL; an empty batch: NGP_OK before any pointer is looked at (every
    pointer is NULL here: nothing may reach a launch)"""
    _lib = ngp._lib
    lib = _lib.load()
    assert "ngp_render_loss_fused_multi" in _lib.PROTOS
    _, args = _lib.PROTOS["ngp_render_loss_fused_multi"]
    names = [a for _, a in args]
    extras = ["term_mask", "labels", "lambda_sem", "lambda_sky", "normals_gt", "lambda_nm", "depth_gt", "lambda_dm",
              "scene_scale", "multi_ws", "dL_dsem_logits", "dL_dnormal_head"]
    _, plain = _lib.PROTOS["ngp_render_loss_fused"]
    assert [a for a in names if a not in extras] == [a for _, a in plain]
    i = names.index("rgb_bg")
    assert names[i + 1:i + 11] == extras[:9] + ["T_threshold"]
    assert names[-4:] == ["multi_ws", "dL_dsem_logits", "dL_dnormal_head", "stream"]

    def run(mask, classes, n_rays, ld_sem=16, ld_normal=3, scale=1.0):
        vals = []
        for t, a in args:
            if t is C.c_void_p:
                vals.append(None)
            elif t is C.c_float:
                vals.append(scale if a == "scene_scale" else 1.0)
            else:
                vals.append({"classes": classes, "n_rays": n_rays, "ld_normal": ld_normal, "ld_sem": ld_sem, "term_mask": mask}[a])
        return lib.ngp_render_loss_fused_multi(*vals)
    OK, EINVAL = 0, -22
    for n_rays in (0, 5):
        for mask in (8, 9, 15, -1, 1 << 20):
            assert run(mask, 7, n_rays) == EINVAL, mask
        # a zero mask is refused with rays to process; an empty batch is NGP_OK whatever it names (the rule of
        # tests/test_cabi_and_host.py for every entry that takes a batch size)
        assert run(0, 7, n_rays) == (EINVAL if n_rays else OK) and run(0, 7, -1) == EINVAL and run(0, 9, n_rays) == EINVAL
        for mask in range(1, 8):
            sem, dep = mask & 1, mask & 4
            assert run(mask, 17, n_rays) == EINVAL and run(mask, -1, n_rays) == EINVAL
            assert run(mask, 9, n_rays) == (EINVAL if not sem or n_rays else OK), mask
            assert run(mask, 0, n_rays) == (EINVAL if sem or n_rays else OK), mask
            assert run(mask, 7, n_rays, ld_normal=2) == EINVAL and run(mask, 7, n_rays, ld_sem=6) == EINVAL
            for bad in (0.0, -1.0, float("nan")):
                assert run(mask, 7, n_rays, scale=bad) == (EINVAL if dep or n_rays else OK), (mask, bad)
            assert run(mask, 7, -1) == EINVAL
            assert run(mask, 7, n_rays) == (EINVAL if n_rays else OK)          # NULL pointers with rays to process
    assert run(7, 16, 0) == OK and run(1, 1, 0) == OK and run(6, 8, 0) == OK
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    for line in ("#define NGP_MULTI_WS_INTS 30", "#define NGP_TERM_SEM 1", "#define NGP_TERM_NRM 2", "#define NGP_TERM_DEP 4",
                 "#define NGP_MULTI_WS_LABELS_NVALID 0", "#define NGP_MULTI_WS_FIT_A 24", "#define NGP_MULTI_WS_FIT_B 25",
                 "#define NGP_MULTI_WS_FIT_NVALID 26"):
        assert line in header, line
    assert 30 % 2 == 0 and 30 == 8 + 4 + 18          # 8-byte aligned: the three single workspaces back to back
    from ngp_amd import rendering
    assert rendering.MULTI_WS_INTS == 30 and rendering.MULTI_TERMS == M.TERMS


# ------------------------------------------------------------------------------------------- the trainer
class _Head:
    n_output_dims = 7


class _Model:          # what the construction checks look at
    rgb_act, use_skybox, differentiable_normals = "Sigmoid", False, False
    semantic_header = _Head()


ALL = ("semantic", "normal_mono", "depth_mono")


def test_trainer_refuses_what_the_multi_tail_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    refused = [dict(msk_model=implicit_mask()), dict(pose_refiner=object()), dict(semantic=True), dict(normal_mono=True),
               dict(depth_mono=True), dict(render_kwargs={"use_skybox": True}), dict(loss_kwargs={"normal_mono": True}),
               dict(loss_kwargs={"semantic": True}), dict(loss_kwargs={"depth_mono": True}),
               dict(loss_kwargs={"normal_ref": True}), dict(loss_kwargs={"embed_msk": True}), dict(num_classes=9),
               dict(num_classes=17), dict(num_classes=0)]
    for kw in refused:
        model = _Model()
        with pytest.raises(ValueError):
            NGPTrainer(model, multi_terms=ALL, **kw)
        assert model.differentiable_normals is False
    for attr, value in (("rgb_act", "None"), ("use_skybox", True), ("differentiable_normals", True)):
        for terms in (ALL, ("normal_mono", "depth_mono"), ("depth_mono",)):
            model = _Model()
            setattr(model, attr, value)
            with pytest.raises(ValueError, match="multi_terms="):
                NGPTrainer(model, multi_terms=terms)
    for bad in (("semantic", "semantic"), ("sky",), ("semantic", "normal_ref"), "normal_ref"):
        with pytest.raises(ValueError, match="multi_terms"):
            NGPTrainer(_Model(), multi_terms=bad)
    # without the semantic term the head's width is not looked at, but the tail's 8 classes are
    with pytest.raises(ValueError, match="above 8"):
        NGPTrainer(_Model(), multi_terms=("normal_mono", "depth_mono"), num_classes=9)
    # the three single flags still refuse one another
    for kw in (dict(semantic=True, normal_mono=True), dict(semantic=True, depth_mono=True), dict(normal_mono=True, depth_mono=True)):
        with pytest.raises(ValueError):
            NGPTrainer(_Model(), **kw)


def test_step_checks_the_targets(ngp):
    """step()'s checks come before anything touches the device: exactly the named terms' targets, their shapes and dtypes,
    no target= and no per-step loss term, CUDA tensors; the default recipe keeps the single flags' messages"""
    from ngp_amd.recipe import Recipe
    from ngp_amd.trainer import NGPTrainer

    class _Trainer:          # what step() looks at before its first launch
        model = None

        def __init__(self, **options):
            self.recipe = Recipe(**options) if options else Recipe(multi_terms=ALL)
    o, d, gt = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, 3)
    lab, nrm, dep = torch.zeros(6, dtype=torch.int64), torch.ones(6, 3), torch.ones(6)
    full = dict(labels=lab, normals=nrm, depths=dep)
    for missing in full:
        with pytest.raises(ValueError, match=f"needs {missing}="):
            NGPTrainer.step(_Trainer(), o, d, gt, **{k: v for k, v in full.items() if k != missing})
    for bad in (nrm[:5], nrm.reshape(-1), nrm.to(torch.int64)):
        with pytest.raises(ValueError, match="normals= must be"):
            NGPTrainer.step(_Trainer(), o, d, gt, **dict(full, normals=bad))
    for bad in (dep[:5], dep.reshape(6, 1), dep.to(torch.int64)):
        with pytest.raises(ValueError, match="depths= must be"):
            NGPTrainer.step(_Trainer(), o, d, gt, **dict(full, depths=bad))
    with pytest.raises(ValueError, match="labels= must hold"):
        NGPTrainer.step(_Trainer(), o, d, gt, **dict(full, labels=lab[:5]))
    with pytest.raises(ValueError, match="no target="):
        NGPTrainer.step(_Trainer(), o, d, gt, target={"depth": dep}, **full)
    with pytest.raises(ValueError, match="no target="):
        NGPTrainer.step(_Trainer(), o, d, gt, scale=2.0, **full)
    with pytest.raises(RuntimeError, match="CUDA"):
        NGPTrainer.step(_Trainer(), o, d, gt, **full)
    # a target of a term that is not named is refused with the single flags' message
    two = _Trainer(multi_terms=("normal_mono", "depth_mono"))
    with pytest.raises(ValueError, match="labels= is for"):
        NGPTrainer.step(two, o, d, gt, **full)
    with pytest.raises(RuntimeError, match="CUDA"):
        NGPTrainer.step(two, o, d, gt, normals=nrm, depths=dep)

    class _Old:          # the default recipe
        model, recipe = None, Recipe()
    for kw, msg in ((dict(labels=lab), "labels= is for"), (dict(normals=nrm), "normals= is for"), (dict(depths=dep), "depths= is for")):
        with pytest.raises(ValueError, match=msg):
            NGPTrainer.step(_Old(), o, d, gt, **kw)


# ------------------------------------------------------------------------------------------- the tool's flag
def test_train_dataset_flag(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    assert td.parse_args(["--root_dir", "x"]).multi_terms == ()
    a = td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--multi_terms", "depth_mono", "semantic", "normal_mono",
                       "--embed_a", "--random_bg", "--num_classes", "5", "--lambda_depth_mono", "0.5", "--proxy_views", "34"])
    assert a.multi_terms == ALL and a.scale == 2.0 and a.num_classes == 5 and a.lambda_depth_mono == 0.5 and a.proxy_views == 34
    assert not (a.render_semantic or a.normal_mono or a.depth_mono)
    a = td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--multi_terms", "normal_mono", "depth_mono"])
    assert a.multi_terms == ("normal_mono", "depth_mono") and a.scale == 0.5
    assert td.parse_args(["--root_dir", "x", "--dataset_name", "tnt", "--multi_terms", "semantic"]).scale == 0.5
    base = ["--root_dir", "x", "--dataset_name", "tnt", "--multi_terms", "semantic", "normal_mono"]
    for bad in (base + ["--render_semantic"], base + ["--normal_mono"], base + ["--depth_mono"], base + ["--embed_msk"],
                base + ["--optimize_ext"], ["--root_dir", "x", "--multi_terms"], ["--root_dir", "x", "--multi_terms", "normal_ref"],
                ["--make_proxy", "d", "--multi_terms", "semantic"],
                ["--make_proxy", "d", "--dataset_name", "colmap", "--multi_terms", "semantic", "depth_mono"],
                # the single flags' mutual refusals stay
                ["--root_dir", "x", "--dataset_name", "tnt", "--depth_mono", "--normal_mono"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--render_semantic", "--normal_mono"]):
        with pytest.raises(SystemExit) as e:
            td.parse_args(bad)
        assert e.value.code == 2, bad

    class _Set:          # a dataset that lacks one of the maps is refused before anything else is looked at
        batch_size = 0
    for terms, word in ((("depth_mono", "normal_mono"), "depth"), (("semantic", "normal_mono"), "normals")):
        with pytest.raises(ValueError, match=word):
            td.train(None, _Set(), 1, 1, 64, 1e-2, multi_terms=terms)
    with pytest.raises(ValueError, match="multi_terms"):
        td.train(None, _Set(), 1, 1, 64, 1e-2, multi_terms=ALL, semantic=True)
    log = [torch.tensor([9.0, 1, 1, 1, 4.0 - 0.1 * i, 0.5, 2.0, 0.0]) for i in range(30)]
    s = td.multi_terms_summary(log)
    assert set(s) == {"CELoss", "sky_depth", "normal_mono", "depth_mono"}
    assert s["CELoss"] == (pytest.approx(3.55), pytest.approx(1.55)) and s["sky_depth"] == (0.5, 0.5) and s["depth_mono"] == (0.0, 0.0)


def test_proxy_with_all_maps(ngp, tmp_path):
    """--make_proxy with --multi_terms writes labels, normals and depth maps together in the tnt layout, and the loader
    reads the three with the matching switches"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd.datasets import dataset_dict
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=9, img_wh=(16, 16), device="cpu")
    root = td.make_proxy_with_all_maps(str(tmp_path / "tnt"), scene, n_quad=64)
    for sub in ("semantic", "normal", "depth"):
        assert len(os.listdir(os.path.join(root, sub))) == 9, sub
    train_set = dataset_dict["tnt"](root, "train", 1.0, use_sem=True, num_classes=5, normal_mono=True, depth_mono=True)
    assert hasattr(train_set, "labels") and hasattr(train_set, "normals") and hasattr(train_set, "depths_2d")
    train_set.batch_size = 32
    s = train_set[0]
    assert tuple(s["label"].shape)[:1] == (32,) and tuple(s["normal"].shape) == (32, 3) and tuple(s["depth"].shape) == (32,)
