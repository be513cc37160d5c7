"""Host-side checks of the semantic training route (no GPU): the float64 restatement of the semantic tail
(tests/semantic_tail_reference.py) against torch's own cross-entropy and against losses.NeRFLoss, the proxy scene's
analytic labels, the label metrics of evaluation.semantic_metrics, the new flags of tools/train_dataset.py and the
argument checks of ngp_render_loss_fused_sem."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import semantic_tail_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("classes", [2, 7, 10, 16])
def test_ce_term_equals_torch_cross_entropy(classes):
    """in-range labels plus 256: value and gradient w.r.t. the composited probabilities are torch's, and labels outside
    [0, classes) (255, -1, classes) count as 256"""
    g = np.random.default_rng(classes)
    P = torch.from_numpy(g.random((200, classes))).requires_grad_(True)
    lab = g.integers(0, classes, 200)
    lab[::7] = 256
    want = S.LAMBDA_SEM * torch.nn.CrossEntropyLoss(ignore_index=256)(P, torch.from_numpy(lab))
    (gw,) = torch.autograd.grad(want, [P])
    odd = lab.copy()
    odd[::7] = np.resize([255, -1, classes, 256, 300], len(odd[::7]))
    for labels in (lab, odd):
        got = S.ce_term(P, labels, classes)
        (gg,) = torch.autograd.grad(got, [P])
        assert float(got.detach()) == float(want.detach()) and torch.equal(gg, gw)
    nothing = S.ce_term(P, np.full(200, 256), classes)
    assert float(nothing.detach()) == 0.0 and not torch.autograd.grad(nothing, [P])[0].any()


@pytest.mark.parametrize("classes", [3, 7, 10])
def test_restatement_equals_nerfloss(ngp, classes):
    """the full term dictionary against losses.NeRFLoss()(..., semantic=True) fed with the restatement's own per-ray
    results (the distortion term, a HIP kernel in the package, is handed the restatement's per-ray value)"""
    x = S.widen(S.make_crafted(0))
    labels = S.mapped(S.make_labels(x["n_rays"], classes), classes)        # what torch may see
    ref = S.evaluate(x, labels, classes=classes)
    rows = x["rays_a"][:, 0]
    t = lambda a: torch.from_numpy(np.array(a))
    loss_fn = ngp.losses.NeRFLoss()
    loss_fn._distortion = lambda results: loss_fn.lambda_distortion * results["dist"]
    # the restatement weighs the two new terms with the float32 values the C entry receives
    loss_fn.lambda_semantic, loss_fn.lambda_sky = (float(np.float32(v)) for v in (loss_fn.lambda_semantic, loss_fn.lambda_sky))
    assert abs(loss_fn.lambda_semantic - 4e-2) < 1e-9 and abs(loss_fn.lambda_sky - 1e-1) < 1e-8
    results = {"rgb": t(ref["rgb"][rows]), "opacity": t(ref["opacity"][rows]), "depth": t(ref["depth"][rows]),
               "semantic": t(ref["sem"][rows]), "dist": t(ref["dist"][rows])}
    d = loss_fn(results, {"rgb": t(x["gt"][rows]).double(), "label": t(labels[rows])}, semantic=True)
    assert list(d) == ["rgb", "opacity", "distortion", "CELoss", "sky_depth"]
    means = np.array([float(v.mean()) for v in d.values()])
    np.testing.assert_allclose(ref["terms"][1:], means, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["terms"][0], means.sum(), rtol=1e-12)
    assert ref["terms"][4] > 0 and (ref["terms"][5] > 0) == bool((labels == 4).any())
    assert ref["n_valid"] == int((labels != 256).sum())
    # dCE/dS of the restatement is torch's on the same probabilities
    P = results["semantic"].clone().requires_grad_(True)
    (g,) = torch.autograd.grad(loss_fn.lambda_semantic * loss_fn.CrossEntropyLoss(P, t(labels[rows])), [P])
    np.testing.assert_allclose(ref["g_S"], g.numpy(), rtol=1e-12, atol=1e-18)


def test_restatement_gradients():
    """d_sem vanishes behind a stop and on ignored rays, sums to zero over the classes of a sample (softmax), and the sky
    term reaches d_sig only on rays labelled 4; the float32 companion stays close"""
    x = S.widen(S.make_crafted(0))
    classes = 10
    labels = S.make_labels(x["n_rays"], classes)
    assert set(S.SPECIAL) <= set(labels.tolist()) and ((labels >= 0) & (labels < classes)).sum() >= 5
    ref = S.evaluate(x, labels, classes=classes, lam_sem=1.0, lam_sky=1.0)
    base = S.evaluate(x, labels, classes=classes, lam_sem=1.0, lam_sky=0.0)
    row, k = S.owned(x)
    own = row >= 0
    stop = np.array([10 ** 6 if s is None else s for _, s in x["cases"]])
    behind = own & (k > stop[np.maximum(row, 0)])
    lab_s = labels[x["rays_a"][np.maximum(row, 0), 0]]
    ignored = own & ~((lab_s >= 0) & (lab_s < classes))
    assert np.isnan(ref["d_sem"][~own]).all() and not ref["d_sem"][behind].any() and not ref["d_sem"][ignored].any()
    live = own & ~behind & ~ignored
    assert np.abs(ref["d_sem"][live]).max() > 1e-4
    np.testing.assert_allclose(ref["d_sem"][own].sum(1), 0, atol=1e-15)
    moved = np.nan_to_num(ref["d_sig"] - base["d_sig"]) != 0
    assert moved.any() and (lab_s[moved] == 4).all()
    noise = S.fp32_error(x, labels, ref=ref, classes=classes, lam_sem=1.0, lam_sky=1.0)
    assert 0 < noise["d_sem"] < 1e-6 and noise["terms"][4] < 1e-5 and noise["terms"][5] < 1e-6


def test_label_maker_shapes():
    for classes in (1, 2, 4, 7, 16):
        lab = S.make_labels(300, classes)
        assert lab.dtype == np.int64 and set(S.SPECIAL) <= set(lab.tolist())
        assert 0.4 < ((lab >= 0) & (lab < classes)).mean() < 0.8
        none = S.make_labels(300, classes, valid=False)
        assert not ((none >= 0) & (none < classes)).any()


# ------------------------------------------------------------------------------------------- the scene's labels
def test_proxy_scene_labels(ngp):
    """34 views of 80 x 80 at n_quad = 128: every class 0-4 holds at least 2 % of the pixels, at most 5 % are ignored,
    nothing else occurs, and a ray through empty space is sky"""
    from ngp_amd.datasets import export
    from ngp_amd.synthetic import IGNORE_LABEL, SKY_LABEL, LegoProxy, analytic_part, analytic_sigma
    scene = LegoProxy(n_images=34, img_wh=(80, 80), device="cpu")
    lab = export.render_scene_labels(scene, range(34), n_quad=128)
    assert lab.shape == (34, 80, 80) and lab.dtype == np.int64
    assert set(np.unique(lab).tolist()) == {0, 1, 2, 3, SKY_LABEL, IGNORE_LABEL}
    share = {c: float((lab == c).mean()) for c in (0, 1, 2, 3, SKY_LABEL, IGNORE_LABEL)}
    print("label shares", share)
    assert all(share[c] >= 0.02 for c in range(5)) and share[IGNORE_LABEL] <= 0.05
    o = torch.tensor([[1.5, 1.5, 1.5], [0.3, 0.0, 1.5]])
    d = torch.tensor([[0.0, 0.1, 1.0], [0.0, 0.0, -1.0]])       # away from the scene; straight down through box1 alone
    assert scene.ground_truth_labels(o, d, n_quad=128).tolist() == [SKY_LABEL, 0]
    # the parts tile the solid: a point has a part exactly where the density is non-zero, the first solid wins
    x = torch.rand(20000, 3, generator=torch.Generator().manual_seed(1)) - 0.5
    part = analytic_part(x)
    assert torch.equal(part >= 0, analytic_sigma(x) > 0) and set(part.unique().tolist()) == {-1, 0, 1, 2, 3}
    assert int(analytic_part(torch.tensor([[0.0, 0.0, -0.09]]))) == 0          # inside box1 and box2


def test_exporters_store_ignore_as_255(ngp, tmp_path):
    """256 does not fit an 8-bit .pgm: both exporters write 255, and the loaders hand back int64 labels"""
    from ngp_amd.datasets import dataset_dict, export
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=9, img_wh=(16, 16), device="cpu")
    images = export.render_scene_views(scene, range(9), rgba=False, n_quad=32)
    labels = export.render_scene_labels(scene, range(9), n_quad=32)
    labels[0, 0, :3] = 256
    c2w, K = scene.poses.numpy().astype(np.float64), scene.K.numpy().astype(np.float64)
    want = np.minimum(labels, 255).reshape(9, -1)
    root = export.export_tnt(str(tmp_path / "tnt"), images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(9)], labels=labels)
    test_set = dataset_dict["tnt"](root, "test", 1.0, use_sem=True, num_classes=5)
    assert test_set.labels.dtype == torch.int64 and np.array_equal(test_set.labels.numpy(), want[[0, 8]])
    assert "label" in test_set[0] and (test_set[0]["label"][:3] == 255).all()
    root = export.export_colmap(str(tmp_path / "colmap"), images, c2w, K, labels=labels)
    train_set = dataset_dict["colmap"](root, "train", 1.0, use_sem=True, num_classes=5)
    assert train_set.labels.dtype == torch.int64 and "label" in train_set[0]
    with pytest.raises(ValueError):
        export.export_tnt(str(tmp_path / "neg"), images, c2w, K, [0] * 9, labels=labels - 1)


def test_labels_belong_to_the_images_of_their_split(ngp, tmp_path):
    """label image i is the constant i % 5 + 10 * (i // 5) < 70.  The colmap loader reads the labels of ALL frames (as
    upstream) while its images are cut to the split: train_dataset.labels_of_split makes labels[k] the labels of the
    split's k-th image, for both layouts, and the sampler then pairs every ray with its own frame's label"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd.datasets import dataset_dict, export
    from ngp_amd.synthetic import LegoProxy
    n = 19
    scene = LegoProxy(n_images=n, img_wh=(8, 8), device="cpu")
    images = export.render_scene_views(scene, range(n), rgba=False, n_quad=8)
    images[:, 0, 0, 0] = np.arange(n) * 10          # the red byte of pixel 0 names the frame
    frame_label = np.array([i % 5 + 10 * (i // 5) for i in range(n)])
    labels = np.broadcast_to(frame_label[:, None, None], (n, 8, 8)).copy()
    c2w, K = scene.poses.numpy().astype(np.float64), scene.K.numpy().astype(np.float64)
    roots = {"tnt": export.export_tnt(str(tmp_path / "tnt"), images, c2w, K, [1 if i % 8 == 0 else 0 for i in range(n)], labels=labels),
             "colmap": export.export_colmap(str(tmp_path / "colmap"), images, c2w, K, labels=labels, shuffle_seed=3)}
    frames = {"train": [i for i in range(n) if i % 8], "test": [0, 8, 16]}
    for fmt, root in roots.items():
        for split in ("train", "test"):
            ds = dataset_dict[fmt](root, split, 1.0, use_sem=True, num_classes=7)
            if fmt == "colmap":
                assert ds.labels.shape[0] == n and len(ds.poses) == len(frames[split])          # the mismatch being mended
            td.labels_of_split(ds)
            td.labels_of_split(ds)          # idempotent
            assert ds.labels.shape == (len(frames[split]), 64)
            named = (ds.rays[:, 0, 0] * 255).round().long().tolist()
            assert named == [10 * i for i in frames[split]], (fmt, split)          # image k of the split is frame frames[k]
            assert ds.labels[:, 0].tolist() == frame_label[frames[split]].tolist(), (fmt, split)
            assert (ds.labels == ds.labels[:, :1]).all()
        ds = dataset_dict[fmt](root, "train", 1.0, use_sem=True, num_classes=7)
        td.labels_of_split(ds)
        ds.batch_size = 256
        s = ds[0]
        assert s["label"].tolist() == frame_label[np.array(frames["train"])[s["img_idxs"].numpy()]].tolist(), fmt
    ds = dataset_dict["colmap"](roots["colmap"], "train", 1.0, use_sem=True, num_classes=7)
    ds.labels = ds.labels[:5]
    with pytest.raises(ValueError):
        td.labels_of_split(ds)


# ------------------------------------------------------------------------------------------- metrics
def _confusion_metrics(pred, label, C):
    valid = (label >= 0) & (label < C)
    conf = np.zeros((C, C))
    for l, p in zip(label[valid], pred[valid]):
        conf[l, p] += 1
    hit = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - hit
    seen = union > 0
    return hit.sum() / conf.sum(), (hit[seen] / union[seen]).mean()


@pytest.mark.parametrize("classes", [5, 7])
def test_semantic_metrics_match_a_confusion_matrix(ngp, classes):
    """class 3 occurs in neither the labels nor the predictions and must not count in the mean IoU; 255, 256 and -1 are
    left out of both figures"""
    from ngp_amd.evaluation import semantic_metrics
    g = np.random.default_rng(5)
    keep = np.array([c for c in range(classes) if c != 3])
    label = keep[g.integers(0, len(keep), 4000)]
    pred = np.where(g.random(4000) < 0.7, label, keep[g.integers(0, len(keep), 4000)])
    label[::9] = np.resize([256, 255, -1], len(label[::9]))
    acc, miou = semantic_metrics(torch.from_numpy(pred)[:, None], torch.from_numpy(label), classes)
    want = _confusion_metrics(pred, label, classes)
    assert abs(float(acc) - want[0]) < 1e-12 and abs(float(miou) - want[1]) < 1e-12
    with3 = _confusion_metrics(np.where(np.arange(4000) == 1, 3, pred), label, classes)
    assert with3[1] < want[1]          # (a class that does occur, with IoU 0, would lower the mean)
    # the split's summary: accuracy weighted by the valid pixels, images without a valid label (NaN) left out
    from ngp_amd.evaluation import semantic_summary
    res = {"sem_acc": [0.5, float("nan"), 1.0], "sem_miou": [0.25, float("nan"), 0.75], "sem_valid": [300, 0, 100]}
    assert semantic_summary(res) == (0.625, 0.5)
    assert semantic_summary({"sem_acc": [float("nan")], "sem_miou": [float("nan")], "sem_valid": [0]}) == (None, None)
    none = semantic_metrics(torch.from_numpy(pred), torch.full((4000,), 256), classes)
    assert torch.isnan(none[0]) and torch.isnan(none[1])
    perfect = semantic_metrics(torch.from_numpy(label), torch.from_numpy(label), classes)
    assert float(perfect[0]) == 1.0 and float(perfect[1]) == 1.0


# ------------------------------------------------------------------------------------------- the tool's flags
def test_train_dataset_flags(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    a = td.parse_args(["--root_dir", "x"])
    assert a.render_semantic is False and a.num_classes == 7 and a.scale == 0.5
    assert td.parse_args(["--make_proxy", "d"]).scale == 0.5
    assert td.parse_args(["--make_proxy", "d", "--dataset_name", "colmap", "--render_semantic"]).scale == 2.0
    assert td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--render_semantic", "--scale", "1"]).scale == 1.0

    class _Set:
        poses = torch.tensor([[[1, 0, 0, 0.3], [0, 1, 0, -0.8], [0, 0, 1, 0.1]]], dtype=torch.float32)
    assert td.cameras_outside(_Set, 0.5) == pytest.approx(0.8) and td.cameras_outside(_Set, 2.0) is None
    a = td.parse_args(["--make_proxy", "d", "--dataset_name", "tnt", "--render_semantic", "--num_classes", "10"])
    assert a.render_semantic and a.num_classes == 10
    for bad in (["--root_dir", "x", "--num_classes", "17"], ["--root_dir", "x", "--num_classes", "0"],
                ["--make_proxy", "d", "--render_semantic", "--dataset_name", "nerf"],
                ["--make_proxy", "d", "--render_semantic"],
                ["--root_dir", "x", "--dataset_name", "tnt", "--render_semantic", "--embed_msk"]):
        with pytest.raises(SystemExit) as e:
            td.parse_args(bad)
        assert e.value.code == 2, bad


# ------------------------------------------------------------------------------------------- the C entry
def test_c_entry_checks_its_arguments(ngp):
    """classes outside [1, 16] and a negative ray count are NGP_EINVAL, an empty batch is NGP_OK before any pointer is
    looked at (every pointer is NULL here: nothing may reach a launch)"""
    _lib = ngp._lib
    lib = _lib.load()
    _, args = _lib.PROTOS["ngp_render_loss_fused_sem"]
    names = [a for _, a in args]
    assert names[-4:] == ["dL_drgbs", "sem_ws", "dL_dsem_logits", "stream"] and "labels" in names

    def run(classes, n_rays, ld_sem=16):
        vals = []
        for t, a in args:
            if t is C.c_void_p:
                vals.append(None)
            elif t is C.c_float:
                vals.append(1.0)
            else:
                vals.append({"classes": classes, "n_rays": n_rays, "ld_normal": 3, "ld_sem": ld_sem}[a])
        return lib.ngp_render_loss_fused_sem(*vals)
    for n_rays in (0, 5):
        assert run(0, n_rays) == -22 and run(17, n_rays) == -22 and run(-1, n_rays) == -22
    assert run(1, 0) == 0 and run(16, 0) == 0 and run(10, 0) == 0
    assert run(7, -1) == -22 and run(10, 0, ld_sem=9) == -22
    assert run(7, 5) == -22            # NULL pointers with rays to process
