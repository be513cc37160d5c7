"""Image kernels on the MI355X: ngp_ssim through ngp_amd.metrics.ssim against the float64 restatement of
tests/image_reference.py, ngp_frame_pack bit for bit against its float32 restatement, and the whole route from a trained
field through evaluate_split, a checkpoint and tools/render.py to PNG files.

SSIM bar: |kernel - float64 restatement| <= 1e-5 on the per-image mean.  Provenance: a float32 evaluation of the
definition with per-tile pivots, emulated on the CPU, stays within 2.5e-6 of the float64 one on cases (i)-(vii) below;
the bar is 4x that.  A plain float32 E[x^2] - mu^2 misses it on (iii) and (iv) by 6x and 13x.  The measured error of
each case is printed (pytest -s) before it is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_BAR = 1e-5
_F = np.float32


def _smooth(g, h, w):
    """a smooth random colour field in [0.1, 0.9], (h, w, 3) float32"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    img = np.zeros((h, w, 3))
    for ch in range(3):
        for _ in range(4):
            fx, fy, ph = g.uniform(0.5, 6), g.uniform(0.5, 6), g.uniform(0, 2 * np.pi)
            img[..., ch] += g.uniform(0.2, 1) * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    img -= img.min()
    return (0.1 + 0.8 * img / img.max()).astype(_F)


def _noisy(g, x, sigma):
    return np.clip(x + g.normal(0, sigma, x.shape), 0, 1).astype(_F)


def _case(name):
    """-> (pred, gt), each (H, W, 3) float32, generated from a seed per case"""
    g = np.random.default_rng({"i": 11, "ii": 12, "iii": 13, "iv": 14, "v": 15, "vi": 16, "vii": 17}.get(name, 18))
    if name in ("i", "ii", "vii"):
        gt = _smooth(np.random.default_rng(11), 200, 160)
        pred = _noisy(np.random.default_rng(11 if name != "ii" else 12), gt, 0.01 if name == "ii" else 0.05)
        if name == "vii":
            pred, gt = (np.round(pred * 255) / 255).astype(_F), (np.round(gt * 255) / 255).astype(_F)
        return pred, gt
    if name == "iii":
        white = np.ones((64, 64, 3), _F)
        return white, (white - _F(1 / 255)).astype(_F)
    if name == "iv":
        flat = np.full((96, 96, 3), 0.95, _F)
        return (flat + g.normal(0, 0.002, flat.shape)).astype(_F), flat
    if name == "v":
        gt = np.zeros((200, 200, 3), _F)
        gt[50:150, 50:150] = 0.5 * _smooth(g, 100, 100) + 0.5 * g.uniform(0, 1, (100, 100, 3)).astype(_F)
        pred = gt.copy()
        pred[50:150, 50:150] = _noisy(g, gt[50:150, 50:150], 0.03)
        return pred, gt
    if name == "vi":
        x = _noisy(g, _smooth(g, 120, 90), 0.05)
        return x, x.copy()
    h, w = {"11x11": (11, 11), "11x64": (11, 64), "37x53": (37, 53), "800x800": (800, 800)}[name]
    gt = _smooth(g, h, w)
    return _noisy(g, gt, 0.05), gt


def _gpu_ssim(ngp, pred, gt):
    out = ngp.metrics.ssim(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


SSIM_CASES = ["i", "ii", "iii", "iv", "v", "vi", "vii", "11x11", "11x64", "37x53", "800x800"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", SSIM_CASES)
def test_ssim_matches_the_float64_restatement(ngp, name):
    pred, gt = _case(name)
    got = float(_gpu_ssim(ngp, pred, gt))
    want = ref.ssim(pred, gt)
    print(f"ssim case {name:8s} {pred.shape[0]}x{pred.shape[1]}: kernel {got:.9f} float64 {want:.9f} "
          f"|err| {abs(got - want):.3e}")
    assert abs(got - want) <= SSIM_BAR, (name, got, want)
    if name == "vi":
        assert abs(got - 1.0) <= 2.0 ** -23, got
    else:
        assert 0 < got < 1
    # the row layout with img_wh=(W, H) is the same call
    h, w = pred.shape[:2]
    rows = ngp.metrics.ssim(torch.from_numpy(pred).to(DEV).reshape(h * w, 3), torch.from_numpy(gt).to(DEV).reshape(h * w, 3),
                            img_wh=(w, h))
    assert rows.dim() == 0 and float(rows) == got


@pytest.mark.timeout(600)
def test_ssim_batch_equals_single_calls_bitwise(ngp):
    g = np.random.default_rng(21)
    gts = [_smooth(g, 75, 130) for _ in range(3)]
    preds = [_noisy(g, gts[0], 0.05), _noisy(g, gts[1], 0.01), np.full_like(gts[2], 0.95)]
    single = np.stack([_gpu_ssim(ngp, p, t) for p, t in zip(preds, gts)])
    assert len(set(single.tolist())) == 3
    batch = _gpu_ssim(ngp, np.stack(preds), np.stack(gts))
    assert batch.shape == (3,) and np.array_equal(batch.view(np.int32), single.view(np.int32))
    rows = ngp.metrics.ssim(torch.from_numpy(np.stack(preds)).to(DEV).reshape(3, -1, 3),
                            torch.from_numpy(np.stack(gts)).to(DEV).reshape(3, -1, 3), img_wh=(130, 75))
    assert np.array_equal(rows.cpu().numpy().view(np.int32), single.view(np.int32))
    for p, t, s in zip(preds, gts, single):
        assert abs(float(s) - ref.ssim(p, t)) <= SSIM_BAR


@pytest.mark.timeout(600)
def test_ssim_two_runs_are_bit_identical_and_small_images_raise(ngp):
    pred, gt = _case("800x800")
    a, b = _gpu_ssim(ngp, pred, gt), _gpu_ssim(ngp, pred, gt)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    z = torch.zeros(10, 64, 3, device=DEV)
    with pytest.raises(ValueError):
        ngp.metrics.ssim(z, z.clone())


# ------------------------------------------------------------------------------------------------------ frame packing
def _pack_inputs(n, classes, seed):
    g = np.random.default_rng(seed)
    depth_scale = 3.0
    rgb = g.uniform(-0.2, 1.2, (n, 3)).astype(_F)
    opacity = g.uniform(-0.2, 1.2, n).astype(_F)
    depth = g.uniform(-0.1, 1.3, n).astype(_F) * _F(depth_scale)
    k = g.integers(0, 256, n)
    on_grid = (k.astype(_F) / _F(255)) * _F(depth_scale)           # depth / depth_scale lands on k/255 (or beside it)
    pick = g.uniform(size=n) < 0.3
    depth[pick] = on_grid[pick]
    for arr in (rgb.reshape(-1), opacity, depth):                    # exact end points and out-of-range values
        m = arr.size
        arr[g.integers(0, m, max(m // 16, 1))] = 1.0
        arr[g.integers(0, m, max(m // 16, 1))] = 0.0
        arr[g.integers(0, m, max(m // 32, 1))] = -3.5
        arr[g.integers(0, m, max(m // 32, 1))] = 7.25
    nrm = g.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(_F)
    nraw = g.normal(size=(n, 3))
    nraw /= np.linalg.norm(nraw, axis=1, keepdims=True)
    nraw = nraw.astype(_F)
    tiny = g.uniform(size=n) < 0.2
    nraw[tiny] = (g.normal(size=(int(tiny.sum()), 3)) * 1e-7).astype(_F)
    nrm[g.uniform(size=n) < 0.1] = 0.0
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    rot = q.astype(_F)
    sem = g.integers(0, classes, n).astype(np.int64)
    sem[: min(n, classes)] = np.arange(classes)[: min(n, classes)]   # every label 0..classes-1 when there is room
    return dict(rgb=rgb, opacity=opacity, depth=depth, normal=nrm, normal_raw=nraw, semantic=sem), rot, depth_scale


def _pack_reference(ins, rot, depth_scale, classes, lut):
    return {"rgb": ref.pack_rgb(ins["rgb"]), "opacity": ref.pack_opacity(ins["opacity"]),
            "depth": ref.pack_depth(ins["depth"], depth_scale, lut), "normal": ref.pack_normal(ins["normal"], rot),
            "normal_raw": ref.pack_normal(ins["normal_raw"], rot),
            "semantic": ref.pack_semantic(ins["semantic"], classes, lut)}


_ARG = {"rgb": "rgb", "opacity": "opacity", "depth": "depth", "normal": "normal_pred", "normal_raw": "normal_raw",
        "semantic": "semantic"}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("classes", [2, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 640000])
def test_frame_pack_bit_for_bit(ngp, n, classes):
    from ngp_amd.colormap import turbo_lut
    from ngp_amd.evaluation import pack_frame
    ins, rot, depth_scale = _pack_inputs(n, classes, 1000 * classes + n % 997)
    lut = turbo_lut()
    want = _pack_reference(ins, rot, depth_scale, classes, lut)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in ins.items()}
    rot_d = torch.from_numpy(rot).to(DEV)

    def run(names):
        kw = {_ARG[k]: dev[k] for k in names}
        out = pack_frame(n, depth_scale=depth_scale, rotation=rot_d, classes=classes, **kw)
        torch.cuda.synchronize()
        assert sorted(out) == sorted(names)
        return {k: v.cpu().numpy() for k, v in out.items()}

    together = run(list(want))
    for k, w in want.items():
        assert together[k].shape == w.shape and together[k].dtype == np.uint8
        bad = int((together[k] != w).sum())
        assert bad == 0, (k, n, classes, bad)
    for k, w in want.items():                      # each output alone: the others NULL
        alone = run([k])[k]
        assert np.array_equal(alone, w), (k, n, classes)


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.timeout(1500)
def test_trained_scene_metrics_checkpoint_and_render_tool(ngp, tmp_path):
    """the recipe of test_train_from_dataset_directory (proxy scene, 24+2 views of 80x80, 400 steps)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from PIL import Image
    from ngp_amd import ckpt
    from ngp_amd.datasets import NeRFDataset, write_synthetic_dataset
    from ngp_amd.evaluation import evaluate_split, frame_images, render_image
    from ngp_amd.synthetic import LegoProxy
    scene = LegoProxy(n_images=26, img_wh=(80, 80), device=DEV)
    root = write_synthetic_dataset(str(tmp_path / "scene"), scene, n_train=24, n_test=2, rgba=False, n_quad=128)
    train_set = NeRFDataset(root, "train", 0.1, device=DEV)
    test_set = NeRFDataset(root, "test", 0.1, device=DEV)
    torch.manual_seed(41)
    model = td.build_model(0.5, DEV)
    tr = td.train(model, train_set, num_epochs=2, steps_per_epoch=200, batch_size=2048, lr=1e-2)
    assert tr.global_step == 400

    images = []
    res = evaluate_split(model, test_set, on_image=lambda i, rgb, results: images.append(rgb.cpu().numpy()))
    psnrs = td.evaluate(model, test_set)
    assert res["psnr"] == psnrs and len(psnrs) == 2 and min(psnrs) > 22.0, (res, psnrs)
    w, h = test_set.img_wh
    for i in range(2):
        gt = test_set[i]["rgb"].cpu().numpy()
        img = images[i]
        assert img.shape == (h * w, 3) and img.min() >= 0 and img.max() <= 1
        p64 = -10 * np.log10(np.mean((img.astype(np.float64) - gt.astype(np.float64)) ** 2))
        s64 = ref.ssim(img.reshape(h, w, 3), gt.reshape(h, w, 3))
        print(f"trained proxy scene, test image {i}: psnr {res['psnr'][i]:.4f} dB (float64 {p64:.4f}), "
              f"ssim {res['ssim'][i]:.6f} (float64 {s64:.6f}, |err| {abs(res['ssim'][i] - s64):.2e})")
        assert abs(res["psnr"][i] - p64) <= 1e-3
        assert abs(res["ssim"][i] - s64) <= SSIM_BAR
        assert 0 < res["ssim"][i] <= 1

    path = str(tmp_path / "model.ckpt")
    ckpt.save_ckpt(model, path)
    out_dir = str(tmp_path / "frames")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py"), "--ckpt", path, "--scale", "0.5",
                          "--root_dir", root, "--dataset_name", "nerf", "--downsample", "0.1", "--out_dir", out_dir,
                          "--render_rgb", "--render_depth", "--render_normal", "--render_semantic", "--render_points"],
                         capture_output=True, text=True, timeout=1200)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames"] == 2 and line["img_wh"] == [w, h]
    assert line["psnr"] == res["psnr"] and line["ssim"] == res["ssim"], (line, res)
    assert all(line[k] >= 0 for k in ("render_s", "pack_s", "d2h_s", "png_s"))
    points = np.load(os.path.join(out_dir, "points.npy"))
    assert points.shape == (2, h, w, 3) and points.dtype == np.float32
    files = {"rgb": "rgb", "depth": "depth", "normal": "normal", "normal_raw": "normal-raw", "semantic": "semantic"}
    for i in range(2):
        pose = test_set[i]["pose"]
        results = render_image(model, test_set.directions, pose)
        frames = frame_images(results, pose, 0.5, 7, tuple(files), img_wh=(w, h))
        torch.cuda.synchronize()
        assert np.array_equal(points[i], results["points"].reshape(h, w, 3).cpu().numpy())
        for k, stem in files.items():
            png = np.asarray(Image.open(os.path.join(out_dir, f"{i:03d}-{stem}.png")))
            mine = frames[k].cpu().numpy()
            assert mine.shape == (h, w, 3) and mine.dtype == np.uint8
            assert np.array_equal(png, mine), (i, k)
        # and the packed frames are what the restatement makes of the same results
        rot = pose[:3, :3].cpu().numpy()
        lut = ngp.colormap.turbo_lut()
        assert np.array_equal(frames["rgb"].cpu().numpy().reshape(-1, 3), ref.pack_rgb(results["rgb"].cpu().numpy()))
        assert np.array_equal(frames["depth"].cpu().numpy().reshape(-1, 3),
                              ref.pack_depth(results["depth"].cpu().numpy(), 2 * 0.5, lut))
        assert np.array_equal(frames["normal"].cpu().numpy().reshape(-1, 3),
                              ref.pack_normal(results["normal_pred"].cpu().numpy(), rot))
    assert sorted(os.listdir(out_dir)) == sorted([f"{i:03d}-{s}.png" for i in range(2) for s in files.values()]
                                                 + ["points.npy"])
