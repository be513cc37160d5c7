"""ngp_resize_bicubic_u8 on the MI355X: imaging.resize_u8 byte for byte against the numpy restatement of Pillow's 8-bit
bicubic resize (tests/resample_reference.py, itself held against Pillow in tests/test_resample_host.py), batches, the C
ABI's argument checks, and the whole route: a trained field rendered on the supersampled lattice, packed, resized, and
written by tools/render.py and tools/render_panorama.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the host list, a copy, many tiles with ragged edges, one frame-sized case, and ratios 5, 6 and 8, at which three
# channels take the kernel's 32 x 8, 16 x 16 and 16 x 8 tiles instead of 32 x 16
GPU_SHAPES = ref.SHAPES + [(9, 9, 9, 9), (200, 160, 100, 80), (1600, 1600, 800, 800), (100, 165, 20, 33),
                           (102, 210, 17, 35), (136, 280, 17, 35)]


def _resize(ngp, img, out_wh):
    out = ngp.imaging.resize_u8(torch.from_numpy(img).to(DEV), out_wh)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_u8_equals_the_restatement(ngp, shape):
    ih, iw, oh, ow = shape
    for channels in ((3,) if ih >= 1600 else (1, 3)):
        for kind in ("random", "binary", "white"):
            src = ref.make_input(200 + ih * iw + channels, ih, iw, channels, kind)
            got = _resize(ngp, src, (ow, oh))
            want = ref.resize_bicubic_u8(src, (ow, oh))
            assert got.dtype == np.uint8 and got.shape == want.shape == ((oh, ow) if channels == 1 else (oh, ow, 3))
            bad = int((got != want).sum())
            assert bad == 0, (shape, channels, kind, bad)
            if kind == "white":
                assert (got == 255).all()
            if (ih, iw) == (oh, ow):
                assert np.array_equal(got, src)
            if channels == 1:                              # (H, W, 1) is the same call as (H, W)
                assert np.array_equal(_resize(ngp, src[..., None], (ow, oh))[..., 0], got)


def test_batch_equals_single_calls_and_two_runs_agree(ngp):
    g = np.random.default_rng(31)
    imgs = g.integers(0, 256, (3, 75, 130, 3), dtype=np.uint8)
    imgs[2] = (imgs[2] > 127) * 255
    single = np.stack([_resize(ngp, np.ascontiguousarray(im), (43, 30)) for im in imgs])
    batch = _resize(ngp, imgs, (43, 30))
    assert batch.shape == (3, 30, 43, 3) and np.array_equal(batch, single)
    assert np.array_equal(_resize(ngp, imgs, (43, 30)), batch)
    for im, out in zip(imgs, single):
        assert np.array_equal(out, ref.resize_bicubic_u8(im, (43, 30)))
    assert len({out.tobytes() for out in single}) == 3


def test_argument_checks_through_the_c_abi(ngp):
    """none of these reaches a launch: the pointers that are given are never read"""
    lib = ngp._lib.load()
    fn = lib.ngp_resize_bicubic_u8
    src = torch.zeros(18 * 18 * 3, dtype=torch.uint8, device=DEV)
    dst = torch.full((18 * 18 * 3,), 7, dtype=torch.uint8, device=DEV)
    kk, bounds, ksize = ngp.imaging.bicubic_taps(16, 8)
    k = torch.from_numpy(kk.copy()).to(DEV)
    b = torch.from_numpy(bounds.copy()).to(DEV)
    s, d, kp, bp = src.data_ptr(), dst.data_ptr(), k.data_ptr(), b.data_ptr()
    assert fn(None, 0, 0, 0, 0, None, 0, 0, None, None, 0, None, None, 0, None) == 0          # count == 0 first
    assert fn(None, 0, 16, 16, 2, None, 8, 8, None, None, 3, None, None, 3, None) == 0
    assert fn(None, -1, 0, 0, 0, None, 0, 0, None, None, 0, None, None, 0, None) == -22
    assert fn(s, -1, 16, 16, 3, d, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22
    assert fn(s, 1, 16, 16, 2, d, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22            # channels
    assert fn(s, 1, 16, 16, 4, d, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22
    assert fn(s, 1, 16, 0, 3, d, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22             # sizes
    assert fn(s, 1, 16, 16, 3, d, 8, -8, kp, bp, ksize, kp, bp, ksize, None) == -22
    assert fn(s, 1, 18, 16, 3, d, 2, 8, kp, bp, ksize, kp, bp, 37, None) == -22               # ratio 9 on the rows
    assert fn(s, 1, 16, 18, 3, d, 8, 2, kp, bp, 37, kp, bp, ksize, None) == -22               # ... on the columns
    assert fn(s, 1, 16, 16, 3, d, 8, 8, kp, bp, ksize + 2, kp, bp, ksize, None) == -22        # ksize
    assert fn(s, 1, 16, 16, 3, d, 8, 8, kp, bp, ksize, kp, bp, ksize - 2, None) == -22
    assert fn(s, 1, 16, 16, 3, d, 8, 8, None, None, ksize, kp, bp, ksize, None) == -22        # taps of a changing axis
    assert fn(s, 1, 16, 16, 3, d, 8, 8, kp, bp, ksize, kp, None, ksize, None) == -22
    assert fn(None, 1, 16, 16, 3, d, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22         # images
    assert fn(s, 1, 16, 16, 3, None, 8, 8, kp, bp, ksize, kp, bp, ksize, None) == -22
    torch.cuda.synchronize()
    assert (dst == 7).all()
    # an unchanged axis takes NULL taps
    img = torch.from_numpy(ref.make_input(3, 16, 8, 3, "random")).to(DEV)
    out = torch.empty(8, 8, 3, dtype=torch.uint8, device=DEV)
    assert fn(img.data_ptr(), 1, 16, 8, 3, out.data_ptr(), 8, 8, None, None, 0, kp, bp, ksize,
              C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref.resize_bicubic_u8(img.cpu().numpy(), (8, 8)))


def test_wrapper_errors(ngp):
    from ngp_amd.imaging import resize_u8
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        resize_u8(img.float(), (8, 8))
    with pytest.raises(ValueError):
        resize_u8(img.permute(1, 0, 2), (8, 8))
    with pytest.raises(ValueError):
        resize_u8(img[:, ::2], (8, 8))
    with pytest.raises(ValueError):
        resize_u8(torch.zeros(16, 16, 4, dtype=torch.uint8, device=DEV), (8, 8))
    with pytest.raises(ValueError):
        resize_u8(torch.zeros(18, 16, 3, dtype=torch.uint8, device=DEV), (8, 2))          # ratio 9
    with pytest.raises(ValueError):
        resize_u8(torch.zeros(16, dtype=torch.uint8, device=DEV), (8, 8))
    assert resize_u8(img, (8, 8)).shape == (8, 8, 3)


# --------------------------------------------------------------------------------------------------------- end to end
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


@pytest.fixture(scope="module")
def trained(ngp, tmp_path_factory):
    """the recipe of test_trained_scene_metrics_checkpoint_and_render_tool (proxy scene, 24+2 views of 80x80), one epoch
    of 200 steps, no quality bar; trained once for the tests below -> (model, test split, scene directory, checkpoint)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td
    from ngp_amd import ckpt
    from ngp_amd.datasets import NeRFDataset, write_synthetic_dataset
    from ngp_amd.synthetic import LegoProxy
    tmp = tmp_path_factory.mktemp("antialias")
    scene = LegoProxy(n_images=26, img_wh=(80, 80), device=DEV)
    root = write_synthetic_dataset(str(tmp / "scene"), scene, n_train=24, n_test=2, rgba=False, n_quad=128)
    train_set = NeRFDataset(root, "train", 0.1, device=DEV)
    test_set = NeRFDataset(root, "test", 0.1, device=DEV)
    torch.manual_seed(41)
    model = td.build_model(0.5, DEV)
    tr = td.train(model, train_set, num_epochs=1, steps_per_epoch=200, batch_size=2048, lr=1e-2)
    assert tr.global_step == 200 and tuple(test_set.img_wh) == (80, 80)
    path = str(tmp / "model.ckpt")
    ckpt.save_ckpt(model, path)
    return model, test_set, root, path


@pytest.mark.timeout(600)
def test_antialiased_frames_in_process_and_from_the_tool(ngp, trained, tmp_path):
    from ngp_amd.evaluation import frame_images, render_image
    model, test_set, root, path = trained
    w, h = test_set.img_wh
    K_before = test_set.K.clone()
    want = ("rgb", "depth")

    # factor 2 in process: the resized frames are the restatement of the fine packed frames
    mine = []
    for i in range(2):
        pose = test_set[i]["pose"]
        results = render_image(model, None, pose, anti_aliasing_factor=2, K=test_set.K, img_wh=(w, h))
        assert results["rgb"].shape == (4 * h * w, 3)
        fine = frame_images(results, pose, 0.5, 7, want, img_wh=(2 * w, 2 * h))
        small = frame_images(results, pose, 0.5, 7, want, img_wh=(2 * w, 2 * h), out_wh=(w, h))
        same = frame_images(results, pose, 0.5, 7, want, img_wh=(2 * w, 2 * h), out_wh=(2 * w, 2 * h))
        torch.cuda.synchronize()
        assert len(np.unique(fine["rgb"].cpu().numpy())) >= 16
        for k in want:
            assert fine[k].shape == (2 * h, 2 * w, 3) and torch.equal(same[k], fine[k])
            got = small[k].cpu().numpy()
            assert got.shape == (h, w, 3) and got.dtype == np.uint8
            assert np.array_equal(got, ref.resize_bicubic_u8(fine[k].cpu().numpy(), (w, h))), (i, k)
        mine.append({k: small[k].cpu().numpy() for k in want})
        with pytest.raises(ValueError):
            frame_images(results, pose, 0.5, 7, ("rgb", "semantic"), img_wh=(2 * w, 2 * h), out_wh=(w, h))
    assert torch.equal(test_set.K, K_before)                 # the loader's intrinsics are not scaled in place
    with pytest.raises(ValueError):
        render_image(model, None, test_set[0]["pose"], anti_aliasing_factor=2)

    # the tool in a child process writes the same frames, and agrees with Pillow itself (--aa_host_check)
    out_dir = str(tmp_path / "frames")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py"), "--ckpt", path, "--scale", "0.5",
                          "--root_dir", root, "--dataset_name", "nerf", "--downsample", "0.1", "--out_dir", out_dir,
                          "--render_rgb", "--render_depth", "--anti_aliasing_factor", "2", "--aa_host_check"],
                         capture_output=True, text=True, timeout=500)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames"] == 2 and line["img_wh"] == [w, h] and line["supersampled_wh"] == [2 * w, 2 * h]
    assert line["metrics_on"] == "antialiased_u8" and len(line["psnr"]) == 2 and len(line["ssim"]) == 2
    assert all(line[k] >= 0 for k in ("render_s", "pack_s", "resize_s", "host_route_s", "d2h_s", "png_s"))
    for i in range(2):
        for k in want:
            assert np.array_equal(_png(os.path.join(out_dir, f"{i:03d}-{k}.png")), mine[i][k]), (i, k)
        # the metrics are those of the anti-aliased 8-bit frame
        gt = test_set[i]["rgb"].cpu().numpy().astype(np.float64)
        img = mine[i]["rgb"].reshape(-1, 3).astype(np.float32) / np.float32(255)
        p64 = -10 * np.log10(np.mean((img.astype(np.float64) - gt) ** 2))
        assert abs(line["psnr"][i] - p64) <= 1e-3
    assert sorted(os.listdir(out_dir)) == sorted(f"{i:03d}-{k}.png" for i in range(2) for k in want)


def test_antialiasing_factor_one_and_a_half(ngp, trained):
    """120 x 120 -> 80 x 80: a ratio that is no integer"""
    from ngp_amd.evaluation import frame_images, render_image
    from ngp_amd.imaging import supersampled_size
    model, test_set, _, _ = trained
    w, h = test_set.img_wh
    pose = test_set[0]["pose"]
    assert supersampled_size(h, w, 1.5) == (120, 120)
    results = render_image(model, None, pose, anti_aliasing_factor=1.5, K=test_set.K, img_wh=(w, h))
    fine = frame_images(results, pose, 0.5, 7, ("rgb",), img_wh=(120, 120))["rgb"]
    small = frame_images(results, pose, 0.5, 7, ("rgb",), img_wh=(120, 120), out_wh=(w, h))["rgb"]
    assert fine.shape == (120, 120, 3) and small.shape == (h, w, 3)
    assert len(np.unique(fine.cpu().numpy())) >= 16
    assert np.array_equal(small.cpu().numpy(), ref.resize_bicubic_u8(fine.cpu().numpy(), (w, h)))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("factor", [1, 2])
def test_panorama_tool_equals_the_in_process_route(ngp, trained, tmp_path, factor):
    """a 32 x 64 panorama from below the object, one ray per pixel and supersampled (64 x 128 rays)"""
    from ngp_amd.evaluation import frame_images, render_rays
    from ngp_amd.imaging import panorama_rays
    model, _, _, path = trained
    basis = dict(forward=(0.0, 0.0, 1.0), down=(0.0, 1.0, 0.0), right=(1.0, 0.0, 0.0))
    origin, radius = (0.0, 0.0, -1.2), 0.05
    pano_dir = str(tmp_path / "pano")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "render_panorama.py"), "--ckpt", path, "--scale", "0.5",
           "--pano_hw", "32", "64", "--origin", *map(str, origin), "--pano_radius", str(radius), "--render_depth",
           "--out_dir", pano_dir, "--anti_aliasing_factor", str(factor)]
    for name, v in basis.items():
        cmd += [f"--v_{name}", *map(str, v)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["pano_hw"] == [32, 64] and line["rays"] == 32 * 64 * factor * factor
    assert all(line[k] >= 0 for k in ("rays_s", "render_s", "pack_s", "resize_s", "d2h_s", "png_s"))
    names = ("rgb", "opacity", "depth")
    rays_o, rays_d = panorama_rays(32 * factor, 64 * factor, origin=origin, radius=radius, device=DEV, **basis)
    results = render_rays(model, rays_o, rays_d)
    frames = frame_images(results, None, 0.5, 7, names, img_wh=(64 * factor, 32 * factor))
    frames = {k: v.cpu().numpy() for k, v in frames.items()}
    assert len(np.unique(frames["rgb"])) >= 16
    if factor == 2:
        assert line["supersampled_hw"] == [64, 128]
        frames = {k: ref.resize_bicubic_u8(v, (64, 32)) for k, v in frames.items()}
    for k in names:
        png = _png(os.path.join(pano_dir, f"{k}.png"))
        assert png.shape == ((32, 64) if k == "opacity" else (32, 64, 3)) and png.dtype == np.uint8
        assert np.array_equal(png, frames[k]), (factor, k)
    mask = _png(os.path.join(pano_dir, "mask.png"))
    assert mask.shape == (32, 64) and np.array_equal(mask, np.where(frames["opacity"] == 0, 255, 0))
    assert 0 < int((mask == 255).sum()) < mask.size and line["transparent_pixels"] == int((mask == 255).sum())
    assert sorted(os.listdir(pano_dir)) == ["depth.png", "mask.png", "opacity.png", "rgb.png"]
