"""CPU checks of the image metrics and the frame tool: properties of the float64 SSIM restatement the GPU tests hold
the kernel against (tests/image_reference.py), the shipped colour table, the argument checks of metrics.ssim and of the
ngp_ssim / ngp_frame_pack entry points without a launch, and tools/render.py --help."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def _smooth(g, h, w, c=3):
    """a smooth random colour field in [0.1, 0.9]"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    img = np.zeros((h, w, c))
    for ch in range(c):
        for _ in range(4):
            fx, fy, ph = g.uniform(0.5, 6), g.uniform(0.5, 6), g.uniform(0, 2 * np.pi)
            img[..., ch] += g.uniform(0.2, 1) * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    img -= img.min()
    return 0.1 + 0.8 * img / img.max()


def test_taps_are_the_normalised_gaussian():
    t = ref.gaussian_taps()
    assert t.shape == (11,) and abs(t.sum() - 1) < 1e-15 and np.array_equal(t, t[::-1])
    assert abs(t[5] / t[4] - np.exp(1 / 4.5)) < 1e-14 and t.argmax() == 5


def test_ssim_of_an_image_with_itself_is_exactly_one():
    g = np.random.default_rng(1)
    for shape in ((11, 11), (37, 53), (64, 64)):
        x = _smooth(g, *shape)
        assert ref.ssim(x, x) == 1.0
    flat = np.full((20, 20, 3), 0.95)
    assert ref.ssim(flat, flat) == 1.0


def test_ssim_is_symmetric_and_below_one_for_different_images():
    g = np.random.default_rng(2)
    x = _smooth(g, 40, 56)
    y = np.clip(x + g.normal(0, 0.05, x.shape), 0, 1)
    a, b = ref.ssim(x, y), ref.ssim(y, x)
    assert a == b and 0 < a < 1
    assert ref.ssim(x, np.clip(x + g.normal(0, 0.01, x.shape), 0, 1)) > a    # less noise, more similar


def test_single_window_equals_the_hand_evaluated_formula():
    g = np.random.default_rng(3)
    x, y = g.uniform(0, 1, (11, 11, 3)), g.uniform(0, 1, (11, 11, 3))
    t = ref.gaussian_taps()
    w2 = np.outer(t, t)[..., None]
    mx, my = (w2 * x).sum((0, 1)), (w2 * y).sum((0, 1))
    vx, vy = (w2 * x * x).sum((0, 1)) - mx ** 2, (w2 * y * y).sum((0, 1)) - my ** 2
    cxy = (w2 * x * y).sum((0, 1)) - mx * my
    want = (((2 * mx * my + 1e-4) * (2 * cxy + 9e-4)) / ((mx ** 2 + my ** 2 + 1e-4) * (vx + vy + 9e-4))).mean()
    assert abs(ref.ssim(x, y) - want) < 1e-14


def test_two_formulations_agree():
    g = np.random.default_rng(4)
    for shape, noise in (((11, 11), 0.1), ((11, 64), 0.05), ((37, 53), 0.05), ((96, 80), 0.01)):
        x = _smooth(g, *shape)
        y = np.clip(x + g.normal(0, noise, x.shape), 0, 1)
        assert abs(ref.ssim(x, y) - ref.ssim_correlate(x, y)) < 1e-12, shape
    white = np.ones((64, 64, 3))
    assert abs(ref.ssim(white, white - 1 / 255) - ref.ssim_correlate(white, white - 1 / 255)) < 1e-12


def test_restatement_rejects_small_images():
    with pytest.raises(ValueError):
        ref.ssim(np.zeros((10, 20, 3)), np.zeros((10, 20, 3)))


def test_colour_table_shape_and_end_points(ngp):
    from ngp_amd.colormap import turbo_lut
    lut = turbo_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [48, 18, 59] and lut[255].tolist() == [122, 4, 2]     # Turbo's published end points
    assert len({tuple(r) for r in lut.tolist()}) == 256


def test_colour_table_is_matplotlibs_turbo(ngp):
    matplotlib = pytest.importorskip("matplotlib")
    from ngp_amd.colormap import turbo_lut
    assert np.array_equal(turbo_lut(), matplotlib.colormaps["turbo"](np.arange(256), bytes=True)[:, :3])


def test_packing_restatement_truncates_and_clips():
    assert ref.u8([-0.5, 0.0, 0.999, 1.0, 7.0, 0.5]).tolist() == [0, 0, 254, 255, 255, 127]
    lut = np.arange(768, dtype=np.uint8).reshape(256, 3)
    assert np.array_equal(ref.pack_depth(np.float32([0.0, 1.0, 2.0]), 1.0, lut), lut[[0, 255, 255]])
    assert np.array_equal(ref.pack_semantic(np.int64([0, 3, 6]), 7, lut), lut[[0, 127, 255]])
    eye = np.eye(3, dtype=np.float32)
    assert ref.pack_normal(np.float32([[0, 0, 1], [0, -1, 0]]), eye).tolist() == [[127, 127, 255], [127, 0, 127]]


def test_metrics_ssim_rejects_bad_shapes_then_cpu_tensors(ngp):
    from ngp_amd.metrics import ssim
    z = torch.zeros
    for a, b, wh in ((z(10, 32, 3), z(10, 32, 3), None),            # H < 11
                     (z(32, 10, 3), z(32, 10, 3), None),            # W < 11
                     (z(2, 32, 10, 3), z(2, 32, 10, 3), None),
                     (z(32, 32, 4), z(32, 32, 4), None),            # channels
                     (z(32, 32), z(32, 32), None),
                     (z(32, 32, 3), z(32, 31, 3), None),            # mismatch
                     (z(1024, 3), z(1024, 3), None),                # rows without img_wh
                     (z(1024, 3), z(1024, 3), (32, 31)),            # img_wh does not match the rows
                     (z(320, 3), z(320, 3), (32, 10)),              # (W, H) order: H = 10
                     (z(2, 1024, 3), z(2, 1024, 3), (64, 32))):
        with pytest.raises(ValueError):
            ssim(a, b, wh)
    for a, wh in ((z(32, 32, 3), None), (z(2, 16, 20, 3), None), (z(320, 3), (20, 16)),
                  (z(2, 320, 3), (16, 20))):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            ssim(a, a.clone(), wh)


def test_image_entry_points_check_arguments_without_a_launch(ngp):
    _lib = ngp._lib
    lib = _lib.load()
    for name in ("ngp_ssim", "ngp_ssim_workspace", "ngp_frame_pack"):
        assert name in _lib.PROTOS
    ws = _lib.call_host("ssim_workspace", 3, 800, 800)
    assert ws == 3 * 50 * 50
    assert _lib.call_host("ssim_workspace", 1, 11, 11) == 1 and _lib.call_host("ssim_workspace", 1, 27, 26) == 2
    assert _lib.call_host("ssim_workspace", 1, 10, 64) == EINVAL and _lib.call_host("ssim_workspace", 1, 64, 10) == EINVAL
    assert _lib.call_host("ssim_workspace", -1, 64, 64) == EINVAL
    fake = 4096   # a non-NULL address that must never be dereferenced: every call below fails its checks first
    assert lib.ngp_ssim(fake, fake, 1, 10, 64, fake, fake, None) == EINVAL
    assert lib.ngp_ssim(None, fake, 1, 64, 64, fake, fake, None) == EINVAL
    assert lib.ngp_ssim(fake, fake, 1, 64, 64, None, fake, None) == EINVAL
    assert lib.ngp_ssim(None, None, 0, 0, 0, None, None, None) == 0

    def pack(n=8, rgb=None, opacity=None, depth=None, npred=None, nraw=None, R=None, sem=None, classes=7, lut=None,
             out=(None,) * 6):
        return lib.ngp_frame_pack(n, rgb, opacity, depth, 1.0, npred, nraw, R, sem, classes, lut, *out, None)
    only = lambda k: tuple(fake if i == k else None for i in range(6))   # noqa: E731
    assert pack(n=-1) == EINVAL and pack(n=0, out=(fake,) * 6) == 0
    assert pack() == 0                                         # nothing asked for: nothing launched
    assert pack(out=only(0)) == EINVAL and pack(out=only(1)) == EINVAL        # outputs without their inputs
    assert pack(depth=fake, out=only(2)) == EINVAL             # depth without a colour table
    assert pack(npred=fake, out=only(3)) == EINVAL and pack(nraw=fake, out=only(4)) == EINVAL   # normals without R
    assert pack(sem=fake, lut=fake, classes=1, out=only(5)) == EINVAL
    assert pack(sem=fake, classes=7, out=only(5)) == EINVAL


def test_camera_path_poses_are_the_poses_of_the_camera_path_rays(ngp, monkeypatch):
    """tools/render.py --render_traj renders the loader's render_traj_rays and rotates the normals by render_c2w: the
    two must describe the same cameras (T&T fixture with its camera_path/; COLMAP fixture with a denser interpolation,
    since its few views give fewer than the 400 poses the loader cuts off the front of the path)"""
    import shutil
    import helpers
    from ngp_amd import datasets
    from ngp_amd.datasets import colmap, export, get_rays
    root = helpers.dataset_tmp_root()
    try:
        dirs = helpers.write_dataset_dirs(root, export)
        dense = colmap.generate_interpolated_path
        monkeypatch.setattr(colmap, "generate_interpolated_path", lambda poses, n, **kw: dense(poses, 4 * n, **kw))
        for name in ("tnt", "colmap"):
            key, path, kwargs = dirs[name]
            ds = datasets.dataset_dict[key](path, split="test", render_traj=True, **kwargs)
            assert len(ds.render_traj_rays) == len(ds.render_c2w) > 0, name
            assert ds.render_c2w.dtype == torch.float32 and tuple(ds.render_c2w.shape[1:]) == (3, 4)
            for j in range(len(ds.render_c2w)):
                o, d = get_rays(ds.directions, ds.render_c2w[j].to(ds.directions.device))
                assert torch.equal(torch.cat([o, d], 1).cpu(), ds.render_traj_rays[j]), (name, j)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def test_render_tool_help_runs_without_a_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    txt = " ".join(out.stdout.split())
    for flag in ("--ckpt", "--scale", "--root_dir", "--dataset_name", "--downsample", "--exp_step_factor",
                 "--num_classes", "--chunk_size", "--out_dir", "--render_rgb", "--render_depth", "--render_normal",
                 "--render_semantic", "--render_points", "--render_traj"):
        assert flag in txt, flag
    none = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render.py"), "--ckpt", "x", "--root_dir", "y",
                           "--out_dir", "z"], capture_output=True, text=True, timeout=300)
    assert none.returncode == 2 and "nothing to render" in none.stderr
