"""Host side of the anti-aliased frames and panoramas: the numpy restatement of Pillow's 8-bit bicubic resize
(tests/resample_reference.py) against recorded Pillow output and against Pillow itself, imaging.bicubic_taps against the
restatement's taps, the supersampled size, panorama rays against a float64 restatement, and the two tools' parsers."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import resample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

def test_restatement_equals_recorded_pillow_output(golden):
    g16 = golden("g16_pillow_bicubic.npz")
    n = sum(1 for k in g16.files if k.startswith("in_"))
    assert n >= 12
    for i in range(n):
        src, want = g16[f"in_{i}"], g16[f"out_{i}"]
        got = ref.resize_bicubic_u8(src, (want.shape[1], want.shape[0]))
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (i, src.shape, want.shape)


@pytest.mark.parametrize("kind", ["random", "binary"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_restatement_equals_pillow(shape, channels, kind):
    Image = pytest.importorskip("PIL.Image")
    ih, iw, oh, ow = shape
    src = ref.make_input(100 + ih * iw + channels, ih, iw, channels, kind)
    want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.Resampling.BICUBIC))
    got = ref.resize_bicubic_u8(src, (ow, oh))
    assert got.shape == want.shape and np.array_equal(got, want)


def test_bicubic_taps_equal_the_restatement(ngp):
    from ngp_amd.imaging import bicubic_taps
    pairs = 0
    for n_out in range(1, 25):
        for n_in in range(max(1, math.ceil(n_out / 2)), 8 * n_out + 1):
            kk, bounds, ksize = bicubic_taps(n_in, n_out)
            kk_ref, bounds_ref, ksize_ref = ref.taps(n_in, n_out)
            assert ksize == ksize_ref == math.ceil(2 * max(n_in / n_out, 1.0)) * 2 + 1
            assert kk.dtype == np.int32 and bounds.dtype == np.int32
            assert kk.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
            assert np.array_equal(kk, kk_ref) and np.array_equal(bounds, bounds_ref), (n_in, n_out)
            # what the kernel's window relies on: neither end of a row of taps moves backwards
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()
            assert bounds[:, 0].min() >= 0 and bounds.sum(1).max() <= n_in
            # normalised: the taps of a row add up to 1 within the rounding of ksize fixed-point values
            assert np.abs(kk.astype(np.int64).sum(1) - (1 << 22)).max() <= ksize
            pairs += 1
    assert pairs > 2000
    assert bicubic_taps(16, 8)[0] is bicubic_taps(16, 8)[0]          # cached
    with pytest.raises(ValueError):
        bicubic_taps(0, 4)


def test_supersampled_size(ngp):
    from ngp_amd.imaging import supersampled_size
    assert supersampled_size(80, 80, 2) == (160, 160)
    assert supersampled_size(80, 80, 1.5) == (120, 120)
    assert supersampled_size(33, 47, 1.5) == (49, 70)               # int() truncates 49.5 and 70.5
    assert supersampled_size(7, 5, 1.0) == (7, 5)
    assert supersampled_size(101, 75, 2.5) == (252, 187)
    assert all(isinstance(v, int) for v in supersampled_size(33, 47, 1.5))


def _panorama_f64(H, W, forward, down, right, origin, radius):
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    theta = ((u - W / 2 + 0.5) * 2 * np.pi / W).reshape(-1, 1)
    phi = ((v - H / 2 + 0.5) * np.pi / H).reshape(-1, 1)
    f, d, r = (np.asarray(x, np.float64)[None] for x in (forward, down, right))
    dirs = np.sin(phi) * d + np.cos(phi) * np.sin(theta) * r + np.cos(phi) * np.cos(theta) * f
    dirs = dirs / np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-9)
    return np.asarray(origin, np.float64)[None] + radius * dirs, dirs


@pytest.mark.parametrize("H,W", [(32, 64), (7, 13)])
def test_panorama_rays_against_float64(ngp, H, W):
    """atol 2e-6: angles up to pi carry at most 2.4e-7 of float32 rounding through a handful of operations"""
    from ngp_amd.imaging import panorama_rays
    q, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(3, 3)))
    bases = [((0, 0, 1), (0, 1, 0), (1, 0, 0)), tuple(tuple(row) for row in q)]
    for forward, down, right in bases:
        for origin, radius in (((0.0, 0.0, 0.0), 0.0), ((0.25, -0.5, 0.125), 0.75)):
            rays_o, rays_d = panorama_rays(H, W, forward, down, right, origin=origin, radius=radius, device="cpu")
            assert rays_o.shape == rays_d.shape == (H * W, 3)
            assert rays_o.dtype == rays_d.dtype == torch.float32
            assert rays_o.is_contiguous() and rays_d.is_contiguous()
            want_o, want_d = _panorama_f64(H, W, forward, down, right, origin, radius)
            assert np.abs(rays_d.numpy() - want_d).max() <= 2e-6
            assert np.abs(rays_o.numpy() - want_o).max() <= 2e-6
            assert np.abs(np.linalg.norm(rays_d.numpy().astype(np.float64), axis=1) - 1).max() <= 2e-6
            # the origins lie `radius` along their own rays
            assert np.abs((rays_o.numpy() - np.float32(origin)) - np.float32(radius) * rays_d.numpy()).max() <= 2e-6
    # the two centre columns straddle `forward` on the equator rows; with an odd W the centre column looks along it
    _, d = panorama_rays(8, 9, (0, 0, 1), (0, 1, 0), (1, 0, 0))
    d = d.reshape(8, 9, 3).numpy()
    assert np.abs(d[:, 4, 0]).max() <= 2e-6 and (d[:, 4, 2] > 0).all()         # no `right` component, forward
    mid = 0.5 * (d[3, 4] + d[4, 4])                                             # rows 3 and 4 straddle the equator
    assert np.abs(mid / np.linalg.norm(mid) - np.float32([0, 0, 1])).max() <= 2e-6
    assert d[0, 4, 1] < 0 < d[7, 4, 1] and d[4, 0, 0] < 0 < d[4, 8, 0]          # down grows with v, right with u


def test_render_parser_anti_aliasing():
    import render
    base = ["--ckpt", "a", "--root_dir", "b", "--out_dir", "c", "--render_rgb"]
    args = render.parse_args(base)
    assert args.anti_aliasing_factor == 1.0 and args.aa_host_check is False
    args = render.parse_args(base + ["--render_depth", "--render_normal", "--anti_aliasing_factor", "1.5",
                                     "--aa_host_check"])
    assert args.anti_aliasing_factor == 1.5 and args.aa_host_check
    assert render.parse_args(base + ["--anti_aliasing_factor", "8"]).anti_aliasing_factor == 8.0
    for bad in (["--anti_aliasing_factor", "9"], ["--anti_aliasing_factor", "0.5"],
                ["--anti_aliasing_factor", "2", "--render_semantic"], ["--anti_aliasing_factor", "2", "--render_points"],
                ["--anti_aliasing_factor", "2", "--render_traj"], ["--aa_host_check"]):
        with pytest.raises(SystemExit) as e:
            render.parse_args(base + bad)
        assert e.value.code == 2, bad
    # the combinations stay allowed at one ray per pixel
    assert render.parse_args(base + ["--render_semantic", "--render_points", "--render_traj"]).render_traj


def test_render_panorama_parser():
    import render_panorama as rp
    base = ["--ckpt", "a", "--out_dir", "c", "--pano_hw", "32", "64", "--v_forward", "0", "0", "1", "--v_down", "0", "1",
            "0", "--v_right", "1", "0", "0"]
    args = rp.parse_args(base)
    assert args.pano_hw == [32, 64] and args.v_forward == [0.0, 0.0, 1.0] and args.v_down == [0.0, 1.0, 0.0]
    assert args.v_right == [1.0, 0.0, 0.0] and args.origin == [0.0, 0.0, 0.0] and args.pano_radius == 0.0
    assert args.scale == 0.5 and args.exp_step_factor == 0.0 and args.anti_aliasing_factor == 1.0
    assert args.render_depth is False
    args = rp.parse_args(base + ["--origin", "0.1", "0.2", "0.3", "--pano_radius", "0.5", "--anti_aliasing_factor", "2",
                                 "--render_depth", "--scale", "8", "--exp_step_factor", "0.00390625"])
    assert args.origin == [0.1, 0.2, 0.3] and args.pano_radius == 0.5 and args.anti_aliasing_factor == 2.0
    assert args.render_depth and args.scale == 8.0
    for bad in (["--anti_aliasing_factor", "9"], ["--anti_aliasing_factor", "0.5"], ["--pano_hw", "0", "64"]):
        with pytest.raises(SystemExit) as e:
            rp.parse_args(base + bad)
        assert e.value.code == 2, bad
    with pytest.raises(SystemExit):
        rp.parse_args(base[:4])                                                # the basis vectors are required
