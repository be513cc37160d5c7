"""The HDR-NeRF recipe (use_exposure) without a GPU: the float64 restatement of the tone-mappers (tonemap_reference.py)
against the reference's recorded outputs (G13) and against central differences, the HDR-NeRF synthetic exporter read back
by the COLMAP loader, the trainer's and the tools' refusals, and the C interface's declarations."""
import os
import sys

import numpy as np
import pytest
import torch

import tonemap_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def g13_params(g):
    return [g[f"tonemapper_net_{i}.params"] for i in range(3)]


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_matches_reference_golden(golden):
    """G13 holds the reference's own tone-mapped colours of 160 samples and their radiances exp(log-radiance): the
    restatement at u = ln(radiance) gives fwd_ldr_rgbs, with the recorded exposure fwd_ldr_exposure_rgbs, and at zero
    log-radiance and unit exposure unit_exposure_rgb; tolerances of test_tonemapper_and_exposure_match_reference_golden"""
    g = golden("g13_tonemapper.npz")
    p = g13_params(g)
    u = np.log(g["fwd_radiance_rgbs"].astype(np.float64))
    close(R.forward(p, u), g["fwd_ldr_rgbs"], 5e-4, 1e-5)
    close(R.forward(p, u, g["exposure"]), g["fwd_ldr_exposure_rgbs"], 5e-4, 1e-5)
    close(R.forward(p, u, g["exposure"]), g["test_ldr_exposure_rgbs"], 5e-4, 1e-5)
    close(R.forward(p, np.zeros((1, 3)), np.ones((1, 1))), g["unit_exposure_rgb"], 1e-5, 1e-6)
    # one broadcast value is that value for every sample; no exposure is unit exposure
    close(R.forward(p, u, np.full((1, 1), 2.5)), R.forward(p, u, np.full((160, 1), 2.5)), 0, 0)
    close(R.forward(p, u), R.forward(p, u, np.ones(1)), 0, 0)


def test_restatement_backward_against_central_differences(golden):
    """the analytic backward against central differences of sum(rgb * dL_drgb) in float64: every input gradient, and every
    parameter of W1 column 0, of two padding columns and of W2 row 0; rows 1..15 of W2 get exactly nothing, the 15 padding
    columns of a row of W1 the same sum.  Samples whose pre-activations lie within the step of a ReLU kink are left out of
    the comparison's inputs (the difference quotient straddles the kink there)."""
    g = golden("g13_tonemapper.npz")
    p = [a.astype(np.float64) for a in g13_params(g)]
    rng = np.random.default_rng(5)
    n, h = 40, 1e-6
    u = rng.uniform(-6, 6, (n, 3))
    e = rng.choice([0.125, 0.5, 2.0, 8.0, 32.0], (n, 1))
    le = np.log(e)
    for c in range(3):   # move samples away from every kink of their channel
        W1, _ = R.split(p[c])
        for _ in range(50):
            z = np.outer(u[:, c] + le[:, 0], W1[:, 0]) + W1[:, 1:].sum(1)
            bad = (np.abs(z) < 1e-3).any(1)
            if not bad.any():
                break
            u[bad, c] = rng.uniform(-6, 6, int(bad.sum()))
        assert not bad.any()
    dy = rng.normal(size=(n, 3))
    dlr, dparams, scale = R.backward(p, u, e, dy)
    assert (scale >= np.abs(dparams) - 1e-12).all()
    for i in range(n):
        for c in range(3):
            up, um = u.copy(), u.copy()
            up[i, c] += h
            um[i, c] -= h
            fd = (R.loss(p, up, e, dy) - R.loss(p, um, e, dy)) / (2 * h)
            assert abs(fd - dlr[i, c]) <= 1e-6 * max(1.0, abs(fd)), (i, c, fd, dlr[i, c])
    for c in range(3):
        d = dparams[c]
        assert not d[R.H * R.IN + R.H:].any()                      # rows 1..15 of W2
        dW1 = d[:R.H * R.IN].reshape(R.H, R.IN)
        close(dW1[:, 1:], np.repeat(dW1[:, 1:2], 15, 1), 1e-13, 1e-15)
        idx = [j * R.IN + k for j in (0, 7, 63) for k in (0, 1, 15)] + [R.H * R.IN + j for j in (0, 31, 63)]
        for k in idx:
            pp, pm = [a.copy() for a in p], [a.copy() for a in p]
            pp[c][k] += h
            pm[c][k] -= h
            fd = (R.loss(pp, u, e, dy) - R.loss(pm, u, e, dy)) / (2 * h)
            assert abs(fd - d[k]) <= 1e-6 * max(1.0, abs(fd)), (c, k, fd, d[k])


def test_restatement_edges(golden):
    """dead hidden layer: every gradient exactly 0; a z_j of exactly 0 has derivative 0"""
    g = golden("g13_tonemapper.npz")
    p = [np.abs(a.astype(np.float64)) for a in g13_params(g)]     # positive W1[:, 0] ...
    for a in p:
        a[:R.H * R.IN].reshape(R.H, R.IN)[:, 1:] = -0.01           # ... and biases that cannot lift u = -40 above 0
    dlr, dparams, scale = R.backward(p, np.full((5, 3), -40.0), None, np.ones((5, 3)))
    assert not dlr.any() and not dparams.any() and not scale.any()
    p[0][:R.IN] = 0.0                                              # unit 0 of channel 0: z = 0 for every input
    base = R.backward(p, np.full((1, 3), 1.0), None, np.ones((1, 3)))[1]
    assert not base[0][:R.IN].any() and base[0][R.H * R.IN] == 0.0


# ------------------------------------------------------------------------------------------- exporter and loader
def _tiny_hdr_scene(root, h=4, w=6):
    from ngp_amd.datasets import export
    rng = np.random.default_rng(11)
    radiance = rng.uniform(0.0, 1.0, (35, h, w, 3))
    radiance[:, 0, 0] = 0.0
    c2w = np.zeros((35, 3, 4))
    for i in range(35):
        a = 0.3 * i
        c2w[i, :, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c2w[i, :, 3] = (1.0 + 0.02 * i) * np.array([np.sin(a), 0.1, np.cos(a)])
    K = np.array([[5.0, 0, w / 2], [0, 5.0, h / 2], [0, 0, 1]])
    return export.export_hdr_nerf_syn(root, radiance, c2w, K, scene="chair"), radiance, c2w


def test_exporter_output_is_read_back_by_the_loader(ngp, tmp_path):
    from ngp_amd.datasets import ColmapDataset, export
    from ngp_amd.datasets.colmap import _HDR_EXPOSURES
    root = str(tmp_path / "tmp.dir" / "HDR-NeRF" / "syndata" / "chair")   # (a dot in a directory name is no file suffix)
    out, radiance, c2w = _tiny_hdr_scene(root)
    assert out == root
    assert sorted(os.listdir(os.path.join(root, "train"))) == [f"{i:03d}_{e}.png" for i in range(17, 35) for e in (0, 2, 4)]
    assert sorted(os.listdir(os.path.join(root, "test"))) == [f"{i:03d}_{e}.png" for i in range(17) for e in (1, 3)]
    assert sorted(os.listdir(root)) == ["sparse", "test", "train"]
    times = _HDR_EXPOSURES["chair"]
    assert [times[e] for e in range(5)] == [0.125, 0.5, 2.0, 8.0, 32.0]
    train, test = ColmapDataset(root, "train"), ColmapDataset(root, "test")
    assert train.unit_exposure_rgb == 0.73 and test.unit_exposure_rgb == 0.73
    assert tuple(train.rays.shape) == (54, 24, 4) and tuple(test.rays.shape) == (34, 24, 4)
    assert tuple(train.poses.shape) == (54, 3, 4) and tuple(test.poses.shape) == (34, 3, 4)
    # the poses repeat as _hdr_split repeats them: pose-major, exposure-minor; rescaled by the largest camera distance
    far = np.linalg.norm(c2w[:, :, 3], axis=-1).max()
    want = c2w.copy()
    want[:, :, 3] /= far
    close(train.poses.numpy(), np.repeat(want[17:], 3, 0), 0, 1e-5)
    close(test.poses.numpy(), np.repeat(want[:17], 2, 0), 0, 1e-5)
    # the fourth column holds the table's times, in that order, and the colours are the response at those times
    close(train.rays[:, :, 3].numpy(), np.tile(np.repeat([[0.125], [2.0], [32.0]], 24, 1), (18, 1)), 0, 0)
    close(test.rays[:, :, 3].numpy(), np.tile(np.repeat([[0.5], [8.0]], 24, 1), (17, 1)), 0, 0)
    for k, (i, t) in enumerate((i, t) for i in range(17, 35) for t in (0.125, 2.0, 32.0)):
        want_rgb = (export.hdr_response(radiance[i], t) * 255.0 + 0.5).astype(np.uint8).reshape(24, 3) / 255.0
        close(train.rays[k, :, :3].numpy(), want_rgb, 0, 1e-6)
    assert not train.rays[:, 0, :3].any()                            # zero radiance stays black at every exposure
    close(export.hdr_response(1.0, 1.0), 0.73, 1e-15, 0)             # unit radiance at unit exposure
    x = np.array([0.03, 0.4, 2.0])
    close(export.hdr_response(x, 8.0), 1 / (1 + np.exp(-(np.log(x * 8.0) + np.log(0.73 / 0.27)))), 1e-13, 0)
    # samples: a per-ray exposure column when training, one value per test image
    torch.manual_seed(0)
    train.batch_size = 16
    s = train[0]
    assert tuple(s["exposure"].shape) == (16, 1) and tuple(s["rgb"].shape) == (16, 3)
    assert set(np.unique(s["exposure"].numpy())) <= {0.125, 2.0, 32.0}
    assert float(test[3]["exposure"]) == 8.0 and test[3]["exposure"].dim() == 0


def test_exporter_refuses_what_the_loader_could_not_read(ngp, tmp_path):
    from ngp_amd.datasets import export
    K, c2w = np.eye(3), np.zeros((35, 3, 4))
    with pytest.raises(ValueError, match="35 poses"):
        export.export_hdr_nerf_syn(str(tmp_path / "HDR-NeRF" / "syndata" / "chair"), np.zeros((34, 2, 2, 3)), c2w, K)
    with pytest.raises(ValueError, match="must end in"):
        export.export_hdr_nerf_syn(str(tmp_path / "chair"), np.zeros((35, 2, 2, 3)), c2w, K)
    with pytest.raises(ValueError, match="exposure table"):
        export.export_hdr_nerf_syn(str(tmp_path / "HDR-NeRF" / "syndata" / "stool"), np.zeros((35, 2, 2, 3)), c2w, K,
                                   scene="stool")


# ------------------------------------------------------------------------------------------- the trainer
class _Head:
    n_output_dims = 7


class _Model:          # what the construction checks look at
    rgb_act, use_skybox, differentiable_normals = "None", False, False
    semantic_header = _Head()


def test_trainer_refuses_what_use_exposure_does_not_cover(ngp):
    """construction only: every refusal is decided before the trainer touches its parameters"""
    from ngp_amd.implicit_mask import implicit_mask
    from ngp_amd.trainer import NGPTrainer
    sig = _Model()
    sig.rgb_act = "Sigmoid"
    with pytest.raises(ValueError, match="rgb_act='None'"):
        NGPTrainer(sig, use_exposure=True)
    for kw, what in ((dict(msk_model=implicit_mask()), "a msk_model"), (dict(pose_refiner=object()), "a pose_refiner"),
                     (dict(render_kwargs={"use_skybox": True}), "a skybox")):
        with pytest.raises(ValueError, match="use_exposure=True does not combine with " + what):
            NGPTrainer(_Model(), use_exposure=True, **kw)
    sky = _Model()
    sky.use_skybox = True
    with pytest.raises(ValueError, match="a skybox"):
        NGPTrainer(sky, use_exposure=True)
    # the fused-tail options refuse a tone-mapped model through their existing message
    for kw in (dict(semantic=True), dict(normal_mono=True), dict(depth_mono=True), dict(multi_terms=("depth_mono",))):
        with pytest.raises(ValueError, match="rgb_act != 'Sigmoid'"):
            NGPTrainer(_Model(), use_exposure=True, **kw)


def test_step_checks_the_exposure(ngp):
    """step()'s checks come before anything touches the device"""
    from ngp_amd.recipe import Recipe
    from ngp_amd.trainer import NGPTrainer

    class _Plain:          # what step() looks at before its first launch
        model, recipe = None, Recipe(use_exposure=False)

    class _Hdr(_Plain):
        recipe = Recipe(use_exposure=True)

    class _Old:          # the default recipe
        model, recipe = None, Recipe()
    o, d, gt, e = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, 3), torch.ones(6, 1)
    for tr in (_Plain(), _Old()):
        with pytest.raises(ValueError, match="exposure= is for a trainer built with use_exposure=True"):
            NGPTrainer.step(tr, o, d, gt, exposure=e)
    with pytest.raises(ValueError, match="needs exposure="):
        NGPTrainer.step(_Hdr(), o, d, gt)
    for bad in (e[:5], torch.ones(6, 2), torch.ones(6, 1, dtype=torch.int64), torch.ones(6, 1, 1), 2.0):
        with pytest.raises(ValueError, match="exposure= must be"):
            NGPTrainer.step(_Hdr(), o, d, gt, exposure=bad)
    for good in (e, e.reshape(6)):
        with pytest.raises(RuntimeError, match="exposure must be a CUDA tensor"):
            NGPTrainer.step(_Hdr(), o, d, gt, exposure=good)


def test_model_refuses_cpu_tensors(ngp):
    model = ngp.networks.NGP(scale=0.5, rgb_act="None")
    assert model._stock_tonemappers() is not None
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model.log_radiance_to_rgb(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model.log_radiance_to_rgb(torch.zeros(4, 3), exposure=torch.ones(4, 1))


# ------------------------------------------------------------------------------------------- the tools' flags
def test_tool_flags(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render
    import train_dataset as td
    a = td.parse_args(["--make_proxy", "x", "--dataset_name", "colmap", "--use_exposure"])
    assert a.use_exposure and a.scale == 0.5
    assert not td.parse_args(["--root_dir", "x"]).use_exposure
    for bad in (["--embed_msk"], ["--optimize_ext"], ["--render_semantic"], ["--normal_mono"], ["--depth_mono"],
                ["--multi_terms", "depth_mono"]):
        with pytest.raises(SystemExit) as ex:
            td.parse_args(["--root_dir", "x", "--use_exposure"] + bad)
        assert ex.value.code == 2
    with pytest.raises(SystemExit) as ex:
        td.parse_args(["--make_proxy", "x", "--dataset_name", "tnt", "--use_exposure"])
    assert ex.value.code == 2
    td.parse_args(["--root_dir", "x", "--use_exposure", "--embed_a", "--random_bg"])
    base = ["--ckpt", "c", "--root_dir", "x", "--out_dir", "o", "--render_rgb"]
    r = render.parse_args(base + ["--use_exposure", "--exposure", "0.5"])
    assert r.use_exposure and r.exposure == 0.5
    assert render.parse_args(base + ["--use_exposure"]).exposure is None
    for bad in (["--exposure", "0.5"], ["--use_exposure", "--exposure", "0"]):
        with pytest.raises(SystemExit) as ex:
            render.parse_args(base + bad)
        assert ex.value.code == 2


def test_train_refuses_a_dataset_without_exposures(ngp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_dataset as td

    class _Set:
        rays = torch.zeros(2, 4, 3)
        poses = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="--use_exposure needs an exposure time per ray"):
        td.train(None, _Set(), 1, 1, 4, 1e-2, use_exposure=True)


# ------------------------------------------------------------------------------------------- the C interface
def test_entries_are_declared_and_built(ngp):
    from ngp_amd import _lib, build
    assert "tonemap_kernels.hip" in [s for s, _ in build.SOURCES]
    fwd, bwd, ws = (_lib.PROTOS[f"ngp_tonemap_{k}"] for k in ("fwd", "bwd", "bwd_workspace"))
    assert [n for _, n in fwd[1]] == ["params0", "params1", "params2", "log_radiance", "exposure", "exposure_stride", "n",
                                      "rgb", "stream"]
    assert [n for _, n in bwd[1]] == ["params0", "params1", "params2", "log_radiance", "exposure", "exposure_stride",
                                      "dL_drgb", "n", "d_log_radiance", "dparams0", "dparams1", "dparams2", "workspace",
                                      "stream"]
    assert [n for _, n in ws[1]] == ["n"]
    # one row of 576 partial sums (doubles, counted in floats) per workgroup, a workgroup per tile of 256 samples up to
    # NGP_TONEMAP_BWD_MAX_BLOCKS
    assert [_lib.call_host("tonemap_bwd_workspace", n) for n in (0, 1, 256, 257, 512 * 256, 10 ** 12, -1)] == \
        [0, 1152, 1152, 2304, 512 * 1152, 512 * 1152, -22]
    assert "#define NGP_TONEMAP_BWD_MAX_BLOCKS 512" in open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    src = open(os.path.join(ROOT, "instant-ngp-pp_amd", "csrc", "tonemap_kernels.hip")).read()
    assert "atomicAdd" not in src and "printf" not in src and "asm" not in src
