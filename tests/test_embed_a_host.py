"""Appearance codes (embed_a) without a GPU: appearance.FrameEmbedding against the reference's own class (G18,
tests/golden/make_golden_embed.py), the 'embedding_a.' checkpoint prefix, the RayCodes carrier's argument checks, the two
new prototypes of the C ABI and the tools' new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_frame_embedding.npz")


@pytest.fixture()
def frame_embedding(ngp, g18):
    from ngp_amd.appearance import FrameEmbedding
    fe = FrameEmbedding(8, torch.from_numpy(g18["poses"]))
    assert isinstance(fe.embedding_a, torch.nn.Embedding) and tuple(fe.embedding_a.weight.shape) == (12, 8)
    with torch.no_grad():
        fe.embedding_a.weight.copy_(torch.from_numpy(g18["weight"]))
    return fe


def test_frame_embedding_equals_the_reference_in_all_three_modes(frame_embedding, g18):
    """exact equality: index (int, 1-D, 2-D; also as the default mode), nearest and mean for every recorded query pose —
    a training pose itself, the midpoint of two training cameras and a far-away pose among them"""
    fe = frame_embedding
    with torch.no_grad():
        for i, pose in enumerate(torch.from_numpy(g18["query_poses"])):
            for mode in ("nearest", "mean"):
                got = fe(pose, mode=mode)
                assert got.shape == (1, 8)
                assert np.array_equal(got.numpy(), g18[mode][i]), (mode, i)
        assert np.array_equal(fe(int(g18["index_int"]), mode="index").numpy(), g18["index_int_out"])
        assert np.array_equal(fe(torch.from_numpy(g18["index_1d"]), mode="index").numpy(), g18["index_1d_out"])
        assert np.array_equal(fe(torch.from_numpy(g18["index_2d"])).numpy(), g18["index_2d_out"])
    # the training pose itself is its own nearest camera
    assert np.array_equal(g18["nearest"][4][0], g18["weight"][5])


def test_default_initialisation_is_the_embedding_layers(ngp):
    from ngp_amd.appearance import FrameEmbedding
    torch.manual_seed(5)
    a = FrameEmbedding(4, torch.zeros(300, 3, 4)).embedding_a.weight
    torch.manual_seed(5)
    b = torch.nn.Embedding(300, 4).weight
    assert torch.equal(a, b)                       # N(0, 1), drawn as nn.Embedding draws it


def test_unknown_mode_raises(frame_embedding, g18):
    assert str(g18["unknown_mode_error"]) == "ValueError"
    with pytest.raises(ValueError, match="Invalid mode"):
        frame_embedding(torch.zeros(3, 4), mode="median")


def test_checkpoint_round_trip_of_the_embedding_a_prefix(ngp, frame_embedding, g18, tmp_path):
    """save_ckpt(..., embedding_a=) writes 'embedding_a.weight' beside 'model.' and 'msk_model.' in the reference's key
    order; FrameEmbedding(E, poses, path) and the reference's load_ckpt call restore it; the tools' call, which ignores
    the prefix, still loads the scene model from the same file; a table of another size raises"""
    from ngp_amd import ckpt
    from ngp_amd.appearance import FrameEmbedding
    from ngp_amd.implicit_mask import implicit_mask
    torch.manual_seed(3)
    model, msk = torch.nn.Linear(3, 2), implicit_mask()
    path = os.path.join(tmp_path, "a.ckpt")
    ckpt.save_ckpt(model, path, msk_model=msk, embedding_a=frame_embedding.embedding_a)
    assert list(torch.load(path, weights_only=True)["state_dict"]) == [str(k) for k in g18["ckpt_keys"]]
    poses = torch.from_numpy(g18["poses"])
    fresh = FrameEmbedding(8, poses, path)
    assert torch.equal(fresh.embedding_a.weight, torch.from_numpy(g18["weight"]))
    bare = torch.nn.Embedding(12, 8)
    ckpt.load_ckpt(bare, path, model_name='embedding_a', prefixes_to_ignore=['model', 'msk_model'])
    assert torch.equal(bare.weight, torch.from_numpy(g18["weight"]))
    other = torch.nn.Linear(3, 2)
    ckpt.load_ckpt(other, path, prefixes_to_ignore=['embedding_a', 'msk_model'])
    assert torch.equal(other.weight, model.weight) and torch.equal(other.bias, model.bias)
    for n_imgs, E in ((11, 8), (12, 4)):
        with pytest.raises(RuntimeError, match="size mismatch"):
            FrameEmbedding(E, poses[:n_imgs], path)
    # a FrameEmbedding is accepted in place of its table, and without the argument the file is what it was before
    ckpt.save_ckpt(model, path, embedding_a=frame_embedding)
    assert list(torch.load(path, weights_only=True)["state_dict"]) == ["model.weight", "model.bias", "embedding_a.weight"]
    ckpt.save_ckpt(model, path)
    assert set(torch.load(path, weights_only=True)["state_dict"]) == {"model.weight", "model.bias"}


def test_ray_codes_checks_its_arguments(ngp):
    from ngp_amd.appearance import RayCodes
    from ngp_amd.rendering import render
    w = torch.zeros(6, 8)
    rc = RayCodes(torch.nn.Embedding(6, 8), [0, 5, 2])
    assert rc.img_idxs.dtype == torch.int64 and rc.rays_a is None and tuple(rc.weight.shape) == (6, 8)
    with pytest.raises(ValueError, match="1 to 32"):
        RayCodes(torch.zeros(6, 33), [0])
    with pytest.raises(ValueError, match="float32"):
        RayCodes(torch.zeros(6, 8, dtype=torch.float64), [0])
    with pytest.raises(ValueError, match="integer"):
        RayCodes(w, torch.zeros(3))
    with pytest.raises(ValueError, match="batch has 2"):
        rc.for_batch(torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="not bound"):
        rc.expand()
    rays_a = torch.tensor([[2, 0, 2], [0, 2, 0], [1, 2, 3]])
    bound = RayCodes(torch.arange(48, dtype=torch.float32).reshape(6, 8), [0, 5, 9]).for_batch(rays_a)
    want = torch.arange(48, dtype=torch.float32).reshape(6, 8)[[0, 0, 5, 5, 5]]
    want[:2] = 0                                             # ray 2 names image 9 of 6: zeros
    assert torch.equal(bound.expand(), want)
    # test-time rendering refuses the carrier before anything is launched
    with pytest.raises(ValueError, match="test-time"):
        render(None, torch.zeros(1, 3), torch.ones(1, 3), test_time=True, embedding_a=rc)


def test_trainer_argument_is_checked(ngp):
    """NGPTrainer refuses a table whose code length is not the model's"""
    import inspect
    from ngp_amd.trainer import NGPTrainer
    sig = inspect.signature(NGPTrainer.__init__).parameters
    assert "embedding_a" in sig and sig["embedding_a"].default is None
    assert "img_idxs" in inspect.signature(NGPTrainer.step).parameters


def test_header_prototypes_parse(ngp):
    from ngp_amd import _lib, build
    protos = _lib.parse_header()
    names = lambda k: [a for _, a in protos[k][1]]
    assert names("ngp_embed_a_fwd") == ["weight", "n_imgs", "E", "img_idxs", "rays_a", "n_rays", "out", "ld", "n_cols",
                                        "stream"]
    assert names("ngp_embed_a_bwd") == ["dL_dcols", "ld", "E", "img_idxs", "rays_a", "n_rays", "n_imgs", "d_weight",
                                        "stream"]
    import ctypes as C
    assert [t for t, _ in protos["ngp_embed_a_fwd"][1]] == [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    assert "embed_kernels.hip" in [s for s, _ in build.SOURCES]
    assert os.path.exists(os.path.join(build.CSRC, "embed_kernels.hip"))


@pytest.mark.parametrize("tool,flags", [
    ("train_dataset.py", ("--embed_a", "--embed_a_len", "--embed_msk")),
    ("render.py", ("--embed_a", "--embed_a_len", "--embed_a_mode")),
    ("render_panorama.py", ("--embed_a", "--embed_a_len")),
    ("extract_mesh.py", ("--embed_a", "--embed_a_len")),
    pytest.param("step_bench.py embed_a", ("--leg", "--solo"), id="step_bench.py-embed_a"),
])
def test_tools_accept_the_new_flags(tool, flags):
    tool, *recipe = tool.split()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *recipe, "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for f in flags:
        assert f in out.stdout, (tool, f)
    if tool == "render.py":
        assert "{mean,nearest,index}" in out.stdout
    if recipe == ["embed_a"]:
        assert "{none,tensor,fused}" in out.stdout
