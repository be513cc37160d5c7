"""Transient mask field (implicit_mask) and the masked loss, without a GPU: the float64 restatement of
tests/mask_reference.py against the reference's own run (G17, tests/golden/make_golden_mask.py), this package's
NeRFLoss(embed_msk=True) on CPU tensors, the module's state dict / uvi / checkpoint prefix, and the selection rule
of the GPU tests."""
import os

import numpy as np
import pytest
import torch

import mask_reference as R
from helpers import table_rule

RTOL, ATOL = 1e-5, 1e-6      # tests/test_oracle_golden.py's bar for reference-pinned quantities


@pytest.fixture(scope="module")
def g17(golden):
    g = golden("g17_implicit_mask.npz")
    p = {k: g["param_" + k] for k in R.KEYS if k != "mask_encoder.params"}
    p["mask_encoder.params"] = table_rule(R.SHAPES["mask_encoder.params"][0], float(g["table_rule_amp"]))
    return g, p


def test_restatement_reproduces_the_reference_mask_and_gradients(g17):
    """mask_reference.forward / masked_loss / backward against what the reference's implicit_mask + NeRFLoss returned
    at step 0 and at the annealing floor (step 5000)"""
    g, p = g17
    uvi = g["uvi"]
    fwd = R.forward(p, uvi)
    for step in g["steps"]:
        sd = float(g[f"size_delta_{step}"])
        assert sd == (1.0 if step == 0 else 6e-2)
        np.testing.assert_allclose(fwd["mask"], g[f"mask_{step}"][:, 0], rtol=RTOL, atol=ATOL)
        r_ms, term, d_mask, _ = R.masked_loss(g["in_rgb"], g["tgt_rgb"], fwd["mask"], sd)
        np.testing.assert_allclose(r_ms, g[f"term_r_ms_{step}"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(term, g[f"term_rgb_{step}"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(d_mask, g[f"grad_mask_{step}"][:, 0], rtol=RTOL, atol=ATOL)
        grads = R.backward(p, uvi, d_mask, fwd)
        for k in R.KEYS[1:]:
            np.testing.assert_allclose(grads[k].reshape(R.SHAPES[k]), g[f"grad_{k}_{step}"], rtol=RTOL, atol=ATOL, err_msg=k)
        want = np.zeros(R.SHAPES["mask_encoder.params"], np.float32)
        want[g[f"grad_table_idx_{step}"]] = g[f"grad_table_val_{step}"]
        assert np.count_nonzero(want) > 1000
        np.testing.assert_allclose(grads["mask_encoder.params"], want, rtol=RTOL, atol=ATOL)


def test_package_loss_reproduces_the_reference_terms(ngp, g17):
    """losses.NeRFLoss(embed_msk=True) on CPU tensors: r_ms and the masked colour term, and through autograd the
    gradient w.r.t. the mask (the distortion term needs the GPU and does not depend on the mask: switched off here)"""
    from ngp_amd.losses import NeRFLoss
    g, _ = g17
    loss_fn = NeRFLoss()
    loss_fn.lambda_distortion = 0
    res = {"rgb": torch.from_numpy(g["in_rgb"]), "opacity": torch.from_numpy(g["in_opacity"])}
    for step in g["steps"]:
        mask = torch.from_numpy(g[f"mask_{step}"]).clone().requires_grad_(True)
        d = loss_fn(res, {"rgb": torch.from_numpy(g["tgt_rgb"])}, embed_msk=True, mask=mask, step=int(step))
        assert list(d) == ["r_ms", "rgb", "opacity"]
        np.testing.assert_allclose(d["r_ms"].detach().numpy(), g[f"term_r_ms_{step}"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(d["rgb"].detach().numpy(), g[f"term_rgb_{step}"], rtol=RTOL, atol=ATOL)
        sum(t.mean() for t in d.values()).backward()
        np.testing.assert_allclose(mask.grad.numpy(), g[f"grad_mask_{step}"], rtol=RTOL, atol=ATOL)


def test_state_dict_matches_the_reference(ngp, g17):
    from ngp_amd.implicit_mask import implicit_mask
    g, _ = g17
    msk = implicit_mask()
    got = [f"{k}:{','.join(map(str, v.shape))}" for k, v in msk.state_dict().items()]
    assert got == [str(s) for s in g["param_shapes"]]
    assert {k: tuple(v.shape) for k, v in msk.state_dict().items()} == R.SHAPES
    desc = msk.mask_encoder.desc
    assert [int(desc.offsets[l + 1] - desc.offsets[l]) for l in range(8)] == [4096, 32768] + [65536] * 6
    t = msk.mask_encoder.params.detach()
    assert float(t.abs().max()) <= 1e-4 and float(t.abs().max()) > 0.9e-4          # tinycudann.Encoding's +-1e-4
    assert implicit_mask(latent=8, W=16).state_dict().keys() == msk.state_dict().keys()   # both arguments are unused


def test_uvi_matches_the_reference(ngp, g17):
    from ngp_amd.implicit_mask import implicit_mask
    g, _ = g17
    w, h = (int(v) for v in g["img_wh"])
    uvi = implicit_mask.uvi(torch.from_numpy(g["uv"]), torch.from_numpy(g["img_idxs"]), (w, h), int(g["n_imgs"]))
    assert uvi.dtype == torch.float32 and uvi.shape == (len(g["uv"]), 3)
    assert np.array_equal(uvi.numpy(), g["uvi"])
    assert (uvi[0] == -0.5).all() and (uvi[1] == 0).all()


def test_cpu_tensors_raise(ngp):
    from ngp_amd.implicit_mask import implicit_mask
    with pytest.raises(RuntimeError, match="CUDA"):
        implicit_mask()(torch.zeros(4, 3))


def test_checkpoint_round_trip_of_the_msk_model_prefix(ngp, tmp_path):
    """save_ckpt writes the mask model under 'msk_model.' beside 'model.'; the reference's call (train.py:236) restores
    it, and the render tools' call (which ignores the prefix) still loads the scene model from the same file"""
    from ngp_amd import ckpt
    from ngp_amd.implicit_mask import implicit_mask
    torch.manual_seed(3)
    model, msk = torch.nn.Linear(3, 2), implicit_mask()
    with torch.no_grad():
        msk.mask_encoder.params.uniform_(-1, 1)
    path = os.path.join(tmp_path, "m.ckpt")
    ckpt.save_ckpt(model, path, msk_model=msk)
    keys = set(torch.load(path, weights_only=True)["state_dict"])
    assert keys == {"model.weight", "model.bias"} | {"msk_model." + k for k in R.KEYS}
    fresh = implicit_mask()
    ckpt.load_ckpt(fresh, path, model_name='msk_model', prefixes_to_ignore=['model', 'embedding_a'])
    for k, v in msk.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    other = torch.nn.Linear(3, 2)
    ckpt.load_ckpt(other, path, prefixes_to_ignore=['embedding_a', 'msk_model'])
    assert torch.equal(other.weight, model.weight)
    ckpt.save_ckpt(model, path)                      # without a mask model the file is what it was before
    assert set(torch.load(path, weights_only=True)["state_dict"]) == {"model.weight", "model.bias"}


def test_gpu_test_inputs_keep_their_promises():
    """the seeded batches of tests/test_mask_gpu.py, on the float64 reference: the rows left out of the backward tests
    (a first-layer pre-activation within RELU_MARGIN of zero) stay under the cap, both ReLU branches and both sigmoid
    tails occur, the special rows are there and every input lies in [-0.5, 0.5)"""
    p = R.make_params()
    for n in R.SIZES:
        uvi = R.make_uvi(n)
        assert uvi.shape == (n, 3) and uvi.min() >= -0.5 and uvi.max() < 0.5
        keep = R.select_rows(p, uvi)
        assert 1.0 - keep.mean() <= R.MAX_DROPPED, (n, keep.mean())
        f = R.forward(p, uvi)
        assert 0.1 < (f["z1"] > 0).mean() < 0.9
        if n >= 63:
            assert f["mask"].min() < 0.2 and f["mask"].max() > 0.8, (n, f["mask"].min(), f["mask"].max())
            assert (uvi[0] == -0.5).all() and (uvi[1] == 0).all() and (uvi[3] == np.float32(0.49999997)).all()
            m32 = f["mask"].astype(np.float32)
            assert m32.min() > 0 and m32.max() < 1
