#!/usr/bin/env python3
"""Writes g17_implicit_mask.npz by RUNNING THE REFERENCE'S OWN models/implicit_mask.py and losses.NeRFLoss on the CPU.

Runs only where the reference tree is at hand (make_golden.py's REF); the tests use the committed .npz.  `tinycudann` is
tcnn_cpu_shim.py, `vren`'s distortion entry points are the C oracle's (make_golden.install_oracle_vren), as for G14.
Before anything is recorded the shim's grid is asserted equal to oracle.grid_fwd on the recorded uvi — which lies in
[-0.5, 0.5) and so has NEGATIVE grid coordinates: the shim reduces a signed index with a floored modulo, the oracle
(and tiny-cuda-nn) wrap an unsigned one; every level of this configuration has a power-of-two size (4096, 32768,
6 x 65536), which divides 2^32, so the two coincide here.

One batch of 257 rays, at step 0 (size_delta 1) and at step 5000 (the annealing floor 6e-2): parameters, uv / image
indices / uvi (rows at -0.5 exactly and at 0 exactly included; the table follows make_golden.table_rule and its gradient
is stored as (index, value) pairs), the mask, the terms r_ms and rgb, and the gradients of
sum(term.mean()) (train.py:307) w.r.t. the mask and the five parameter tensors.  Numbers only.

  python tests/golden/make_golden_mask.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg   # noqa: E402  (its stubs and helpers are reused, the file itself stays as it is)

N_RAYS, IMG_WH, N_IMGS = 257, (40, 30), 10
STEPS = (0, 5000)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import oracle
    import tcnn_cpu_shim
    mg.import_reference()
    mg.install_oracle_vren(oracle)
    sys.modules["tinycudann"] = tcnn_cpu_shim
    ref_mask = _load("ref_implicit_mask", mg.REF + "/models/implicit_mask.py")
    ref_losses = _load("ref_losses", mg.REF + "/losses.py")

    torch.manual_seed(mg.SEED + 17)
    msk = ref_mask.implicit_mask()
    with torch.no_grad():   # tcnn's +-1e-4 tables would leave the mask a constant: a table that matters, by the rule the
        # tests reproduce (helpers.table_rule) instead of storing 3.4 MB
        msk.mask_encoder.params.copy_(torch.from_numpy(mg.table_rule(msk.mask_encoder.params.numel())))
    w, h = IMG_WH
    uv = torch.stack([torch.randint(h, (N_RAYS,)), torch.randint(w, (N_RAYS,))], -1)
    img_idxs = torch.randint(N_IMGS, (N_RAYS,))
    uv[0], img_idxs[0] = torch.tensor([0, 0]), 0                      # uvi = -0.5 exactly
    uv[1], img_idxs[1] = torch.tensor([h // 2, w // 2]), N_IMGS // 2   # uvi = 0 exactly
    uv[2], img_idxs[2] = torch.tensor([h - 1, w - 1]), N_IMGS - 1
    # train.py:281-287, with N_imgs = the number of training images
    uvi = torch.zeros((N_RAYS, 3))
    uvi[:, 0] = (uv[:, 0] - h / 2) / h
    uvi[:, 1] = (uv[:, 1] - w / 2) / w
    uvi[:, 2] = (img_idxs - N_IMGS / 2) / N_IMGS
    assert (uvi[0] == -0.5).all() and (uvi[1] == 0).all() and uvi.min() >= -0.5 and uvi.max() < 0.5

    enc = msk.mask_encoder
    desc, n_params = oracle.grid_layout(8, 2, 16, 16, float(np.exp(np.log(2048 / 16) / 7)))
    sizes = [int(desc.offsets[l + 1] - desc.offsets[l]) for l in range(8)]
    assert n_params == enc.params.numel() == 860160
    assert all(s & (s - 1) == 0 for s in sizes), sizes
    got = enc(uvi).detach().numpy()
    want = oracle.grid_fwd(desc, enc.params.detach().numpy(), uvi.numpy())
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (
        "tcnn_cpu_shim (signed floored modulo) and the oracle (unsigned wrap) disagree on negative coordinates: they "
        "coincide only while every level size is a power of two", float(np.abs(got - want).max()))

    counts = torch.randint(0, 9, (N_RAYS,))
    starts = torch.cumsum(counts, 0) - counts
    N = int(counts.sum())
    res = {"rgb": torch.rand(N_RAYS, 3), "opacity": torch.rand(N_RAYS) * 0.98 + 0.01, "ws": torch.rand(N) * 0.2,
           "deltas": torch.rand(N) * 0.01 + 1e-3, "ts": torch.sort(torch.rand(N) * 3)[0],
           "rays_a": torch.stack([torch.arange(N_RAYS), starts, counts], 1).long()}
    tgt = {"rgb": torch.rand(N_RAYS, 3)}
    params = dict(msk.named_parameters())
    out = {"uv": uv, "img_idxs": img_idxs, "img_wh": np.array(IMG_WH), "n_imgs": np.array(N_IMGS), "uvi": uvi,
           "steps": np.array(STEPS), "tgt_rgb": tgt["rgb"]}
    out.update({"in_" + k: v for k, v in res.items()})
    out.update({"param_" + k: v.detach().clone() for k, v in params.items() if k != "mask_encoder.params"})
    out["table_rule_amp"] = np.float64(0.6)
    out["param_shapes"] = np.array([f"{k}:{','.join(map(str, v.shape))}" for k, v in msk.state_dict().items()])
    loss_fn = ref_losses.NeRFLoss()
    for step in STEPS:
        msk.zero_grad()
        mask = msk(uvi)
        mask.retain_grad()
        loss_d = loss_fn(res, tgt, embed_msk=True, mask=mask, step=step)
        sum(lo.mean() for lo in loss_d.values()).backward()
        out[f"mask_{step}"] = mask.detach()
        out[f"size_delta_{step}"] = np.float64(loss_fn.Annealing.getWeight(step))
        out[f"term_r_ms_{step}"] = loss_d["r_ms"].detach()
        out[f"term_rgb_{step}"] = loss_d["rgb"].detach()
        out[f"grad_mask_{step}"] = mask.grad.clone()
        out.update({f"grad_{k}_{step}": v.grad.clone() for k, v in params.items() if k != "mask_encoder.params"})
        gt = params["mask_encoder.params"].grad     # 257 rays touch at most 257 * 8 * 8 rows: stored sparsely
        nz = torch.nonzero(gt)[:, 0]
        out[f"grad_table_idx_{step}"], out[f"grad_table_val_{step}"] = nz, gt[nz].clone()
    mg.npz("g17_implicit_mask.npz", **out)
    print(os.path.getsize(os.path.join(HERE, "g17_implicit_mask.npz")), "bytes")


if __name__ == "__main__":
    main()
