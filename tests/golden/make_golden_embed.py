#!/usr/bin/env python3
"""Writes g18_frame_embedding.npz by RUNNING THE REFERENCE'S OWN utils.FrameEmbedding on the CPU.

Runs only where the reference tree is at hand (make_golden.py's REF); the tests use the committed .npz.

Recorded: seeded training poses (12, 3, 4), a seeded table (12, 8), query poses — random ones, one that IS a training
pose, one at the midpoint of two training camera centres (equidistant from both up to rounding: what the reference
returns for it is what is stored) and one far outside — with the reference's result for mode 'nearest' and 'mean';
index queries (a Python int, a 1-D and a 2-D index tensor) with the result of mode 'index'; and the key list of a
checkpoint whose state dict holds model.*, msk_model.* and embedding_a.weight, registered in train.py's order (the scene
model is a stand-in Linear layer: only the prefixes matter here; the mask model is the reference's implicit_mask on
tcnn_cpu_shim.py, as for G17).  Numbers and names only.

  python tests/golden/make_golden_embed.py
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg   # noqa: E402  (its helpers are reused, the file itself stays as it is)

N_IMGS, E = 12, 8


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import tcnn_cpu_shim
    ref_utils = _load("ref_utils", mg.REF + "/utils.py")
    torch.manual_seed(mg.SEED + 18)
    poses = torch.randn(N_IMGS, 3, 4)
    fe = ref_utils.FrameEmbedding(E, poses)
    assert tuple(fe.embedding_a.weight.shape) == (N_IMGS, E)
    weight = fe.embedding_a.weight.detach().clone()

    q = [torch.randn(3, 4) for _ in range(4)]
    q.append(poses[5].clone())                                   # a training pose itself
    mid = torch.randn(3, 4)
    mid[:, 3] = 0.5 * (poses[2, :, 3] + poses[9, :, 3])          # between two training cameras
    q.append(mid)
    q.append(torch.randn(3, 4) * 50)                             # far outside
    queries = torch.stack(q)
    out = {"poses": poses, "weight": weight, "query_poses": queries}
    with torch.no_grad():
        out["nearest"] = torch.stack([fe(p, mode="nearest") for p in queries])   # (Q, 1, E)
        out["mean"] = torch.stack([fe(p, mode="mean") for p in queries])
        out["index_int"] = np.array(3)
        out["index_int_out"] = fe(3, mode="index")
        out["index_1d"] = torch.tensor([0, 5, 11, 5])
        out["index_1d_out"] = fe(out["index_1d"], mode="index")
        out["index_2d"] = torch.tensor([[1, 2], [3, 4], [11, 0]])
        out["index_2d_out"] = fe(out["index_2d"])                                # the default mode is 'index'
    try:
        fe(queries[0], mode="median")
        raise AssertionError("the reference accepted an unknown mode")
    except ValueError as e:
        out["unknown_mode_error"] = np.array(type(e).__name__)

    # the checkpoint layout: modules registered as train.py does (model, msk_model in __init__, embedding_a in setup)
    sys.modules["tinycudann"] = tcnn_cpu_shim
    ref_mask = _load("ref_implicit_mask", mg.REF + "/models/implicit_mask.py")
    system = torch.nn.Module()
    system.model = torch.nn.Linear(3, 2)
    system.msk_model = ref_mask.implicit_mask()
    system.embedding_a = fe.embedding_a
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "system.ckpt")
        torch.save({"state_dict": system.state_dict()}, path)
        keys = list(torch.load(path, map_location="cpu")["state_dict"])
        # the reference reads its own table back from such a file
        again = ref_utils.FrameEmbedding(E, poses, path)
        assert torch.equal(again.embedding_a.weight, weight)
    out["ckpt_keys"] = np.array(keys)
    mg.npz("g18_frame_embedding.npz", **out)
    print(os.path.getsize(os.path.join(HERE, "g18_frame_embedding.npz")), "bytes")


if __name__ == "__main__":
    main()
