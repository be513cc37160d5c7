"""Pose refinement without a GPU: the float64 restatements of tests/pose_reference.py against the package's own
get_rays / axisangle_to_R and the oracle's SH forward (before any GPU test uses them), the C ABI of the three new entries,
PoseRefiner's state and checkpoint keys, and the tool's new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_reference as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_get_rays_at_zero_and_axisangle_to_R(ngp):
    from ngp_amd.datasets.ray_utils import axisangle_to_R, get_rays
    poses, dR, dT, directions = pr.make_cameras(7, 1)
    g = np.random.default_rng(2)
    img = torch.from_numpy(g.integers(0, 7, 200))
    pix = torch.from_numpy(g.integers(0, len(directions), 200))
    for dtype, tol in ((torch.float64, 1e-15), (torch.float32, 1e-6)):
        P, D = torch.from_numpy(poses).to(dtype), torch.from_numpy(directions).to(dtype)
        zero = torch.zeros(7, 3, dtype=dtype)
        o, d = pr.pose_rays(P, zero, zero, D, img, pix)
        o_ref, d_ref = get_rays(D[pix], P[img])
        assert torch.equal(o, o_ref)
        np.testing.assert_allclose(d.numpy(), d_ref.numpy(), rtol=0, atol=tol * 4)
        v = torch.from_numpy(dR).to(dtype)
        np.testing.assert_allclose(pr.rodrigues(v).numpy(), axisangle_to_R(v).numpy(), rtol=0, atol=tol)
    # the refined pose of the reference's training step (train.py:143-149), spelled out
    P, v, t = torch.from_numpy(poses).double(), torch.from_numpy(dR).double(), torch.from_numpy(dT).double()
    o, d = pr.pose_rays(P, v, t, torch.from_numpy(directions).double(), img, pix)
    refined = torch.cat([axisangle_to_R(v) @ P[..., :3], (P[..., 3] + t)[..., None]], -1)
    o_ref, d_ref = get_rays(torch.from_numpy(directions).double()[pix], refined[img])
    np.testing.assert_allclose(o.numpy(), o_ref.numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(d.numpy(), d_ref.numpy(), rtol=0, atol=1e-14)


def test_out_of_range_rays_of_the_restatement_are_zero():
    poses, dR, dT, directions = (torch.from_numpy(a).double() for a in pr.make_cameras(3, 3))
    img, pix = torch.tensor([0, 3, -1, 2, 1]), torch.tensor([5, 5, 5, 144, -2])
    o, d = pr.pose_rays(poses, dR, dT, directions, img, pix)
    assert (o[1:] == 0).all() and (d[1:] == 0).all() and d[0].abs().sum() > 0


def test_direction_encoding_equals_the_oracle_sh_forward():
    import oracle
    g = np.random.default_rng(4)
    d = g.standard_normal((500, 3)) * np.exp(g.uniform(np.log(1e-3), np.log(1e3), (500, 1)))
    d[:3] = np.eye(3)
    d[3:6] = -np.eye(3)
    want = pr.dir_encoding(torch.from_numpy(d)).numpy()
    dn = d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    got = oracle.sh_fwd(np.ascontiguousarray(((dn + 1) / 2).astype(np.float32)), 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    assert got.shape == (500, 16)
    # under the clamp: d / 1e-6, and the zero vector encodes the basis at the origin
    tiny = torch.tensor([[0.0, 0.0, 0.0], [3e-7, 0.0, 0.0]], dtype=torch.float64)
    enc = pr.dir_encoding(tiny).numpy()
    np.testing.assert_allclose(enc[0, :4], [0.28209479177387814, 0, 0, 0], atol=1e-15)
    np.testing.assert_allclose(enc[1, 3], -0.48860251190291987 * 0.3, atol=1e-12)


def test_new_entries_in_the_c_abi(ngp):
    import ctypes as C
    protos = ngp._lib.PROTOS
    for name, sizes in (("ngp_pose_rays_fwd", {"n_rays"}), ("ngp_pose_rays_bwd", {"n_rays", "n"}), ("ngp_sh_bwd_dirs", {"n"})):
        assert name in protos
        args = protos[name][1]
        names = [a for _, a in args]
        assert names[-1] == "stream" and sizes <= set(names)
        lib = ngp._lib.load()
        for size, want in ((-1, -22), (0, 0)):
            vals = [size if a in ("n", "n_rays") else (None if t is C.c_void_p else 0) for t, a in args]
            assert getattr(lib, name)(*vals) == want, (name, size)


def test_pose_refiner_state_and_checkpoint_keys(ngp, tmp_path):
    from ngp_amd import ckpt
    from ngp_amd.datasets.ray_utils import axisangle_to_R
    from ngp_amd.pose import PoseRefiner, perturb_poses, pose_errors
    poses, dR, dT, directions = (torch.from_numpy(a) for a in pr.make_cameras(5, 6))
    ref = PoseRefiner(poses, directions)
    assert list(ref.state_dict()) == ["dR", "dT", "poses"]
    assert [n for n, _ in ref.named_parameters()] == ["dR", "dT"]
    assert not ref.dR.any() and not ref.dT.any() and tuple(ref.dR.shape) == tuple(ref.dT.shape) == (5, 3)
    assert torch.equal(ref.refined_poses()[..., 3], poses[..., 3])
    np.testing.assert_allclose(ref.refined_poses().detach().numpy(), poses.numpy(), rtol=0, atol=1e-7)
    with torch.no_grad():
        ref.dR.copy_(dR)
        ref.dT.copy_(dT)
    want = torch.cat([axisangle_to_R(dR) @ poses[..., :3], (poses[..., 3] + dT)[..., None]], -1)
    assert torch.equal(ref.refined_poses().detach(), want)
    # checkpoint: top-level keys, the model's tools do not see them, the loader restores them bit for bit
    model = torch.nn.Linear(2, 2)
    path = str(tmp_path / "p.ckpt")
    ckpt.save_ckpt(model, path, pose_refiner=ref)
    sd = torch.load(path, weights_only=True)["state_dict"]
    assert {"dR", "dT", "poses", "model.weight", "model.bias"} == set(sd)
    assert set(ckpt.extract_model_state_dict(path)) == {"weight", "bias"}
    assert set(ckpt.slim_ckpt(path, save_poses=True)) >= {"dR", "dT", "poses"} and "poses" not in ckpt.slim_ckpt(path)
    other = PoseRefiner(torch.zeros(5, 3, 4), directions)
    ckpt.load_poses(other, path)
    for k in ("dR", "dT", "poses"):
        assert torch.equal(other.state_dict()[k], ref.state_dict()[k]), k
    with pytest.raises(RuntimeError, match="size mismatch"):
        ckpt.load_poses(PoseRefiner(torch.zeros(4, 3, 4), directions), path)
    ckpt.save_ckpt(model, path)
    with pytest.raises(KeyError, match="pose keys"):
        ckpt.load_poses(other, path)
    # the perturbation is seeded and of the size asked for
    a, b, c = perturb_poses(poses, 0.02, 0.5, seed=3), perturb_poses(poses, 0.02, 0.5, seed=3), perturb_poses(poses, 0.02, 0.5, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    t_err, r_err = pose_errors(a, poses)
    assert 0.01 < t_err < 0.08 and abs(r_err - 0.5) < 1e-2
    assert pose_errors(poses, poses)[0] == 0.0


def test_tool_has_the_new_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_dataset.py"), "--help"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--optimize_ext", "--pose_lr", "--perturb_poses"):
        assert flag in out.stdout, flag
