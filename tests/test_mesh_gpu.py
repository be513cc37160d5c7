"""Mesh export on the MI355X: ngp_mc_count / ngp_mc_emit through ngp_amd.mesh against analytic surfaces and the CPU
restatement of tests/mesh_reference.py (bit for bit), awkward inputs, the reference's lattice size, and the whole
route from a trained field to a PLY file written by tools/extract_mesh.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mesh_reference import (euler_characteristic, face_normals, is_closed_oriented, marching_cubes, mc_counts,
                            mc_tables, n_components, signed_volume)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(ngp):
    return mc_tables(ngp)


def _lattice(n, lo=-1.0, hi=1.0):
    ax = torch.linspace(lo, hi, n, device=DEV)
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1), (hi - lo) / (n - 1)


def _gpu_mc(ngp, vol, level, spacing=(1, 1, 1), origin=(0, 0, 0)):
    v, f = ngp.mesh.marching_cubes(vol.contiguous(), level, spacing, origin)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def _check_closed(v, f):
    assert len(f) and f.min() >= 0 and f.max() < len(v)
    assert np.unique(f).size == len(v)
    assert is_closed_oriented(f, len(v))


def test_sphere(ngp, tables):
    """sigma = r0 - |x| on 96^3 over [-1,1]^3: one closed sphere (chi = 2), volume within 1 %, every vertex within one
    cell of the radius, every face normal pointing out"""
    x, h = _lattice(96)
    r0 = 0.6
    vol = r0 - x.norm(dim=-1)
    v, f = _gpu_mc(ngp, vol, 0.0, (h, h, h), (-1, -1, -1))
    _check_closed(v, f)
    assert euler_characteristic(f, len(v)) == 2 and n_components(f, len(v)) == 1
    assert abs(signed_volume(v, f) / (4 / 3 * np.pi * r0 ** 3) - 1) < 0.01
    assert np.abs(np.linalg.norm(v, axis=1) - r0).max() < h
    centroid = v[f].mean(1)
    assert ((face_normals(v, f) * centroid).sum(1) > 0).all()
    rv, rf = marching_cubes(vol.cpu().numpy(), 0.0, tables, (h, h, h), (-1, -1, -1))
    assert np.array_equal(f, rf) and np.array_equal(v.view(np.int32), rv.view(np.int32))


def test_torus_and_two_spheres(ngp):
    x, h = _lattice(96)
    q = torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - 0.55
    torus = 0.2 - torch.sqrt(q ** 2 + x[..., 2] ** 2)
    v, f = _gpu_mc(ngp, torus, 0.0, (h, h, h), (-1, -1, -1))
    _check_closed(v, f)
    assert euler_characteristic(f, len(v)) == 0 and n_components(f, len(v)) == 1
    c = torch.tensor([0.45, 0.0, 0.0], device=DEV)
    two = torch.maximum(0.3 - (x - c).norm(dim=-1), 0.3 - (x + c).norm(dim=-1))
    v, f = _gpu_mc(ngp, two, 0.0, (h, h, h), (-1, -1, -1))
    _check_closed(v, f)
    assert euler_characteristic(f, len(v)) == 4 and n_components(f, len(v)) == 2
    assert signed_volume(v, f) > 0


def _smooth_volume(shape, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(1, 1, *[max(2, s // 6) for s in shape], generator=g)
    return torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=True)[0, 0].contiguous()


# (65, 64, 64): 266 240 points are 1040 workgroups, more sums than the 1024 threads that scan them take in one tile
@pytest.mark.parametrize("shape", [(37, 64, 19), (130, 9, 71), (2, 2, 2), (65, 3, 300), (65, 64, 64)])
def test_matches_cpu_restatement_bit_for_bit(ngp, tables, shape):
    """seeded smooth random volumes of odd shapes (surfaces open at the border): faces identical to the restatement,
    vertices bit-identical, and two GPU runs bit-identical"""
    for seed, level in ((1, 0.0), (2, 0.25)):
        vol = _smooth_volume(shape, seed)
        spacing, origin = (0.5, 0.25, 1.5), (-3.0, 0.125, 7.0)
        v, f = _gpu_mc(ngp, vol.to(DEV), level, spacing, origin)
        rv, rf = marching_cubes(vol.numpy(), level, tables, spacing, origin)
        assert (len(v), len(f)) == mc_counts(vol.numpy(), level, tables)
        assert np.array_equal(f, rf)
        assert np.array_equal(v.view(np.int32), rv.view(np.int32))
        v2, f2 = _gpu_mc(ngp, vol.to(DEV), level, spacing, origin)
        assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)


def test_awkward_inputs(ngp, tables):
    """exact level values, NaN and +-inf: only finite vertices inside the box, no index out of range, and still the
    restatement's output bit for bit"""
    g = np.random.default_rng(7)
    shape = (23, 17, 29)
    vol = (g.random(shape) * 20).astype(np.float32)
    sel = g.random(shape)
    vol[sel < 0.1] = 10.0
    vol[(sel >= 0.1) & (sel < 0.15)] = np.nan
    vol[(sel >= 0.15) & (sel < 0.2)] = np.inf
    vol[(sel >= 0.2) & (sel < 0.25)] = -np.inf
    spacing, origin = (0.1, 0.2, 0.3), (1.0, -2.0, 0.5)
    v, f = _gpu_mc(ngp, torch.from_numpy(vol).to(DEV), 10.0, spacing, origin)
    assert len(v) > 1000 and np.isfinite(v).all()
    hi = np.array(origin, np.float32) + (np.array(shape) - 1) * np.array(spacing, np.float32)
    assert (v >= np.array(origin, np.float32)).all() and (v <= hi + 1e-5).all()
    assert f.min() >= 0 and f.max() < len(v)
    rv, rf = marching_cubes(vol, 10.0, tables, spacing, origin)
    assert np.array_equal(f, rf) and np.array_equal(v.view(np.int32), rv.view(np.int32))
    # the empty cases: a flat lattice, and a volume without a crossing
    v, f = _gpu_mc(ngp, torch.zeros(1, 5, 5, device=DEV), 0.5)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = _gpu_mc(ngp, torch.zeros(4, 5, 6, device=DEV), 0.5)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_reference_size_counts(ngp, tables):
    """512 x 128 x 512 (33.5 M points, the reference's lattice): the counts of the multi-workgroup scan equal the
    restatement's"""
    n = (512, 128, 512)
    axes = [torch.linspace(-1, 1, m, device=DEV) for m in n]
    vol = (torch.sin(7 * axes[0])[:, None, None] * torch.cos(11 * axes[1])[None, :, None]
           + torch.sin(5 * axes[2] + 1)[None, None, :] * 0.7).contiguous()
    v, f = ngp.mesh.marching_cubes(vol, 0.1)
    torch.cuda.synchronize()
    assert (v.shape[0], f.shape[0]) == mc_counts(vol.cpu().numpy(), 0.1, tables)
    assert v.shape[0] > 1_000_000 and int(f.min()) >= 0 and int(f.max()) < v.shape[0]


# --------------------------------------------------------------------------------------- end to end on a trained field
@pytest.fixture(scope="module")
def trained(ngp):
    """the lego proxy trained for 300 steps of 4096 rays"""
    from ngp_amd.synthetic import LegoProxy
    from ngp_amd.trainer import NGPTrainer
    torch.manual_seed(3)
    model = ngp.networks.NGP(scale=0.5).to(DEV)
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=DEV))
    coords = torch.stack(torch.meshgrid(*[torch.arange(G, dtype=torch.int32, device=DEV)] * 3, indexing="ij"), -1)
    model.register_buffer("grid_coords", coords.reshape(-1, 3).contiguous())
    scene = LegoProxy(n_images=40, img_wh=(200, 200), device=DEV)
    tr = NGPTrainer(model, lr=1e-2)
    gen = torch.Generator(device=DEV).manual_seed(4)
    for _ in range(300):
        img, pix = scene.sample_batch(4096, generator=gen)
        o, d = scene.rays(img, pix)
        gt, _ = scene.ground_truth(o, d, n_quad=128)
        tr.step(o, d, gt)
    tr.wait()
    torch.cuda.synchronize()
    return model


def test_reference_spacing_relates_vertex_for_vertex(ngp, trained):
    """extract_mesh at 512 x 128 x 512 (chunked density): reference_spacing=True is the default mesh shrunk by
    (n-1)/n toward the lattice's low corner"""
    n = (512, 128, 512)
    v, f = ngp.mesh.extract_mesh(trained, resolution=n, level=10.0)
    rv, rf = ngp.mesh.extract_mesh(trained, resolution=n, level=10.0, reference_spacing=True)
    assert v.shape[0] > 10_000 and torch.equal(f, rf)
    lo = trained.xyz_min.reshape(1, 3).double()
    k = torch.tensor([(m - 1) / m for m in n], device=DEV, dtype=torch.float64)
    want = (v.double() - lo) * k + lo
    assert (rv.double() - want).abs().max().item() < 1e-6


def _near_fraction(verts, r):
    """share of vertices where synthetic.analytic_sigma is not constant over the vertex and its 26 neighbours at +-r"""
    from ngp_amd.synthetic import analytic_sigma
    off = torch.stack(torch.meshgrid(*[torch.tensor([-1.0, 0.0, 1.0], device=DEV)] * 3, indexing="ij"), -1).reshape(-1, 3)
    s = analytic_sigma(verts[:, None, :] + r * off[None])
    return (s.amax(1) != s.amin(1)).float().mean().item()


def test_trained_field_mesh_normals_and_ply(ngp, trained, tmp_path):
    """extract_mesh(resolution=160, level=10, normals=True) on the trained proxy.  Measured once on the MI355X
    (V 155027, F 308958): 37 / 51 / 61 / 67 % of the vertices are within 1 / 2 / 3 / 4 voxel widths of the analytic
    surface (the rest lie on what 300 steps leave of floaters and soft edges), the field's normals agree with the
    area-weighted face normals at a mean cosine of 0.71 (median 0.87), and they are unit length to 2e-7.  The
    thresholds keep a margin below those.  The PLY written by tools/extract_mesh.py in a child process reads back
    equal."""
    verts, faces, nrm = ngp.mesh.extract_mesh(trained, resolution=160, level=10.0, normals=True)
    torch.cuda.synchronize()
    assert verts.shape[0] > 5_000 and faces.shape[0] > 10_000
    h = 1.0 / 159
    near = {k: _near_fraction(verts, k * h) for k in (1, 2, 3, 4)}
    # area-weighted face normals gathered at the vertices vs the field's own normals
    v64 = verts.double()
    fn = torch.cross(v64[faces[:, 1].long()] - v64[faces[:, 0].long()], v64[faces[:, 2].long()] - v64[faces[:, 0].long()],
                     dim=-1)
    acc = torch.zeros_like(v64)
    for c in range(3):
        acc.index_add_(0, faces[:, c].long(), fn)
    acc = torch.nn.functional.normalize(acc, dim=-1)
    cos = (acc * nrm.double()).sum(-1)
    print(f"[mesh e2e] V {verts.shape[0]} F {faces.shape[0]} near {near} cos mean {cos.mean().item():.4f} "
          f"cos median {cos.median().item():.4f} unit {(nrm.norm(dim=-1) - 1).abs().max().item():.2e}")
    assert near[3] > 0.45
    assert cos.mean().item() > 0.55 and cos.median().item() > 0.7
    assert ((nrm.norm(dim=-1) - 1).abs() < 1e-4).float().mean().item() > 0.99

    from ngp_amd import ckpt
    from ngp_amd.mesh import read_ply
    ck = tmp_path / "proxy.ckpt"
    ckpt.save_ckpt(trained, str(ck))
    out = tmp_path / "mesh.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--ckpt", str(ck),
                        "--scale", "0.5", "--out", str(out), "--resolution", "160", "--level", "10", "--normals"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    print("[mesh e2e] tool:", line)
    pv, pf, pn = read_ply(str(out))
    assert np.array_equal(pv, verts.cpu().numpy()) and np.array_equal(pf, faces.cpu().numpy())
    assert np.allclose(pn, nrm.cpu().numpy(), atol=1e-6)
