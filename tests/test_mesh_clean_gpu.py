"""Mesh cleaning and vertex colours on the MI355X: ngp_mesh_labels_* / ngp_mesh_face_counts / ngp_mesh_compact_*
through ngp_amd.mesh against the numpy restatement of tests/mesh_clean_reference.py (bit for bit), vertex_colors
against volume_render on the same rays, and the whole route from a trained field to a cleaned, coloured PLY written by
tools/extract_mesh.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clean_reference as ref
from mesh_reference import euler_characteristic, is_closed_oriented, n_components

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.cpu().numpy()


def _check_against_restatement(ngp, verts, faces, criteria, tag):
    """labels, face counts and clean_mesh outputs (verts, faces, normals rows, colour rows) bit-identical to the
    restatement for each (keep_largest, min_faces), and two GPU runs identical -> the rounds the labels needed"""
    n_verts = verts.shape[0]
    g = torch.Generator(device=DEV).manual_seed(n_verts)
    nrm = torch.randn(n_verts, 3, device=DEV, generator=g)
    cols = torch.randint(0, 256, (n_verts, 3), device=DEV, generator=g, dtype=torch.uint8)
    labels, rounds = ngp.mesh.component_labels(faces, n_verts)
    lab, counts = ngp.mesh.mesh_components(faces, n_verts)
    want_lab = ref.labels(_np(faces), n_verts)
    assert np.array_equal(_np(labels), want_lab) and np.array_equal(_np(lab), want_lab)
    assert np.array_equal(_np(counts), ref.face_counts(_np(faces), want_lab))
    assert rounds <= ngp.mesh.label_round_bound(n_verts)
    print(f"[mesh clean] {tag}: V {n_verts} F {faces.shape[0]} components {int((counts > 0).sum())} rounds {rounds}")
    for k, m in criteria:
        got = ngp.mesh.clean_mesh(verts, faces, normals=nrm, colors=cols, keep_largest=k, min_faces=m)
        want, _, _ = ref.clean(_np(verts), _np(faces), (_np(nrm), _np(cols)), k, m)
        for a, b in zip(got, want):
            assert a.dtype == torch.from_numpy(b).dtype and np.array_equal(_np(a).view(np.uint8), b.view(np.uint8)), \
                (tag, k, m)
        again = ngp.mesh.clean_mesh(verts, faces, normals=nrm, colors=cols, keep_largest=k, min_faces=m)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    return rounds


def _blobby_volume(shape, seed, coarse=5):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(1, 1, *[max(2, s // coarse) for s in shape], generator=g)
    return torch.nn.functional.interpolate(c, size=shape, mode="trilinear", align_corners=True)[0, 0].contiguous()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape,level", [((64, 64, 64), 0.9), ((97, 41, 130), 1.2), ((40, 200, 33), 0.5)])
def test_marching_cubes_meshes_match_restatement(ngp, shape, level):
    vol = _blobby_volume(shape, sum(shape)).to(DEV)
    verts, faces = ngp.mesh.marching_cubes(vol, level)
    assert faces.shape[0] > 1000
    assert n_components(_np(faces), verts.shape[0]) > 3
    _check_against_restatement(ngp, verts, faces, [(None, None), (1, None), (3, None), (None, 40), (2, 100)],
                               f"mc {shape}")


@pytest.mark.timeout(300)
def test_sphere_with_floaters_keeps_exactly_the_sphere(ngp):
    n = 96
    ax = torch.linspace(-1, 1, n, device=DEV)
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    h = 2 / (n - 1)
    sphere = 0.45 - x.norm(dim=-1)
    blobs = torch.full_like(sphere, -10.0)
    g = np.random.default_rng(5)
    for _ in range(12):   # small blobs in the corners, far from the sphere
        c = torch.tensor(np.sign(g.standard_normal(3)) * g.uniform(0.7, 0.85, 3), dtype=torch.float32, device=DEV)
        blobs = torch.maximum(blobs, g.uniform(0.03, 0.08) - (x - c).norm(dim=-1))
    vol = torch.maximum(sphere, blobs).contiguous()
    verts, faces = ngp.mesh.marching_cubes(vol, 0.0, (h, h, h), (-1, -1, -1))
    sv, sf = ngp.mesh.marching_cubes(sphere.contiguous(), 0.0, (h, h, h), (-1, -1, -1))
    assert n_components(_np(faces), verts.shape[0]) > 3
    stats = {}
    cv, cf = ngp.mesh.clean_mesh(verts, faces, keep_largest=1, stats=stats)
    assert torch.equal(cf, sf) and np.array_equal(_np(cv).view(np.int32), _np(sv).view(np.int32))
    f = _np(cf)
    assert is_closed_oriented(f, cv.shape[0]) and euler_characteristic(f, cv.shape[0]) == 2
    assert stats["components_kept"] == 1 and stats["F_removed"] == faces.shape[0] - sf.shape[0] > 0
    _check_against_restatement(ngp, verts, faces, [(1, None), (None, 50)], "sphere + blobs")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", range(3))
def test_random_face_lists_match_restatement(ngp, seed):
    g = np.random.default_rng(50 + seed)
    n_verts = [60_000, 200_000, 5_000][seed]
    n_faces = [20_000, 90_000, 6_000][seed]
    faces = ref.random_faces(g, n_verts, n_faces, n_isolated=n_verts // 10, degenerate=0.15)
    verts = torch.from_numpy(g.standard_normal((n_verts, 3)).astype(np.float32)).to(DEV)
    _check_against_restatement(ngp, verts, torch.from_numpy(faces).to(DEV),
                               [(None, None), (1, None), (10, 2), (None, 3)], f"random {seed}")


SCAN_TILE = 1024 * 256    # items whose workgroup sums fill one tile of the 1024-thread scan (256-thread workgroups)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_verts,n_faces", [(SCAN_TILE + 1, 20_000), (60_000, SCAN_TILE + 1)], ids=["verts", "faces"])
def test_second_tile_of_the_workgroup_sums(ngp, n_verts, n_faces):
    """one vertex, or one face, more than 1024 workgroups cover: its offset is the first entry of the scan's second tile
    and is made of the first tile's carry alone.  The last vertex is put into the component with the most faces (it
    trades places with that component's largest vertex: no label changes) and the last face is one of that component's,
    so both criteria keep them."""
    criteria = [(None, None), (1, None)]
    g = np.random.default_rng(60 + n_verts % 7)
    faces = ref.random_faces(g, n_verts, n_faces, n_isolated=n_verts // 10, degenerate=0.15)
    lab = ref.labels(faces, n_verts)
    big = np.argmax(ref.face_counts(faces, lab))                   # label of the component with the most faces
    of_big = np.nonzero(lab[faces[:, 0]] == big)[0]
    faces[[of_big[-1], n_faces - 1]] = faces[[n_faces - 1, of_big[-1]]]
    w, last = faces[lab[faces[:, 0]] == big].max(), n_verts - 1
    swap = np.arange(n_verts, dtype=np.int32)
    swap[[w, last]] = last, w
    faces = swap[faces]
    lab = ref.labels(faces, n_verts)
    counts = ref.face_counts(faces, lab)
    for k, m in criteria:
        kept = ref.select(counts, k, m)[lab[faces[:, 0]]] != 0
        assert (faces[kept] >= SCAN_TILE).any() if n_verts > SCAN_TILE else kept[SCAN_TILE:].any(), (k, m)
    verts = torch.from_numpy(g.standard_normal((n_verts, 3)).astype(np.float32)).to(DEV)
    _check_against_restatement(ngp, verts, torch.from_numpy(faces).to(DEV), criteria, f"second tile V {n_verts} F {n_faces}")


@pytest.mark.timeout(300)
def test_long_chain_stays_within_the_round_bound(ngp):
    """faces (i, i+1, i+2) over 10^5 vertices: one component whose label has to travel the whole chain"""
    n = 100_000
    g = np.random.default_rng(9)
    i = np.arange(n - 2)
    chain = np.stack([i, i + 1, i + 2], 1)
    verts = torch.from_numpy(g.standard_normal((n, 3)).astype(np.float32)).to(DEV)
    for tag, f in (("chain", chain), ("chain reversed", chain[::-1]), ("chain shuffled", chain[g.permutation(n - 2)]),
                   ("chain relabelled", g.permutation(n)[chain])):
        faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV)
        _check_against_restatement(ngp, verts, faces, [(1, None)], tag)
    with pytest.raises(RuntimeError, match="did not settle"):
        ngp.mesh.component_labels(torch.from_numpy(chain.astype(np.int32)).to(DEV), n, max_rounds=2)


@pytest.mark.timeout(120)
def test_empty_single_face_and_bad_indices(ngp):
    verts = torch.randn(4, 3, device=DEV)
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    lab, cnt = ngp.mesh.mesh_components(none, 4)
    assert np.array_equal(_np(lab), np.arange(4)) and not cnt.any()
    v, f = ngp.mesh.clean_mesh(verts, none)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = ngp.mesh.clean_mesh(torch.zeros(0, 3, device=DEV), none, keep_largest=1)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    one = torch.tensor([[3, 1, 2]], dtype=torch.int32, device=DEV)
    nrm = torch.randn(4, 3, device=DEV)
    lab, cnt = ngp.mesh.mesh_components(one, 4)
    assert _np(lab).tolist() == [0, 1, 1, 1] and _np(cnt).tolist() == [0, 1, 0, 0]
    v, f, n = ngp.mesh.clean_mesh(verts, one, normals=nrm, keep_largest=1)
    assert torch.equal(v, verts[1:]) and torch.equal(n, nrm[1:]) and _np(f).tolist() == [[2, 0, 1]]
    _check_against_restatement(ngp, verts, one, [(None, None), (1, 2)], "single face")
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="outside"):
            ngp.mesh.clean_mesh(verts, torch.tensor(bad, dtype=torch.int32, device=DEV))


# --------------------------------------------------------------------------------------- end to end on a trained field
@pytest.fixture(scope="module")
def trained(ngp):
    """the lego proxy trained for 300 steps of 4096 rays (the fixture of test_mesh_gpu.py)"""
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


def _near(verts, r):
    """per vertex: synthetic.analytic_sigma is not constant over the vertex and its 26 neighbours at +-r"""
    from ngp_amd.synthetic import analytic_sigma
    off = torch.stack(torch.meshgrid(*[torch.tensor([-1.0, 0.0, 1.0], device=DEV)] * 3, indexing="ij"), -1).reshape(-1, 3)
    s = analytic_sigma(verts[:, None, :] + r * off[None])
    return s.amax(1) != s.amin(1)


@pytest.mark.timeout(900)
def test_vertex_colors_equal_volume_render_on_the_same_rays(ngp, trained):
    from ngp_amd.mesh import FALLBACK_DIR, MIN_OPACITY, vertex_colors, vertex_rays
    from ngp_amd.rendering import volume_render
    verts, faces, nrm = ngp.mesh.extract_mesh(trained, resolution=96, level=10.0, normals=True)
    off = 2 / 95
    col = vertex_colors(trained, verts, nrm, off, quantize=False)
    q = vertex_colors(trained, verts, nrm, off)
    assert q.dtype == torch.uint8 and torch.equal(q, torch.floor(255 * col + 0.5).to(torch.uint8))
    rows = torch.nonzero(nrm.abs().amax(1) > 0).squeeze(1)
    rays_o, rays_d, hits_t = vertex_rays(verts[rows], nrm[rows], off)
    assert torch.equal(hits_t[:, 0], torch.zeros_like(hits_t[:, 0])) and (hits_t[:, 1] == np.float32(2 * off)).all()
    m = rows.numel()
    opacity, rgb = torch.zeros(m, device=DEV), torch.zeros(m, 3, device=DEV)
    volume_render(trained, rays_o, rays_d, hits_t, opacity, torch.zeros(m, device=DEV), rgb,
                  torch.zeros(m, 3, device=DEV), torch.zeros(m, 3, device=DEV), torch.zeros(m, 7, device=DEV))
    ok = opacity >= MIN_OPACITY
    want = (rgb / opacity[:, None]).clamp(0, 1)
    assert torch.equal(col[rows[ok]], want[ok])
    seen = torch.zeros(verts.shape[0], dtype=torch.bool, device=DEV)
    seen[rows[ok]] = True
    rest = torch.nonzero(~seen).squeeze(1)
    d = torch.tensor(FALLBACK_DIR, device=DEV).expand(rest.numel(), 3).contiguous()
    fb = trained.forward_test(verts[rest].contiguous(), d)[1].float().clamp(0, 1)
    assert torch.equal(col[rest], fb)
    print(f"[mesh colors] V {verts.shape[0]}: rays that see the surface {ok.float().mean().item():.4f}")
    assert ok.float().mean().item() > 0.8


@pytest.mark.timeout(900)
def test_trained_field_floaters_and_colours(ngp, trained, tmp_path):
    """extract_mesh(resolution=160, level=10) on the trained proxy with and without keep_largest=1 and colours;
    the tool writes the same cleaned, coloured mesh as a PLY.  Measured once on the MI355X: keep_largest=1 keeps 1 of
    1201 components (V 155023 -> 143624) and raises the share of vertices within 3 voxels of the analytic surface from
    0.605 to 0.635; the mean colour error of the vertices within 1 voxel is 0.077.  The thresholds keep a margin."""
    h = 1.0 / 159
    v0, f0 = ngp.mesh.extract_mesh(trained, resolution=160, level=10.0)
    verts, faces, nrm, rgb = ngp.mesh.extract_mesh(trained, resolution=160, level=10.0, normals=True, keep_largest=1,
                                                   colors=True)
    torch.cuda.synchronize()
    stats = {}
    cv, cf = ngp.mesh.clean_mesh(v0, f0, keep_largest=1, stats=stats)
    assert torch.equal(cv, verts) and torch.equal(cf, faces)
    near0 = _near(v0, 3 * h).float().mean().item()
    near1 = _near(verts, 3 * h).float().mean().item()
    from ngp_amd.synthetic import analytic_rgb
    close = _near(verts, h)
    err = (rgb.float() / 255 - analytic_rgb(verts)).abs()[close].mean().item()
    print(f"[mesh clean e2e] V {v0.shape[0]} -> {verts.shape[0]}, F {f0.shape[0]} -> {faces.shape[0]}, {stats}, "
          f"within 3 voxels {near0:.4f} -> {near1:.4f}, colour error within 1 voxel {err:.4f} "
          f"({int(close.sum())} vertices)")
    assert near1 > near0 + 0.01
    assert err < 0.12

    from ngp_amd import ckpt
    from ngp_amd.mesh import read_ply
    ck = tmp_path / "proxy.ckpt"
    ckpt.save_ckpt(trained, str(ck))
    out = tmp_path / "mesh.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--ckpt", str(ck),
                        "--scale", "0.5", "--out", str(out), "--resolution", "160", "--level", "10",
                        "--keep_largest", "1", "--colors"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("[mesh clean e2e] tool:", line)
    assert line["components"] == stats["components"] and line["V_removed"] == stats["V_removed"]
    assert line["F_removed"] == stats["F_removed"]
    pv, pf, pn, pc = read_ply(str(out), colors=True)
    assert pn is None
    assert np.array_equal(pv, _np(verts)) and np.array_equal(pf, _np(faces)) and np.array_equal(pc, _np(rgb))


@pytest.mark.timeout(900)
def test_tool_timings_at_the_reference_lattice(ngp, trained, tmp_path):
    """the reference's call (512 x 128 x 512) with --keep_largest 1 --colors: cleaning is small beside the density
    pass"""
    from ngp_amd import ckpt
    ck = tmp_path / "proxy.ckpt"
    ckpt.save_ckpt(trained, str(ck))
    out = tmp_path / "mesh.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--ckpt", str(ck),
                        "--scale", "0.5", "--out", str(out), "--bbox", "-1", "-0.3", "-1", "1", "0.15", "1",
                        "--resolution", "512", "128", "512", "--level", "10", "--reference_spacing",
                        "--keep_largest", "1", "--colors"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("[mesh clean 512x128x512] tool:", line)
    V = line["V"] + line["V_removed"]
    print(f"[mesh clean 512x128x512] removed {line['V_removed'] / V:.4f} of the vertices, "
          f"{line['F_removed'] / (line['F'] + line['F_removed']):.4f} of the faces")
    assert line["V"] > 10_000 and line["components"] >= 1
    assert line["clean_ms"] < 1000     # a fresh process: includes loading the kernels on first use
    # warm, in this process, on the same uncleaned mesh
    import time
    v, f = ngp.mesh.extract_mesh(trained, xyz_min=(-1, -0.3, -1), xyz_max=(1, 0.15, 1), resolution=(512, 128, 512),
                                 level=10.0, reference_spacing=True)
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = {}
        cv, cf = ngp.mesh.clean_mesh(v, f, keep_largest=1, stats=stats)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    print(f"[mesh clean 512x128x512] clean_mesh warm: V {v.shape[0]} F {f.shape[0]} {stats} "
          f"ms {[round(x, 3) for x in ms]}")
    assert cv.shape[0] == line["V"] and cf.shape[0] == line["F"]
    assert min(ms) < 20
