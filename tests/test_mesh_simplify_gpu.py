"""Mesh simplification on the MI355X: ngp_mesh_simplify_* through ngp_amd.mesh.simplify_mesh against the numpy
restatement of tests/mesh_simplify_reference.py (topology, counts and colours bit for bit, positions and normals to two
float32 ulp), run-to-run identity, the edges, the displacement bound, the wedge that motivates quadric placement, the
target_faces search, and the route from a trained field to a simplified, coloured PLY written by
tools/extract_mesh.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_simplify_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("cell", "clusters", "V_in", "V_out", "F_in", "F_out", "degenerate", "duplicate")


def _np(t):
    return t.cpu().numpy()


def _attributes(n_verts):
    g = torch.Generator(device=DEV).manual_seed(n_verts)
    nrm = torch.nn.functional.normalize(torch.randn(n_verts, 3, device=DEV, generator=g), dim=-1).contiguous()
    cols = torch.randint(0, 256, (n_verts, 3), device=DEV, generator=g, dtype=torch.uint8)
    return nrm, cols


def _check_against_restatement(ngp, verts, faces, cell, origin, tag):
    """both placements: faces, counts and colours bit-identical to the restatement, positions within 2^-22 of the
    largest coordinate and unit normals within 2^-22 (both sides sum in double in the same order; what is left is the
    final rounding to float32 and rare double rounding), and a second GPU run identical -> the restatement's output
    of the last placement"""
    nrm, cols = _attributes(verts.shape[0])
    for placement in ("mean", "quadric"):
        stats = {}
        got = ngp.mesh.simplify_mesh(verts, faces, cell=cell, origin=origin, placement=placement, normals=nrm,
                                     colors=cols, stats=stats)
        want = ref.simplify(_np(verts), _np(faces), cell=cell, origin=origin, placement=placement, normals=_np(nrm),
                            colors=_np(cols))
        v, f, n, c = got
        assert (v.dtype, f.dtype, n.dtype, c.dtype) == (torch.float32, torch.int32, torch.float32, torch.uint8)
        assert {k: stats[k] for k in COUNTS} == {k: want["stats"][k] for k in COUNTS}, (tag, placement)
        assert np.array_equal(_np(f), want["faces"]) and np.array_equal(_np(c), want["colors"]), (tag, placement)
        scale = float(verts.abs().max()) if verts.numel() else 1.0
        dv = np.abs(_np(v).astype(np.float64) - want["verts"]).max() if len(want["verts"]) else 0.0
        dn = np.abs(_np(n).astype(np.float64) - want["normals"]).max() if len(want["verts"]) else 0.0
        print(f"[mesh simplify] {tag} {placement}: V {stats['V_in']} -> {stats['V_out']} F {stats['F_in']} -> "
              f"{stats['F_out']} degenerate {stats['degenerate']} duplicate {stats['duplicate']} "
              f"|dv|/scale {dv / scale:.3g} |dn| {dn:.3g}")
        assert dv <= 2.0 ** -22 * scale, (tag, placement)
        assert dn <= 2.0 ** -22, (tag, placement)
        again = ngp.mesh.simplify_mesh(verts, faces, cell=cell, origin=origin, placement=placement, normals=nrm,
                                       colors=cols)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (tag, placement)
    return want


def _blobby_volume(shape, seed, coarse=5):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(1, 1, *[max(2, s // coarse) for s in shape], generator=g)
    return torch.nn.functional.interpolate(c, size=shape, mode="trilinear", align_corners=True)[0, 0].contiguous()


@pytest.fixture(scope="module")
def mc_meshes(ngp):
    out = {}
    for shape in ((48, 48, 48), (33, 70, 41)):
        out[shape] = ngp.mesh.marching_cubes(_blobby_volume(shape, sum(shape)).to(DEV), 0.5)
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cell,lattice_origin", [(1.7, False), (3.0, False), (6.3, False), (4.0, True)])
@pytest.mark.parametrize("shape", [(48, 48, 48), (33, 70, 41)])
def test_marching_cubes_meshes_match_restatement(ngp, mc_meshes, shape, cell, lattice_origin):
    """spacing h = 1; with the lattice origin and cell 4h many vertices lie exactly on cell faces"""
    verts, faces = mc_meshes[shape]
    assert faces.shape[0] > 1000
    if lattice_origin:
        on_face = (verts == torch.floor(verts / 4) * 4).any(1).sum().item()
        assert on_face > 20
    want = _check_against_restatement(ngp, verts, faces, cell, (0.0, 0.0, 0.0) if lattice_origin else None,
                                      f"mc {shape} cell {cell}")
    assert 0 < want["stats"]["F_out"] < faces.shape[0]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", range(3))
def test_random_soups_match_restatement(ngp, seed):
    v, f = ref.soup(seed)
    cell = float(np.float32((v.max(0) - v.min(0)).max() / 10))
    want = _check_against_restatement(ngp, torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), cell, None,
                                      f"soup {seed}")
    assert want["stats"]["degenerate"] > 0 and want["stats"]["duplicate"] > 0


SCAN_TILE = 1024 * 256    # items whose workgroup sums fill one tile of the 1024-thread scan (256-thread workgroups)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_verts,n_faces", [(SCAN_TILE + 1, 20_000), (60_000, SCAN_TILE + 1)], ids=["verts", "faces"])
def test_second_tile_of_the_workgroup_sums(ngp, n_verts, n_faces):
    """one vertex, or one face, more than 1024 workgroups cover: its offset is the first entry of the scan's second tile
    and is made of the first tile's carry alone.  A thousand cells along the longest side leave most vertices alone in
    their cell: the last vertex is its cluster's representative, the last face is kept."""
    v, f = ref.soup(7, n_verts, n_faces)
    cell = float(np.float32((v.max(0) - v.min(0)).max() / 1000))
    cluster, _ = ref.clusters(ref.cell_keys(v, v.min(0), cell))
    if n_verts > SCAN_TILE:
        assert np.nonzero(cluster == cluster[-1])[0].min() >= SCAN_TILE
    else:
        assert ref.face_pass(f, cluster)[1][SCAN_TILE:].any()
    _check_against_restatement(ngp, torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), cell, None,
                               f"second tile V {n_verts} F {n_faces}")


@pytest.mark.timeout(120)
def test_edges_and_errors(ngp):
    simplify = ngp.mesh.simplify_mesh
    none_v = torch.zeros(0, 3, device=DEV)
    none_f = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    stats = {}
    v, f = simplify(none_v, none_f, cell=1.0, stats=stats)
    assert v.shape == (0, 3) and f.shape == (0, 3) and stats["V_out"] == 0 and stats["F_out"] == 0
    v, f = simplify(torch.randn(5, 3, device=DEV), none_f, cell=0.1)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # one face
    tri = torch.eye(3, device=DEV)
    one = torch.tensor([[2, 0, 1]], dtype=torch.int32, device=DEV)
    nrm, cols = _attributes(3)
    v, f, n, c = simplify(tri, one, cell=0.5, normals=nrm, colors=cols, stats=stats)
    assert torch.equal(f, one) and torch.equal(c, cols)         # each vertex lies on its only plane: it stays
    assert (v - tri).abs().max() <= 2.0 ** -22 and (n - nrm).abs().max() <= 2.0 ** -22
    assert stats["clusters"] == 3 and stats["degenerate"] == 0 and stats["duplicate"] == 0
    _check_against_restatement(ngp, tri, one, 0.5, None, "one face")
    # all vertices in one cell / a cell larger than the bounding box: nothing is left
    sv, sf = ref.soup(11, 60, 90)
    sv, sf = torch.from_numpy(sv).to(DEV), torch.from_numpy(sf).to(DEV)
    for cell, origin in ((64.0, (-32.0, -32.0, -32.0)), (1000.0, None)):
        out = simplify(sv, sf, cell=cell, origin=origin, normals=_attributes(60)[0], stats=stats)
        assert [tuple(a.shape) for a in out] == [(0, 3)] * 3
        assert stats["clusters"] == 1 and stats["degenerate"] == 90 and stats["F_out"] == 0 and stats["V_out"] == 0
    _check_against_restatement(ngp, sv, sf, 1000.0, None, "one cell")
    # errors
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(), dict(cell=1.0, target_faces=10),
               dict(target_faces=-1), dict(cell=1.0, placement="median"), dict(cell=1.0, regularization=0.0)):
        with pytest.raises(ValueError):
            simplify(sv, sf, **kw)
    bad = sv.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        simplify(bad, sf, cell=1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        simplify(sv, sf, cell=1e-7)                       # keys beyond 2^21
    with pytest.raises(ValueError, match="2\\^21"):
        simplify(sv, sf, cell=1.0, origin=(100.0, 0.0, 0.0))   # negative keys
    for idx in ([[0, 1, 60]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="outside"):
            simplify(sv, torch.tensor(idx, dtype=torch.int32, device=DEV), cell=1.0)
    # the calls above left nothing behind: the same mesh still simplifies
    _check_against_restatement(ngp, sv, sf, 0.7, None, "after the errors")


@pytest.mark.timeout(300)
def test_displacement_is_bounded_by_the_cell_diagonal(ngp, mc_meshes):
    cases = [(*mc_meshes[(48, 48, 48)], 3.0), (*mc_meshes[(33, 70, 41)], 6.3)]
    sv, sf = ref.soup(1)
    cases.append((torch.from_numpy(sv).to(DEV), torch.from_numpy(sf).to(DEV),
                  float(np.float32((sv.max(0) - sv.min(0)).max() / 10))))
    for verts, faces, cell in cases:
        vmap = ref.simplify(_np(verts), _np(faces), cell=cell)["vertex_map"]     # the topology is bit-identical
        live = torch.from_numpy(vmap >= 0).to(DEV)
        idx = torch.from_numpy(vmap).to(DEV)[live]
        for placement in ("quadric", "mean"):
            out, _ = ngp.mesh.simplify_mesh(verts, faces, cell=cell, placement=placement)
            d = (verts[live].double() - out[idx].double()).norm(dim=-1).max().item()
            print(f"[mesh simplify] displacement {placement} cell {cell}: {d / cell:.4f} cells")
            assert d <= math.sqrt(3) * float(np.float32(cell)) * (1 + 2.0 ** -20)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cell", [0.05, 0.11])
def test_wedge_quadric_keeps_the_crease_and_the_planes(ngp, cell):
    """two 60 x 60 sheets at 90 degrees, rotated and shifted: the largest distance of an output vertex to the nearer
    plane under 'quadric' is at most a quarter of that under 'mean'.  The restatement gives 0.0445 against 0.2034
    cells (cell 0.05) and 0.0165 against 0.1813 (cell 0.11)."""
    v, f, R, t = ref.wedge()
    verts, faces = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    worst = {}
    for placement in ("quadric", "mean"):
        out, _ = ngp.mesh.simplify_mesh(verts, faces, cell=cell, placement=placement)
        worst[placement] = ref.plane_distance(_np(out), R, t).max() / cell
    print(f"[mesh simplify] wedge cell {cell}: quadric {worst['quadric']:.4f} mean {worst['mean']:.4f} cells")
    assert worst["quadric"] <= worst["mean"] / 4


@pytest.fixture(scope="module")
def sphere(ngp):
    n = 64
    ax = torch.linspace(-1, 1, n, device=DEV)
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    h = 2 / (n - 1)
    return ngp.mesh.marching_cubes((0.45 - x.norm(dim=-1)).contiguous(), 0.0, (h, h, h), (-1, -1, -1))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("target", [200, 2000, 20000])
def test_target_faces(ngp, sphere, target):
    verts, faces = sphere
    stats = {}
    v, f = ngp.mesh.simplify_mesh(verts, faces, target_faces=target, stats=stats)
    print(f"[mesh simplify] sphere V {verts.shape[0]} F {faces.shape[0]} target {target}: {stats}")
    assert f.shape[0] <= target and stats["F_out"] == f.shape[0] and stats["V_out"] == v.shape[0]
    if faces.shape[0] <= target:        # small enough: the input comes back
        assert torch.equal(v, verts) and torch.equal(f, faces) and stats["probes"] == 0 and stats["k"] is None
        return
    k = stats["k"]
    lo, hi = torch.aminmax(verts, dim=0)
    extent = float((hi - lo).max())
    assert stats["cell"] == float(np.float32(extent / k))
    more = {}
    ngp.mesh.simplify_mesh(verts, faces, cell=float(np.float32(extent / (k + 1))), stats=more)
    assert more["F_out"] > target
    assert stats["probes"] <= 2 * math.ceil(math.log2(k)) + 2
    want = ref.simplify(_np(verts), _np(faces), target_faces=target)
    assert want["stats"]["k"] == k and want["stats"]["probes"] == stats["probes"]
    assert np.array_equal(_np(f), want["faces"])
    assert int(f.max()) == v.shape[0] - 1 and torch.unique(f).numel() == v.shape[0]


# --------------------------------------------------------------------------------------- end to end on a trained field
@pytest.fixture(scope="module")
def trained(ngp):
    """the lego proxy trained for 300 steps of 4096 rays (the fixture of test_mesh_clean_gpu.py)"""
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


@pytest.mark.timeout(900)
def test_trained_field_to_a_simplified_coloured_ply(ngp, trained, tmp_path):
    """extract_mesh(resolution=160, level=10, keep_largest=1, target_faces=20000) with normals and colours evaluated
    at the new vertices; tools/extract_mesh.py writes the same bytes from a fresh process (the sums run in a fixed
    order, so nothing depends on the run)."""
    stats = {}
    verts, faces, nrm, rgb = ngp.mesh.extract_mesh(trained, resolution=160, level=10.0, keep_largest=1,
                                                   target_faces=20000, normals=True, colors=True, stats=stats)
    torch.cuda.synchronize()
    print(f"[mesh simplify e2e] {stats}")
    assert 0 < faces.shape[0] <= 20000
    assert stats["V_out"] == verts.shape[0] == nrm.shape[0] == rgb.shape[0] and stats["F_out"] == faces.shape[0]
    assert stats["F_in"] > 20000 and stats["F_in"] == stats["F_out"] + stats["degenerate"] + stats["duplicate"]
    assert stats["k"] >= 1 and stats["probes"] <= 2 * math.ceil(math.log2(stats["k"])) + 2
    assert int(faces.min()) == 0 and int(faces.max()) == verts.shape[0] - 1
    assert rgb.dtype == torch.uint8

    from ngp_amd import ckpt
    from ngp_amd.mesh import read_ply
    ck = tmp_path / "proxy.ckpt"
    ckpt.save_ckpt(trained, str(ck))
    out = tmp_path / "mesh.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--ckpt", str(ck),
                        "--scale", "0.5", "--out", str(out), "--resolution", "160", "--level", "10",
                        "--keep_largest", "1", "--target_faces", "20000", "--normals", "--colors"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("[mesh simplify e2e] tool:", line)
    for key in COUNTS + ("k", "probes"):
        assert line[key] == stats[key], key
    assert line["V"] == verts.shape[0] and line["F"] == faces.shape[0] and line["simplify_ms"] > 0
    pv, pf, pn, pc = read_ply(str(out), colors=True)
    assert pv.tobytes() == _np(verts).tobytes() and pf.tobytes() == _np(faces).tobytes()
    assert pc.tobytes() == _np(rgb).tobytes()
