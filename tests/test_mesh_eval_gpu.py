"""Mesh evaluation on the MI355X: ngp_mesh_closest through ngp_amd.mesh.closest_on_mesh against the brute force of
tests/mesh_eval_reference.py (d2 bit for bit, faces equal, for every grid the wrapper is asked to build), clipping at
max_dist, ngp_mesh_sample_surface against its restatement (bit for bit), mesh_distance end to end on meshes whose
distances are known, and the two tools."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_eval_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAR = 100.0          # a max_dist that clips nothing in the cases below


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ the cases
def _random_points(seed, n, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


def _case_one_triangle():
    verts = np.array([ref.HAND_A, ref.HAND_B, ref.HAND_C], F32)
    return np.array([h[0] for h in ref.HAND_CASES], F32), verts, np.array([[0, 1, 2]], np.int32)


def _case_counts(n):
    verts, faces = ref.small_triangles(n, 50, 0.15)
    return _random_points(100 + n, n, -1.3, 1.3), verts, faces


def _case_shared_edge():
    """two triangles over the edge (0,0,0)-(0,1,0); points whose nearest point lies on that edge: both faces give the
    same d2 there (the same two corners enter the same operations in another order where it is exact: the second
    face names the edge's corners in the same positions), and the smaller index wins"""
    verts = np.array([(0, 0, 0), (0, 1, 0), (1, 0.5, -0.5), (-1, 0.5, -0.5)], F32)
    faces = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    g = np.random.default_rng(2)
    pts = np.stack([np.zeros(64), g.uniform(0.05, 0.95, 64), g.uniform(0.1, 1.0, 64)], 1).astype(F32)
    return pts, verts, faces


def _case_fan():
    """six faces around an apex that each face names first; points on the axis above it are nearest to the apex in
    every face, with the same bits: a tie of six"""
    rim = [(math.cos(k * math.pi / 3), math.sin(k * math.pi / 3), 0.0) for k in range(6)]
    verts = np.array([(0.0, 0.0, 0.5)] + rim, F32)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
    pts = np.array([(0, 0, z) for z in (0.5, 0.75, 1.0, 3.0)] + [(0.3, 0.1, 0.9), (-0.2, 0.4, 0.2), (2, 2, 0)], F32)
    return pts, verts, faces


def _case_dead_faces():
    verts, faces = ref.mesh_with_dead_faces()
    return _random_points(7, 300, -1.3, 1.3), verts, faces


def _case_long_triangle():
    verts, faces = ref.small_triangles(11, 2000, 0.02)
    verts = np.concatenate([verts, np.array([(-1.1, -1.1, -1.1), (1.1, 1.1, 1.1), (1.1, -1.1, 1.0)], F32)])
    faces = np.concatenate([faces, np.array([[6000, 6001, 6002]], np.int32)])
    return _random_points(12, 600, -1.2, 1.2), verts, faces


def _case_random():
    verts, faces = ref.small_triangles(21, 2048, 0.03)
    pts = np.concatenate([_random_points(22, 3072, -1.0, 1.0), _random_points(23, 1024, -4.0, 4.0)])
    return pts, verts, faces


CELL_BOUNDARY = 0.25


def _case_cell_boundaries():
    """points exactly on the planes between cells of edge 0.25 from the mesh's lower corner, and one float32 ulp on
    either side of them, inside and outside the grid"""
    verts, faces = ref.small_triangles(31, 300, 0.05)
    lo = verts.min(0)
    g = np.random.default_rng(32)
    pts = []
    for axis in range(3):
        for k in range(-2, 12):
            plane = F32(lo[axis] + F32(k) * F32(CELL_BOUNDARY))
            for x in (np.nextafter(plane, F32(-np.inf)), plane, np.nextafter(plane, F32(np.inf))):
                p = g.uniform(-1.2, 1.2, 3).astype(F32)
                p[axis] = x
                pts.append(p)
    return np.array(pts, F32), verts, faces


CASES = {
    "one_triangle": (_case_one_triangle, (None, 0.3, 1.0, 8.0)),
    "n1": (lambda: _case_counts(1), (None, 0.05, 0.4, 5.0)),
    "n63": (lambda: _case_counts(63), (None, 0.05, 0.4, 5.0)),
    "n64": (lambda: _case_counts(64), (None, 0.05, 0.4, 5.0)),
    "n65": (lambda: _case_counts(65), (None, 0.05, 0.4, 5.0)),
    "n257": (lambda: _case_counts(257), (None, 0.05, 0.4, 5.0)),
    "shared_edge": (_case_shared_edge, (None, 0.1, 0.5, 4.0)),
    "fan": (_case_fan, (None, 0.2, 0.7, 4.0)),
    "dead_faces": (_case_dead_faces, (None, 0.05, 0.5, 4.0)),
    "single_cell": (_case_dead_faces, (10.0, 64.0, 1e6)),          # the whole mesh in one cell
    "long_triangle": (_case_long_triangle, (None, 0.02, 0.1, 1.0)),
    "random": (_case_random, (None, 0.02, 0.06, 0.5)),
    "cell_boundaries": (_case_cell_boundaries, (CELL_BOUNDARY, 0.03, 1.0)),
}
_REFERENCE = {}


def _reference(name):
    """(points, verts, faces, d2, face) of a case: the brute force runs once per case"""
    if name not in _REFERENCE:
        pts, verts, faces = CASES[name][0]()
        _REFERENCE[name] = (pts, verts, faces, *ref.closest_brute(pts, verts, faces, FAR))
    return _REFERENCE[name]


def _assert_same(got_d2, got_face, want_d2, want_face, tag):
    got_d2, got_face = _np(got_d2), _np(got_face)
    assert got_d2.dtype == F32 and got_face.dtype == np.int32
    bad = np.nonzero((_bits(got_d2) != _bits(want_d2)) | (got_face != want_face))[0]
    assert bad.size == 0, (tag, bad[:5], got_d2[bad[:5]], want_d2[bad[:5]], got_face[bad[:5]], want_face[bad[:5]])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(CASES))
def test_query_matches_brute_force_bit_for_bit(ngp, name):
    """every case with the wrapper's own cell and with forced ones (one of them smaller than the triangles)"""
    pts, verts, faces, want_d2, want_face = _reference(name)
    assert (want_face >= 0).all()
    if name == "shared_edge":
        assert (want_face == 0).all()            # the tie is real: the second face alone gives the same bits
        alone = ref.closest_brute(pts, verts, faces[1:], FAR)[0]
        assert np.array_equal(_bits(alone), _bits(want_d2))
    if name == "fan":
        each = [ref.closest_brute(pts[:4], verts, faces[k:k + 1], FAR)[0] for k in range(6)]
        assert all(np.array_equal(_bits(e), _bits(each[0])) for e in each) and (want_face[:4] == 0).all()
    if name == "dead_faces":
        assert not ref.nondegenerate(verts, faces).all()
    for cell in CASES[name][1]:
        stats = {}
        d2, face = ngp.mesh.closest_on_mesh(_t(pts), _t(verts), _t(faces), max_dist=FAR, cell=cell, stats=stats,
                                            squared=True)
        print(f"[mesh eval] {name} cell {cell}: {stats}")
        _assert_same(d2, face, want_d2, want_face, (name, cell))
        if cell is not None:
            assert stats["cell"] == float(F32(cell)) and stats["probes"] == 1
        if name == "single_cell":
            assert stats["dims"] == [1, 1, 1]
        if name == "long_triangle" and cell is not None:
            assert stats["references"] >= stats["dims"][0] * stats["dims"][1] * stats["dims"][2]   # it is in every cell
    # dist is the square root of d2; max_dist=None clips nothing; a second run gives the same bytes
    dist, face = ngp.mesh.closest_on_mesh(_t(pts), _t(verts), _t(faces))
    assert torch.equal(dist, torch.sqrt(_t(want_d2))) and np.array_equal(_np(face), want_face)
    again = ngp.mesh.closest_on_mesh(_t(pts), _t(verts), _t(faces))
    assert torch.equal(dist, again[0]) and torch.equal(face, again[1])


# --------------------------------------------------------------------------------------------------------- clipping
@pytest.mark.timeout(120)
def test_clipping(ngp):
    closest = ngp.mesh.closest_on_mesh
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F32)
    faces = np.array([[0, 1, 2]], np.int32)
    above = np.nextafter(F32(0.5), F32(1))
    xy = [(0.25, 0.25), (0.5, 0.25), (0.125, 0.5)]
    pts = np.array([(x, y, z) for z in (0.5, above, -0.5, -above) for x, y in xy], F32)
    want_d2, want_face = ref.closest_brute(pts, verts, faces, 0.5)
    assert want_face.tolist() == [0, 0, 0, -1, -1, -1] * 2 and (want_d2 == F32(0.25)).all()
    for cell in (None, 0.1, 3.0):
        d2, face = closest(_t(pts), _t(verts), _t(faces), max_dist=0.5, cell=cell, squared=True)
        _assert_same(d2, face, want_d2, want_face, ("clip", cell))
    dist, _ = closest(_t(pts), _t(verts), _t(faces), max_dist=0.5)
    assert (dist == 0.5).all()
    # no face: everything is clipped
    none_f = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    stats = {}
    d2, face = closest(_t(pts), _t(verts), none_f, max_dist=0.5, squared=True, stats=stats)
    assert (d2 == 0.25).all() and (face == -1).all() and stats["references"] == 0 and stats["dims"] is None
    dist, face = closest(_t(pts), torch.zeros(0, 3, device=DEV), none_f)
    assert (face == -1).all() and dist.shape == (12,)
    # no point
    d2, face = closest(torch.zeros(0, 3, device=DEV), _t(verts), _t(faces))
    assert d2.shape == (0,) and face.shape == (0,)
    # the random case at the median distance: the restatement alone says which half is clipped
    pts, verts, faces, far_d2, _ = _reference("random")
    max_dist = float(np.sqrt(np.median(far_d2)))
    want_d2, want_face = ref.closest_brute(pts, verts, faces, max_dist)
    clipped = (want_face < 0).mean()
    assert 0.4 < clipped < 0.6
    for cell in (None, 0.02, 0.3):
        d2, face = closest(_t(pts), _t(verts), _t(faces), max_dist=max_dist, cell=cell, squared=True)
        _assert_same(d2, face, want_d2, want_face, ("clip half", cell))
    for kw in (dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(cell=0.0), dict(cell=float("inf")),
               dict(cell=1e-4)):                                  # the last: more than 1024 cells per axis
        with pytest.raises(ValueError):
            closest(_t(pts), _t(verts), _t(faces), **kw)
    bad = verts.copy()
    bad[5, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        closest(_t(pts), _t(bad), _t(faces))


# ---------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.timeout(120)
def test_sampler_matches_restatement_bit_for_bit(ngp):
    mesh = ngp.mesh
    dead_v, dead_f = ref.mesh_with_dead_faces()             # its first and last faces have no area
    soup_v, soup_f = ref.small_triangles(41, 3000, 0.05)
    for tag, verts, faces in (("dead", dead_v, dead_f), ("soup", soup_v, soup_f), ("one", dead_v[3:6], dead_f[:1] * 0 + [[0, 1, 2]])):
        faces = faces.astype(np.int32)
        tv, tf = _t(verts), _t(faces)
        cdf = mesh.face_area_cdf(tv, tf)
        assert cdf.dtype == torch.float64 and cdf.shape == (faces.shape[0],)
        want_cdf = ref.area_cdf(verts, faces)
        assert np.abs(_np(cdf) - want_cdf).max() <= 1e-12 * want_cdf[-1]
        for n in (0, 1, 65, 10_000):
            pts, face = mesh.sample_surface(tv, tf, n, seed=5)
            assert pts.shape == (n, 3) and pts.dtype == torch.float32 and face.dtype == torch.int32
            if n == 0:
                continue
            want_pts, want_face = ref.sample_surface(verts, faces, _np(cdf), n, 5)      # the GPU's own cdf
            assert np.array_equal(_np(face), want_face), (tag, n)
            assert np.array_equal(_bits(_np(pts)), _bits(want_pts)), (tag, n)
            again = mesh.sample_surface(tv, tf, n, seed=5, cdf=cdf)
            assert torch.equal(again[0], pts) and torch.equal(again[1], face)
            if n >= 65:
                other = mesh.sample_surface(tv, tf, n, seed=6)
                assert not torch.equal(other[0], pts)
        if tag == "dead":
            dead = np.nonzero(np.diff(np.concatenate([[0.0], want_cdf])) == 0)[0]
            assert {0, 39} <= set(dead) and not np.isin(_np(face), dead).any()
    # a mesh without area, a negative count, a cdf of the wrong size
    flat = _t(np.array([[0, 0, 1], [1, 1, 1]], np.int32))
    with pytest.raises(ValueError, match="area"):
        mesh.sample_surface(_t(dead_v), flat, 10)
    with pytest.raises(ValueError, match="area"):
        mesh.sample_surface(_t(dead_v), flat[:0], 10)
    with pytest.raises(ValueError):
        mesh.sample_surface(_t(dead_v), _t(dead_f), -1)
    with pytest.raises(ValueError, match="cdf"):
        mesh.sample_surface(_t(dead_v), _t(dead_f), 10, cdf=torch.ones(3, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.timeout(120)
def test_sheets_a_quarter_apart_and_a_mesh_against_itself(ngp):
    va, fa = ref.sheet(20, 0.0)
    vb, fb = ref.sheet(20, 0.25)
    stats = {}
    out = ngp.mesh.mesh_distance(_t(va), _t(fa), _t(vb), _t(fb), n_samples=20_000, thresholds=(0.2, 0.3), stats=stats)
    print(f"[mesh eval] sheets: {out} {stats}")
    for key in ("accuracy", "completeness", "chamfer", "hausdorff"):
        assert abs(out[key] - 0.25) <= 1e-6, key
    assert out["fscore"] == [0.0, 1.0] and out["precision"] == [0.0, 1.0] and out["recall"] == [0.0, 1.0]
    assert out["clipped_a"] == 0.0 and out["clipped_b"] == 0.0
    assert stats["a_to_b"]["references"] > 0 and stats["b_to_a"]["query_ms"] > 0
    # clipped at 0.1: every sample, and the distances are max_dist
    out = ngp.mesh.mesh_distance(_t(va), _t(fa), _t(vb), _t(fb), n_samples=1000, max_dist=0.1)
    assert out["clipped_a"] == 1.0 and out["clipped_b"] == 1.0 and abs(out["hausdorff"] - 0.1) <= 1e-7
    # a mesh against itself: the sampler's and the query's rounding
    for verts, faces in (ref.small_triangles(51, 500, 0.1), ref.sheet(20, 0.3, extent=3.0)):
        out = ngp.mesh.mesh_distance(_t(verts), _t(faces), _t(verts), _t(faces), n_samples=20_000, thresholds=(1e-5,))
        bound = 2.0 ** -19 * float(np.abs(verts).max())
        print(f"[mesh eval] self: accuracy {out['accuracy']:.3g} hausdorff {out['hausdorff']:.3g} bound {bound:.3g}")
        assert out["accuracy"] <= bound and out["completeness"] <= bound and out["clipped_a"] == 0.0


# ------------------------------------------------------------------------------------------------------------ tools
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _json_line(capsys):
    return json.loads([line for line in capsys.readouterr().out.splitlines() if line.startswith("{")][-1])


@pytest.mark.timeout(120)
def test_eval_mesh_tool_prints_what_mesh_distance_gives(ngp, tmp_path, capsys):
    va, fa = ref.sheet(12, 0.0)
    vb, fb = ref.small_triangles(61, 400, 0.1, lo=0.0, hi=1.0)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ngp.mesh.write_ply(a, va, fa)
    ngp.mesh.write_ply(b, vb, fb)
    want = ngp.mesh.mesh_distance(_t(va), _t(fa), _t(vb), _t(fb), n_samples=5000, thresholds=(0.05, 0.2), seed=9)
    _tool("eval_mesh").main(["--mesh", a, "--ref", b, "--samples", "5000", "--thresholds", "0.05", "0.2", "--seed", "9"])
    line = _json_line(capsys)
    for key, value in want.items():
        assert line[key] == value, key
    assert (line["V"], line["F"], line["V_ref"], line["F_ref"]) == (va.shape[0], fa.shape[0], vb.shape[0], fb.shape[0])
    assert line["a_to_b_query_ms"] > 0 and line["b_to_a_build_ms"] > 0
    # clipped, and against the analytic proxy scene: the sheet z = 0 cuts through its solids
    _tool("eval_mesh").main(["--mesh", a, "--ref", b, "--samples", "5000", "--max_dist", "0.01"])
    assert abs(_json_line(capsys)["hausdorff"] - 0.01) <= 1e-8
    _tool("eval_mesh").main(["--mesh", a, "--ref_proxy", "--ref_resolution", "64", "--samples", "5000"])
    line = _json_line(capsys)
    assert line["F_ref"] > 1000 and 0 < line["completeness"] < 1 and line["clipped_a"] == 0


@pytest.fixture(scope="module")
def checkpoint(ngp, tmp_path_factory):
    """the lego proxy trained for 300 steps of 4096 rays (the fixture of test_mesh_simplify_gpu.py), saved"""
    from ngp_amd import ckpt
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
    path = str(tmp_path_factory.mktemp("mesh_eval") / "proxy.ckpt")
    ckpt.save_ckpt(model, path)
    return path


# the keys of extract_mesh.py's JSON line with --target_faces before --report_distance existed
TODAY_KEYS = {"V", "F", "lattice", "density_ms", "mc_ms", "normals_ms", "d2h_ms", "ply_ms", "clean_ms", "colors_ms",
              "simplify_ms", "components", "V_removed", "F_removed", "cell", "k", "probes", "clusters", "V_in", "V_out",
              "F_in", "F_out", "degenerate", "duplicate", "probe_ms", "emit_ms"}


@pytest.mark.timeout(600)
def test_extract_mesh_reports_the_simplification_distance(ngp, checkpoint, tmp_path, capsys):
    tool = _tool("extract_mesh")
    base = ["--ckpt", checkpoint, "--scale", "0.5", "--out", str(tmp_path / "mesh.ply"), "--resolution", "128",
            "--level", "10", "--keep_largest", "1"]
    tool.main(base + ["--target_faces", "5000"])
    plain = _json_line(capsys)
    tool.main(base + ["--target_faces", "5000", "--report_distance", "--distance_samples", "100000"])
    line = _json_line(capsys)
    print("[mesh eval] extract_mesh --report_distance:", line["simplify_distance"])
    assert set(plain) == TODAY_KEYS
    assert set(line) == TODAY_KEYS | {"simplify_distance", "simplify_distance_ms"}
    assert all(line[k] == plain[k] for k in plain if not k.endswith("_ms"))
    sd = line["simplify_distance"]
    assert set(sd) == {"accuracy", "completeness", "hausdorff", "accuracy_cells", "completeness_cells",
                       "hausdorff_cells", "cell", "samples"}
    assert all(math.isfinite(sd[k]) for k in sd) and sd["cell"] == line["cell"] and sd["samples"] == 100000
    assert 0 < sd["accuracy"] <= sd["hausdorff"] and 0 < sd["completeness"] <= sd["hausdorff"]
    assert sd["hausdorff_cells"] == sd["hausdorff"] / sd["cell"]
    assert sd["hausdorff"] <= math.sqrt(3) * sd["cell"] * (1 + 2.0 ** -20)     # the bound simplify_mesh documents
    # without simplification the flag means nothing and is refused, as other meaningless combinations are
    with pytest.raises(SystemExit):
        tool.main(base + ["--report_distance"])
    assert "report_distance" in capsys.readouterr().err
