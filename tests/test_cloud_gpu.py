"""Point clouds on the MI355X (include/ngp_hip.h M5) through ngp_amd.cloud: ngp_cloud_nearest against the f32 brute
force of tests/cloud_reference.py (d2 bit for bit, indices equal, for every grid asked for) and against scipy's k-d
tree, the transform path, the 18 sums against float64 numpy within the worst-case accumulation bound and byte for byte
from run to run, ngp_cloud_voxel_mean bit for bit, ICP on the subset input against the known pose, the metrics on
clouds whose distances are known, and tools/eval_mesh.py --ref_points end to end."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cloud_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAR = 1.0e4          # a max_dist that clips nothing in the cases below


@pytest.fixture(scope="module")
def cloud(ngp):
    from ngp_amd import cloud
    return cloud


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _uniform(seed, n, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


def _assert_same(got_d2, got_index, want_d2, want_index, tag):
    got_d2, got_index = _np(got_d2), _np(got_index)
    assert got_d2.dtype == F32 and got_index.dtype == np.int32
    bad = np.nonzero((_bits(got_d2) != _bits(want_d2)) | (got_index != want_index))[0]
    assert bad.size == 0, (tag, bad[:5], got_d2[bad[:5]], want_d2[bad[:5]], got_index[bad[:5]], want_index[bad[:5]])


# ------------------------------------------------------------------------------------------------------ the cases
# name -> (queries, cloud, forced cells beside the wrapper's own)
def _case_cube():
    return _uniform(1, 2000), _uniform(2, 3000), (1.0 / 200, 4.0)


def _case_slab():
    """a cloud of extent 1 x 1 x 0.1, so that cells of 1/512 of the extent stay below 2^24: 513 x 513 x 52 of them for
    3000 points, many empty rings around every query"""
    squash = np.array([1, 1, 0.1], F32)
    q = np.concatenate([_uniform(10, 1500) * squash, _uniform(11, 500)])
    return q, _uniform(12, 3000) * squash, (1.0 / 512,)


def _case_offset():
    q, c, _ = _case_cube()
    return q + F32(1000), c + F32(1000), (0.05,)


def _case_duplicates():
    c = _uniform(3, 1500)
    return _uniform(4, 2000), np.concatenate([c, c[::-1]]), (0.03,)      # point k and point 2999 - k coincide


def _case_one_cell():
    return _uniform(5, 500), (F32(0.5) + _uniform(6, 700) * F32(1e-3)), (1.0,)


def _case_one_point():
    return _uniform(7, 300), np.array([[0.25, 0.5, 0.75]], F32), (0.1,)


def _case_outside():
    return _uniform(8, 500) + F32(50) * np.array([1, -1, 1], F32), _uniform(9, 3000), (0.05,)


CASES = {"cube": _case_cube, "slab": _case_slab, "offset": _case_offset, "duplicates": _case_duplicates, "one_cell": _case_one_cell,
         "one_point": _case_one_point, "outside": _case_outside}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(CASES))
def test_nearest_matches_brute_force_bit_for_bit(cloud, name):
    from scipy.spatial import cKDTree
    q, c, cells = CASES[name]()
    want_d2, want_index = ref.nearest_brute(q, c, FAR)
    assert (want_index >= 0).all()
    if name == "duplicates":
        assert (want_index < 1500).all()                     # the tie is real and the smaller index wins
    for cell in (None,) + cells:
        stats = {}
        d2, index = cloud.nearest_points(_t(q), _t(c), max_dist=FAR, cell=cell, squared=True, stats=stats)
        print(f"[cloud] {name} cell {cell}: {stats}")
        _assert_same(d2, index, want_d2, want_index, (name, cell))
        assert stats["references"] == c.shape[0] and stats["dropped"] == 0
        if cell is not None:
            assert stats["cell"] == float(F32(cell))
    if name == "cube":
        assert stats["dims"] == [1, 1, 1]                    # the last forced cell: 4 extents
    # dist is the square root; max_dist=None clips nothing; a built grid gives the same; a second run the same bytes
    dist, index = cloud.nearest_points(_t(q), _t(c))
    assert torch.equal(dist, torch.sqrt(_t(want_d2))) and np.array_equal(_np(index), want_index)
    grid = cloud.PointGrid(_t(c))
    again = cloud.nearest_points(_t(q), grid)
    assert torch.equal(dist, again[0]) and torch.equal(index, again[1])
    assert torch.equal(grid.sorted_points, _t(c)[grid.order.long()])
    # against a k-d tree in float64: 4 ulp of the largest coordinate
    exact = cKDTree(c.astype(np.float64)).query(q.astype(np.float64))[0]
    ulp = float(np.spacing(F32(max(np.abs(q).max(), np.abs(c).max()))))
    assert np.abs(_np(dist).astype(np.float64) - exact).max() <= 4 * ulp


@pytest.mark.timeout(120)
def test_clipping_empty_cloud_and_queries_that_are_not_finite(cloud):
    nearest = cloud.nearest_points
    # max_dist equal to an exact distance keeps it, one ulp below clips it
    c = np.array([[3, 4, 0], [30, 40, 0]], F32)
    q = np.array([[0, 0, 0], [0, 0, 1]], F32)
    for cell in (None, 0.5, 100.0):
        d2, index = nearest(_t(q), _t(c), max_dist=5.0, cell=cell, squared=True)
        assert _np(d2).tolist() == [25.0, 25.0] and _np(index).tolist() == [0, -1]
        below = float(np.nextafter(F32(5), F32(0)))
        d2, index = nearest(_t(q), _t(c), max_dist=below, cell=cell, squared=True)
        assert _np(index).tolist() == [-1, -1] and (_np(d2) == F32(below) * F32(below)).all()
    # the cube at the median distance: the restatement alone says which half is clipped
    q, c, _ = _case_cube()
    far_d2, _ = ref.nearest_brute(q, c, FAR)
    max_dist = float(np.sqrt(np.median(far_d2)))
    want_d2, want_index = ref.nearest_brute(q, c, max_dist)
    assert 0.4 < (want_index < 0).mean() < 0.6
    for cell in (None, 0.01, 0.3):
        d2, index = nearest(_t(q), _t(c), max_dist=max_dist, cell=cell, squared=True)
        _assert_same(d2, index, want_d2, want_index, ("clip half", cell))
    # an empty cloud clips everything; no query is no work
    none = torch.zeros(0, 3, device=DEV)
    stats = {}
    d2, index = nearest(_t(q), none, max_dist=0.5, squared=True, stats=stats)
    assert (d2 == 0.25).all() and (index == -1).all() and stats["references"] == 0 and stats["dims"] is None
    dist, index = nearest(_t(q), none)
    assert (index == -1).all() and dist.shape == (2000,)
    d2, index = nearest(none, _t(c))
    assert d2.shape == (0,) and index.shape == (0,) and index.dtype == torch.int32
    # a query with a NaN or infinite coordinate matches nothing; its neighbours are untouched
    bad = q[:300].copy()
    bad[7, 1] = np.nan
    bad[100] = np.nan
    bad[200, 0] = np.inf
    want_d2, want_index = ref.nearest_brute(bad, c, 2.0)
    assert want_index[[7, 100, 200]].tolist() == [-1, -1, -1] and (want_index >= 0).sum() == 297
    for cell in (None, 0.02):
        d2, index = nearest(_t(bad), _t(c), max_dist=2.0, cell=cell, squared=True)
        _assert_same(d2, index, want_d2, want_index, ("nan", cell))
    # points of the cloud that are not finite are dropped and counted; indices stay those of the input
    holes = c.copy()
    holes[[0, 17, 2999]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    want_d2, want_index = ref.nearest_brute(q, holes, FAR)
    stats = {}
    d2, index = nearest(_t(q), _t(holes), max_dist=FAR, squared=True, stats=stats)
    _assert_same(d2, index, want_d2, want_index, "holes")
    assert stats["dropped"] == 3 and stats["references"] == 2997
    for kw in (dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(cell=0.0), dict(cell=float("inf")),
               dict(cell=1e-4)):                              # the last: more than 1024 cells per axis
        with pytest.raises(ValueError):
            nearest(_t(q), _t(c), **kw)


@pytest.mark.timeout(120)
def test_transform_is_the_f32_expression_of_the_header(cloud):
    q, c, _ = _case_cube()
    T = ref.similarity(ref.rotation((1, -2, 0.5), 20.0), (0.1, -0.2, 0.05), 1.1)
    T[:3, 3] += 0.5 - T[:3, :3] @ np.full(3, 0.5)             # about the cube's centre: the queries stay near it
    moved = ref.transform_f32(q, T[:3, :4].astype(F32).reshape(-1))
    want_d2, want_index = ref.nearest_brute(moved, c, FAR)
    d2, index = cloud.nearest_points(_t(q), _t(c), max_dist=FAR, transform=T, squared=True)
    _assert_same(d2, index, want_d2, want_index, "transform")
    plain = cloud.nearest_points(_t(moved), _t(c), max_dist=FAR, squared=True)
    assert torch.equal(plain[0], d2) and torch.equal(plain[1], index)
    assert np.array_equal(_bits(_np(cloud.transform_points(_t(q), np.eye(4)))), _bits(q))


@pytest.mark.timeout(120)
def test_sums_of_a_registration_step(ngp, cloud):
    n = 4096
    c = _uniform(21, 3000)
    q = (c[np.random.default_rng(22).integers(0, 3000, n)] + _uniform(23, n, -0.01, 0.01)).astype(F32)
    T = ref.similarity(ref.rotation((0.3, 1, -0.2), 2.0), (0.01, 0.0, -0.01))
    x12 = T[:3, :4].astype(F32).reshape(-1)
    grid = cloud.PointGrid(_t(c))
    centre = np.array(list(grid.centre), F32)
    assert np.array_equal(centre, (0.5 * (c.min(0).astype(np.float64) + c.max(0).astype(np.float64))).astype(F32))
    for max_dist, some_clipped in ((1.0, False), (0.03, True)):
        d2, index = cloud.nearest_points(_t(q), grid, max_dist=max_dist, transform=T, squared=True)
        d2, index = _np(d2), _np(index)
        ok = index >= 0
        assert ok.all() != some_clipped and ok.sum() > 1000
        moved = ref.transform_f32(q, x12)
        terms = np.concatenate([ref.sums18_terms(moved[ok], c[index[ok]], centre), d2[ok, None].astype(np.float64)], 1)
        want = terms.sum(0)
        bound = n * 2.0 ** -53 * np.abs(terms).sum(0)
        rows = n // 256
        results = []
        for _ in range(2):
            partials = torch.full((rows, 18), np.nan, dtype=torch.float64, device=DEV)
            sums = torch.full((18,), np.nan, dtype=torch.float64, device=DEV)
            grid.launch(_t(q), float(F32(max_dist)), cloud._xform12(T), partials=partials)
            ngp._lib.call("cloud_sum_partials", partials, rows, sums)
            results.append((_np(partials), _np(sums)))
        got = results[0][1]
        print(f"[cloud] sums at max_dist {max_dist}: worst error / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3g}")
        assert got[0] == ok.sum()
        assert (np.abs(got - want) <= bound).all(), (got, want, bound)
        assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
        # a row is its own 256 queries
        assert np.array_equal(results[0][0][:, 0], ok.reshape(rows, 256).sum(1).astype(np.float64))


@pytest.mark.timeout(120)
def test_voxel_mean_matches_the_sequential_restatement(cloud):
    g = np.random.default_rng(31)
    p = _uniform(32, 5000)
    p[4999] = [7.0, 7.0, 7.0]                                   # a voxel of its own
    nrm = g.normal(size=(5000, 3)).astype(F32)
    col = g.integers(0, 256, (5000, 3)).astype(np.uint8)
    for voxel in (0.1, 0.013, 10.0):
        want = ref.voxel_mean(p, voxel, nrm, col)
        got = cloud.voxel_downsample(_t(p), voxel, normals=_t(nrm), colors=_t(col))
        assert got[0].shape == want[0].shape
        assert np.array_equal(_bits(_np(got[0])), _bits(want[0])) and np.array_equal(_bits(_np(got[1])), _bits(want[1]))
        assert np.array_equal(_np(got[2]), want[2])
        alone = cloud.voxel_downsample(_t(p), voxel)
        assert torch.equal(alone[0], got[0]) and alone[1] is None and alone[2] is None
    assert got[0].shape == (1, 3)                                # voxel 10: every point in one
    assert np.array_equal(_np(cloud.voxel_downsample(_t(p), 0.1)[0])[-1], p[4999])
    # colours: a mean of k + 1/2 rounds away from zero
    two = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [5.3, 0.1, 0.1], [5.6, 0.1, 0.1]], F32)
    c2 = np.array([[0, 1, 255], [1, 2, 254], [10, 20, 30], [11, 23, 30]], np.uint8)
    got = cloud.voxel_downsample(_t(two), 1.0, colors=_t(c2))
    assert _np(got[2]).tolist() == [[1, 2, 255], [11, 22, 30]]
    # an origin moves the lattice; keys that do not fit int64 are refused
    want = ref.voxel_mean(p, 0.1, origin=(-0.05, -0.05, -0.05))
    got = cloud.voxel_downsample(_t(p), 0.1, origin=(-0.05, -0.05, -0.05))
    assert np.array_equal(_bits(_np(got[0])), _bits(want[0]))
    with pytest.raises(ValueError, match="int64"):
        cloud.voxel_downsample(_t(p), 1e-7 * 1e-7)
    with pytest.raises(ValueError):
        cloud.voxel_downsample(_t(p), 0.0)
    assert cloud.voxel_downsample(_t(p[:0]), 0.1)[0].shape == (0, 3)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("scale", [1.0, 1.03])
def test_icp_recovers_the_pose_of_the_subset_input(cloud, scale):
    """once every correspondence is exact the only error left is the f32 rounding of the moved query, 2^-24 ~ 6e-8 per
    coordinate at unit extent; the bounds allow 16 times that"""
    source, target, T_true = ref.subset_problem(scale=scale)
    grid = cloud.PointGrid(_t(target))
    T, info = cloud.icp(_t(source), None, 0.1, with_scale=scale != 1.0, grid=grid)
    print(f"[cloud] icp scale {scale}: {info['iterations']} iterations, rmse {info['inlier_rmse']:.3g}, "
          f"{info['ms_per_iteration']:.3f} ms per iteration, |R - R_true| {np.linalg.norm(T[:3, :3] - T_true[:3, :3]):.3g}, "
          f"|t - t_true| {np.abs(T[:3, 3] - T_true[:3, 3]).max():.3g}")
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert np.linalg.norm(T[:3, :3] - T_true[:3, :3]) <= 1e-6
    assert np.abs(T[:3, 3] - T_true[:3, 3]).max() <= 1e-6
    assert info["fitness"] == 1.0 and 0 < info["iterations"] < 30
    assert len(info["fitness_history"]) == len(info["rmse_history"]) == len(info["iteration_ms"]) == info["iterations"] + 1
    if scale == 1.0:
        # the same through `target`, and from an init that holds most of the motion
        again, _ = cloud.icp(_t(source), _t(target), 0.1)
        assert np.array_equal(again, T)
        near = T_true @ ref.similarity(ref.rotation((0, 0, 1), 0.5), (0.002, 0, 0))
        T2, info2 = cloud.icp(_t(source), None, 0.1, init=near, grid=grid)
        assert np.abs(T2 - T_true).max() <= 1e-6 and info2["iterations"] <= info["iterations"]
        # fewer than 3 matches: nothing to fit
        with pytest.raises(ValueError, match="correspondences"):
            cloud.icp(_t(source + F32(5)), None, 0.1, grid=grid)
        with pytest.raises(ValueError):
            cloud.icp(_t(source[:0]), None, 0.1, grid=grid)


@pytest.mark.timeout(120)
def test_metrics_of_two_lattices_a_quarter_apart(ngp, cloud):
    xy = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2) / 64.0
    a = np.concatenate([xy, np.zeros((4096, 1))], 1).astype(F32)
    b = np.concatenate([xy, np.full((4096, 1), 0.25)], 1).astype(F32)
    out = cloud.cloud_distance(_t(a), _t(b), thresholds=(0.2, 0.25))
    for key in ("accuracy", "completeness", "chamfer", "hausdorff"):
        assert out[key] == 0.25, key
    assert out["fscore"] == [0.0, 1.0] and out["precision"] == [0.0, 1.0] and out["recall"] == [0.0, 1.0]
    assert out["clipped_a"] == 0.0 and out["clipped_b"] == 0.0
    want = ngp.mesh.distance_metrics(*[torch.zeros(1, device=DEV)] * 4, thresholds=(0.2, 0.25))
    assert list(out) == list(want)                               # the keys of mesh_distance, in its order
    out = cloud.cloud_distance(_t(a), _t(a), thresholds=(1e-9,))
    assert out["accuracy"] == 0.0 and out["hausdorff"] == 0.0 and out["fscore"] == [1.0]
    out = cloud.cloud_distance(_t(a), _t(b), max_dist=0.1)
    assert out["clipped_a"] == 1.0 and abs(out["hausdorff"] - 0.1) <= 1e-7


# ------------------------------------------------------------------------------------------------------------- tool
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _json_line(capsys):
    return json.loads([line for line in capsys.readouterr().out.splitlines() if line.startswith("{")][-1])


def _box(lo, hi):
    lo, hi = np.array(lo, F32), np.array(hi, F32)
    v = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def _l_mesh():
    """two boxes that form an L of unit extent: no symmetry, so its pose is unique"""
    v0, f0 = _box((0.0, 0.0, 0.0), (1.0, 0.3, 0.2))
    v1, f1 = _box((0.0, 0.3, 0.0), (0.25, 0.8, 0.45))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + 8]).astype(np.int32)


@pytest.mark.timeout(300)
def test_eval_mesh_tool_registers_against_a_point_cloud(ngp, cloud, tmp_path, capsys):
    tool = _tool("eval_mesh")
    verts, faces = _l_mesh()
    gt, _ = ngp.mesh.sample_surface(_t(verts), _t(faces), 1 << 15, seed=1)
    ref_ply, mesh_ply, moved_ply = (str(tmp_path / n) for n in ("gt.ply", "mesh.ply", "moved.ply"))
    cloud.write_ply_points(ref_ply, gt)
    ngp.mesh.write_ply(mesh_ply, verts, faces)
    # the reconstruction lives in another frame: S takes the reference's frame to it; the file holds a guess at S^-1
    S = ref.similarity(ref.rotation((1, 1, 0.3), 40.0), (0.5, -0.3, 0.2), 1.7)
    moved = (verts.astype(np.float64) @ S[:3, :3].T + S[:3, 3]).astype(F32)
    ngp.mesh.write_ply(moved_ply, moved, faces)
    guess = ref.similarity(ref.rotation((0.2, -1, 0.4), 2.0), (0.015, -0.01, 0.01)) @ np.linalg.inv(S)
    init_txt, out_txt = str(tmp_path / "init.txt"), str(tmp_path / "refined.txt")
    np.savetxt(init_txt, guess)
    dtau = 0.01
    common = ["--ref_points", ref_ply, "--samples", str(1 << 17), "--seed", "2", "--dtau", str(dtau)]
    tool.main(["--mesh", mesh_ply] + common + ["--align", "none"])
    plain = _json_line(capsys)
    tool.main(["--mesh", moved_ply] + common + ["--init_transform", init_txt, "--align", "tnt", "--save_transform",
                                                 out_txt])
    line = _json_line(capsys)
    T = np.array(line["transform"])
    err = np.abs(T @ S - np.eye(4)).max()
    with capsys.disabled():
        print(f"[cloud] tool: F at dtau aligned {line['fscore_dtau']:.4f}, un-moved {plain['fscore_dtau']:.4f}, "
              f"|T S - I| {err:.3g}, stages {line['stages']}, points {line['points']}")
    assert err <= 1e-3                                            # of the unit extent
    assert line["fscore_dtau"] >= plain["fscore_dtau"] - 0.01
    assert np.array_equal(np.loadtxt(out_txt), T)
    assert line["align"] == "tnt" and len(line["stages"]) == 3
    assert all(s["fitness"] > 0.9 and s["iterations"] <= 20 and s["ms"] > 0 for s in line["stages"])
    assert line["points"]["gt"] == 1 << 15 and 0 < line["points"]["gt_scored"] <= 1 << 15
    assert set(plain) == set(line) and plain["align"] == "none" and plain["stages"] == []
    assert np.array_equal(np.array(plain["transform"]), np.eye(4))
    # a crop in the reference's frame keeps the long bar only; vertices stand for the mesh
    crop_json = str(tmp_path / "crop.json")
    with open(crop_json, "w") as fh:
        json.dump({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0,
                   "bounding_polygon": [[-0.1, -0.1, 0], [1.1, -0.1, 0], [1.1, 0.29, 0], [-0.1, 0.29, 0]]}, fh)
    tool.main(["--mesh", mesh_ply] + common + ["--crop", crop_json, "--align", "icp", "--recon_from", "vertices"])
    line = _json_line(capsys)
    assert 0 < line["points"]["gt_cropped"] < 1 << 15 and line["points"]["recon"] == 16
    assert len(line["stages"]) == 1 and line["clipped_a"] == 0.0
    # the new flags mean nothing without --ref_points
    with pytest.raises(SystemExit):
        tool.main(["--mesh", mesh_ply, "--ref", mesh_ply, "--align", "tnt"])
    assert "ref_points" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tool.main(["--mesh", mesh_ply, "--ref_points", ref_ply, "--align", "tnt"])
    assert "dtau" in capsys.readouterr().err
