"""The host side of ngp_amd.cloud, without a GPU: point-cloud PLY files, the crop volume against a float64
restatement, kabsch() on exact sums, and the restatement ICP of tests/cloud_reference.py on the input the GPU test
uses (so that a failure there is the kernels', not the problem's)."""
import json

import numpy as np
import pytest
import torch

import cloud_reference as ref

F32 = np.float32


@pytest.fixture(scope="module")
def cloud(ngp):
    from ngp_amd import cloud
    return cloud


# -------------------------------------------------------------------------------------------------------- PLY files
def _points(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.uniform(-2, 2, (n, 3)).astype(F32), g.normal(size=(n, 3)).astype(F32),
            g.integers(0, 256, (n, 3)).astype(np.uint8))


def test_read_ply_points_ascii(cloud, tmp_path):
    p, nrm, col = _points(7)
    path = tmp_path / "a.ply"
    head = ["ply", "format ascii 1.0", "comment made by hand", "element vertex 7"]
    head += [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    head += [f"property uchar {k}" for k in ("red", "green", "blue")] + ["end_header"]
    rows = [" ".join([repr(float(v)) for v in np.concatenate([p[i], nrm[i]])] + [str(int(c)) for c in col[i]])
            for i in range(7)]
    path.write_text("\n".join(head + rows) + "\n")
    got = cloud.read_ply_points(str(path))
    assert got[0].dtype == F32 and got[2].dtype == np.uint8
    assert np.array_equal(got[0], p) and np.array_equal(got[1], nrm) and np.array_equal(got[2], col)
    # an ascii file may carry a list inside the vertex element: it is its length and that many values
    head = ["ply", "format ascii 1.0", "element vertex 2", "property float x", "property list uchar int seen_from",
            "property float y", "property float z", "end_header", "1 2 7 8 2 3", "4 0 5 6"]
    path.write_text("\n".join(head) + "\n")
    got = cloud.read_ply_points(str(path))
    assert np.array_equal(got[0], np.array([[1, 2, 3], [4, 5, 6]], F32)) and got[1] is None and got[2] is None


def test_read_ply_points_binary_mixed_types(cloud, tmp_path):
    p, _, col = _points(33, 1)
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("scalar_intensity", "<f4"), ("red", "u1"),
                   ("green", "u1"), ("blue", "u1")])
    rec = np.empty(33, dt)
    for k, name in enumerate("xyz"):
        rec[name] = p[:, k].astype(np.float64)
    rec["scalar_intensity"] = 0.5
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = col[:, k]
    head = ["ply", "format binary_little_endian 1.0", "element vertex 33", "property double x", "property double y",
            "property double z", "property float scalar_intensity", "property uchar red", "property uchar green",
            "property uchar blue", "end_header"]
    path = tmp_path / "b.ply"
    path.write_bytes(("\n".join(head) + "\n").encode() + rec.tobytes())
    got = cloud.read_ply_points(str(path))
    assert np.array_equal(got[0], p) and got[1] is None and np.array_equal(got[2], col)


def test_read_ply_points_skips_faces_and_refuses_what_it_cannot_read(cloud, ngp, tmp_path):
    p, nrm, _ = _points(5, 2)
    faces = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    path = str(tmp_path / "mesh.ply")
    ngp.mesh.write_ply(path, p, faces, normals=nrm)              # a trailing face element with a list
    got = cloud.read_ply_points(path)
    assert np.array_equal(got[0], p) and np.array_equal(got[1], nrm) and got[2] is None
    # what write_ply_points wrote, with and without attributes
    p, nrm, col = _points(100, 3)
    for kw in ({}, dict(normals=nrm), dict(colors=col), dict(normals=nrm, colors=col)):
        cloud.write_ply_points(path, p, **kw)
        got = cloud.read_ply_points(path)
        assert np.array_equal(got[0], p)
        assert (got[1] is None) == ("normals" not in kw) and (got[2] is None) == ("colors" not in kw)
        assert got[1] is None or np.array_equal(got[1], nrm)
        assert got[2] is None or np.array_equal(got[2], col)
    cloud.write_ply_points(path, p[:0])
    assert cloud.read_ply_points(path)[0].shape == (0, 3)
    # big-endian is refused, by name
    raw = open(path, "rb").read().replace(b"binary_little_endian", b"binary_big_endian")
    open(path, "wb").write(raw)
    with pytest.raises(ValueError, match="binary_big_endian"):
        cloud.read_ply_points(path)
    # a list before the vertices of a binary file cannot be skipped
    head = ["ply", "format binary_little_endian 1.0", "element face 1", "property list uchar int vertex_indices",
            "element vertex 1", "property float x", "property float y", "property float z", "end_header"]
    open(path, "wb").write(("\n".join(head) + "\n").encode() + bytes(13 + 12))
    with pytest.raises(ValueError, match="list"):
        cloud.read_ply_points(path)
    open(path, "wb").write(b"not a ply")
    with pytest.raises(ValueError):
        cloud.read_ply_points(path)


# ------------------------------------------------------------------------------------------------------------ crops
# a non-convex polygon (an arrow head with a notch); its third coordinate is ignored
POLYGON_2D = [(0.0, 0.0), (2.0, 0.0), (2.0, 2.0), (1.0, 0.7), (0.0, 2.0), (-0.5, 1.0)]


def _away_from_edges(points2, margin):
    """the points at least `margin` from every edge of POLYGON_2D (segment distance, float64)"""
    poly = np.array(POLYGON_2D)
    keep = np.ones(len(points2), bool)
    for k in range(len(poly)):
        a, b = poly[k], poly[(k + 1) % len(poly)]
        t = np.clip(((points2 - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
        keep &= np.linalg.norm(points2 - (a + t[:, None] * (b - a)), axis=1) >= margin
    return keep


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_volume_matches_the_float64_restatement(cloud, tmp_path, axis):
    u, v, w = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}[axis]
    polygon = np.zeros((len(POLYGON_2D), 3))
    polygon[:, u], polygon[:, v] = np.array(POLYGON_2D).T
    polygon[:, w] = 123.0                                       # ignored
    path = tmp_path / "crop.json"
    path.write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": axis, "axis_min": -0.25,
                                "axis_max": 0.5, "bounding_polygon": polygon.tolist(), "version_major": 1}))
    vol = cloud.CropVolume.from_json(str(path))
    g = np.random.default_rng(5)
    flat = g.uniform(-1, 2.5, (4000, 2))
    flat = flat[_away_from_edges(flat, 1e-6)]
    pts = np.zeros((len(flat), 3), F32)
    pts[:, u], pts[:, v] = flat[:, 0], flat[:, 1]
    pts[:, w] = g.uniform(-0.6, 0.9, len(flat))
    pts = pts[_away_from_edges(np.stack([pts[:, u], pts[:, v]], 1).astype(np.float64), 1e-6)]   # after the f32 rounding
    want = ref.crop_contains(pts, axis, -0.25, 0.5, polygon)
    got = vol.contains(torch.from_numpy(pts)).numpy()
    assert got.dtype == bool and np.array_equal(got, want)
    assert 0.05 < want.mean() < 0.6
    # hand-checked: inside the notch is outside the polygon
    hand = np.zeros((3, 3), F32)
    hand[:, u], hand[:, v] = [1.0, 1.0, 1.0], [1.5, 0.5, 0.5]
    hand[2, w] = 0.75                                            # beyond axis_max
    assert vol.contains(torch.from_numpy(hand)).tolist() == [False, True, False]
    box = cloud.crop_box(torch.from_numpy(pts), [-1, -1, -1], [0.5, 0.5, 0.5]).numpy()
    assert np.array_equal(box, ((pts >= -1) & (pts <= 0.5)).all(1))
    with pytest.raises(ValueError):
        cloud.CropVolume("W", 0, 1, polygon)


# ----------------------------------------------------------------------------------------------------------- kabsch
def _angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("scale", [1.0, 1.03])
def test_kabsch_gives_back_a_known_similarity(cloud, scale):
    g = np.random.default_rng(11)
    p = g.uniform(-1, 1, (500, 3))
    T = ref.similarity(ref.rotation((1, 2, 3), 25.0), (0.3, -0.2, 0.1), scale)
    q = p @ T[:3, :3].T + T[:3, 3]
    got = cloud.kabsch(ref.exact_sums18(p, q), with_scale=scale != 1.0)
    assert got.dtype == np.float64 and got.shape == (4, 4)
    assert np.abs(got - T).max() <= 1e-12 and np.array_equal(got[3], [0, 0, 0, 1])
    # sums about a centre give the same transform of the uncentred points
    c = np.array([0.5, -1.5, 2.0], F32)
    got = cloud.kabsch(ref.exact_sums18(p - c, q - c), with_scale=scale != 1.0, centre=c)
    assert np.abs(got - T).max() <= 1e-12
    if scale == 1.0:                                              # without with_scale the scale stays 1
        assert abs(np.linalg.det(cloud.kabsch(ref.exact_sums18(p, 1.5 * q))[:3, :3]) - 1) <= 1e-12


def test_kabsch_mirror_and_too_few(cloud):
    g = np.random.default_rng(12)
    p = g.uniform(-1, 1, (200, 3))
    q = p * np.array([1.0, 1.0, -1.0])                            # a reflection: the best ROTATION is wanted
    R = cloud.kabsch(ref.exact_sums18(p, q))[:3, :3]
    assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    with pytest.raises(ValueError, match="3"):
        cloud.kabsch(ref.exact_sums18(p[:2], q[:2]))
    with pytest.raises(ValueError):
        cloud.kabsch(np.zeros(18))
    line = np.outer(np.linspace(0, 1, 10), [1.0, 2.0, 3.0])       # collinear: rank 1
    with pytest.raises(ValueError, match="rotation"):
        cloud.kabsch(ref.exact_sums18(line, line))
    with pytest.raises(ValueError):
        cloud.kabsch(np.zeros(17))


# ------------------------------------------------------------------------------------------- the restatement's ICP
@pytest.mark.parametrize("degrees,shift", [(3.0, 0.02), (5.0, 0.05), (10.0, 0.05)])
def test_restatement_icp_recovers_the_truth_on_the_subset_input(degrees, shift):
    source, target, T_true = ref.subset_problem(degrees=degrees, shift=shift)
    assert source.shape == (5000, 3) and target.shape == (20000, 3)
    assert np.ptp(target, 0).max() == 1.0                        # unit extent
    T, fitness, rmse, iterations = ref.icp_reference(source, target, 0.1)
    print(f"[cloud] reference icp {degrees} deg / {shift}: {iterations} iterations, rmse {rmse:.3g}, "
          f"|t - t_true| {np.abs(T[:3, 3] - T_true[:3, 3]).max():.3g}, angle {_angle(T[:3, :3].T @ T_true[:3, :3]):.3g}")
    assert fitness == 1.0 and iterations < 30
    assert np.abs(T[:3, 3] - T_true[:3, 3]).max() <= 1e-6
    assert np.linalg.norm(T[:3, :3] - T_true[:3, :3]) <= 1e-6
