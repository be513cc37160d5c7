"""Mesh evaluation without a GPU: the float32 restatement of the closest-point sequence against float64 and against
hand cases, the sampler's restatement, the reductions of mesh_distance on hand-made distances, and the edges of the
C ABI that must not reach a launch (tests/mesh_eval_reference.py; include/ngp_hip.h M4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_eval_reference as ref

F32, F64 = np.float32, np.float64


def _random_cases(seed, n):
    """points and triangles in [-1, 1]^3; the triangles' sizes spread log-uniformly over 1e-3 .. 1"""
    g = np.random.default_rng(seed)
    size = 10.0 ** g.uniform(-3, 0, (n, 1, 1))
    centre = g.uniform(-1 + size, 1 - size, (n, 1, 3))
    tri = (centre + size * g.uniform(-1, 1, (n, 3, 3))).astype(F32)
    # half of the points anywhere in the box, half within two sizes of the triangle (every region, near its borders)
    near = np.clip(centre[:, 0] + 2 * size[:, 0] * g.uniform(-1, 1, (n, 3)), -1, 1)
    p = np.where(g.random((n, 1)) < 0.5, g.uniform(-1, 1, (n, 3)), near).astype(F32)
    return p, tri[:, 0], tri[:, 1], tri[:, 2]


def _f32_against_f64(seed, n):
    p, a, b, c = _random_cases(seed, n)
    d32, r32 = ref.tri_d2(p, a, b, c)
    d64, r64 = ref.tri_d2(*(x.astype(F64) for x in (p, a, b, c)))
    err = np.abs(np.sqrt(d32.astype(F64)) - np.sqrt(d64))
    return err.max(), int((r32 != r64).sum()), np.bincount(r64, minlength=7)


def test_f32_sequence_against_float64():
    """distances (square roots of the two d2) for coordinates in [-1, 1].  Measured with this restatement over 2 000 000
    cases (seeds 0-9, 200 000 each): worst |dist32 - dist64| = 2.09 * 2^-23 (seed 3; seed 0, which runs here, gives
    1.80; the prototype quoted with the feature request gave 1.9 * 2^-23), and no case where the two precisions pick
    different regions.  The bound asserted is 4 x that worst case, 8.36 * 2^-23, times the largest coordinate
    magnitude, 1."""
    worst, disagree, regions = _f32_against_f64(0, 200_000)
    print(f"[mesh eval] f32 vs f64: worst {worst / 2.0 ** -23:.3f} * 2^-23, region disagreements {disagree}, "
          f"cases per region {regions.tolist()}")
    assert regions.min() > 1000                      # every region is exercised
    assert worst <= 4 * MEASURED_WORST * 2.0 ** -23 * 1.0


MEASURED_WORST = 2.09      # in units of 2^-23: see test_f32_sequence_against_float64


# ------------------------------------------------------------------------------------------------------ hand cases
A, B, CC, HAND = ref.HAND_A, ref.HAND_B, ref.HAND_C, ref.HAND_CASES


@pytest.mark.parametrize("dtype", [F32, F64])
def test_hand_cases_on_one_triangle(dtype):
    a, b, c = (np.array(x, dtype) for x in (A, B, CC))
    for point, want, region in HAND:
        d, r = ref.tri_d2(np.array(point, dtype), a, b, c)
        assert d == dtype(want), (point, d, want)
        assert ref.REGIONS[int(r)] == region, (point, ref.REGIONS[int(r)], region)
    # the brute force over a mesh of this triangle, a collinear face and a face with a repeated vertex
    verts = np.array([A, B, CC, (1.0, 0.0, 0.0), (5.0, 5.0, 5.0)], F32)
    faces = np.array([[0, 3, 1], [4, 4, 2], [0, 1, 2]], np.int32)
    assert ref.nondegenerate(verts, faces).tolist() == [False, False, True]
    pts = np.array([h[0] for h in HAND] + [(5.0, 5.0, 5.0)], F32)
    d2, face = ref.closest_brute(pts, verts, faces, 3.0, dtype)
    for k, (point, want, _) in enumerate(HAND):
        assert (d2[k], face[k]) == ((want, 2) if want <= 9.0 else (9.0, -1)), point      # 9 = max_dist^2 is kept
    assert (d2[-1], face[-1]) == (9.0, -1)        # the degenerate face at the point itself does not count
    # ties go to the smaller index, NaN never wins
    two = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    assert ref.closest_brute(pts[:3], verts, two, 10.0, dtype)[1].tolist() == [0, 0, 0]
    bad = verts.copy()
    bad[4] = np.nan
    d2, face = ref.closest_brute(pts[:3], bad, np.array([[0, 1, 4], [0, 1, 2]], np.int32), 10.0, dtype)
    assert face.tolist() == [1, 1, 1] and d2.tolist() == [9.0, 0.0, 1.0]
    d2, face = ref.closest_brute(pts[:3], bad, np.array([[0, 1, 4]], np.int32), 10.0, dtype)
    assert face.tolist() == [-1] * 3 and d2.tolist() == [100.0] * 3
    d2, face = ref.closest_brute(pts[:3], verts, faces[:0], 2.0, dtype)
    assert face.tolist() == [-1] * 3 and d2.tolist() == [4.0] * 3


# ---------------------------------------------------------------------------------------------------------- sampler
def test_fmix32_known_answers():
    """by hand, the five steps mod 2^32 (h ^= h >> 16, h *= 0x85ebca6b, h ^= h >> 13, h *= 0xc2b2ae35, h ^= h >> 16):
       0          -> 0 at every step
       1          -> 1 -> 0x85ebca6b -> 0x85efe535 -> 0x514e79f9 -> 0x514e28b7
       0xffffffff -> 0xffff0000 -> 0x35950000 -> 0x3594aca8 -> 0x81f1eec8 -> 0x81f16f39"""
    def steps(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B % 2 ** 32
        h ^= h >> 13
        h = h * 0xC2B2AE35 % 2 ** 32
        return h ^ h >> 16
    assert steps(1) == 0x514E28B7 and steps(0xFFFFFFFF) == 0x81F16F39 and steps(0) == 0
    assert ref.fmix32(np.array([0, 1, 0xFFFFFFFF], np.uint64)).tolist() == [0, 0x514E28B7, 0x81F16F39]


def test_sampler_restatement():
    verts, faces = ref.mesh_with_dead_faces()
    cdf = ref.area_cdf(verts, faces)
    dead = np.nonzero(np.diff(np.concatenate([[0.0], cdf])) == 0)[0]
    assert set(dead) == {0, 17, 23, 39}
    n = 20_000
    pts, face = ref.sample_surface(verts, faces, cdf, n, seed=3)
    assert pts.dtype == F32 and face.dtype == np.int32 and pts.shape == (n, 3)
    assert not np.isin(face, dead).any() and face.min() >= 1 and face.max() <= 38
    # every sample lies in its face: barycentric coordinates >= 0 and summing to 1 within float32 rounding of
    # coordinates of magnitude <= 1.2 (a few ulp, relative to a face of edge ~0.2: 1e-5)
    bary = ref.barycentric(pts, verts, faces, face)
    assert bary.min() >= -1e-5 and np.abs(bary.sum(1) - 1).max() <= 1e-12
    # area-weighted: the share of each live face is its share of the area (n = 20 000: 5 sigma of a binomial)
    share = np.bincount(face, minlength=40) / n
    want = np.diff(np.concatenate([[0.0], cdf])) / cdf[-1]
    assert (np.abs(share - want) <= 5 * np.sqrt(want * (1 - want) / n) + 1e-9).all()
    # a function of (seed, i): a prefix of a longer run, another seed differs
    again, _ = ref.sample_surface(verts, faces, cdf, 100, seed=3)
    other, _ = ref.sample_surface(verts, faces, cdf, 100, seed=4)
    assert np.array_equal(again, pts[:100]) and not np.array_equal(other, pts[:100])
    # one face
    one = np.array([[0, 1, 2]], np.int32)
    pts, face = ref.sample_surface(verts[3:6], one, ref.area_cdf(verts[3:6], one), 50, 0)
    assert (face == 0).all() and ref.barycentric(pts, verts[3:6], one, face).min() >= -1e-5


# ---------------------------------------------------------------------------------------------------------- metrics
def test_metric_arithmetic_with_stubbed_queries(ngp, monkeypatch):
    mesh = ngp.mesh
    d_ab = torch.tensor([0.0, 0.1, 0.2, 0.5], dtype=torch.float32)          # A's samples to B
    d_ba = torch.tensor([0.3, 0.3, 0.1, 0.9], dtype=torch.float32)          # B's samples to A
    f_ab = torch.tensor([0, 1, 1, -1], dtype=torch.int32)
    f_ba = torch.tensor([2, 2, 0, 5], dtype=torch.int32)
    va, vb = torch.zeros(3, 3), torch.ones(3, 3)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    seeds = []

    def fake_sample(verts, faces, n, seed=0, cdf=None):
        seeds.append(seed)
        return verts[:1].expand(n, 3).contiguous(), torch.zeros(n, dtype=torch.int32)

    def fake_closest(points, verts, faces, max_dist=None, cell=None, stats=None):
        return (d_ab, f_ab) if bool((verts == 1).all()) else (d_ba, f_ba)     # the target mesh says which direction

    monkeypatch.setattr(mesh, "sample_surface", fake_sample)
    monkeypatch.setattr(mesh, "closest_on_mesh", fake_closest)
    out = mesh.mesh_distance(va, faces, vb, faces, n_samples=4, thresholds=(0.2, 0.05, 0.001, 1.0), seed=7)
    assert seeds == [7, 8]
    f32 = lambda xs: [float(np.float32(x)) for x in xs]                      # noqa: E731
    acc, comp = np.mean(f32([0.0, 0.1, 0.2, 0.5])), np.mean(f32([0.3, 0.3, 0.1, 0.9]))
    assert out["accuracy"] == pytest.approx(acc, abs=1e-15) and out["completeness"] == pytest.approx(comp, abs=1e-15)
    assert out["chamfer"] == pytest.approx((acc + comp) / 2, abs=1e-15)
    assert out["hausdorff"] == float(np.float32(0.9))
    assert out["clipped_a"] == 0.25 and out["clipped_b"] == 0.0
    assert out["thresholds"] == [0.2, 0.05, 0.001, 1.0]
    # 0.2 as float32 is above 0.2, so it is NOT within the threshold 0.2: the comparison is made in float64
    assert out["precision"] == [0.5, 0.25, 0.25, 1.0] and out["recall"] == [0.25, 0.0, 0.0, 1.0]
    assert out["fscore"][0] == pytest.approx(2 * 0.5 * 0.25 / 0.75, abs=1e-15)
    assert out["fscore"][1] == 0.0 and out["fscore"][3] == 1.0
    # P + R = 0
    d_ab += 1.0
    out = mesh.mesh_distance(va, faces, vb, faces, n_samples=4, thresholds=(0.05,))
    assert out["precision"] == [0.0] and out["recall"] == [0.0] and out["fscore"] == [0.0]
    with pytest.raises(ValueError):
        mesh.mesh_distance(va, faces, vb, faces, n_samples=0)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_edges_reach_no_launch(ngp):
    """n == 0 is NGP_OK with every pointer NULL; a NULL pointer or a bad size with n > 0 is NGP_EINVAL before any
    launch (there is no GPU here: a launch would not return NGP_EINVAL)."""
    lib = ngp._lib.load()
    OK, EINVAL = 0, -22
    buf = (C.c_double * 64)()                      # host memory standing in for device pointers: never dereferenced
    ptr = C.addressof(buf)
    origin, dims = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    assert lib.ngp_mesh_sample_surface(None, 0, None, 0, None, 0.0, 0, 0, None, None, None) == OK
    assert lib.ngp_mesh_closest(None, 0, None, 0, None, 0, None, 0.0, None, None, None, -1.0, None, None, None) == OK
    assert lib.ngp_mesh_grid_count(None, 0, None, 0, None, 0.0, None, None, None, None) == OK
    assert lib.ngp_mesh_grid_fill(None, 0, None, 0, None, 0.0, None, None, None, None, None) == OK

    sample = [ptr, 3, ptr, 1, ptr, 1.0, 5, 0, ptr, ptr, None]
    for k in (0, 2, 4, 8, 9):                      # each pointer in turn
        assert lib.ngp_mesh_sample_surface(*[None if j == k else a for j, a in enumerate(sample)]) == EINVAL, k
    for total in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ngp_mesh_sample_surface(*[total if j == 5 else a for j, a in enumerate(sample)]) == EINVAL
    assert lib.ngp_mesh_sample_surface(*[-1 if j == 6 else a for j, a in enumerate(sample)]) == EINVAL
    assert lib.ngp_mesh_sample_surface(*[2 ** 30 + 1 if j == 6 else a for j, a in enumerate(sample)]) == EINVAL
    assert lib.ngp_mesh_sample_surface(*[0 if j == 3 else a for j, a in enumerate(sample)]) == EINVAL   # no face

    closest = [ptr, 5, ptr, 3, ptr, 1, origin, 1.0, dims, ptr, ptr, 1.0, ptr, ptr, None]
    for k in (0, 2, 4, 6, 8, 9, 10, 12, 13):
        assert lib.ngp_mesh_closest(*[None if j == k else a for j, a in enumerate(closest)]) == EINVAL, k
    for k, bad in ((1, -1), (5, -1), (7, 0.0), (7, float("inf")), (11, -1.0), (11, float("nan"))):
        assert lib.ngp_mesh_closest(*[bad if j == k else a for j, a in enumerate(closest)]) == EINVAL, (k, bad)
    for bad_dims in ((0, 4, 4), (4, 1025, 4), (1024, 1024, 17)):
        d = (C.c_int32 * 3)(*bad_dims)
        assert lib.ngp_mesh_closest(*[d if j == 8 else a for j, a in enumerate(closest)]) == EINVAL, bad_dims
    # with no face the grid is not looked at, but the outputs are
    assert lib.ngp_mesh_closest(ptr, 5, None, 0, None, 0, None, 0.0, None, None, None, 1.0, None, ptr, None) == EINVAL

    count = [ptr, 3, ptr, 1, origin, 1.0, dims, ptr, ptr, None]
    for k in (0, 2, 4, 6, 7, 8):
        assert lib.ngp_mesh_grid_count(*[None if j == k else a for j, a in enumerate(count)]) == EINVAL, k
    fill = [ptr, 3, ptr, 1, origin, 1.0, dims, ptr, ptr, ptr, None]
    for k in (0, 2, 4, 6, 7, 8, 9):
        assert lib.ngp_mesh_grid_fill(*[None if j == k else a for j, a in enumerate(fill)]) == EINVAL, k
    assert lib.ngp_mesh_grid_count(*[-1 if j == 3 else a for j, a in enumerate(count)]) == EINVAL


def test_python_checks_refuse_before_the_library(ngp):
    """CPU tensors, wrong dtypes and shapes are refused by mesh.py's own checks"""
    mesh = ngp.mesh
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for fn in (lambda: mesh.sample_surface(v, f, 4), lambda: mesh.closest_on_mesh(v, v, f),
               lambda: mesh.face_area_cdf(v, f)):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn()
