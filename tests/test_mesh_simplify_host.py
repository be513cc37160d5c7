"""Mesh simplification without a GPU: properties of the numpy restatement of tests/mesh_simplify_reference.py (cluster
and face order, degenerate and duplicate counts, vertices inside their cells, the target_faces search, the wedge that
motivates quadric placement), the M3 C ABI contract (no launch) and the tool's new options."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_simplify_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "extract_mesh.py")

# cells at cell = 1 from the origin: (0,0,0) (2,0,0) (0,0,0) (0,1,0) (2,0,0) (0,1,0) (5,5,5) (7,0,0)
HAND_VERTS = np.array([[0.1, 0.1, 0.1], [2.5, 0.1, 0.1], [0.2, 0.3, 0.1], [0.1, 1.5, 0.2], [2.7, 0.2, 0.3],
                       [0.3, 1.2, 0.9], [5.5, 5.5, 5.5], [7.5, 0.5, 0.5]], np.float32)
HAND_CLUSTER = [0, 1, 0, 2, 1, 2, 3, 4]
# kept, degenerate, duplicate (permuted), duplicate (reversed), degenerate, degenerate, kept
HAND_FACES = np.array([[0, 1, 3], [0, 2, 1], [4, 5, 2], [3, 1, 0], [6, 6, 0], [0, 0, 6], [7, 3, 1]], np.int32)


def test_cluster_and_face_order_on_a_hand_made_mesh():
    keys = ref.cell_keys(HAND_VERTS, (0, 0, 0), 1.0)
    assert keys.tolist() == [[0, 0, 0], [2, 0, 0], [0, 0, 0], [0, 1, 0], [2, 0, 0], [0, 1, 0], [5, 5, 5], [7, 0, 0]]
    cluster, n = ref.clusters(keys)
    assert n == 5 and cluster.tolist() == HAND_CLUSTER          # numbered by their smallest member
    c, kept, deg, dup = ref.face_pass(HAND_FACES, cluster)
    assert kept.tolist() == [True, False, False, False, False, False, True] and (deg, dup) == (3, 2)
    assert ref.count(HAND_VERTS, HAND_FACES, 1.0, (0, 0, 0)) == (5, 2, 3, 2)
    cols = (np.arange(24).reshape(8, 3) * 10).astype(np.uint8)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (8, 1))
    nrm[2] = (0, 0, -1)                                          # cluster 0: the mean vanishes
    out = ref.simplify(HAND_VERTS, HAND_FACES, cell=1.0, origin=(0, 0, 0), placement="mean", normals=nrm, colors=cols)
    # cluster 3 (vertex 6) is used by no kept face: it goes and cluster 4 moves up; order and winding stay
    assert out["faces"].tolist() == [[0, 1, 2], [3, 2, 1]] and out["faces"].dtype == np.int32
    assert out["vertex_map"].tolist() == [0, 1, 0, 2, 1, 2, -1, 3]
    want = np.stack([HAND_VERTS[[0, 2]].astype(np.float64).mean(0), HAND_VERTS[[1, 4]].astype(np.float64).mean(0),
                     HAND_VERTS[[3, 5]].astype(np.float64).mean(0), HAND_VERTS[7]]).astype(np.float32)
    assert np.array_equal(out["verts"], want)
    assert out["normals"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]]
    assert out["colors"].tolist() == [[30, 40, 50], [75, 85, 95], [120, 130, 140], [210, 220, 230]]
    s = out["stats"]
    assert (s["clusters"], s["V_in"], s["V_out"], s["F_in"], s["F_out"], s["degenerate"], s["duplicate"]) == \
           (5, 8, 4, 7, 2, 3, 2)


def test_colour_rounding_is_floor_of_mean_plus_half():
    verts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.5, 0.1, 0.1], [0.1, 1.5, 0.1]], np.float32)
    cols = np.array([[0, 1, 255], [1, 2, 254], [9, 9, 9], [7, 7, 7]], np.uint8)
    out = ref.simplify(verts, np.array([[0, 2, 3], [1, 2, 3]], np.int32), cell=1.0, origin=(0, 0, 0), colors=cols)
    assert out["colors"].tolist() == [[1, 2, 255], [9, 9, 9], [7, 7, 7]]      # 0.5 -> 1, 1.5 -> 2, 254.5 -> 255
    assert out["faces"].tolist() == [[0, 1, 2]] and out["stats"]["duplicate"] == 1


def test_keys_on_cell_faces_and_bad_keys():
    # a vertex exactly on a cell face belongs to the upper cell; float32 arithmetic decides, as in the kernel
    v = np.array([[1.0, 2.0, 3.0], [0.99999994, 1.9999999, 2.9999998]], np.float32)
    assert ref.cell_keys(v, (0, 0, 0), 1.0).tolist() == [[1, 2, 3], [0, 1, 2]]
    third = np.float32(1) / np.float32(3)
    want = np.floor(np.float32(np.float32(7) - np.float32(1)) * (np.float32(1) / third))
    assert ref.cell_keys(np.array([[7, 7, 7]], np.float32), (1, 1, 1), third)[0, 0] == int(want)
    for bad in ([[np.nan, 0, 0]], [[np.inf, 0, 0]], [[-0.5, 0, 0]], [[2.0 ** 21, 0, 0]]):
        with pytest.raises(ValueError):
            ref.cell_keys(np.array(bad, np.float32), (0, 0, 0), 1.0)
    assert ref.cell_keys(np.array([[2.0 ** 21 - 1, 0, 0]], np.float32), (0, 0, 0), 1.0)[0, 0] == 2 ** 21 - 1
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            ref.cell_keys(np.zeros((1, 3), np.float32), (0, 0, 0), cell)


def _inside_cells(verts, out, origin, cell):
    """every output vertex lies in the cell of the input vertices mapped to it (up to its float32 rounding)"""
    keys = ref.cell_keys(verts, origin, cell).astype(np.float64)
    m = out["vertex_map"]
    live = m >= 0
    x = out["verts"][m[live]].astype(np.float64)
    o = np.asarray(origin, np.float32).astype(np.float64)
    c = float(np.float32(cell))
    slack = 2.0 ** -22 * (np.abs(x) + np.abs(o))    # the key's two float32 roundings of v - o, and the output's own
    return ((x >= o + keys[live] * c - slack) & (x <= o + (keys[live] + 1) * c + slack)).all()


@pytest.mark.parametrize("seed", range(3))
def test_soup_vertices_stay_inside_their_cells(seed):
    verts, faces = ref.soup(seed)
    origin = verts.min(0)
    cell = np.float32((verts.max(0) - origin).max() / 10)
    for placement in ("quadric", "mean"):
        out = ref.simplify(verts, faces, cell=cell, placement=placement)
        s = out["stats"]
        assert s["degenerate"] > 0 and s["duplicate"] > 0 and 0 < s["F_out"] < s["F_in"]
        assert s["F_out"] + s["degenerate"] + s["duplicate"] == s["F_in"]
        assert s["V_out"] == len(out["verts"]) <= s["clusters"] and s["F_out"] == len(out["faces"])
        assert _inside_cells(verts, out, origin, cell)
        f = out["faces"]
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert len(np.unique(np.sort(f, 1), axis=0)) == len(f)
        assert np.array_equal(np.unique(f), np.arange(s["V_out"]))          # every output vertex is used
        d = np.linalg.norm(verts.astype(np.float64) - out["verts"][out["vertex_map"]].astype(np.float64), axis=1)
        assert d[out["vertex_map"] >= 0].max() <= math.sqrt(3) * float(cell) * (1 + 2.0 ** -20)


@pytest.mark.parametrize("cell", [0.05, 0.11])
def test_wedge_quadric_keeps_the_crease_and_the_planes(cell):
    """two sheets at 90 degrees: every output vertex of 'quadric' is at most a quarter as far from the nearer plane
    as the worst of 'mean' (which pulls the crease's cells into the corner)"""
    verts, faces, R, t = ref.wedge()
    worst = {}
    for placement in ("quadric", "mean"):
        out = ref.simplify(verts, faces, cell=cell, placement=placement)
        assert _inside_cells(verts, out, verts.min(0), cell)
        worst[placement] = ref.plane_distance(out["verts"], R, t).max() / cell
    print(f"[wedge host] cell {cell}: quadric {worst['quadric']:.4f} mean {worst['mean']:.4f} cells")
    assert worst["mean"] > 0.05
    assert worst["quadric"] <= worst["mean"] / 4


def _uv_sphere(n_lat=48, n_lon=96):
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones_like(ph))], -1).reshape(-1, 3)
    verts = np.concatenate([ring, [[0, 0, 1]], [[0, 0, -1]]]).astype(np.float32)
    idx = np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    a, b = idx[:-1], idx[1:]
    ar, br = np.roll(a, -1, 1), np.roll(b, -1, 1)
    faces = [np.stack([a, b, br], -1).reshape(-1, 3), np.stack([a, br, ar], -1).reshape(-1, 3)]
    top, bot = len(ring), len(ring) + 1
    faces.append(np.stack([np.full(n_lon, top), idx[0], np.roll(idx[0], -1)], 1))
    faces.append(np.stack([np.full(n_lon, bot), np.roll(idx[-1], -1), idx[-1]], 1))
    return verts, np.concatenate(faces).astype(np.int32)


@pytest.mark.parametrize("target", [0, 100, 1000, 5000])
def test_target_faces_search(target):
    verts, faces = _uv_sphere()
    out = ref.simplify(verts, faces, target_faces=target)
    s = out["stats"]
    k = s["k"]
    assert s["F_out"] == len(out["faces"]) <= target and k >= 1
    extent = float((verts.max(0) - verts.min(0)).max())
    assert s["cell"] == float(np.float32(extent / k))
    assert ref.count(verts, faces, np.float32(extent / (k + 1)), verts.min(0))[1] > target
    assert s["probes"] <= 2 * math.ceil(math.log2(k)) + 2
    # a mesh that is small enough comes back as it is
    same = ref.simplify(verts, faces, target_faces=len(faces))
    assert np.shares_memory(same["verts"], verts) and np.array_equal(same["faces"], faces)
    assert same["stats"]["probes"] == 0 and same["stats"]["F_out"] == len(faces)


def test_one_cell_and_empty_meshes():
    verts, faces = ref.soup(7, 50, 80)
    out = ref.simplify(verts, faces, cell=1000.0)
    assert out["verts"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert out["stats"]["clusters"] == 1 and out["stats"]["degenerate"] == len(faces)
    out = ref.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), cell=1.0)
    assert out["verts"].shape == (0, 3) and out["stats"]["V_out"] == 0
    one = ref.simplify(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32), cell=0.5)
    assert one["faces"].tolist() == [[0, 1, 2]] and one["stats"]["clusters"] == 3


def test_m3_c_abi_contract_without_launch(ngp):
    lib = ngp._lib.load()
    ws = lib.ngp_mesh_simplify_workspace
    assert ws(0, 0) >= 0 and ws(1000, 300) >= 3 * 2048 + 2 * 1024 + 3 * 1000 + 2 * 300
    assert ws(-1, 5) == -22 and ws(5, -1) == -22 and ws(2 ** 28 + 1, 5) == -22 and ws(5, 2 ** 28 + 1) == -22
    assert ws(2 ** 28, 2 ** 28) > 2 ** 31                  # an int64 element count
    buf = C.c_void_p(16)    # never dereferenced: every call below must return before a launch
    o3 = (C.c_float * 3)(0, 0, 0)
    count = lambda a: lib.ngp_mesh_simplify_count(*a)
    groups = lambda a: lib.ngp_mesh_simplify_groups(*a)
    place = lambda a: lib.ngp_mesh_simplify_place(*a)
    emit = lambda a: lib.ngp_mesh_simplify_faces(*a)
    count_args = [buf, 5, buf, 5, o3, 1.0, buf, buf, None]
    groups_args = [buf, 5, 5, buf, buf, buf, None]
    place_args = [buf, 5, buf, 5, o3, 1.0, 1.0, 1e-3, 1, 3, buf, buf, buf, buf, buf, buf, buf, buf, buf, None]
    emit_args = [buf, 5, 5, buf, buf, buf, None]
    # empty inputs: NGP_OK before any pointer is looked at
    assert count([None, 0, None, 7, None, 1.0, None, None, None]) == 0
    assert groups([None, 7, 0, None, None, None, None]) == 0
    assert place([None, 0, None, 7, None, 1.0, 1.0, 1e-3, 1, 0] + [None] * 10) == 0
    assert place([None, 5, None, 7, None, 1.0, 1.0, 1e-3, 1, 0] + [None] * 10) == 0       # no cluster to write
    for nv, nf in ((0, 7), (7, 0), (0, 0)):
        assert emit([None, nf, nv, None, None, None, None]) == 0
    # negative or oversized sizes
    for nv, nf in ((-1, 5), (5, -1), (2 ** 28 + 1, 5)):
        assert count([buf, nv, buf, nf, o3, 1.0, buf, buf, None]) == -22
        assert groups([buf, nf, nv, buf, buf, buf, None]) == -22
        a = list(place_args)
        a[1], a[3] = nv, nf
        assert place(a) == -22
        assert emit([buf, nf, nv, buf, buf, buf, None]) == -22
    for n_clusters in (-1, 6):                                                            # more clusters than vertices
        a = list(place_args)
        a[9] = n_clusters
        assert place(a) == -22
    # a NULL in any pointer position of a non-empty input
    for fn, args, ptrs in ((count, count_args, (0, 2, 4, 6, 7)), (groups, groups_args, (0, 3, 4, 5)),
                           (place, place_args, (0, 2, 4, 10, 11, 12, 13, 16)), (emit, emit_args, (0, 3, 4, 5))):
        for i in ptrs:
            a = list(args)
            a[i] = None
            assert fn(a) == -22, (args is count_args, i)
    for i, out in ((14, 17), (15, 18)):                     # an attribute without its output
        a = list(place_args)
        a[out] = None
        assert place(a) == -22
        a[i] = None                                          # neither: fine as far as the pointers go
    # cell sizes and regularisation that cannot be used
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        a = list(count_args)
        a[5] = inv
        assert count(a) == -22
        a = list(place_args)
        a[6] = inv
        assert place(a) == -22
    for reg in (0.0, -1e-3, float("nan")):
        a = list(place_args)
        a[7] = reg
        assert place(a) == -22
    a = list(count_args)
    a[6] = C.c_void_p(20)                                    # the workspace holds 64-bit keys: 8-byte aligned
    assert count(a) == -22


def test_tool_names_and_checks_the_simplification_options():
    run = lambda *a: subprocess.run([sys.executable, TOOL, *a], capture_output=True, text=True, timeout=300)
    out = run("--help")
    assert out.returncode == 0, out.stderr
    for opt in ("--simplify_cell X", "--target_faces N", "--placement {quadric,mean}"):
        assert opt in out.stdout, opt
    base = ("--ckpt", "none.ckpt", "--out", "none.ply")
    for flags, msg in ((("--simplify_cell", "0.1", "--target_faces", "100"), "not allowed with"),
                       (("--simplify_cell", "0"), "--simplify_cell must be positive"),
                       (("--target_faces", "-1"), "--target_faces must be >= 0"),
                       (("--placement", "median"), "invalid choice")):
        out = run(*base, *flags)
        assert out.returncode == 2 and msg in out.stderr, (flags, out.stderr[-500:])
