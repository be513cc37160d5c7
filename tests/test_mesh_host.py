"""CPU checks of mesh export: the marching-cubes case table of libngp_hip.so (ngp_mc_tables), a numpy restatement of
the two kernel passes with that table on many random volumes (closed, positively oriented surfaces), the C-ABI
contract of the ngp_mc_* entry points without a launch, the PLY writer / reader, and no CPU fallback."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mesh_reference import (corner_offset, is_closed_oriented, marching_cubes, mc_counts, mc_tables, n_components,
                            signed_volume)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(ngp):
    return mc_tables(ngp)


def _faces_of_cube():
    """(axis, side, corners in cyclic order) of the 6 cube faces"""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in range(2):
            cyc = []
            for ub, uc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                o = [0, 0, 0]
                o[a], o[b], o[c] = s, ub, uc
                cyc.append(o[0] | o[1] << 1 | o[2] << 2)
            out.append(cyc)
    return out


def test_table_edges_and_empty_cases(tables):
    tri, cnt, ec = tables
    # the edge numbering documented in include/ngp_hip.h: the corners of an edge differ on exactly its axis
    for e in range(12):
        d = corner_offset(int(ec[e, 1])) - corner_offset(int(ec[e, 0]))
        assert d.tolist() == [int(i == e >> 2) for i in range(3)], e
    assert cnt[0] == 0 and cnt[255] == 0 and (tri[0] == -1).all() and (tri[255] == -1).all()
    for cs in range(256):
        n = int(cnt[cs])
        assert 0 <= n <= 5 and (tri[cs, 3 * n:] == -1).all() and (tri[cs, :3 * n] >= 0).all(), cs
        inside = [(cs >> c) & 1 for c in range(8)]
        crossing = {e for e in range(12) if inside[ec[e, 0]] != inside[ec[e, 1]]}
        used = set(tri[cs, :3 * n].tolist())
        assert used == crossing, (cs, used, crossing)
        t = tri[cs, :3 * n].reshape(-1, 3)
        assert all(len(set(r)) == 3 for r in t.tolist()), cs


def test_table_face_rule_inside_corners_separated(tables):
    """the triangles' boundary segments on each cube face pair that face's crossing edges as the face-local rule says:
    two crossing edges are paired; four (inside corners diagonal) are paired around each inside corner"""
    tri, cnt, ec = tables
    edge_of = {frozenset((int(a), int(b))): e for e, (a, b) in enumerate(ec)}
    faces = _faces_of_cube()
    for cs in range(256):
        inside = [(cs >> c) & 1 for c in range(8)]
        t = tri[cs, :3 * cnt[cs]].reshape(-1, 3).tolist()
        seg = {}
        for a, b, c in t:
            for u, v in ((a, b), (b, c), (c, a)):
                seg[(u, v)] = seg.get((u, v), 0) + 1
        boundary = set()
        for (u, v), k in seg.items():
            assert k == 1, (cs, u, v)
            if (v, u) not in seg:
                boundary.add(frozenset((u, v)))
        got_total = set()
        for cyc in faces:
            fe = [edge_of[frozenset((cyc[q], cyc[(q + 1) % 4]))] for q in range(4)]
            crossing = [fe[q] for q in range(4) if inside[cyc[q]] != inside[cyc[(q + 1) % 4]]]
            if len(crossing) == 2:
                want = {frozenset(crossing)}
            elif len(crossing) == 4:
                want = {frozenset((fe[(q + 3) % 4], fe[q])) for q in range(4) if inside[cyc[q]]}
            else:
                want = set()
            got = {s for s in boundary if s <= set(fe)}
            assert got == want, (cs, cyc, got, want)
            got_total |= got
        assert got_total == boundary, cs     # every boundary segment lies on a face
        # the fan's chords (edges inside the cell) lie on no face: the neighbouring cell could draw the same chord
        for u, v in seg:
            if (v, u) in seg:
                shared = [cyc for cyc in faces if {*ec[u], *ec[v]} <= set(cyc)]
                assert not shared, (cs, u, v)


def _random_volume(g, shape):
    kind = g.integers(3)
    if kind == 0:      # white noise: every ambiguous configuration occurs
        v = g.random(shape, dtype=np.float32)
    elif kind == 1:    # blobs: a few Gaussians
        x = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij"), -1)
        v = np.zeros(shape, np.float32)
        for _ in range(g.integers(1, 5)):
            c = g.random(3) * (np.array(shape) - 1)
            v += np.exp(-((x - c) ** 2).sum(-1) / (2 * (0.5 + 2 * g.random()) ** 2)).astype(np.float32)
    else:              # coarse noise with exact-level plateaus
        v = np.round(g.random(shape, dtype=np.float32) * 4) / 4
    v = v.astype(np.float32)
    level = np.float32(0.5)
    v[[0, -1]] = v[:, [0, -1]] = 0      # border outside: every surface is closed
    v[:, :, [0, -1]] = 0
    return v, level


def test_restatement_closed_and_positively_oriented(tables):
    """>= 1000 seeded random volumes (6^3 - 10^3, border outside): the restated passes give closed, consistently
    oriented surfaces (every edge in two faces, opposite directions) whose signed volume is positive"""
    g = np.random.default_rng(20220806)
    n_nonempty = 0
    for it in range(1000):
        shape = tuple(int(s) for s in g.integers(6, 11, 3))
        vol, level = _random_volume(g, shape)
        verts, faces = marching_cubes(vol, level, tables)
        assert (len(verts), len(faces)) == mc_counts(vol, level, tables)
        if len(faces) == 0:
            continue
        n_nonempty += 1
        assert faces.min() >= 0 and faces.max() < len(verts)
        assert np.unique(faces).size == len(verts), it          # no unused vertex
        assert is_closed_oriented(faces, len(verts)), (it, shape)
        assert signed_volume(verts, faces) > 0, (it, shape)
    assert n_nonempty > 900


def test_restatement_single_inside_point(tables):
    """hand-checkable: one inside lattice point gives a closed octahedron of 8 triangles around it with vertices
    half-way along its 6 edges"""
    vol = np.zeros((3, 3, 3), np.float32)
    vol[1, 1, 1] = 2.0
    verts, faces = marching_cubes(vol, 1.0, tables, spacing=(0.5, 0.5, 0.5), origin=(-0.5, -0.5, -0.5))
    assert verts.shape == (6, 3) and faces.shape == (8, 3)
    assert sorted(map(tuple, verts.tolist())) == sorted([(-0.25, 0, 0), (0.25, 0, 0), (0, -0.25, 0), (0, 0.25, 0),
                                                          (0, 0, -0.25), (0, 0, 0.25)])
    assert is_closed_oriented(faces, 6) and n_components(faces, 6) == 1
    assert abs(signed_volume(verts, faces) - 4 / 3 * 0.25 ** 3) < 1e-9    # the octahedron's volume
    # the vertex on the x edge from (0,1,1) comes first: point-major order, x < y < z
    assert verts[0].tolist() == [-0.25, 0.0, 0.0]


def test_mc_c_abi_contract_without_launch(ngp):
    lib = ngp._lib.load()
    assert lib.ngp_mc_workspace(0, 5, 5) == 0 and lib.ngp_mc_workspace(5, 1, 5) == 0
    assert lib.ngp_mc_workspace(-1, 5, 5) == -22 and lib.ngp_mc_workspace(2048, 2048, 512) == -22
    n = 5 * 6 * 7
    assert lib.ngp_mc_workspace(5, 6, 7) >= n
    for dims in ((0, 5, 5), (5, 5, 1), (1, 1, 1), (0, 0, 0)):           # empty: OK before any pointer is looked at
        assert lib.ngp_mc_count(None, *dims, 1.0, None, None, None) == 0, dims
        assert lib.ngp_mc_emit(None, *dims, 1.0, None, None, None, None, None, None) == 0, dims
    host3 = (C.c_float * 3)(0, 0, 0)
    buf = C.c_void_p(16)   # never dereferenced: every call below must fail its argument checks first
    for dims in ((-1, 5, 5), (5, -1, 5), (5, 5, -2), (2048, 2048, 512), (1 << 16, 1 << 16, 2)):
        assert lib.ngp_mc_count(buf, *dims, 1.0, buf, buf, None) == -22, dims
        assert lib.ngp_mc_emit(buf, *dims, 1.0, host3, host3, buf, buf, buf, None) == -22, dims
    # a NULL in any pointer position of a non-empty lattice
    count_args = [buf, 5, 6, 7, 1.0, buf, buf, None]
    for i in (0, 5, 6):
        a = list(count_args)
        a[i] = None
        assert lib.ngp_mc_count(*a) == -22, i
    emit_args = [buf, 5, 6, 7, 1.0, host3, host3, buf, buf, buf, None]
    for i in (0, 5, 6, 7, 8, 9):
        a = list(emit_args)
        a[i] = None
        assert lib.ngp_mc_emit(*a) == -22, i
    t = (C.c_int8 * 4096)()
    assert lib.ngp_mc_tables(None, t, t) == -22 and lib.ngp_mc_tables(t, None, t) == -22
    assert lib.ngp_mc_tables(t, t, None) == -22


def test_ply_round_trip_and_header(ngp, tmp_path):
    from ngp_amd.mesh import read_ply, write_ply
    g = np.random.default_rng(1)
    v = g.standard_normal((17, 3)).astype(np.float32)
    f = g.integers(0, 17, (29, 3)).astype(np.int32)
    nrm = g.standard_normal((17, 3)).astype(np.float32)
    p = tmp_path / "a.ply"
    write_ply(str(p), torch.from_numpy(v), torch.from_numpy(f))
    data = p.read_bytes()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\nproperty float y\n"
              b"property float z\nelement face 29\nproperty list uchar int vertex_indices\nend_header\n")
    assert data.startswith(header) and len(data) == len(header) + 17 * 12 + 29 * 13
    assert data[len(header) + 17 * 12] == 3     # list length of the first face
    rv, rf, rn = read_ply(str(p))
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rn is None
    write_ply(str(p), v, f, normals=nrm)
    data = p.read_bytes()
    assert b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face 29\n" in data
    rv, rf, rn = read_ply(str(p))
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rn, nrm)
    write_ply(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    rv, rf, _ = read_ply(str(p))
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_marching_cubes_refuses_cpu_tensors(ngp):
    from ngp_amd.mesh import marching_cubes as mc
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        mc(torch.zeros(4, 4, 4), 0.5)


def test_extract_mesh_tool_help_names_the_reference_call():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    txt = " ".join(out.stdout.split())
    assert "--bbox -1 -0.3 -1 1 0.15 1 --resolution 512 128 512 --level 10 --reference_spacing" in txt
