"""Mesh cleaning and coloured PLY without a GPU: the numpy restatement of tests/mesh_clean_reference.py against
brute-force BFS, the component choice of ngp_amd.mesh against the restatement, the M2 C ABI contract (no launch), the
PLY colour properties, and the tool's new options."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clean_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(8))
def test_restatement_labels_match_bfs(seed):
    g = np.random.default_rng(seed)
    n_verts = int(g.integers(1, 300))
    n_faces = int(g.integers(0, n_verts // 2 + 1))
    faces = ref.random_faces(g, n_verts, n_faces, n_isolated=int(g.integers(0, n_verts // 4 + 1)), degenerate=0.2)
    lab = ref.labels(faces, n_verts)
    assert np.array_equal(lab, ref.labels_bfs(faces, n_verts))
    assert (lab <= np.arange(n_verts)).all() and np.array_equal(lab[lab], lab)
    cnt = ref.face_counts(faces, lab)
    assert cnt.sum() == n_faces and (cnt[lab != np.arange(n_verts)] == 0).all()


def test_restatement_edge_cases():
    # F = 0: every vertex is its own component, with no faces, and nothing survives the compaction
    lab = ref.labels(np.zeros((0, 3), np.int32), 5)
    assert np.array_equal(lab, np.arange(5)) and np.array_equal(ref.labels_bfs(np.zeros((0, 3)), 5), lab)
    (v, f), _, cnt = ref.clean(np.ones((5, 3), np.float32), np.zeros((0, 3), np.int32))
    assert v.shape == (0, 3) and f.shape == (0, 3) and not cnt.any()
    # one degenerate face (a single vertex used three times) and an isolated vertex
    faces = np.array([[2, 2, 2]], np.int32)
    (v, f), lab, cnt = ref.clean(np.arange(9, dtype=np.float32).reshape(3, 3), faces)
    assert np.array_equal(lab, [0, 1, 2]) and np.array_equal(cnt, [0, 0, 1])
    assert np.array_equal(v, [[6, 7, 8]]) and np.array_equal(f, [[0, 0, 0]])
    # a chain: faces (i, i+1, i+2) join everything into one component labelled 0
    n = 2000
    chain = np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.int32)
    assert not ref.labels(chain[::-1], n).any()


def test_restatement_selection_and_compaction():
    # three components with 3, 1 and 3 faces (labels 0, 5, 3: a tie between 0 and 3), one isolated vertex (8)
    faces = np.array([[0, 1, 2], [1, 2, 4], [2, 4, 0], [5, 6, 7], [3, 9, 10], [9, 10, 11], [10, 11, 3]], np.int32)
    verts = np.arange(12 * 3, dtype=np.float32).reshape(12, 3)
    cols = np.arange(12 * 3, dtype=np.uint8).reshape(12, 3)
    lab = ref.labels(faces, 12)
    cnt = ref.face_counts(faces, lab)
    assert np.array_equal(np.nonzero(cnt)[0], [0, 3, 5]) and list(cnt[[0, 3, 5]]) == [3, 3, 1]
    assert np.array_equal(np.nonzero(ref.select(cnt, keep_largest=1))[0], [0])       # tie: the smaller label
    assert np.array_equal(np.nonzero(ref.select(cnt, keep_largest=2))[0], [0, 3])
    assert np.array_equal(np.nonzero(ref.select(cnt, min_faces=2))[0], [0, 3])
    assert np.array_equal(np.nonzero(ref.select(cnt, keep_largest=3, min_faces=2))[0], [0, 3])
    assert np.array_equal(np.nonzero(ref.select(cnt))[0], [0, 3, 5])
    v, f, c = ref.compact(verts, faces, lab, cnt, ref.select(cnt, keep_largest=1), (cols,))
    assert np.array_equal(v, verts[[0, 1, 2, 4]]) and np.array_equal(c, cols[[0, 1, 2, 4]])
    assert np.array_equal(f, [[0, 1, 2], [1, 2, 3], [2, 3, 0]])
    v, f = ref.compact(verts, faces, lab, cnt, ref.select(cnt))
    assert len(v) == 11 and not (v == verts[8]).all(1).any() and len(f) == 7    # only the isolated vertex goes


@pytest.mark.parametrize("seed", range(4))
def test_select_components_matches_restatement(ngp, seed):
    g = np.random.default_rng(100 + seed)
    counts = np.where(g.random(500) < 0.3, g.integers(0, 6, 500), 0).astype(np.int32)   # many ties
    for k, m in ((None, None), (1, None), (7, None), (None, 3), (4, 2), (0, None), (1000, 1)):
        got = ngp.mesh.select_components(torch.from_numpy(counts), keep_largest=k, min_faces=m)
        assert got.dtype == torch.uint8
        assert np.array_equal(got.numpy(), ref.select(counts, k, m)), (k, m)
    with pytest.raises(ValueError):
        ngp.mesh.select_components(torch.from_numpy(counts), keep_largest=-1)


def test_m2_c_abi_contract_without_launch(ngp):
    lib = ngp._lib.load()
    assert lib.ngp_mesh_clean_workspace(0, 0) == 0
    assert lib.ngp_mesh_clean_workspace(-1, 5) == -22 and lib.ngp_mesh_clean_workspace(5, -1) == -22
    assert lib.ngp_mesh_clean_workspace(2 ** 31 - 1, (2 ** 31 - 1) // 3 + 1) == -22
    assert lib.ngp_mesh_clean_workspace(1000, 300) >= 1000 + 300 + 2 * (4 + 2)
    big = lib.ngp_mesh_clean_workspace(2 ** 31 - 1, (2 ** 31 - 1) // 3)
    assert big > 2 ** 31    # an int64 element count
    buf = C.c_void_p(16)    # never dereferenced: every call below must return before a launch
    # empty inputs: NGP_OK before any pointer is looked at
    assert lib.ngp_mesh_labels_init(None, 0, None) == 0
    for nv, nf in ((0, 0), (0, 7), (7, 0)):
        assert lib.ngp_mesh_labels_round(None, nf, nv, None, None, None) == 0, (nv, nf)
    for nv, nf in ((0, 0), (0, 7)):
        assert lib.ngp_mesh_face_counts(None, nf, nv, None, None, None) == 0
        assert lib.ngp_mesh_compact_count(None, nf, nv, None, None, None, None, None, None) == 0
    for nv, nf in ((0, 0), (0, 7), (7, 0)):
        assert lib.ngp_mesh_compact_faces(None, nf, nv, None, None, None) == 0
    assert lib.ngp_mesh_compact_rows(None, 12, 0, 5, None, None, None) == 0
    assert lib.ngp_mesh_compact_rows(None, 0, 5, 5, None, None, None) == 0
    # negative sizes
    assert lib.ngp_mesh_labels_init(buf, -1, None) == -22
    for nv, nf in ((-1, 5), (5, -1)):
        assert lib.ngp_mesh_labels_round(buf, nf, nv, buf, buf, None) == -22
        assert lib.ngp_mesh_face_counts(buf, nf, nv, buf, buf, None) == -22
        assert lib.ngp_mesh_compact_count(buf, nf, nv, buf, buf, buf, buf, buf, None) == -22
        assert lib.ngp_mesh_compact_rows(buf, 12, nv, nf, buf, buf, None) == -22
        assert lib.ngp_mesh_compact_faces(buf, nf, nv, buf, buf, None) == -22
    assert lib.ngp_mesh_compact_rows(buf, -3, 5, 5, buf, buf, None) == -22
    # a NULL in any pointer position of a non-empty input
    assert lib.ngp_mesh_labels_init(None, 5, None) == -22
    calls = [(lib.ngp_mesh_labels_round, [buf, 5, 5, buf, buf, None], (0, 3, 4)),
             (lib.ngp_mesh_face_counts, [buf, 5, 5, buf, buf, None], (0, 3, 4)),
             (lib.ngp_mesh_compact_count, [buf, 5, 5, buf, buf, buf, buf, buf, None], (0, 3, 4, 5, 6, 7)),
             (lib.ngp_mesh_compact_rows, [buf, 12, 5, 5, buf, buf, None], (0, 4, 5)),
             (lib.ngp_mesh_compact_faces, [buf, 5, 5, buf, buf, None], (0, 3, 4))]
    for fn, args, ptrs in calls:
        for i in ptrs:
            a = list(args)
            a[i] = None
            assert fn(*a) == -22, (fn.__name__, i)


def _old_writer_bytes(v, f, nrm=None):
    """what write_ply wrote before colours existed, restated"""
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if nrm is not None else [])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property float {p}" for p in props]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    rows = v if nrm is None else np.concatenate([v, nrm], 1)
    face = b"".join(b"\x03" + np.asarray(t, "<i4").tobytes() for t in f)
    return ("\n".join(head) + "\n").encode() + rows.astype("<f4").tobytes() + face


def test_colourless_ply_is_unchanged(ngp, tmp_path):
    from ngp_amd.mesh import write_ply
    g = np.random.default_rng(2)
    v = g.standard_normal((23, 3)).astype(np.float32)
    f = g.integers(0, 23, (31, 3)).astype(np.int32)
    nrm = g.standard_normal((23, 3)).astype(np.float32)
    p = tmp_path / "a.ply"
    write_ply(str(p), torch.from_numpy(v), torch.from_numpy(f))
    assert p.read_bytes() == _old_writer_bytes(v, f)
    write_ply(str(p), v, f, normals=nrm, colors=None)
    assert p.read_bytes() == _old_writer_bytes(v, f, nrm)


def test_ply_colours_round_trip_and_header(ngp, tmp_path):
    from ngp_amd.mesh import read_ply, write_ply
    g = np.random.default_rng(3)
    v = g.standard_normal((19, 3)).astype(np.float32)
    f = g.integers(0, 19, (27, 3)).astype(np.int32)
    nrm = g.standard_normal((19, 3)).astype(np.float32)
    rgb = g.integers(0, 256, (19, 3)).astype(np.uint8)
    p = tmp_path / "c.ply"
    for normals in (None, nrm):
        write_ply(str(p), v, torch.from_numpy(f), normals=normals, colors=torch.from_numpy(rgb))
        data = p.read_bytes()
        floats = ["x", "y", "z"] + ([] if normals is None else ["nx", "ny", "nz"])
        header = ("ply\nformat binary_little_endian 1.0\nelement vertex 19\n"
                  + "".join(f"property float {q}\n" for q in floats)
                  + "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  + "element face 27\nproperty list uchar int vertex_indices\nend_header\n").encode()
        row = 4 * len(floats) + 3
        assert data.startswith(header) and len(data) == len(header) + 19 * row + 27 * 13
        first = data[len(header):len(header) + row]
        assert first[:12] == v[0].tobytes() and first[-3:] == rgb[0].tobytes()
        assert data[len(header) + 19 * row] == 3
        rv, rf, rn = read_ply(str(p))                       # the 3-tuple stays
        assert np.array_equal(rv, v) and np.array_equal(rf, f)
        assert (rn is None) if normals is None else np.array_equal(rn, nrm)
        rv, rf, rn, rc = read_ply(str(p), colors=True)
        assert rc.dtype == np.uint8 and np.array_equal(rc, rgb) and np.array_equal(rv, v) and np.array_equal(rf, f)
    write_ply(str(p), v, f)
    assert read_ply(str(p), colors=True)[3] is None
    write_ply(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), colors=np.zeros((0, 3), np.uint8))
    rv, rf, _, rc = read_ply(str(p), colors=True)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc.shape == (0, 3)


def test_ply_colours_readable_by_a_generic_parser(ngp, tmp_path):
    """a reader that knows only the PLY specification (numpy dtype from the header) sees floats then uchar RGB"""
    from ngp_amd.mesh import write_ply
    v = np.array([[0, 1, 2], [3, 4, 5]], np.float32)
    rgb = np.array([[255, 0, 7], [1, 2, 3]], np.uint8)
    p = tmp_path / "g.ply"
    write_ply(str(p), v, np.array([[0, 1, 1]], np.int32), colors=rgb)
    data = p.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    types = {"float": "<f4", "uchar": "u1"}
    fields = [(w[2], types[w[1]]) for w in (l.split() for l in data[:end].decode().splitlines())
              if w[0] == "property" and w[1] != "list"]
    assert [n for n, _ in fields] == ["x", "y", "z", "red", "green", "blue"]
    rec = np.frombuffer(data, np.dtype(fields), 2, end)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), v)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgb)


def test_extract_mesh_tool_help_names_the_cleaning_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--help"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for opt in ("--keep_largest K", "--min_faces M", "--colors"):
        assert opt in out.stdout, opt
