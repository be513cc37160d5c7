"""numpy restatement of mesh cleaning (mesh_clean_kernels.hip and ngp_amd.mesh.clean_mesh): component labels, faces
per component, the choice of components and the compaction, plus a brute-force BFS to check the labels against."""
from collections import deque

import numpy as np


def labels(faces, n_verts):
    """labels[v] = the smallest vertex index of v's component (faces sharing a vertex are connected)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.arange(n_verts, dtype=np.int64)
    if not len(f):
        return lab.astype(np.int32)
    while True:
        old = lab.copy()
        m = lab[f].min(1)
        np.minimum.at(lab, f.reshape(-1), np.repeat(m, 3))
        while True:
            jumped = lab[lab]
            if np.array_equal(jumped, lab):
                break
            lab = jumped
        if np.array_equal(lab, old):
            return lab.astype(np.int32)


def labels_bfs(faces, n_verts):
    """the same labels by breadth-first search over the vertex graph"""
    adj = [[] for _ in range(n_verts)]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3):
        for x, y in ((a, b), (b, c), (c, a)):
            adj[x].append(y)
            adj[y].append(x)
    lab = np.full(n_verts, -1, np.int32)
    for s in range(n_verts):          # ascending: the first vertex reached of a component is its smallest
        if lab[s] >= 0:
            continue
        lab[s] = s
        q = deque([s])
        while q:
            x = q.popleft()
            for y in adj[x]:
                if lab[y] < 0:
                    lab[y] = s
                    q.append(y)
    return lab


def face_counts(faces, lab):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.bincount(lab[f[:, 0]], minlength=len(lab)).astype(np.int32)


def select(counts, keep_largest=None, min_faces=None):
    """keep (V,) uint8 by label: components with faces that are among the keep_largest with the most faces (ties to
    the smaller label) and have at least min_faces faces"""
    counts = np.asarray(counts)
    keep = counts > 0
    if min_faces is not None:
        keep &= counts >= min_faces
    if keep_largest is not None:
        roots = np.nonzero(counts > 0)[0]
        order = np.lexsort((roots, -counts[roots]))      # most faces first, then the smaller label
        top = np.zeros_like(keep)
        top[roots[order[:keep_largest]]] = True
        keep &= top
    return keep.astype(np.uint8)


def compact(verts, faces, lab, counts, keep, attrs=()):
    """-> kept verts, faces renumbered, and the kept rows of each attribute, all in their original order"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vk = (keep[lab] != 0) & (counts[lab] > 0)
    fk = keep[lab[f[:, 0]]] != 0 if len(f) else np.zeros(0, bool)
    new = np.cumsum(vk) - 1
    out_f = new[f[fk]].astype(np.int32).reshape(-1, 3)
    return (np.asarray(verts)[vk], out_f) + tuple(np.asarray(a)[vk] for a in attrs)


def clean(verts, faces, attrs=(), keep_largest=None, min_faces=None):
    """the whole of clean_mesh -> (verts, faces, *attrs), labels, counts"""
    lab = labels(faces, len(verts))
    cnt = face_counts(faces, lab)
    keep = select(cnt, keep_largest, min_faces)
    return compact(verts, faces, lab, cnt, keep, attrs), lab, cnt


def random_faces(g, n_verts, n_faces, n_isolated=0, degenerate=0.1):
    """random triangles over the first n_verts - n_isolated vertices (the rest are used by no face), a share of them
    with repeated corners"""
    used = n_verts - n_isolated
    f = g.integers(0, used, (n_faces, 3)) if used > 0 else np.zeros((0, 3), np.int64)
    deg = g.random(len(f)) < degenerate
    f[deg, 1] = f[deg, 0]
    perm = g.permutation(n_verts)      # scatter the unused vertices over the index range
    return perm[f].astype(np.int32)
