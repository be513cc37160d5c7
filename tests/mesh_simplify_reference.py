"""fp64 numpy restatement of mesh simplification (mesh_simplify_kernels.hip and ngp_amd.mesh.simplify_mesh): uniform
vertex clustering with one quadric solve per cell.  Keys are formed in float32 exactly as the kernel forms them, so
clusters and faces are comparable bit for bit; every sum is in float64 in ascending vertex, then (face, corner) order
(np.add.at adds in index order)."""
import numpy as np

KEY_LIMIT = 1 << 21
MAX_CELLS = 1 << 20


def cell_keys(verts, origin, cell):
    """(V,3) int64 keys floorf((v - origin) * (1/cell)), every operation in float32; ValueError for a cell that is
    not positive, a coordinate that is not finite or a key outside [0, 2^21)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32).reshape(3)
    cell = np.float32(cell)
    with np.errstate(all="ignore"):
        inv = np.float32(1) / cell
        if not (cell > 0 and np.isfinite(cell) and np.isfinite(inv)):
            raise ValueError(f"cell {cell}")
        q = np.floor((v - o) * inv)
    assert q.dtype == np.float32
    if not ((q >= 0) & (q < KEY_LIMIT)).all():
        raise ValueError("a vertex is not finite or its key lies outside [0, 2^21)")
    return q.astype(np.int64)


def clusters(keys):
    """cluster number of every vertex, numbered in ascending order of the smallest member -> (cluster (V,), count)"""
    packed = keys[:, 0] << 42 | keys[:, 1] << 21 | keys[:, 2]
    _, first, inverse = np.unique(packed, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)], len(first)


def face_pass(faces, cluster):
    """-> corners as cluster numbers (F,3), kept mask, degenerate count, duplicate count"""
    c = cluster[np.asarray(faces, np.int64).reshape(-1, 3)]
    deg = (c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 0] == c[:, 2])
    kept = np.zeros(len(c), bool)
    live = np.nonzero(~deg)[0]
    if len(live):
        _, first = np.unique(np.sort(c[live], 1), axis=0, return_index=True)    # first = the smallest face index
        kept[live[first]] = True
    return c, kept, int(deg.sum()), int(len(live) - kept.sum())


def count(verts, faces, cell, origin):
    """the count-only path -> (clusters, kept faces, degenerate, duplicate)"""
    cluster, n = clusters(cell_keys(verts, origin, cell))
    _, kept, deg, dup = face_pass(faces, cluster)
    return n, int(kept.sum()), deg, dup


def place(verts, faces, cluster, n, keys, origin, cell, placement, regularization):
    """one position per cluster (n,3) float32"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cnt = np.bincount(cluster, minlength=n).astype(np.float64)
    m = np.zeros((n, 3))
    np.add.at(m, cluster, v)
    m /= cnt[:, None]
    if placement == "mean":
        return m.astype(np.float32)
    assert placement == "quadric"
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                    e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    d = nrm[:, 0] * p0[:, 0] + nrm[:, 1] * p0[:, 1] + nrm[:, 2] * p0[:, 2]
    A = np.zeros((n, 3, 3))
    b = np.zeros((n, 3))
    corner = cluster[f].reshape(-1)                        # ascending (face, corner)
    np.add.at(A, corner, np.repeat(nrm[:, :, None] * nrm[:, None, :], 3, axis=0))
    np.add.at(b, corner, np.repeat(d[:, None] * nrm, 3, axis=0))
    t = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    ok = (t != 0) & np.isfinite(t)
    x = m.copy()
    if ok.any():
        lam = regularization * t[ok] / 3.0
        s = np.linalg.solve(A[ok] + lam[:, None, None] * np.eye(3), (b[ok] + lam[:, None] * m[ok])[:, :, None])[:, :, 0]
        first = np.zeros(n, np.int64)
        first[cluster[::-1]] = np.arange(len(cluster))[::-1]      # the smallest member of each cluster
        k = keys[first][ok].astype(np.float64)
        o = np.asarray(origin, np.float32).astype(np.float64)
        c = float(np.float32(cell))
        x[ok] = np.minimum(np.maximum(s, o + k * c), o + (k + 1.0) * c)
    return x.astype(np.float32)


def search_cells(verts, faces, origin, extent, target_faces):
    """-> (k, probes): k doubles from 1 until more than target_faces faces are kept (or nothing merges, or k = 2^20),
    then a bisection between the last k that kept <= target_faces and that one; 0 if k = 1 already keeps too many"""
    probes, k, lo, hi = 0, 1, 0, None
    n_verts = len(verts)
    while True:
        n, kept, _, _ = count(verts, faces, np.float32(extent / k), origin)
        probes += 1
        if kept > target_faces:
            hi = k
            break
        lo = k
        if n == n_verts or k >= MAX_CELLS:
            break
        k *= 2
    while hi is not None and hi - lo > 1:
        mid = (lo + hi) // 2
        kept = count(verts, faces, np.float32(extent / mid), origin)[1]
        probes += 1
        if kept <= target_faces:
            lo = mid
        else:
            hi = mid
    return lo, probes


def simplify(verts, faces, cell=None, target_faces=None, origin=None, placement="quadric", regularization=1e-3,
             normals=None, colors=None):
    """the whole of simplify_mesh -> dict(verts, faces, normals, colors, vertex_map, stats); vertex_map[v] is the
    output vertex of input vertex v, or -1 where its cluster is used by no kept face"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    assert (cell is None) != (target_faces is None)
    V, F = len(verts), len(faces)
    stats = dict(cell=None, k=None, probes=0, clusters=V, V_in=V, V_out=V, F_in=F, F_out=F, degenerate=0, duplicate=0)
    empty = dict(verts=verts[:0], faces=faces[:0], normals=None if normals is None else normals[:0],
                 colors=None if colors is None else colors[:0], vertex_map=np.full(V, -1, np.int64), stats=stats)
    if V == 0:
        stats.update(V_out=0, F_out=0)
        return empty
    if target_faces is not None and F <= target_faces:
        return dict(verts=verts, faces=faces, normals=normals, colors=colors, vertex_map=np.arange(V), stats=stats)
    if not np.isfinite(verts).all():
        raise ValueError("verts holds a value that is not finite")
    lo, hi = verts.min(0), verts.max(0)
    origin = lo if origin is None else np.asarray(origin, np.float32)
    if target_faces is not None:
        extent = float((hi - lo).max())
        extent = extent if extent > 0 else 1.0
        k, probes = search_cells(verts, faces, origin, extent, target_faces)
        stats.update(k=k, probes=probes)
        if k == 0:
            stats.update(V_out=0, F_out=0)
            return empty
        cell = extent / k
    cell = np.float32(cell)
    keys = cell_keys(verts, origin, cell)
    cluster, n = clusters(keys)
    c, kept, deg, dup = face_pass(faces, cluster)
    stats.update(cell=float(cell), clusters=n, degenerate=deg, duplicate=dup)
    x = place(verts, faces, cluster, n, keys, origin, cell, placement, regularization)
    kept_faces = c[kept]
    used = np.zeros(n, bool)
    used[kept_faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    out = dict(verts=x[used], faces=new[kept_faces].astype(np.int32).reshape(-1, 3), normals=None, colors=None,
               vertex_map=np.where(used[cluster], new[cluster], -1), stats=stats)
    cnt = np.bincount(cluster, minlength=n)
    if normals is not None:
        s = np.zeros((n, 3))
        np.add.at(s, cluster, np.asarray(normals, np.float32).astype(np.float64))
        mean = s / cnt[:, None]
        length = np.sqrt(mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1] + mean[:, 2] * mean[:, 2])
        with np.errstate(all="ignore"):
            unit = np.where((length > 0)[:, None], mean / length[:, None], 0.0)
        out["normals"] = unit.astype(np.float32)[used]
    if colors is not None:
        s = np.zeros((n, 3), np.int64)
        np.add.at(s, cluster, np.asarray(colors, np.uint8).astype(np.int64))
        out["colors"] = ((2 * s + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)[used]
    stats.update(V_out=int(used.sum()), F_out=int(kept.sum()))
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def wedge(n=60, seed=0):
    """two n x n grid sheets of edge 1 in planes at 90 degrees that share the crease, rotated by a seeded random
    rotation R and shifted by t off the origin -> verts (float32), faces, R, t (a point p of the unrotated wedge,
    z = 0 or y = 0, sits at p @ R.T + t)"""
    g = np.random.default_rng(seed)
    a = np.linspace(0.0, 1.0, n)
    x, u = np.meshgrid(a, a, indexing="ij")
    sheet_a = np.stack([x, u, np.zeros_like(x)], -1).reshape(-1, 3)          # plane z = 0
    sheet_b = np.stack([x, np.zeros_like(x), u], -1).reshape(-1, 3)          # plane y = 0; u = 0 is the crease
    idx_a = np.arange(n * n).reshape(n, n)
    idx_b = idx_a + n * n
    idx_b[:, 0] = idx_a[:, 0]                                               # welded along the crease

    def quads(idx, flip):
        q = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 4)
        t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
        return t[:, ::-1] if flip else t

    pts = np.concatenate([sheet_a, sheet_b])
    faces = np.concatenate([quads(idx_a, False), quads(idx_b, True)])
    used = np.zeros(len(pts), bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    R, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    t = g.uniform(2.0, 5.0, 3) * np.sign(g.standard_normal(3))
    verts = (pts[used] @ R.T + t).astype(np.float32)
    return verts, np.ascontiguousarray(new[faces], np.int32), R, t


def plane_distance(verts, R, t):
    """distance of every vertex to the nearer of the wedge's two planes"""
    p = (np.asarray(verts, np.float64) - t) @ R
    return np.minimum(np.abs(p[:, 2]), np.abs(p[:, 1]))


def soup(seed, n_verts=500, n_faces=3000):
    """a seeded random triangle soup whose indices repeat: degenerate and duplicate faces occur"""
    g = np.random.default_rng(seed)
    verts = (g.standard_normal((n_verts, 3)) + g.uniform(-3, 3, 3)).astype(np.float32)
    faces = g.integers(0, n_verts, (n_faces, 3))
    same = g.random(n_faces) < 0.05
    faces[same, 1] = faces[same, 0]                                          # degenerate before any clustering
    again = g.random(n_faces) < 0.05
    faces[again] = faces[g.integers(0, n_faces, int(again.sum()))][:, g.permutation(3)]   # copies, corners permuted
    return verts, faces.astype(np.int32)
