"""numpy restatement of mesh evaluation (include/ngp_hip.h M4): the squared distance from a point to a triangle by the
seven-region closest-point sequence, operation for operation in the dtype of its inputs, as a brute force over all
faces with the tie, NaN, degenerate-face and clip rules of ngp_mesh_closest (float32: what the kernel must give bit for
bit; float64: what the float32 sequence is measured against), and the surface sampler given a cdf."""
import numpy as np

REGIONS = ("a", "b", "ab", "c", "ac", "bc", "interior")   # in the order they are tested


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def tri_d2(p, a, b, c):
    """p, a, b, c (..., 3) of ONE float dtype, broadcastable -> (d2 (...), region (...) int: index into REGIONS)"""
    assert p.dtype == a.dtype == b.dtype == c.dtype and p.dtype in (np.float32, np.float64)
    one = p.dtype.type(1)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        zero = np.zeros(np.broadcast(p, a).shape, p.dtype)
        qs = [a + zero, b + zero,
              a + ab * (d1 / (d1 - d3))[..., None],
              c + zero,
              a + ac * (d2 / (d2 - d6))[..., None],
              b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]]
        den = one / ((va + vb) + vc)
        q = (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]
        region = np.full(q.shape[:-1], 6)
        for k in range(5, -1, -1):                      # the first condition that holds wins
            q = np.where(conds[k][..., None], qs[k], q)
            region = np.where(conds[k], k, region)
        e = p - q
        out = _dot(e, e)
    assert out.dtype == p.dtype
    return out, region


def nondegenerate(verts, faces):
    """(F,) bool: the float32 cross product (v1 - v0) x (v2 - v0) is not exactly (0, 0, 0)"""
    v = verts.astype(np.float32)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    with np.errstate(all="ignore"):
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return ~((n == 0).all(1))


def closest_brute(points, verts, faces, max_dist, dtype=np.float32, chunk=128):
    """every point against every face -> (d2 (n,) dtype, face (n,) int32): the smallest d2 over the non-degenerate
    faces, the smallest face index among equal d2, a NaN or infinite d2 never wins; a winner beyond max_dist^2 (one
    product in dtype), or none, gives (max_dist^2, -1)"""
    p, v = points.astype(dtype), verts.astype(dtype)
    n, n_faces = p.shape[0], faces.shape[0]
    md2 = dtype(np.float32(max_dist)) * dtype(np.float32(max_dist))
    d2 = np.full(n, md2, dtype)
    face = np.full(n, -1, np.int32)
    if n == 0 or n_faces == 0:
        return d2, face
    keep = nondegenerate(verts, faces)
    a, b, c = (v[faces[:, k]][None] for k in range(3))
    for s in range(0, n, chunk):
        d, _ = tri_d2(p[s:s + chunk, None, :], a, b, c)
        d = np.where(keep[None] & (d < np.inf), d, np.inf)      # NaN < inf is False
        f = np.argmin(d, 1)                                      # the first of equal minima
        best = d[np.arange(d.shape[0]), f]
        won = (best < np.inf) & ~(best > md2)
        d2[s:s + chunk] = np.where(won, best, md2)
        face[s:s + chunk] = np.where(won, f, -1)
    return d2, face


# ---------------------------------------------------------------------------------------------------------- sampler
def fmix32(h):
    """the 32-bit finaliser of MurmurHash3 on uint64 arrays holding 32-bit values"""
    m = np.uint64(0xFFFFFFFF)
    h = np.asarray(h, np.uint64) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def _first(cdf, pred_true_is_right, n):
    """the kernel's binary search: the first f in [0, hi0) with pred(cdf[f]) per element (hi0 where there is none)"""
    lo = np.zeros(n, np.int64)
    hi = np.full(n, pred_true_is_right[1], np.int64)
    while (lo < hi).any():
        live = lo < hi
        mid = lo + (hi - lo) // 2
        right = pred_true_is_right[0](cdf[np.minimum(mid, cdf.size - 1)])
        hi = np.where(live & right, mid, hi)
        lo = np.where(live & ~right, mid + 1, lo)
    return lo


def sample_surface(verts, faces, cdf, n, seed):
    """-> (points (n,3) float32, face (n,) int32), given the inclusive running sum `cdf` (F,) float64 of the areas"""
    verts = verts.astype(np.float32)
    i = np.arange(n, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    u = [fmix32((np.uint64(seed & 0xFFFFFFFF) + np.uint64(0x9E3779B9) * ((np.uint64(3) * i + np.uint64(k + 1)) & m)) & m)
         for k in range(3)]
    total = np.float64(cdf[-1])
    t = ((u[0].astype(np.float64) + 0.5) * 2.0 ** -32) * total
    n_faces = faces.shape[0]
    lo = _first(cdf, (lambda x: x > t, n_faces), n)
    last = _first(cdf, (lambda x: x >= total, n_faces - 1), n)
    f = np.minimum(lo, last)
    r1 = (u[1] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    r2 = (u[2] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    fold = r1 + r2 > np.float32(1)
    r1 = np.where(fold, np.float32(1) - r1, r1)
    r2 = np.where(fold, np.float32(1) - r2, r2)
    v0, v1, v2 = (verts[faces[f, k]] for k in range(3))
    pts = (v0 + r1[:, None] * (v1 - v0)) + r2[:, None] * (v2 - v0)
    assert pts.dtype == np.float32
    return pts, f.astype(np.int32)


def area_cdf(verts, faces):
    """float64 running sum of 0.5 |(v1 - v0) x (v2 - v0)|"""
    v = verts.astype(np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    return np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))


def barycentric(points, verts, faces, face):
    """float64 barycentric coordinates (n, 3) of each point in the plane of its face"""
    v = verts.astype(np.float64)
    a, b, c = (v[faces[face, k]] for k in range(3))
    e1, e2, ep = b - a, c - a, points.astype(np.float64) - a
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    p1, p2 = (ep * e1).sum(1), (ep * e2).sum(1)
    det = d11 * d22 - d12 * d12
    s, t = (d22 * p1 - d12 * p2) / det, (d11 * p2 - d12 * p1) / det
    return np.stack([1 - s - t, s, t], 1)


# ----------------------------------------------------------------------------------------------------------- meshes
def sheet(n_quads, z, extent=1.0):
    """an n x n-quad square sheet [0, extent]^2 at height z -> verts (.,3) float32, faces (.,3) int32"""
    ax = np.linspace(0.0, extent, n_quads + 1)
    x, y = np.meshgrid(ax, ax, indexing="ij")
    verts = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n_quads), np.arange(n_quads), indexing="ij")
    v00 = (i * (n_quads + 1) + j).ravel()
    v10, v01, v11 = v00 + n_quads + 1, v00 + 1, v00 + n_quads + 2
    faces = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)
    return verts, faces


def small_triangles(seed, n_faces, size, lo=-1.0, hi=1.0):
    """n_faces separate triangles of edge ~size with centres uniform in [lo, hi]^3"""
    g = np.random.default_rng(seed)
    centre = g.uniform(lo, hi, (n_faces, 1, 3))
    verts = (centre + g.uniform(-size, size, (n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def mesh_with_dead_faces():
    """a soup whose first and last faces, and some between, have no area (collinear, or a repeated vertex)"""
    verts, faces = small_triangles(5, 40, 0.2)
    faces = faces.copy()
    faces[0] = (0, 0, 1)
    faces[-1] = (5, 5, 5)
    faces[17] = (3, 4, 3)
    verts[3 * 23:3 * 23 + 3] = np.array([[0, 0, 0], [0.25, 0.25, 0.5], [0.5, 0.5, 1.0]], np.float32)   # collinear
    return verts, faces


# the hand cases: one triangle, points with known answers in every region and on every boundary
HAND_A, HAND_B, HAND_C = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
HAND_CASES = [  # point, squared distance, region
    ((0.5, 0.5, 3.0), 9.0, "interior"),           # above the interior
    ((0.5, 0.5, 0.0), 0.0, "interior"),           # in the plane, inside
    ((1.0, -1.0, 0.0), 1.0, "ab"),                # beyond edge ab
    ((-1.0, 1.0, 2.0), 5.0, "ac"),                # beyond edge ac, and above
    ((2.0, 2.0, 0.0), 2.0, "bc"),                 # beyond edge bc: closest (1, 1, 0)
    ((-1.0, -2.0, 0.0), 5.0, "a"),                # beyond vertex a
    ((4.0, -1.0, 0.0), 5.0, "b"),                 # beyond vertex b
    ((-1.0, 5.0, 1.0), 11.0, "c"),                # beyond vertex c
    ((0.0, 0.0, 0.0), 0.0, "a"),                  # exactly on vertex a
    ((2.0, 0.0, 0.0), 0.0, "b"),                  # exactly on vertex b
    ((0.0, 2.0, 0.0), 0.0, "c"),                  # exactly on vertex c
    ((1.0, 0.0, 0.0), 0.0, "ab"),                 # exactly on edge ab
    ((1.0, 1.0, 0.0), 0.0, "bc"),                 # exactly on edge bc
    ((0.0, 0.5, 0.0), 0.0, "ac"),                 # exactly on edge ac
    ((3.0, 3.0, 0.0), 8.0, "bc"),                 # in the plane, outside
]
