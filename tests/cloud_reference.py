"""Numpy restatements of include/ngp_hip.h M5 and of ngp_amd.cloud's host algorithms: the f32 brute-force nearest
point, the f32 transform of a query, the 18 sums of a registration step in float64, the sequential voxel mean, the
even-odd crop test, and a float64 point-to-point ICP on scipy's k-d tree.  Shared by test_cloud_host.py and
test_cloud_gpu.py."""
import numpy as np

F32 = np.float32


def transform_f32(points, xform12):
    """p'_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a in float32, in that order"""
    m = np.asarray(xform12, F32).reshape(3, 4)
    x, y, z = (np.ascontiguousarray(points[:, k], F32) for k in range(3))
    return np.stack([((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3] for a in range(3)], 1).astype(F32)


def nearest_brute(queries, cloud, max_dist, chunk=256):
    """-> (d2 f32, index int32): d2 = (dx dx + dy dy) + dz dz in f32 over every cloud point, compared with < from
    infinity (NaN and infinity never win), the first of equal minima, clipped at f32(max_dist)^2"""
    q, c = np.asarray(queries, F32), np.asarray(cloud, F32).reshape(-1, 3)
    md2 = F32(max_dist) * F32(max_dist)
    d2 = np.full(q.shape[0], md2, F32)
    index = np.full(q.shape[0], -1, np.int32)
    if c.shape[0] == 0:
        return d2, index
    with np.errstate(all="ignore"):
        for s in range(0, q.shape[0], chunk):
            p = q[s:s + chunk]
            dx, dy, dz = (p[:, None, k] - c[None, :, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == F32
            d = np.where(d < np.inf, d, F32(np.inf))
            best = d.argmin(1)                           # the first of equal minima: the smallest index
            bd = d[np.arange(p.shape[0]), best]
            won = (bd < np.inf) & ~(bd > md2)
            d2[s:s + chunk] = np.where(won, bd, md2)
            index[s:s + chunk] = np.where(won, best, -1)
    return d2, index


def sums18_terms(moved, matched_points, centre):
    """(n, 18) float64: the terms of the header's partials for matched queries p' = moved and winners q"""
    p = moved.astype(np.float64) - np.asarray(centre, F32).astype(np.float64)
    q = matched_points.astype(np.float64) - np.asarray(centre, F32).astype(np.float64)
    pq = (p[:, :, None] * q[:, None, :]).reshape(-1, 9)
    pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    return np.concatenate([np.ones((p.shape[0], 1)), p, q, pq, pp[:, None]], 1)


def exact_sums18(p, q):
    """the 18 sums of correspondences p -> q in float64 (d2 included), for kabsch()"""
    t = sums18_terms(np.asarray(p, np.float64), np.asarray(q, np.float64), np.zeros(3))
    d2 = ((np.asarray(p, np.float64) - np.asarray(q, np.float64)) ** 2).sum(1)
    return np.concatenate([t.sum(0), [d2.sum()]])


def voxel_keys(points, voxel, origin=None):
    p = np.asarray(points, F32).astype(np.float64)
    lo = p.min(0) if origin is None else np.asarray(origin, np.float64)
    c = np.floor((p - lo) / float(voxel))
    c = (c - c.min(0)).astype(np.int64)
    dims = c.max(0) + 1
    return (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]


def voxel_mean(points, voxel, normals=None, colors=None, origin=None):
    """one thread's work per voxel, restated: rows added in input order in double from 0.0, one division, one rounding;
    colours floor(mean + 0.5)"""
    keys = voxel_keys(points, voxel, origin)
    order = np.argsort(keys, kind="stable")
    uniq = np.unique(keys)
    out_p = np.zeros((uniq.size, 3), F32)
    out_n = None if normals is None else np.zeros((uniq.size, 3), F32)
    out_c = None if colors is None else np.zeros((uniq.size, 3), np.uint8)
    starts = np.searchsorted(keys[order], uniq)
    ends = np.append(starts[1:], keys.size)
    for v, (b, e) in enumerate(zip(starts, ends)):
        sp, sn, sc = np.zeros(3), np.zeros(3), np.zeros(3)
        for k in order[b:e]:
            sp = sp + points[k].astype(np.float64)
            if normals is not None:
                sn = sn + normals[k].astype(np.float64)
            if colors is not None:
                sc = sc + colors[k].astype(np.float64)
        count = float(e - b)
        out_p[v] = (sp / count).astype(F32)
        if normals is not None:
            out_n[v] = (sn / count).astype(F32)
        if colors is not None:
            out_c[v] = np.floor(sc / count + 0.5).astype(np.uint8)
    return out_p, out_n, out_c


def crop_contains(points, axis, axis_min, axis_max, polygon):
    """the even-odd crossing test of a SelectionPolygonVolume in float64, point by point"""
    u, v, w = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}[axis]
    poly = np.asarray(polygon, np.float64)
    out = np.zeros(len(points), bool)
    for i, p in enumerate(np.asarray(points, np.float64)):
        inside = False
        for k in range(len(poly)):
            a, b = poly[k], poly[(k + 1) % len(poly)]
            if (a[v] > p[v]) != (b[v] > p[v]) and p[u] < (b[u] - a[u]) * (p[v] - a[v]) / (b[v] - a[v]) + a[u]:
                inside = not inside
        out[i] = inside and axis_min <= p[w] <= axis_max
    return out


# -------------------------------------------------------------------------------------------------- registration
def rotation(axis, degrees):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def similarity(R, t, scale=1.0):
    T = np.eye(4)
    T[:3, :3] = scale * np.asarray(R, np.float64)
    T[:3, 3] = t
    return T


def l_shape(n, seed):
    """n float32 points on the faces of two boxes that form an L of unit extent: asymmetric, so a pose is unique"""
    g = np.random.default_rng(seed)
    boxes = [((0.0, 0.0, 0.0), (1.0, 0.3, 0.2)), ((0.0, 0.3, 0.0), (0.25, 0.8, 0.45))]
    out = []
    for (lo, hi), share in zip(boxes, (0.6, 0.4)):
        lo, hi = np.array(lo), np.array(hi)
        m = int(round(n * share))
        p = g.uniform(lo, hi, (m, 3))
        axis = g.integers(0, 3, m)
        side = g.integers(0, 2, m)
        p[np.arange(m), axis] = np.where(side == 0, lo[axis], hi[axis])
        out.append(p)
    return np.concatenate(out)[:n].astype(F32)


def subset_problem(seed=0, n_target=20_000, n_source=5_000, degrees=3.0, shift=0.02, scale=1.0):
    """-> (source f32, target f32, T_true): the source is a subset of the target moved by the inverse of T_true, a
    rotation by `degrees`, a translation of length `shift` and `scale`, and rounded to float32"""
    target = l_shape(n_target, seed)
    g = np.random.default_rng(seed + 1)
    pick = g.choice(n_target, n_source, replace=False)
    t = g.normal(size=3)
    T = similarity(rotation(g.normal(size=3), degrees), shift * t / np.linalg.norm(t), scale)
    Ti = np.linalg.inv(T)
    source = (target[pick].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)
    return source, target, T


def kabsch_points(p, q, with_scale=False):
    """Kabsch / Umeyama on explicit correspondences in float64: independent of the sums route"""
    mp, mq = p.mean(0), q.mean(0)
    H = (p - mp).T @ (q - mq)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    s = (S * np.diag(D)).sum() / ((p - mp) ** 2).sum() if with_scale else 1.0
    return similarity(R, mq - s * R @ mp, s)


def icp_reference(source, target, max_corr_dist, init=None, max_iter=30, tol=1e-6, with_scale=False):
    """float64 point-to-point ICP on scipy's k-d tree; the moved source is rounded to float32 each iteration, as the
    kernel's query is -> (T, fitness, rmse, iterations)"""
    from scipy.spatial import cKDTree
    tree = cKDTree(target.astype(np.float64))
    T = np.eye(4) if init is None else np.array(init, np.float64)
    prev = None
    for it in range(max_iter + 1):
        moved = (source.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32).astype(np.float64)
        d, j = tree.query(moved, distance_upper_bound=max_corr_dist)
        ok = np.isfinite(d)
        fitness, rmse = ok.mean(), float(np.sqrt((d[ok] ** 2).mean())) if ok.any() else 0.0
        if prev is not None and abs(fitness - prev[0]) < tol and abs(rmse - prev[1]) < tol:
            break
        if it == max_iter:
            break
        prev = (fitness, rmse)
        T = kabsch_points(moved[ok], target[j[ok]].astype(np.float64), with_scale) @ T
    return T, fitness, rmse, it
