"""CPU restatement of the marching-cubes passes of mesh_kernels.hip (numpy, float32 operation for operation) with the
case table the library exports (ngp_mc_tables), and the mesh checks the host and GPU tests share."""
import numpy as np


def mc_tables(ngp):
    tri = np.zeros((256, 16), np.int8)
    cnt = np.zeros(256, np.int8)
    ec = np.zeros((12, 2), np.int8)
    assert ngp._lib.call_host("mc_tables", tri.ctypes.data, cnt.ctypes.data, ec.ctypes.data) == 0
    return tri, cnt, ec


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def mc_counts(vol, level, tables):
    """(V, F) of the count pass"""
    tri, cnt, _ = tables
    inside = np.asarray(vol) > np.float32(level)
    nv = int((inside[:-1] != inside[1:]).sum() + (inside[:, :-1] != inside[:, 1:]).sum()
             + (inside[:, :, :-1] != inside[:, :, 1:]).sum())
    return nv, int(cnt[_cases(inside)].astype(np.int64).sum())


def _cases(inside):
    cs = np.zeros(tuple(s - 1 for s in inside.shape), np.int32)
    for c in range(8):
        dx, dy, dz = corner_offset(c)
        cs |= inside[dx:dx + cs.shape[0], dy:dy + cs.shape[1], dz:dz + cs.shape[2]].astype(np.int32) << c
    return cs


def marching_cubes(vol, level, tables, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """the two passes of mesh_kernels.hip -> verts (V,3) f32, faces (F,3) i32, in the kernels' order"""
    tri, cnt, ec = tables
    vol = np.ascontiguousarray(vol, np.float32)
    nx, ny, nz = vol.shape
    lv = np.float32(level)
    inside = vol > lv
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    cross = cross.reshape(-1, 3)
    vid = np.cumsum(cross.reshape(-1)) - 1            # vertex of (point, axis): point-major, x < y < z
    p, a = np.nonzero(cross)
    stride = np.array([ny * nz, nz, 1])
    flat = vol.reshape(-1)
    v0, v1 = flat[p], flat[p + stride[a]]
    with np.errstate(all="ignore"):
        t = (lv - v0) / (v1 - v0)
    t = np.fmin(np.fmax(t, np.float32(0)), np.float32(1)).astype(np.float32)
    idx = np.stack(np.unravel_index(p, vol.shape), 1).astype(np.float32)
    o, s = np.asarray(origin, np.float32), np.asarray(spacing, np.float32)
    verts = np.empty((p.size, 3), np.float32)
    for c in range(3):
        on = a == c
        verts[:, c] = o[c] + np.where(on, idx[:, c] + t, idx[:, c]) * s[c]
    cs = _cases(inside).reshape(-1)
    ci, cj, ck = np.unravel_index(np.arange(cs.size), (nx - 1, ny - 1, nz - 1))
    owner_p = (ci * ny + cj) * nz + ck                # the point that owns each cell
    rows = tri[cs].astype(np.int64)                   # (cells, 16), -1 terminated
    keep = rows >= 0
    e = rows[keep]
    cell_p = np.broadcast_to(owner_p[:, None], rows.shape)[keep]
    off = np.array([corner_offset(c) @ stride for c in range(8)])
    q = cell_p + off[ec[e, 0]]
    faces = vid[3 * q + (e >> 2)].astype(np.int32).reshape(-1, 3)
    return verts, faces


# ------------------------------------------------------------------------------------------------------ mesh checks
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces, n_verts):
    """every undirected edge in exactly two faces, traversed in opposite directions"""
    d = directed_edges(faces)
    key = d[:, 0] * n_verts + d[:, 1]
    rev = d[:, 1] * n_verts + d[:, 0]
    u = np.unique(key)
    return u.size == key.size and np.array_equal(np.sort(key), np.sort(rev))


def euler_characteristic(faces, n_verts):
    d = directed_edges(faces)
    n_edges = np.unique(np.sort(d, 1), axis=0).shape[0]
    return n_verts - n_edges + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6)


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])   # length = 2 * area


def n_components(faces, n_verts):
    parent = np.arange(n_verts)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in directed_edges(faces)[: len(faces) * 2]:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    used = np.unique(np.asarray(faces))
    return len({find(x) for x in used})
