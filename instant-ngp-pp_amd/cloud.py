"""Point clouds as ground truth (include/ngp_hip.h M5): what the benchmarks ship is a laser scan, a crop volume and
an initial alignment that the protocol refines by ICP before it measures anything.

  read_ply_points / write_ply_points   point-cloud PLY files (ascii and binary little-endian)
  PointGrid, nearest_points            the nearest point of a cloud: ngp_cloud_nearest on M4's uniform grid, exact in
                                       the sense of the header (what an f32 brute force gives, bit for bit)
  voxel_downsample                     one mean point per occupied voxel (ngp_cloud_voxel_mean), deterministic
  crop_box, CropVolume                 masks of an axis-aligned box and of Open3D's SelectionPolygonVolume JSON
  kabsch, icp                          point-to-point registration: one ngp_cloud_nearest + ngp_cloud_sum_partials and
                                       one 18-double read per iteration, the 3x3 solve in numpy float64
  cloud_distance, tnt_score            mesh.distance_metrics over two clouds; the shape of the Tanks-and-Temples script

Only the query and the per-iteration sums are device kernels of this module; sorting, cropping and the metrics are torch
on the same device, the PLY files and the SVD are numpy.  There is no CPU fallback."""
import ctypes as C
import json
import time

import numpy as np
import torch

from . import mesh as _mesh
from ._lib import call, check_input

_f32 = torch.float32
POINTS_PER_CELL = 4          # what the default cell aims at for points spread over the faces of their box
SUMS = 18                    # doubles per row of ngp_cloud_nearest's partials
BLOCK = 256                  # queries per row


# ------------------------------------------------------------------------------------------------------- PLY files
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_XYZ, _NORMAL, _RGB = ("x", "y", "z"), ("nx", "ny", "nz"), ("red", "green", "blue")


def _ply_elements(path, lines):
    """-> [(name, count, [(property name, numpy type or None for a list)])] of a PLY header's lines after `format`"""
    elements = []
    for line in lines:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "element" and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list":
            elements[-1][2].append((w[4], None))
        elif w[0] == "property" and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
        else:
            raise ValueError(f"{path}: header line {line!r} is not understood")
    return elements


def read_ply_points(path):
    """-> (points (n,3) f32, normals (n,3) f32 or None, colors (n,3) u8 or None) of the `vertex` element of an `ascii`
    or `binary_little_endian` PLY.  x y z, nx ny nz and red green blue may have any scalar PLY type; other scalar
    properties are skipped by their size and other elements (faces) are skipped or never reached.  A list property can
    only be skipped where its length need not be known in advance: in an ascii file or in an element after `vertex`;
    in or before the vertex element of a binary file it raises ValueError, as does any other format."""
    with open(path, "rb") as fh:
        data = fh.read()
    marker = data.find(b"end_header")
    if not data.startswith(b"ply") or marker < 0:
        raise ValueError(f"{path}: not a PLY file")
    end = data.index(b"\n", marker) + 1
    lines = [line.strip() for line in data[:end].decode("ascii").splitlines()]
    fmt = lines[1].split()
    if len(fmt) != 3 or fmt[0] != "format" or fmt[1] not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: {lines[1]!r} is not supported (ascii and binary_little_endian are)")
    elements = _ply_elements(path, lines[2:])
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: no vertex element")
    at = names.index("vertex")
    _, n, props = elements[at]
    cols = [p for p, _ in props]
    if not set(_XYZ) <= set(cols):
        raise ValueError(f"{path}: the vertex element has no x y z")
    if fmt[1] == "ascii":
        rows = data[end:].decode("ascii").splitlines()
        skip = sum(e[1] for e in elements[:at])
        rows = rows[skip:skip + n]
        if len(rows) != n:
            raise ValueError(f"{path}: {len(rows)} vertex lines, the header says {n}")
        if all(t is not None for _, t in props):
            table = np.array(" ".join(rows).split(), np.float64).reshape(n, len(props))
        else:                                     # a list is its length and that many values
            table = np.empty((n, len(props)), np.float64)
            for i, row in enumerate(rows):
                w, k = row.split(), 0
                for j, (_, t) in enumerate(props):
                    if t is None:
                        k += 1 + int(w[k])
                        table[i, j] = 0.0
                    else:
                        table[i, j] = float(w[k])
                        k += 1

        def column(key):
            return table[:, cols.index(key)]
    else:
        for name, _, pr in elements[:at + 1]:
            if any(t is None for _, t in pr):
                raise ValueError(f"{path}: a list property in the binary element {name!r} cannot be skipped")
        offset = end + sum(c * np.dtype([(p, "<" + t) for p, t in pr]).itemsize for _, c, pr in elements[:at])
        dt = np.dtype([(p, "<" + t) for p, t in props])
        if len(data) < offset + n * dt.itemsize:
            raise ValueError(f"{path}: the file ends inside the vertex element")
        table = np.frombuffer(data, dt, n, offset)

        def column(key):
            return table[key]

    def block(keys, dtype):
        if not set(keys) <= set(cols):
            return None
        return np.ascontiguousarray(np.stack([column(k) for k in keys], 1).astype(dtype)).reshape(n, 3)
    return block(_XYZ, np.float32), block(_NORMAL, np.float32), block(_RGB, np.uint8)


def write_ply_points(path, points, normals=None, colors=None):
    """binary little-endian PLY with one element: vertex (float x y z [nx ny nz] [uchar red green blue])"""
    fields = [("p", "<f4", (3,))] + ([("n", "<f4", (3,))] if normals is not None else []) + \
             ([("c", "u1", (3,))] if colors is not None else [])
    pts = _mesh._np(points).reshape(-1, 3)
    rec = np.empty(pts.shape[0], fields)
    rec["p"] = pts
    if normals is not None:
        rec["n"] = _mesh._np(normals).reshape(-1, 3)
    if colors is not None:
        rec["c"] = _mesh._np(colors).reshape(-1, 3)
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {rec.shape[0]}"]
    lines += [f"property float {p}" for p in _XYZ + (_NORMAL if normals is not None else ())]
    lines += [f"property uchar {p}" for p in _RGB] if colors is not None else []
    with open(path, "wb") as fh:
        fh.write(("\n".join(lines + ["end_header"]) + "\n").encode("ascii"))
        fh.write(rec.tobytes())


# ------------------------------------------------------------------------------------------------ transforms, crops
def _matrix(T):
    """a 4x4 float64 numpy matrix from anything that holds one (None: the identity)"""
    if T is None:
        return np.eye(4)
    T = np.array(_mesh._np(T), np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"a transform must be a finite 4x4 matrix, got shape {T.shape}")
    return T


def _xform12(T):
    """the upper 3x4 of T rounded once to float32: the HOST array ngp_cloud_nearest takes"""
    return (C.c_float * 12)(*[float(x) for x in T[:3, :4].reshape(-1)])


def transform_points(points, T):
    """T (4x4, upper 3x4 used) applied to (n,3) points in float64, rounded once to float32"""
    T = torch.from_numpy(_matrix(T)).to(points.device)
    return (points.double() @ T[:3, :3].T + T[:3, 3]).to(_f32).contiguous()


def crop_box(points, lo, hi):
    """-> (n,) bool: lo <= p <= hi on every axis"""
    lo = torch.as_tensor(lo, dtype=torch.float64, device=points.device)
    hi = torch.as_tensor(hi, dtype=torch.float64, device=points.device)
    p = points.double()
    return ((p >= lo) & (p <= hi)).all(1)


class CropVolume:
    """Open3D's SelectionPolygonVolume, the crop file Tanks and Temples ships: a polygon swept along one axis.
    contains(points) keeps a point whose coordinate on `axis` lies in [axis_min, axis_max] and that an even-odd
    crossing test on the other two axes puts inside the polygon.  Torch, float64."""
    _OTHERS = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}

    def __init__(self, orthogonal_axis, axis_min, axis_max, bounding_polygon):
        axis = str(orthogonal_axis).upper()
        if axis not in self._OTHERS:
            raise ValueError(f"orthogonal_axis must be X, Y or Z, got {orthogonal_axis!r}")
        self.axis, self.axis_min, self.axis_max = axis, float(axis_min), float(axis_max)
        self.polygon = np.array(bounding_polygon, np.float64).reshape(-1, 3)
        if self.polygon.shape[0] < 3:
            raise ValueError("bounding_polygon needs at least 3 vertices")

    @classmethod
    def from_json(cls, path):
        with open(path) as fh:
            d = json.load(fh)
        return cls(d["orthogonal_axis"], d["axis_min"], d["axis_max"], d["bounding_polygon"])

    def contains(self, points, chunk=1 << 20):
        u, v, w = self._OTHERS[self.axis]
        poly = torch.from_numpy(self.polygon).to(points.device)
        au, av = poly[:, u], poly[:, v]
        bu, bv = torch.roll(au, -1), torch.roll(av, -1)          # edge k runs from vertex k to vertex k + 1
        out = torch.empty(points.shape[0], dtype=torch.bool, device=points.device)
        for s in range(0, points.shape[0], chunk):
            p = points[s:s + chunk].double()
            pu, pv, pw = p[:, u:u + 1], p[:, v:v + 1], p[:, w]
            straddles = (av > pv) != (bv > pv)
            cross = pu < (bu - au) * (pv - av) / (bv - av) + au       # 0/0 only where straddles is False
            odd = (straddles & cross).sum(1) % 2 == 1
            out[s:s + chunk] = odd & (pw >= self.axis_min) & (pw <= self.axis_max)
        return out


# ------------------------------------------------------------------------------------------------ the nearest point
def _union_diagonal(boxes):
    span = torch.stack([b[1] for b in boxes]).amax(0).double() - torch.stack([b[0] for b in boxes]).amin(0).double()
    return float(span.norm()) * (1 + 2.0 ** -20)         # the float32 square stays above every distance


class PointGrid:
    """The built grid of one target cloud (include/ngp_hip.h M5), so that ICP builds it once: the finite points sorted
    by cell as 16-byte rows (x, y, z, bits of the original index), `order` (int32: sorted position -> original index)
    and the cells' offsets.  cell: the cell's edge; default: POINTS_PER_CELL points per cell if they were spread over
    the faces of their box, doubled while the grid exceeds 1024 cells per axis or 2^24 cells (a `cell` given by the
    caller is refused instead).  No result depends on it.  dropped: how many points were not finite."""

    def __init__(self, cloud, cell=None):
        _mesh._check_points(cloud)
        if cell is not None and not (float(cell) > 0 and np.isfinite(float(cell))):
            raise ValueError(f"cell must be positive, got {cell}")
        dev = cloud.device
        self.device = dev
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        finite = torch.isfinite(cloud).all(1)
        keep = torch.nonzero(finite).reshape(-1)
        self.dropped = int(cloud.shape[0] - keep.numel())
        points = cloud[keep] if self.dropped else cloud
        self.n = int(points.shape[0])
        self.cell = self.inv = self.dims = self.lo = self.hi = None
        self.origin = self.dims3 = self.cloud4 = self.offset = None
        self.centre = (C.c_float * 3)(0.0, 0.0, 0.0)
        self.order = torch.empty(0, dtype=torch.int32, device=dev)
        if self.n:
            self.lo, self.hi = (x.cpu().numpy() for x in torch.aminmax(points, dim=0))
            self.origin = (C.c_float * 3)(*[float(x) for x in self.lo])
            mid = 0.5 * (self.lo.astype(np.float64) + self.hi.astype(np.float64))
            self.centre = (C.c_float * 3)(*[float(x) for x in mid])
            if cell is not None:
                if not self.fits(self.shape(cell)[2]):
                    raise ValueError(f"cell {cell} needs a grid of {self.shape(cell)[2]} cells: more than "
                                     f"{_mesh.GRID_MAX_DIM} per axis or {_mesh.GRID_MAX_CELLS} in all")
            else:
                cell = self._default_cell()
                for _ in range(64):
                    if self.fits(self.shape(cell)[2]):
                        break
                    cell *= 2
            self.cell, self.inv, self.dims = self.shape(cell)
            self.dims3 = (C.c_int32 * 3)(*self.dims)
            keys = self.keys(points)
            by_cell = torch.argsort(keys, stable=True)
            cells = self.dims[0] * self.dims[1] * self.dims[2]
            self.offset = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
            self.offset[1:] = torch.cumsum(torch.bincount(keys, minlength=cells), 0)
            self.order = keep[by_cell].to(torch.int32)
            self.cloud4 = torch.empty(self.n, 4, dtype=_f32, device=dev)
            self.cloud4[:, :3] = points[by_cell]
            self.cloud4[:, 3] = self.order.view(_f32)
            self.occupied = int((self.offset[1:] > self.offset[:-1]).sum())
        torch.cuda.synchronize(dev)
        self.build_ms = 1e3 * (time.perf_counter() - t0)

    # the grid's f32 expressions are mesh._FaceGrid's: one copy of them
    shape = _mesh._FaceGrid.shape
    fits = staticmethod(_mesh._FaceGrid.fits)
    keys = _mesh._FaceGrid.keys

    @property
    def sorted_points(self):
        """the finite points sorted by cell, (n, 3) f32: a view of the 16-byte rows"""
        return self.cloud4[:, :3] if self.n else torch.empty(0, 3, dtype=_f32, device=self.device)

    def _default_cell(self):
        s = self.hi.astype(np.float64) - self.lo.astype(np.float64)
        area, extent = 2 * (s[0] * s[1] + s[1] * s[2] + s[2] * s[0]), float(s.max())
        if area > 0:
            cell = float(np.sqrt(POINTS_PER_CELL * area / self.n))
        elif extent > 0:
            cell = extent * POINTS_PER_CELL / self.n          # the points lie on a line
        else:
            cell = 1.0
        return max(cell, extent / _mesh.GRID_MAX_DIM, 1e-30)

    def sort_queries(self, queries, T=None):
        """-> the permutation that sorts the (transformed) queries by cell: locality for the query, nothing more"""
        if self.n == 0:
            return torch.arange(queries.shape[0], device=queries.device)
        return torch.argsort(self.keys(queries if T is None else transform_points(queries, T)))

    def launch(self, queries, max_dist, xform12=None, d2=None, index=None, partials=None):
        """one ngp_cloud_nearest over `queries` as they are ordered; outputs that are None are not written"""
        n = queries.shape[0]
        if partials is not None and (partials.dtype != torch.float64 or partials.numel() < -(-n // BLOCK) * SUMS):
            raise ValueError("partials must hold ceil(n / 256) rows of 18 float64")
        if self.n:
            grid = (self.cloud4, self.n, self.origin, self.inv, self.dims3, self.offset)
        else:
            grid = (None, 0, None, 1.0, None, None)
        call("cloud_nearest", queries, n, *grid, max_dist, xform12, self.centre if partials is not None else None, d2,
             index, partials)


def nearest_points(queries, cloud, max_dist=None, cell=None, transform=None, squared=False, stats=None):
    """The distance from each query to the nearest point of a cloud -> (dist (n,) f32, index (n,) int32 into `cloud`).

    Exact in the sense of include/ngp_hip.h M5: dist = sqrt(d2), d2 the smallest float32 squared distance to a finite
    point of the cloud, ties to the smaller index - what a brute force gives, bit for bit.  Queries farther than
    max_dist (or with a coordinate that is not finite) get dist = sqrt(max_dist^2 in f32) and index -1; max_dist=None
    takes the diagonal of the union bounding box times 1 + 2^-20, so nothing is clipped (with an empty cloud everything
    is).  transform: a 4x4 applied to the queries first (its upper 3x4 rounded to f32, the f32 expression of the
    header).  cloud: an (m, 3) f32 tensor or a PointGrid built from one (then `cell` must be None); points that are
    not finite are dropped and counted.  squared=True returns d2 itself.  A dict passed as `stats` receives cell,
    dims, references (the points in the grid), probes, dropped, occupied, build_ms and query_ms."""
    _mesh._check_points(queries)
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f"max_dist must be >= 0, got {max_dist}")
    if isinstance(cloud, PointGrid):
        if cell is not None:
            raise ValueError("cell belongs to the PointGrid that was built")
        grid, build_ms, probes = cloud, 0.0, 0
    else:
        grid = PointGrid(cloud, cell)
        build_ms, probes = grid.build_ms, 1 if grid.n else 0
    n, dev = queries.shape[0], queries.device
    T = None if transform is None else _matrix(transform)
    t1 = time.perf_counter()
    if max_dist is None:
        moved = queries if T is None else transform_points(queries, T)
        boxes = [torch.aminmax(moved, dim=0)] if n else []
        boxes += [(torch.from_numpy(grid.lo).to(dev), torch.from_numpy(grid.hi).to(dev))] if grid.n else []
        max_dist = _union_diagonal(boxes) if boxes else 0.0
        if not np.isfinite(max_dist):
            raise ValueError("the bounding box of queries and cloud is not finite: give max_dist")
    max_dist = float(np.float32(max_dist))
    d2 = torch.empty(n, dtype=_f32, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        order = grid.sort_queries(queries, T)
        d2_s, index_s = torch.empty_like(d2), torch.empty_like(index)
        grid.launch(queries[order].contiguous(), max_dist, None if T is None else _xform12(T), d2_s, index_s)
        d2[order] = d2_s
        index[order] = index_s
    torch.cuda.synchronize(dev)
    if stats is not None:
        stats.update(cell=grid.cell, dims=grid.dims, references=grid.n, probes=probes, dropped=grid.dropped,
                     occupied=getattr(grid, "occupied", 0), build_ms=build_ms,
                     query_ms=1e3 * (time.perf_counter() - t1))
    return (d2 if squared else torch.sqrt(d2)), index


def cloud_distance(points_a, points_b, thresholds=(), max_dist=None, stats=None):
    """How far cloud A (the reconstruction) is from cloud B (the reference): mesh.distance_metrics over the two
    directed nearest_points, unchanged - the keys of mesh.mesh_distance, reductions in float64 (clipped_a / clipped_b:
    the share of points beyond max_dist)."""
    ab, ba = {}, {}
    dist_a, index_a = nearest_points(points_a, points_b, max_dist=max_dist, stats=ab)
    dist_b, index_b = nearest_points(points_b, points_a, max_dist=max_dist, stats=ba)
    if stats is not None:
        stats.update(a_to_b=ab, b_to_a=ba)
    return _mesh.distance_metrics(dist_a, index_a, dist_b, index_b, thresholds)


# ---------------------------------------------------------------------------------------------------- down-sampling
def voxel_downsample(points, voxel, normals=None, colors=None, origin=None):
    """One point per occupied voxel: the mean of its points (and of their normals, not renormalised, and of their
    uint8 colours, rounded half away from zero), each added in the input's order in double (ngp_cloud_voxel_mean) ->
    (points (v,3) f32, normals or None, colors or None), voxels in rising order of (x, y, z) index.

    The voxel of a point is floor((p - origin) / voxel) per axis in float64 (origin: default the lower corner of the
    points).  Every point must be finite, and the key (x * dims_y + y) * dims_z + z must fit int64: a voxel edge too
    small for that raises ValueError."""
    _mesh._check_points(points)
    voxel = float(voxel)
    if not (voxel > 0 and np.isfinite(voxel)):
        raise ValueError(f"voxel must be positive, got {voxel}")
    n, dev = points.shape[0], points.device
    for name, attr, dtype in (("normals", normals, _f32), ("colors", colors, torch.uint8)):
        if attr is not None:
            check_input(attr, name)
            if attr.dtype != dtype or tuple(attr.shape) != (n, 3):
                raise ValueError(f"{name} must be an ({n}, 3) {dtype} tensor, got {tuple(attr.shape)} {attr.dtype}")
    if n == 0:
        return points.clone(), normals, colors
    if not bool(torch.isfinite(points).all()):
        raise ValueError("a point is not finite")
    p = points.double()
    lo = p.amin(0) if origin is None else torch.as_tensor(origin, dtype=torch.float64, device=dev).reshape(3)
    c = torch.floor((p - lo) / torch.tensor(voxel, dtype=torch.float64, device=dev))   # a true division, not * (1 / voxel)
    first, last = (x.cpu().numpy() for x in torch.aminmax(c, dim=0))
    dims = last - first + 1
    if not np.isfinite(dims).all() or float(dims[0]) * float(dims[1]) * float(dims[2]) >= 2.0 ** 63:
        raise ValueError(f"voxel {voxel} needs {dims.tolist()} voxels per axis: their keys do not fit int64")
    c = (c - torch.from_numpy(first).to(dev)).long()
    keys = (c[:, 0] * int(dims[1]) + c[:, 1]) * int(dims[2]) + c[:, 2]
    order = torch.argsort(keys, stable=True)
    _, counts = torch.unique_consecutive(keys[order], return_counts=True)
    n_voxels = int(counts.numel())
    offsets = torch.zeros(n_voxels + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    out_p = torch.empty(n_voxels, 3, dtype=_f32, device=dev)
    out_n = None if normals is None else torch.empty(n_voxels, 3, dtype=_f32, device=dev)
    out_c = None if colors is None else torch.empty(n_voxels, 3, dtype=torch.uint8, device=dev)
    call("cloud_voxel_mean", points[order].contiguous(), None if normals is None else normals[order].contiguous(),
         None if colors is None else colors[order].contiguous(), n, offsets, n_voxels, out_p, out_n, out_c)
    return out_p, out_n, out_c


# ----------------------------------------------------------------------------------------------------- registration
def kabsch(sums18, with_scale=False, centre=None):
    """The similarity q ~ s R p + t that fits the correspondences summed in `sums18` (the 18 doubles of
    ngp_cloud_sum_partials: count, sum p, sum q, sum p q^T row-major, sum |p|^2, sum d2) -> 4x4 float64.

    H = sum p q^T - count * mean_p mean_q^T; with H = U S V^T (np.linalg.svd), R = V diag(1, 1, det(V U^T)) U^T, so
    det R = +1 for a mirrored configuration too; s = trace(S diag(1, 1, det)) / (sum |p|^2 - count |mean_p|^2) with
    with_scale (Umeyama), else 1; t = mean_q - s R mean_p.  The sums are taken about `centre` (3 values; None: the
    origin) and the result maps uncentred points.  Fewer than 3 correspondences, or an H of rank below 2 (coincident
    or collinear points leave a rotation free; a planar set does not), raises ValueError.  Pure numpy."""
    s = np.asarray(sums18, np.float64).reshape(-1)
    if s.shape != (SUMS,):
        raise ValueError(f"sums18 must hold 18 values, got {s.shape}")
    count = s[0]
    if not count >= 3:
        raise ValueError(f"{int(count) if np.isfinite(count) else count} correspondences: at least 3 are needed")
    mean_p, mean_q = s[1:4] / count, s[4:7] / count
    H = s[7:16].reshape(3, 3) - count * np.outer(mean_p, mean_q)
    U, S, Vt = np.linalg.svd(H)
    if not (np.isfinite(S).all() and S[0] > 0 and S[1] > 1e-12 * S[0]):
        raise ValueError(f"the correspondences do not fix a rotation (singular values {S.tolist()})")
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    R = Vt.T @ D @ U.T
    scale = 1.0
    if with_scale:
        var = s[16] - count * float(mean_p @ mean_p)
        if not var > 0:
            raise ValueError("the source points coincide: no scale")
        scale = float((S * np.diag(D)).sum() / var)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mean_q - scale * R @ mean_p
    if centre is not None:
        c = np.asarray(list(centre), np.float64)
        T[:3, 3] += c - T[:3, :3] @ c
    return T


def icp(source, target, max_corr_dist, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, with_scale=False,
        grid=None):
    """Point-to-point ICP of `source` onto `target` -> (T 4x4 float64 with target ~ T source, info).

    The running transform is kept in float64 on the host and rounded to float32 once per iteration, for the kernel.
    An iteration is one ngp_cloud_nearest (no per-query output, the per-workgroup sums on), one ngp_cloud_sum_partials
    and one read of 18 doubles; kabsch() of those composes onto T.  init: any 4x4 (a scale included), applied through
    the same path.  The loop stops when fitness (the matched share of the source) and inlier_rmse both change by less
    than rel_fitness / rel_rmse between two evaluations (Open3D's criteria and defaults), or after max_iter updates;
    the returned fitness / inlier_rmse belong to the returned T.  info: fitness, inlier_rmse, iterations (updates),
    fitness_history, rmse_history (one entry per evaluation), iteration_ms (each, HIP events around the two launches),
    ms_per_iteration (their mean), dropped (source points that were not finite).  grid: the target's PointGrid, if the
    caller has it (`target` may then be None).  Fewer than 3 matches raise ValueError (kabsch)."""
    _mesh._check_points(source)
    if not (float(max_corr_dist) >= 0 and np.isfinite(float(max_corr_dist))):
        raise ValueError(f"max_corr_dist must be finite and >= 0, got {max_corr_dist}")
    if grid is None:
        grid = target if isinstance(target, PointGrid) else PointGrid(target)
    dev = source.device
    finite = torch.isfinite(source).all(1)
    dropped = int((~finite).sum())
    if dropped:
        source = source[finite]
    n = source.shape[0]
    if n == 0 or grid.n == 0:
        raise ValueError("icp needs points on both sides")
    T = _matrix(init)
    src = source[grid.sort_queries(source, T)].contiguous()       # sorted once: the transform moves little after that
    rows = -(-n // BLOCK)
    partials = torch.empty(rows, SUMS, dtype=torch.float64, device=dev)
    sums = torch.empty(SUMS, dtype=torch.float64, device=dev)
    max_dist = float(np.float32(max_corr_dist))
    fitness_h, rmse_h, ms = [], [], []
    iterations = 0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        grid.launch(src, max_dist, _xform12(T), partials=partials)
        call("cloud_sum_partials", partials, rows, sums)
        e1.record()
        s = sums.cpu().numpy()
        ms.append(e0.elapsed_time(e1))
        fitness_h.append(float(s[0]) / n)
        rmse_h.append(float(np.sqrt(s[17] / s[0])) if s[0] > 0 else 0.0)
        settled = len(fitness_h) > 1 and abs(fitness_h[-1] - fitness_h[-2]) < rel_fitness and \
            abs(rmse_h[-1] - rmse_h[-2]) < rel_rmse
        if settled or iterations >= max_iter:
            break
        T = kabsch(s, with_scale=with_scale, centre=grid.centre) @ T
        iterations += 1
    info = dict(fitness=fitness_h[-1], inlier_rmse=rmse_h[-1], iterations=iterations, fitness_history=fitness_h,
                rmse_history=rmse_h, iteration_ms=ms, ms_per_iteration=float(np.mean(ms)), dropped=dropped)
    return T, info


# the registration stages of the Tanks-and-Temples evaluation script, in units of dtau, as remembered: parity with the
# official toolbox is unpinned.  voxel: both clouds are voxel-down-sampled at that edge; max_points: both
# are thinned to every k-th point, k = max(1, n // max_points); corr: the correspondence distance.
TNT_STAGES = (dict(voxel=1.0, corr=80.0, max_iter=20),
              dict(voxel=0.5, corr=20.0, max_iter=20),
              dict(max_points=4_000_000, corr=2.0, max_iter=20))


def _keep(points, crop):
    return points if crop is None else points[crop.contains(points)].contiguous()


def tnt_score(recon_points, gt_points, dtau, init=None, crop=None, stages=TNT_STAGES, with_scale=False,
              thresholds=(), stats=None):
    """Precision / recall / F-score at dtau after the protocol's registration -> dict.

    The reconstruction is moved by the running transform (init first), cropped (crop: a CropVolume in the ground
    truth's frame, applied to both clouds) and registered stage by stage (`stages`, see TNT_STAGES); then both clouds
    are voxel-down-sampled at dtau / 2 and scored with cloud_distance at dtau (first) and any further `thresholds`;
    `stats` goes to cloud_distance.  Keys: precision, recall, fscore (floats, at dtau), transform (4x4 as lists, ground truth ~ transform * reconstruction), metrics (cloud_distance's dict),
    stages (per stage: fitness, inlier_rmse, iterations, ms_per_iteration, source_points, target_points, ms),
    points (recon, recon_cropped, recon_scored, gt, gt_cropped, gt_scored)."""
    dtau = float(dtau)
    if not (dtau > 0 and np.isfinite(dtau)):
        raise ValueError(f"dtau must be positive, got {dtau}")
    _mesh._check_points(recon_points)
    _mesh._check_points(gt_points)
    T = _matrix(init)
    gt = _keep(gt_points, crop)
    report = []
    for stage in stages:
        t0 = time.perf_counter()
        src = _keep(transform_points(recon_points, T), crop)
        dst = gt
        if stage.get("voxel"):
            src = voxel_downsample(src, stage["voxel"] * dtau)[0]
            dst = voxel_downsample(dst, stage["voxel"] * dtau)[0]
        if stage.get("max_points"):
            src = src[::max(1, src.shape[0] // int(stage["max_points"]))].contiguous()
            dst = dst[::max(1, dst.shape[0] // int(stage["max_points"]))].contiguous()
        step, info = icp(src, dst, stage["corr"] * dtau, max_iter=stage.get("max_iter", 20), with_scale=with_scale)
        T = step @ T
        torch.cuda.synchronize(recon_points.device)
        report.append(dict(fitness=info["fitness"], inlier_rmse=info["inlier_rmse"], iterations=info["iterations"],
                           ms_per_iteration=info["ms_per_iteration"], source_points=int(src.shape[0]),
                           target_points=int(dst.shape[0]), ms=1e3 * (time.perf_counter() - t0)))
    moved = _keep(transform_points(recon_points, T), crop)
    a = voxel_downsample(moved, dtau / 2)[0]
    b = voxel_downsample(gt, dtau / 2)[0]
    metrics = cloud_distance(a, b, thresholds=(dtau,) + tuple(t for t in thresholds if t != dtau), stats=stats)
    return dict(precision=metrics["precision"][0], recall=metrics["recall"][0], fscore=metrics["fscore"][0],
                transform=T.tolist(), metrics=metrics, stages=report,
                points=dict(recon=int(recon_points.shape[0]), recon_cropped=int(moved.shape[0]),
                            recon_scored=int(a.shape[0]), gt=int(gt_points.shape[0]), gt_cropped=int(gt.shape[0]),
                            gt_scored=int(b.shape[0])))
