"""Mesh export of a trained field: what the reference's extract_mesh.py does with skimage.measure.marching_cubes and
plyfile, on the GPU (libngp_hip.so: ngp_mc_count / ngp_mc_emit, include/ngp_hip.h M1) and with a PLY writer of our
own.

  marching_cubes(volume, level, spacing, origin) -> verts (V,3) f32, faces (F,3) i32 on the volume's device
  extract_mesh(model, ...)                        -> the same for NGP.density sampled on a dense lattice
                                                     (MC -> clean_mesh -> simplify_mesh -> normals -> colours)
  mesh_components(faces, n_verts)                 -> per-vertex component labels and faces per component (M2)
  clean_mesh(verts, faces, keep_largest=, min_faces=) -> the mesh without its small disconnected pieces (M2)
  simplify_mesh(verts, faces, cell= | target_faces=)  -> a smaller mesh: vertex clustering, quadric placement (M3)
  face_area_cdf / sample_surface(verts, faces, n, seed) -> n area-weighted surface points and their faces (M4)
  closest_on_mesh(points, verts, faces, max_dist=)    -> exact distance to the mesh and the closest face (M4)
  mesh_distance(verts_a, faces_a, verts_b, faces_b)   -> accuracy, completeness, Chamfer, Hausdorff, F-score (M4)
  vertex_colors(model, verts, normals, offset)    -> (V,3) uint8 colours rendered by the test-time marcher
  write_ply(path, verts, faces, normals, colors) / read_ply(path, colors=False)

Triangles are wound so that (v1-v0) x (v2-v0) points toward lower density (out of the object).  Ambiguous cell faces
are resolved by one face-local rule (inside corners are separated), so closed surfaces come out as closed 2-manifolds;
the triangle order and the ambiguity choices are not skimage's (Lewiner) ones.
"""
import ctypes as C
import time

import numpy as np
import torch

from ._lib import call, call_host, check_input

_f32 = torch.float32


def _vec3(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).tolist()
    v = [float(a) for a in v]
    if len(v) != 3:
        raise ValueError(f"expected 3 values, got {len(v)}")
    return v


def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """volume (nx, ny, nz) f32 CUDA tensor, C order (meshgrid indexing='ij') -> verts (V,3) f32, faces (F,3) int32,
    both on the volume's device.  Inside iff v > level (NaN and v == level are outside); a vertex on the lattice edge
    from idx along axis a lies at origin + (idx + t*e_a) * spacing, t = (level-v0)/(v1-v0) clamped to [0,1].
    Runs count -> emit on the current stream and reads the two totals back once (to size the outputs)."""
    check_input(volume, "volume")
    if volume.dtype != _f32 or volume.dim() != 3:
        raise ValueError(f"volume must be a 3-D float32 tensor, got {tuple(volume.shape)} {volume.dtype}")
    nx, ny, nz = volume.shape
    dev = volume.device
    spacing, origin = _vec3(spacing), _vec3(origin)
    if min(nx, ny, nz) < 2:
        return torch.empty(0, 3, dtype=_f32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
    n_ws = call_host("mc_workspace", nx, ny, nz)
    if n_ws < 0:
        raise ValueError(f"lattice {tuple(volume.shape)} has 2^31 points or more")
    ws = torch.empty(n_ws, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    call("mc_count", volume, nx, ny, nz, float(level), ws, totals)
    n_v, n_f = totals.tolist()
    if n_v < 0 or n_f < 0:
        raise RuntimeError(f"marching cubes on {tuple(volume.shape)}: more than 2^31-1 vertices or triangles")
    verts = torch.empty(n_v, 3, dtype=_f32, device=dev)
    faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_v:
        call("mc_emit", volume, nx, ny, nz, float(level), (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), ws,
             verts, faces)
    return verts, faces


def lattice_axes(lo, hi, resolution, device):
    """the sample coordinates of each axis: torch.linspace(lo, hi, n), as the reference's extract_mesh.py"""
    n = (resolution,) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    if len(n) != 3 or min(n) < 2:
        raise ValueError(f"resolution must be an int or 3 ints, each >= 2: {resolution}")
    return n, [torch.linspace(lo[a], hi[a], n[a], device=device) for a in range(3)]


def lattice_spacing(lo, hi, n, reference_spacing=False):
    """extent/(n-1) per axis (where linspace put the samples), or extent/n (the reference's extract_mesh.py)"""
    return [(hi[a] - lo[a]) / (n[a] if reference_spacing else n[a] - 1) for a in range(3)]


@torch.no_grad()
def density_volume(model, lo, hi, resolution=512, chunk=128 ** 3):
    """NGP.density(x, grad=False) (grid_fwd + mlp2_fwd) on the lattice linspace(lo, hi, n) per axis -> (nx, ny, nz)
    f32 on the model's device.  The points are made chunk by chunk on the device (never the whole lattice at once)."""
    dev = model.xyz_min.device
    n, axes = lattice_axes(lo, hi, resolution, dev)
    vol = torch.empty(n, dtype=_f32, device=dev)
    flat = vol.view(-1)
    nyz = n[1] * n[2]
    for s in range(0, flat.numel(), chunk):
        idx = torch.arange(s, min(s + chunk, flat.numel()), device=dev)
        i = idx // nyz
        r = idx - i * nyz
        j = r // n[2]
        pts = torch.stack((axes[0][i], axes[1][j], axes[2][r - j * n[2]]), -1)
        flat[s:s + pts.shape[0]] = model.density(pts, grad=False)
    return vol


@torch.no_grad()
def vertex_normals(model, verts, chunk=128 ** 3):
    """-grad(sigma)/|grad(sigma)| at each vertex through NGP.grad (the analytic gradient of the field), chunked;
    (0,0,0) where the gradient vanishes"""
    out = torch.empty_like(verts)
    for s in range(0, verts.shape[0], chunk):
        _, _, g = model.grad(verts[s:s + chunk].contiguous())
        out[s:s + chunk] = -torch.nn.functional.normalize(g, dim=-1)
    return out


def extract_mesh(model, xyz_min=None, xyz_max=None, resolution=512, level=10.0, chunk=128 ** 3, normals=False,
                 reference_spacing=False, keep_largest=None, min_faces=None, colors=False, color_offset=None,
                 simplify_cell=None, target_faces=None, placement='quadric', stats=None):
    """Mesh of the level set {sigma = level} of `model` (an NGP) -> verts (V,3), faces (F,3) [, normals (V,3)].

    The lattice spans [xyz_min, xyz_max] (default: the model's own box) with `resolution` (an int or (nx, ny, nz))
    points per axis at torch.linspace positions, i.e. a spacing of extent/(n-1); the density is evaluated in chunks of
    `chunk` points.  By default vertices lie where the density was sampled (origin xyz_min, spacing extent/(n-1)).

    reference_spacing=True reproduces the placement of the reference's extract_mesh.py: it samples at extent/(n-1) but
    hands skimage a spacing of extent/n, so its meshes are shrunk by (n-1)/n toward xyz_min (v_ref - lo =
    (v - lo) * (n-1)/n).  Its own call is xyz_min=(-1,-0.3,-1), xyz_max=(1,0.15,1), resolution=(512,128,512),
    level=10.

    normals=True adds per-vertex unit normals -grad(sigma)/|grad(sigma)| (pointing out of the object).

    keep_largest / min_faces remove small disconnected pieces (clean_mesh) before normals and colours are computed.
    colors=True adds per-vertex uint8 RGB (vertex_colors) rendered from color_offset (default: twice the largest
    lattice spacing) outside each vertex.

    simplify_cell=X or target_faces=N (one of them) simplifies the cleaned mesh (simplify_mesh, cells from the
    lattice's xyz_min, `placement`) before normals and colours, which are then evaluated on the field at the new
    vertices (nothing is averaged); a dict passed as `stats` receives simplify_mesh's stats.
    The result is (verts, faces[, normals][, colors])."""
    if simplify_cell is not None and target_faces is not None:
        raise ValueError("give at most one of simplify_cell and target_faces")
    lo = _vec3(model.xyz_min if xyz_min is None else xyz_min)
    hi = _vec3(model.xyz_max if xyz_max is None else xyz_max)
    vol = density_volume(model, lo, hi, resolution, chunk)
    spacing = lattice_spacing(lo, hi, vol.shape, reference_spacing)
    verts, faces = marching_cubes(vol, level, spacing, lo)
    del vol
    if keep_largest is not None or min_faces is not None:
        verts, faces = clean_mesh(verts, faces, keep_largest=keep_largest, min_faces=min_faces)
    if simplify_cell is not None or target_faces is not None:
        verts, faces = simplify_mesh(verts, faces, cell=simplify_cell, target_faces=target_faces, origin=lo,
                                     placement=placement, stats=stats)
    out = [verts, faces]
    nrm = vertex_normals(model, verts, chunk) if normals or colors else None
    if normals:
        out.append(nrm)
    if colors:
        out.append(vertex_colors(model, verts, nrm, 2 * max(spacing) if color_offset is None else color_offset))
    return tuple(out)


# ------------------------------------------------------------------------------------------------- cleaning (M2)
def _check_faces(faces, n_verts):
    check_input(faces, "faces")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an (F, 3) int32 tensor, got {tuple(faces.shape)} {faces.dtype}")
    n_verts = int(n_verts)
    if n_verts < 0 or n_verts > 2 ** 31 - 1 or faces.shape[0] > (2 ** 31 - 1) // 3:
        raise ValueError(f"unsupported mesh size: {n_verts} vertices, {faces.shape[0]} faces")
    if faces.shape[0]:
        lo, hi = torch.aminmax(faces)
        if int(lo) < 0 or int(hi) >= n_verts:
            raise ValueError(f"face indices span [{int(lo)}, {int(hi)}], outside [0, {n_verts})")
    return n_verts


def label_round_bound(n_verts):
    """the most label rounds component_labels runs before it gives up (each round at least halves the longest label
    chain of a path; the margin covers what hooking adds)"""
    return 64 + 2 * int(n_verts).bit_length()


def component_labels(faces, n_verts, max_rounds=None):
    """faces (F,3) int32 CUDA tensor over n_verts vertices -> (labels (V,) int32, rounds): labels[v] is the smallest
    vertex index of v's component (faces sharing a vertex are connected; a vertex in no face keeps its own index), the
    same from run to run.  Runs ngp_mesh_labels_round until a round changes nothing, reading one word back per round;
    raises RuntimeError if that takes more than max_rounds (default label_round_bound(n_verts)) rounds."""
    n_verts = _check_faces(faces, n_verts)
    n_faces = faces.shape[0]
    labels = torch.empty(n_verts, dtype=torch.int32, device=faces.device)
    if n_verts == 0:
        return labels, 0
    call("mesh_labels_init", labels, n_verts)
    if n_faces == 0:
        return labels, 0
    bound = label_round_bound(n_verts) if max_rounds is None else int(max_rounds)
    changed = torch.zeros(max(bound, 1), dtype=torch.int32, device=faces.device)
    for r in range(bound):
        call("mesh_labels_round", faces, n_faces, n_verts, labels, changed[r:])
        if not int(changed[r]):
            return labels, r + 1
    raise RuntimeError(f"connected components of {n_verts} vertices / {n_faces} faces did not settle in {bound} rounds")


def mesh_components(faces, n_verts):
    """-> labels (V,) int32 (component_labels) and face_counts (V,) int32: the faces of each component at its label's
    slot, 0 at every other slot"""
    labels, _ = component_labels(faces, n_verts)
    counts = torch.zeros_like(labels)
    if labels.numel():
        call("mesh_face_counts", faces, faces.shape[0], labels.numel(), labels, counts)
    return labels, counts


def select_components(face_counts, keep_largest=None, min_faces=None):
    """-> keep (V,) uint8 indexed by label: 1 for each component with faces that meets every criterion given
    (keep_largest=k: among the k components with the most faces, ties to the smaller label; min_faces=m: at least m
    faces)"""
    keep = face_counts > 0
    if min_faces is not None:
        if int(min_faces) < 0:
            raise ValueError(f"min_faces must be >= 0, got {min_faces}")
        keep &= face_counts >= int(min_faces)
    if keep_largest is not None:
        if int(keep_largest) < 0:
            raise ValueError(f"keep_largest must be >= 0, got {keep_largest}")
        roots = torch.nonzero(face_counts > 0).squeeze(1)                 # ascending labels
        c = face_counts[roots].cpu().numpy()                               # C components: ranked on the host
        order = np.lexsort((np.arange(c.size), -c.astype(np.int64)))[:int(keep_largest)]
        top = torch.zeros_like(keep)
        top[roots[torch.from_numpy(order).to(roots.device)]] = True
        keep &= top
    return keep.to(torch.uint8)


def clean_mesh(verts, faces, *, normals=None, colors=None, keep_largest=None, min_faces=None, stats=None):
    """Drops the components that fail the criteria of select_components -> (verts, faces[, normals][, colors]).

    Labels, sizes and compaction run in libngp_hip.so (M2): kept vertices (those some kept face uses) and kept faces
    keep their original order, faces are renumbered, and normals / colors rows (any (V, ...) tensors) follow their
    vertices.  With no criterion, every component with a face is kept (only vertices no face uses go).  A dict passed
    as `stats` receives rounds, components (those with faces), components_kept, V_removed and F_removed."""
    check_input(verts, "verts")
    if verts.dtype != _f32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be a (V, 3) float32 tensor, got {tuple(verts.shape)} {verts.dtype}")
    n_verts, n_faces = verts.shape[0], faces.shape[0]
    attrs = [a for a in (normals, colors) if a is not None]
    for name, a in (("normals", normals), ("colors", colors)):
        if a is not None:
            check_input(a, name)
            if a.shape[0] != n_verts:
                raise ValueError(f"{name} has {a.shape[0]} rows for {n_verts} vertices")
    labels, rounds = component_labels(faces, n_verts)
    counts = torch.zeros_like(labels)
    if n_verts:
        call("mesh_face_counts", faces, n_faces, n_verts, labels, counts)
    keep = select_components(counts, keep_largest, min_faces)
    out, f_out = _compact([verts] + attrs, faces, labels, counts, keep)
    if stats is not None:
        stats.update(rounds=rounds, components=int((counts > 0).sum()), components_kept=int(keep.sum()),
                     V_removed=n_verts - out[0].shape[0], F_removed=n_faces - f_out.shape[0])
    return (out[0], f_out, *out[1:])


def _compact(rows, faces, labels, counts, keep):
    """ngp_mesh_compact_*: the faces whose label is kept and the vertices those use (keep[label] and counts[label] >
    0), in their original order; rows is a list of (V, ...) per-vertex arrays -> (their kept rows, faces renumbered)"""
    n_verts, n_faces = labels.shape[0], faces.shape[0]
    dev = faces.device
    ws = torch.empty(call_host("mesh_clean_workspace", n_verts, n_faces), dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    if n_verts:
        call("mesh_compact_count", faces, n_faces, n_verts, labels, counts, keep, ws, totals)
    n_v, n_f = totals.tolist()
    out = [torch.empty((n_v,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device) for a in rows]
    for src, dst in zip(rows, out):
        if n_v:
            row_bytes = src[0].numel() * src.element_size()
            call("mesh_compact_rows", src, row_bytes, n_verts, n_faces, ws, dst)
    f_out = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_f:
        call("mesh_compact_faces", faces, n_faces, n_verts, ws, f_out)
    return out, f_out


# ------------------------------------------------------------------------------------------- simplification (M3)
MAX_CELLS = 1 << 20   # the most cells along the longest axis that target_faces tries


def _check_mesh(verts, faces, normals, colors):
    check_input(verts, "verts")
    if verts.dtype != _f32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must be a (V, 3) float32 tensor, got {tuple(verts.shape)} {verts.dtype}")
    _check_faces(faces, verts.shape[0])
    for name, a, dtype in (("normals", normals, _f32), ("colors", colors, torch.uint8)):
        if a is not None:
            check_input(a, name)
            if a.dtype != dtype or tuple(a.shape) != (verts.shape[0], 3):
                raise ValueError(f"{name} must be a ({verts.shape[0]}, 3) {dtype} tensor, got {tuple(a.shape)} "
                                 f"{a.dtype}")


class _Clustering:
    """the count-only path of ngp_mesh_simplify_*: one workspace, one call and one read-back per cell size"""

    def __init__(self, verts, faces, origin):
        self.verts, self.faces = verts, faces
        self.n_verts, self.n_faces = verts.shape[0], faces.shape[0]
        self.origin = (C.c_float * 3)(*origin)
        n_ws = call_host("mesh_simplify_workspace", self.n_verts, self.n_faces)
        if n_ws < 0:
            raise ValueError(f"unsupported mesh size: {self.n_verts} vertices, {self.n_faces} faces")
        self.ws = torch.empty(n_ws, dtype=torch.int32, device=verts.device)
        self.totals = torch.zeros(4, dtype=torch.int32, device=verts.device)
        self.cell = None

    def count(self, cell):
        """-> (clusters, kept faces, degenerate faces) for cells of size float32(cell) from the origin"""
        cell = np.float32(cell)
        with np.errstate(all="ignore"):
            inv = np.float32(1) / cell
        if not (cell > 0 and np.isfinite(cell) and np.isfinite(inv)):
            raise ValueError(f"cell must be a positive float32 with a finite inverse, got {cell}")
        self.cell, self.inv = float(cell), float(inv)
        call("mesh_simplify_count", self.verts, self.n_verts, self.faces, self.n_faces, self.origin, self.inv, self.ws,
             self.totals)
        clusters, kept, degenerate, err = self.totals.tolist()
        if err & 1:
            raise ValueError(f"a vertex is not finite, or its cell lies outside [0, 2^21) per axis (cell {cell}, "
                             f"origin {list(self.origin)})")
        if err:
            raise RuntimeError("ngp_mesh_simplify_count: a hash table had no room")
        return clusters, kept, degenerate


def _search_cells(clustering, extent, target_faces):
    """the number of cells k along the longest axis (cell = float32(extent / k)) for target_faces: k doubles from 1
    until more than target_faces faces are kept (or nothing merges any more, or k = MAX_CELLS), then a bisection
    finds a k that keeps <= target_faces faces while k + 1 keeps more -> (k, probes); k = 0 when even k = 1 keeps too
    many (vertices exactly on the upper faces of the bounding box open a second layer of cells)"""
    probes, k, lo, hi = 0, 1, 0, None
    while True:
        clusters, kept, _ = clustering.count(extent / k)
        probes += 1
        if kept > target_faces:
            hi = k
            break
        lo = k
        if clusters == clustering.n_verts or k >= MAX_CELLS:
            break
        k *= 2
    while hi is not None and hi - lo > 1:
        mid = (lo + hi) // 2
        kept = clustering.count(extent / mid)[1]
        probes += 1
        lo, hi = (mid, hi) if kept <= target_faces else (lo, mid)
    return lo, probes


def simplify_mesh(verts, faces, *, cell=None, target_faces=None, origin=None, placement='quadric', regularization=1e-3,
                  normals=None, colors=None, stats=None):
    """Uniform vertex clustering with quadric placement (M3) -> (verts, faces[, normals][, colors]).

    Vertices whose key floorf((v - origin) * (1/cell)) (float32, per axis) agrees form a cluster; clusters are numbered
    by their smallest member.  Each cluster becomes one vertex: placement='mean' puts it at the members' mean;
    'quadric' at the minimiser of the squared distances to the planes of the faces at its members, weighted by squared
    face area and regularised toward the mean (lambda = regularization * trace / 3), clamped to the cell, so creases
    and corners stay where a mean rounds them off.  Faces are renumbered; a face with two corners in one cluster is
    dropped (`degenerate`), as is every face but the first of each unordered corner triple (`duplicate`); kept faces
    keep order and winding, and clusters no kept face uses are dropped.  Every vertex moves by at most the cell's
    diagonal.  The mesh need not stay manifold.  normals (V,3) f32 / colors (V,3) uint8 are averaged per cluster
    (normalised / rounded).  All sums run in double in a fixed order: the result is the same from run to run.

    Exactly one of cell (> 0) and target_faces (>= 0).  target_faces=N picks cell = float32(longest bounding-box
    extent / k) by the search of _search_cells (count-only passes) so that at most N faces are kept; a mesh that has
    no more than N faces comes back unchanged.  origin defaults to verts.amin(0); keys must lie in [0, 2^21).
    A dict passed as `stats` receives cell, k and probes (None / 0 without target_faces), clusters, V_in, V_out, F_in,
    F_out, degenerate, duplicate, and probe_ms / emit_ms (host clocks around device synchronisation)."""
    _check_mesh(verts, faces, normals, colors)
    if (cell is None) == (target_faces is None):
        raise ValueError("give exactly one of cell and target_faces")
    if placement not in ('quadric', 'mean'):
        raise ValueError(f"placement must be 'quadric' or 'mean', got {placement!r}")
    if not (regularization > 0 and np.isfinite(regularization)):
        raise ValueError(f"regularization must be positive, got {regularization}")
    if cell is not None and not (float(cell) > 0 and np.isfinite(float(cell))):
        raise ValueError(f"cell must be positive, got {cell}")
    if target_faces is not None and int(target_faces) < 0:
        raise ValueError(f"target_faces must be >= 0, got {target_faces}")
    n_verts, n_faces = verts.shape[0], faces.shape[0]
    dev = verts.device
    attrs = [a for a in (normals, colors) if a is not None]
    info = dict(cell=None, k=None, probes=0, clusters=n_verts, V_in=n_verts, V_out=n_verts, F_in=n_faces,
                F_out=n_faces, degenerate=0, duplicate=0, probe_ms=0.0, emit_ms=0.0)

    def done(out_v, out_f, out_attrs):
        info.update(V_out=out_v.shape[0], F_out=out_f.shape[0])
        if stats is not None:
            stats.update(info)
        return (out_v, out_f, *out_attrs)

    def nothing():
        return done(verts[:0].clone(), faces[:0].clone(), [a[:0].clone() for a in attrs])

    if n_verts == 0:
        return nothing()
    if target_faces is not None and n_faces <= int(target_faces):
        return done(verts, faces, attrs)
    lo, hi = torch.aminmax(verts, dim=0)
    if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("verts holds a value that is not finite")
    origin = _vec3(lo if origin is None else origin)
    clustering = _Clustering(verts, faces, origin)
    t0 = time.perf_counter()
    if target_faces is not None:
        extent = float((hi - lo).max())
        if not np.isfinite(extent):
            raise ValueError("the bounding box of verts is not finite")
        extent = extent if extent > 0 else 1.0     # one point: every cell size merges everything
        k, probes = _search_cells(clustering, extent, int(target_faces))
        info.update(k=k, probes=probes)
        if k == 0:
            return nothing()
        cell = extent / k
    info["probe_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    # the workspace holds the last probe's tables: count once more at the chosen cell, then emit from it
    clusters, kept, degenerate = clustering.count(cell)
    info.update(cell=clustering.cell, clusters=clusters, degenerate=degenerate, duplicate=n_faces - degenerate - kept)
    if kept == 0:
        return nothing()
    vert_cluster = torch.empty(n_verts, dtype=torch.int32, device=dev)
    corner_cluster = torch.empty(3 * n_faces, dtype=torch.int32, device=dev)
    call("mesh_simplify_groups", faces, n_faces, n_verts, clustering.ws, vert_cluster, corner_cluster)
    # members of a cluster side by side, in ascending index order: one stable sort per array
    sorted_v, order_v = torch.sort(vert_cluster, stable=True)
    sorted_c, order_c = torch.sort(corner_cluster, stable=True)
    order_v, order_c = order_v.to(torch.int32), order_c.to(torch.int32)
    rows = [torch.empty(clusters, 3, dtype=_f32, device=dev)]
    rows += [torch.empty(clusters, 3, dtype=a.dtype, device=dev) for a in attrs]
    call("mesh_simplify_place", verts, n_verts, faces, n_faces, clustering.origin, clustering.cell, clustering.inv,
         float(regularization), int(placement == 'quadric'), clusters, sorted_v, order_v, sorted_c, order_c,
         normals, colors, rows[0], rows[1] if normals is not None else None,
         rows[-1] if colors is not None else None)
    kept_faces = torch.empty(kept, 3, dtype=torch.int32, device=dev)
    used = torch.zeros(clusters, dtype=torch.int32, device=dev)
    call("mesh_simplify_faces", faces, n_faces, n_verts, clustering.ws, kept_faces, used)
    # clusters that no kept face uses go, as in clean_mesh without a criterion: every cluster is its own label
    labels = torch.empty(clusters, dtype=torch.int32, device=dev)
    call("mesh_labels_init", labels, clusters)
    out, f_out = _compact(rows, kept_faces, labels, used, torch.ones(clusters, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize(dev)
    info["emit_ms"] = 1e3 * (time.perf_counter() - t0)
    return done(out[0], f_out, out[1:])


# ----------------------------------------------------------------------------------------------- evaluation (M4)
GRID_MAX_DIM = 1024          # cells per axis, cells and references ngp_mesh_grid_* / ngp_mesh_closest take
GRID_MAX_CELLS = 1 << 24
GRID_MAX_REFS = 1 << 28
GRID_MAX_PROBES = 32         # count passes while the references do not fit
MAX_SAMPLES = 1 << 30


def _check_points(points):
    check_input(points, "points")
    if points.dtype != _f32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be an (n, 3) float32 tensor, got {tuple(points.shape)} {points.dtype}")
    if points.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"unsupported number of points: {points.shape[0]}")


def face_area_cdf(verts, faces):
    """-> (F,) float64: the inclusive running sum of the face areas 0.5 |(v1 - v0) x (v2 - v0)|, taken in double"""
    _check_mesh(verts, faces, None, None)
    v = verts.double()
    a, b, c = (v[faces[:, k].long()] for k in range(3))
    return torch.cumsum(0.5 * torch.linalg.cross(b - a, c - a, dim=1).norm(dim=1), 0)


def sample_surface(verts, faces, n, seed=0, cdf=None):
    """n points on the surface, uniform by area -> (points (n,3) f32, face (n,) int32: the face each lies on).

    Sample i is a function of (seed, i) alone (ngp_mesh_sample_surface, include/ngp_hip.h M4): the same bytes from run
    to run, and the first n samples of a longer run.  cdf: face_area_cdf(verts, faces) if the caller has it.  Faces
    without area are never drawn; a mesh without area is refused."""
    _check_mesh(verts, faces, None, None)
    n = int(n)
    if n < 0 or n > MAX_SAMPLES:
        raise ValueError(f"n must lie in [0, 2^30], got {n}")
    dev = verts.device
    points = torch.empty(n, 3, dtype=_f32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return points, face
    n_faces = faces.shape[0]
    if cdf is None:
        cdf = face_area_cdf(verts, faces)
    check_input(cdf, "cdf")
    if cdf.dtype != torch.float64 or tuple(cdf.shape) != (n_faces,):
        raise ValueError(f"cdf must be a ({n_faces},) float64 tensor, got {tuple(cdf.shape)} {cdf.dtype}")
    total = float(cdf[-1]) if n_faces else 0.0
    if not (total > 0 and np.isfinite(total)):
        raise ValueError(f"the mesh has no area to sample (total {total}, {n_faces} faces)")
    call("mesh_sample_surface", verts, verts.shape[0], faces, n_faces, cdf, total, n, int(seed) & 0xFFFFFFFF, points,
         face)
    return points, face


class _FaceGrid:
    """the uniform grid of face references ngp_mesh_closest walks: cells of one size from the mesh's lower corner"""

    def __init__(self, verts, faces, lo, hi):
        self.verts, self.faces = verts, faces
        self.lo, self.hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        self.origin = (C.c_float * 3)(*[float(x) for x in self.lo])
        self.totals = torch.zeros(2, dtype=torch.int64, device=verts.device)
        self.probes = 0

    def shape(self, cell):
        """-> (float32 cell, its float32 inverse, dims): dims[a] = the upper corner's cell coordinate + 1, by the
        kernels' own f32 expression, so every vertex falls inside"""
        cell = np.float32(cell)
        with np.errstate(all="ignore"):
            inv = np.float32(1) / cell
            dims = np.floor((self.hi - self.lo) * inv) + 1
        if not (cell > 0 and np.isfinite(cell) and np.isfinite(inv) and np.isfinite(dims).all()):
            raise ValueError(f"cell must be a positive float32 with a finite inverse, got {cell}")
        return float(cell), float(inv), [int(d) for d in dims]

    @staticmethod
    def fits(dims):
        return max(dims) <= GRID_MAX_DIM and dims[0] * dims[1] * dims[2] <= GRID_MAX_CELLS

    def count(self, cell):
        """one count pass at this cell (its dims must fit) -> references; the per-cell counts stay in self.counts"""
        self.cell, self.inv, self.dims = self.shape(cell)
        self.dims3 = (C.c_int32 * 3)(*self.dims)
        self.counts = torch.zeros(self.dims[0] * self.dims[1] * self.dims[2], dtype=torch.int32,
                                  device=self.verts.device)
        call("mesh_grid_count", self.verts, self.verts.shape[0], self.faces, self.faces.shape[0], self.origin, self.inv,
             self.dims3, self.counts, self.totals)
        self.probes += 1
        refs, err = self.totals.tolist()
        if err & 1:
            raise ValueError("a face has a vertex that is not finite")
        if err:
            raise RuntimeError(f"ngp_mesh_grid_count: a face lies outside the grid (cell {self.cell}, dims {self.dims})")
        return refs

    def fill(self, refs):
        dev = self.verts.device
        self.offset = torch.zeros(self.counts.numel() + 1, dtype=torch.int32, device=dev)
        self.offset[1:] = torch.cumsum(self.counts, 0)
        self.refs = torch.empty(max(refs, 1), dtype=torch.int32, device=dev)
        self.counts.zero_()     # now the cursors
        call("mesh_grid_fill", self.verts, self.verts.shape[0], self.faces, self.faces.shape[0], self.origin, self.inv,
             self.dims3, self.offset, self.counts, self.refs)

    def keys(self, points):
        """the index of each point's cell (clamped to the grid): what the points are sorted by, nothing more"""
        lo = torch.tensor(self.lo, device=points.device)
        c = torch.nan_to_num(torch.floor((points - lo) * self.inv), nan=0.0)
        top = torch.tensor([d - 1 for d in self.dims], dtype=_f32, device=points.device)
        c = torch.minimum(c.clamp_min(0), top).long()
        return (c[:, 0] * self.dims[1] + c[:, 1]) * self.dims[2] + c[:, 2]


def _start_cell(verts, faces, lo, hi, max_dist):
    """twice the mean edge length: a handful of faces per cell and per face a handful of cells; with a max_dist
    below that, max_dist itself but no less than one mean edge (the walk ends after ceil(max_dist / cell) + 1 rings
    anyway, and faces span the cells whatever their size)"""
    v = verts.double()
    a, b, c = (v[faces[:, k].long()] for k in range(3))
    edge = float(((b - a).norm(dim=1) + (c - b).norm(dim=1) + (a - c).norm(dim=1)).mean()) / 3
    extent = float(np.max(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    if not (edge > 0 and np.isfinite(edge)):
        edge = extent / 128 if extent > 0 else 1.0
    cell = 2 * edge
    if max_dist is not None and np.isfinite(max_dist):
        cell = min(cell, max(float(max_dist), edge))
    return max(cell, extent / GRID_MAX_DIM)


def closest_on_mesh(points, verts, faces, max_dist=None, cell=None, stats=None, squared=False):
    """The distance from each point to the mesh -> (dist (n,) f32, face (n,) int32: the closest face).

    Exact in the sense of include/ngp_hip.h M4: dist = sqrt(d2), d2 the smallest float32 squared distance to any face
    with a non-zero cross product (Ericson's closest point on a triangle), ties to the smaller face index - what a
    brute force over all faces gives, bit for bit.  Points farther than max_dist get dist = sqrt(max_dist^2 in f32)
    and face -1; max_dist=None takes the diagonal of the union bounding box, so nothing is clipped (with no face,
    everything is).  The faces go into a uniform grid (cell: its size, default _start_cell, doubled while the grid
    exceeds 1024 cells per axis, 2^24 cells or, found by at most 32 count passes, 2^28 references; a `cell` given
    by the caller is refused instead), the points are sorted by cell for the query and the outputs put back.
    squared=True returns d2 itself in place of dist.  A dict passed as `stats` receives cell, dims, references, probes,
    build_ms and query_ms (host clocks around device synchronisation)."""
    _check_points(points)
    _check_mesh(verts, faces, None, None)
    n, n_faces = points.shape[0], faces.shape[0]
    dev = points.device
    info = dict(cell=None, dims=None, references=0, probes=0, build_ms=0.0, query_ms=0.0)
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f"max_dist must be >= 0, got {max_dist}")
    if cell is not None and not (float(cell) > 0 and np.isfinite(float(cell))):
        raise ValueError(f"cell must be positive, got {cell}")
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    lo = hi = None
    if n_faces:
        used = verts[faces.reshape(-1).long()]
        lo, hi = (x.cpu().numpy() for x in torch.aminmax(used, dim=0))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("a face has a vertex that is not finite")
    if max_dist is None:
        boxes = [torch.aminmax(points, dim=0)] if n else []
        boxes += [(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))] if n_faces else []
        if boxes:
            span = torch.stack([b[1] for b in boxes]).amax(0).double() - torch.stack([b[0] for b in boxes]).amin(0).double()
            max_dist = float(span.norm()) * (1 + 2.0 ** -20)     # the float32 square stays above every distance
        else:
            max_dist = 0.0
        if not np.isfinite(max_dist):
            raise ValueError("the bounding box of points and mesh is not finite: give max_dist")
    max_dist = float(np.float32(max_dist))
    grid = None
    if n_faces:
        grid = _FaceGrid(verts, faces, lo, hi)
        if cell is not None:
            if not grid.fits(grid.shape(cell)[2]):
                raise ValueError(f"cell {cell} needs a grid of {grid.shape(cell)[2]} cells: more than {GRID_MAX_DIM} "
                                 f"per axis or {GRID_MAX_CELLS} in all")
            refs = grid.count(cell)
            if refs > GRID_MAX_REFS:
                raise ValueError(f"cell {cell} needs {refs} face references, more than {GRID_MAX_REFS}")
        else:
            cell = _start_cell(verts, faces, lo, hi, max_dist)
            for _ in range(64):                       # sizes alone: no pass over the mesh
                if grid.fits(grid.shape(cell)[2]):
                    break
                cell *= 2
            for _ in range(GRID_MAX_PROBES):
                refs = grid.count(cell)
                if refs <= GRID_MAX_REFS:
                    break
                cell *= 2
            else:
                raise RuntimeError(f"no cell up to {cell} keeps the face references below {GRID_MAX_REFS}")
        grid.fill(refs)
        info.update(cell=grid.cell, dims=grid.dims, references=refs, probes=grid.probes)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    d2 = torch.empty(n, dtype=_f32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        if grid is None:
            call("mesh_closest", points, n, None, verts.shape[0], None, 0, None, 1.0, None, None, None, max_dist, d2,
                 face)
        else:
            order = torch.argsort(grid.keys(points))
            d2_s, face_s = torch.empty_like(d2), torch.empty_like(face)
            call("mesh_closest", points[order].contiguous(), n, verts, verts.shape[0], faces, n_faces, grid.origin,
                 grid.inv, grid.dims3, grid.offset, grid.refs, max_dist, d2_s, face_s)
            d2[order] = d2_s
            face[order] = face_s
    torch.cuda.synchronize(dev)
    info.update(build_ms=1e3 * (t1 - t0), query_ms=1e3 * (time.perf_counter() - t1))
    if stats is not None:
        stats.update(info)
    return (d2 if squared else torch.sqrt(d2)), face


def distance_metrics(dist_a, face_a, dist_b, face_b, thresholds=()):
    """the reductions of mesh_distance over the two directed results (dist, face) of closest_on_mesh, in float64"""
    da, db = dist_a.double(), dist_b.double()
    if da.numel() == 0 or db.numel() == 0:
        raise ValueError("both sides need at least one sample")
    accuracy, completeness = float(da.mean()), float(db.mean())
    out = dict(accuracy=accuracy, completeness=completeness, chamfer=0.5 * (accuracy + completeness),
               hausdorff=max(float(da.max()), float(db.max())),
               clipped_a=float((face_a < 0).double().mean()), clipped_b=float((face_b < 0).double().mean()),
               thresholds=[float(t) for t in thresholds], precision=[], recall=[], fscore=[])
    for t in out["thresholds"]:
        p, r = float((da <= t).double().mean()), float((db <= t).double().mean())
        out["precision"].append(p)
        out["recall"].append(r)
        out["fscore"].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def mesh_distance(verts_a, faces_a, verts_b, faces_b, n_samples=1_000_000, thresholds=(), max_dist=None, seed=0,
                  stats=None):
    """How far mesh A (the reconstruction) is from mesh B (the reference) -> a dict of Python floats.

    n_samples points are drawn on each surface (sample_surface, seed for A, seed + 1 for B) and sent to the other mesh
    (closest_on_mesh): accuracy = the mean distance from A's samples to B, completeness = from B's samples to A,
    chamfer = their mean, hausdorff = the larger of the two maxima, clipped_a / clipped_b = the share of samples beyond
    max_dist (they count as max_dist; None: the diagonal of the box around both meshes, nothing is clipped).
    thresholds / precision / recall / fscore are lists, one entry per threshold t: the share of A's samples within t
    of B, of B's within t of A, and 2PR / (P + R) (0 when both are 0).  All reductions in float64.  A dict passed as
    `stats` receives sample_ms and closest_on_mesh's stats of each direction under a_to_b and b_to_a."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"n_samples must be >= 1, got {n_samples}")
    if max_dist is None:
        both = torch.cat([verts_a, verts_b])
        lo, hi = torch.aminmax(both, dim=0)
        max_dist = float((hi.double() - lo.double()).norm()) * (1 + 2.0 ** -20)
    t0 = time.perf_counter()
    pts_a, _ = sample_surface(verts_a, faces_a, n_samples, seed=seed)
    pts_b, _ = sample_surface(verts_b, faces_b, n_samples, seed=seed + 1)
    if pts_a.is_cuda:
        torch.cuda.synchronize(pts_a.device)
    sample_ms = 1e3 * (time.perf_counter() - t0)
    ab, ba = {}, {}
    dist_a, face_a = closest_on_mesh(pts_a, verts_b, faces_b, max_dist=max_dist, stats=ab)
    dist_b, face_b = closest_on_mesh(pts_b, verts_a, faces_a, max_dist=max_dist, stats=ba)
    if stats is not None:
        stats.update(sample_ms=sample_ms, a_to_b=ab, b_to_a=ba)
    return distance_metrics(dist_a, face_a, dist_b, face_b, thresholds)


# ------------------------------------------------------------------------------------------------- vertex colours
FALLBACK_DIR = (0.0, 0.0, -1.0)   # view direction of the colour network where no ray sees the surface (from above)
MIN_OPACITY = 1e-3


def vertex_rays(verts, normals, offset):
    """the ray of each vertex: from v + offset*n toward -n over t in [0, 2*offset] -> rays_o, rays_d, hits_t (V,2)"""
    offset = float(offset)
    rays_o = (verts + offset * normals).contiguous()
    rays_d = (-normals).contiguous()
    hits_t = torch.tensor([0.0, 2 * offset], dtype=_f32, device=verts.device).expand(verts.shape[0], 2).contiguous()
    return rays_o, rays_d, hits_t


@torch.no_grad()
def vertex_colors(model, verts, normals, offset, chunk=1 << 20, quantize=True, **render_kwargs):
    """Per-vertex colour of the trained appearance field -> (V,3) uint8 (quantize=False: the float colour in [0,1]).

    Each vertex with a non-zero normal casts the ray of vertex_rays through rendering.volume_render (the HIP marcher,
    field and compositor; hits_t is set directly, with no near clamp), `chunk` rays at a time; its colour is
    rgb / opacity clamped to [0,1] where opacity >= MIN_OPACITY.  Where the ray sees nothing, or the normal vanished,
    the colour is the colour network at the vertex itself viewed along FALLBACK_DIR.  Quantised as floor(255*c + 0.5).
    render_kwargs (exp_step_factor, embedding_a, ...) pass through to volume_render and the field."""
    from .rendering import volume_render
    n = verts.shape[0]
    dev = verts.device
    col = torch.zeros(n, 3, dtype=_f32, device=dev)
    seen = torch.zeros(n, dtype=torch.bool, device=dev)
    rows = torch.nonzero(normals.abs().amax(1) > 0).squeeze(1) if n else torch.zeros(0, dtype=torch.int64, device=dev)
    classes = render_kwargs.get('num_classes', 7)
    for s in range(0, rows.numel(), chunk):
        idx = rows[s:s + chunk]
        m = idx.numel()
        rays_o, rays_d, hits_t = vertex_rays(verts[idx], normals[idx], offset)
        opacity = torch.zeros(m, device=dev)
        rgb = torch.zeros(m, 3, device=dev)
        volume_render(model, rays_o, rays_d, hits_t, opacity, torch.zeros(m, device=dev), rgb,
                      torch.zeros(m, 3, device=dev), torch.zeros(m, 3, device=dev),
                      torch.zeros(m, classes, device=dev), **render_kwargs)
        ok = opacity >= MIN_OPACITY
        col[idx] = torch.where(ok[:, None], (rgb / opacity.clamp_min(MIN_OPACITY)[:, None]).clamp(0, 1), col[idx])
        seen[idx] = ok
    rest = torch.nonzero(~seen).squeeze(1)
    for s in range(0, rest.numel(), chunk):
        idx = rest[s:s + chunk]
        d = torch.tensor(FALLBACK_DIR, dtype=_f32, device=dev).expand(idx.numel(), 3).contiguous()
        col[idx] = model.forward_test(verts[idx].contiguous(), d, **render_kwargs)[1].float().clamp(0, 1)
    if not quantize:
        return col
    return torch.floor(255 * col + 0.5).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- PLY
_RGB = ("red", "green", "blue")


def _ply_header(n_v, n_f, normals, colors=False):
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else [])
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_v}"]
    lines += [f"property float {p}" for p in props]
    lines += [f"property uchar {p}" for p in _RGB] if colors else []
    lines += [f"element face {n_f}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


_FACE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])   # 13 bytes per face, unaligned as in the file


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def write_ply(path, verts, faces, normals=None, colors=None):
    """binary little-endian PLY with the element / property names the reference writes through plyfile:
    vertex (float x y z [nx ny nz] [uchar red green blue]), face (list uchar int vertex_indices)"""
    v = _np(verts)
    f = _np(faces)
    v = v.astype("<f4").reshape(-1, 3)
    if normals is not None:
        v = np.concatenate([v, _np(normals).astype("<f4").reshape(-1, 3)], 1)
    if colors is not None:
        rec_v = np.empty(v.shape[0], [("f", "<f4", (v.shape[1],)), ("rgb", "u1", (3,))])   # packed, as in the file
        rec_v["f"] = v
        rec_v["rgb"] = _np(colors).reshape(-1, 3)
        v = rec_v
    rec = np.empty(f.shape[0], _FACE)
    rec["n"] = 3
    rec["idx"] = f.reshape(-1, 3)
    with open(path, "wb") as fh:
        fh.write(_ply_header(v.shape[0], rec.shape[0], normals is not None, colors is not None))
        fh.write(np.ascontiguousarray(v).tobytes())
        fh.write(rec.tobytes())


def read_ply(path, colors=False):
    """-> (verts (V,3) f32, faces (F,3) int32, normals (V,3) f32 or None) of a file write_ply wrote;
    colors=True appends the (V,3) uint8 red / green / blue rows, or None"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    if header[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts, props, elem = {}, [], None
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            elem = w[1]
            counts[elem] = int(w[2])
        elif w[0] == "property" and elem == "vertex":
            if w[1] != "float" and not (w[1] == "uchar" and w[2] in _RGB):
                raise ValueError(f"{path}: vertex property {line!r} is not supported")
            props.append((w[2], "<f4" if w[1] == "float" else "u1"))
        elif w[0] == "property" and line != "property list uchar int vertex_indices":
            raise ValueError(f"{path}: face property {line!r} is not supported")
    n_v, n_f = counts["vertex"], counts["face"]
    vt = np.dtype(props)
    rv = np.frombuffer(data, vt, n_v, end)
    rec = np.frombuffer(data, _FACE, n_f, end + vt.itemsize * n_v)
    if n_f and (rec["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are supported")
    names = [p for p, _ in props]

    def cols(keys, dtype):
        return np.stack([rv[k] for k in keys], 1).astype(dtype) if set(keys) <= set(names) else None
    out = (cols(("x", "y", "z"), np.float32).reshape(n_v, 3), rec["idx"].astype(np.int32),
           cols(("nx", "ny", "nz"), np.float32))
    return out + (cols(_RGB, np.uint8),) if colors else out
